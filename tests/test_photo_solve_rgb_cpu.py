"""CPU: the colour photometric solve (csrc/fr_photo_solve.hip).  The entry points exist, answer their sizes and their geometry, and
validate in the header's order before any HIP call -- every single bad argument and every pair, the earlier item winning, with
pre-filled outputs untouched; the Python surface is there; and the float64 model of the GPU tests (tests/ref_photo_solve_rgb.py)
has the properties the alternation rests on, on the standard inputs."""
import ctypes
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
import ref_albedo_lse as RA
import ref_photo_solve_rgb as RS

NEW = {"fr_albedo_basis_rgb_bytes": "z:ii", "fr_albedo_basis_rgb_build": "i:pppiiipzp", "fr_albedo_image_rgb": "i:pppiiiiipp",
       "fr_photo_solve_rgb_workspace_bytes": "z:iii", "fr_photo_light_lse_rgb_forward": "i:ppppppiiiffdppppzp",
       "fr_albedo_lse_rgb_forward": "i:ppppppiiiiiffdppppzp", "fr_debug_photo_solve_rgb_geom": "v:iiiI"}


def _L():
    return pkg("_lib").lib()


def _geom(B, H, W):
    out = (ctypes.c_int * 6)()
    _L().fr_debug_photo_solve_rgb_geom(B, H, W, out)
    return list(out)


def test_symbols_exported():
    host, L = pkg("_lib"), _L()
    for name, row in NEW.items():
        assert hasattr(L, name) and name in host.EXPORTS and host.SIGNATURES[name] == row, name
    assert "fr_photo_solve.hip" in host.SOURCES


def test_sizes_and_geometry():
    L = _L()
    T = _geom(1, 1, 1)[0]
    assert T == 256
    for B, H, W in [(3, 32, 32), (1, 13, 11), (1, 1, 1), (1, 25, 41), (3, 67, 65), (1, 1, T), (1, 1, T + 1), (5, 1, 4 * T + 1),
                    (64, 200, 200), (65535, 4, 4)]:
        g = _geom(B, H, W)
        tiles = -(-H * W // T)
        assert g[:5] == [T, tiles, B * -(-tiles // 4), 3 * B, B], (B, H, W, g)
        assert 0 < g[5] <= 64 * 1024
        assert L.fr_photo_solve_rgb_workspace_bytes(B, H, W) == B * tiles * 3 * 257 * 8
    assert _geom(1, 25, 41)[1:3] == [5, 2] and _geom(1, 67, 65)[1] == 18
    for bad in [(0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (65536, 4, 4), (1, 1 << 16, 1 << 15),
                (1 << 12, 1 << 15, 1 << 15)]:
        assert _geom(*bad) == [0] * 6 and L.fr_photo_solve_rgb_workspace_bytes(*bad) == 0, bad
    assert _geom(1, 1, 0x7FFFFFFF)[1] == 1 << 23                          # 2^31 - 1 pixels are served
    assert L.fr_albedo_basis_rgb_bytes(7, 10) == 7 * 3 * 11 * 8 and L.fr_albedo_basis_rgb_bytes(105694, 10) == 105694 * 264
    for bad in [(0, 10), (-1, 10), (7, 0), (7, 16)]:
        assert L.fr_albedo_basis_rgb_bytes(*bad) == 0, bad


# ---- the checks: every single bad argument, and every pair ----------------------------------------------------------------------------
# A defect = (the header's item it trips, the arguments it replaces); a call answers the code of the LOWEST item among its defects:
#   1 negative size / bad ridge, gain, offset -> -1, 2 empty -> 0, 3 NULL -> -1, 4 workspace / basis buffer -> -2, 5 limits -> -4
CODE = {1: -1, 2: 0, 3: -1, 4: -2, 5: -4}
OUTPUTS = ("light", "alpha", "moments", "stats", "workspace", "tex_img", "basis_out")
INPUTS = ("tex", "normal", "tri_ind", "target", "weight", "gate", "basis", "lightin", "alphain", "tri", "mu_tex", "pc_tex")
FILL = 0x5A


class _Buffers:
    """host buffers for every pointer argument: inputs zeroed, outputs pre-filled -- no check may touch either"""

    def __init__(self, nbytes):
        self.store = {k: np.full(nbytes + 32, FILL if k in OUTPUTS else 0, np.uint8) for k in OUTPUTS + INPUTS}

    def addr(self, k, odd=False):
        a = self.store[k].ctypes.data
        a += (-a) % 16
        return a + (8 if odd else 0)

    def untouched(self):
        return all((self.store[k] == FILL).all() for k in OUTPUTS)


def _entry_points(buf):
    L = _L()
    nul = ctypes.c_void_p(0)
    nws = L.fr_photo_solve_rgb_workspace_bytes(3, 17, 33)
    nba = L.fr_albedo_basis_rgb_bytes(40, 10)
    assert 0 < nba <= nws

    def P(a, k):
        v = a[k]
        return ctypes.c_void_p(v if isinstance(v, int) else buf.addr(k, v == "odd"))

    def light(a):
        return L.fr_photo_light_lse_rgb_forward(P(a, "tex"), P(a, "normal"), P(a, "tri_ind"), P(a, "target"), P(a, "weight"),
                                                P(a, "gate"), a["B"], a["H"], a["W"], a["gain"], a["offset"], a["ridge"],
                                                P(a, "light"), P(a, "moments"), P(a, "stats"), P(a, "workspace"), a["ws_bytes"], nul)

    def albedo(a):
        return L.fr_albedo_lse_rgb_forward(P(a, "basis"), P(a, "tri_ind"), P(a, "normal"), P(a, "lightin"), P(a, "target"),
                                           P(a, "weight"), a["B"], a["ntri"], a["H"], a["W"], a["K"], a["gain"], a["offset"],
                                           a["ridge"], P(a, "alpha"), P(a, "moments"), P(a, "stats"), P(a, "workspace"),
                                           a["ws_bytes"], nul)

    def image(a):
        return L.fr_albedo_image_rgb(P(a, "basis"), P(a, "tri_ind"), P(a, "alphain"), a["B"], a["ntri"], a["H"], a["W"], a["K"],
                                     P(a, "tex_img"), nul)

    def basis(a):
        return L.fr_albedo_basis_rgb_build(P(a, "tri"), P(a, "mu_tex"), P(a, "pc_tex"), a["nver"], a["ntri"], a["K"],
                                           P(a, "basis_out"), a["basis_bytes"], nul)
    shape = dict(B=3, H=17, W=33)
    scal = dict(gain=1.0, offset=0.0, ridge=1e-9)
    big = [(5, dict(H=1 << 16, W=1 << 15)), (5, dict(B=65536))]
    neg = [(1, dict(B=-1)), (1, dict(H=-1)), (1, dict(W=-5))]
    empty = [(2, dict(B=0)), (2, dict(H=0)), (2, dict(W=0))]
    bad_scal = [(1, dict(ridge=-1.0)), (1, dict(ridge=float("nan"))), (1, dict(ridge=float("inf"))), (1, dict(gain=float("nan"))),
                (1, dict(offset=float("inf")))]
    bad_ws = [(4, dict(workspace=0)), (4, dict(workspace="odd")), (4, dict(ws_bytes=nws - 1)), (4, dict(ws_bytes=0))]
    bad_k = [(5, dict(K=0)), (5, dict(K=16)), (5, dict(K=-2))]
    ptr = lambda *names: {k: "ok" for k in names}   # noqa: E731
    return {
        "light": (light, dict(shape, **scal, ws_bytes=nws, **ptr("tex", "normal", "tri_ind", "target", "weight", "gate", "light",
                                                                  "moments", "stats", "workspace")),
                  neg + bad_scal + empty + [(3, {k: 0}) for k in ("tex", "normal", "tri_ind", "target", "light", "moments", "stats")]
                  + bad_ws + big),
        "albedo": (albedo, dict(shape, **scal, ntri=40, K=10, ws_bytes=nws,
                                **ptr("basis", "tri_ind", "normal", "lightin", "target", "weight", "alpha", "moments", "stats",
                                      "workspace")),
                   neg + [(1, dict(ntri=-1))] + bad_scal + empty
                   + [(3, {k: 0}) for k in ("basis", "tri_ind", "normal", "lightin", "target", "alpha", "moments", "stats")]
                   + bad_ws + bad_k + big),
        "image": (image, dict(shape, ntri=40, K=10, **ptr("basis", "tri_ind", "alphain", "tex_img")),
                  neg + [(1, dict(ntri=-1))] + empty + [(3, {k: 0}) for k in ("basis", "tri_ind", "alphain", "tex_img")] + bad_k + big),
        "basis": (basis, dict(nver=30, ntri=40, K=10, basis_bytes=nba, **ptr("tri", "mu_tex", "pc_tex", "basis_out")),
                  [(1, dict(nver=-1)), (1, dict(ntri=-1)), (2, dict(ntri=0)), (3, dict(tri=0)), (3, dict(mu_tex=0)), (3, dict(pc_tex=0)),
                   (4, dict(basis_out=0)), (4, dict(basis_out="odd")), (4, dict(basis_bytes=nba - 1)), (5, dict(K=0)), (5, dict(K=16)),
                   (5, dict(ntri=(1 << 24) + 1, basis_bytes=1 << 40))]),
    }, nws


def _call(fn, base, *defects):
    a = dict(base)
    for _, d in defects:
        a.update(d)
    return fn(a)


def test_checks_hold_singly_and_in_pairs_and_touch_nothing():
    """Every call here carries at least one defect, so each returns from the checks: none reaches HIP.  The test SKIPS where a GPU is
    visible, as tests/test_albedo_lse_cpu.py does: it checks host code, and if a regression let a case through the checks, the call
    would launch on host addresses.  (A refused shape or K has a size of 0, so a short byte count is no defect beside it.)"""
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    buf = _Buffers(1 << 16)
    eps, nws = _entry_points(buf)
    assert nws <= 1 << 16
    singles = pairs = 0
    for name, (fn, base, defects) in eps.items():
        for d in defects:
            assert _call(fn, base, d) == CODE[d[0]], (name, d)
            singles += 1
        for d1, d2 in itertools.combinations(defects, 2):
            if set(d1[1]) & set(d2[1]):
                continue                                       # two values for one argument: not a pair
            if {d1[0], d2[0]} == {4, 5} and (set(d1[1]) | set(d2[1])) & {"ws_bytes", "basis_bytes"}:
                continue                                       # the byte count belongs to the shape: a pair of its own kind
            want = CODE[min(d1[0], d2[0])]
            assert _call(fn, base, d1, d2) == want, (name, d1, d2, want)
            pairs += 1
    print("held %d single defects and %d pairs over four entry points" % (singles, pairs))
    assert singles >= 80 and pairs >= 700
    assert buf.untouched()
    # weight and gate_light may be NULL; an empty shape needs nothing; no triangles: the basis is not read
    fn, base, _ = eps["light"]
    assert _call(fn, base, (0, dict(weight=0, gate=0)), (4, dict(ws_bytes=0))) == -2
    assert _call(fn, base, (2, dict(B=0, workspace=0, ws_bytes=0, **{k: 0 for k in ("tex", "normal", "tri_ind", "target", "light",
                                                                                      "moments", "stats")}))) == 0
    fn, base, _ = eps["albedo"]
    assert _call(fn, base, (0, dict(ntri=0, basis=0)), (4, dict(workspace=0))) == -2
    fn, base, _ = eps["basis"]
    assert _call(fn, base, (0, dict(nver=0, mu_tex=0, pc_tex=0)), (4, dict(basis_out=0))) == -2
    assert buf.untouched()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface():
    ops, net = pkg("rendering_layer.ops"), pkg("nets.network").FaceRecNet
    for name in ("albedo_basis_rgb", "albedo_image_rgb", "photo_light_lse_rgb", "albedo_lse_rgb", "photo_solve_rgb"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(ops.photo_solve_rgb).parameters
    assert list(sig)[:4] == ["basis", "tri_ind", "normal", "target"]
    assert sig["iters"].default == 8 and sig["gate"].default is True and sig["gain"].default == 1.0 and sig["offset"].default == 0.0
    assert sig["alpha0"].default is None and sig["light0"].default is None and sig["weight"].default is None
    assert callable(net.albedo_basis_rgb) and callable(net.photo_solve_rgb)
    with open(os.path.join(ROOT, "examples", "photo_fit.py")) as f:
        assert "--closed-form" in f.read()


# ---- the model's own properties on the standard inputs --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def std(oracle, small_assets):
    A = small_assets
    pc = RS.std_pc_tex(A)
    mu_tex = np.asarray(A["mu_tex"], np.float32)
    V = RA.std_vertices(A, B=RS.STD_B, S=RS.STD_S)
    _, _, nrm, tind = oracle.render_depth(V, A["tri"], mu_tex[None], RS.STD_S, RS.STD_S)
    basis = RS.basis_ref(A["tri"], mu_tex, pc)
    star, light = RS.std_alpha_star(), RS.std_light()
    target, tex, st = RS.std_target(basis, tind, nrm, light, star)
    return dict(basis=basis, tri_ind=tind, normal=nrm, star=star, light=light, target=target, tex=tex, st=st, tri=A["tri"], pc=pc,
                mu_tex=mu_tex)


def test_standard_inputs_meet_their_preconditions(std):
    """every counted pixel is lit in every channel, every albedo exceeds 1e-3, every face has a few hundred pixels, every pixel hit is
    a triangle of the basis"""
    cov = std["st"]["covered"]
    assert (std["st"]["s"][cov] > 0).all() and std["tex"][cov].min() > 1e-3
    n = cov.reshape(RS.STD_B, -1).sum(1)
    assert (n > 300).all() and (n < 450).all()
    t = RA.f2i_x86(std["tri_ind"]).reshape(cov.shape)
    assert ((t >= 0) == cov).all() and t.max() < std["basis"].shape[0]


def test_basis_and_image_models(std):
    """the basis is the lookup average per channel, and the image is the render of the blended texture to float rounding"""
    pc, mu = std["pc"].astype(np.float64), std["mu_tex"].astype(np.float64).reshape(-1)
    N = pc.shape[0] // 3
    v = np.asarray(std["tri"]).astype(np.int64)
    for c in range(3):
        want = sum(np.concatenate([pc[c * N + v[j]], mu[c * N + v[j]][:, None]], 1) for j in range(3)) / 3.0
        assert np.abs(std["basis"][:, c] - want).max() <= 4 * 2.0 ** -53 * max(np.abs(pc).max(), np.abs(mu).max())
    bad = np.asarray(std["tri"], np.float32).copy()
    bad[1, 3], bad[2, 5] = N, np.nan
    got = RS.basis_ref(bad, std["mu_tex"], std["pc"])
    assert not got[3].any() and not got[5].any() and np.array_equal(got[4], std["basis"][4])
    tex = (mu[None] + std["star"].astype(np.float64) @ pc.T).reshape(RS.STD_B, 3, N)
    t = RA.f2i_x86(std["tri_ind"]).reshape(RS.STD_B, -1)
    cov = t >= 0
    for b in range(RS.STD_B):
        want = sum(tex[b][:, v[j][np.where(cov[b], t[b], 0)]] for j in range(3)).T / 3.0
        got = std["tex"][b].reshape(-1, 3).astype(np.float64)
        assert np.abs(got - want)[cov[b]].max() <= 2.0 ** -23 and not got[~cov[b]].any()


def test_each_half_step_recovers_the_truth(std):
    """The light step at the true texture recovers the true light, and the albedo step at the true light recovers alpha*.  Measured
    with the model here: relative errors of the light 3.3e-7, 4.6e-7, 3.3e-7 per face (Gram condition 3e3 .. 7.4e3) and of alpha
    2.5e-8, 2.4e-8, 3.1e-8 (condition 1.5 .. 1.7); asserted at ten times the largest, the margin being for another summation order."""
    light, st, M, _ = RS.light_fit_ref(std["tex"], std["normal"], std["tri_ind"], std["target"])
    alpha, sa, Ma, _ = RS.albedo_fit_ref(std["basis"], std["tri_ind"], std["normal"], std["light"], std["target"])
    for b in range(RS.STD_B):
        el = np.linalg.norm(light[b].astype(np.float64) - std["light"][b]) / np.linalg.norm(std["light"][b])
        ea = np.linalg.norm(alpha[b].astype(np.float64) - std["star"][b]) / np.linalg.norm(std["star"][b])
        print("face %d: light %.3g (cond %.3g), alpha %.3g (cond %.3g)"
              % (b, el, max(np.linalg.cond(M[b, c, :9, :9]) for c in range(3)), ea, np.linalg.cond(Ma[b, :RS.STD_K, :RS.STD_K])))
        assert el <= 4.6e-6 and ea <= 3.2e-7
        assert (st[b, :, 3] == 1.0).all() and sa[b, 3] == 1.0
        assert (st[b, :, 2] <= st[b, :, 1]).all() and sa[b, 2] <= sa[b, 1]
        assert st[b, :, 2].sum() <= 1e-10 * st[b, :, 1].sum() and sa[b, 2] <= 1e-10 * sa[b, 1]
    # an independent least squares on the same design agrees to one fp32 rounding of the coefficients
    x, w, counted = RS.albedo_x(std["basis"], std["tri_ind"], std["normal"], std["light"], std["target"])
    for b in range(RS.STD_B):
        X = x[b][counted[b]].reshape(-1, 16)
        sol = np.linalg.lstsq(X[:, :RS.STD_K], X[:, RS.STD_K], rcond=None)[0]
        assert np.linalg.norm(alpha[b] - sol) <= 4 * 2.0 ** -24 * np.linalg.norm(sol)


def test_alternation_descends_and_converges(std):
    """from alpha = 0 with no prior light: E is non-increasing over all 2 x 8 half-steps (up to 1e-12 E for rounding) and ends at most
    1e-6 of its value after the first light step (the model gives 7e-13 on these inputs)"""
    light, alpha, tex, E, ok = RS.solve_loop_ref(std["basis"], std["tri_ind"], std["normal"], std["target"], iters=8)
    assert ok.all()
    flat = E.reshape(-1, RS.STD_B)
    print("E per half-step and face:\n", flat)
    assert (flat[1:] <= flat[:-1] * (1 + 1e-12)).all()
    assert (flat[-1] <= 1e-6 * flat[0]).all()
    for b in range(RS.STD_B):
        assert np.linalg.norm(alpha[b] - std["star"][b]) <= 1e-3 * np.linalg.norm(std["star"][b])


def test_model_failure_rules(std):
    """no counted pixel, three pixels without a ridge and a non-finite target fail their unit alone; the ridge rescues the three-pixel
    face; a failed light unit receives the gate's row"""
    tind = np.asarray(std["tri_ind"], np.float32).copy()
    flat = tind.reshape(RS.STD_B, -1)
    cov = np.flatnonzero(flat[1] >= 0)
    flat[1, cov[3:]] = -1.0
    flat[2, :] = -1.0
    gate = std["light"]
    light, st, _, _ = RS.light_fit_ref(std["tex"], std["normal"], tind, std["target"], gate_light=gate)
    assert st[:, :, 0].tolist() == [[float((std["tri_ind"][0] >= 0).sum())] * 3, [3.0] * 3, [0.0] * 3]
    assert st[:, :, 3].tolist() == [[1.0] * 3, [0.0] * 3, [0.0] * 3] and np.array_equal(light[1:], gate[1:])
    light, st, _, _ = RS.light_fit_ref(std["tex"], std["normal"], tind, std["target"], ridge=1e-6)
    assert st[:, :, 3].tolist() == [[1.0] * 3, [1.0] * 3, [0.0] * 3] and not light[2].any()
    alpha, sa, _, _ = RS.albedo_fit_ref(std["basis"], tind, std["normal"], std["light"], std["target"])
    assert sa[:, 3].tolist() == [1.0, 0.0, 0.0] and not alpha[1:].any()       # nine samples, ten unknowns
    alpha, sa, _, _ = RS.albedo_fit_ref(std["basis"], tind, std["normal"], std["light"], std["target"], ridge=1e-6)
    assert sa[:, 3].tolist() == [1.0, 1.0, 0.0] and alpha[1].any()
    T = std["target"].copy()
    T.reshape(RS.STD_B, -1, 3)[0, np.flatnonzero(std["tri_ind"].reshape(RS.STD_B, -1)[0] >= 0)[7], 1] = np.nan
    light, st, _, _ = RS.light_fit_ref(std["tex"], std["normal"], std["tri_ind"], T)
    assert st[:, :, 3].tolist() == [[1.0, 0.0, 1.0], [1.0] * 3, [1.0] * 3]
    alpha, sa, _, _ = RS.albedo_fit_ref(std["basis"], std["tri_ind"], std["normal"], std["light"], T)
    assert sa[:, 3].tolist() == [0.0, 1.0, 1.0]
