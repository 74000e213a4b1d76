"""CPU: the per-face albedo fit (csrc/fr_albedo_lse.hip, fr_sfs_lighting).  The entry points exist, answer their sizes and their
geometry, and validate in the header's order before any HIP call -- every single bad argument and every pair, the earlier item
winning; the Python surface keeps its defaults and raises its three ValueErrors; and the float64 model of the GPU tests
(tests/ref_albedo_lse.py) is held to an independent numpy.linalg.lstsq on the standard inputs."""
import ctypes
import inspect
import itertools
import os
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
import ref_albedo_lse as RA

NEW = ("fr_albedo_basis_bytes", "fr_albedo_basis_build", "fr_sfs_lighting", "fr_albedo_lse_workspace_bytes",
       "fr_albedo_lse_forward", "fr_debug_albedo_lse_geom")


def _L():
    return pkg("_lib").lib()


def _geom(B, H, W, K):
    out = (ctypes.c_int * 5)()
    _L().fr_debug_albedo_lse_geom(B, H, W, K, out)
    return list(out)


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert "fr_albedo_lse.hip" in pkg("_lib").SOURCES


def test_sizes_and_geometry():
    L = _L()
    T = _geom(1, 1, 1, 10)[0]
    assert T > 0 and T % 64 == 0
    for B, H, W in [(3, 32, 32), (1, 13, 11), (1, 1, 1), (1, 1, T), (1, 1, T + 1), (2, 3, T), (5, 1, 4 * T + 1), (64, 200, 200),
                    (7, 448, 448)]:
        for K in (1, 10, 15):
            g = _geom(B, H, W, K)
            tiles = -(-H * W // T)
            assert g[0] == T and g[1] == tiles and g[2] == B * -(-tiles // 4) and g[3] == B, (B, H, W, K, g)
            assert 0 < g[4] <= 64 * 1024
            assert L.fr_albedo_lse_workspace_bytes(B, H, W, K) == B * tiles * 257 * 8
    for bad in [(0, 5, 5, 10), (5, 0, 5, 10), (5, 5, 0, 10), (-1, 5, 5, 10), (5, -1, 5, 10), (5, 5, -1, 10), (5, 5, 5, 0),
                (5, 5, 5, 16), (5, 5, 5, -3), (1, 1 << 16, 1 << 15, 10), (1 << 12, 1 << 15, 1 << 15, 10)]:
        assert _geom(*bad) == [0] * 5 and L.fr_albedo_lse_workspace_bytes(*bad) == 0, bad
    assert L.fr_albedo_basis_bytes(7, 10) == 7 * 10 * 8 and L.fr_albedo_basis_bytes(105694, 10) == 105694 * 80
    for bad in [(0, 10), (-1, 10), (7, 0), (7, 16)]:
        assert L.fr_albedo_basis_bytes(*bad) == 0, bad


# ---- the checks: every single bad argument, and every pair ----------------------------------------------------------------------------
# A defect = (the header's item it trips, the arguments it replaces); a call answers the code of the LOWEST item among its defects.
#   fit:       1 negative size / bad ridge -> -1, 2 K unserved -> -4, 3 empty -> 0, 4 NULL -> -1, 5 workspace -> -2, 6 too large -> -4
#   basis:     1 negative size -> -1, 2 K unserved -> -4, 3 ntri == 0 -> 0, 4 NULL -> -1, 5 buffer -> -2, 6 ntri > 2^24 -> -4
#   lighting:  1 negative size / bad rcond / nparts -> -1, 3 empty image -> 0, 4 NULL parts -> -1, 5 state -> -2, 6 too large -> -4
CODE = {1: -1, 2: -4, 3: 0, 4: -1, 5: -2, 6: -4}
GOOD, ODD = 0x1000, 0x1008          # made-up addresses: 16-byte aligned, and not
POINTERS = ("basis", "tri_ind", "lighting", "normal_new", "abedo", "im_gray", "alpha", "moments", "stats", "workspace", "tri",
            "pc_tex", "parts", "state")


def _entry_points():
    L = _L()
    nul = ctypes.c_void_p(0)
    nws = L.fr_albedo_lse_workspace_bytes(3, 17, 33, 10)
    nst = L.fr_sfs_state_bytes(17, 33)
    nba = L.fr_albedo_basis_bytes(40, 10)
    assert nws > 0 and nst > 0 and nba > 0

    def fit(a):
        return L.fr_albedo_lse_forward(a["basis"], a["tri_ind"], a["lighting"], a["normal_new"], a["abedo"], a["im_gray"], a["B"],
                                       a["ntri"], a["H"], a["W"], a["K"], a["ridge"], a["alpha"], a["moments"], a["stats"],
                                       a["workspace"], a["ws_bytes"], nul)

    def basis(a):
        return L.fr_albedo_basis_build(a["tri"], a["pc_tex"], a["nver"], a["ntri"], a["K"], a["basis"], a["basis_bytes"], nul)

    def lighting(a):
        return L.fr_sfs_lighting(a["parts"], a["nparts"], a["H"], a["W"], a["rcond"], a["state"], a["state_bytes"], nul)
    big = dict(H=1 << 16, W=1 << 15)
    return {
        "fit": (fit, dict(B=3, H=17, W=33, ntri=40, K=10, ridge=1e-6, ws_bytes=nws,
                          **{k: GOOD for k in POINTERS[:10]}),
                [(1, dict(B=-1)), (1, dict(H=-1)), (1, dict(W=-5)), (1, dict(ntri=-1)), (1, dict(ridge=-1.0)),
                 (1, dict(ridge=float("nan"))), (1, dict(ridge=float("inf"))), (2, dict(K=0)), (2, dict(K=16)), (2, dict(K=-2)),
                 (3, dict(B=0)), (3, dict(H=0)), (3, dict(W=0))] +
                [(4, {k: 0}) for k in POINTERS[:9]] +
                [(5, dict(workspace=0)), (5, dict(workspace=ODD)), (5, dict(ws_bytes=nws - 1)), (5, dict(ws_bytes=0)), (6, big)]),
        "basis": (basis, dict(tri=GOOD, pc_tex=GOOD, nver=30, ntri=40, K=10, basis=GOOD, basis_bytes=nba),
                  [(1, dict(nver=-1)), (1, dict(ntri=-1)), (2, dict(K=0)), (2, dict(K=16)), (3, dict(ntri=0)), (4, dict(tri=0)),
                   (4, dict(pc_tex=0)), (5, dict(basis=0)), (5, dict(basis=ODD)), (5, dict(basis_bytes=nba - 1)),
                   (6, dict(ntri=(1 << 24) + 1, basis_bytes=1 << 40))]),
        "lighting": (lighting, dict(parts=GOOD, nparts=2, H=17, W=33, rcond=1e-15, state=GOOD, state_bytes=nst),
                     [(1, dict(H=-1)), (1, dict(W=-1)), (1, dict(rcond=-1.0)), (1, dict(rcond=float("nan"))), (1, dict(nparts=0)),
                      (1, dict(nparts=4097)), (3, dict(H=0)), (3, dict(W=0)), (4, dict(parts=0)), (5, dict(state=0)),
                      (5, dict(state=ODD)), (5, dict(state_bytes=nst - 1)), (6, dict(H=1 << 16, W=1 << 15, state_bytes=1 << 50))]),
    }


def _call(fn, base, *defects):
    a = dict(base)
    for _, d in defects:
        a.update(d)
    for k in POINTERS:
        if k in a:
            a[k] = ctypes.c_void_p(a[k])
    return fn(a)


def test_checks_hold_singly_and_in_pairs():
    """Every call here carries at least one defect, so each returns from the checks: none reaches HIP.  The test SKIPS where a GPU is
    visible, as tests/test_capi_codes_cpu.py and tests/test_fine_losses_cpu.py do: it checks host code, and if a regression let a
    case through the checks, the call would launch on the made-up addresses.
    (A shape the fit refuses has a workspace size of 0, so a short ws_bytes is no defect beside it.)"""
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    singles = pairs = 0
    for name, (fn, base, defects) in _entry_points().items():
        for d in defects:
            assert _call(fn, base, d) == CODE[d[0]], (name, d)
            singles += 1
        for d1, d2 in itertools.combinations(defects, 2):
            keys = set(d1[1]) | set(d2[1])
            if set(d1[1]) & set(d2[1]):
                continue                                       # two values for one argument: not a pair
            if {d1[0], d2[0]} == {5, 6} and keys & {"ws_bytes", "basis_bytes", "state_bytes"}:
                continue                                       # the byte count belongs to the shape: a pair of its own kind
            want = CODE[min(d1[0], d2[0])]
            assert _call(fn, base, d1, d2) == want, (name, d1, d2, want)
            pairs += 1
    print("held %d single defects and %d pairs over three entry points" % (singles, pairs))
    assert singles >= 50 and pairs >= 400
    fn, base, _ = _entry_points()["fit"]
    # an empty shape writes nothing and needs nothing
    assert _call(fn, base, (3, dict(B=0, workspace=0, ws_bytes=0, **{k: 0 for k in POINTERS[:9]}))) == 0
    # beyond one grid with a small workspace: the size is 0 there, so the answer is the grid's
    assert _call(fn, base, (6, dict(H=1 << 16, W=1 << 15)), (0, dict(ws_bytes=0))) == -4
    fn, base, _ = _entry_points()["basis"]
    assert _call(fn, base, (0, dict(nver=0, pc_tex=0)), (5, dict(basis=0))) == -2   # no vertices: pc_tex is not read


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_defaults_and_refusals():
    losses = pkg("nets.losses")
    sig = inspect.signature(losses.get_spherical_harmonics_model).parameters
    assert sig["alpha_lse"].default is False and sig["alpha_ridge"].default == 1e-6
    sig = inspect.signature(losses.get_loss).parameters
    assert sig["sfs_alpha_lse"].default is False and sig["sfs_alpha_ridge"].default == 1e-6
    ops = pkg("rendering_layer.ops")
    assert inspect.signature(ops.albedo_lse).parameters["ridge"].default == 1e-6
    assert inspect.signature(ops.sfs_lighting).parameters["rcond"].default == 1e-15
    assert callable(ops.albedo_basis) and callable(pkg("nets.network").FaceRecNet.albedo_basis)
    fn = types.SimpleNamespace(mu_tex=None, pc_tex=None, param_tex=None)
    for kw, word in ((dict(fused=False), "fused"), (dict(fused=True, tex_grad=True), "tex_grad"),
                     (dict(fused=True, gather=True), "gather"), (dict(fused=True, gather=True, fused_gather=True), "gather")):
        with pytest.raises(ValueError, match=word):
            losses.get_spherical_harmonics_model(fn, None, None, alpha_lse=True, **kw)
    # the flag off: the refusals above are not made (the call gets as far as the missing texture model)
    with pytest.raises(ValueError, match="texture model"):
        losses.get_spherical_harmonics_model(fn, None, None, tex_grad=True)
    with open(os.path.join(ROOT, "examples", "coarse_loop.py")) as f:
        ex = f.read()
    assert "--sfs-alpha-lse" in ex and "--sfs-alpha-ridge" in ex


# ---- the model against an independent least squares -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def std(oracle, small_assets):
    A = small_assets
    pc = RA.std_pc_tex(A)
    V = RA.std_vertices(A)
    _, tex, nrm, tind = oracle.render_depth(V, A["tri"], np.asarray(A["mu_tex"], np.float32)[None], RA.STD_S, RA.STD_S)
    a, n = RA.maps_from_render(tex, nrm)
    basis = RA.basis_ref(A["tri"], pc)
    l = RA.std_lighting(RA.STD_S, RA.STD_S)
    star = RA.std_alpha_star(RA.STD_B)
    I = RA.std_image(basis, tind, l, n, a, star)
    return dict(basis=basis, tri_ind=tind, lighting=l, normal=n, abedo=a, im_gray=I, star=star, pc=pc, tri=A["tri"])


def test_basis_model_is_the_lookup_average(std, small_assets):
    """Phi[t] = the mean over channels of (t[p1] + t[p2] + t[p3]) / 3 of the basis columns, to float64 rounding"""
    pc = std["pc"].astype(np.float64)
    N = pc.shape[0] // 3
    v = np.asarray(std["tri"]).astype(np.int64)
    want = sum(pc[c * N + v[j]] for c in range(3) for j in range(3)) / 9.0
    assert np.abs(std["basis"] - want).max() <= 16 * 2.0 ** -53 * np.abs(pc).max()
    bad = np.asarray(std["tri"], np.float32).copy()
    bad[1, 3] = N
    bad[2, 5] = np.nan
    got = RA.basis_ref(bad, std["pc"])
    assert not got[3].any() and not got[5].any() and np.array_equal(got[4], std["basis"][4])


def test_model_against_lstsq_on_the_standard_inputs(std):
    """preconditions on the INPUTS (not on the kernel): cond(G) < 10, recovery <= 1e-5 at ridge 0 -- and the model's alpha is the
    minimiser an independent numpy.linalg.lstsq finds on the same design"""
    K = RA.STD_K
    alpha, stats, M, S = RA.fit_ref(std["basis"], std["tri_ind"], std["lighting"], std["normal"], std["abedo"], std["im_gray"], 0.0)
    x, counted = RA.pixel_x(std["basis"], std["tri_ind"], std["lighting"], std["normal"], std["abedo"], std["im_gray"])
    for b in range(RA.STD_B):
        cond = np.linalg.cond(M[b, :K, :K])
        rec = np.linalg.norm(alpha[b] - std["star"][b]) / np.linalg.norm(std["star"][b])
        sol = np.linalg.lstsq(x[b][counted[b]][:, :K], x[b][counted[b]][:, K], rcond=None)[0]
        dif = np.linalg.norm(alpha[b] - sol) / np.linalg.norm(sol)
        print("face %d: %d pixels, cond(G) %.2f, recovery %.2e, against lstsq %.2e, E0 %.3e, E1 %.3e"
              % (b, stats[b, 0], cond, rec, dif, stats[b, 1], stats[b, 2]))
        assert 300 < stats[b, 0] < 450 and stats[b, 3] == 1.0
        assert cond < 10
        assert rec <= 1e-5
        assert dif <= 4 * 2.0 ** -24                      # one fp32 rounding of alpha; the float64 solves agree far below it
        assert stats[b, 2] <= stats[b, 1] and abs(stats[b, 2]) <= 1e-10 * stats[b, 1]
    # the ridge moves the minimiser by about ridge x cond: still a recovery, and a larger E1
    alpha_r, stats_r, _, _ = RA.fit_ref(std["basis"], std["tri_ind"], std["lighting"], std["normal"], std["abedo"], std["im_gray"],
                                        1e-6)
    for b in range(RA.STD_B):
        rec = np.linalg.norm(alpha_r[b] - std["star"][b]) / np.linalg.norm(std["star"][b])
        assert rec <= 1e-5 and stats_r[b, 3] == 1.0 and stats_r[b, 2] <= stats_r[b, 1]


def test_model_failure_rules(std):
    """no counted pixel, a vanishing pivot (three pixels, ten unknowns, no ridge) and a non-finite moment fail a face; the ridge
    rescues the three-pixel face"""
    K = RA.STD_K
    tind = std["tri_ind"].copy()
    flat = tind.reshape(RA.STD_B, -1)
    cov = np.flatnonzero(flat[1] >= 0)
    flat[1, cov[3:]] = -1.0                                  # face 1 keeps three covered pixels
    flat[2, :] = -1.0                                        # face 2 none
    args = (std["basis"], tind, std["lighting"], std["normal"], std["abedo"], std["im_gray"])
    alpha, stats, _, _ = RA.fit_ref(*args, 0.0)
    assert stats[:, 0].tolist() == [float((std["tri_ind"][0] >= 0).sum()), 3.0, 0.0]
    assert stats[:, 3].tolist() == [1.0, 0.0, 0.0] and not alpha[1:].any()
    alpha, stats, _, _ = RA.fit_ref(*args, 1e-6)
    assert stats[:, 3].tolist() == [1.0, 1.0, 0.0] and alpha[1].any() and stats[1, 2] <= stats[1, 1]
    I = std["im_gray"].copy()
    I.reshape(RA.STD_B, -1)[0, np.flatnonzero(std["tri_ind"].reshape(RA.STD_B, -1)[0] >= 0)[7]] = np.nan
    alpha, stats, _, _ = RA.fit_ref(std["basis"], std["tri_ind"], std["lighting"], std["normal"], std["abedo"], I, 1e-6)
    assert stats[:, 3].tolist() == [0.0, 1.0, 1.0] and not alpha[0].any()
