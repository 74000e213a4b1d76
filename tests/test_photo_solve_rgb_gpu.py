"""GPU: the colour photometric solve (fr_albedo_basis_rgb_build, fr_albedo_image_rgb, fr_photo_light_lse_rgb_forward,
fr_albedo_lse_rgb_forward, rendering_layer.ops.photo_solve_rgb) against tests/ref_photo_solve_rgb.py.  The basis and the image bit
for bit, the image within the header's bound of the render; both moment sets within the summation-order bound of the fsum value (the
x themselves are bit-identical by construction), symmetric, reproducible and independent of the batch; both solves by their backward
error on the kernel's own moments; the failure rules; the loop against the raw calls chained by hand, its descent and its end."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from conftest import pkg
import ref_albedo_lse as RA
import ref_photo_solve_rgb as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _ops():
    return pkg("rendering_layer.ops")


def _L():
    return pkg("_lib").lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        u, v = a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32)
    else:
        u, v = _bits64(a), _bits64(b)
    return a.shape == b.shape and bool(((u == v) | (np.isnan(a) & np.isnan(b))).all())


def _geom(B, H, W):
    out = (ctypes.c_int * 6)()
    _L().fr_debug_photo_solve_rgb_geom(B, H, W, out)
    return list(out)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the raw calls: numpy in, numpy out --------------------------------------------------------------------------------------------------
def raw_light(inp, tex, weight=None, gate=None, ridge=0.0, gain=1.0, offset=0.0, fill=7.0, ws=None):
    L = _L()
    B, H, W = inp["normal"].shape[:3]
    light = torch.full((B, 3, 9), fill, dtype=torch.float32, device=DEV)
    M = torch.full((B, 3, 16, 16), fill, dtype=torch.float64, device=DEV)
    st = torch.full((B, 3, 4), fill, dtype=torch.float64, device=DEV)
    nws = L.fr_photo_solve_rgb_workspace_bytes(B, H, W)
    if ws is None:
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
    else:
        assert ws.dtype == torch.uint8 and ws.numel() == nws, (ws.numel(), nws)     # (exactly the stated bytes)
    d = [_dev(x) for x in (tex, inp["normal"], inp["tri_ind"], inp["target"], weight, gate)]
    rc = L.fr_photo_light_lse_rgb_forward(*[_p(x) for x in d], B, H, W, gain, offset, ridge, _p(light), _p(M), _p(st), _p(ws), nws,
                                          _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return light.cpu().numpy(), st.cpu().numpy(), M.cpu().numpy()


def raw_albedo(inp, light, weight=None, ridge=0.0, gain=1.0, offset=0.0, fill=7.0, ws=None, basis=None):
    L = _L()
    B, H, W = inp["normal"].shape[:3]
    T, K = inp["basis"].shape[0], inp["basis"].shape[2] - 1
    alpha = torch.full((B, K), fill, dtype=torch.float32, device=DEV)
    M = torch.full((B, 16, 16), fill, dtype=torch.float64, device=DEV)
    st = torch.full((B, 4), fill, dtype=torch.float64, device=DEV)
    nws = L.fr_photo_solve_rgb_workspace_bytes(B, H, W)
    if ws is None:
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
    else:
        assert ws.dtype == torch.uint8 and ws.numel() == nws, (ws.numel(), nws)     # (exactly the stated bytes)
    basis = _dev(inp["basis"], torch.float64) if basis is None else basis      # (basis: a device image to read instead)
    d = [_dev(x) for x in (inp["tri_ind"], inp["normal"], light, inp["target"], weight)]
    rc = L.fr_albedo_lse_rgb_forward(_p(basis), *[_p(x) for x in d], B, T, H, W, K, gain, offset, ridge, _p(alpha), _p(M), _p(st),
                                     _p(ws), nws, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return alpha.cpu().numpy(), st.cpu().numpy(), M.cpu().numpy()


def raw_image(inp, alpha):
    B, H, W = inp["normal"].shape[:3]
    T, K = inp["basis"].shape[0], inp["basis"].shape[2] - 1
    out = torch.full((B, H, W, 3), 7.0, dtype=torch.float32, device=DEV)
    basis, ti, al = _dev(inp["basis"], torch.float64), _dev(inp["tri_ind"]), _dev(alpha)
    assert _L().fr_albedo_image_rgb(_p(basis), _p(ti), _p(al), B, T, H, W, K, _p(out), _stream()) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _faces(inp, sel):
    return dict(inp, **{k: np.ascontiguousarray(inp[k][sel]) for k in ("tri_ind", "normal", "target", "tex", "light", "weight")})


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(small_assets):
    A = dict(small_assets, pc_tex=RS.std_pc_tex(small_assets))
    return pkg("nets.network").FaceRecNet(mesh_data=A, batch_size=RS.STD_B, im_size=RS.STD_S, device=DEV)


def _rendered(net, B, shift=None):
    """the standard inputs for B faces through the project's own render and basis build"""
    V = _dev(RA.std_vertices({"mu": net.mu.cpu().numpy()}, B=B, S=RS.STD_S, shift=shift))
    image = torch.zeros((B, RS.STD_S, RS.STD_S, 3), device=DEV)
    with torch.no_grad():
        _, _, nrm, tind = _ops().render_depth(V, net.tri, net.mu_tex[None], image)
    basis = net.albedo_basis_rgb()
    torch.cuda.synchronize()
    basis, nrm, tind = basis.cpu().numpy(), nrm.cpu().numpy(), tind.cpu().numpy()
    star, light = RS.std_alpha_star(B), RS.std_light(B)
    target, tex, st = RS.std_target(basis, tind, nrm, light, star)
    weight = np.random.RandomState(8).uniform(0.25, 2.0, tind.shape[:3]).astype(F)
    weight[np.random.RandomState(9).uniform(size=weight.shape) < 0.2] = 0.0
    return dict(basis=basis, tri_ind=tind, normal=nrm, target=target, tex=tex, light=light, star=star, weight=weight, st=st, V=V)


@pytest.fixture(scope="module")
def std(net):
    inp = _rendered(net, RS.STD_B)
    cov = inp["st"]["covered"]
    assert (inp["st"]["s"][cov] > 0).all() and inp["tex"][cov].min() > 1e-3          # the preconditions of the CPU file
    return inp


def _synthetic(B, H, W, K, seed, ntri=37):
    """shapes with no render behind them: random winners (a third background), normals in a cap, a positive random texture model,
    the picture of a random alpha under a light of the sampler's ranges plus noise (so that the residuals are not zero)"""
    rs = np.random.RandomState(seed)
    tind = np.where(rs.rand(B, H, W, 1) < 0.3, -1.0, rs.randint(0, ntri, (B, H, W, 1))).astype(F)
    if H * W == 1:
        tind[:] = 5.0
    n = rs.standard_normal((B, H, W, 3))
    n[..., 2] = np.abs(n[..., 2]) + 0.7
    n = (n * rs.uniform(0.5, 2.0, (B, H, W, 1))).astype(F)
    basis = np.concatenate([0.05 * rs.standard_normal((ntri, 3, K)), rs.uniform(0.3, 0.8, (ntri, 3, 1))], 2)
    star, light = (0.5 * rs.standard_normal((B, K))).astype(F), RS.std_light(B, seed)
    target, tex, st = RS.std_target(basis, tind, n, light, star)
    target = (target + 0.05 * rs.standard_normal(target.shape) * (tind >= 0)).astype(F)
    weight = rs.uniform(0.25, 2.0, (B, H, W)).astype(F)
    weight[rs.uniform(size=weight.shape) < 0.2] = 0.0
    return dict(basis=basis, tri_ind=tind, normal=n, target=target, tex=tex, light=light, star=star, weight=weight, st=st)


SHAPES = {"13x11": (1, 13, 11, 10), "1x1": (1, 1, 1, 1), "25x41": (3, 25, 41, 15), "67x65": (1, 67, 65, 10), "8x40": (3, 8, 40, 1)}


@pytest.fixture(scope="module")
def cases(std):
    assert _geom(1, 13, 11)[1] == 1 and _geom(1, 25, 41)[1:3] == [5, 2] and _geom(1, 67, 65)[1] == 18   # the tile's edges
    out = {name: _synthetic(*shape, seed=k + 1) for k, (name, shape) in enumerate(SHAPES.items())}
    out["standard"] = std
    return out


def _gate_for(inp):
    """a lighting under which every channel has both lit and unlit counted pixels: a side light per channel"""
    B = inp["normal"].shape[0]
    gate = np.zeros((B, 3, 9), F)
    gate[:, 0, 1], gate[:, 1, 2], gate[:, 2, 1] = 1.0, 1.0, -1.0
    gate[:, :, 0] = 0.05
    return gate


# ---- basis and image -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kb", [1, 10, 15])
def test_basis_build_is_bit_exact(small_assets, Kb):
    rs = np.random.RandomState(Kb)
    N = np.asarray(small_assets["mu"]).size // 3
    pc = (0.05 * rs.standard_normal((3 * N, Kb))).astype(F)
    mu = rs.uniform(0.2, 0.8, (3, N)).astype(F)
    tri = np.asarray(small_assets["tri"], F).copy()
    tri[0, 2], tri[1, 5], tri[2, 9], tri[1, 11] = N, -1.0, np.nan, 3e9      # out-of-range ids -> rows of +0.0
    got = _ops().albedo_basis_rgb(_dev(tri), _dev(mu), _dev(pc))
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (tri.shape[1], 3, Kb + 1) and not got.requires_grad
    got = got.cpu().numpy()
    assert _same_bits(got, RS.basis_ref(tri, mu, pc))
    for t in (2, 5, 9, 11):
        assert not _bits64(got[t]).any()                                    # +0.0, not -0.0
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("name", ["standard", "13x11", "1x1", "25x41", "67x65", "8x40"])
def test_image_is_bit_exact(cases, name):
    inp = cases[name]
    got = raw_image(inp, inp["star"])
    assert _same_bits(got, RS.image_ref(inp["basis"], inp["tri_ind"], inp["star"]))
    assert not got[inp["tri_ind"][..., 0] < 0].view(np.uint32).any()          # +0 at the background: every element written
    op = _ops().albedo_image_rgb(_dev(inp["basis"], torch.float64), _dev(inp["tri_ind"]), _dev(inp["star"]))
    assert not op.requires_grad and _same_bits(op.cpu().numpy(), got)


def test_image_against_the_render_within_the_stated_bound(net, std):
    """the plane of fr_albedo_image_rgb against render_depth's tex_img of the texture synth_texture blends from the same alpha"""
    ops = _ops()
    alpha = _dev(std["star"])
    image = torch.zeros((RS.STD_B, RS.STD_S, RS.STD_S, 3), device=DEV)
    with torch.no_grad():
        _, tex_img, _, tind = ops.render_depth(std["V"], net.tri, ops.synth_texture(net.mu_tex, net.pc_tex, alpha), image)
    got = raw_image(std, std["star"]).astype(np.float64)
    want = tex_img.cpu().numpy().astype(np.float64)
    assert _same_bits(tind.cpu().numpy(), std["tri_ind"])
    bound = RS.image_bound(net.tri.cpu().numpy(), net.mu_tex.cpu().numpy(), net.pc_tex.cpu().numpy(), std["tri_ind"], std["star"])
    cov = std["tri_ind"][..., 0] >= 0
    frac = (np.abs(got - want)[cov] / bound[cov]).max()
    print("max |image - render| / bound = %.3f over %d covered pixels" % (frac, cov.sum()))
    assert frac <= 1.0 and (bound[cov] > 0).all()


# ---- moments and solves ------------------------------------------------------------------------------------------------------------------
def _check_solve(M, K, ridge, x32, stats, what):
    G, r = M[:K, :K], M[:K, K]
    Gp = G + RS.ridge_lambda(M, K, ridge) * np.eye(K)
    xh = x32.astype(np.float64)
    res = np.abs(Gp @ xh - r).max()
    lim = 2.0 ** -23 * ((np.abs(Gp) @ np.abs(xh)).max() + np.abs(r).max())
    print("  %s: backward error %.3g of %.3g, E0 %.6g, E1 %.6g" % (what, res, lim, stats[1], stats[2]))
    assert res <= lim
    want = RS.e1_of(M, K, x32)
    assert abs(stats[2] - want) <= 1e-12 * abs(want) and stats[2] <= stats[1] and stats[1] == M[K, K]


VARIANTS = [("standard", "plain"), ("standard", "weight"), ("standard", "gate"), ("13x11", "plain"), ("1x1", "plain"),
            ("25x41", "plain"), ("25x41", "weight+gate"), ("67x65", "plain"), ("67x65", "weight"), ("8x40", "gate")]


@pytest.mark.parametrize("name,variant", VARIANTS)
def test_light_moments_and_solve(cases, name, variant):
    inp = cases[name]
    B, H, W = inp["normal"].shape[:3]
    weight = inp["weight"] if "weight" in variant else None
    gate = _gate_for(inp) if "gate" in variant else None
    ridge = 0.0 if name == "standard" else 1e-9
    light, st, M = raw_light(inp, inp["tex"], weight, gate, ridge)
    rlight, rst, RM, RSc = RS.light_fit_ref(inp["tex"], inp["normal"], inp["tri_ind"], inp["target"], weight, gate, ridge=ridge)
    if gate is not None and H * W > 64:      # the gate leaves both lit and unlit counted pixels in every channel
        live = RS.light_x(inp["tex"], inp["normal"], inp["tri_ind"], inp["target"], weight)[2]
        assert ((rst[:, :, 0] > 0) & (rst[:, :, 0] < live.sum(2))).all()
    if weight is not None:
        assert (weight[inp["tri_ind"][..., 0] >= 0] == 0).any()
    bound = RA.gamma(H * W) * RSc
    err = np.abs(M - RM)
    print("%s %s: max |M - fsum| / (gamma_n sum|w x_i x_j|) = %.3g" % (name, variant, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert _same_bits(M, np.swapaxes(M, 2, 3)) and not _bits64(M[:, :, 10:, :]).any() and not _bits64(M[:, :, :, 10:]).any()
    assert np.array_equal(st[:, :, 0], rst[:, :, 0]) and np.array_equal(st[:, :, 3], rst[:, :, 3])
    light2, st2, M2 = raw_light(inp, inp["tex"], weight, gate, ridge)
    assert _same_bits(M, M2) and _same_bits(light, light2) and _same_bits(st, st2)
    for b in range(B):
        one = _faces(inp, slice(b, b + 1))
        l1, s1, M1 = raw_light(one, one["tex"], None if weight is None else one["weight"], None if gate is None else gate[b:b + 1], ridge)
        assert _same_bits(M1[0], M[b]) and _same_bits(l1[0], light[b]) and _same_bits(s1[0], st[b]), b
        for c in range(3):
            if st[b, c, 3] == 1.0:
                _check_solve(M[b, c], 9, ridge, light[b, c], st[b, c], "face %d channel %d" % (b, c))
            else:
                want = np.zeros(9, F) if gate is None else gate[b, c]
                assert _same_bits(light[b, c], want) and st[b, c, 2] == st[b, c, 1]
    if H * W > 64:
        assert (st[:, :, 3] == 1.0).all()
    if name == "standard" and variant == "plain":
        for b in range(B):
            rec = np.linalg.norm(light[b].astype(np.float64) - inp["light"][b]) / np.linalg.norm(inp["light"][b])
            assert rec <= 4.6e-6, (b, rec)                                   # ten times the model's (the CPU file)


@pytest.mark.parametrize("name,variant", [("standard", "plain"), ("standard", "weight"), ("13x11", "plain"), ("1x1", "plain"),
                                          ("25x41", "plain"), ("25x41", "weight"), ("67x65", "plain"), ("8x40", "weight")])
def test_albedo_moments_and_solve(cases, name, variant):
    inp = cases[name]
    B, H, W = inp["normal"].shape[:3]
    K = inp["basis"].shape[2] - 1
    weight = inp["weight"] if "weight" in variant else None
    ridge = 0.0 if name == "standard" else 1e-9
    alpha, st, M = raw_albedo(inp, inp["light"], weight, ridge)
    ralpha, rst, RM, RSc = RS.albedo_fit_ref(inp["basis"], inp["tri_ind"], inp["normal"], inp["light"], inp["target"], weight, ridge=ridge)
    bound = RA.gamma(3 * H * W) * RSc
    err = np.abs(M - RM)
    print("%s %s: max |M - fsum| / (gamma_n sum|w x_i x_j|) = %.3g" % (name, variant, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert _same_bits(M, np.swapaxes(M, 1, 2)) and not _bits64(M[:, K + 1:, :]).any() and not _bits64(M[:, :, K + 1:]).any()
    assert np.array_equal(st[:, 0], rst[:, 0]) and np.array_equal(st[:, 3], rst[:, 3])
    alpha2, st2, M2 = raw_albedo(inp, inp["light"], weight, ridge)
    assert _same_bits(M, M2) and _same_bits(alpha, alpha2) and _same_bits(st, st2)
    for b in range(B):
        one = _faces(inp, slice(b, b + 1))
        a1, s1, M1 = raw_albedo(one, one["light"], None if weight is None else one["weight"], ridge)
        assert _same_bits(M1[0], M[b]) and _same_bits(a1[0], alpha[b]) and _same_bits(s1[0], st[b]), b
        if st[b, 3] == 1.0:
            _check_solve(M[b], K, ridge, alpha[b], st[b], "face %d" % b)
        else:
            assert not alpha[b].view(np.uint32).any() and st[b, 2] == st[b, 1]
    if 3 * H * W > 64:
        assert (st[:, 3] == 1.0).all()
    if name == "standard" and variant == "plain":
        for b in range(B):
            rec = np.linalg.norm(alpha[b].astype(np.float64) - inp["star"][b]) / np.linalg.norm(inp["star"][b])
            assert rec <= 3.2e-7, (b, rec)                                   # ten times the model's (the CPU file)


# ---- the failure rules -------------------------------------------------------------------------------------------------------------------
def test_face_off_the_image(net):
    inp = _rendered(net, 5, shift={3: (100.0, 0.0)})
    assert (inp["tri_ind"][3] >= 0).sum() == 0 and (inp["tri_ind"][4] >= 0).sum() > 300
    prev = RS.std_light(5, seed=21)
    light, st, M = raw_light(inp, inp["tex"], gate=prev)
    assert (st[3] == 0).all() and _same_bits(light[3], prev[3]) and not _bits64(M[3]).any()      # previous values kept
    keep = [0, 1, 2, 4]
    assert (st[keep, :, 3] == 1.0).all()
    l4, s4, M4 = raw_light(_faces(inp, keep), inp["tex"][keep], gate=prev[keep])
    assert _same_bits(l4, light[keep]) and _same_bits(s4, st[keep]) and _same_bits(M4, M[keep])
    alpha, sa, Ma = raw_albedo(inp, inp["light"])
    assert sa[:, 3].tolist() == [1.0, 1.0, 1.0, 0.0, 1.0] and not sa[3].any() and not alpha[3].view(np.uint32).any()
    a4, s4, M4 = raw_albedo(_faces(inp, keep), inp["light"][keep])
    assert _same_bits(a4, alpha[keep]) and _same_bits(s4, sa[keep]) and _same_bits(M4, Ma[keep])
    # the loop: the face keeps its starting values, no other face moves by a bit
    ops = _ops()
    a0 = _dev(0.1 * np.random.RandomState(4).standard_normal((5, RS.STD_K)))
    args = (_dev(inp["basis"], torch.float64), _dev(inp["tri_ind"]), _dev(inp["normal"]), _dev(inp["target"]))
    lf, af, _, info = ops.photo_solve_rgb(*args, alpha0=a0, light0=_dev(prev), iters=3)
    assert info["ok"][:, :, 3].sum() == 0 and bool(info["ok"][:, :, keep].all())
    assert _same_bits(lf[3].cpu().numpy(), prev[3]) and _same_bits(af[3].cpu().numpy(), a0[3].cpu().numpy())
    sub = [x[keep].contiguous() for x in args[1:]]
    l4, a4, _, _ = ops.photo_solve_rgb(args[0], *sub, alpha0=a0[keep].contiguous(), light0=_dev(prev[keep]), iters=3)
    assert _same_bits(l4.cpu().numpy(), lf[keep].cpu().numpy()) and _same_bits(a4.cpu().numpy(), af[keep].cpu().numpy())


def test_poisoned_face(std):
    T = std["target"].copy()
    cov = np.flatnonzero(std["tri_ind"].reshape(RS.STD_B, -1)[1] >= 0)
    T.reshape(RS.STD_B, -1, 3)[1, cov[17], 2] = np.nan
    bad = dict(std, target=T)
    light, st, M = raw_light(bad, std["tex"])
    clean = raw_light(std, std["tex"])
    assert st[:, :, 3].tolist() == [[1.0] * 3, [1.0, 1.0, 0.0], [1.0] * 3] and not light[1, 2].view(np.uint32).any()
    assert np.isnan(M[1, 2, 9, 9]) and st[1, 2, 0] == clean[1][1, 2, 0]
    for b, c in [(0, 0), (0, 2), (1, 0), (1, 1), (2, 2)]:                   # the other channels and faces: not a bit moves
        assert _same_bits(light[b, c], clean[0][b, c]) and _same_bits(st[b, c], clean[1][b, c]) and _same_bits(M[b, c], clean[2][b, c])
    alpha, sa, Ma = raw_albedo(bad, std["light"])
    cleana = raw_albedo(std, std["light"])
    assert sa[:, 3].tolist() == [1.0, 0.0, 1.0] and not alpha[1].view(np.uint32).any()
    for b in (0, 2):
        assert _same_bits(alpha[b], cleana[0][b]) and _same_bits(sa[b], cleana[1][b]) and _same_bits(Ma[b], cleana[2][b])
    # a NaN at a pixel the face does not cover is not counted
    T = std["target"].copy()
    T.reshape(RS.STD_B, -1, 3)[1, np.flatnonzero(std["tri_ind"].reshape(RS.STD_B, -1)[1] < 0)[5]] = np.nan
    again = raw_light(dict(std, target=T), std["tex"])
    assert all(_same_bits(x, y) for x, y in zip(again, clean))
    again = raw_albedo(dict(std, target=T), std["light"])
    assert all(_same_bits(x, y) for x, y in zip(again, cleana))


def test_three_pixel_face_fails_without_a_ridge_and_fits_with_one(std):
    tind = std["tri_ind"].copy()
    flat = tind.reshape(RS.STD_B, -1)
    flat[1, np.flatnonzero(flat[1] >= 0)[3:]] = -1.0
    inp = dict(std, tri_ind=tind)
    l0, s0, M0 = raw_light(inp, std["tex"], ridge=0.0)
    assert (s0[1, :, 0] == 3.0).all() and s0[:, :, 3].tolist() == [[1.0] * 3, [0.0] * 3, [1.0] * 3]
    assert not l0[1].view(np.uint32).any() and (s0[1, :, 2] == s0[1, :, 1]).all()
    l1, s1, M1 = raw_light(inp, std["tex"], ridge=1e-6)
    assert (s1[:, :, 3] == 1.0).all() and l1[1].any() and (s1[1, :, 2] <= s1[1, :, 1]).all() and _same_bits(M0, M1)
    a0, t0, N0 = raw_albedo(inp, std["light"], ridge=0.0)                    # nine samples, ten unknowns
    assert t0[1, 0] == 3.0 and t0[:, 3].tolist() == [1.0, 0.0, 1.0] and not a0[1].view(np.uint32).any() and t0[1, 2] == t0[1, 1]
    a1, t1, N1 = raw_albedo(inp, std["light"], ridge=1e-6)
    assert (t1[:, 3] == 1.0).all() and a1[1].any() and t1[1, 2] <= t1[1, 1] and _same_bits(N0, N1)
    full_l, full_a = raw_light(std, std["tex"]), raw_albedo(std, std["light"])
    for b in (0, 2):                                                        # the failed face leaves the others' bits alone
        assert _same_bits(l0[b], full_l[0][b]) and _same_bits(M0[b], full_l[2][b])
        assert _same_bits(a0[b], full_a[0][b]) and _same_bits(N0[b], full_a[2][b])


def test_special_tri_ind_values(cases):
    """-1 and NaN are uncovered; -0.0 is triangle 0; ntri and 2^24 are covered for the light fit (tri_ind >= 0, nothing gathered) and
    off the basis for the image and the albedo fit; a fractional id truncates"""
    inp = dict(cases["13x11"])
    ntri = inp["basis"].shape[0]
    tind = inp["tri_ind"].copy()
    flat = tind.reshape(-1)
    flat[:7] = [-1.0, np.nan, -0.0, ntri, 2.0 ** 24, 3.75, ntri - 0.5]
    inp["tri_ind"] = tind
    img = raw_image(inp, inp["star"])
    want = RS.image_ref(inp["basis"], tind, inp["star"])
    assert _same_bits(img, want)
    px = img.reshape(-1, 3)
    assert not px[[0, 1, 3, 4]].any() and px[[2, 5, 6]].all()
    assert _same_bits(px[5], RS.image_ref(inp["basis"], np.full((1, 1, 1, 1), 3.0, F), inp["star"]).reshape(3))
    tex = inp["tex"].copy()
    tex.reshape(-1, 3)[:7] = 0.5
    light, st, M = raw_light(inp, tex, ridge=1e-9)
    _, rst, RM, RSc = RS.light_fit_ref(tex, inp["normal"], tind, inp["target"], ridge=1e-9)
    base = float((flat[7:] >= 0).sum())
    assert (rst[0, :, 0] == base + 5).all() and np.array_equal(st[:, :, 0], rst[:, :, 0])
    assert (np.abs(M - RM) <= RA.gamma(tind.size) * RSc).all() and (st[:, :, 3] == 1.0).all()
    alpha, sa, Ma = raw_albedo(inp, inp["light"], ridge=1e-9)
    _, rsa, RMa, RSa = RS.albedo_fit_ref(inp["basis"], tind, inp["normal"], inp["light"], inp["target"], ridge=1e-9)
    assert rsa[0, 0] == base + 3 and sa[0, 0] == rsa[0, 0] and sa[0, 3] == 1.0
    assert (np.abs(Ma - RMa) <= RA.gamma(3 * tind.size) * RSa).all()


# ---- the operator and the loop -----------------------------------------------------------------------------------------------------------
def _loop_args(std):
    return (_dev(std["basis"], torch.float64), _dev(std["tri_ind"]), _dev(std["normal"]), _dev(std["target"]))


def test_operators_and_the_loop_equal_the_raw_calls_chained_by_hand(std):
    ops = _ops()
    args = _loop_args(std)
    w = _dev(std["weight"])
    light, st = ops.photo_light_lse_rgb(_dev(std["tex"]), args[2], args[1], args[3], weight=w, ridge=1e-9)
    assert light.dtype == torch.float32 and st.dtype == torch.float64 and not light.requires_grad and not st.requires_grad
    rl, rs, _ = raw_light(std, std["tex"], std["weight"], ridge=1e-9)
    assert _same_bits(light.cpu().numpy(), rl) and _same_bits(st.cpu().numpy(), rs)
    alpha, sa = ops.albedo_lse_rgb(args[0], args[1], args[2], light, args[3], weight=w, ridge=1e-9)
    ra, rsa, _ = raw_albedo(std, rl, std["weight"], ridge=1e-9)
    assert not alpha.requires_grad and _same_bits(alpha.cpu().numpy(), ra) and _same_bits(sa.cpu().numpy(), rsa)
    # the loop, three iterations, against the raw calls
    lf, af, tf, info = ops.photo_solve_rgb(*args, iters=3)
    torch.cuda.synchronize()
    al, li = np.zeros((RS.STD_B, RS.STD_K), F), None
    E = np.zeros((3, 2, RS.STD_B))
    for it in range(3):
        tex = raw_image(std, al)
        li, s, _ = raw_light(std, tex, gate=li)
        E[it, 0] = s[:, :, 2].sum(1)
        al, s, _ = raw_albedo(std, li)
        E[it, 1] = s[:, 2]
    assert _same_bits(lf.cpu().numpy(), li) and _same_bits(af.cpu().numpy(), al) and _same_bits(tf.cpu().numpy(), raw_image(std, al))
    assert info["E"].dtype == torch.float64 and tuple(info["E"].shape) == (3, 2, RS.STD_B) and bool(info["ok"].all())
    assert np.allclose(info["E"].cpu().numpy(), E, rtol=1e-14, atol=0)
    assert not lf.requires_grad and not af.requires_grad and not tf.requires_grad


def test_loop_descends_converges_and_lowers_the_photometric_loss(net, std):
    ops = _ops()
    args = _loop_args(std)
    lf, af, tf, info = net.photo_solve_rgb(*args[1:], iters=8)
    E = info["E"].cpu().numpy().reshape(-1, RS.STD_B)
    print("E per half-step and face:\n", E)
    assert bool(info["ok"].all())
    assert (E[1:] <= E[:-1] * (1 + 1e-12)).all()
    assert (E[-1] <= 1e-6 * E[0]).all()
    for b in range(RS.STD_B):
        assert np.linalg.norm(af[b].cpu().numpy() - std["star"][b]) <= 1e-3 * np.linalg.norm(std["star"][b])
    # photo_loss_rgb at the returned (tex_img, light) against its value at the start: the mean albedo under the first fitted light
    tex0 = _dev(raw_image(std, np.zeros((RS.STD_B, RS.STD_K), F)))
    l0, _ = ops.photo_light_lse_rgb(tex0, args[2], args[1], args[3])
    with torch.no_grad():
        sse0, cnt = ops.photo_loss_rgb(tex0, args[2], args[1], l0, args[3])
        sse1, _ = ops.photo_loss_rgb(tf, args[2], args[1], lf, args[3])
    print("photo_loss_rgb sse per face: start", sse0.cpu().numpy(), "end", sse1.cpu().numpy())
    assert bool((sse1 <= sse0).all()) and bool((cnt > 300).all())


# ---- threads -----------------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(std):
    ops = _ops()
    base = _loop_args(std)
    inputs = [base, base[:3] + ((base[3] * 0.5 + 0.1).contiguous(),)]
    single = []
    for a in inputs:
        l, al, _, info = ops.photo_solve_rgb(*a, iters=2)
        single.append((l.cpu().numpy(), al.cpu().numpy(), info["E"].cpu().numpy()))
    torch.cuda.synchronize()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                gate.wait(timeout=30)
                outs = [ops.photo_solve_rgb(*inputs[i], iters=2) for _ in range(10)]
                stream.synchronize()
            results[i] = [(l.cpu().numpy(), al.cpu().numpy(), info["E"].cpu().numpy()) for l, al, _, info in outs]
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for got in results[i]:
            assert all(_same_bits(x, y) for x, y in zip(got, single[i])), i
