"""GPU: fr_render_normal_backward (nbwd_records_kernel, nbwd_owner_kernel; csrc/fr_render_nbwd.hip) held to its float64 model with exact sums
(tests/ref_normal_backward.py, pinned on the CPU by tests/test_normal_backward_cpu.py), and the opt-in `normal_grad` flag of the
Python surface.

Raw mode:   |got - S| <= 2^-24 |S| + n_v 2^(shift - 39) M        S the exact sum of the model's fp32 terms, n_v their number,
post mode:  the same + 2^-23 A                                   M the face's largest |term|, A = sum |term|  (a post-mode term
                                                                 may differ from the model's by one fp32 ulp: sqrt and divide)
evaluated in integers; an element without terms must be +0.  tri_ind always comes from the product's own forward; the launch
geometry a case is written for is read from fr_debug_render_normal_bwd_geom (the launcher's own function)."""
import ctypes

import numpy as np
import pytest
import torch

import ref_normal_backward as RN
from conftest import pkg
from gpu_util import ops, net_mod
from raw_calls import nbwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _h():
    return pkg("_lib")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def geom(B, nver, H, W):
    out = (ctypes.c_int * 6)()
    _h().lib().fr_debug_render_normal_bwd_geom(B, nver, H, W, out)
    return dict(zip(("splits", "range", "shift", "chunks", "lds", "xcd"), out))


# ---- scenes: a handful of large triangles over chosen vertex ids of a mesh of any size -----------------------------------------
def make_scene(seed, B, nver, H, W, flip=False):
    """-> dict of numpy arrays: V [B,3,nver], tri [3,ntri], tind [B,H*W] (the product's forward), g [B,H*W,3].  The triangles
    use the vertices next to every owner boundary the launcher chooses for (B, nver) -- the last of one owner's range, the first
    of the next -- and the two ends of the mesh; the list holds a triangle twice, a triangle with a repeated vertex id (a
    segment: it paints the pixel centres its bounding box holds) and, for flip, clockwise triangles."""
    rs = np.random.RandomState(seed)
    r = geom(B, nver, H, W)["range"]
    special = sorted({0, 1, 2, nver - 1, nver - 2, nver // 2} | {min(nver - 1, max(0, k * r + d)) for k in (1, 2, 3) for d in (-1, 0)})
    special = np.array([s for s in special if 0 <= s < nver])
    V = np.zeros((B, 3, nver), np.float32)
    V[:, 0] = rs.uniform(0, W - 1, (B, nver))
    V[:, 1] = rs.uniform(0, H - 1, (B, nver))
    V[:, 2] = rs.uniform(1, 9, (B, nver))
    ntri = 10
    tri = np.stack([rs.choice(special, 3, replace=len(special) < 3) for _ in range(ntri)], axis=1).astype(np.float32)
    tri[:, 0] = special[[0, len(special) // 2, -1]]                           # one triangle across the whole vertex range
    tri[:, 3] = tri[:, 2]                                                     # the same triangle twice
    tri[:, 4] = (tri[0, 0], tri[0, 0], tri[2, 0])                             # a repeated vertex id
    p, q, apex = int(tri[0, 4]), int(tri[2, 4]), int(tri[1, 0])               # ... on a pixel row, in front of everything;
    V[:, 0, p], V[:, 0, q] = 0.4, W - 1.6                                     # triangle 0 stands on it, its apex near row 0
    V[:, 1, p] = V[:, 1, q] = H // 2
    V[:, 2, p] = V[:, 2, q] = 9.5
    V[:, 1, apex] = 0.3
    if flip:
        tri = tri[[0, 2, 1]].copy()
    tex = np.zeros((1, 3, nver), np.float32)
    outs = ops().render_depth(_t(V), _t(tri), _t(tex), torch.zeros((B, H, W, 3), device=DEV))
    tind = outs[3].cpu().numpy().reshape(B, H * W)
    g = rs.standard_normal((B, H * W, 3)).astype(np.float32)
    g[g == 0] = 1.0
    return dict(V=V, tri=tri, tind=tind, g=g, normal=outs[2].cpu().numpy().reshape(B, H * W, 3), H=H, W=W, B=B, nver=nver)


_SCENES = {}


def scene(B, nver, H, W, flip=False):
    key = (B, nver, H, W, flip)
    if key not in _SCENES:
        _SCENES[key] = make_scene(1000 * B + nver + 7 * H + int(flip), B, nver, H, W, flip)
    return _SCENES[key]


def run_case(sc, mode, **over):
    """the scene (with overrides) through the model and the kernel -> (got [B,3,nver] numpy, model)"""
    d = dict(sc, **over)
    R = RN.model(d["g"], d["V"], d["tri"], d["tind"], d["H"], d["W"], mode)
    got = nbwd(_t(d["g"]), _t(d["V"]), _t(d["tri"]), _t(d["tind"]), d["H"], d["W"], mode)
    torch.cuda.synchronize()
    return got.cpu().numpy(), R


BS = (1, 3, 8, 16)
HWS = ((5, 6), (33, 40), (40, 33))
NVERS = (3, 12, 20000)


# ---- K1 ----------------------------------------------------------------------------------------------------------------------------
def test_k1_known_answer_bit_for_bit():
    """(1,1,5), (4,1,5), (1,4,5) on W = 6, H = 5: six covered pixels, G = (0,0,1) on each."""
    V = np.array([[[1, 4, 1], [1, 1, 4], [5, 5, 5]]], np.float32)
    tri = np.array([[0], [1], [2]], np.float32)
    tind = ops().render_depth(_t(V), _t(tri), _t(np.zeros((1, 3, 3))), torch.zeros((1, 5, 6, 3), device=DEV))[3]
    assert int((tind >= 0).sum()) == 6
    g = np.zeros((1, 5, 6, 3), np.float32)
    g[..., 2] = 1
    got = nbwd(_t(g), _t(V), _t(tri), tind, 5, 6, 0)
    want = np.array([[[-18, 18, 0], [-18, 0, 18], [0, 0, 0]]], np.float32)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- differential cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nver", NVERS)
@pytest.mark.parametrize("H,W", HWS)
@pytest.mark.parametrize("B", BS)
def test_raw_mode_within_the_bound(B, H, W, nver):
    sc = scene(B, nver, H, W)
    gm = geom(B, nver, H, W)
    if nver == 20000:
        assert gm["splits"] >= 3 and gm["lds"] <= 160 * 1024, gm
        owners = {int(v) // gm["range"] for v in sc["tri"].ravel()}
        assert len(owners) >= 3                                               # the triangles do straddle owner boundaries
    assert gm["xcd"] == (1 if B % 8 == 0 else 0)
    cov = sc["tind"] >= 0
    assert cov.any() and not cov.all()                                        # covered pixels and background
    assert (sc["tind"] == 4).any() and (sc["tind"] == 0).any()                # the repeated-id triangle wins pixels
    got, R = run_case(sc, 0)
    assert not any(F.bad for F in R.faces)
    assert RN.check_bound(got, R) <= 1.0
    assert np.count_nonzero(got) > 0


@pytest.mark.parametrize("nver", NVERS)
@pytest.mark.parametrize("H,W", HWS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("flip", [False, True])
def test_post_mode_within_the_bound(B, H, W, nver, flip):
    sc = scene(B, nver, H, W, flip)
    got, R = run_case(sc, 1)
    for m in R.mag32:                                                         # the branch is a factor of 2 away from 1e-6 ...
        assert np.all((m == 0) | (m > 2e-6))                                  # ... except where the normal is exactly zero
    assert RN.check_bound(got, R, post=True) <= 1.0
    assert np.count_nonzero(got) > 0


def test_largest_owner_range_full_lds():
    """B = 64, nver = 4 * 6,656: four owners per face at the largest range the 160 KiB of LDS hold, through the XCD block map"""
    B, nver, H, W = 64, 26624, 5, 6
    gm = geom(B, nver, H, W)
    assert gm["splits"] == 4 and gm["range"] == 6656 and gm["xcd"] == 1 and 156 * 1024 <= gm["lds"] <= 160 * 1024
    sc = scene(B, nver, H, W)
    for mode in (0, 1):
        got, R = run_case(sc, mode)
        assert RN.check_bound(got, R, post=mode == 1) <= 1.0


def test_out_of_range_ids_and_indices_contribute_nothing():
    """a vertex id of nver, one of -1, and a tri_ind beyond a shortened triangle list: the model and the kernel skip the pixels"""
    sc = scene(3, 12, 33, 40)
    tri = sc["tri"].copy()
    used = [t for t in range(tri.shape[1] - 1) if (sc["tind"] == t).any()]
    assert len(used) >= 3 and (sc["tind"] == tri.shape[1] - 1).any()
    tri[1, used[0]] = sc["nver"]
    tri[2, used[1]] = -1
    short = np.ascontiguousarray(tri[:, :-1])
    R = RN.model(sc["g"], sc["V"], short, sc["tind"], 33, 40, 0)
    got = nbwd(_t(sc["g"]), _t(sc["V"]), _t(short), _t(sc["tind"]), 33, 40, 0)
    full = RN.model(sc["g"], sc["V"], sc["tri"], sc["tind"], 33, 40, 0)
    assert sum(int(F.n.sum()) for F in R.faces) < sum(int(F.n.sum()) for F in full.faces)
    assert RN.check_bound(got.cpu().numpy(), R) <= 1.0


def test_post_mode_zero_normal_and_negative_zero():
    """SURVEY K4's collinear triangle (1,1), (4,4), (2.5,2.5) paints its bounding box with a zero normal: the mag <= 1e-6
    branch, G = g' / (1 + 1e-6).  A second face: a triangle whose n.z is -0 (a vertical wall seen edge-on ... with n.z = (-0)):
    s = +1, no flip."""
    V = np.zeros((2, 3, 3), np.float32)
    V[0] = [[1, 4, 2.5], [1, 4, 2.5], [5, 8, 6.5]]                            # (collinear in z as well: a x b = 0)
    # face 1: a = P1 - P2 = (-3, 0, -2), b = P1 - P3 = (0, 0, -3): n = (0*-3 - -2*0, -2*0 - -3*-3, -3*0 - 0*0) = (0, -9, -0)
    V[1] = [[1, 4, 1], [2, 2, 2], [5, 7, 8]]
    tri = np.array([[0], [1], [2]], np.float32)
    outs = ops().render_depth(_t(V), _t(tri), _t(np.zeros((1, 3, 3))), torch.zeros((2, 5, 6, 3), device=DEV))
    tind, normal = outs[3].cpu().numpy().reshape(2, -1), outs[2].cpu().numpy().reshape(2, -1, 3)
    assert (tind[0] == 0).sum() == 16 and not normal[0].any()
    cov1 = tind[1] == 0
    assert cov1.any() and np.all(normal[1][cov1].view(np.uint32) == np.array([0, 0xC1100000, 0x80000000], np.uint32))
    rs = np.random.RandomState(5)
    g = rs.standard_normal((2, 30, 3)).astype(np.float32)
    R = RN.model(g, V, tri, tind, 5, 6, 1)
    assert np.all(R.mag32[0] == 0) and np.all(R.mag32[1] == 81)
    got = nbwd(_t(g), _t(V), _t(tri), _t(tind), 5, 6, 1).cpu().numpy()
    assert RN.check_bound(got, R, post=True) <= 1.0
    assert np.count_nonzero(got[0]) > 0 and np.count_nonzero(got[1]) > 0


# ---- accumulate, zeros, layouts, reproducibility, non-finite ------------------------------------------------------------------------------
def test_accumulate_completes_the_depth_backward():
    h, L = _h(), _h().lib()
    sc = scene(8, 20000, 33, 40)
    B, nver, H, W = 8, 20000, 33, 40
    g, V, tri, ti = _t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    dg = torch.randn((B, H, W, 1), generator=torch.Generator().manual_seed(3)).to(DEV)
    nws = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    ws = torch.empty((nws,), dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in (0, 1):
        depth_part = torch.full((B, 3, nver), float("nan"), device=DEV)
        assert L.fr_render_depth_backward_ws(h.ptr(dg), h.ptr(tri), h.ptr(ti), h.ptr(depth_part), B, nver, int(tri.shape[1]), H, W,
                                             h.ptr(ws), nws, st) == 0
        both = depth_part.clone()
        normal_part = nbwd(g, V, tri, ti, H, W, mode)
        nbwd(g, V, tri, ti, H, W, mode, out=both, accumulate=1)
        assert _same(both, depth_part + normal_part)
        untouched = normal_part == 0
        assert bool(untouched.any()) and bool((_bits(both)[untouched] == _bits(depth_part)[untouched]).all())
        assert float(both[:, 2].abs().max()) > 0 and float(both[:, 0].abs().max()) > 0


def test_zero_gradient_and_all_background_give_plus_zero():
    sc = scene(3, 12, 33, 40)
    g0 = np.zeros_like(sc["g"])
    g0[0] = -0.0
    for mode in (0, 1):
        got = nbwd(_t(g0), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"]), 33, 40, mode)
        assert not bool(_bits(got).any())
        tind = sc["tind"].copy()
        tind[1] = -1                                                          # one face all background, gradients non-zero
        got = nbwd(_t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(tind), 33, 40, mode)
        assert not bool(_bits(got[1]).any()) and bool(got[0].abs().sum() > 0)


def test_pitched_vertices_and_stride_7_give_the_dense_bits():
    L = _h().lib()
    for B, nver in ((3, 12), (8, 20000)):
        sc = scene(B, nver, 33, 40)
        H, W = 33, 40
        pitch = L.fr_decode_render_vertex_pitch(nver)
        assert pitch >= nver and (nver != 12 or pitch > nver)
        g, tri, ti = _t(sc["g"]), _t(sc["tri"]), _t(sc["tind"])
        Vp = torch.full((B, 3, pitch), float("nan"), device=DEV)
        Vp[:, :, :nver] = _t(sc["V"])
        g7 = torch.full((B, H * W, 7), float("nan"), device=DEV)
        g7[:, :, 4:7] = g
        for mode in (0, 1):
            dense = nbwd(g, _t(sc["V"]), tri, ti, H, W, mode)
            assert _same(nbwd(g, Vp, tri, ti, H, W, mode, pitch=(pitch, nver)), dense)
            assert _same(nbwd(g7, _t(sc["V"]), tri, ti, H, W, mode, stride=7, offset=4), dense)
            assert _same(nbwd(g7, Vp, tri, ti, H, W, mode, stride=7, offset=4, pitch=(pitch, nver)), dense)


def test_two_runs_and_two_streams_are_bit_identical():
    sc = scene(16, 20000, 40, 33)
    g, V, tri, ti = _t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    for mode in (0, 1):
        first = nbwd(g, V, tri, ti, 40, 33, mode)
        second = nbwd(g, V, tri, ti, 40, 33, mode)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
        outs = []
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs.append(nbwd(g, V, tri, ti, 40, 33, mode))
        torch.cuda.synchronize()
        assert _same(first, second) and _same(outs[0], first) and _same(outs[1], first)


def test_an_infinite_gradient_reaches_exactly_its_triangle():
    sc = scene(3, 20000, 33, 40)
    g = sc["g"].copy()
    px = int(np.flatnonzero(sc["tind"][1] >= 0)[3])
    g[1, px, 0] = np.inf
    ids = {int(sc["tri"][k, int(sc["tind"][1, px])]) for k in range(3)}
    got, R = run_case(sc, 0, g=g)
    assert [F.bad for F in R.faces] == [False, True, False]
    assert RN.check_bound(got, R) <= 1.0                                      # the other faces are untouched by it
    nonfinite = ~np.isfinite(got[1])
    np.testing.assert_array_equal(nonfinite, R.dense(1, "nonfinite"))         # element by element, as the model's terms say
    assert set(np.flatnonzero(nonfinite.any(axis=0)).tolist()) == ids         # ... which is: the pixel's three vertices


# ---- Python surface ------------------------------------------------------------------------------------------------------------------------
class _Py:
    pass


@pytest.fixture(scope="module")
def py(small_assets, synth):
    """the small mesh decoded at 40 x 40, four faces; random weights for every output"""
    s = _Py()
    s.B, s.S = 4, 40
    A = small_assets
    s.net = net_mod().FaceRecNet(mesh_data=A, batch_size=s.B, im_size=s.S, device=torch.device(DEV))
    rs = np.random.RandomState(0)
    P = np.zeros((s.B, 7 + A["ndim_shape"] + A["ndim_exp"]), np.float32)
    P[:, 0:3] = rs.uniform(-0.5, 0.5, (s.B, 3))
    P[:, 3:5] = rs.uniform(17, 23, (s.B, 2))
    P[:, 6] = rs.uniform(1.6e-4, 2.2e-4, s.B)
    P[:, 7:7 + A["ndim_shape"]] = rs.uniform(0, 1e4, (s.B, A["ndim_shape"]))
    P[:, 7 + A["ndim_shape"]:] = rs.uniform(-1.5, 1.5, (s.B, A["ndim_exp"]))
    s.P = _t(P)
    s.V = s.net.vertices_transform(s.P).detach()
    s.nver = int(s.V.shape[2])
    gen = torch.Generator().manual_seed(9)
    s.wn = torch.randn((s.B, s.S, s.S, 3), generator=gen).to(DEV)
    s.wd = torch.randn((s.B, s.S, s.S, 1), generator=gen).to(DEV)
    s.w7 = torch.randn((s.B, s.S, s.S, 7), generator=gen).to(DEV)
    s.im = torch.rand((s.B, s.S, s.S, 1), generator=gen).to(DEV)
    s.image = torch.zeros((s.B, s.S, s.S, 3), device=DEV)
    return s


def _restatement_check(got, w, V, tri, tind, S, mode):
    """|got - float64 autograd| <= (n_v + 1) 2^-24 A per element: half an fp32 ulp per term (2^-24 A in all), one rounding of
    the sum and the fixed-point grid.  The restatement takes the forward's fp32 a, b and n straight-through (RN.torch_grad), as
    the backward is defined to."""
    g, Vn, trin, tin = w.cpu().numpy(), V.cpu().numpy(), tri.cpu().numpy(), tind.cpu().numpy().reshape(V.shape[0], -1)
    want = RN.torch_grad(g, Vn, trin, tin, S, S, mode)
    R = RN.model(g, Vn, trin, tin, S, S, mode)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    worst = 0.0
    for b in range(V.shape[0]):
        bound = (R.dense(b, "n") + 1) * 2.0 ** -24 * R.dense(b, "A")
        assert np.all(err[b] <= bound), float((err[b] / np.maximum(bound, 1e-300)).max())
        worst = max(worst, float((err[b][bound > 0] / bound[bound > 0]).max()))
    return worst


def test_render_depth_normal_grad_flag(py):
    o, s = ops(), py

    def run(flag, use_depth, use_normal):
        V = s.V.clone().requires_grad_(True)
        kw = {} if flag is None else dict(normal_grad=flag)
        outs = o.render_depth(V, s.net.tri, s.net.vertex_code, s.image, **kw)
        loss = 0
        if use_depth:
            loss = loss + (outs[0].clamp_min(0) * s.wd).sum()
        if use_normal:
            loss = loss + (outs[2] * s.wn).sum()
        loss.backward()
        return [t.detach() for t in outs], V.grad
    outs0, g0 = run(None, True, True)
    outsF, gF = run(False, True, True)
    outs1, g1 = run(True, True, True)
    for a, b, c in zip(outs0, outsF, outs1):
        assert _same(a, b) and _same(a, c)
    assert _same(gF, g0) and not bool(_bits(g0[:, 0:2]).any())               # off: as before, x and y rows exactly +0
    _, gn = run(True, False, True)                                            # the normal part alone (accumulate = 0)
    _, gd = run(True, True, False)                                            # the depth part alone through the new node
    assert _same(gd, run(None, True, False)[1])
    assert _same(g1, gd + gn)                                                 # one fp32 add per element
    assert float(gn[:, 0].abs().max()) > 0 and float(gn[:, 1].abs().max()) > 0
    worst = _restatement_check(gn, s.wn, s.V, s.net.tri, outs0[3], s.S, 0)
    print("render_depth(normal_grad=True): worst error / bound = %.3f" % worst)
    # a loss that uses neither output: no gradient, as before
    V = s.V.clone().requires_grad_(True)
    o.render_depth(V, s.net.tri, s.net.vertex_code, s.image, normal_grad=True)[1].sum().backward()
    assert V.grad is None


def test_rendering_layer_fused_normal_grad_flag(py):
    o, s = ops(), py

    def run(flag, w7):
        V = s.V.clone().requires_grad_(True)
        kw = {} if flag is None else dict(normal_grad=flag)
        outs = o.rendering_layer_fused(V, s.net.tri, s.net.vertex_code, s.im, **kw)
        ((outs[0] * w7).sum() + (outs[1] * s.wd).sum()).backward()
        return [t.detach() for t in outs], V.grad
    outs0, g0 = run(None, s.w7)
    outsF, gF = run(False, s.w7)
    outs1, g1 = run(True, s.w7)
    for a, b, c in zip(outs0, outsF, outs1):
        assert _same(a, b) and _same(a, c)
    assert _same(gF, g0) and not bool(_bits(g0[:, 0:2]).any())
    wn = torch.zeros_like(s.w7)
    wn[..., 4:7] = s.w7[..., 4:7]
    V = s.V.clone().requires_grad_(True)
    (o.rendering_layer_fused(V, s.net.tri, s.net.vertex_code, s.im, normal_grad=True)[0] * wn).sum().backward()
    gn = V.grad                                                               # the normal channels alone: the depth part is +0
    assert _same(g1, g0 + gn)
    assert float(gn[:, 0].abs().max()) > 0 and float(gn[:, 1].abs().max()) > 0
    worst = _restatement_check(gn, s.w7[..., 4:7].contiguous(), s.V, s.net.tri, outs0[3], s.S, 1)
    print("rendering_layer_fused(normal_grad=True): worst error / bound = %.3f" % worst)


def test_decode_rendering_layer_normal_grad_is_the_two_step_route(py):
    s, net = py, py.net

    def run(route, flag):
        p = s.P.clone().requires_grad_(True)
        kw = {} if flag is None else dict(normal_grad=flag)
        if route == "one":
            ni, di = net.decode_rendering_layer(p, im_gray=s.im, **kw)
        else:
            ni, di = net.coarse_net_input(net.vertices_transform(p), im_gray=s.im, **kw)
        ((ni * s.w7).sum() + (di * s.wd).sum()).backward()
        return ni.detach(), di.detach(), p.grad, type(ni.grad_fn).__name__
    one = run("one", True)
    two = run("two", True)
    assert one[3] == two[3] and not one[3].startswith("_DecodeRenderingLayer")
    assert _same(one[0], two[0]) and _same(one[1], two[1]) and _same(one[2], two[2])
    off, never = run("one", False), run("one", None)
    assert never[3].startswith("_DecodeRenderingLayer") and off[3] == never[3]
    assert _same(off[0], never[0]) and _same(off[1], never[1]) and _same(off[2], never[2])
    assert _same(one[0], never[0]) and _same(one[1], never[1])
    assert not _same(one[2], never[2])                                        # the normal channels now move the parameters
    with pytest.raises(NotImplementedError):
        ops().decode_rendering_layer(s.P, None, s.im, net.tri, net.vertex_code, net._basis, net.im_size, normal_grad=True)


def test_coarse_net_normal_grad_reaches_the_network(small_assets):
    """a loss on the normal channels of the final parameters' rendering: without the flag it moves nothing (exact zeros), with
    it the gradient reaches the last iteration and, through the loop's own normal channels, the first"""
    netm, cn = net_mod(), pkg("nets.coarse_net")
    S, B = 40, 2
    face = netm.FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S)
    face.init_pred_params[..., 6] = 2e-4
    torch.manual_seed(1)
    im = torch.rand((B, S, S, 1), device=DEV)
    for flag in (False, True):
        torch.manual_seed(0)
        model = cn.CoarseNet(face, nIter=2, normal_grad=flag).cuda()
        params = model(im)
        kw = dict(normal_grad=True) if flag else {}
        ni, _ = face.coarse_net_input(face.vertices_transform(params), im_gray=im, **kw)
        ni[..., 4:7].square().sum().backward()
        last, first = model.iters[-1].fc.weight.grad, model.iters[0].fc.weight.grad
        assert bool(torch.isfinite(last).all()) and bool(torch.isfinite(first).all())
        if flag:
            assert float(last.abs().max()) > 0 and float(first.abs().max()) > 0
        else:
            assert float(last.abs().max()) == 0 and float(first.abs().max()) == 0
