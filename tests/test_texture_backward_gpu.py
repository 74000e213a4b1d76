"""GPU: fr_render_texture_backward (tbwd_records_kernel, tbwd_owner_kernel, tbwd_finish_kernel; csrc/fr_render_tbwd.hip) held BIT FOR BIT to its integer
model (tests/ref_texture_backward.py, pinned on the CPU by tests/test_texture_backward_cpu.py), fr_sfs_intensity_backward_tex to
numpy float64 on the state the GPU wrote, and the opt-in texture flags of the Python surface.

tri_ind always comes from the product's own forward; the launch geometry a case is written for is read from
fr_debug_render_texture_bwd_geom (the launcher's own function)."""
import argparse
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import ref_texture_backward as RT
from conftest import pkg, ROOT
from gpu_util import ops, net_mod, assert_bits_equal
from raw_calls import tbwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOM = ("splits", "range", "shift", "chunks", "lds", "xcd", "slices")


def _h():
    return pkg("_lib")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def geom(B, nver, H, W, tb):
    out = (ctypes.c_int * 7)()
    _h().lib().fr_debug_render_texture_bwd_geom(B, nver, H, W, tb, out)
    return dict(zip(GEOM, out))


# ---- scenes: a handful of large triangles over chosen vertex ids of a mesh of any size -----------------------------------------
def make_scene(seed, B, nver, H, W):
    """-> dict of numpy arrays: tri [3,ntri], tind [B,H*W] (the product's forward), g [B,H*W,3].  The triangles use the vertices
    next to every owner boundary the launcher chooses for (B, nver) -- the last of one owner's range, the first of the next -- and
    the two ends of the mesh; the list holds a triangle twice and a triangle that names one vertex three times... which covers no
    pixel, so another names one vertex twice (a segment: it paints the pixel centres its bounding box holds)."""
    rs = np.random.RandomState(seed)
    r = max(geom(B, nver, H, W, B)["range"], 1)
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
    tex = np.zeros((1, 3, nver), np.float32)
    outs = ops().render_depth(_t(V), _t(tri), _t(tex), torch.zeros((B, H, W, 3), device=DEV))
    tind = outs[3].cpu().numpy().reshape(B, H * W)
    g = rs.standard_normal((B, H * W, 3)).astype(np.float32)
    g[g == 0] = 1.0
    return dict(tri=tri, tind=tind, g=g, H=H, W=W, B=B, nver=nver)


_SCENES = {}


def scene(B, nver, H, W):
    key = (B, nver, H, W)
    if key not in _SCENES:
        _SCENES[key] = make_scene(1000 * B + nver + 7 * H, B, nver, H, W)
    return _SCENES[key]


def run_case(sc, tb, **over):
    """the scene (with overrides) through the model and the kernel -> (got [tb,3,nver] numpy, model)"""
    d = dict(sc, **over)
    M = RT.model(d["g"], d["tri"], d["tind"], d["nver"], d["H"], d["W"], tb)
    got = tbwd(_t(d["g"]), _t(d["tri"]), _t(d["tind"]), d["nver"], d["H"], d["W"], tb)
    torch.cuda.synchronize()
    return got.cpu().numpy(), M


def assert_model_bits(got, M, what=""):
    assert not M.bad.any()
    assert_bits_equal(got, M.value(), what)


BS = (1, 3, 8, 17)
HWS = ((5, 7), (33, 31), (40, 40))
NVERS = (12, 20000)


# ---- known answer -----------------------------------------------------------------------------------------------------------------------
def test_known_answer_bit_for_bit():
    """(1,1,5), (4,1,5), (1,4,5) on W = 6, H = 5: six covered pixels, g = (3, 6, -9) on each -> six terms (1, 2, -3) a vertex"""
    V = np.array([[[1, 4, 1], [1, 1, 4], [5, 5, 5]]], np.float32)
    tri = np.array([[0], [1], [2]], np.float32)
    tind = ops().render_depth(_t(V), _t(tri), _t(np.zeros((1, 3, 3))), torch.zeros((1, 5, 6, 3), device=DEV))[3]
    assert int((tind >= 0).sum()) == 6
    g = np.zeros((1, 5, 6, 3), np.float32)
    g[...] = (3, 6, -9)
    got = tbwd(_t(g), _t(tri), tind, 3, 5, 6, 1)
    want = np.array([[[6, 6, 6], [12, 12, 12], [-18, -18, -18]]], np.float32)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- differential cases: bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nver", NVERS)
@pytest.mark.parametrize("H,W", HWS)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B", BS)
def test_bits_are_the_models(B, shared, H, W, nver):
    tb = 1 if shared else B
    sc = scene(B, nver, H, W)
    gm = geom(B, nver, H, W, tb)
    assert gm["chunks"] == (2 if H * W > 1024 else 1) and gm["lds"] <= 160 * 1024 and gm["shift"] == 0
    if nver == 12:
        assert gm["splits"] == 1
    else:
        assert gm["splits"] >= 3, gm
        owners = {int(v) // gm["range"] for v in sc["tri"].ravel()}
        assert len(owners) >= 3                                               # the triangles do straddle owner boundaries
    if shared and B > 1:
        assert gm["slices"] >= 1 and gm["xcd"] == (1 if gm["slices"] % 8 == 0 else 0)
        if B == 17 and nver == 20000:
            assert gm["slices"] < B                                           # slices of more than one face
        if B == 8:
            assert gm["xcd"] == 1
    else:
        assert gm["slices"] == 0 and gm["xcd"] == (1 if B % 8 == 0 else 0)
    cov = sc["tind"] >= 0
    assert cov.any() and not cov.all()                                        # covered pixels and background
    assert (sc["tind"] == 4).any() and (sc["tind"] == 0).any()                # the repeated-id triangle wins pixels
    got, M = run_case(sc, tb)
    assert_model_bits(got, M, "B=%d tb=%d %dx%d nver=%d" % (B, tb, H, W, nver))
    assert np.count_nonzero(got) > 0


@pytest.mark.parametrize("shared", [False, True])
def test_largest_owner_range_full_lds(shared):
    """B = 64, nver = 4 * 6,656 on 32 x 32: four owners per face (or slice) at the largest range the 160 KiB of LDS hold"""
    B, nver, H, W = 64, 26624, 32, 32
    tb = 1 if shared else B
    gm = geom(B, nver, H, W, tb)
    assert gm["splits"] == 4 and gm["range"] == 6656 and gm["xcd"] == 1 and 156 * 1024 <= gm["lds"] <= 160 * 1024
    got, M = run_case(scene(B, nver, H, W), tb)
    assert_model_bits(got, M)
    assert np.count_nonzero(got) > 0


def test_shift_above_zero_shared_scope():
    """17 faces of 256 x 256 into one texture: 1,114,112 pixels in the scope, shift 1 (each face alone: shift 0)"""
    B, nver, H, W = 17, 12, 256, 256
    assert geom(B, nver, H, W, 1)["shift"] == 1 and geom(B, nver, H, W, B)["shift"] == 0
    got, M = run_case(scene(B, nver, H, W), 1)
    assert M.shift == 1
    assert_model_bits(got, M)
    assert np.count_nonzero(got) > 0


def test_shift_above_zero_per_face_scope():
    B, nver, H, W = 1, 12, 1025, 1024
    assert geom(B, nver, H, W, 1)["shift"] == 1
    got, M = run_case(scene(B, nver, H, W), 1)
    assert M.shift == 1
    assert_model_bits(got, M)
    assert np.count_nonzero(got) > 0


def test_shared_texture_is_the_whole_batch_and_ignores_the_order_of_the_faces():
    B, nver, H, W = 17, 20000, 33, 31
    sc = scene(B, nver, H, W)
    assert geom(B, nver, H, W, 1)["slices"] < B                              # faces do share slices: the grouping matters
    got, M = run_case(sc, 1)
    assert_model_bits(got, M)
    perm = np.random.RandomState(5).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    again = tbwd(_t(sc["g"][perm]), _t(sc["tri"]), _t(sc["tind"][perm]), nver, H, W, 1).cpu().numpy()
    assert_bits_equal(again, got, "faces permuted")
    # and it is NOT the fp32 sum of the per-face results in general (one rounding, not B)
    per_face = tbwd(_t(sc["g"]), _t(sc["tri"]), _t(sc["tind"]), nver, H, W, B).cpu().numpy()
    np.testing.assert_allclose(per_face.astype(np.float64).sum(0), got[0], rtol=0, atol=1e-4 * np.abs(per_face).sum(0).max())


# ---- edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_out_of_range_ids_and_indices_contribute_nothing(shared):
    """a vertex id of nver, one of -1, a tri_ind beyond a shortened triangle list, and tri_ind NaN, +-Inf, negative: skipped"""
    sc = scene(3, 12, 33, 31)
    tb = 1 if shared else 3
    tri = sc["tri"].copy()
    present = sorted({int(t) for t in sc["tind"][sc["tind"] >= 0]})
    used, last = present[:-1], present[-1]                                    # the highest winning triangle falls off the list
    assert len(used) >= 2
    tri[1, used[0]] = sc["nver"]
    tri[2, used[1]] = -1
    short = np.ascontiguousarray(tri[:, :last])
    tind = sc["tind"].copy()
    cov = np.flatnonzero(tind[0] >= 0)
    tind[0, cov[0:5]] = (np.nan, np.inf, -np.inf, -3.0, 3e9)
    tind[0, cov[5]] += 0.75                                                   # truncates to the same triangle
    M = RT.model(sc["g"], short, tind, 12, 33, 31, tb)
    full = RT.model(sc["g"], sc["tri"], sc["tind"], 12, 33, 31, tb)
    assert not np.array_equal(M.bits, full.bits)
    got = tbwd(_t(sc["g"]), _t(short), _t(tind), 12, 33, 31, tb).cpu().numpy()
    assert_model_bits(got, M)


def test_a_triangle_naming_one_vertex_three_times():
    """tri_ind is the forward's; the triangle list handed to the backward then names one vertex three times for triangle 0: that
    vertex collects three terms a pixel"""
    sc = scene(3, 12, 33, 31)
    tri = sc["tri"].copy()
    tri[:, 0] = 5
    n0 = int((sc["tind"] == 0).sum())
    assert n0 > 0
    for tb in (3, 1):
        got, M = run_case(sc, tb, tri=tri)
        assert_model_bits(got, M)
        _, n, _ = RT.exact(sc["g"], tri, sc["tind"], 12, 33, 31, tb)
        assert int(n[:, 0, 5].sum()) >= 3 * n0


@pytest.mark.parametrize("shared", [False, True])
def test_zero_gradient_and_all_background_give_plus_zero(shared):
    sc = scene(3, 12, 33, 31)
    tb = 1 if shared else 3
    g0 = np.zeros_like(sc["g"])
    g0[0] = -0.0
    got = tbwd(_t(g0), _t(sc["tri"]), _t(sc["tind"]), 12, 33, 31, tb)
    assert not bool(_bits(got).any())
    tind = sc["tind"].copy()
    tind[1] = -1                                                              # one face all background, gradients non-zero
    got = tbwd(_t(sc["g"]), _t(sc["tri"]), _t(tind), 12, 33, 31, tb)
    assert bool(got[0].abs().sum() > 0)
    if not shared:
        assert not bool(_bits(got[1]).any())
    got = tbwd(_t(sc["g"]), _t(sc["tri"]), _t(np.full_like(tind, -1)), 12, 33, 31, tb)
    assert not bool(_bits(got).any())


@pytest.mark.parametrize("shared", [False, True])
def test_all_subnormal_terms(shared):
    sc = scene(3, 12, 33, 31)
    tb = 1 if shared else 3
    g = (sc["g"].astype(np.float64) * 1e-40).astype(np.float32)
    assert np.abs(g).max() < 1.1754944e-38 and np.count_nonzero(g) > g.size // 2
    got, M = run_case(sc, tb, g=g)
    assert np.all(M.e == -127)
    assert_model_bits(got, M)
    assert np.count_nonzero(got) > 0


@pytest.mark.parametrize("B,nver", [(3, 12), (8, 20000)])
def test_accumulate_and_stride_7(B, nver):
    H, W = 33, 31
    sc = scene(B, nver, H, W)
    g, tri, ti = _t(sc["g"]), _t(sc["tri"]), _t(sc["tind"])
    g7 = torch.full((B, H * W, 7), float("nan"), device=DEV)
    g7[:, :, 1:4] = g
    for tb in (B, 1):
        dense = tbwd(g, tri, ti, nver, H, W, tb)
        assert _same(tbwd(g7, tri, ti, nver, H, W, tb, stride=7, offset=1), dense)   # channels 1-3 of a net_input gradient
        old = torch.randn((tb, 3, nver), generator=torch.Generator().manual_seed(4)).to(DEV)
        both = old.clone()
        tbwd(g, tri, ti, nver, H, W, tb, out=both, accumulate=1)
        assert _same(both, old + dense)                                       # one fp32 add per element
        untouched = dense == 0
        assert bool(untouched.any()) or nver == 12
        assert bool((_bits(both)[untouched] == _bits(old)[untouched]).all())
        both7 = old.clone()
        tbwd(g7, tri, ti, nver, H, W, tb, out=both7, accumulate=1, stride=7, offset=1)
        assert _same(both7, both)


def test_two_runs_and_two_streams_are_bit_identical():
    B, nver, H, W = 17, 20000, 40, 40
    sc = scene(B, nver, H, W)
    g, tri, ti = _t(sc["g"]), _t(sc["tri"]), _t(sc["tind"])
    for tb in (B, 1):
        first = tbwd(g, tri, ti, nver, H, W, tb)
        second = tbwd(g, tri, ti, nver, H, W, tb)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
        outs = []
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs.append(tbwd(g, tri, ti, nver, H, W, tb))
        torch.cuda.synchronize()
        assert _same(first, second) and _same(outs[0], first) and _same(outs[1], first)


def test_an_inf_and_a_nan_gradient_reach_exactly_their_triangles():
    B, nver, H, W = 3, 20000, 33, 31
    sc = scene(B, nver, H, W)
    g = sc["g"].copy()
    cov = np.flatnonzero(sc["tind"][1] >= 0)
    px_inf, px_nan = int(cov[3]), int(cov[-2])
    g[1, px_inf, 0] = np.inf
    g[1, px_nan, 2] = np.nan
    ids_inf = {int(sc["tri"][k, int(sc["tind"][1, px_inf])]) for k in range(3)}
    ids_nan = {int(sc["tri"][k, int(sc["tind"][1, px_nan])]) for k in range(3)}
    # per face: faces 0 and 2 keep their bits, face 1 has the classes the definition names
    got, M = run_case(sc, B, g=g)
    assert list(M.bad) == [False, True, False]
    clean = RT.model(sc["g"], sc["tri"], sc["tind"], nver, H, W, B)
    for b in (0, 2):
        assert_bits_equal(got[b], clean.value()[b], "face %d" % b)
    RT.assert_bad_scope(got[1], M, 1)
    assert set(np.flatnonzero(~np.isfinite(got[1][0])).tolist()) == ids_inf and np.all(got[1][0][list(ids_inf)] == np.inf)
    assert set(np.flatnonzero(np.isnan(got[1][2])).tolist()) == ids_nan
    assert np.isfinite(got[1][1]).all() and np.count_nonzero(got[1][1]) > 0
    # shared: the whole batch is one scope
    got, M = run_case(sc, 1, g=g)
    assert list(M.bad) == [True]
    RT.assert_bad_scope(got[0], M, 0)
    assert set(np.flatnonzero(~np.isfinite(got[0][0])).tolist()) == ids_inf
    assert set(np.flatnonzero(~np.isfinite(got[0][2])).tolist()) == ids_nan


# ---- fr_sfs_intensity_backward_tex ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 16])
def test_sfs_backward_tex_is_float64_on_the_state(B):
    h, L = _h(), _h().lib()
    H, W = 9, 13
    gen = torch.Generator().manual_seed(20 + B)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)                         # noqa: E731
    n = unit(torch.randn((B, H, W, 3), generator=gen)).to(DEV)
    n2 = unit(torch.randn((B, H, W, 3), generator=gen)).to(DEV)
    a = torch.rand((B, H, W, 1), generator=gen).to(DEV)
    a2 = torch.rand((B, H, W, 1), generator=gen).to(DEV)
    im = torch.rand((B, H, W, 1), generator=gen).to(DEV)
    g = torch.randn((B, H, W, 1), generator=gen).to(DEV)
    nst = L.fr_sfs_state_bytes(H, W)
    state = torch.empty((nst // 8,), dtype=torch.float64, device=DEV)
    inten = torch.empty((B, H, W, 1), device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.fr_sfs_intensity_forward(h.ptr(a), h.ptr(n), h.ptr(im), h.ptr(a2), h.ptr(n2), B, H, W, 1e-6, h.ptr(inten), h.ptr(state),
                                      nst, st) == 0
    nan = lambda c: torch.full((B, H, W, c), float("nan"), device=DEV)        # noqa: E731
    gn0, gn20 = nan(3), nan(3)
    assert L.fr_sfs_intensity_backward(h.ptr(g), h.ptr(a), h.ptr(im), h.ptr(a2), h.ptr(n2), h.ptr(state), nst, B, H, W, h.ptr(gn0),
                                       h.ptr(gn20), st) == 0
    gn, gn2, ga = nan(3), nan(3), nan(1)
    assert L.fr_sfs_intensity_backward_tex(h.ptr(g), h.ptr(a), h.ptr(im), h.ptr(a2), h.ptr(n2), h.ptr(state), nst, B, H, W,
                                           h.ptr(gn), h.ptr(gn2), h.ptr(ga), st) == 0
    ga_only = nan(1)
    assert L.fr_sfs_intensity_backward_tex(h.ptr(g), h.ptr(a), h.ptr(im), h.ptr(a2), h.ptr(n2), h.ptr(state), nst, B, H, W, None,
                                           None, h.ptr(ga_only), st) == 0
    torch.cuda.synchronize()
    assert _same(gn, gn0) and _same(gn2, gn20) and _same(ga_only, ga)
    l = state.cpu().numpy().reshape(10, H, W)[6:9]                            # state planes 6-8
    N2 = n2.cpu().numpy().astype(np.float64)
    d = (l[0] * N2[..., 0] + l[1] * N2[..., 1]) + l[2] * N2[..., 2]           # [B,H,W], each operation rounded on its own
    want = (g.cpu().numpy().astype(np.float64)[..., 0] * d).astype(np.float32)
    assert_bits_equal(ga.cpu().numpy()[..., 0], want, "grad_abedo_new")
    assert np.count_nonzero(want) > want.size // 2


# ---- Python surface ------------------------------------------------------------------------------------------------------------------------
class _Py:
    pass


@pytest.fixture(scope="module")
def py(small_assets):
    """the small mesh decoded at 40 x 40, four faces; random weights for every output"""
    s = _Py()
    s.B, s.S = 4, 40
    A = small_assets
    s.A = A
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
    s.wt = torch.randn((s.B, s.S, s.S, 3), generator=gen).to(DEV)
    s.wn = torch.randn((s.B, s.S, s.S, 3), generator=gen).to(DEV)
    s.wd = torch.randn((s.B, s.S, s.S, 1), generator=gen).to(DEV)
    s.im = torch.rand((s.B, s.S, s.S, 1), generator=gen).to(DEV)
    s.texB = torch.rand((s.B, 3, s.nver), generator=gen).to(DEV)
    s.image = torch.zeros((s.B, s.S, s.S, 3), device=DEV)
    return s


def test_render_depth_texture_grad_flag(py):
    o, s = ops(), py
    tri = s.net.tri

    def run(tex, flag, normal=False, use=("tex",)):
        t = tex.clone().requires_grad_(True)
        V = s.V.clone().requires_grad_(True)
        kw = {} if flag is None else dict(texture_grad=flag)
        if normal:
            kw["normal_grad"] = True
        outs = o.render_depth(V, tri, t, s.image, **kw)
        hooked = []
        if outs[1].requires_grad:
            outs[1].register_hook(hooked.append)
        loss = 0
        if "tex" in use:
            loss = loss + (outs[1] * s.wt).sum()
        if "depth" in use:
            loss = loss + (outs[0].clamp_min(0) * s.wd).sum()
        if "normal" in use:
            loss = loss + (outs[2] * s.wn).sum()
        loss.backward()
        return [x.detach() for x in outs], t.grad, V.grad, (hooked[0] if hooked else None)

    for tex in (s.net.mu_tex, s.net.mu_tex[None], s.texB):                    # [3,N], [1,3,N], [B,3,N]
        tb = 1 if tex.dim() == 2 else int(tex.shape[0])
        outs0, tg0, vg0, _ = run(tex, None, use=("tex", "depth"))
        outsF, tgF, vgF, _ = run(tex, False, use=("tex", "depth"))
        outs1, tg1, vg1, hook = run(tex, True, use=("tex", "depth"))
        for a, b, c in zip(outs0, outsF, outs1):
            assert _same(a, b) and _same(a, c)                                # the outputs are the same bits either way
        assert tg0 is None and tgF is None                                    # off: no texture gradient
        assert _same(vg0, vgF) and _same(vg0, vg1)                            # the vertex gradient is untouched
        assert tuple(tg1.shape) == tuple(tex.shape)
        want = tbwd(hook.contiguous(), tri, outs1[3], s.nver, s.S, s.S, tb).reshape(tex.shape)
        assert _same(tg1, want) and float(tg1.abs().max()) > 0
        # together with normal_grad: both gradients, each the bits of its own flag alone
        _, tgN, vgN, hookN = run(tex, True, normal=True, use=("tex", "normal", "depth"))
        assert _same(hookN, hook) and _same(tgN, tg1)
        V = s.V.clone().requires_grad_(True)
        outsN = o.render_depth(V, tri, tex, s.image, normal_grad=True)
        ((outsN[2] * s.wn).sum() + (outsN[0].clamp_min(0) * s.wd).sum()).backward()
        assert _same(vgN, V.grad) and float(vgN[:, 0].abs().max()) > 0
    # no backward for an output nobody used: a loss on depth alone leaves the texture without a gradient
    _, tg, vg, _ = run(s.texB, True, use=("depth",))
    assert tg is None and vg is not None
    _, tg, vg, _ = run(s.texB, True, use=("tex",))
    assert tg is not None and vg is None


def test_sfs_intensity_abedo_grad_flag(py):
    o, s = ops(), py
    with torch.no_grad():
        alb, nmap = s.net.compute_abedo_image(s.V, s.net.tri, s.net.mu_tex)
    a2 = (alb * 1.1).clone().requires_grad_(True)
    with pytest.raises(ValueError):
        o.sfs_intensity(alb, nmap, s.im, a2, nmap)                            # off: the existing refusal stays
    with pytest.raises(ValueError):
        o.sfs_intensity(alb.clone().requires_grad_(True), nmap, s.im, a2, nmap, abedo_grad=True)
    I1 = o.sfs_intensity(alb, nmap, s.im, a2, nmap, rcond=1e-6, abedo_grad=True)
    I0 = o.sfs_intensity(alb, nmap, s.im, a2.detach(), nmap, rcond=1e-6)
    assert _same(I0, I1.detach())
    (I1 * s.wd).sum().backward()
    d = o.sfs_intensity(alb, nmap, s.im, torch.ones_like(alb), nmap, rcond=1e-6)   # abedo_new = 1: the intensity is fl32(d)
    np.testing.assert_allclose(a2.grad.cpu().numpy(), (s.wd * d).cpu().numpy(), rtol=3e-7, atol=0)
    assert float(a2.grad.abs().max()) > 0


def _sfs_setup(py):
    """pred / label / maps for get_loss on the fixture's faces, and a net of its own (its param_tex is replaced per run)"""
    s = py
    netm = net_mod()
    net = netm.FaceRecNet(mesh_data=s.A, batch_size=s.B, im_size=s.S, device=torch.device(DEV))
    pred = s.P.clone()
    rs = np.random.RandomState(3)
    label = _t(s.P.cpu().numpy() + rs.standard_normal(tuple(s.P.shape)).astype(np.float32) * 0.01)
    V = net.vertices_transform(pred)
    coarse = net.coarse_net_input(V, im_gray=s.im)[1].detach()
    fine = (coarse + 0.05 * torch.rand((s.B, s.S, s.S, 1), generator=torch.Generator().manual_seed(2)).to(DEV)).detach()
    return net, pred, label, V.detach(), coarse, fine


def test_get_loss_sfs_tex_grad_against_a_float64_restatement(py):
    """d spherical_harmonics_loss / d param_tex on both routes against float64 autograd of the chain
        texture_new = mu_tex + pc_tex param -> lookup (t[p1] + t[p2] + t[p3]) / 3 -> clamp_min 1e-6 -> mean over the channels
        -> intensity = abedo_new * d -> mean((intensity - im)^2)
    with d = l . n' held constant: l does not depend on param_tex on either route (it is solved from the render of the MEAN
    texture), and each route's own d is read off the route itself as its intensity for abedo_new = 1.

    The bound, derived (u = 2^-24, K = 10 coefficients, T = max |mu_tex| + sum_k |pc_tex| |param_k| the scale of the texture, n =
    B H W the pixel count of the mean):
      forward, fp32:   texture_new within (K + 2) u T; tex_img three more roundings, the clamp none, the mean three more:
                       |abedo_new - exact| <= da = (K + 8) u T
                       intensity = abedo_new d, one rounding; the residual one more; g_I = 2 r / n two more:
                       |g_I - exact| <= dg = (2 / n) (|d| da + 4 u (|I| + |im|))
      backward:        g_a = g_I d (one rounding; the fused route's d carries one more: read here as fl32(d));  the mean and the
                       lookup each divide by 3 (two roundings; the second is the 2^-24 A of the texture backward's own bound):
                       |term - exact| <= e = |d| dg / 9 + 6 u |term|
      texture_grad:    the kernel's bound  u |S| + n_v 2^(shift - 39) M  on top of the summed e of the element's terms
      param_tex.grad:  pc_tex^T texture_grad as an fp32 product of 3 N terms: 3 N u sum |pc| |texture_grad|, any order,
                       and every error above carried through |pc_tex|.
    """
    s = py
    L = pkg("nets.losses")
    net, pred, label, V, coarse, fine = _sfs_setup(py)
    B, S, N, K = s.B, s.S, s.nver, net.ndim_tex
    u = 2.0 ** -24
    p0 = net.param_tex.detach().clone()
    with torch.no_grad():
        alb, nmap = net.compute_abedo_image(V, net.tri, net.mu_tex)
        tex_new = net.mu_tex + (net.pc_tex @ p0).reshape(3, -1)
        outs = ops().render_depth(V, net.tri, tex_new, s.image)
        alb2, nmap2 = net.compute_abedo_image(V, net.tri, tex_new)
    tind = outs[3].cpu().numpy().reshape(B, S * S)
    tri = net.tri.cpu().numpy()
    covered = tind >= 0
    assert float(outs[1].cpu().numpy().reshape(B, S * S, 3)[covered].min()) > 1e-3   # the clamp is far from every covered pixel
    ids = [np.stack([RT.f2i_x86(tri[k, RT.f2i_x86(tind[b][covered[b]])]) for k in range(3)]) for b in range(B)]
    mu64, pc64 = net.mu_tex.cpu().double(), net.pc_tex.cpu().double()
    im64 = s.im.cpu().double().reshape(B, S * S)
    apc = pc64.abs().reshape(3, N, K).numpy()
    T = float((mu64.abs() + (pc64.abs() @ p0.cpu().double().abs()).reshape(3, -1)).max())
    npx = B * S * S

    for fused in (False, True):
        net.param_tex = p0.clone().requires_grad_(True)
        kw = dict(sfs_tex_grad=True, sfs_rcond=1e-6, sfs_fused=fused)
        Ls = L.get_loss(net, pred, label, s.im, V, coarse, fine, **kw)
        got = torch.autograd.grad(Ls["spherical_harmonics_loss"], net.param_tex)[0].cpu().numpy().astype(np.float64)
        assert got.shape == (K, 1) and np.isfinite(got).all() and np.count_nonzero(got) == K
        with torch.no_grad():
            d = L.spherical_harmonics_intensity(alb, nmap, s.im, torch.ones_like(alb2), nmap2, fused=fused, rcond=1e-6)
        d64 = d.cpu().double().reshape(B, S * S)
        # the restatement
        p64 = p0.cpu().double().clone().requires_grad_(True)
        t64 = mu64 + (pc64 @ p64).reshape(3, -1)
        a_new = torch.full((B, S * S), 1e-6, dtype=torch.float64)
        rows = []
        for b in range(B):
            i = torch.as_tensor(ids[b])
            img = (t64[:, i[0]] + t64[:, i[1]] + t64[:, i[2]]) / 3.0          # [3,n]
            rows.append(torch.clamp_min(img, 1e-6).mean(dim=0))
        a_cov = torch.cat(rows)
        a_new = a_new.masked_scatter(torch.as_tensor(covered), a_cov)
        I64 = a_new * d64
        loss64 = ((I64 - im64) ** 2).mean()
        want = torch.autograd.grad(loss64, p64)[0].numpy()
        np.testing.assert_allclose(float(Ls["spherical_harmonics_loss"].detach()), float(loss64.detach()), rtol=1e-4)
        # the bound
        dabs, Iabs, imabs = d64.abs().numpy(), I64.detach().abs().numpy(), im64.abs().numpy()
        da = (K + 8) * u * T
        dg = (2.0 / npx) * (dabs * da + 4 * u * (Iabs + imabs))
        term = np.abs((2.0 / npx) * (I64.detach().numpy() - im64.numpy()) * d64.numpy()) / 9.0      # |term|, every channel alike
        e = dabs * dg / 9.0 + 6 * u * term
        E = np.zeros((3, N))                                                  # summed error of each element's terms
        A = np.zeros((3, N))                                                  # sum |term|, n_v
        nv = np.zeros(N)
        for b in range(B):
            eb, tb_ = e[b][covered[b]], term[b][covered[b]]
            for k in range(3):
                np.add.at(E[0], ids[b][k], eb)
                np.add.at(A[0], ids[b][k], tb_)
                np.add.at(nv, ids[b][k], 1)
        E[1] = E[2] = E[0]
        A[1] = A[2] = A[0]
        shift = RT.shift_of(npx)
        kernel = u * A + nv[None] * 2.0 ** (shift - 39) * float(term.max() * (1 + 8 * u))
        bound = np.einsum("cvk,cv->k", apc, E + kernel) + 3 * N * u * np.einsum("cvk,cv->k", apc, A)
        err = np.abs(got[:, 0] - want[:, 0])
        print("fused=%s: d SfS / d param_tex worst error / bound = %.3g (|grad| up to %.3g)" %
              (fused, float((err / bound).max()), float(np.abs(want).max())))
        assert np.all(err <= bound), (err, bound)
        assert np.all(bound <= 1e-2 * np.abs(want).max())                     # ... and the bound says something


def test_get_loss_with_the_new_flags_off_is_unchanged(py):
    L = pkg("nets.losses")
    net, pred, label, V, coarse, fine = _sfs_setup(py)
    net.param_tex = net.param_tex.detach().clone().requires_grad_(True)
    for fused in (False, True):
        base = L.get_loss(net, pred, label, py.im, V, coarse, fine, sfs_fused=fused)
        off = L.get_loss(net, pred, label, py.im, V, coarse, fine, sfs_fused=fused, sfs_tex_grad=False)
        on = L.get_loss(net, pred, label, py.im, V, coarse, fine, sfs_fused=fused, sfs_tex_grad=True)
        for k in base:
            assert _same(base[k], off[k]) and _same(base[k], on[k]), k        # the flag changes no forward bit
        if fused:
            assert not off["total_loss"].requires_grad                        # fused, flag off: no path to param_tex at all
        else:
            # the torch route differentiates abedo_new, but the render without texture_grad hands the texture nothing
            assert torch.autograd.grad(off["total_loss"], net.param_tex, allow_unused=True)[0] is None
        assert net.param_tex.grad is None
        g = torch.autograd.grad(on["total_loss"], net.param_tex)[0]
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def _coarse_loop():
    spec = importlib.util.spec_from_file_location("_coarse_loop_example", os.path.join(ROOT, "examples", "coarse_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_learn_tex_lists_the_parameter_and_one_adam_step_moves_it(small_assets):
    netm, cn = net_mod(), pkg("nets.coarse_net")
    face = netm.FaceRecNet(mesh_data=small_assets, batch_size=2, im_size=40)
    assert inspect.signature(cn.FaceReconModel.__init__).parameters["learn_tex"].default is False   # off unless asked for
    assert not isinstance(face.param_tex, torch.nn.Parameter) and not face.param_tex.requires_grad
    # the example program: coarse_loop --small --train --sfs-fused --sfs-tex-grad, one step
    cl = _coarse_loop()
    args = cl.build_parser().parse_args(["--small", "--train", "--sfs-fused", "--sfs-tex-grad", "--batch", "2", "--im-size", "40",
                                         "--nIter", "1"])
    assert isinstance(args, argparse.Namespace) and args.sfs_tex_grad
    model, net, opt, step = cl.build_harness(args, torch.device(DEV), 0, 1, 0)
    assert "param_tex" in dict(model.named_parameters()) and model.face_net.param_tex is model.param_tex
    assert any(p is model.param_tex for g in opt.param_groups for p in g["params"])
    before = model.param_tex.detach().clone()
    _, losses = step()
    assert np.isfinite(float(losses["total_loss"]))
    assert bool(torch.isfinite(model.param_tex).all()) and not torch.equal(model.param_tex.detach(), before)
