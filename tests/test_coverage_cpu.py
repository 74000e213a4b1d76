"""CPU: the soft-coverage entry points (fr_coverage_forward / _backward and their two companions) exist, validate before any HIP
call in the order include/fr_hotpath.h states, and choose the launch geometry of the three-row owner; the float64 model of the GPU
tests (tests/ref_coverage.py) is itself held to central differences of its own forward and to cases worked out by hand."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import coverage_cases as CC
import ref_coverage as RC
import ref_normal_backward as RN

NEW = ("fr_coverage_forward", "fr_coverage_backward_workspace_bytes", "fr_coverage_backward", "fr_debug_coverage_bwd_geom")


def _L():
    return pkg("_lib").lib()


def _geom(B, nver, H, W, name="fr_debug_coverage_bwd_geom"):
    out = (ctypes.c_int * 6)()
    getattr(_L(), name)(B, nver, H, W, out)
    return list(out)


def test_symbols_exported_and_bound():
    L, lib = _L(), pkg("_lib")
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTS and name in lib.SIGNATURES
    assert "fr_coverage.hip" in lib.SOURCES
    assert lib.SIGNATURES["fr_coverage_forward"] == "i:pippiiiiipp"
    assert lib.SIGNATURES["fr_coverage_backward"] == "i:pppipppiiiiiipzp"
    assert lib.SIGNATURES["fr_coverage_backward_workspace_bytes"] == "z:iiii"
    assert lib.SIGNATURES["fr_debug_coverage_bwd_geom"] == "v:iiiiI"


def test_workspace_formula():
    f = _L().fr_coverage_backward_workspace_bytes
    assert f(2, 10, 8, 9) == 2 * 72 * 48 + 2 * 1 * 8
    assert f(3, 7, 33, 40) == 3 * 1320 * 48 + 3 * 2 * 8
    assert f(0, 10, 8, 9) == 0 and f(2, 10, 0, 9) == 0 and f(2, 10, 8, 0) == 0 and f(-1, 10, 8, 9) == 0
    g = _L().fr_depth_interp_backward_workspace_bytes
    for shape in ((1, 480, 64, 64), (8, 53215, 200, 200)):
        assert f(*shape) == g(*shape)


def _gpu_visible():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_visible(), reason="the made-up pointers of this test must never reach a launch: CPU machines only")
def test_validates_before_any_hip_call():
    """The header's order: (1) sizes / accumulate / pitch, (2) the empty batch or image, (3) pointers, (4) the workspace -- the
    order and the codes of fr_depth_interp_*."""
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    B, nver, ntri, H, W = 2, 10, 5, 8, 9
    need = L.fr_coverage_backward_workspace_bytes(B, nver, H, W)

    def bwd(g=one, c=one, v=one, vp=nver, tri=one, ti=one, vg=one, B=B, nver=nver, ntri=ntri, H=H, W=W, acc=0, ws=al, nb=need):
        return L.fr_coverage_backward(g, c, v, vp, tri, ti, vg, B, nver, ntri, H, W, acc, ws, nb, nul)

    def fwd(v=one, vp=nver, tri=one, ti=one, B=B, nver=nver, ntri=ntri, H=H, W=W, d=one):
        return L.fr_coverage_forward(v, vp, tri, ti, B, nver, ntri, H, W, d, nul)
    # (1)
    for k in ("B", "nver", "ntri", "H", "W"):
        assert bwd(**{k: -1}) == -1 and fwd(**{k: -1}) == -1, k
    assert bwd(acc=2) == -1 and bwd(acc=-1) == -1
    assert bwd(vp=nver - 1) == -1 and fwd(vp=nver - 1) == -1
    # (1) comes before (2): a scalar error is reported for an empty batch too
    assert bwd(B=0, acc=2) == -1 and bwd(H=0, vp=nver - 1) == -1 and fwd(B=0, vp=nver - 1) == -1 and fwd(W=0, H=-1) == -1
    # (2) comes before (3) and (4): nothing is looked at
    for empty in (dict(B=0), dict(H=0), dict(W=0)):
        assert bwd(g=nul, c=nul, v=nul, tri=nul, ti=nul, vg=nul, ws=nul, nb=0, **empty) == 0, empty
        assert fwd(v=nul, tri=nul, ti=nul, d=nul, **empty) == 0, empty
    assert bwd(nver=0, vp=0, vg=nul, ws=nul, nb=0) == 0                      # an empty vertex_grad: nothing to write
    # (3)
    for k in ("g", "c", "v", "tri", "ti", "vg"):
        assert bwd(**{k: nul}) == -1, k
    for k in ("v", "tri", "ti", "d"):
        assert fwd(**{k: nul}) == -1, k
    # (3) comes before (4)
    assert bwd(g=nul, ws=nul) == -1 and bwd(vg=nul, nb=0) == -1 and bwd(c=nul, nb=0) == -1
    assert bwd(ntri=1 << 24, ws=nul) == -4 and fwd(ntri=1 << 24) == -4       # float-stored ids stop being exact
    # (4)
    assert bwd(nb=need - 1) == -2 and bwd(ws=nul) == -2
    assert bwd(ws=ctypes.c_void_p(4096 + 8)) == -2                           # not 16-byte aligned
    assert bwd(vp=nver + 22, acc=1, nb=need - 1) == -2                       # every legal variant gets as far as the workspace


@pytest.mark.parametrize("B", [1, 3, 8, 64])
@pytest.mark.parametrize("nver", [1, 480, 6656, 6657, 53215])
def test_geometry_is_the_three_row_owners(B, nver):
    """the hook equals rows3_geom: what the interpolated-depth and the normal backward report for the same shape"""
    for H, W in ((8, 9), (33, 40), (200, 200), (1100, 1000)):
        splits, rng, shift, chunks, lds, xcd = g = _geom(B, nver, H, W)
        assert splits >= 1 and splits * rng >= nver and (splits - 1) * rng < nver
        assert 3 * 8 * rng <= lds <= 160 * 1024
        assert shift == RN.shift_of(H * W) and chunks == (H * W + 1023) // 1024
        assert xcd == (1 if B % 8 == 0 else 0)
        assert g == _geom(B, nver, H, W, "fr_debug_depth_interp_bwd_geom")
        assert g == _geom(B, nver, H, W, "fr_debug_render_normal_bwd_geom")
    assert _geom(0, nver, 5, 6) == [0] * 6 and _geom(B, nver, 0, 6) == [0] * 6 and _geom(B, 0, 5, 6) == [0] * 6


# ---- the model against central differences of its own forward ---------------------------------------------------------------------
S_IMG = 32


@pytest.fixture(scope="module")
def faces(oracle, small_assets):
    """make_small_assets decoded at a pose that faces the camera, two faces of different shape and expression at 32 x 32, rendered
    by the reference model's own forward: V [2,3,480], tri, tind [2,32*32]."""
    A = small_assets
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    rs = np.random.RandomState(4)
    P = np.zeros((2, 7 + ns + ne), np.float32)
    P[:, 3:5] = S_IMG / 2
    P[:, 6] = (1.5e-4, 1.8e-4)
    P[:, 7:7 + ns] = rs.uniform(0, 1e4, (2, ns))
    P[:, 7 + ns:] = rs.uniform(-1.5, 1.5, (2, ne))
    V = oracle.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], S_IMG)
    tind = oracle.render_depth(V, A["tri"], A["vertex"], S_IMG, S_IMG)[3].reshape(2, -1)
    return V, A["tri"], tind


def test_model_backward_agrees_with_central_differences(faces):
    V, tri, tind = faces
    H = W = S_IMG
    ok = tind >= 0
    assert ok.any() and not ok.all()
    V64 = V.astype(np.float64)
    rs = np.random.RandomState(7)
    g = rs.standard_normal((2, H * W))
    cov = RC.forward64(V64, tri, tind, H, W)
    soft = (cov > 0) & (cov < 1)
    assert soft.sum() > 40
    an = RC.grad64(g, cov, V64, tri, tind, H, W)
    assert np.abs(an[:, 0]).max() > 0 and np.abs(an[:, 1]).max() > 0 and not an[:, 2].any()
    h = 1e-6
    for trial in range(5):
        dV = rs.standard_normal(V64.shape)
        fd = ((g * RC.forward64(V64 + h * dV, tri, tind, H, W)).sum() - (g * RC.forward64(V64 - h * dV, tri, tind, H, W)).sum()) / (2 * h)
        dd = float((an * dV).sum())
        scale = float(np.abs(an * dV).sum())
        print("direction %d: fd %.9e analytic %.9e |difference| %.2e bound %.2e" % (trial, fd, dd, abs(fd - dd), 1e-6 * scale))
        assert abs(dd) > 1e-3 * scale
        assert abs(fd - dd) <= 1e-6 * scale


def test_forward_model_properties(faces):
    V, tri, tind = faces
    H = W = S_IMG
    cov = RC.forward(V, tri, tind, H, W).reshape(2, H, W)
    assert cov.dtype == np.float32 and cov.min() >= 0 and cov.max() <= 1
    ok = (tind >= 0).reshape(2, H, W)
    pad = np.pad(ok, ((0, 0), (1, 1), (1, 1)), mode="edge")
    same = (pad[:, 1:-1, :-2] == ok) & (pad[:, 1:-1, 2:] == ok) & (pad[:, :-2, 1:-1] == ok) & (pad[:, 2:, 1:-1] == ok)
    assert np.all(cov[same & ok] == 1) and np.all(cov[same & ~ok].view(np.uint32) == 0)
    assert ((cov > 0) & (cov < 1)).sum() > 40
    # the soft mask's area stays near the hard mask's
    assert abs(float(cov.sum()) - float(ok.sum())) < 0.15 * ok.sum()


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def _terms(case, g):
    V, tri, tind, H, W = case
    cov = RC.forward(V, tri, tind, H, W).reshape(-1)
    return RC.terms(np.asarray(g, np.float32).reshape(-1), cov, V[0], tri, tind[0], V.shape[2], H, W)


def _one_hot(H, W, j, i):
    g = np.zeros(H * W, np.float32)
    g[j * W + i] = 1
    return g


def test_a_lone_pixel_sized_triangle():
    """coverage_cases.lone_triangle: s = 0.25 to the left, 0.625 up, 0.875 to the right and down, every step exact"""
    case = V, tri, tind, H, W = CC.lone_triangle()
    P = ((1.75, 1.375), (3.5, 1.375), (1.75, 3.125))
    assert RC.pair(P, (2, 2), (1, 2))[:2] == (2, 0.25)
    assert RC.pair(P, (2, 2), (3, 2))[:2] == (1, 0.875)
    assert RC.pair(P, (2, 2), (2, 1))[:2] == (0, 0.625)
    assert RC.pair(P, (2, 2), (2, 3))[:2] == (1, 0.875)
    cov = RC.forward(V, tri, tind, H, W).reshape(H, W)
    want = np.zeros((H, W), np.float32)
    want[2, 2] = 0.75                                                         # the left pair leaves 0.5 - 0.25 of c uncovered
    want[1, 2] = 0.125                                                        # up:    0.625 - 0.5
    want[2, 3] = 0.375                                                        # right: 0.875 - 0.5
    want[3, 2] = 0.375                                                        # down
    assert np.array_equal(cov.view(np.uint32), want.view(np.uint32))          # (the left neighbour: s < 0.5, exactly +0)
    ids, T, _, px = _terms(case, _one_hot(H, W, 2, 2))                        # cov(c) = 0.5 + s_left, s_left = 2 - x0
    assert ids.T.tolist() == [[0, 1, 2]] and T.shape == (1, 3, 3) and px.tolist() == [12]
    assert abs(T[0, :, 0].sum() + 1) < 1e-15 and abs(T[0, :, 1].sum()) < 1e-15 and not T[0, :, 2].any()
    assert T[0, 1, 0] == 0 and T[0, 1, 1] == 0                                # edge (P3, P1): P2 does not move it
    np.testing.assert_allclose(T[0, :, 0], [-1.125 / 1.75, 0, -0.625 / 1.75], rtol=1e-15)
    ids, T, _, _ = _terms(case, _one_hot(H, W, 1, 2))                         # cov(up) = s_up - 0.5, s_up = 2 - y0
    assert abs(T[0, :, 1].sum() + 1) < 1e-15 and abs(T[0, :, 0].sum()) < 1e-15 and T[0, 2, 1] == 0
    ids, T, _, _ = _terms(case, _one_hot(H, W, 2, 3))                         # cov(right) = x0 + y0 + L - 4.5: a shift in x or in y adds 1
    assert abs(T[0, :, 0].sum() - 1) < 1e-15 and abs(T[0, :, 1].sum() - 1) < 1e-15 and T[0, 0, 0] == 0 and T[0, 0, 1] == 0
    ids, T, _, _ = _terms(case, _one_hot(H, W, 2, 1))                         # the left neighbour: s < 0.5, it receives nothing
    assert T.shape == (0, 3, 3)


@pytest.mark.parametrize("xb,inside,outside", [(3.25, 0.75, 0.0), (3.75, 1.0, 0.25)])
def test_a_straight_vertical_border(xb, inside, outside):
    """coverage_cases.vertical_border: s = xb - 3 for every pair ((3, y), (4, y)) -- each side of 0.5 once.  The face covers
    xb + 0.5 of every row."""
    V, tri, tind, H, W = CC.vertical_border(xb)
    pr = RC.pair(((xb, -10.0), (xb, 20.0), (-30.0, 5.0)), (3, 1), (4, 1))
    assert pr[:2] == (0, xb - 3) and pr[4] == 1.0
    cov = RC.forward(V, tri, tind, H, W).reshape(H, W)
    want = np.zeros((H, W), np.float32)
    want[:, :3] = 1
    want[:, 3] = inside
    want[:, 4] = outside
    assert np.array_equal(cov.view(np.uint32), want.view(np.uint32))
    assert np.all(cov.sum(1) == np.float32(xb + 0.5))
    g = np.random.RandomState(1).standard_normal((1, H * W)).astype(np.float32)
    R = RC.model(g, cov, V, tri, tind, H, W)
    dense = R.dense(0)
    soft_col = 3 if xb < 3.5 else 4                                           # d cov / d xb = 1 on the soft pixel of every row
    np.testing.assert_allclose(dense[0, 0] + dense[0, 1], g.reshape(H, W)[:, soft_col].astype(np.float64).sum(), rtol=1e-6)
    assert dense[0, 2] == 0 and not dense[2].any()
    assert sorted(R.records[0].tolist()) == [y * W + 3 for y in range(H)]


def test_inert_and_clamped_pairs_of_the_model():
    ones = np.ones(64, np.float32)
    # a zero-area triangle: inert, the border stays hard
    case = V, tri, tind, H, W = CC.zero_area()
    assert RC.pair(((1.0, 1.0), (2.0, 2.0), (3.0, 3.0)), (1, 1), (2, 1)) is None
    assert RC.forward(V, tri, tind, H, W).reshape(-1).tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert len(_terms(case, ones[:9])[3]) == 0
    # pixels placed outside their triangle: the border x = 2.75 lies on the near side of column 3, s = -0.25, s^ = 0: half of
    # each of those pixels is given up, nothing is added beyond, and nothing moves with the vertices
    case = V, tri, tind, H, W = CC.vertical_border(2.75)
    assert RC.pair(((2.75, -10.0), (2.75, 20.0), (-30.0, 5.0)), (3, 1), (4, 1))[:2] == (0, -0.25)
    cov = RC.forward(V, tri, tind, H, W).reshape(H, W)
    assert np.all(cov[:, :3] == 1) and np.all(cov[:, 3] == 0.5) and np.all(cov[:, 4:].view(np.uint32) == 0)
    assert len(_terms(case, ones[:H * W])[3]) == 0
    # four slivers around one background pixel: it clamps at 1 and passes no gradient back
    case = V, tri, tind, H, W = CC.four_slivers()
    for t, (c, _) in enumerate((((1, 2), 0), ((3, 2), 0), ((2, 1), 0), ((2, 3), 0))):
        P = tuple((float(V[0, 0, 3 * t + k]), float(V[0, 1, 3 * t + k])) for k in range(3))
        assert 0.8 < RC.pair(P, c, (2, 2))[1] < 0.95, t
    cov = RC.forward(V, tri, tind, H, W).reshape(H, W)
    assert cov[2, 2] == 1 and ((cov > 0) & (cov < 1)).any()
    assert len(_terms(case, _one_hot(H, W, 2, 2))[3]) == 0 and len(_terms(case, ones[:25])[3]) == 4
    # a tiny triangle around one centre: that pixel clamps at 0 and passes no gradient back
    case = V, tri, tind, H, W = CC.tiny_triangle()
    cov = RC.forward(V, tri, tind, H, W).reshape(-1)
    assert not cov.view(np.uint32).any()
    assert len(_terms(case, ones[:25])[3]) == 0
