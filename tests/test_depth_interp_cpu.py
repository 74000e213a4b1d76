"""CPU: the interpolated-depth entry points (fr_depth_interp_forward / _backward and their two companions) exist, validate before
any HIP call in the order include/fr_hotpath.h states, and choose a launch geometry that fits the LDS; the float64 model of the GPU
tests (tests/ref_depth_interp.py) is itself held to torch float64 autograd over a gather-based restatement of the interpolation,
and to the plane it must reproduce."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import ref_depth_interp as RD
import ref_normal_backward as RN

NEW = ("fr_depth_interp_forward", "fr_depth_interp_backward_workspace_bytes", "fr_depth_interp_backward",
       "fr_debug_depth_interp_bwd_geom")


def _L():
    return pkg("_lib").lib()


def _geom(B, nver, H, W, name="fr_debug_depth_interp_bwd_geom"):
    out = (ctypes.c_int * 6)()
    getattr(_L(), name)(B, nver, H, W, out)
    return list(out)


def test_symbols_exported_and_bound():
    L, lib = _L(), pkg("_lib")
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTS and name in lib.SIGNATURES
    assert lib.SIGNATURES["fr_depth_interp_forward"] == "i:pippiiiiipp"
    assert lib.SIGNATURES["fr_depth_interp_backward"] == "i:ppipppiiiiiipzp"
    assert lib.SIGNATURES["fr_depth_interp_backward_workspace_bytes"] == "z:iiii"
    assert lib.SIGNATURES["fr_debug_depth_interp_bwd_geom"] == "v:iiiiI"
    assert b"fr_hotpath 0.4 " in L.fr_version()


def test_workspace_formula():
    f = _L().fr_depth_interp_backward_workspace_bytes
    assert f(2, 10, 8, 9) == 2 * 72 * 48 + 2 * 1 * 8
    assert f(3, 7, 33, 40) == 3 * 1320 * 48 + 3 * 2 * 8
    assert f(0, 10, 8, 9) == 0 and f(2, 10, 0, 9) == 0 and f(2, 10, 8, 0) == 0 and f(-1, 10, 8, 9) == 0


def _gpu_visible():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_visible(), reason="the made-up pointers of this test must never reach a launch: CPU machines only")
def test_validates_before_any_hip_call():
    """The header's order: (1) sizes / accumulate / pitch, (2) the empty batch or image, (3) pointers, (4) the workspace."""
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    B, nver, ntri, H, W = 2, 10, 5, 8, 9
    need = L.fr_depth_interp_backward_workspace_bytes(B, nver, H, W)

    def bwd(g=one, v=one, vp=nver, tri=one, ti=one, vg=one, B=B, nver=nver, ntri=ntri, H=H, W=W, acc=0, ws=al, nb=need):
        return L.fr_depth_interp_backward(g, v, vp, tri, ti, vg, B, nver, ntri, H, W, acc, ws, nb, nul)

    def fwd(v=one, vp=nver, tri=one, ti=one, B=B, nver=nver, ntri=ntri, H=H, W=W, d=one):
        return L.fr_depth_interp_forward(v, vp, tri, ti, B, nver, ntri, H, W, d, nul)
    # (1)
    for k in ("B", "nver", "ntri", "H", "W"):
        assert bwd(**{k: -1}) == -1 and fwd(**{k: -1}) == -1, k
    assert bwd(acc=2) == -1 and bwd(acc=-1) == -1
    assert bwd(vp=nver - 1) == -1 and fwd(vp=nver - 1) == -1
    # (1) comes before (2): a scalar error is reported for an empty batch too
    assert bwd(B=0, acc=2) == -1 and bwd(H=0, vp=nver - 1) == -1 and fwd(B=0, vp=nver - 1) == -1 and fwd(W=0, H=-1) == -1
    # (2) comes before (3) and (4): nothing is looked at
    for empty in (dict(B=0), dict(H=0), dict(W=0)):
        assert bwd(g=nul, v=nul, tri=nul, ti=nul, vg=nul, ws=nul, nb=0, **empty) == 0, empty
        assert fwd(v=nul, tri=nul, ti=nul, d=nul, **empty) == 0, empty
    assert bwd(nver=0, vp=0, vg=nul, ws=nul, nb=0) == 0                      # an empty vertex_grad: nothing to write
    # (3)
    for k in ("g", "v", "tri", "ti", "vg"):
        assert bwd(**{k: nul}) == -1, k
    for k in ("v", "tri", "ti", "d"):
        assert fwd(**{k: nul}) == -1, k
    # (3) comes before (4)
    assert bwd(g=nul, ws=nul) == -1 and bwd(vg=nul, nb=0) == -1
    assert bwd(ntri=1 << 24, ws=nul) == -4 and fwd(ntri=1 << 24) == -4       # float-stored ids stop being exact
    # (4)
    assert bwd(nb=need - 1) == -2 and bwd(ws=nul) == -2
    assert bwd(ws=ctypes.c_void_p(4096 + 8)) == -2                           # not 16-byte aligned
    assert bwd(vp=nver + 22, acc=1, nb=need - 1) == -2                       # every legal variant gets as far as the workspace


@pytest.mark.parametrize("B", [1, 3, 8, 64])
@pytest.mark.parametrize("nver", [1, 480, 6656, 6657, 53215])
def test_geometry_fits_the_lds(B, nver):
    for H, W in ((8, 9), (33, 40), (200, 200), (1100, 1000)):
        splits, rng, shift, chunks, lds, xcd = g = _geom(B, nver, H, W)
        assert splits >= 1 and splits * rng >= nver and (splits - 1) * rng < nver
        assert 3 * 8 * rng <= lds <= 160 * 1024
        assert shift == RN.shift_of(H * W) and chunks == (H * W + 1023) // 1024
        assert xcd == (1 if B % 8 == 0 else 0)
        assert g == _geom(B, nver, H, W, "fr_debug_render_normal_bwd_geom")   # the same owners as the normal backward
    assert _geom(0, nver, 5, 6) == [0] * 6 and _geom(B, nver, 0, 6) == [0] * 6 and _geom(B, 0, 5, 6) == [0] * 6


def test_a_face_can_have_two_owners():
    assert _geom(64, 53215, 200, 200)[0] >= 2 and _geom(3, 480, 33, 40)[0] >= 2


# ---- the model against torch float64 autograd -------------------------------------------------------------------------------
S_IMG = 64


@pytest.fixture(scope="module")
def faces(oracle, small_assets):
    """make_small_assets decoded at a pose that faces the camera (all three angles 0), two faces of different shape and
    expression, rendered by the reference model's own forward: V [2,3,480], tri, tind [2,64*64]."""
    A = small_assets
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    rs = np.random.RandomState(4)
    P = np.zeros((2, 7 + ns + ne), np.float32)
    P[:, 3:5] = S_IMG / 2
    P[:, 6] = (3.0e-4, 3.6e-4)
    P[:, 7:7 + ns] = rs.uniform(0, 1e4, (2, ns))
    P[:, 7 + ns:] = rs.uniform(-1.5, 1.5, (2, ne))
    V = oracle.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], S_IMG)
    tind = oracle.render_depth(V, A["tri"], A["vertex"], S_IMG, S_IMG)[3].reshape(2, -1)
    return V, A["tri"], tind


def test_model_agrees_with_float64_autograd(faces):
    V, tri, tind = faces
    nver = V.shape[2]
    covered = int((tind >= 0).sum())
    assert covered > 1500
    kept = tind.copy()
    for b in range(2):                                                       # triangles with den >= 1e-3 dot00 dot11 only
        px, ids = RN.contributing(tri, tind[b], nver)
        q = RD.weights(V[b], ids, px, S_IMG)
        thin = q["den"] < 1e-3 * q["dot00"] * q["dot11"]
        kept[b, px[thin]] = -1
    dropped = covered - int((kept >= 0).sum())
    assert dropped <= 0.05 * covered, (dropped, covered)
    g = np.random.RandomState(5).standard_normal((2, S_IMG * S_IMG)).astype(np.float32)
    got, big = RD.sums64(g, V, tri, kept, S_IMG, S_IMG)
    want = RD.torch_grad(g, V, tri, kept, S_IMG, S_IMG)
    assert np.all(np.isfinite(want)) and big > 0
    assert np.abs(want[:, 0]).max() > 0 and np.abs(want[:, 1]).max() > 0 and np.abs(want[:, 2]).max() > 0
    err = float(np.abs(got - want).max())
    print("model against autograd: worst |difference| = %.3e of the largest |term| %.3e" % (err / big, big))
    assert err <= 1e-10 * big


def test_the_z_row_sums_to_the_gradient_and_a_shift_moves_nothing(faces):
    """Two identities of the exact derivative the terms must keep to rounding: the weights sum to 1, so a pixel's three z terms
    sum to its gradient; and the depth at a pixel does not change when the triangle and the pixel move together, while moving
    the triangle alone by d changes it by -A.d -- so each pixel's x (y) terms sum to -G A."""
    V, tri, tind = faces
    g = np.random.RandomState(6).standard_normal(S_IMG * S_IMG).astype(np.float32)
    px, ids = RN.contributing(tri, tind[0], V.shape[2])
    _, T64, _ = RD.terms(g, V[0], tri, tind[0], V.shape[2], S_IMG)
    G = g[px].astype(np.float64)
    np.testing.assert_allclose(T64[:, :, 2].sum(1), G, rtol=1e-12, atol=0)
    q = RD.weights(V[0], ids, px, S_IMG)
    assert not q["flat"].any()
    h = 2.0 ** -10
    for c in range(2):
        Vs = V[0].astype(np.float64)
        Vs[c] += h                                                           # (exact: the coordinates are below 64)
        moved = RD.weights(Vs.astype(np.float32), ids, px, S_IMG)
        assert np.array_equal(Vs.astype(np.float32).astype(np.float64), Vs)
        d0 = (q["w"] * q["z"]).sum(0)
        d1 = (moved["w"] * moved["z"]).sum(0)
        slope = (d1 - d0) / h                                                # = -A_c: the plane is linear, the quotient exact up to rounding
        scale = np.abs(T64[:, :, c]).sum(1) + np.abs(G * slope)
        assert np.all(np.abs(T64[:, :, c].sum(1) - G * slope) <= 1e-6 * scale + 1e-9)


# ---- the plane property --------------------------------------------------------------------------------------------------------
def test_a_plane_is_reproduced_and_the_flat_depth_is_a_staircase(oracle, small_assets):
    """Vertices on z = a x + b y + c with every value exact in fp32 (x and y multiples of 1/2, a, b, c small integers and
    halves): the interpolated depth of every ok pixel is the plane at the pixel, to 2 fp32 ulp; the flat h is not."""
    tri = small_assets["tri"]
    gu, gv = 20, 24
    iu, iv = np.meshgrid(np.arange(gu), np.arange(gv), indexing="ij")
    x = (1.5 * iv + 2.0).reshape(-1)
    y = (2.0 * iu + 1.5).reshape(-1)
    x[1::2] += 0.5                                                           # (no axis-aligned grid: every triangle is scalene)
    a, b, c = 0.5, -1.5, 70.0
    V = np.stack([x, y, a * x + b * y + c])[None].astype(np.float32)
    assert np.array_equal(V[0, 2].astype(np.float64), a * x + b * y + c) and V[0, 2].min() > 1
    H, W = 44, 40
    tind = oracle.render_depth(V, tri, small_assets["vertex"], H, W)[3].reshape(1, -1)
    px, ids = RN.contributing(tri, tind[0], V.shape[2])
    assert len(px) > 1000
    d = RD.forward(V, tri, tind, H, W).reshape(-1)
    plane = (a * (px % W) + b * (px // W) + c).astype(np.float32)
    ulp = np.spacing(np.abs(plane))
    assert np.all(np.abs(d[px].astype(np.float64) - plane) <= 2 * ulp)
    assert np.all(d[tind[0] < 0].view(np.uint32) == RD.BACKGROUND.view(np.uint32))
    flat = RD.flat_h(V[0], ids)
    off = np.abs(flat.astype(np.float64) - plane)
    assert (off > 2 * ulp).mean() > 0.9 and off.max() > 0.25                 # a step of the facet's z range, pixel after pixel


def test_degenerate_and_uncovered_pixels_of_the_model():
    """den == 0 gives the flat h in both directions; -1, NaN, ntri and a bad id give the background and no term"""
    V = np.array([[[1, 5, 5, 2], [1, 1, 1, 6], [3, 4.5, 6, 9]]], np.float32)       # vertices 1 and 2 coincide in x, y
    tri = np.array([[0, 0, 0], [1, 1, 4], [2, 3, 3]], np.float32)                  # triangle 0: den == 0; triangle 2: a bad id
    tind = np.array([[0, 1, -1, np.nan, 3, 2]], np.float32)
    d = RD.forward(V, tri, tind, 2, 3).reshape(-1)
    assert d[0] == np.float32((np.float32(3 + 4.5) + np.float32(6)) / np.float32(3))
    assert np.isfinite(d[1]) and d[1] != d[0]
    assert np.all(d[2:].view(np.uint32) == RD.BACKGROUND.view(np.uint32))
    g = np.array([[0.75, 2, 1, 1, 1, 1]], np.float32)
    ids, T64, T32 = RD.terms(g[0], V[0], tri, tind[0], 4, 3)
    assert ids.shape == (3, 2)
    assert np.all(T32[0, :, 2] == np.float32(0.25)) and not T32[0, :, 0:2].any()
    R = RD.model(g, V, tri, tind, 2, 3)
    assert not R.faces[0].bad and np.abs(R.dense(0)).sum() > 0
