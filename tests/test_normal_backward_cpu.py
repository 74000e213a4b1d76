"""CPU: the normal-gradient entry points (fr_render_normal_backward and its two companions) exist, validate before any HIP
call and choose a launch geometry that fits the LDS; the float64 model of the GPU tests (tests/ref_normal_backward.py) is itself
held to torch float64 autograd over a gather-based restatement of the forward normal and its post-processing."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import ref_normal_backward as RN

NEW = ("fr_render_normal_backward_workspace_bytes", "fr_render_normal_backward", "fr_debug_render_normal_bwd_geom")


def _L():
    return pkg("_lib").lib()


def _geom(B, nver, H, W):
    out = (ctypes.c_int * 6)()
    _L().fr_debug_render_normal_bwd_geom(B, nver, H, W, out)
    return list(out)


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert b"fr_hotpath 0.4 " in L.fr_version()


def test_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    call = L.fr_render_normal_backward
    B, nver, ntri, H, W = 2, 10, 5, 8, 9
    need = L.fr_render_normal_backward_workspace_bytes(B, nver, H, W)
    assert need == B * H * W * 48 + B * 1 * 8
    assert L.fr_render_normal_backward_workspace_bytes(3, 7, 33, 40) == 3 * 1320 * 48 + 3 * 2 * 8
    assert L.fr_render_normal_backward_workspace_bytes(0, nver, H, W) == 0

    def args(g=one, gs=3, v=one, vp=nver, tri=one, ti=one, vg=one, B=B, nver=nver, ntri=ntri, H=H, W=W, mode=0, acc=0, ws=al,
             nb=need):
        return (g, gs, v, vp, tri, ti, vg, B, nver, ntri, H, W, mode, acc, ws, nb, nul)
    for k in ("B", "nver", "ntri", "H", "W"):
        assert call(*args(**{k: -1})) == -1, k
    for k in ("g", "v", "tri", "ti", "vg"):                                  # bad pointers
        assert call(*args(**{k: nul})) == -1, k
    assert call(*args(mode=2)) == -1 and call(*args(mode=-1)) == -1          # bad mode
    assert call(*args(acc=2)) == -1
    assert call(*args(gs=2)) == -1 and call(*args(gs=0)) == -1               # stride below 3
    assert call(*args(vp=nver - 1)) == -1                                    # pitch below nver
    assert call(*args(nb=need - 1)) == -2 and call(*args(ws=nul)) == -2      # workspace too small / missing
    assert call(*args(ws=ctypes.c_void_p(4096 + 8))) == -2                   # not 16-byte aligned
    assert call(*args(B=0)) == 0                                             # empty batch
    assert call(*args(B=0, g=nul, v=nul, tri=nul, ti=nul, vg=nul, ws=nul, nb=0)) == 0
    assert call(*args(B=0, mode=2)) == -1 and call(*args(B=0, gs=2)) == -1   # the scalar checks come first
    assert call(*args(gs=7, vp=nver + 22, mode=1, acc=1, nb=need - 1)) == -2  # every legal variant gets as far as the workspace


@pytest.mark.parametrize("B", [1, 3, 8, 16, 32, 64])
@pytest.mark.parametrize("nver", [1, 3, 100, 6656, 6657, 20000, 53215, 1 << 20])
def test_geometry_is_consistent(B, nver):
    for H, W in ((5, 6), (200, 200), (1100, 1000)):
        splits, rng, shift, chunks, lds, xcd = _geom(B, nver, H, W)
        assert splits >= 1 and splits * rng >= nver and (splits - 1) * rng < nver
        assert 3 * 8 * rng <= lds <= 160 * 1024
        assert shift == RN.shift_of(H * W) and chunks == (H * W + 1023) // 1024
        assert xcd == (1 if B % 8 == 0 else 0)
        assert rng <= max(1, -(-nver // ((256 + B - 1) // B)))               # small batches: at least ~one workgroup per CU
    assert _geom(0, nver, 5, 6) == [0] * 6 and _geom(B, nver, 0, 6) == [0] * 6
    assert _geom(B, 0, 5, 6) == [0] * 6


# ---- the model against torch float64 autograd -------------------------------------------------------------------------------
def _scene(seed, nver, ntri, B, H, W, flip=False):
    """A random scene whose coordinates are multiples of 1/4 below 32: every difference of two of them AND every component of
    the normal (18 bits) is exact in fp32, so the model's a = fl32(P1 - P2) and n = fl32(a x b) -- roundings the backward treats
    as the identity -- are the numbers the float64 restatement differentiates."""
    rs = np.random.RandomState(seed)
    V = (rs.randint(-128, 128, (B, 3, nver)) / 4.0).astype(np.float32)
    tri = rs.randint(0, nver, (3, ntri)).astype(np.float32)
    if flip:
        tri = tri[[0, 2, 1]].copy()
    tind = rs.randint(-1, ntri, (B, H * W)).astype(np.float32)
    g = rs.standard_normal((B, H * W, 3)).astype(np.float32)
    return g, V, tri, tind


def _model_sums64(g, V, tri, tind, mode):
    """The model's terms BEFORE their rounding to fp32, summed in float64 per element, and the sum of their magnitudes."""
    B, _, nver = V.shape
    S = np.zeros((B, 3, nver))
    A = np.zeros((B, 3, nver))
    for b in range(B):
        ids, T64, _, _ = RN.terms(g[b], V[b], tri, tind[b], nver, mode)
        for k in range(3):
            for c in range(3):
                np.add.at(S[b, c], ids[k], T64[:, k, c])
                np.add.at(A[b, c], ids[k], np.abs(T64[:, k, c]))
    return S, A


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("flip", [False, True])
def test_model_agrees_with_float64_autograd(mode, flip):
    H, W = 7, 9
    for seed, nver, ntri in ((0, 12, 9), (1, 40, 60), (2, 5, 30)):           # (few vertices: repeated ids, shared vertices)
        g, V, tri, tind = _scene(seed, nver, ntri, 2, H, W, flip)
        tri[:, 0] = (1, 1, 2)                                                # a repeated vertex id: a = 0
        V[:, :, 3] = V[:, :, 4]                                              # two vertices at one point: degenerate triangles
        if nver > 10:
            V[0, :, 7] = 2 * V[0, :, 6] - V[0, :, 5]                         # three collinear vertices ...
            tri[:, 1] = (5, 6, 7)                                            # ... and the triangle over them: zero normal
        S, A = _model_sums64(g, V, tri, tind, mode)
        want = RN.torch_grad(g, V, tri, tind, H, W, mode)
        assert np.all(np.isfinite(want))
        assert np.abs(want).max() > 1.0
        # relative to the element's own sum of |terms| -- or, where the model's terms vanish identically (a x G with a == 0)
        # and autograd's chain leaves the rounding of products that cancel, to a lower bound of the batch's largest |term|:
        # its largest element sum over the number of covered pixels
        scale = np.maximum(A, A.max(axis=(1, 2), keepdims=True) / max(1, int((tind >= 0).sum())))
        assert np.all(np.abs(S - want) <= 1e-12 * scale), float((np.abs(S - want) / scale).max())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("flip", [False, True])
def test_model_agrees_with_float64_autograd_where_the_forward_rounds(mode, flip):
    """Arbitrary fp32 coordinates: a, b and n are rounded by the forward, the backward treats those roundings as the identity,
    and so does the restatement (straight-through in RN.torch_grad) -- the derivative is taken at the forward's numbers."""
    H, W, nver, ntri = 7, 9, 40, 60
    rs = np.random.RandomState(11 + mode)
    V = np.stack([rs.uniform(0, W, (2, nver)), rs.uniform(0, H, (2, nver)), rs.uniform(1, 9, (2, nver))], axis=1).astype(np.float32)
    tri = rs.randint(0, nver, (3, ntri)).astype(np.float32)
    if flip:
        tri = tri[[0, 2, 1]].copy()
    tind = rs.randint(-1, ntri, (2, H * W)).astype(np.float32)
    g = rs.standard_normal((2, H * W, 3)).astype(np.float32)
    ids = RN.contributing(tri, tind[0], nver)[1]
    a, _, _ = RN.forward_normal(V[0], ids)
    P = V[0].astype(np.float64)
    assert np.any(a != (P[:, ids[0]] - P[:, ids[1]]).T)                      # the forward does round here
    S, A = _model_sums64(g, V, tri, tind, mode)
    want = RN.torch_grad(g, V, tri, tind, H, W, mode)
    scale = np.maximum(A, A.max(axis=(1, 2), keepdims=True) / max(1, int((tind >= 0).sum())))
    assert np.all(np.abs(S - want) <= 1e-12 * scale), float((np.abs(S - want) / scale).max())


def test_model_k1_known_answer():
    """one triangle (1,1,5), (4,1,5), (1,4,5) on a 6 x 5 screen, six covered pixels, G = (0,0,1) on each."""
    V = np.array([[[1, 4, 1], [1, 1, 4], [5, 5, 5]]], np.float32)
    tri = np.array([[0], [1], [2]], np.float32)
    tind = np.full((1, 30), -1, np.float32)
    tind[0, [7, 8, 9, 13, 14, 19]] = 0
    g = np.zeros((1, 30, 3), np.float32)
    g[..., 2] = 1
    R = RN.model(g, V, tri, tind, 5, 6, 0)
    F = R.faces[0]
    np.testing.assert_array_equal(R.dense(0), [[-18, 18, 0], [-18, 0, 18], [0, 0, 0]])
    assert len(F.elem) == 9 and np.all(F.n == 6) and RN.to_float(F.M) == 3.0 and not F.bad
    np.testing.assert_array_equal(R.dense(0, "A"), [[18, 18, 0], [18, 0, 18], [0, 0, 0]])
    # the exact check accepts the model's own sums and refuses one that is off by an fp32 ulp beyond the grid error
    got = R.dense(0)[None].astype(np.float32)
    assert RN.check_bound(got, R) == 0.0
    got[0, 0, 0] = np.nextafter(np.float32(-18), np.float32(0))
    with pytest.raises(AssertionError):
        RN.check_bound(got, R)
