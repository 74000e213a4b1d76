"""CPU: the texture-gradient entry points (fr_render_texture_backward and its companions, fr_sfs_intensity_backward_tex) exist,
validate before any HIP call and choose a launch geometry that fits the LDS; the integer model of the GPU tests
(tests/ref_texture_backward.py) is itself held to exact integer sums, to torch float64 autograd over a gather-based restatement of
the forward lookup, and to a hand-computed answer."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from conftest import pkg
import ref_texture_backward as RT

NEW = ("fr_render_texture_backward_workspace_bytes", "fr_render_texture_backward", "fr_debug_render_texture_bwd_geom",
       "fr_sfs_intensity_backward_tex")
GEOM = ("splits", "range", "shift", "chunks", "lds", "xcd", "slices")


def _L():
    return pkg("_lib").lib()


def _geom(B, nver, H, W, tb):
    out = (ctypes.c_int * 7)()
    _L().fr_debug_render_texture_bwd_geom(B, nver, H, W, tb, out)
    return dict(zip(GEOM, out))


def test_symbols_exported_and_version_unchanged():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert b"fr_hotpath 0.4 " in L.fr_version()


def _ws_formula(B, nver, H, W, tb):
    """the header's formula: 24 bytes per pixel, 8 per 1,024-pixel chunk rounded up to 16, 24 nver per face slice"""
    npix = H * W
    chunks = (npix + 1023) // 1024
    return B * npix * 24 + ((B * chunks * 8 + 15) & ~15) + _geom(B, nver, H, W, tb)["slices"] * 24 * nver


def test_workspace_size_formula():
    L = _L()
    ws = L.fr_render_texture_backward_workspace_bytes
    assert ws(2, 10, 8, 9, 2) == 2 * 72 * 24 + 16
    assert ws(3, 7, 33, 40, 3) == 3 * 1320 * 24 + 48
    assert ws(1, 7, 33, 40, 1) == 1320 * 24 + 16                              # one face: its own scope, no slabs
    for B, nver, H, W in ((3, 7, 33, 40), (17, 20000, 5, 7), (64, 53215, 200, 200), (8, 12, 40, 40)):
        for tb in (1, B):
            g = _geom(B, nver, H, W, tb)
            assert (g["slices"] > 0) == (tb == 1 and B > 1)
            assert ws(B, nver, H, W, tb) == _ws_formula(B, nver, H, W, tb)
    assert ws(0, 10, 8, 9, 1) == 0 and ws(2, 0, 8, 9, 2) == 0 and ws(2, 10, 0, 9, 2) == 0 and ws(2, 10, 8, 0, 1) == 0
    assert ws(4, 10, 8, 9, 2) == 0 and ws(-1, 10, 8, 9, 1) == 0               # a tex_batch that is neither 1 nor B


def test_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    call = L.fr_render_texture_backward
    B, nver, ntri, H, W = 2, 10, 5, 8, 9
    need = L.fr_render_texture_backward_workspace_bytes(B, nver, H, W, B)
    need1 = L.fr_render_texture_backward_workspace_bytes(B, nver, H, W, 1)
    assert need1 > need > 0

    def args(g=one, gs=3, tri=one, ti=one, tg=one, B=B, nver=nver, ntri=ntri, H=H, W=W, tb=B, acc=0, ws=al, nb=need1):
        return (g, gs, tri, ti, tg, B, nver, ntri, H, W, tb, acc, ws, nb, nul)
    for k in ("B", "nver", "ntri", "H", "W"):
        assert call(*args(**{k: -1})) == -1, k
    assert call(*args(tb=3)) == -1 and call(*args(tb=0)) == -1 and call(*args(tb=-1)) == -1
    assert call(*args(acc=2)) == -1 and call(*args(acc=-1)) == -1
    assert call(*args(gs=2)) == -1 and call(*args(gs=0)) == -1               # stride below 3
    assert call(*args(B=0)) == 0 and call(*args(nver=0)) == 0                # empty batch, empty texture
    assert call(*args(B=0, g=nul, tri=nul, ti=nul, tg=nul, ws=nul, nb=0)) == 0
    assert call(*args(B=0, tb=5)) == 0                                       # (tex_batch is only judged against a batch)
    assert call(*args(B=0, acc=2)) == -1 and call(*args(B=0, gs=2)) == -1 and call(*args(nver=0, acc=2)) == -1   # scalars first
    for k in ("g", "tri", "ti", "tg"):                                       # bad pointers
        assert call(*args(**{k: nul})) == -1, k
    assert call(*args(tg=nul, H=0)) == -1                                    # texture_grad is needed even without pixels
    for tb, nb in ((B, need), (1, need1)):
        assert call(*args(tb=tb, nb=nb - 1)) == -2 and call(*args(tb=tb, ws=nul)) == -2   # workspace too small / missing
        assert call(*args(tb=tb, ws=ctypes.c_void_p(4096 + 8))) == -2        # not 16-byte aligned
        assert call(*args(tb=tb, gs=7, acc=1, nb=nb - 1)) == -2              # every legal variant gets as far as the workspace
    assert call(*args(H=65536, W=32768, nb=1 << 62)) == -4                   # 2^31 pixels per face
    assert call(*args(H=65536, W=32768, ws=nul, nb=0)) == -4
    assert call(*args(ntri=1 << 24)) == -4


def test_sfs_backward_tex_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    call = L.fr_sfs_intensity_backward_tex
    B, H, W = 3, 4, 5
    need = L.fr_sfs_state_bytes(H, W)

    def args(g=one, a=one, im=one, a2=one, n2=one, st=al, nb=need, B=B, H=H, W=W, gn=one, gn2=one, ga=one):
        return (g, a, im, a2, n2, st, nb, B, H, W, gn, gn2, ga, nul)
    for k in ("B", "H", "W"):
        assert call(*args(**{k: -1})) == -1, k
    assert call(*args(B=0)) == 0 and call(*args(H=0)) == 0 and call(*args(W=0, gn=nul, gn2=nul, ga=nul)) == 0
    assert call(*args(gn=nul, gn2=nul, ga=nul)) == -1                        # all three outputs NULL
    for k in ("g", "a", "im", "a2", "n2"):
        assert call(*args(**{k: nul})) == -1, k
    for outs in (dict(gn=nul), dict(gn2=nul), dict(ga=nul), dict(gn=nul, gn2=nul), dict(gn=nul, ga=nul), dict(gn2=nul, ga=nul)):
        assert call(*args(nb=need - 1, **outs)) == -2, outs                  # any one output is enough to get to the state
    assert call(*args(st=nul)) == -2 and call(*args(st=ctypes.c_void_p(4096 + 8))) == -2
    assert call(*args(H=65536, W=32768, nb=1 << 62)) == -4
    # the old entry point is this call with a NULL third output
    old = L.fr_sfs_intensity_backward
    assert old(one, one, one, one, one, al, need, B, H, W, nul, nul, nul) == -1
    assert old(one, one, one, one, one, al, need - 1, B, H, W, one, nul, nul) == -2


@pytest.mark.parametrize("B", [1, 3, 8, 17, 32, 64])
@pytest.mark.parametrize("nver", [1, 3, 100, 256, 257, 6656, 6657, 20000, 53215, 1 << 20])
def test_geometry_is_consistent(B, nver):
    for tb in sorted({1, B}):
        for H, W in ((5, 7), (200, 200), (256, 256), (1025, 1024)):
            g = _geom(B, nver, H, W, tb)
            assert g["splits"] >= 1 and g["splits"] * g["range"] >= nver and (g["splits"] - 1) * g["range"] < nver   # [0, nver) once
            assert 3 * 8 * g["range"] <= g["lds"] <= 160 * 1024
            assert g["chunks"] == (H * W + 1023) // 1024
            shared = tb == 1 and B > 1
            assert g["shift"] == RT.shift_of(H * W * (B if shared else 1))
            if shared:
                assert 1 <= g["slices"] <= B
                fpg = -(-B // g["slices"])
                assert (g["slices"] - 1) * fpg < B <= g["slices"] * fpg       # every face in one slice, no slice empty
                assert g["xcd"] == (1 if g["slices"] % 8 == 0 else 0)
            else:
                assert g["slices"] == 0 and g["xcd"] == (1 if B % 8 == 0 else 0)
    assert _geom(0, nver, 5, 6, 1) == dict.fromkeys(GEOM, 0) and _geom(B, nver, 0, 6, 1) == dict.fromkeys(GEOM, 0)
    assert _geom(B, 0, 5, 6, B) == dict.fromkeys(GEOM, 0) and _geom(B, nver, 5, 6, B + 2) == dict.fromkeys(GEOM, 0)


def test_shift_rises_in_both_scopes():
    assert _geom(17, 100, 256, 256, 1)["shift"] == 1 and _geom(17, 100, 256, 256, 17)["shift"] == 0
    assert _geom(1, 100, 1025, 1024, 1)["shift"] == 1 and _geom(1, 100, 1024, 1024, 1)["shift"] == 0
    assert _geom(64, 100, 200, 200, 1)["shift"] == 2 and _geom(64, 100, 200, 200, 64)["shift"] == 0


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _scene(seed, nver, ntri, B, H, W, scale=1.0):
    rs = np.random.RandomState(seed)
    tri = rs.randint(0, nver, (3, ntri)).astype(np.float32)
    tri[:, 0] = (1, 1, 1)                                                    # one vertex named three times
    tri[:, 1] = (2, 2, 0)
    tri[:, 2] = (nver, 0, 1)                                                 # ids out of range: contribute nothing
    tri[:, 3] = (0, -1, 1)
    tind = rs.randint(-1, ntri, (B, H * W)).astype(np.float32)
    tind[:, 0], tind[:, 1], tind[:, 2], tind[:, 3] = np.nan, ntri, -np.inf, 0.75   # not counted x3, truncates to triangle 0
    g = (rs.standard_normal((B, H * W, 3)) * scale).astype(np.float32)
    g[:, 5] = 0.0
    return g, tri, tind


@pytest.mark.parametrize("tb_shared", [False, True])
def test_model_within_the_bound_of_the_exact_sums(tb_shared):
    """|model - exact| <= 2^-24 |S| + n 2^(shift - 39) M: every q is off by at most half a grid unit 2^(e - 39 + shift) <=
    2^(shift - 39) M, the int64 -> fp32 rounding by at most 2^-24 of the (grid) sum."""
    for seed, nver, ntri, B, H, W, scale in ((0, 12, 9, 3, 20, 17, 1.0), (1, 40, 60, 2, 9, 13, 1e-3), (2, 5, 30, 4, 7, 9, 3e7)):
        g, tri, tind = _scene(seed, nver, ntri, B, H, W, scale)
        tb = 1 if tb_shared else B
        M = RT.model(g, tri, tind, nver, H, W, tb)
        X, n, _ = RT.exact(g, tri, tind, nver, H, W, tb)
        assert not M.bad.any() and n.max() > 3
        assert int(n[:, :, 1].max()) >= 3                                    # the repeated vertex collected its triples
        for s in range(M.bits.shape[0]):
            worst = RT.check_bound(M.value()[s], X[s], n[s], M.M[s], M.shift)
            assert worst <= 1.0
        assert np.all(M.bits[n == 0] == 0)                                   # no term: +0


@pytest.mark.parametrize("tb_shared", [False, True])
def test_model_agrees_with_float64_autograd(tb_shared):
    """the same bound plus 2^-24 A for the roundings of g / 3 (each term is within 2^-24 of its own magnitude of g / 3)"""
    for seed, nver, ntri, B, H, W in ((3, 12, 9, 3, 20, 17), (4, 40, 60, 2, 9, 13)):
        g, tri, tind = _scene(seed, nver, ntri, B, H, W)
        tb = 1 if tb_shared else B
        M = RT.model(g, tri, tind, nver, H, W, tb)
        X, n, A = RT.exact(g, tri, tind, nver, H, W, tb)
        want = RT.torch_grad(g, tri, tind, nver, H, W, tb)
        assert np.abs(want).max() > 1.0
        got = M.value().astype(np.float64)
        for s in range(got.shape[0]):
            for i in np.ndindex(got[s].shape):
                x = Fraction(int(X[s][i]), 1 << RT.UNIT)
                a = Fraction(int(A[s][i]), 1 << RT.UNIT)
                bound = abs(x) / (1 << 24) + int(n[s][i]) * Fraction(M.M[s]) * Fraction(2) ** (M.shift - 39) + a / (1 << 24)
                assert abs(Fraction(got[s][i]) - Fraction(want[s][i])) <= bound, (s, i)
                if n[s][i] == 0:
                    assert want[s][i] == 0 and got[s][i] == 0


def test_model_known_answer_by_hand():
    """one triangle (0, 1, 2) over six pixels, g = (3, 6, -9) on each: terms (1, 2, -3), every vertex collects six of each row.
    A second face with g = (1.5, 0, 3) over two pixels of triangle 1 = (2, 2, 3): vertex 2 twice per pixel."""
    tri = np.array([[0, 2], [1, 2], [2, 3]], np.float32)
    tind = np.full((2, 30), -1, np.float32)
    tind[0, [7, 8, 9, 13, 14, 19]] = 0
    tind[1, [3, 4]] = 1
    g = np.zeros((2, 30, 3), np.float32)
    g[0] = (3, 6, -9)
    g[1] = (1.5, 0, 3)
    per_face = RT.model(g, tri, tind, 5, 5, 6, 2)
    np.testing.assert_array_equal(per_face.value()[0], [[6, 6, 6, 0, 0], [12, 12, 12, 0, 0], [-18, -18, -18, 0, 0]])
    np.testing.assert_array_equal(per_face.value()[1], [[0, 0, 2, 1, 0], [0, 0, 0, 0, 0], [0, 0, 4, 2, 0]])
    assert list(per_face.M) == [3.0, 1.0] and list(per_face.e) == [1, 0] and per_face.shift == 0
    shared = RT.model(g, tri, tind, 5, 5, 6, 1)
    np.testing.assert_array_equal(shared.value()[0], [[6, 6, 8, 1, 0], [12, 12, 12, 0, 0], [-18, -18, -14, 2, 0]])
    assert not shared.value().view(np.uint32)[0, 1, 3] and shared.M[0] == 3.0
    X, n, A = RT.exact(g, tri, tind, 5, 5, 6, 1)
    assert n[0, 0].tolist() == [6, 6, 10, 2, 0] and int(X[0, 2, 2]) == -14 << RT.UNIT and int(A[0, 2, 2]) == 22 << RT.UNIT


def test_model_classes_of_a_bad_scope():
    tri = np.array([[0, 2, 4], [1, 3, 4], [2, 3, 5]], np.float32)
    tind = np.full((2, 12), -1, np.float32)
    tind[0, 0:3] = (0, 1, 1)
    tind[1, 0:2] = (2, 0)
    g = np.ones((2, 12, 3), np.float32)
    g[0, 0, 0] = np.inf                                                      # +Inf to row 0 of 0, 1, 2
    g[0, 1, 0] = -np.inf                                                     # -Inf to row 0 of 2, 3: vertex 2 has both -> NaN
    g[0, 2, 1] = np.nan                                                      # NaN to row 1 of 2, 3
    M = RT.model(g, tri, tind, 6, 3, 4, 2)
    assert list(M.bad) == [True, False]
    F, P, N, Q = RT.FINITE, RT.POS_INF, RT.NEG_INF, RT.NAN
    np.testing.assert_array_equal(M.cls[0], [[P, P, Q, N, F, F], [F, F, Q, Q, F, F], [F, F, F, F, F, F]])
    np.testing.assert_array_equal(M.sum64[0][2], np.array([1, 1, 3, 4, 0, 0]) * float(np.float32(1) / np.float32(3)))
    assert M.nterm[0][2].tolist() == [1, 1, 3, 4, 0, 0]
    shared = RT.model(g, tri, tind, 6, 3, 4, 1)
    assert list(shared.bad) == [True] and shared.cls[0][0, 4] == F and shared.nterm[0][0, 4] == 2
