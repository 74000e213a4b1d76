"""CPU: the shape-from-shading entry points (fr_sfs_intensity_forward / _backward and their companions) exist, validate before any
HIP call and report their launch geometry; the kernel's pseudo-inverse, through its host instantiation fr_debug_sfs_pinv, is held to
np.linalg.pinv; the float64 model of the GPU tests (tests/ref_sfs.py) is itself held to np.linalg.pinv and to torch float64
autograd over the stock-torch route."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
import ref_sfs as RS

NEW = ("fr_sfs_state_bytes", "fr_sfs_intensity_forward", "fr_sfs_intensity_backward", "fr_debug_sfs_geom", "fr_debug_sfs_pinv")
DP = ctypes.POINTER(ctypes.c_double)


def _L():
    return pkg("_lib").lib()


def _geom(B, H, W):
    out = (ctypes.c_int * 4)()
    _L().fr_debug_sfs_geom(B, H, W, out)
    return list(out)


def _pinv(M, rcond):
    m = np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]], np.float64)
    p = np.zeros(6)
    rank = ctypes.c_int(-1)
    assert _L().fr_debug_sfs_pinv(m.ctypes.data_as(DP), rcond, p.ctypes.data_as(DP), ctypes.byref(rank)) == 0
    return np.array([[p[0], p[1], p[2]], [p[1], p[3], p[4]], [p[2], p[4], p[5]]]), rank.value


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert b"fr_hotpath 0.4 " in L.fr_version()


def test_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    B, H, W = 5, 8, 9
    need = L.fr_sfs_state_bytes(H, W)
    assert need == 10 * H * W * 8
    assert L.fr_sfs_state_bytes(0, W) == 0 and L.fr_sfs_state_bytes(H, 0) == 0 and L.fr_sfs_state_bytes(-1, W) == 0
    assert L.fr_sfs_state_bytes(200, 200) == 3200000

    def fwd(a=one, n=one, im=one, a2=one, n2=one, B=B, H=H, W=W, rc=1e-6, out=one, st=al, nb=need):
        return L.fr_sfs_intensity_forward(a, n, im, a2, n2, B, H, W, rc, out, st, nb, nul)

    def bwd(g=one, a=one, im=one, a2=one, n2=one, st=al, nb=need, B=B, H=H, W=W, gn=one, gn2=one):
        return L.fr_sfs_intensity_backward(g, a, im, a2, n2, st, nb, B, H, W, gn, gn2, nul)
    for k in ("B", "H", "W"):
        assert fwd(**{k: -1}) == -1 and bwd(**{k: -1}) == -1, k
    for rc in (-1e-9, float("nan"), float("inf"), -float("inf")):
        assert fwd(rc=rc) == -1, rc
    for k in ("a", "n", "im", "a2", "n2", "out"):
        assert fwd(**{k: nul}) == -1, k
    for k in ("g", "a", "im", "a2", "n2"):
        assert bwd(**{k: nul}) == -1, k
    assert bwd(gn=nul, gn2=nul) == -1                                        # both outputs missing
    for call in (fwd, bwd):
        assert call(nb=need - 1) == -2 and call(st=nul) == -2                # state too small / missing
        assert call(st=ctypes.c_void_p(4096 + 8)) == -2                      # not 16-byte aligned
        assert call(B=0) == 0 and call(H=0) == 0 and call(W=0) == 0          # no work
        assert call(B=0, H=-1) == -1                                         # the scalar checks come first
    assert fwd(B=0, a=nul, n=nul, im=nul, a2=nul, n2=nul, out=nul, st=nul, nb=0) == 0
    assert bwd(B=0, g=nul, a=nul, im=nul, a2=nul, n2=nul, gn=nul, gn2=nul, st=nul, nb=0) == 0
    assert fwd(B=0, rc=-1.0) == -1
    assert bwd(gn=nul, nb=need - 1) == -2 and bwd(gn2=nul, nb=need - 1) == -2   # one output alone is legal: as far as the state
    assert fwd(rc=0.0, nb=need - 1) == -2 and fwd(n2=one, n=one, nb=need - 1) == -2
    assert fwd(H=1 << 16, W=1 << 15, st=al, nb=1 << 62) == -4                # 2^31 pixels
    p = np.zeros(6)
    r = ctypes.c_int(0)
    bad = L.fr_debug_sfs_pinv
    assert bad(p.ctypes.data_as(DP), -1.0, p.ctypes.data_as(DP), ctypes.byref(r)) == -1
    assert bad(p.ctypes.data_as(DP), float("nan"), p.ctypes.data_as(DP), ctypes.byref(r)) == -1
    assert bad(None, 1e-6, p.ctypes.data_as(DP), ctypes.byref(r)) == -1


def test_geometry():
    assert _geom(0, 5, 4) == [0] * 4 and _geom(6, 0, 4) == [0] * 4 and _geom(6, 5, 0) == [0] * 4
    for B, H, W in RS.CASES + ((32, 200, 200), (64, 200, 200)):
        px, slices, blocks, lds = _geom(B, H, W)
        assert px == 64 and blocks == -(-H * W // px)
        assert slices == min(4, max(1, B // 4))                              # the header's S: a function of B alone
        assert lds == (9 * slices + 3) * px * 8 <= 64 * 1024
        assert _geom(B, W, H)[1] == slices and _geom(B, 1, 1)[1] == slices
    assert _geom(64, 9, 70)[1] > 1 and _geom(65, 3, 67)[1] > 1               # the split kernel is what those cases run
    px, _, blocks, _ = _geom(65, 3, 67)
    assert blocks * px > 201 > (blocks - 1) * px and 201 % px != 0           # a partial last workgroup
    assert _geom(64, 200, 200)[2] == 625


# ---- the solver against numpy ------------------------------------------------------------------------------------------------
def _matrices():
    rs = np.random.RandomState(0)
    out = [np.zeros((3, 3))]
    for _ in range(3000):
        Y = rs.standard_normal((3, rs.randint(1, 65)))
        Y /= np.linalg.norm(Y, axis=0)
        out.append(Y @ Y.T)
    for _ in range(200):
        v, w = rs.standard_normal(3), rs.standard_normal(3)
        v /= np.linalg.norm(v)
        w /= np.linalg.norm(w)
        Q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        out += [np.outer(v, v) * rs.uniform(0.5, 30), np.outer(v, v) * 3 + np.outer(w, w),          # exact rank 1, rank 2
                np.diag(rs.uniform(0.1, 10, 3)), np.diag([rs.uniform(0.1, 10), 0.0, rs.uniform(0.1, 10)]),
                Q @ np.diag([2.0, 2.0, rs.uniform(0.5, 5)]) @ Q.T, Q @ np.diag([2.0, 2.0, 2.0]) @ Q.T,   # equal eigenvalues
                Q @ np.diag([1.0, 1.0, 0.0]) @ Q.T]
    return out


@pytest.mark.parametrize("rcond", [1e-6, 1e-8])
def test_pinv_against_numpy(rcond):
    worst, n = 0.0, 0
    for M in _matrices():
        for scale in (1.0, 1e-30, 1e30):
            A = M * scale
            A = (A + A.T) / 2
            lam = np.linalg.eigvalsh(A)
            ratio = np.abs(lam) / max(lam.max(), 1e-300)
            if not np.all((ratio > RS.GAP_HI) | (ratio < RS.GAP_LO)):        # the gap condition: rcond sits inside the gap,
                continue                                                     # every kept eigenvalue within 1e3 of the largest
            want = np.linalg.pinv(A, rcond=rcond, hermitian=True)
            got, rank = _pinv(A, rcond)
            assert rank == (int((ratio > rcond).sum()) if lam.max() > 0 else 0), (rank, lam)
            nrm = np.linalg.norm(want)
            assert np.abs(got - want).max() <= 2.0 ** -40 * nrm, (np.abs(got - want).max(), nrm, lam)
            if nrm == 0:
                assert not got.any()
            else:
                worst = max(worst, np.abs(got - want).max() / nrm)
            n += 1
    assert n > 9000, n
    print("matrices %d, worst |P - pinv| / ||pinv|| = %.3g (bound %.3g)" % (n, worst, 2.0 ** -40))


def test_pinv_non_finite_returns():
    """a NaN (or an Inf) in the matrix: the call returns -- the sweep count is fixed -- with NaN in P and rank 0"""
    for bad in (np.nan, np.inf, -np.inf):
        for i, j in ((0, 0), (0, 1), (1, 2), (2, 2)):
            A = np.eye(3) + 0.25
            A[i, j] = A[j, i] = bad
            P, rank = _pinv(A, 1e-6)
            assert np.isnan(P).all() and rank == 0, (bad, i, j, P, rank)


# ---- the model's self-checks -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=RS.CASES, ids=lambda c: "B%d_%dx%d" % c)
def case(request):
    d = RS.inputs(*request.param)                                            # (asserts the gap condition)
    return request.param, d, RS.model(*RS.args(d))


def test_model_pinv_is_numpys(case):
    _, _, m = case
    want = np.linalg.pinv(m.M, rcond=RS.RCOND, hermitian=True)
    assert np.abs(m.P - want).max() <= 4e-15, np.abs(m.P - want).max()
    assert np.array_equal(m.rank[0, :3], np.minimum([0, 1, 2], m.rank[0, :3]))   # pixels (0,0), (0,1), (0,2): at most 0, 1, 2 faces
    assert m.rank[0, 0] == 0 and not m.P[0, 0].any() and not m.intensity[:, 0, 0].any()
    assert m.rank[1, 1] <= 1                                                 # one normal repeated by every face


def test_model_grads_are_float64_autograd_of_the_torch_route(case, monkeypatch):
    """torch float64 autograd over the stock-torch spherical_harmonics_intensity with the model's P in place of the (detached)
    pinv: the two gradient maps of ref_sfs.grads, to 3e-16 -- an ABSOLUTE figure that belongs to ref_sfs.grad_out's g (seed 1:
    gradients up to 1.4 in magnitude, one float64 ulp there is 2.2e-16; autograd forms P^T (q u_b) where the model forms u_b (P q),
    so single elements differ by an ulp)."""
    (B, H, W), d, m = case
    Lm = pkg("nets.losses")
    monkeypatch.setattr(Lm, "_pinv_sym3", lambda A, rtol=1e-15: torch.as_tensor(m.P))
    t = {k: torch.as_tensor(v.astype(np.float64)) for k, v in d.items()}
    t["normal"].requires_grad_(True)
    t["normal_new"].requires_grad_(True)
    out = Lm.spherical_harmonics_intensity(t["abedo"], t["normal"], t["im_gray"], t["abedo_new"], t["normal_new"])
    assert np.abs(out.detach().numpy() - m.intensity).max() <= 3e-16
    g = RS.grad_out(B, H, W)
    out.backward(torch.as_tensor(g.astype(np.float64)))
    gn, gn2, _, _ = RS.grads(g, *RS.args(d), m=m)
    e1 = np.abs(t["normal"].grad.numpy() - gn).max()
    e2 = np.abs(t["normal_new"].grad.numpy() - gn2).max()
    print("B%d %dx%d: |grad_normal - autograd| %.3g, |grad_normal_new - autograd| %.3g" % (B, H, W, e1, e2))
    assert e1 <= 3e-16 and e2 <= 3e-16, (e1, e2)
