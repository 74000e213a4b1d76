"""numpy float64 restatement of the per-face albedo fit (include/fr_hotpath.h, "per-face albedo fit"): the basis per triangle and the
per-pixel arithmetic in the kernel's source order -- every product and sum rounded on its own, which numpy's float64 scalars do --
with math.fsum for the moments (the correctly rounded sum of the rounded products: the kernel differs from it by its order of
summation alone) and numpy's Cholesky for the solve.  Also the standard inputs of tests/test_albedo_lse_cpu.py and _gpu.py."""
import math

import numpy as np

KMAX = 15
PIVOT_TOL = 2.0 ** -40


def f2i_x86(x):
    """the x86 conversion of the render backwards on an fp32 array: NaN / out of range -> INT_MIN"""
    x = np.asarray(x, np.float32)
    ok = (x >= np.float32(-2147483648.0)) & (x < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, x, 0)).astype(np.int64), -2 ** 31)


def basis_ref(tri, pc_tex):
    """Phi [T,K] float64: nine widened fp32 terms, channel-major, then vertex 1, 2, 3, onto the first; / 9.0; +0.0 rows for bad ids"""
    tri = np.asarray(tri, np.float32)
    pc = np.asarray(pc_tex, np.float32)
    nver, K = pc.shape[0] // 3, pc.shape[1]
    v = f2i_x86(tri)                                          # [3,T]
    ok = ((v >= 0) & (v < nver)).all(0)
    vs = np.where(ok[None], v, 0)
    s = None
    for c in range(3):
        for j in range(3):
            term = pc[c * nver + vs[j]].astype(np.float64)    # [T,K]
            s = term if s is None else s + term
    s = s / 9.0
    s[~ok] = 0.0
    return s


def shading(lighting, normal_new):
    """d = (l_x n_x + l_y n_y) + l_z n_z -> [B,npix] float64"""
    n = np.asarray(normal_new, np.float32)
    B = n.shape[0]
    n = n.reshape(B, -1, 3).astype(np.float64)
    l = np.asarray(lighting, np.float64).reshape(3, -1)
    with np.errstate(all="ignore"):
        return (l[0][None] * n[..., 0] + l[1][None] * n[..., 1]) + l[2][None] * n[..., 2]


def pixel_x(basis, tri_ind, lighting, normal_new, abedo, im_gray):
    """x [B,npix,16] float64 in the kernel's source order, and counted [B,npix]"""
    basis = np.asarray(basis, np.float64)
    ntri, K = basis.shape
    B = tri_ind.shape[0]
    t = f2i_x86(np.asarray(tri_ind, np.float32).reshape(B, -1))
    npix = t.shape[1]
    counted = (t >= 0) & (t < ntri)
    ts = np.where(counted, t, 0)
    a = np.asarray(abedo, np.float32).reshape(B, npix).astype(np.float64)
    I = np.asarray(im_gray, np.float32).reshape(B, npix).astype(np.float64)
    d = shading(lighting, normal_new)
    with np.errstate(all="ignore"):
        rho = I - a * d
        x = np.zeros((B, npix, 16), np.float64)
        if ntri > 0:
            x[..., :K] = d[..., None] * basis[ts]
        x[..., K] = rho
    x[~counted] = 0.0
    return x, counted


def moments_fsum(x):
    """M [B,16,16]: fsum of the rounded products x_i x_j over the pixels, and S [B,16,16] = sum |x_i x_j| (the bound's scale)"""
    B = x.shape[0]
    M = np.zeros((B, 16, 16), np.float64)
    S = np.zeros((B, 16, 16), np.float64)
    for b in range(B):
        for i in range(16):
            for j in range(i, 16):
                with np.errstate(all="ignore"):
                    prod = x[b, :, i] * x[b, :, j]
                m = math.fsum(prod) if np.isfinite(prod).all() else float(np.sum(prod))
                M[b, i, j] = M[b, j, i] = m
                S[b, i, j] = S[b, j, i] = float(np.sum(np.abs(prod)))
    return M, S


def gamma(n):
    u = n * 2.0 ** -53
    return u / (1.0 - u)


def ridge_lambda(M, K, ridge):
    """lambda = (ridge tr) / K with tr the chain over k < K from +0.0 of M_kk"""
    tr = np.float64(0.0)
    for k in range(K):
        tr = tr + np.float64(M[k, k])
    return (np.float64(ridge) * tr) / np.float64(K)


def e1_ref(M, K, alpha32):
    """E1 = (E0 - 2 S1) + S2 in the header's order, on the fp32 alpha widened and the unridged G"""
    a = np.asarray(alpha32, np.float32).astype(np.float64)
    M = np.asarray(M, np.float64)
    s1 = np.float64(0.0)
    for k in range(K):
        s1 = s1 + a[k] * M[k, K]
    s2 = np.float64(0.0)
    for k in range(K):
        ga = np.float64(0.0)
        for j in range(K):
            ga = ga + M[k, j] * a[j]
        s2 = s2 + a[k] * ga
    return (M[K, K] - np.float64(2.0) * s1) + s2


def solve_ref(M, K, ridge, count):
    """one face: -> (alpha fp32 [K], E0, E1, ok) by the header's rules, numpy's Cholesky for the factor"""
    M = np.asarray(M, np.float64)
    E0 = M[K, K]
    zero = np.zeros(K, np.float32)
    if not (count > 0 and np.isfinite(M[:K + 1, :K + 1]).all()):
        return zero, E0, E0, 0.0
    Gp = M[:K, :K] + ridge_lambda(M, K, ridge) * np.eye(K)
    try:
        L = np.linalg.cholesky(Gp)
    except np.linalg.LinAlgError:
        return zero, E0, E0, 0.0
    piv = np.diag(L) ** 2
    if not (np.isfinite(piv).all() and (piv > PIVOT_TOL * np.diag(Gp)).all()):
        return zero, E0, E0, 0.0
    y = np.linalg.solve(L, M[:K, K])
    al = np.linalg.solve(L.T, y)
    if not np.isfinite(al).all():
        return zero, E0, E0, 0.0
    a32 = al.astype(np.float32)
    return a32, E0, e1_ref(M, K, a32), 1.0


def fit_ref(basis, tri_ind, lighting, normal_new, abedo, im_gray, ridge):
    """the whole call: -> (alpha [B,K] fp32, stats [B,4], M [B,16,16], S [B,16,16])"""
    K = np.asarray(basis).shape[1]
    x, counted = pixel_x(basis, tri_ind, lighting, normal_new, abedo, im_gray)
    M, S = moments_fsum(x)
    B = x.shape[0]
    alpha = np.zeros((B, K), np.float32)
    stats = np.zeros((B, 4), np.float64)
    for b in range(B):
        cnt = float(counted[b].sum())
        alpha[b], E0, E1, ok = solve_ref(M[b], K, ridge, cnt)
        stats[b] = (cnt, E0, E1, ok)
    return alpha, stats, M, S


# ---- the standard inputs ------------------------------------------------------------------------------------------------------
STD_B, STD_S, STD_K = 3, 32, 10


def std_pc_tex(assets, seed=1234):
    N = np.asarray(assets["mu"]).size // 3
    return (0.05 * np.random.RandomState(seed).standard_normal((3 * N, STD_K))).astype(np.float32)


def std_vertices(assets, B=STD_B, S=STD_S, shift=None):
    """R_y(0.2 b) mu 1.5e-4 + (S/2, S/2, 0) -> [B,3,N] fp32; shift: {b: (dx, dy)} moves a face"""
    mu = np.asarray(assets["mu"], np.float64).reshape(3, -1)
    V = np.empty((B, 3, mu.shape[1]), np.float32)
    for b in range(B):
        c, s = math.cos(0.2 * b), math.sin(0.2 * b)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        v = R @ (mu * 1.5e-4) + np.array([[S / 2.0], [S / 2.0], [0.0]])
        if shift and b in shift:
            v = v + np.array([[shift[b][0]], [shift[b][1]], [0.0]])
        V[b] = v.astype(np.float32)
    return V


def maps_from_render(tex_img, normal):
    """compute_abedo_image's post-processing (nets/network.py) in numpy fp32: the albedo image and the normalised normal map"""
    a = np.maximum(np.asarray(tex_img, np.float32), np.float32(1e-6)).mean(-1, keepdims=True, dtype=np.float32)
    n = np.asarray(normal, np.float32)
    n = np.where(n[..., 2:3] < 0, np.float32(-1.0) * n, n)
    mag = (n * n).sum(-1, dtype=np.float32)
    mag = np.where(mag > np.float32(1e-6), mag, np.float32(1.0))
    return a, (n / (np.sqrt(mag) + np.float32(1e-6))[..., None]).astype(np.float32)


def std_lighting(H, W, seed=5):
    rs = np.random.RandomState(seed)
    return np.array([0.2, 0.1, 0.9])[:, None, None] + 0.1 * rs.standard_normal((3, H, W))


def std_alpha_star(B, seed=6):
    return np.random.RandomState(seed).standard_normal((B, STD_K))


def std_image(basis, tri_ind, lighting, normal, abedo, alpha_star):
    """I = fl32((a + phi . alpha*) d) at the counted pixels, 0 elsewhere -> [B,H,W,1] fp32"""
    B, H, W = tri_ind.shape[:3]
    t = f2i_x86(np.asarray(tri_ind, np.float32).reshape(B, -1))
    counted = (t >= 0) & (t < basis.shape[0])
    t = np.where(counted, t, 0)
    a = np.asarray(abedo, np.float32).reshape(B, -1).astype(np.float64)
    d = shading(lighting, normal)
    phi_alpha = np.einsum("bpk,bk->bp", basis[t], alpha_star)
    I = np.where(counted, (a + phi_alpha) * d, 0.0)
    return I.astype(np.float32).reshape(B, H, W, 1)
