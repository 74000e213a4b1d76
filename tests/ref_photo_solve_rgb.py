"""The numpy model of the colour photometric solve (include/fr_hotpath.h, "colour photometric solve"): the basis per triangle and
channel, the albedo plane, the per-pixel x of both fits in the header's source order -- every product and sum rounded on its own,
which numpy's float64 arrays do -- math.fsum for the moments (the correctly rounded sum of the rounded products: the kernels differ
from it by their order of summation alone), numpy's Cholesky for the solves, and the alternation.  It shares no code with the
kernels; of the other models it takes the fp32 shading chain (ref_photo_rgb.shade_terms) and gamma and the x86 conversion
(ref_albedo_lse).  Also the standard inputs of tests/test_photo_solve_rgb_cpu.py and _gpu.py."""
import math

import numpy as np

from ref_albedo_lse import f2i_x86, gamma  # noqa: F401
from ref_photo_rgb import LIGHT_RANGES_RGB, shade_terms

F = np.float32
NL = 9
KMAX = 15
PIVOT_TOL = 2.0 ** -40


# ---- basis and image ------------------------------------------------------------------------------------------------------------------
def basis_ref(tri, mu_tex, pc_tex):
    """[T,3,K+1] float64: ((x[v1] + x[v2]) + x[v3]) / 3.0 of the widened fp32 basis columns (slots k < K) and mean (slot K); a
    triangle with a vertex id outside [0, N) gets +0.0"""
    tri = np.asarray(tri, F)
    pc = np.asarray(pc_tex, F)
    mu = np.asarray(mu_tex, F).reshape(-1)
    N, K = pc.shape[0] // 3, pc.shape[1]
    v = f2i_x86(tri)
    ok = ((v >= 0) & (v < N)).all(0)
    vs = np.where(ok[None], v, 0)
    out = np.zeros((tri.shape[1], 3, K + 1), np.float64)
    for c in range(3):
        q = [np.concatenate([pc[c * N + vs[j]].astype(np.float64), mu[c * N + vs[j]].astype(np.float64)[:, None]], 1) for j in range(3)]
        out[:, c] = ((q[0] + q[1]) + q[2]) / 3.0
    out[~ok] = 0.0
    return out


def _hit(basis, tri_ind):
    B = np.shape(tri_ind)[0]
    t = f2i_x86(np.asarray(tri_ind, F).reshape(B, -1))
    hit = (t >= 0) & (t < basis.shape[0])
    return np.where(hit, t, 0), hit


def image_ref(basis, tri_ind, alpha):
    """tex_img [B,H,W,3] fp32: the float64 chain from m_c[t] of + Phi_c[t][k] alpha_k, k ascending, rounded once; +0 off the basis"""
    basis = np.asarray(basis, np.float64)
    K = basis.shape[2] - 1
    shape = np.shape(tri_ind)[:3]
    t, hit = _hit(basis, tri_ind)
    al = np.asarray(alpha, F).astype(np.float64)
    if basis.shape[0] == 0:
        return np.zeros(shape + (3,), F)
    rows = basis[t]                                                    # [B,npix,3,K+1]
    acc = rows[..., K].copy()
    for k in range(K):
        acc = acc + rows[..., k] * al[:, None, None, k]
    return np.where(hit[..., None], acc, 0.0).astype(F).reshape(shape + (3,))


def image_bound(tri, mu_tex, pc_tex, tri_ind, alpha):
    """the header's bound between image_ref and the render of the blended texture: gamma_(K+6)(2^-24) A, [B,H,W,3]"""
    pc = np.abs(np.asarray(pc_tex, np.float64))
    mu = np.abs(np.asarray(mu_tex, np.float64).reshape(-1))
    N, K = pc.shape[0] // 3, pc.shape[1]
    al = np.abs(np.asarray(alpha, np.float64))
    v = np.asarray(tri).astype(np.int64)
    shape = np.shape(tri_ind)[:3]
    t = f2i_x86(np.asarray(tri_ind, F).reshape(shape[0], -1))
    hit = (t >= 0) & (t < v.shape[1])
    t = np.where(hit, t, 0)
    per_vertex = mu[None] + al @ pc.T                                   # [B,3N]
    A = np.zeros(t.shape + (3,))
    for c in range(3):
        for j in range(3):
            A[..., c] += np.take_along_axis(per_vertex, c * N + v[j][t], 1)
    n = K + 6
    u = n * 2.0 ** -24
    return (np.where(hit[..., None], A / 3.0, 0.0) * (u / (1.0 - u))).reshape(shape + (3,))


# ---- the per-pixel x of both fits -----------------------------------------------------------------------------------------------------
def _weight(weight, B, npix):
    return None if weight is None else np.asarray(weight, F).reshape(B, npix)


def light_x(tex_img, normal, tri_ind, target, weight=None, gate_light=None, gain=1.0, offset=0.0):
    """-> x [B,3,npix,16] float64, w [B,npix] float64 (1 without a weight), counted [B,3,npix]"""
    B = np.shape(tex_img)[0]
    gl = np.zeros((B, 3, 9), F) if gate_light is None else gate_light
    st = shade_terms(tex_img, normal, tri_ind, gl)
    npix = st["mag"][0].size
    w32 = _weight(weight, B, npix)
    live = st["covered"].reshape(B, npix)
    with np.errstate(all="ignore"):
        if w32 is not None:
            live = live & (w32 > 0)
        a = st["a"].reshape(B, npix, 3).astype(np.float64)
        H = st["H"].reshape(B, npix, 9).astype(np.float64)
        T = np.asarray(target, F).reshape(B, npix, 3).astype(np.float64)
        g, o = np.float64(F(gain)), np.float64(F(offset))
        x = np.zeros((B, 3, npix, 16))
        counted = np.zeros((B, 3, npix), bool)
        for c in range(3):
            counted[:, c] = live & ((st["s"].reshape(B, npix, 3)[..., c] > 0) if gate_light is not None else True)
            x[:, c, :, 0] = a[..., c] * g
            for k in range(1, NL):
                x[:, c, :, k] = (a[..., c] * H[..., k]) * g
            x[:, c, :, NL] = T[..., c] - o
            x[:, c][~counted[:, c]] = 0.0
    w = np.ones((B, npix)) if w32 is None else w32.astype(np.float64)
    return x, w, counted


def albedo_x(basis, tri_ind, normal, light, target, weight=None, gain=1.0, offset=0.0):
    """-> x [B,npix,3,16] float64 (pixel-major, the channels ascending within a pixel), w [B,npix], counted [B,npix]"""
    basis = np.asarray(basis, np.float64)
    K = basis.shape[2] - 1
    B = np.shape(normal)[0]
    st = shade_terms(np.zeros(np.shape(normal), F), normal, tri_ind, light)
    npix = st["mag"][0].size
    t, counted = _hit(basis, tri_ind)
    w32 = _weight(weight, B, npix)
    with np.errstate(all="ignore"):
        if w32 is not None:
            counted = counted & (w32 > 0)
        s = st["s"].reshape(B, npix, 3)
        sp = np.where(s < 0, F(0.0), s).astype(np.float64)
        T = np.asarray(target, F).reshape(B, npix, 3).astype(np.float64)
        g, o = np.float64(F(gain)), np.float64(F(offset))
        x = np.zeros((B, npix, 3, 16))
        if basis.shape[0] > 0:
            rows = basis[t]                                            # [B,npix,3,K+1]
            q = (sp[..., None] * rows) * g
            x[..., :K] = q[..., :K]
            x[..., K] = (T - o) - q[..., K]
        x[~counted] = 0.0
    w = np.ones((B, npix)) if w32 is None else w32.astype(np.float64)
    return x, w, counted


def moments_fsum(x, w, used, n_used):
    """x [n,16], w [n], used [n] (the counted samples: w is not looked at elsewhere) -> M [16,16]: fsum of the rounded products
    (w x_i) x_j, i <= j mirrored, and S = sum |(w x_i) x_j|"""
    M = np.zeros((16, 16))
    S = np.zeros((16, 16))
    for i in range(n_used):
        with np.errstate(all="ignore"):
            wx = np.where(used, w * x[:, i], 0.0)
        for j in range(i, n_used):
            with np.errstate(all="ignore"):
                prod = wx * x[:, j]
            m = math.fsum(prod) if np.isfinite(prod).all() else float(np.sum(prod))
            M[i, j] = M[j, i] = m
            S[i, j] = S[j, i] = float(np.sum(np.abs(prod)))
    return M, S


# ---- the solve ------------------------------------------------------------------------------------------------------------------------
def ridge_lambda(M, K, ridge):
    tr = np.float64(0.0)
    for k in range(K):
        tr = tr + np.float64(M[k, k])
    return (np.float64(ridge) * tr) / np.float64(K)


def e1_of(M, K, x32):
    """E1 = (E0 - 2 S1) + S2 in the header's order, on the fp32 coefficients widened and the unridged G"""
    a = np.asarray(x32, F).astype(np.float64)
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


def solve_unit(M, K, ridge, count, fallback=None):
    """-> (coefficients fp32 [K], E0, E1, ok) by the header's rules"""
    M = np.asarray(M, np.float64)
    E0 = M[K, K]
    fb = np.zeros(K, F) if fallback is None else np.asarray(fallback, F)
    fail = (fb, E0, E0, 0.0)
    if not (count > 0 and np.isfinite(M[:K + 1, :K + 1]).all()):
        return fail
    Gp = M[:K, :K] + ridge_lambda(M, K, ridge) * np.eye(K)
    try:
        L = np.linalg.cholesky(Gp)
    except np.linalg.LinAlgError:
        return fail
    piv = np.diag(L) ** 2
    if not (np.isfinite(piv).all() and (piv > PIVOT_TOL * np.diag(Gp)).all()):
        return fail
    sol = np.linalg.solve(L.T, np.linalg.solve(L, M[:K, K]))
    if not np.isfinite(sol).all():
        return fail
    s32 = sol.astype(F)
    return s32, E0, e1_of(M, K, s32), 1.0


def light_fit_ref(tex_img, normal, tri_ind, target, weight=None, gate_light=None, gain=1.0, offset=0.0, ridge=0.0):
    """-> (light [B,3,9] fp32, stats [B,3,4], M [B,3,16,16], S [B,3,16,16])"""
    x, w, counted = light_x(tex_img, normal, tri_ind, target, weight, gate_light, gain, offset)
    B = x.shape[0]
    light, stats = np.zeros((B, 3, 9), F), np.zeros((B, 3, 4))
    M, S = np.zeros((B, 3, 16, 16)), np.zeros((B, 3, 16, 16))
    for b in range(B):
        for c in range(3):
            M[b, c], S[b, c] = moments_fsum(x[b, c], w[b], counted[b, c], NL + 1)
            cnt = float(counted[b, c].sum())
            light[b, c], E0, E1, ok = solve_unit(M[b, c], NL, ridge, cnt, None if gate_light is None else np.asarray(gate_light, F)[b, c])
            stats[b, c] = (cnt, E0, E1, ok)
    return light, stats, M, S


def albedo_fit_ref(basis, tri_ind, normal, light, target, weight=None, gain=1.0, offset=0.0, ridge=0.0):
    """-> (alpha [B,K] fp32, stats [B,4], M [B,16,16], S [B,16,16])"""
    K = np.asarray(basis).shape[2] - 1
    x, w, counted = albedo_x(basis, tri_ind, normal, light, target, weight, gain, offset)
    B, npix = w.shape
    alpha, stats = np.zeros((B, K), F), np.zeros((B, 4))
    M, S = np.zeros((B, 16, 16)), np.zeros((B, 16, 16))
    for b in range(B):
        M[b], S[b] = moments_fsum(x[b].reshape(npix * 3, 16), np.repeat(w[b], 3), np.repeat(counted[b], 3), K + 1)
        cnt = float(counted[b].sum())
        alpha[b], E0, E1, ok = solve_unit(M[b], K, ridge, cnt)
        stats[b] = (cnt, E0, E1, ok)
    return alpha, stats, M, S


def solve_loop_ref(basis, tri_ind, normal, target, weight=None, alpha0=None, light0=None, iters=8, gate=True, ridge_light=0.0,
                   ridge_alpha=0.0, gain=1.0, offset=0.0):
    """rendering_layer.ops.photo_solve_rgb in the model -> (light, alpha, tex_img, E [iters,2,B], ok [iters,2,B])"""
    B = np.shape(tri_ind)[0]
    K = np.asarray(basis).shape[2] - 1
    alpha = np.zeros((B, K), F) if alpha0 is None else np.asarray(alpha0, F)
    light = None if light0 is None else np.asarray(light0, F)
    E, ok = np.zeros((iters, 2, B)), np.zeros((iters, 2, B), bool)
    for it in range(iters):
        tex = image_ref(basis, tri_ind, alpha)
        new, st, _, _ = light_fit_ref(tex, normal, tri_ind, target, weight, light if gate else None, gain, offset, ridge_light)
        good = st[:, :, 3] > 0
        light = new if light is None else np.where(good[:, :, None], new, light)
        E[it, 0], ok[it, 0] = st[:, :, 2].sum(1), good.all(1)
        new, st, _, _ = albedo_fit_ref(basis, tri_ind, normal, light, target, weight, gain, offset, ridge_alpha)
        good = st[:, 3] > 0
        alpha = np.where(good[:, None], new, alpha)
        E[it, 1], ok[it, 1] = st[:, 2], good
    return light, alpha, image_ref(basis, tri_ind, alpha), E, ok


# ---- the standard inputs --------------------------------------------------------------------------------------------------------------
STD_B, STD_S, STD_K = 3, 32, 10
STD_LIGHT_SEED = 3


def std_pc_tex(assets, K=STD_K, seed=1234):
    N = np.asarray(assets["mu"]).size // 3
    return (0.05 * np.random.RandomState(seed).standard_normal((3 * N, K))).astype(F)


def std_alpha_star(B=STD_B, K=STD_K, seed=14):
    return np.random.RandomState(seed).standard_normal((B, K)).astype(F)


def std_light(B=STD_B, seed=STD_LIGHT_SEED):
    """uniform in the RGB ranges of the sampler -> [B,3,9] fp32"""
    rg = np.asarray(LIGHT_RANGES_RGB, np.float64).reshape(3, 9, 2)
    u = np.random.RandomState(seed).uniform(size=(B, 3, 9))
    return (rg[None, ..., 0] + (rg[None, ..., 1] - rg[None, ..., 0]) * u).astype(F)


def std_target(basis, tri_ind, normal, light, alpha, gain=1.0, offset=0.0):
    """the fp32 shader's image of the model's own albedo plane: [B,H,W,3] fp32, 0 at an uncovered pixel"""
    tex = image_ref(basis, tri_ind, alpha)
    st = shade_terms(tex, normal, tri_ind, light, gain, offset)
    return np.where(st["covered"][..., None], st["im"], F(0.0)).astype(F), tex, st
