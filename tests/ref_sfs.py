"""numpy float64 model of the shape-from-shading term (fr_sfs_intensity_forward / _backward), written from the section
"shape-from-shading term" of include/fr_hotpath.h alone; it shares no code with the product.  TEST INFRASTRUCTURE ONLY.

Per pixel, on the fp32 inputs widened to float64:
    u_b = I_b / (a_b + 1)      M = sum_b n_b n_b^T      r = sum_b n_b u_b
    P = sum over the kept eigenpairs of v v^T / lambda   (kept: lambda > rcond * lambda_max and lambda > 0)      l = P r
    intensity_b = fl32(a'_b (l . n'_b))
backward with P held constant:  q = sum_b (g_b a'_b) n'_b,  s = P q,  grad_normal_b = fl32(u_b s),  grad_normal_new_b = fl32((g_b a'_b) l)
The sums here are numpy's; the kernel's association differs, which is what the 2^-40 terms of the GPU bounds are for."""
import collections

import numpy as np

CASES = ((6, 5, 4), (64, 9, 70), (65, 3, 67), (1, 4, 4))     # (B, H, W); seed 1 satisfies the gap condition on each
RCOND = 1e-6
GAP_HI, GAP_LO = 1e-3, 1e-9

Model = collections.namedtuple("Model", "intensity P l rank lam u M r")


def _planes(abedo, normal, im_gray):
    a = np.asarray(abedo, np.float32).astype(np.float64)[..., 0]                 # [B,H,W]
    I = np.asarray(im_gray, np.float32).astype(np.float64)[..., 0]
    n = np.asarray(normal, np.float32).astype(np.float64)                          # [B,H,W,3]
    return a, n, I


def model(abedo, normal, im_gray, abedo_new, normal_new, rcond=RCOND):
    """-> Model(intensity [B,H,W,1] float64 BEFORE its rounding to fp32, P [H,W,3,3], l [H,W,3], rank [H,W], lam [H,W,3] ascending,
    u [B,H,W], M [H,W,3,3], r [H,W,3])"""
    a, n, I = _planes(abedo, normal, im_gray)
    a2, n2, _ = _planes(abedo_new, normal_new, im_gray)
    u = I / (a + 1.0)
    M = np.einsum("bhwi,bhwj->hwij", n, n)
    r = np.einsum("bhwi,bhw->hwi", n, u)
    lam, V = np.linalg.eigh(M)                                                     # ascending; columns are eigenvectors
    lmax = lam[..., 2:3]
    keep = (lam > rcond * lmax) & (lam > 0)
    inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)
    P = np.einsum("hwik,hwk,hwjk->hwij", V, inv, V)
    l = np.einsum("hwij,hwj->hwi", P, r)
    inten = a2 * np.einsum("hwi,bhwi->bhw", l, n2)
    return Model(inten[..., None], P, l, keep.sum(-1), lam, u, M, r)


def grads(g, abedo, normal, im_gray, abedo_new, normal_new, rcond=RCOND, m=None):
    """-> (grad_normal, grad_normal_new) [B,H,W,3] float64 before rounding, and (q [H,W,3], ga [B,H,W]) for the bounds"""
    m = model(abedo, normal, im_gray, abedo_new, normal_new, rcond) if m is None else m
    a2, n2, _ = _planes(abedo_new, normal_new, im_gray)
    ga = np.asarray(g, np.float32).astype(np.float64)[..., 0] * a2
    q = np.einsum("bhw,bhwi->hwi", ga, n2)
    s = np.einsum("hwij,hwj->hwi", m.P, q)
    return m.u[..., None] * s[None], ga[..., None] * m.l[None], q, ga


def p6(P):
    """[H,W,3,3] -> the six state planes xx, xy, xz, yy, yz, zz"""
    return np.stack([P[..., 0, 0], P[..., 0, 1], P[..., 0, 2], P[..., 1, 1], P[..., 1, 2], P[..., 2, 2]])


def check_gap(lam, rcond=RCOND):
    """the gap condition: every eigenvalue ratio is above 1e-3 or below 1e-9 (in magnitude), so keeping at `rcond` is unambiguous"""
    assert GAP_LO < rcond < GAP_HI
    lmax = lam.max(-1, keepdims=True)
    ratio = np.abs(lam) / np.where(lmax > 0, lmax, 1.0)
    ok = (ratio > GAP_HI) | (ratio < GAP_LO)
    assert ok.all(), ("gap condition violated at", np.argwhere(~ok)[:4], ratio[~ok][:4])


def inputs(B, H, W, seed=1):
    """The generator of the issue, steps 1-7 -> dict of fp32 arrays (abedo, normal, im_gray, abedo_new, normal_new)."""
    rs = np.random.RandomState(seed)
    n = rs.standard_normal((B, H, W, 3))
    n[..., 2] = np.abs(n[..., 2])
    n = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(np.float32)
    n[rs.uniform(size=(B, H, W)) < 0.2] = 0                                        # uncovered (face, pixel) entries
    n[:, 0, 0] = 0                                                                 # nobody covers pixel (0,0)
    if W > 1:
        n[1:, 0, 1] = 0                                                            # only face 0 at (0,1)
    if W > 2:
        n[2:, 0, 2] = 0                                                            # only faces 0 and 1 at (0,2)
    if H > 1 and W > 1:
        n[:, 1, 1] = n[0, 1, 1]                                                    # every face has face 0's normal at (1,1)
    d = {"normal": n}
    for k in ("abedo", "abedo_new"):
        d[k] = rs.uniform(0.2, 0.8, (B, H, W, 1)).astype(np.float32)
    d["im_gray"] = rs.uniform(-0.5, 0.5, (B, H, W, 1)).astype(np.float32)
    n2 = rs.standard_normal((B, H, W, 3))
    n2[..., 2] = np.abs(n2[..., 2])
    d["normal_new"] = (n2 / np.sqrt((n2 * n2).sum(-1, keepdims=True))).astype(np.float32) * (n.any(-1, keepdims=True))
    m = model(d["abedo"], d["normal"], d["im_gray"], d["abedo_new"], d["normal_new"])
    check_gap(m.lam)
    return d


def grad_out(B, H, W, seed=1):
    """the seeded standard-normal g = dL / d intensity of the backward tests, fp32 [B,H,W,1]"""
    return np.random.RandomState(seed).standard_normal((B, H, W, 1)).astype(np.float32)


def args(d):
    return d["abedo"], d["normal"], d["im_gray"], d["abedo_new"], d["normal_new"]
