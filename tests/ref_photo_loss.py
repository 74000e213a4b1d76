"""The numpy model of the photometric loss (include/fr_hotpath.h, "photometric loss") and of the albedo blend's adjoint ("synthetic
batches", TEXTURE BACKWARD): the shader's float32 chain (the operations of tests/ref_synth_batch.py::shade, with the intermediates
kept), the six float64 sums in the header's association (tile and finish width read from fr_debug_photo_loss_geom), and the backward.
numpy fuses nothing and rounds every float64 product and sum on its own, which is what the kernels do.  Also the planes the tests
share."""
import ctypes

import numpy as np

from conftest import pkg

F = np.float32
EPS = F(1e-6)
TX_ROWS = 256          # rows per tile of the blend's adjoint (the header states it)


def geom(B, H, W):
    """fr_debug_photo_loss_geom -> [pixels per tile, tiles per face, finish threads, sums per face]"""
    out = (ctypes.c_int * 4)()
    pkg("_lib").lib().fr_debug_photo_loss_geom(B, H, W, out)
    return list(out)


def flat(x, shape):
    """[B,H,W] or [B,H,W,1] -> [B,H,W] float32"""
    return np.asarray(x, F).reshape(shape)


def shade_terms(tex_img, normal, tri_ind, light, gain=1.0, offset=0.0):
    """the fp32 chain per pixel -> dict of [B,H,W] float32 planes (a, n flipped [..,3], nh [..,3], mag, d, s, im) and the bool planes
    covered, flipped, unit"""
    t = np.asarray(tex_img, F)
    n = np.asarray(normal, F)
    B, H, W = t.shape[:3]
    ti = flat(tri_ind, (B, H, W))
    l = np.asarray(light, F)[:, None, None, :]
    gain, offset = F(gain), F(offset)
    with np.errstate(all="ignore"):
        m = np.where(t < EPS, EPS, t)
        a = ((m[..., 0] + m[..., 1]) + m[..., 2]) / F(3.0)
        flipped = n[..., 2] < 0
        n = np.where(flipped[..., None], -n, n)
        mag = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        unit = ~(mag > EPS)
        mag = np.where(unit, F(1.0), mag)
        d = np.sqrt(mag) + EPS
        nh = n / d[..., None]
        s = ((l[..., 0] + l[..., 1] * nh[..., 0]) + l[..., 2] * nh[..., 1]) + l[..., 3] * nh[..., 2]
        im = (a * np.where(s < 0, F(0.0), s)) * gain + offset
    for x in (a, n, mag, d, nh, s, im):
        assert x.dtype == F
    return dict(a=a, n=n, nh=nh, mag=mag, d=d, s=s, im=im, covered=ti >= 0, flipped=flipped, unit=unit)


def pixel_terms(tex_img, normal, tri_ind, light, target, weight=None, gain=1.0, offset=0.0):
    """-> (shade terms, r, w, t): float64 planes"""
    st = shade_terms(tex_img, normal, tri_ind, light, gain, offset)
    shape = st["a"].shape
    w = np.ones(shape, np.float64) if weight is None else flat(weight, shape).astype(np.float64)
    with np.errstate(all="ignore"):
        r = st["im"].astype(np.float64) - flat(target, shape).astype(np.float64)
        t = ((2.0 * w) * r) * np.float64(F(gain))
    return st, r, w, t


def _tree64(v):
    v = v.copy()
    k = 32
    while k >= 1:
        v[..., :k] = v[..., :k] + v[..., k:2 * k]
        k //= 2
    return v[..., 0]


def _tree4(w):
    return (w[..., 0] + w[..., 2]) + (w[..., 1] + w[..., 3])


def block_tree(v):
    """[..., 256] float64 -> [...]: groups of 64 with k = 32 .. 1, then (w0 + w2) + (w1 + w3)"""
    return _tree4(_tree64(v.reshape(v.shape[:-1] + (4, 64))))


def associate(terms):
    """[B, HW] float64 terms (+0.0 where nothing contributes) -> [B] in the header's association"""
    B, HW = terms.shape
    T, tiles, Fin, _ = geom(B, 1, HW)
    assert T == 256 and Fin == 256 and tiles == -(-HW // T)
    pad = np.zeros((B, tiles * T), np.float64)
    pad[:, :HW] = terms
    with np.errstate(all="ignore"):
        part = block_tree(pad.reshape(B, tiles, T))                 # [B, tiles]
        rows = -(-tiles // Fin)
        acc = np.zeros((B, Fin), np.float64)
        for j in range(rows):                                        # thread i: chain over partial[i + F j] from +0.0
            chunk = part[:, j * Fin:(j + 1) * Fin]
            acc[:, :chunk.shape[1]] = acc[:, :chunk.shape[1]] + chunk
        return block_tree(acc)


def forward(tex_img, normal, tri_ind, light, target, weight=None, gain=1.0, offset=0.0):
    """-> sums [B,6] float64: sse, cnt, L0, L1, L2, L3"""
    st, r, w, t = pixel_terms(tex_img, normal, tri_ind, light, target, weight, gain, offset)
    B = r.shape[0]
    cov = st["covered"]
    with np.errstate(all="ignore"):
        u = np.where(st["s"] > 0, t * st["a"].astype(np.float64), 0.0)
        planes = [(w * r) * r, np.ones_like(r), u] + [u * st["nh"][..., k].astype(np.float64) for k in range(3)]
        return np.stack([associate(np.where(cov, p, 0.0).reshape(B, -1)) for p in planes], 1)


def backward(tex_img, normal, tri_ind, light, target, grad_sse, weight=None, gain=1.0, offset=0.0, sums=None, rounded=True):
    """-> (grad_tex_img [B,H,W,3], grad_normal [B,H,W,3], grad_light [B,4], A [B,H,W]) -- A is the magnitude the normal gradient's
    bound is stated in, (|g~|_1 + |n|_1 |n . g~| / (d rho)) / d.  rounded=False: the float64 values before the one fp32 rounding."""
    st, r, w, t = pixel_terms(tex_img, normal, tri_ind, light, target, weight, gain, offset)
    if sums is None:
        sums = forward(tex_img, normal, tri_ind, light, target, weight, gain, offset)
    g = np.asarray(grad_sse, np.float64)
    tex = np.asarray(tex_img, F)
    l = np.asarray(light, F).astype(np.float64)[:, None, None, :]
    cov, lit = st["covered"], st["s"] > 0
    with np.errstate(all="ignore"):
        dI = g[:, None, None] * t
        gc = (dI * st["s"].astype(np.float64)) * (1.0 / 3.0)
        gt = np.where((cov & lit)[..., None] & ~(tex < EPS), gc[..., None], 0.0)
        q = np.where(lit, dI * st["a"].astype(np.float64), 0.0)
        gv = q[..., None] * l[..., 1:4]
        n = st["n"].astype(np.float64)
        d = st["d"].astype(np.float64)
        rho = np.sqrt(st["mag"].astype(np.float64))
        dot = (n[..., 0] * gv[..., 0] + n[..., 1] * gv[..., 1]) + n[..., 2] * gv[..., 2]
        c = dot / (d * rho)
        kept = (gv - n * c[..., None]) / d[..., None]
        gn = np.where(st["unit"][..., None], gv / d[..., None], kept)
        gn = np.where(st["flipped"][..., None], -gn, gn)
        gn = np.where(cov[..., None], gn, 0.0)
        A = (np.abs(gv).sum(-1) + np.where(st["unit"], 0.0, np.abs(n).sum(-1) * np.abs(dot) / (d * rho))) / d
        A = np.where(cov, A, 0.0)
        gl = g[:, None] * sums[:, 2:6]
        if rounded:
            return gt.astype(F), gn.astype(F), gl.astype(F), A
    return gt, gn, gl, A


def forward64(tex, nrm, covered, light, target, weight, gain, offset):
    """the same loss evaluated wholly in float64 (no fp32 rounding, no stated association): what central differences are taken of.
    Inputs float64; -> sse [B]"""
    m = np.where(tex < 1e-6, 1e-6, tex)
    a = m.sum(-1) / 3.0
    n = np.where(nrm[..., 2:3] < 0, -nrm, nrm)
    mag = (n * n).sum(-1)
    mag = np.where(mag > 1e-6, mag, 1.0)
    nh = n / (np.sqrt(mag) + 1e-6)[..., None]
    l = light[:, None, None, :]
    s = l[..., 0] + (l[..., 1:4] * nh).sum(-1)
    im = a * np.maximum(s, 0.0) * gain + offset
    r = im - target
    return np.where(covered, weight * r * r, 0.0).reshape(r.shape[0], -1).sum(1)


# ---- the blend's adjoint ------------------------------------------------------------------------------------------------------------------
def texture_backward(pc_tex, grad_tex, rounded=True):
    """pc_tex [3N,K], grad_tex [B,3,N] -> grad_alpha [B,K]: exact float64 products, the tile tree, the tiles' partials in 64 chains and
    one more tree"""
    pc = np.asarray(pc_tex, F).astype(np.float64)
    R, K = pc.shape
    g = np.asarray(grad_tex, F).astype(np.float64).reshape(-1, R)
    B = g.shape[0]
    tiles = -(-R // TX_ROWS)
    prod = np.zeros((B, K, tiles * TX_ROWS), np.float64)
    with np.errstate(all="ignore"):
        prod[:, :, :R] = g[:, None, :] * pc.T[None, :, :]
        part = block_tree(prod.reshape(B, K, tiles, TX_ROWS))       # [B, K, tiles]
        acc = np.zeros((B, K, 64), np.float64)                       # lane i: chain over the tiles i, i + 64, .. from +0.0
        for j in range(-(-tiles // 64)):
            chunk = part[:, :, j * 64:(j + 1) * 64]
            acc[:, :, :chunk.shape[2]] = acc[:, :, :chunk.shape[2]] + chunk
        acc = _tree64(acc)
        return acc.astype(F) if rounded else acc


# ---- planes the tests share -----------------------------------------------------------------------------------------------------------------
def hand_planes(B, H, W, seed, nan=False):
    """planes in the style of tests/test_synth_batch_gpu.py::_hand_planes that reach every branch -- n_z < 0, mag <= 1e-6, s < 0,
    tex < 1e-6, background on every border and at scattered inner pixels -- plus an independent target and a weight plane.
    nan=True plants a NaN in tex_img of one covered pixel of the LAST face."""
    rs = np.random.RandomState(seed)
    tex = rs.uniform(-0.2, 1.0, (B, H, W, 3)).astype(F)
    nrm = rs.standard_normal((B, H, W, 3)).astype(F)
    tiny = rs.uniform(size=(B, H, W)) < 0.1
    nrm[tiny] *= F(1e-4)
    ti = rs.randint(0, 500, (B, H, W, 1)).astype(F)
    ti[rs.uniform(size=(B, H, W)) < 0.2] = -1
    ti[:, 0], ti[:, -1], ti[:, :, 0], ti[:, :, -1] = -1, -1, -1, -1
    light = rs.uniform(-1, 1, (B, 4)).astype(F)
    target = rs.uniform(0, 1, (B, H, W, 1)).astype(F)
    weight = rs.uniform(0.25, 2.0, (B, H, W, 1)).astype(F)
    if nan:
        ti[B - 1, 2, 2, 0] = 3
        tex[B - 1, 2, 2, 1] = np.nan
    return tex, nrm, ti, light, target, weight


BRANCHES = ("flipped", "not flipped", "unit", "not unit", "unlit", "lit", "tex clamped", "tex kept")


def branches(tex, nrm, ti, light):
    """which side of each clamp and of the lit / unlit branch the covered pixels of these planes reach -> dict over BRANCHES"""
    st = shade_terms(tex, nrm, ti, light)
    cov = st["covered"]
    low = np.asarray(tex, F) < EPS
    sides = ((cov & st["flipped"]), (cov & ~st["flipped"]), (cov & st["unit"]), (cov & ~st["unit"]), (cov & (st["s"] < 0)),
             (cov & (st["s"] > 0)), (cov & low.any(-1)), (cov & ~low.all(-1)))
    return {name: bool(side.any()) for name, side in zip(BRANCHES, sides)}


def reaches_every_branch(tex, nrm, ti, light):
    cov = np.asarray(ti, F).reshape(np.shape(tex)[:3]) >= 0
    return bool(all(branches(tex, nrm, ti, light).values()) and
                (~cov[:, 1:-1, 1:-1]).any() and not cov[:, 0].any() and not cov[:, :, -1].any())


def smooth_case(B=2, H=6, W=7, seed=3):
    """float64 inputs away from every kink (s and tex - 1e-6 bounded away from 0, mag > 1e-3), exactly representable in fp32, with
    an independent target so that the residuals are O(1)"""
    rs = np.random.RandomState(seed)
    tex = rs.uniform(0.2, 1.0, (B, H, W, 3)).astype(F)
    nrm = rs.standard_normal((B, H, W, 3)).astype(F)
    nrm[..., 2] = np.where(np.abs(nrm[..., 2]) < 0.3, F(0.5), nrm[..., 2])        # away from the flip, and mag > 1e-3
    light = np.stack([rs.uniform(0.8, 1.2, B), rs.uniform(-0.2, 0.2, B), rs.uniform(-0.2, 0.2, B), rs.uniform(0.1, 0.3, B)], 1).astype(F)
    ti = rs.randint(0, 50, (B, H, W, 1)).astype(F)
    ti[rs.uniform(size=(B, H, W)) < 0.25] = -1
    target = rs.uniform(-1, 2, (B, H, W, 1)).astype(F)
    weight = rs.uniform(0.5, 1.5, (B, H, W, 1)).astype(F)
    return tex, nrm, ti, light, target, weight
