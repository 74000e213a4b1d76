"""The numpy model of the colour shading (include/fr_hotpath.h, "colour shading"): the float32 shader with its gray plane, the
lighting's Philox sampler, the 29 float64 sums in the gray loss's association, and the backward.  It shares no code with the kernels;
of tests/ref_photo_loss.py it takes the stated association (`associate`, `geom`) and nothing else.  numpy fuses nothing and rounds every
product and sum on its own, which is what the kernels do.  Also the planes the tests share."""
import ctypes

import numpy as np

from conftest import pkg
from ref_photo_loss import associate, geom  # noqa: F401  (the association is the gray loss's: stated there once)

F = np.float32
EPS = F(1e-6)
NS = 29
GRAY = (F(0.3), F(0.59), F(0.11))
# the ranges of rendering_layer.ops.SYNTH_LIGHT_RANGES_RGB, stated here on their own
LIGHT_RANGES_RGB = tuple(((0.3, 0.7), (-0.4, 0.4), (-0.4, 0.4), (0.2, 0.9))[k] if k < 4 else (-0.15, 0.15) for c in range(3) for k in range(9))


def geom_rgb(B, H, W):
    """fr_debug_photo_loss_rgb_geom -> [pixels per tile, tiles per face, finish threads, sums per face]"""
    out = (ctypes.c_int * 4)()
    pkg("_lib").lib().fr_debug_photo_loss_rgb_geom(B, H, W, out)
    return list(out)


def _flat(x, shape):
    return np.asarray(x, F).reshape(shape)


# ---- the float32 shader ---------------------------------------------------------------------------------------------------------------
def shade_terms(tex_img, normal, tri_ind, light, gain=1.0, offset=0.0, F=F):
    """the fp32 chain per pixel -> dict: a, s, im [B,H,W,3], n (flipped), nh [B,H,W,3], H [B,H,W,9], mag, d [B,H,W] float32 and the bool
    planes covered, flipped, unit.  F=np.float64: the same chain with no fp32 rounding (the derivative test's)."""
    EPS = F(1e-6)
    t = np.asarray(tex_img, F)
    n = np.asarray(normal, F)
    B, H, W = t.shape[:3]
    ti = np.asarray(tri_ind, F).reshape(B, H, W)
    l = np.asarray(light, F).reshape(B, 1, 1, 3, 9)
    gain, offset = F(gain), F(offset)
    with np.errstate(all="ignore"):
        a = np.where(t < EPS, EPS, t)
        flipped = n[..., 2] < 0
        n = np.where(flipped[..., None], -n, n)
        mag = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        unit = ~(mag > EPS)
        mag = np.where(unit, F(1.0), mag)
        d = np.sqrt(mag) + EPS
        nh = n / d[..., None]
        hx, hy, hz = nh[..., 0], nh[..., 1], nh[..., 2]
        Hb = np.stack([np.ones_like(hx), hx, hy, hz, hx * hy, hx * hz, hy * hz, hx * hx - hy * hy, F(3.0) * (hz * hz) - F(1.0)], -1)
        s = l[..., 0] + l[..., 1] * Hb[..., None, 1]
        for k in range(2, 9):
            s = s + l[..., k] * Hb[..., None, k]
        im = (a * np.where(s < 0, F(0.0), s)) * gain + offset
    for x in (a, n, mag, d, nh, Hb, s, im):
        assert x.dtype == F
    return dict(a=a, n=n, nh=nh, H=Hb, mag=mag, d=d, s=s, im=im, covered=ti >= 0, flipped=flipped, unit=unit)


def gray_of(rgb):
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return (GRAY[0] * rgb[..., 0] + GRAY[1] * rgb[..., 1]) + GRAY[2] * rgb[..., 2]


def shade(tex_img, normal, tri_ind, light, background=None, gain=1.0, offset=0.0):
    """-> (im_rgb [B,H,W,3], im_gray [B,H,W,1], mask [B,H,W,1]) float32; background None, [1,H,W,3] or [B,H,W,3]"""
    st = shade_terms(tex_img, normal, tri_ind, light, gain, offset)
    cov = st["covered"]
    bg = np.zeros(st["im"].shape, F) if background is None else np.broadcast_to(np.asarray(background, F), st["im"].shape)
    im = np.where(cov[..., None], st["im"], bg).astype(F)
    return im, gray_of(im)[..., None], cov.astype(F)[..., None]


# ---- the float64 sums and the backward ----------------------------------------------------------------------------------------------------
def pixel_terms(tex_img, normal, tri_ind, light, target, weight=None, gain=1.0, offset=0.0, F=F):
    """-> (shade terms, r [B,H,W,3], w [B,H,W], t [B,H,W,3]): float64"""
    st = shade_terms(tex_img, normal, tri_ind, light, gain, offset, F)
    shape = st["mag"].shape
    w = np.ones(shape, np.float64) if weight is None else _flat(weight, shape).astype(np.float64)
    with np.errstate(all="ignore"):
        r = st["im"].astype(np.float64) - np.asarray(target, F).reshape(shape + (3,)).astype(np.float64)
        t = ((2.0 * w)[..., None] * r) * np.float64(F(gain))
    return st, r, w, t


def forward(tex_img, normal, tri_ind, light, target, weight=None, gain=1.0, offset=0.0):
    """-> sums [B,29] float64: sse, cnt, L[c][k] at 2 + 9 c + k"""
    st, r, w, t = pixel_terms(tex_img, normal, tri_ind, light, target, weight, gain, offset)
    B = r.shape[0]
    cov = st["covered"]
    H64 = st["H"].astype(np.float64)
    with np.errstate(all="ignore"):
        wr = [(w * r[..., c]) * r[..., c] for c in range(3)]
        planes = [(wr[0] + wr[1]) + wr[2], np.ones_like(w)]
        for c in range(3):
            u = np.where(st["s"][..., c] > 0, t[..., c] * st["a"][..., c].astype(np.float64), 0.0)
            planes.append(u)
            planes += [u * H64[..., k] for k in range(1, 9)]
        assert len(planes) == NS
        return np.stack([associate(np.where(cov, p, 0.0).reshape(B, -1)) for p in planes], 1)


def backward(tex_img, normal, tri_ind, light, target, grad_sse, weight=None, gain=1.0, offset=0.0, sums=None, rounded=True, F=F):
    """-> (grad_tex_img [B,H,W,3], grad_normal [B,H,W,3], grad_light [B,3,9], A [B,H,W]) -- A is the magnitude the normal gradient's
    bound is stated in, (|g~|_1 + |n|_1 |n . g~| / (d rho)) / d with the colour g~.  rounded=False: the float64 values before the one
    fp32 rounding.  F=np.float64 (with rounded=False): the same formulas on a shading chain with no fp32 rounding either -- the
    derivative of forward64 up to float64 rounding; grad_light is then summed plainly, not in the stated association."""
    st, r, w, t = pixel_terms(tex_img, normal, tri_ind, light, target, weight, gain, offset, F)
    if sums is None and F is np.float32:
        sums = forward(tex_img, normal, tri_ind, light, target, weight, gain, offset)
    g = np.asarray(grad_sse, np.float64)
    B = g.shape[0]
    tex = np.asarray(tex_img, F)
    EPS = F(1e-6)
    l = np.asarray(light, F).astype(np.float64).reshape(B, 1, 1, 3, 9)
    cov, lit = st["covered"], st["s"] > 0
    with np.errstate(all="ignore"):
        dI = g[:, None, None, None] * t
        gt = np.where(cov[..., None] & lit & ~(tex < EPS), dI * st["s"].astype(np.float64), 0.0)
        q = np.where(lit, dI * st["a"].astype(np.float64), 0.0)
        nh = st["nh"].astype(np.float64)
        hx, hy, hz = nh[..., 0:1], nh[..., 1:2], nh[..., 2:3]
        dx = ((l[..., 1] + l[..., 4] * hy) + l[..., 5] * hz) + (2.0 * l[..., 7]) * hx
        dy = ((l[..., 2] + l[..., 4] * hx) + l[..., 6] * hz) - (2.0 * l[..., 7]) * hy
        dz = ((l[..., 3] + l[..., 5] * hx) + l[..., 6] * hy) + (6.0 * l[..., 8]) * hz
        gv = np.zeros(nh.shape, np.float64)
        for c in range(3):
            gv[..., 0] = gv[..., 0] + q[..., c] * dx[..., c]
            gv[..., 1] = gv[..., 1] + q[..., c] * dy[..., c]
            gv[..., 2] = gv[..., 2] + q[..., c] * dz[..., c]
        n = st["n"].astype(np.float64)
        d = st["d"].astype(np.float64)
        rho = np.sqrt(st["mag"].astype(np.float64))
        dot = (n[..., 0] * gv[..., 0] + n[..., 1] * gv[..., 1]) + n[..., 2] * gv[..., 2]
        c_ = dot / (d * rho)
        kept = (gv - n * c_[..., None]) / d[..., None]
        gn = np.where(st["unit"][..., None], gv / d[..., None], kept)
        gn = np.where(st["flipped"][..., None], -gn, gn)
        gn = np.where(cov[..., None], gn, 0.0)
        A = (np.abs(gv).sum(-1) + np.where(st["unit"], 0.0, np.abs(n).sum(-1) * np.abs(dot) / (d * rho))) / d
        A = np.where(cov, A, 0.0)
        if sums is None:   # (F = float64) the lighting sums of this chain, summed plainly
            u = np.where(cov[..., None] & lit, t * st["a"].astype(np.float64), 0.0)
            sums = np.concatenate([np.zeros((B, 2)), np.einsum("bhwc,bhwk->bck", u, st["H"].astype(np.float64)).reshape(B, 27)], 1)
        gl = (g[:, None] * sums[:, 2:NS]).reshape(B, 3, 9)
        if rounded:
            return gt.astype(F), gn.astype(F), gl.astype(F), A
    return gt, gn, gl, A


def forward64(tex, nrm, covered, light, target, weight, gain, offset):
    """the same loss evaluated wholly in float64 (no fp32 rounding, no stated association): what central differences are taken of.
    tex, nrm, target [B,H,W,3], light [B,3,9], weight, covered [B,H,W]; -> sse [B]"""
    a = np.where(tex < 1e-6, 1e-6, tex)
    n = np.where(nrm[..., 2:3] < 0, -nrm, nrm)
    mag = (n * n).sum(-1)
    mag = np.where(mag > 1e-6, mag, 1.0)
    nh = n / (np.sqrt(mag) + 1e-6)[..., None]
    hx, hy, hz = nh[..., 0], nh[..., 1], nh[..., 2]
    Hb = np.stack([np.ones_like(hx), hx, hy, hz, hx * hy, hx * hz, hy * hz, hx * hx - hy * hy, 3.0 * hz * hz - 1.0], -1)
    s = np.einsum("bck,bhwk->bhwc", light, Hb)
    im = a * np.maximum(s, 0.0) * gain + offset
    r = im - target
    return np.where(covered, weight * (r * r).sum(-1), 0.0).reshape(r.shape[0], -1).sum(1)


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words, key: two ints -> four uint64 arrays (Salmon et al., SC'11)"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in ctr)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK)
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def sample_light(seed, first_face, B, ranges=LIGHT_RANGES_RGB):
    """fr_synth_light_rgb -> light [B,3,9] float32: counter (j >> 2, g lo, g hi, 1), j = 9 c + k, word j & 3"""
    seed, first_face = int(seed) & (2 ** 64 - 1), int(first_face) & (2 ** 64 - 1)
    rg = np.asarray(ranges, F).reshape(27, 2)
    out = np.zeros((B, 27), F)
    j = np.arange(27, dtype=np.uint64)
    for b in range(B):
        g = (first_face + b) & (2 ** 64 - 1)
        w = philox4x32_10((j >> np.uint64(2), np.full(27, g & 0xFFFFFFFF, np.uint64), np.full(27, g >> 32, np.uint64),
                           np.full(27, 1, np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
        word = np.stack(w, 1)[np.arange(27), (j & np.uint64(3)).astype(np.int64)]
        u = (word >> np.uint64(8)).astype(F) * F(2.0 ** -24)
        out[b] = rg[:, 0] + (rg[:, 1] - rg[:, 0]) * u
    assert out.dtype == F
    return out.reshape(B, 3, 9)


# ---- planes the tests share -----------------------------------------------------------------------------------------------------------------
def hand_planes_rgb(B, H, W, seed, nan=False):
    """planes that reach every branch -- n_z < 0, mag <= 1e-6, s_c < 0 and > 0 per channel (and mixed within a pixel), tex_c < 1e-6 per
    channel, background on every border and at inner pixels -- with an independent colour target and a weight plane.  Four inner
    pixels of face 0 are set by hand, so that the smallest shape reaches the rare branches too.  nan=True plants a NaN in tex_img of
    one covered pixel of the LAST face.  -> tex, nrm, ti [B,H,W,1], light [B,3,9], target [B,H,W,3], weight [B,H,W,1]"""
    rs = np.random.RandomState(seed)
    tex = rs.uniform(-0.2, 1.0, (B, H, W, 3)).astype(F)
    nrm = rs.standard_normal((B, H, W, 3)).astype(F)
    tiny = rs.uniform(size=(B, H, W)) < 0.1
    nrm[tiny] *= F(1e-4)
    ti = rs.randint(0, 500, (B, H, W, 1)).astype(F)
    ti[rs.uniform(size=(B, H, W)) < 0.2] = -1
    ti[:, 0], ti[:, -1], ti[:, :, 0], ti[:, :, -1] = -1, -1, -1, -1
    light = rs.uniform(-1, 1, (B, 3, 9)).astype(F)
    target = rs.uniform(0, 1, (B, H, W, 3)).astype(F)
    weight = rs.uniform(0.25, 2.0, (B, H, W, 1)).astype(F)
    ti[0, 1, 1, 0], nrm[0, 1, 1], tex[0, 1, 1] = 7, (0.3, -0.2, 0.9), (0.5, -0.1, 0.7)        # kept normal, one channel clamped
    ti[0, 1, 2, 0], nrm[0, 1, 2], tex[0, 1, 2] = 8, (-0.4, 0.5, -0.6), (0.25, 0.5, 0.75)      # flipped
    ti[0, 1, 3, 0], nrm[0, 1, 3] = 9, (3e-4, -2e-4, 1e-4)                                     # mag replaced by 1
    ti[0, 2, 2, 0] = -1                                                                        # an inner background pixel
    if nan:
        ti[B - 1, 2, 3, 0] = 3
        tex[B - 1, 2, 3, 1] = np.nan
    return tex, nrm, ti, light, target, weight


# the GPU tests' shapes -- one partial tile; two full tiles plus 49 pixels; sixteen full tiles; 257 tiles: one more than the finish
# workgroup's 256 threads -- and for each a seed whose planes reach every branch (tests/test_photo_rgb_cpu.py holds them to it)
SHAPES = [(1, 5, 6), (3, 33, 17), (2, 64, 64), (1, 257, 256)]
SEEDS = {(1, 5, 6): 8, (3, 33, 17): 5, (2, 64, 64): 6, (1, 257, 256): 1}

BRANCHES = ("flipped", "not flipped", "unit", "not unit") + tuple("%s %d" % (n, c) for c in range(3) for n in ("lit", "unlit", "clamped", "kept")) + (
    "mixed lit", "uncovered", "weighted")


def branches(tex, nrm, ti, light, weight=None):
    """which side of each clamp and of the lit / unlit branch the covered pixels of these planes reach -> dict over BRANCHES"""
    st = shade_terms(tex, nrm, ti, light)
    cov = st["covered"]
    low = np.asarray(tex, F) < EPS
    out = {"flipped": cov & st["flipped"], "not flipped": cov & ~st["flipped"], "unit": cov & st["unit"], "not unit": cov & ~st["unit"]}
    for c in range(3):
        out["lit %d" % c] = cov & (st["s"][..., c] > 0)
        out["unlit %d" % c] = cov & (st["s"][..., c] < 0)
        out["clamped %d" % c] = cov & low[..., c]
        out["kept %d" % c] = cov & ~low[..., c]
    lit = st["s"] > 0
    out["mixed lit"] = cov & lit.any(-1) & ~lit.all(-1)
    out["uncovered"] = np.pad(~cov[:, 1:-1, 1:-1], ((0, 0), (1, 1), (1, 1)))      # an INNER background pixel
    out["weighted"] = np.zeros(cov.shape, bool) if weight is None else cov & (_flat(weight, cov.shape) != 1)
    assert tuple(out) == BRANCHES
    return {k: bool(v.any()) for k, v in out.items()}


def reaches_every_branch(tex, nrm, ti, light, weight):
    cov = np.asarray(ti, F).reshape(np.shape(tex)[:3]) >= 0
    return bool(all(branches(tex, nrm, ti, light, weight).values()) and not cov[:, 0].any() and not cov[:, :, -1].any())


def smooth_case(B=2, H=6, W=7, seed=3):
    """inputs away from every kink (every s_c and tex_c - 1e-6 bounded away from 0, mag > 1e-3), exactly representable in fp32, with an
    independent target so that the residuals are O(1)"""
    rs = np.random.RandomState(seed)
    tex = rs.uniform(0.2, 1.0, (B, H, W, 3)).astype(F)
    nrm = rs.standard_normal((B, H, W, 3)).astype(F)
    nrm[..., 2] = np.where(np.abs(nrm[..., 2]) < 0.3, F(0.5), nrm[..., 2])        # away from the flip, and mag > 1e-3
    light = rs.uniform(-0.08, 0.08, (B, 3, 9)).astype(F)
    light[:, :, 0] = rs.uniform(0.9, 1.2, (B, 3)).astype(F)                          # |sum over k > 0 of l_k H_k| <= 0.08 (3 + 1.5 + 1 + 2) = 0.6
    ti = rs.randint(0, 50, (B, H, W, 1)).astype(F)
    ti[rs.uniform(size=(B, H, W)) < 0.25] = -1
    target = rs.uniform(-1, 2, (B, H, W, 3)).astype(F)
    weight = rs.uniform(0.5, 1.5, (B, H, W, 1)).astype(F)
    return tex, nrm, ti, light, target, weight
