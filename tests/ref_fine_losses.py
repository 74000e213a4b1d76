"""The fine-depth losses (include/fr_hotpath.h, "fine-depth losses") in numpy float64, which fuses nothing: the Laplacian's chain, the
two sums in the header's association (the tile and the finish width read from fr_debug_fine_losses_geom), the outputs, the backward
bit by bit, and math.fsum values of the two sums for a bound that knows no association.  Also the inputs the tests share."""
import ctypes
import math

import numpy as np

from conftest import pkg

K = ((0.5, 1.0, 0.5), (1.0, -6.0, 1.0), (0.5, 1.0, 0.5))
GRADS = ((1.0, 1.0), (-0.37, 1e-3), (100.0, 1e-5))        # (g_f, g_s)


def geom(B, H, W):
    """fr_debug_fine_losses_geom -> [tile width, tile height, threads, tiles across, tiles down, finish threads, backward LDS bytes]"""
    out = (ctypes.c_int * 7)()
    pkg("_lib").lib().fr_debug_fine_losses_geom(B, H, W, out)
    return list(out)


def tile():
    g = geom(1, 1, 1)
    return g[0], g[1]


def shapes():
    """(B, H, W): the smallest shapes at which a kernel of TW x TH tiles with a 2-pixel halo can still go wrong -- images smaller than
    the halo, one tile exactly, one past a tile both ways, ragged multi-tile -- each at B in {1, 3}; and the model's image at B = 2"""
    tw, th = tile()
    hw = [(1, 1), (1, 5), (2, 2), (3, 3), (th, tw), (th + 1, tw + 1), (2 * th + 1, 2 * tw + 3)]
    return [(B, H, W) for H, W in hw for B in (1, 3)] + [(2, 200, 200)]


def case_id(s):
    return "B%d-%dx%d" % s


def inputs(B, H, W, seed=0, wide=False):
    """(z, c, planted): seeded fp32 depths; `planted` marks pixels whose Laplacian the inputs make exactly zero.
    wide=True: the random depths span 28 binades, so the Laplacian's partial sums round (depths of one binade add exactly).
    face 0: random depths with a constant patch and an integer-valued linear ramp where the image has room;
    face 1 (B > 1): all zero (every term of the chain is a signed zero); its c is random;
    face 2 (B > 2): random, and c == z there."""
    rs = np.random.RandomState(1000 * seed + 7 * H + W + 31 * B)
    z = (rs.standard_normal((B, H, W)) * 3.0 + 40.0).astype(np.float32)
    if wide:
        z = (rs.standard_normal((B, H, W)) * np.exp2(rs.randint(-20, 9, (B, H, W)))).astype(np.float32)
    c = (z + rs.standard_normal((B, H, W)).astype(np.float32) * 0.5).astype(np.float32)
    planted = np.zeros((B, H, W), bool)
    if H >= 8 and W >= 8:
        h2, w2 = H // 2, W // 2
        z[0, :h2, :w2] = np.float32(37.25)                       # constant patch; its interior (clear of the image's edge) has L == 0
        planted[0, 1:h2 - 1, 1:w2 - 1] = True
        rr, cc = np.mgrid[h2:H, w2:W]
        z[0, h2:, w2:] = (3 * rr - 2 * cc + 11).astype(np.float32)   # integer-valued linear ramp: every partial sum is exact
        planted[0, h2 + 1:H - 1, w2 + 1:W - 1] = True
    if B > 1:
        z[1] = 0.0
        planted[1] = True
    if B > 2:
        c[2] = z[2]
    return z, c, planted


def _shift(a, dr, dc):
    """a(p + (dr, dc)) and whether p + (dr, dc) lies inside the image, per face"""
    B, H, W = a.shape
    out = np.zeros_like(a)
    ok = np.zeros((H, W), bool)
    r0, r1 = max(0, -dr), min(H, H - dr)
    c0, c1 = max(0, -dc), min(W, W - dc)
    if r0 < r1 and c0 < c1:
        out[:, r0:r1, c0:c1] = a[:, r0 + dr:r1 + dr, c0 + dc:c1 + dc]
        ok[r0:r1, c0:c1] = True
    return out, ok


def laplacian(z):
    """L [B,H,W] float64: the nine taps in row-major order from +0.0, a tap outside the image not added"""
    z64 = z.astype(np.float64)
    L = np.zeros(z64.shape, np.float64)
    for i in range(3):
        for j in range(3):
            v, ok = _shift(z64, i - 1, j - 1)
            with np.errstate(invalid="ignore", over="ignore"):
                L = np.where(ok[None], L + K[i][j] * v, L)
    return L


def sign(x):
    """s(x) = (x > 0) - (x < 0): 0 at +-0 and at NaN"""
    with np.errstate(invalid="ignore"):
        return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def terms(z, c):
    """the two planes of terms, float64: (z - c)^2 and |L|"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = z.astype(np.float64) - c.astype(np.float64)
        return d * d, np.abs(laplacian(z))


def _tree64(v):
    """[..., 64] -> [...]: v[i] = v[i] + v[i + k] for i < k, k = 32 .. 1"""
    v = v.copy()
    k = 32
    while k >= 1:
        v[..., :k] = v[..., :k] + v[..., k:2 * k]
        k //= 2
    return v[..., 0]


def _tree(v):
    """[..., n] (n a power of two <= 64) -> [...], strides n/2 .. 1"""
    v = v.copy()
    k = v.shape[-1] // 2
    while k >= 1:
        v[..., :k] = v[..., :k] + v[..., k:2 * k]
        k //= 2
    return v[..., 0]


def associate(t):
    """one plane of terms [B,H,W] float64 -> (partials [P], S): the header's association"""
    B, H, W = t.shape
    tw, th, _, tx, ty, F, _ = geom(B, H, W)
    pad = np.zeros((B, ty * th, tx * tw), np.float64)              # a slot outside the image: +0.0
    pad[:, :H, :W] = t
    # [B, ty, th, tx, tw] -> [B, ty, tx, th * tw]: slot = row in tile * tw + column in tile; p = (face * ty + tile row) * tx + tile column
    slots = pad.reshape(B, ty, th, tx, tw).transpose(0, 1, 3, 2, 4).reshape(B * ty * tx, th * tw // 64, 64)
    with np.errstate(invalid="ignore", over="ignore"):
        part = _tree(_tree64(slots))
        P = part.shape[0]
        rows = -(-P // F)
        a = np.zeros((rows * F,), np.float64)
        a[:P] = part
        a = a.reshape(rows, F)
        acc = np.zeros((F,), np.float64)
        for j in range(rows):                                      # thread i: chain over partial[i + F j] from +0.0
            live = np.arange(F) + F * j < P
            acc = np.where(live, acc + a[j], acc)
        S = _tree(_tree64(acc.reshape(F // 64, 64)))
    return part, float(S)


def forward(z, c):
    """-> dict: part_f, part_s [P]; S_f, S_s (python floats); fidelity, smoothness (np.float32); fsum_f, fsum_s, abs_f, abs_s"""
    tf, ts = terms(z, c)
    part_f, S_f = associate(tf)
    part_s, S_s = associate(ts)
    n = float(z.shape[0]) * float(z.shape[1]) * float(z.shape[2])
    out = dict(part_f=part_f, part_s=part_s, S_f=S_f, S_s=S_s, n=n)
    with np.errstate(invalid="ignore", over="ignore"):
        out["fidelity"] = np.float32(np.float64(S_f) / n)
        out["smoothness"] = np.float32(np.float64(S_s))
    if np.isfinite(tf).all() and np.isfinite(ts).all():
        out["fsum_f"], out["fsum_s"] = math.fsum(tf.ravel().tolist()), math.fsum(ts.ravel().tolist())
    return out


def T_plane(z):
    """T [B,H,W] float64: the stencil over s(L), taps inside the image, row-major from +0.0 (exact)"""
    s = sign(laplacian(z))
    T = np.zeros(s.shape, np.float64)
    for i in range(3):
        for j in range(3):
            v, ok = _shift(s, i - 1, j - 1)
            T = np.where(ok[None], T + K[i][j] * v, T)
    return T


def backward(z, c, g_f, g_s, rounded=True):
    """(grad_pred, grad_coarse) as the header states them; g_f / g_s: a number (taken as fp32) or None = the term is absent.
    rounded=False: the float64 values before the one fp32 rounding."""
    B, H, W = z.shape
    cf = 2.0 / (float(B) * float(H) * float(W))
    with np.errstate(invalid="ignore", over="ignore"):
        fid = None
        if g_f is not None:
            fid = (np.float64(np.float32(g_f)) * cf) * (z.astype(np.float64) - c.astype(np.float64))
        sm = np.float64(np.float32(g_s)) * T_plane(z) if g_s is not None else None
        if fid is not None and sm is not None:
            gp = fid + sm
        elif fid is not None:
            gp = fid
        elif sm is not None:
            gp = sm
        else:
            gp = np.zeros(z.shape, np.float64)
        gc = -fid if fid is not None else np.zeros(z.shape, np.float64)
        if rounded:
            return gp.astype(np.float32), gc.astype(np.float32)
    return gp, gc
