"""The numpy model of the synthetic-batch kernels (include/fr_hotpath.h, "synthetic batches"): Philox4x32-10 on integers, and
float32 arithmetic in the header's written order -- every product, sum, quotient and root rounded on its own, which is what numpy
does with float32 operands.  tests/test_synth_batch_cpu.py holds the model to known answers and to the sampler's intervals;
tests/test_synth_batch_gpu.py holds the kernels to the model bit for bit."""
import numpy as np

F = np.float32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
C_DEG = F(np.pi / 180.0)          # fl32(pi / 180)
FOCAL = F(1e-3)
U_SCALE = F(2.0 ** -24)


def philox4x32_10(ctr, key):
    """ctr: four words, key: two words (python ints or uint64 arrays of one shape) -> four words"""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in ctr]
    k = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in key]
    m = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & m
        hi1, lo1 = p1 >> np.uint64(32), p1 & m
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & m, (k[1] + np.uint64(W1)) & m]
    return c


def n_draws(ns, ne, K):
    return 6 + ns + ne + 4 + K


def uniforms(seed, first_face, B, ndraw):
    """u [B, ndraw] float32 in [0, 1): draw j of global face g = first_face + b is word j & 3 of counter (j >> 2, g lo, g hi, 0)"""
    seed, first_face = int(seed) & (2 ** 64 - 1), int(first_face) & (2 ** 64 - 1)
    g = [(first_face + b) & (2 ** 64 - 1) for b in range(B)]
    glo = np.array([x & MASK for x in g], np.uint64)[:, None]
    ghi = np.array([x >> 32 for x in g], np.uint64)[:, None]
    nblk = (ndraw + 3) // 4
    blk = np.arange(nblk, dtype=np.uint64)[None, :]
    zero = np.zeros((B, nblk), np.uint64)
    w = philox4x32_10((blk + zero, glo + zero, ghi + zero, zero), (seed & MASK, seed >> 32))
    words = np.stack(w, -1).reshape(B, 4 * nblk)[:, :ndraw]
    return (words >> np.uint64(8)).astype(F) * U_SCALE


def sample(seed, first_face, B, ns, ne, K, im_size, beta, light_ranges, alpha_ranges, focal=FOCAL):
    """-> params [B, 7 + ns + ne], light [B, 4], alpha [B, K], u [B, draws]; all float32"""
    u = uniforms(seed, first_face, B, n_draws(ns, ne, K))
    beta, focal, half = F(beta), F(focal), F(im_size) * F(0.5)
    omb = F(1.0) - beta
    P = np.zeros((B, 7 + ns + ne), F)

    def mix(base, rnd):
        return beta * F(base) + omb * rnd
    P[:, 0] = mix(0.0, (F(-75.0) + F(120.0) * u[:, 0]) * C_DEG)
    P[:, 1] = mix(0.0, (F(-90.0) + F(180.0) * u[:, 1]) * C_DEG)
    P[:, 2] = mix(0.0, (F(-30.0) + F(60.0) * u[:, 2]) * C_DEG)
    P[:, 6] = mix(focal, u[:, 3] * focal)
    P[:, 3] = mix(half, F(60.0) * u[:, 4])
    P[:, 4] = mix(half, F(60.0) * u[:, 5])
    P[:, 5] = F(0.0)
    P[:, 7:7 + ns] = u[:, 6:6 + ns] * F(1.0e4)
    P[:, 7 + ns:] = F(-1.5) + F(3.0) * u[:, 6 + ns:6 + ns + ne]
    o = 6 + ns + ne
    lr = np.asarray(light_ranges, F).reshape(4, 2)
    light = lr[None, :, 0] + (lr[None, :, 1] - lr[None, :, 0]) * u[:, o:o + 4]
    ar = np.asarray(alpha_ranges, F).reshape(K, 2)
    alpha = ar[None, :, 0] + (ar[None, :, 1] - ar[None, :, 0]) * u[:, o + 4:o + 4 + K]
    assert P.dtype == F and light.dtype == F and alpha.dtype == F
    return P, light, alpha, u


def pose_intervals(im_size, beta, focal=FOCAL):
    """[7][2]: the ends of the reference sampler's intervals (get_random_params.m) pushed through the same float32 operations as
    a draw.  Every operation is monotone in u (non-decreasing: all factors are >= 0) and rounding is monotone, so every value
    drawn from u in [0, 1] lies between the images of u = 0 and u = 1."""
    beta, focal, half = F(beta), F(focal), F(im_size) * F(0.5)
    omb = F(1.0) - beta
    out = np.zeros((7, 2), F)
    for e, u in enumerate((F(0.0), F(1.0))):
        out[0, e] = beta * F(0) + omb * ((F(-75.0) + F(120.0) * u) * C_DEG)
        out[1, e] = beta * F(0) + omb * ((F(-90.0) + F(180.0) * u) * C_DEG)
        out[2, e] = beta * F(0) + omb * ((F(-30.0) + F(60.0) * u) * C_DEG)
        out[3, e] = beta * half + omb * (F(60.0) * u)
        out[4, e] = out[3, e]
        out[5, e] = F(0)
        out[6, e] = beta * focal + omb * (u * focal)
    return out


def texture(mu_tex, pc_tex, alpha):
    """mu_tex [3,N], pc_tex [3N,K], alpha [B,K] -> tex [B,3,N]: acc = acc + pc alpha, k ascending from mu_tex"""
    mu = np.asarray(mu_tex, F).reshape(-1)
    pc = np.asarray(pc_tex, F).reshape(mu.size, -1)
    al = np.asarray(alpha, F)
    B, K = al.shape[0], al.shape[1]
    acc = np.repeat(mu[None], B, 0).copy()
    for k in range(K):
        acc = acc + pc[None, :, k] * al[:, k:k + 1]
    assert acc.dtype == F
    return acc.reshape(B, 3, -1)


def shade(tex_img, normal, tri_ind, light, background=None, gain=1.0, offset=0.0):
    """-> im_gray, mask [B,H,W,1] float32"""
    t = np.asarray(tex_img, F)
    n = np.asarray(normal, F)
    ti = np.asarray(tri_ind, F)[..., 0]
    l = np.asarray(light, F)
    gain, offset = F(gain), F(offset)
    B, H, W = ti.shape
    with np.errstate(all="ignore"):
        m = np.where(t < F(1e-6), F(1e-6), t)
        a = ((m[..., 0] + m[..., 1]) + m[..., 2]) / F(3.0)
        n = np.where(n[..., 2:3] < 0, -n, n)
        mag = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        mag = np.where(mag > F(1e-6), mag, F(1.0))
        d = np.sqrt(mag) + F(1e-6)
        lb = l[:, None, None, :]
        s = ((lb[..., 0] + lb[..., 1] * (n[..., 0] / d)) + lb[..., 2] * (n[..., 1] / d)) + lb[..., 3] * (n[..., 2] / d)
        inten = a * np.where(s < 0, F(0.0), s)
        out = inten * gain + offset
    assert out.dtype == F
    covered = ti >= 0
    if background is None:
        bg = np.zeros((B, H, W), F)
    else:
        bg = np.broadcast_to(np.asarray(background, F)[..., 0], (B, H, W))
    return np.where(covered, out, bg)[..., None].astype(F), covered.astype(F)[..., None]


def same_bits(a, b):
    """equal float32 bit patterns, any NaN equal to any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
