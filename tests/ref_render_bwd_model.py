"""The render backward's integer model in numpy: what fr_render_depth_backward(_ws) must return, BIT FOR BIT.

Written from the text of include/fr_hotpath.h ("render_depth backward") and the header comments of
csrc/fr_render_bwd.hip and csrc/fr_owner_scatter.h; it shares no code with the oracle or the product.  Per face:

  counted pixels   0 <= (int)tri_ind < ntri                 (x86 conversion: truncation, NaN / out of int32 -> INT_MIN)
  m                largest finite |g| over the counted pixels (as fp32 bits);  bad = an Inf / NaN among them
  e                (m >> 23) - 127
  terms            c = (g * 1.0f) / 3.0f in fp32, from the counted pixels whose three vertex ids (int)tri[k, t] are all
                   inside [0, nver) -- a counted pixel with an id outside adds nothing, but counts towards m and bad
  q                rint(c * 2^(40 - shift - e)) as int64  (the product is exact in double; ties to even)
  per vertex       S = sum of q (integers: any order), r = fp32(S) (one rounding), z = fp32(double(r) * 2^(e - 40 + shift))
  shift            0 up to 2^20 pixels, then one per doubling of H * W

x and y rows are +0.  A bad face has no bits to predict (fp32 atomics in an unknown order): the model gives the class of
every vertex and, for the finite ones, the float64 sum of the terms, their number and the sum of their magnitudes.

exact() is the same sum in exact integer arithmetic (Python ints, units of 2^-149: every finite fp32 is a multiple)."""
import numpy as np

INT_MIN = -(1 << 31)
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
UNIT = 149                    # exact(): sums are integers in units of 2^-UNIT


def f2i_x86(a):
    """(int)float as cvttss2si does it: toward zero; NaN and values outside int32 give INT_MIN."""
    a = np.asarray(a, np.float32)
    ok = (a >= np.float32(-2147483648.0)) & (a < np.float32(2147483648.0))      # False for NaN
    return np.where(ok, np.trunc(np.where(ok, a, 0)).astype(np.int64), INT_MIN)


def shift_of(npix):
    s = 0
    while (1 << (20 + s)) < npix:
        s += 1
    return s


def ulp_fp32(x):
    """Spacing of fp32 at |x| (float64 in, float64 out): 2^(floor(log2 |x|) - 23), 2^-149 below the normal range."""
    _, ex = np.frexp(np.abs(np.asarray(x, np.float64)))          # |x| = f * 2^ex, f in [0.5, 1)
    return np.ldexp(1.0, np.maximum(ex - 1, -126) - 23)


def _face_terms(g, tri, tind, nver):
    """One face: (counted mask, ids [3, n] and fp32 gradients [n] of the pixels that contribute)."""
    ntri = tri.shape[1]
    t = f2i_x86(tind)
    counted = (t >= 0) & (t < ntri)
    tc = t[counted]
    ids = np.stack([f2i_x86(tri[k, tc]) for k in range(3)]) if ntri else np.zeros((3, 0), np.int64)
    ok = np.all((ids >= 0) & (ids < nver), axis=0)
    return counted, ids[:, ok], g[counted][ok]


def _scatter(ids, vals, nver, dtype):
    out = np.zeros(nver, dtype)
    for k in range(3):
        np.add.at(out, ids[k], vals)
    return out


class Model:
    """bits [B,3,nver] uint32 (rows of a bad face: 0, not a prediction), m [B] uint32, bad [B] bool, e [B] int, shift, and
    for each bad face b: cls[b] [nver] (FINITE / POS_INF / NEG_INF / NAN), sum64[b], nterm[b], abssum[b] over the finite
    terms of each vertex."""


def model(g, tri, tri_ind, nver, H, W):
    npix = H * W
    g = np.ascontiguousarray(g, np.float32).reshape(-1, npix)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(-1, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    B = g.shape[0]
    M = Model()
    M.shift = shift_of(npix)
    M.bits = np.zeros((B, 3, nver), np.uint32)
    M.m = np.zeros(B, np.uint32)
    M.bad = np.zeros(B, bool)
    M.e = np.zeros(B, np.int64)
    M.cls, M.sum64, M.nterm, M.abssum = {}, {}, {}, {}
    for b in range(B):
        counted, ids, gc = _face_terms(g[b], tri, tind[b], nver)
        mag = g[b][counted].view(np.uint32) & np.uint32(0x7FFFFFFF)
        fin = mag < np.uint32(0x7F800000)
        M.bad[b] = bool((~fin).any())
        M.m[b] = mag[fin].max() if fin.any() else 0
        e = M.e[b] = (int(M.m[b]) >> 23) - 127
        with np.errstate(all="ignore"):
            c = (gc * np.float32(1.0)) / np.float32(3.0)
        assert c.dtype == np.float32
        if M.bad[b]:
            isf = np.isfinite(c)
            has = lambda sel: _scatter(ids[:, sel], 1, nver, np.int64) > 0       # noqa: E731
            nan, pinf, ninf = has(np.isnan(c)), has(c == np.inf), has(c == -np.inf)
            cls = np.full(nver, FINITE, np.int8)
            cls[pinf] = POS_INF
            cls[ninf] = NEG_INF
            cls[nan | (pinf & ninf)] = NAN
            M.cls[b] = cls
            c64 = c[isf].astype(np.float64)
            M.sum64[b] = _scatter(ids[:, isf], c64, nver, np.float64)
            M.nterm[b] = _scatter(ids[:, isf], 1, nver, np.int64)
            M.abssum[b] = _scatter(ids[:, isf], np.abs(c64), nver, np.float64)
            # the class of a sequential fp32 sum is the class of its terms as long as no partial sum of finite terms
            # overflows; the model refuses to speak where that is not certain
            assert M.abssum[b][cls == FINITE].max(initial=0.0) < 3.0e38
            continue
        # c has 24 significant bits and the scale is a power of two: the product is exact in double, rint is the one rounding
        q = np.rint(c.astype(np.float64) * np.ldexp(1.0, int(40 - M.shift - e))).astype(np.int64)
        S = _scatter(ids, q, nver, np.int64)
        r = S.astype(np.float32)                                               # int64 -> fp32, ties to even
        with np.errstate(over="ignore"):
            z = (r.astype(np.float64) * np.ldexp(1.0, int(e - 40 + M.shift))).astype(np.float32)
        M.bits[b, 2] = z.view(np.uint32)
    return M


def exact(g, tri, tri_ind, nver, H, W):
    """(sums [B, nver] of Python ints in units of 2^-UNIT, n_v [B, nver]): the per-vertex sum of the fp32 terms c, exactly.
    A non-finite term is an error (a bad face has no exact sum)."""
    npix = H * W
    g = np.ascontiguousarray(g, np.float32).reshape(-1, npix)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(-1, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    B = g.shape[0]
    LIMB = 16                                     # 24-bit mantissa << (< 16) is below 2^40: 2^22 of them fit an int64 limb
    nlimb = (UNIT + 128) // LIMB + 1
    weights = np.array([1 << (LIMB * j) for j in range(nlimb)], object)
    sums = np.empty((B, nver), object)
    n_v = np.zeros((B, nver), np.int64)
    for b in range(B):
        _, ids, gc = _face_terms(g[b], tri, tind[b], nver)
        c = (gc * np.float32(1.0)) / np.float32(3.0)
        if not np.isfinite(c).all():
            raise ValueError("face %d has a non-finite term" % b)
        f, ex = np.frexp(c.astype(np.float64))
        mant = np.rint(np.ldexp(f, 24)).astype(np.int64)                      # c = mant * 2^(ex - 24), |mant| < 2^24
        sh = ex.astype(np.int64) - 24 + UNIT
        low = sh < 0                                                          # subnormals: trailing zero bits below the unit
        assert np.all(mant[low] & ((1 << np.minimum(-sh[low], 62)) - 1) == 0)
        mant[low] >>= -sh[low]
        sh[low] = 0
        sh[c == 0] = 0
        limbs = np.zeros((nver, nlimb), np.int64)
        for k in range(3):
            np.add.at(limbs, (ids[k], sh // LIMB), mant << (sh % LIMB))
            np.add.at(n_v[b], ids[k], 1)
        sums[b] = limbs.astype(object) @ weights
    return sums, n_v


def round_to_fp32(x_units):
    """A Python int in units of 2^-UNIT rounded to fp32 (ties to even; overflow -> +-Inf), without floating point."""
    a = abs(x_units)
    if a == 0:
        return np.float32(0.0)
    drop = max(a.bit_length() - 24, 0)                     # the units are the subnormal spacing: never finer than that
    keep, rest = a >> drop, a & ((1 << drop) - 1)
    half = 1 << (drop - 1) if drop else 0
    if drop and (rest > half or (rest == half and (keep & 1))):
        keep += 1
    if keep << drop >= 1 << (128 + UNIT):
        v = np.float32(np.inf)
    else:
        v = np.float32(np.ldexp(float(keep), drop - UNIT))
    return -v if x_units < 0 else v


BOUND_UNIT = 170               # bound_ratio(): 2^-170 holds both the fp32 values (2^-149) and the grid error (>= 2^-168)


def bound_ratio(z, X, n_v, e, shift):
    """One fixed-point face: asserts  |z - exact| <= n_v * 2^(e - 41 + shift) + ulp_fp32(exact)  on every vertex, in Python
    ints (z [nver] fp32, X / n_v from exact()); where the rounded exact sum overflows, z must be the same infinity.  The
    bound is derived, not measured: each q is off by at most half a grid unit; the int64 -> fp32 rounding is at most half
    an ulp; the second half ulp covers the double rounding of a subnormal result.  Returns the worst error / bound."""
    U = BOUND_UNIT
    worst = 0.0
    for v in range(len(z)):
        x = int(X[v])
        want = round_to_fp32(x)
        if np.isinf(want):
            assert z[v] == want, (v, z[v], want)
            continue
        assert np.isfinite(z[v]), (v, z[v])
        ulp = int(np.ldexp(float(ulp_fp32(np.ldexp(float(x), -UNIT))), U))
        bound = int(n_v[v]) * (1 << (int(e) - 41 + int(shift) + U)) + ulp
        err = abs((int(np.ldexp(float(z[v]), UNIT)) - x) << (U - UNIT))
        assert err <= bound, (v, err, bound)
        worst = max(worst, err / bound)
    return worst


def assert_bad_face(z, M, b):
    """A bad face of model M against the fp32 row z [nver] a kernel returned: the class of every vertex, and every finite
    vertex within n_v * ulp_fp32(sum |terms|) of the float64 sum -- the standard bound of an fp32 sum in ANY order: each of
    the n_v additions rounds a partial sum of magnitude at most sum |terms|, by at most half an ulp of it."""
    cls = np.where(np.isnan(z), NAN, np.where(z == np.inf, POS_INF, np.where(z == -np.inf, NEG_INF, FINITE)))
    np.testing.assert_array_equal(cls, M.cls[b])
    f = M.cls[b] == FINITE
    err = np.abs(z[f].astype(np.float64) - M.sum64[b][f])
    assert np.all(err <= M.nterm[b][f] * ulp_fp32(M.abssum[b][f])), float(err.max())
