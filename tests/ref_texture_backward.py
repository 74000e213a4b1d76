"""The texture backward's integer model in numpy: what fr_render_texture_backward must return, BIT FOR BIT.

Written from the text of include/fr_hotpath.h ("texture gradients"); it shares no code with the product.

  counted pixels   0 <= (int)tri_ind < ntri                 (x86 conversion: truncation, NaN / out of int32 -> INT_MIN)
  contributing     counted, and all three ids (int)tri[k, t] inside [0, nver)
  terms            term_c = fl32(g_c / 3.0f), c = 0..2; each of the triangle's three vertices receives term_c in row c
  scope            one face (tex_batch == B) or the whole batch (tex_batch == 1)
  m                largest finite |term| over the scope's contributing pixels, all channels (as fp32 bits); e = (m >> 23) - 127
  shift            smallest s >= 0 with 2^(20 + s) >= the scope's pixel count (H*W, or B*H*W)
  q                rint(term * 2^(39 - shift - e)) as int64 (the product is exact in double; ties to even)
  per element      S = sum of q (integers: any order), r = fp32(S) (one rounding), out = fp32(double(r) * 2^(e - 39 + shift))

An element without a term is +0.  A scope with a non-finite term has no bits to predict: the model gives the class of every
element and, for the finite ones, the float64 sum of the terms, their number and the sum of their magnitudes.

exact() is the same sum in exact integer arithmetic (Python ints in units of 2^-149: every finite fp32 is a multiple)."""
from fractions import Fraction

import numpy as np

INT_MIN = -(1 << 31)
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
UNIT = 149


def f2i_x86(a):
    """(int)float as cvttss2si does it: toward zero; NaN and values outside int32 give INT_MIN."""
    a = np.asarray(a, np.float32)
    ok = (a >= np.float32(-2147483648.0)) & (a < np.float32(2147483648.0))      # False for NaN
    return np.where(ok, np.trunc(np.where(ok, a, 0)).astype(np.int64), INT_MIN)


def shift_of(count):
    s = 0
    while (1 << (20 + s)) < count:
        s += 1
    return s


def face_terms(g, tri, tind, nver):
    """One face: g [npix,3], tind [npix] -> (ids [3,n] int64, terms [n,3] fp32) of the contributing pixels."""
    ntri = tri.shape[1]
    t = f2i_x86(tind)
    counted = (t >= 0) & (t < ntri)
    tc = t[counted]
    ids = np.stack([f2i_x86(tri[k, tc]) for k in range(3)]) if ntri else np.zeros((3, 0), np.int64)
    ok = np.all((ids >= 0) & (ids < nver), axis=0)
    with np.errstate(all="ignore"):
        terms = np.asarray(g, np.float32)[counted][ok] / np.float32(3.0)
    assert terms.dtype == np.float32
    return ids[:, ok], terms.reshape(-1, 3)


def _scatter(ids, vals, nver, dtype):
    """vals [n,3] (or a scalar) -> [3,nver]: every vertex of the triangle receives the pixel's value of each row"""
    out = np.zeros((3, nver), dtype)
    for c in range(3):
        for k in range(3):
            np.add.at(out[c], ids[k], vals if np.isscalar(vals) else vals[:, c])
    return out


def _prep(g, tri, tri_ind, H, W):
    npix = H * W
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(-1, npix)
    B = tind.shape[0]
    g = np.ascontiguousarray(g, np.float32).reshape(B, npix, 3)
    return g, np.ascontiguousarray(tri, np.float32), tind, B, npix


def scopes_of(B, tex_batch):
    assert tex_batch in (1, B)
    return [list(range(B))] if tex_batch == 1 else [[b] for b in range(B)]


def _scope_terms(g, tri, tind, nver, faces):
    parts = [face_terms(g[b], tri, tind[b], nver) for b in faces]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=0)


class Model:
    """bits [tex_batch,3,nver] uint32 (a bad scope: 0, not a prediction), per scope m, e, bad, M (largest finite |term| as a
    float), the shift, and for a bad scope s: cls[s], sum64[s], nterm[s], abssum[s], each [3,nver], over the finite terms."""

    def value(self):
        return self.bits.view(np.float32)


def model(g, tri, tri_ind, nver, H, W, tex_batch):
    g, tri, tind, B, npix = _prep(g, tri, tri_ind, H, W)
    scopes = scopes_of(B, tex_batch)
    M = Model()
    M.shift = shift_of(npix * (B if tex_batch == 1 else 1))
    M.bits = np.zeros((len(scopes), 3, nver), np.uint32)
    M.m = np.zeros(len(scopes), np.uint32)
    M.e = np.zeros(len(scopes), np.int64)
    M.bad = np.zeros(len(scopes), bool)
    M.M = np.zeros(len(scopes), np.float64)
    M.cls, M.sum64, M.nterm, M.abssum = {}, {}, {}, {}
    for s, faces in enumerate(scopes):
        ids, terms = _scope_terms(g, tri, tind, nver, faces)
        mag = terms.view(np.uint32) & np.uint32(0x7FFFFFFF)
        fin = mag < np.uint32(0x7F800000)
        M.bad[s] = bool((~fin).any())
        M.m[s] = mag[fin].max() if fin.any() else 0
        M.M[s] = float(np.array([M.m[s]], np.uint32).view(np.float32)[0])
        e = M.e[s] = (int(M.m[s]) >> 23) - 127
        if M.bad[s]:
            has = lambda sel: _scatter(ids, sel.astype(np.int64), nver, np.int64) > 0       # noqa: E731
            nan, pinf, ninf = has(np.isnan(terms)), has(terms == np.inf), has(terms == -np.inf)
            cls = np.full((3, nver), FINITE, np.int8)
            cls[pinf] = POS_INF
            cls[ninf] = NEG_INF
            cls[nan | (pinf & ninf)] = NAN
            t64 = np.where(fin, terms, 0).astype(np.float64)
            M.cls[s] = cls
            M.sum64[s] = _scatter(ids, t64, nver, np.float64)
            M.nterm[s] = _scatter(ids, fin.astype(np.int64), nver, np.int64)
            M.abssum[s] = _scatter(ids, np.abs(t64), nver, np.float64)
            continue
        # a term has 24 significant bits and the scale is a power of two: the product is exact in double, rint is the one rounding
        q = np.rint(terms.astype(np.float64) * np.ldexp(1.0, int(39 - M.shift - e))).astype(np.int64)
        S = _scatter(ids, q, nver, np.int64)
        r = S.astype(np.float32)                                               # int64 -> fp32, ties to even
        with np.errstate(over="ignore"):
            out = (r.astype(np.float64) * np.ldexp(1.0, int(e - 39 + M.shift))).astype(np.float32)
        M.bits[s] = out.view(np.uint32)
    return M


def exact(g, tri, tri_ind, nver, H, W, tex_batch):
    """(sums, n, A) each [scopes,3,nver]: the per-element sum of the fp32 terms as Python ints in units of 2^-UNIT, the number
    of terms and the sum of their magnitudes (same units).  A non-finite term is an error."""
    g, tri, tind, B, npix = _prep(g, tri, tri_ind, H, W)
    scopes = scopes_of(B, tex_batch)
    sums = np.zeros((len(scopes), 3, nver), object)
    A = np.zeros((len(scopes), 3, nver), object)
    n = np.zeros((len(scopes), 3, nver), np.int64)
    for s, faces in enumerate(scopes):
        ids, terms = _scope_terms(g, tri, tind, nver, faces)
        if not np.isfinite(terms).all():
            raise ValueError("scope %d has a non-finite term" % s)
        scaled = np.ldexp(terms.astype(np.float64), UNIT)                      # exact: an integer below 2^277 with 24 bits
        ints = np.array([int(x) for x in scaled.ravel()], object).reshape(scaled.shape)
        assert all(float(i) == x for i, x in zip(ints.ravel()[:64], scaled.ravel()[:64]))
        for c in range(3):
            for k in range(3):
                np.add.at(sums[s, c], ids[k], ints[:, c])
                np.add.at(A[s, c], ids[k], abs(ints[:, c]))
                np.add.at(n[s, c], ids[k], 1)
    return sums, n, A


def units(z):
    """fp32 array -> Python ints in units of 2^-UNIT (exact)"""
    z64 = np.ldexp(np.asarray(z, np.float32).astype(np.float64), UNIT)
    return np.array([int(x) for x in z64.ravel()], object).reshape(z64.shape)


def check_bound(z, X, n, M, shift, extra=None):
    """asserts |z - X| <= 2^-24 |X| + n 2^(shift - 39) M (+ extra) on every element, in rationals: z fp32 [..], X exact sums in
    units of 2^-UNIT, n term counts, M the scope's largest |term| (float), extra an optional array of Fractions in the same
    units.  Returns the worst error / bound (0 where both are 0)."""
    zu = units(z)
    Mu = Fraction(float(M)) * (1 << UNIT)
    worst = 0.0
    for i in np.ndindex(zu.shape):
        x = int(X[i])
        bound = Fraction(abs(x), 1 << 24) + int(n[i]) * Mu * Fraction(2) ** (int(shift) - 39)
        if extra is not None:
            bound += extra[i]
        err = abs(int(zu[i]) - x)
        assert err <= bound, (i, float(err), float(bound))
        if bound:
            worst = max(worst, float(Fraction(err) / bound))
    return worst


def assert_bad_scope(z, M, s):
    """A bad scope of model M against the fp32 rows z [3,nver] a kernel returned: the class of every element, and every finite
    element within 2^-23 A of the float64 sum of its terms, A = sum |term| (the header's bound)."""
    cls = np.where(np.isnan(z), NAN, np.where(z == np.inf, POS_INF, np.where(z == -np.inf, NEG_INF, FINITE)))
    np.testing.assert_array_equal(cls, M.cls[s])
    f = M.cls[s] == FINITE
    err = np.abs(z[f].astype(np.float64) - M.sum64[s][f])
    assert np.all(err <= 2.0 ** -23 * M.abssum[s][f]), float(err.max())


def torch_grad(g, tri, tri_ind, nver, H, W, tex_batch):
    """float64 autograd of a gather-based restatement of the forward lookup: tex_img[b,p,c] = (t[c,p1] + t[c,p2] + t[c,p3]) / 3 on
    the contributing pixels, loss = sum(tex_img * g) -> d loss / d texture, [tex_batch,3,nver] float64"""
    import torch
    g, tri, tind, B, npix = _prep(g, tri, tri_ind, H, W)
    tex = torch.zeros((tex_batch, 3, nver), dtype=torch.float64, requires_grad=True)
    loss = torch.zeros((), dtype=torch.float64)
    ntri = tri.shape[1]
    for b in range(B):
        t = f2i_x86(tind[b])
        counted = (t >= 0) & (t < ntri)
        tc = t[counted]
        ids = np.stack([f2i_x86(tri[k, tc]) for k in range(3)]) if ntri else np.zeros((3, 0), np.int64)
        ok = np.all((ids >= 0) & (ids < nver), axis=0)
        ids = torch.as_tensor(ids[:, ok])
        gb = torch.as_tensor(g[b][counted][ok].astype(np.float64))             # [n,3]
        tb = tex[0 if tex_batch == 1 else b]                                   # [3,nver]
        img = (tb[:, ids[0]] + tb[:, ids[1]] + tb[:, ids[2]]) / 3.0            # [3,n]
        loss = loss + (img.t() * gb).sum()
    loss.backward()
    return tex.grad.numpy()
