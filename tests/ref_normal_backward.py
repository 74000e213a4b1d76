"""The normal backward's float64 model in numpy: what fr_render_normal_backward must return, to a derived bound.

Written from the text of include/fr_hotpath.h ("normal-map gradients"); it shares no code with the product.  Per pixel whose
tri_ind names a triangle t = (p1, p2, p3) with 0 <= t < ntri and all three ids inside [0, nver):

  a = fl32(P1 - P2), b = fl32(P1 - P3);  G = the pixel's normal_grad (mode 0), or the gradient of the normalised map pulled back
  through post_normal (mode 1);  da = b x G, db = G x a in float64, every product and sum rounded on its own (numpy ufuncs do
  not contract);  term(p1) = fl32(da + db), term(p2) = fl32(-da), term(p3) = fl32(-db).

model() sums the fp32 terms of every (face, row, vertex) EXACTLY (integers in units of 2^-149, of which every finite fp32 is
a multiple: int64 limbs, then Python integers) and returns the sums S, the number of terms n_v, the face's largest |term| M and
A = sum |term|, for the elements that receive a term.
terms() exposes the terms themselves, before and after the rounding to fp32; torch_grad() is the same gradient by torch
float64 autograd over a gather-based restatement of the forward normal and its post-processing."""
import numpy as np

INT_MIN = -(1 << 31)
UNIT = 149
EPS = np.float64(np.float32(1e-6))


def f2i_x86(a):
    """(int)float as cvttss2si does it: toward zero; NaN and values outside int32 give INT_MIN."""
    a = np.asarray(a, np.float32)
    ok = (a >= np.float32(-2147483648.0)) & (a < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, a, 0)).astype(np.int64), INT_MIN)


def shift_of(npix):
    s = 0
    while (1 << (20 + s)) < npix:
        s += 1
    return s


def contributing(tri, tind, nver):
    """One face: (pixel indices [n], ids [3, n]) of the pixels that contribute."""
    ntri = tri.shape[1]
    t = f2i_x86(tind)
    px = np.nonzero((t >= 0) & (t < ntri))[0]
    ids = np.stack([f2i_x86(tri[k, t[px]]) for k in range(3)]) if ntri else np.zeros((3, 0), np.int64)
    ok = np.all((ids >= 0) & (ids < nver), axis=0)
    return px[ok], ids[:, ok]


def forward_normal(V, ids):
    """(a, b [n,3] float64 holding fp32 values, n32 [n,3] fp32): the forward's differences and its normal (resolve_pixel)."""
    P = [V[:, ids[k]].T.astype(np.float32) for k in range(3)]                       # [n, 3]
    with np.errstate(all="ignore"):
        a = (P[0] - P[1]).astype(np.float64)
        b = (P[0] - P[2]).astype(np.float64)
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        return a, b, n.astype(np.float32)


def post_branch(n32):
    """(s [n] float64 in {-1, 1}, m [n,3] float64, big [n] bool): post_normal's flip and its fp32 branch mag32 > 1e-6f."""
    s32 = np.where(n32[:, 2] < 0, np.float32(-1), np.float32(1))
    m32 = s32[:, None] * n32
    with np.errstate(all="ignore"):
        mag32 = (m32[:, 0] * m32[:, 0] + m32[:, 1] * m32[:, 1]) + m32[:, 2] * m32[:, 2]
    assert mag32.dtype == np.float32
    return s32.astype(np.float64), m32.astype(np.float64), mag32 > np.float32(1e-6), mag32


def terms(g, V, tri, tind, nver, mode):
    """One face (g [npix,3] fp32, V [3,nver] fp32, tind [npix]): (ids [3,n], T64 [n,3,3] the terms in float64 before their
    rounding, T32 [n,3,3] fp32, mag32 [n]) -- axis 1 is the vertex of the triangle, axis 2 the coordinate."""
    px, ids = contributing(tri, tind, nver)
    a, b, n32 = forward_normal(V, ids)
    G = g[px].astype(np.float64)
    mag32 = None
    with np.errstate(all="ignore"):
        if mode == 1:
            s, m, big, mag32 = post_branch(n32)
            r = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
            d = r + EPS
            k = (G[:, 0] * m[:, 0] + G[:, 1] * m[:, 1] + G[:, 2] * m[:, 2]) / (d * d * r)
            Gb = G / d[:, None] - m * k[:, None]
            Gs = G / (1.0 + EPS)
            G = s[:, None] * np.where(big[:, None], Gb, Gs)
        da = np.stack([b[:, 1] * G[:, 2] - b[:, 2] * G[:, 1], b[:, 2] * G[:, 0] - b[:, 0] * G[:, 2],
                       b[:, 0] * G[:, 1] - b[:, 1] * G[:, 0]], axis=1)
        db = np.stack([G[:, 1] * a[:, 2] - G[:, 2] * a[:, 1], G[:, 2] * a[:, 0] - G[:, 0] * a[:, 2],
                       G[:, 0] * a[:, 1] - G[:, 1] * a[:, 0]], axis=1)
        T64 = np.stack([da + db, -da, -db], axis=1)
        T32 = T64.astype(np.float32)
    return ids, T64, T32, mag32


LIMB = 16                      # a 24-bit mantissa << (< 16) is below 2^40: 2^22 of them fit an int64 limb
NLIMB = (UNIT + 128) // LIMB + 1
_WEIGHTS = np.array([1 << (LIMB * j) for j in range(NLIMB)], object)


def _exact_sums(slot, nslot, x32):
    """sum of the finite fp32 values x32 [n] into `nslot` slots (slot [n]) -> object array of Python ints, units of 2^-UNIT."""
    f, ex = np.frexp(x32.astype(np.float64))
    mant = np.rint(np.ldexp(f, 24)).astype(np.int64)                          # x = mant * 2^(ex - 24), |mant| <= 2^24
    sh = ex.astype(np.int64) - 24 + UNIT
    low = sh < 0                                                              # subnormals: trailing zero bits below the unit
    assert np.all(mant[low] & ((1 << np.minimum(-sh[low], 62)) - 1) == 0)
    mant[low] >>= -sh[low]
    sh[low] = 0
    sh[x32 == 0] = 0
    limbs = np.zeros((nslot, NLIMB), np.int64)
    np.add.at(limbs, (slot, sh // LIMB), mant << (sh % LIMB))
    return limbs.astype(object) @ _WEIGHTS


class Face:
    """One face, sparse: elem [k] = row * nver + vertex of every element that receives a term; S, A [k] Python ints in units of
    2^-UNIT (sum of the finite fp32 terms, sum of their magnitudes); n [k] terms per element (zeros included); nonfinite [k] the
    element receives an Inf / NaN term; M the face's largest finite |term| (Python int, same units); bad: a non-finite term."""


class Model:
    """faces [B] of Face, shift, nver; mag32 [B] (mode 1: post_normal's fp32 |m|^2 of every contributing pixel)."""

    def dense(self, b, what="S"):
        """float64 [3, nver] of face b's S or A (rounded), or int64 of n / bool of nonfinite."""
        F = self.faces[b]
        v = getattr(F, what)
        out = np.zeros(3 * self.nver, np.float64 if what in "SA" else v.dtype)
        out[F.elem] = to_float(v) if what in "SA" else v
        return out.reshape(3, self.nver)


def model(normal_grad, vertex, tri, tri_ind, H, W, mode):
    npix = H * W
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    g = np.ascontiguousarray(normal_grad, np.float32).reshape(B, npix, 3)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    R = Model()
    R.shift, R.nver, R.faces, R.mag32 = shift_of(npix), nver, [], []
    for b in range(B):
        ids, _, T32, mag32 = terms(g[b], vertex[b], tri, tind[b], nver, mode)
        R.mag32.append(mag32)
        R.faces.append(face_of(ids, T32, nver))
    return R


FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3


def face_of(ids, T32, nver):
    """The Face of one face's terms (ids [3,n], T32 [n,3,3] fp32: axis 1 the vertex of the triangle, axis 2 the row).  Beside the
    fields the class names: cls [k], what the header's rule for a face with a non-finite term makes of the element -- NAN where a
    NaN term or Inf terms of both signs arrive, POS_INF / NEG_INF where Inf terms of that one sign arrive, else FINITE."""
    F = Face()
    flat = (np.arange(3)[None, None, :] * nver + ids.T[:, :, None]).ravel()          # [n, vertex k, row c] -> c * nver + id
    t = T32.ravel()
    fin = np.isfinite(t)
    F.bad = bool((~fin).any())
    F.elem, slot = np.unique(flat, return_inverse=True)
    slot = slot.reshape(-1)
    k = len(F.elem)
    tf = np.where(fin, t, np.float32(0))
    F.S = _exact_sums(slot, k, tf)
    F.A = _exact_sums(slot, k, np.abs(tf))
    F.n = np.bincount(slot, minlength=k).astype(np.int64)
    F.nonfinite = np.bincount(slot, weights=~fin, minlength=k) > 0
    F.M = to_units(np.abs(tf).max()) if tf.size else 0
    has = lambda sel: np.bincount(slot, weights=sel, minlength=k) > 0                 # noqa: E731
    nan, pinf, ninf = has(np.isnan(t)), has(t == np.inf), has(t == -np.inf)
    F.cls = np.full(k, FINITE, np.int8)
    F.cls[pinf] = POS_INF
    F.cls[ninf] = NEG_INF
    F.cls[nan | (pinf & ninf)] = NAN
    return F


def check_bad_faces(got, R):
    """The header's rule on every face of R with a non-finite term (the faces check_bound leaves out; it names what the float-atomic
    route guarantees, not bits): an element that receives a non-finite term comes out non-finite -- NaN where a NaN term or Infs of
    both signs arrive, the Inf otherwise; every other element of the face is finite; an element with no term is +0.
    Returns the number of such faces."""
    got = np.ascontiguousarray(got, np.float32)
    count = 0
    for b, F in enumerate(R.faces):
        if not F.bad:
            continue
        count += 1
        flat = got[b].reshape(-1)
        none = np.ones(flat.size, bool)
        none[F.elem] = False
        assert np.all(flat[none].view(np.uint32) == 0), "face %d: an element without terms is not +0" % b
        z = flat[F.elem]
        cls = np.where(np.isnan(z), NAN, np.where(z == np.inf, POS_INF, np.where(z == -np.inf, NEG_INF, FINITE)))
        wrong = np.flatnonzero(cls != F.cls)
        assert wrong.size == 0, "face %d: %d elements of the wrong class, first (row %d, vertex %d): got %r, the terms say class %d" % (
            b, wrong.size, int(F.elem[wrong[0]]) // R.nver, int(F.elem[wrong[0]]) % R.nver, float(z[wrong[0]]), int(F.cls[wrong[0]]))
    return count


def to_units(x32):
    """A finite fp32 scalar as a Python int in units of 2^-UNIT."""
    return int(np.ldexp(np.float64(x32), UNIT))


def to_float(units):
    """Python-int units (array or scalar) -> float64 (rounded)."""
    f = np.frompyfunc(lambda u: float(np.ldexp(np.float64(u), -UNIT)), 1, 1)
    return np.asarray(f(units), np.float64)


def check_bound(got, R, post=False):
    """Asserts  |got - S| <= 2^-24 |S| + n_v 2^(shift - 39) M  (+ 2^-23 A in post mode)  on every element of every finite face,
    in exact integer arithmetic (all sides times 2^63); an element without terms must be +0.  Returns the worst error / bound."""
    got = np.ascontiguousarray(got, np.float32)
    worst = 0.0
    for b, F in enumerate(R.faces):
        if F.bad:
            continue
        flat = got[b].reshape(-1)
        none = np.ones(flat.size, bool)
        none[F.elem] = False
        assert np.all(flat[none].view(np.uint32) == 0), "face %d: an element without terms is not +0" % b
        assert np.all(np.isfinite(flat)), "face %d: non-finite result on a finite face" % b
        for e, S, A, n in zip(F.elem, F.S, F.A, F.n):
            S, A, n = int(S), int(A), int(n)
            err = abs(to_units(flat[e]) - S) << 63
            bound = (abs(S) << 39) + ((n * F.M) << (R.shift + 24)) + ((A << 40) if post else 0)
            assert err <= bound, (b, int(e) // R.nver, int(e) % R.nver, float(flat[e]), float(to_float(S)), err / max(bound, 1))
            if bound:
                worst = max(worst, err / bound)
    return worst


# ---- the same gradient by torch float64 autograd ---------------------------------------------------------------------------
def _straight_through(x, value):
    """A float64 tensor that holds `value` (numpy, the forward's fp32 number) and passes its gradient to x unchanged: the
    forward's rounding of x to fp32, which the backward is defined to treat as the identity."""
    import torch
    return x + (torch.as_tensor(value) - x.detach())


def torch_grad(normal_grad, vertex, tri, tri_ind, H, W, mode):
    """d/dV of sum(normal_grad * out) in float64, out = the forward normal (mode 0) or its normalised map (mode 1) restated
    with gathers: -> [B,3,nver] float64.  The restatement is of the forward as it is defined, fp32 roundings included:
    a = fl32(P1 - P2), b = fl32(P1 - P3) and n = fl32(a x b) take the forward's values and are straight-through to autograd, so
    the derivative is evaluated at the numbers the forward produced.  (Without them autograd differentiates another function,
    the normal of exact differences: the two differ by 2^-24 |b| |G| per product of da = b x G, which is NOT small against
    |da| where the products cancel, so no bound in terms of the terms themselves could hold between them.)  The flip and the
    branch follow the forward's fp32 values (post_branch)."""
    import torch
    npix = H * W
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    g = np.ascontiguousarray(normal_grad, np.float32).reshape(B, npix, 3)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    out = np.zeros((B, 3, nver), np.float64)
    for b in range(B):
        px, ids = contributing(tri, tind[b], nver)
        if px.size == 0:
            continue
        V = torch.tensor(vertex[b].astype(np.float64), requires_grad=True)
        P = [V[:, torch.as_tensor(ids[k])].T for k in range(3)]
        a32, b32, n32 = forward_normal(vertex[b], ids)
        a, bb = _straight_through(P[0] - P[1], a32), _straight_through(P[0] - P[2], b32)
        n = _straight_through(torch.linalg.cross(a, bb, dim=1), n32.astype(np.float64))
        if mode == 1:
            s, _, big, _ = post_branch(n32)
            m = torch.as_tensor(s)[:, None] * n
            mag = (m * m).sum(1)
            mag = torch.where(torch.as_tensor(big), mag, torch.ones_like(mag))        # network.py:190-192
            n = m / (torch.sqrt(mag) + float(EPS))[:, None]
        (n * torch.as_tensor(g[b][px].astype(np.float64))).sum().backward()
        out[b] = V.grad.numpy()
    return out
