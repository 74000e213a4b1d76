"""The smooth planes' float64 models in numpy: what fr_attr_interp_forward and fr_mesh_vertex_normals_backward must return bit for
bit, and what fr_attr_interp_backward must return to a derived bound.

Written from the text of include/fr_hotpath.h ("smooth planes"); it shares no code with the product.  The weights are those of
tests/ref_depth_interp.py (the header defines them as the interpolated depth's), the exact-sum and bound machinery that of
tests/ref_normal_backward.py (the backwards form their sums the same way).  Every product and sum is rounded on its own: numpy
ufuncs and Python floats do not contract.

  forward()             the plane [B,H,W,3] fp32
  terms()               per contributing pixel the nine attribute terms and the nine vertex terms, before and after rounding to fp32
  model()               (attribute Model, vertex Model): the exact sums of the fp32 terms per (face, row, vertex)
  sums64()              the float64 terms summed in float64: the derivative the central differences of forward64() are held to
  forward64()           the interpolation in float64 on float64 inputs, no rounding to fp32, no den == 0 branch
  normals64()           the vertex normals in float64 on float64 inputs, no rounding to fp32
  normals_backward()    the vertex-normal backward in its stated chain order: (vertex_grad fp32, the chains in float64, h)"""
import math

import numpy as np

import ref_depth_interp as RD
import ref_normal_backward as RN


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _attr_of(A, ids):
    """one face's attribute [3,nver] -> a [k][c] float64 [n] arrays"""
    return [[A[c, ids[k]].astype(np.float64) for c in range(3)] for k in range(3)]


def forward(vertex, attr, tri, tri_ind, H, W):
    """-> out [B,H,W,3] fp32"""
    vertex, attr, tri = _f32(vertex), _f32(attr), _f32(tri)
    B, _, nver = vertex.shape
    tind = _f32(tri_ind).reshape(B, H * W)
    out = np.zeros((B, H * W, 3), np.float32)
    for b in range(B):
        px, ids = RN.contributing(tri, tind[b], nver)
        q = RD.weights(vertex[b], ids, px, W)
        a = _attr_of(attr[b], ids)
        for c in range(3):
            with np.errstate(all="ignore"):
                v = ((q["w"][0] * a[0][c] + q["w"][1] * a[1][c]) + q["w"][2] * a[2][c]).astype(np.float32)
                a32 = [attr[b][c, ids[k]] for k in range(3)]
                flat = ((a32[0] + a32[1]) + a32[2]) / np.float32(3.0)                  # the render's own lookup, in fp32
            assert flat.dtype == np.float32
            out[b, px, c] = np.where(q["flat"], flat, v)
    return out.reshape(B, H, W, 3)


def terms(g, V, A, tri, tind, nver, W):
    """One face (g [npix,3] fp32, V, A [3,nver] fp32, tind [npix]) -> (ids [3,n], Ta64, Ta32, Tv64, Tv32), the T [n,3,3]: axis 1 the
    vertex of the triangle, axis 2 the channel (attribute terms) or the coordinate x, y, z (vertex terms)."""
    px, ids = RN.contributing(tri, tind, nver)
    q = RD.weights(V, ids, px, W)
    g32 = g[px].astype(np.float32)
    G = g32.astype(np.float64)
    a = _attr_of(A, ids)
    n = len(px)
    with np.errstate(all="ignore"):
        gux = (q["dot11"] * q["v0x"] - q["dot01"] * q["v1x"]) * q["inv"]
        guy = (q["dot11"] * q["v0y"] - q["dot01"] * q["v1y"]) * q["inv"]
        gvx = (q["dot00"] * q["v1x"] - q["dot01"] * q["v0x"]) * q["inv"]
        gvy = (q["dot00"] * q["v1y"] - q["dot01"] * q["v0y"]) * q["inv"]
        Ax, Ay = [], []
        for c in range(3):
            d2, d3 = a[1][c] - a[0][c], a[2][c] - a[0][c]
            Ax.append(d2 * gvx + d3 * gux)
            Ay.append(d2 * gvy + d3 * guy)
        Sx = (G[:, 0] * Ax[0] + G[:, 1] * Ax[1]) + G[:, 2] * Ax[2]
        Sy = (G[:, 0] * Ay[0] + G[:, 1] * Ay[1]) + G[:, 2] * Ay[2]
        Ta64, Tv64 = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
        for k in range(3):
            for c in range(3):
                Ta64[:, k, c] = G[:, c] * q["w"][k]
            Tv64[:, k, 0] = -(q["w"][k] * Sx)
            Tv64[:, k, 1] = -(q["w"][k] * Sy)
        third = ((g32 * np.float32(1.0)) / np.float32(3.0)).astype(np.float64)          # the flat lookup's term, formed in fp32
        f = q["flat"]
        Ta64[f] = third[f][:, None, :]
        Tv64[f] = 0.0
        Ta32, Tv32 = Ta64.astype(np.float32), Tv64.astype(np.float32)
    return ids, Ta64, Ta32, Tv64, Tv32


def _faces(grad, vertex, attr, tri, tri_ind, H, W):
    vertex, attr, tri = _f32(vertex), _f32(attr), _f32(tri)
    B, _, nver = vertex.shape
    g = _f32(grad).reshape(B, H * W, 3)
    tind = _f32(tri_ind).reshape(B, H * W)
    return nver, [terms(g[b], vertex[b], attr[b], tri, tind[b], nver, W) for b in range(B)]


def model(grad, vertex, attr, tri, tri_ind, H, W):
    """-> (RN.Model of attr_grad, RN.Model of vertex_grad): RN.check_bound(got, model) is the header's bound in integers, each output
    against the largest |term| of its own terms."""
    nver, faces = _faces(grad, vertex, attr, tri, tri_ind, H, W)
    Ra, Rv = RN.Model(), RN.Model()
    for R, j in ((Ra, 2), (Rv, 4)):
        R.shift, R.nver = RN.shift_of(H * W), nver
        R.faces = [RN.face_of(t[0], t[j], nver) for t in faces]
    return Ra, Rv


def sums64(grad, vertex, attr, tri, tri_ind, H, W):
    """The terms BEFORE their rounding to fp32, summed in float64 per element -> (attr_grad, vertex_grad) [B,3,nver] float64."""
    nver, faces = _faces(grad, vertex, attr, tri, tri_ind, H, W)
    out = []
    for j in (1, 3):
        S = np.zeros((len(faces), 3, nver))
        for b, t in enumerate(faces):
            for k in range(3):
                for c in range(3):
                    np.add.at(S[b, c], t[0][k], t[j][:, k, c])
        out.append(S)
    return out


def weights64(V, ids, px, W):
    """the barycentric weights [3,n] of float64 positions V [3,nver]; den must not vanish"""
    P = [V[:, ids[k]] for k in range(3)]
    i, j = (px % W).astype(np.float64), (px // W).astype(np.float64)
    v0x, v0y = P[2][0] - P[0][0], P[2][1] - P[0][1]
    v1x, v1y = P[1][0] - P[0][0], P[1][1] - P[0][1]
    v2x, v2y = i - P[0][0], j - P[0][1]
    dot00, dot01, dot02 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v0x * v2x + v0y * v2y
    dot11, dot12 = v1x * v1x + v1y * v1y, v1x * v2x + v1y * v2y
    den = dot00 * dot11 - dot01 * dot01
    assert np.all(den != 0)
    u = (dot11 * dot02 - dot01 * dot12) / den
    v = (dot00 * dot12 - dot01 * dot02) / den
    return np.stack([(1 - u) - v, v, u]), den


def forward64(V, A, ids, px, W):
    """One face in float64 (V, A [3,nver] float64; ids [3,n], px [n] held fixed) -> (out [n,3], w [3,n], den [n])"""
    w, den = weights64(V, ids, px, W)
    out = np.stack([(w[0] * A[c, ids[0]] + w[1] * A[c, ids[1]]) + w[2] * A[c, ids[2]] for c in range(3)], axis=1)
    return out, w, den


# ---- vertex normals -------------------------------------------------------------------------------------------------------------
def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _triangles_of(v, ids, adj_start, adj_tri, nver):
    ntri = ids.shape[1]
    for e in range(max(int(adj_start[v]), 0), min(int(adj_start[v + 1]), 3 * ntri)):
        t = int(adj_tri[e])
        if not 0 <= t < ntri:
            continue
        p = [int(ids[k, t]) for k in range(3)]
        if all(0 <= i < nver for i in p):
            yield p


def _normal_sums(V, ids, adj_start, adj_tri):
    """one face V [3,nver] (any float dtype, widened) -> (N [nver][3] Python floats, s [nver]): the forward's chains and length"""
    nver = V.shape[1]
    P = V.astype(np.float64).T.tolist()
    N, S = [], []
    for v in range(nver):
        n = [0.0, 0.0, 0.0]
        for p in _triangles_of(v, ids, adj_start, adj_tri, nver):
            a = [P[p[1]][c] - P[p[0]][c] for c in range(3)]
            b = [P[p[2]][c] - P[p[0]][c] for c in range(3)]
            x = _cross(a, b)
            n = [n[c] + x[c] for c in range(3)]
        sq = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        N.append(n)
        S.append(math.sqrt(sq) if sq >= 0 else float("nan"))                             # (an overflowed sum: inf; NaN stays NaN)
    return P, N, S


def normals64(V, tri, adj_start, adj_tri):
    """one face V [3,nver] float64 -> unit normals [3,nver] float64 ((0, 0, 0) where the sum vanishes), not rounded to fp32"""
    ids = RN.f2i_x86(_f32(tri))
    _, N, S = _normal_sums(V, ids, adj_start, adj_tri)
    out = np.zeros((3, V.shape[1]))
    for v, (n, s) in enumerate(zip(N, S)):
        if s > 0.0 and math.isfinite(s):
            out[:, v] = [n[c] / s for c in range(3)]
    return out


def normals_backward(normal_grad, vertex, tri, adj_start, adj_tri, old=None):
    """normal_grad, vertex [B,3,nver] fp32 -> (vertex_grad [B,3,nver] fp32 -- fl32(old + it) with `old` --, the chains [B,3,nver]
    float64 before their rounding, h [B,3,nver] float64)"""
    g, vertex = _f32(normal_grad), _f32(vertex)
    ids = RN.f2i_x86(_f32(tri))
    B, _, nver = vertex.shape
    H = np.zeros((B, 3, nver))
    R = np.zeros((B, 3, nver))
    for b in range(B):
        P, N, S = _normal_sums(vertex[b], ids, adj_start, adj_tri)
        gb = g[b].astype(np.float64).T.tolist()
        h = []
        for u in range(nver):
            n, s = N[u], S[u]
            if not (s > 0.0 and math.isfinite(s)):
                h.append((0.0, 0.0, 0.0))
                continue
            nh = [n[c] / s for c in range(3)]
            d = (nh[0] * gb[u][0] + nh[1] * gb[u][1]) + nh[2] * gb[u][2]
            with np.errstate(all="ignore"):
                h.append(tuple(float((np.float64(gb[u][c]) - np.float64(nh[c]) * np.float64(d)) / np.float64(s)) for c in range(3)))
        H[b] = np.array(h).T
        for v in range(nver):
            r = [0.0, 0.0, 0.0]
            for p in _triangles_of(v, ids, adj_start, adj_tri, nver):
                Hs = list(h[p[0]])
                if p[1] != p[0]:
                    Hs = [Hs[c] + h[p[1]][c] for c in range(3)]
                if p[2] != p[0] and p[2] != p[1]:
                    Hs = [Hs[c] + h[p[2]][c] for c in range(3)]
                for k in range(3):
                    if p[k] != v:
                        continue
                    if k == 0:
                        x = _cross([P[p[1]][c] - P[p[2]][c] for c in range(3)], Hs)
                    elif k == 1:
                        x = _cross([P[p[2]][c] - P[p[0]][c] for c in range(3)], Hs)
                    else:
                        x = _cross(Hs, [P[p[1]][c] - P[p[0]][c] for c in range(3)])
                    r = [r[c] + x[c] for c in range(3)]
            R[b, :, v] = r
    with np.errstate(all="ignore"):
        out = R.astype(np.float32)
        if old is not None:
            out = (_f32(old) + out).astype(np.float32)
    return out, R, H
