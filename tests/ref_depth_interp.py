"""The interpolated depth's float64 model in numpy: what fr_depth_interp_forward must return bit for bit, and what
fr_depth_interp_backward must return to a derived bound.

Written from the text of include/fr_hotpath.h ("interpolated depth"); it shares no code with the product (the exact-sum and
bound machinery is that of tests/ref_normal_backward.py: the two backwards form their sums the same way).  Per pixel (row j,
column i) whose tri_ind names a triangle t = (p1, p2, p3) with 0 <= t < ntri and all three ids inside [0, nver), in float64 with
every product and sum rounded on its own (numpy ufuncs do not contract):

  v0 = P3 - P1, v1 = P2 - P1, v2 = (i, j) - P1;  den = dot00 dot11 - dot01 dot01;  u, v by get_point_weight's lines;
  w = ((1 - u) - v, v, u);  depth = fl32((w1 z1 + w2 z2) + w3 z3), or the flat fp32 h where den == 0, or the background.

forward() is the plane; terms() the nine backward terms of every contributing pixel before and after their rounding to fp32;
model() sums the fp32 terms of every (face, row, vertex) exactly (Python integers); torch_grad() is the same gradient by torch
float64 autograd over a gather-based restatement of the interpolation."""
import numpy as np

import ref_normal_backward as RN

BACKGROUND = np.float32(-99999999999999.0)


def weights(V, ids, px, W):
    """One face (V [3,nver] fp32, ids [3,n], px [n] pixel indices) -> dict of float64 [n] arrays, the header's names."""
    P = [V[:, ids[k]].astype(np.float64) for k in range(3)]                       # [3, n] each
    i, j = (px % W).astype(np.float64), (px // W).astype(np.float64)
    with np.errstate(all="ignore"):
        v0x, v0y = P[2][0] - P[0][0], P[2][1] - P[0][1]
        v1x, v1y = P[1][0] - P[0][0], P[1][1] - P[0][1]
        v2x, v2y = i - P[0][0], j - P[0][1]
        dot00 = v0x * v0x + v0y * v0y
        dot01 = v0x * v1x + v0y * v1y
        dot02 = v0x * v2x + v0y * v2y
        dot11 = v1x * v1x + v1y * v1y
        dot12 = v1x * v2x + v1y * v2y
        den = dot00 * dot11 - dot01 * dot01
        flat = den == 0
        inv = 1 / np.where(flat, 1.0, den)
        u = (dot11 * dot02 - dot01 * dot12) * inv
        v = (dot00 * dot12 - dot01 * dot02) * inv
        w = np.stack([(1 - u) - v, v, u])
    return dict(v0x=v0x, v0y=v0y, v1x=v1x, v1y=v1y, dot00=dot00, dot01=dot01, dot11=dot11, den=den, flat=flat, inv=inv, w=w,
                z=np.stack([P[k][2] for k in range(3)]))


def flat_h(V, ids):
    """The op's own h of the triangles `ids`, in fp32 as the forward forms it."""
    z = [V[2, ids[k]].astype(np.float32) for k in range(3)]
    with np.errstate(all="ignore"):
        h = ((z[0] + z[1]) + z[2]) / np.float32(3.0)
    assert h.dtype == np.float32
    return h


def forward(vertex, tri, tri_ind, H, W):
    """-> depth [B,H,W,1] fp32"""
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    tri = np.ascontiguousarray(tri, np.float32)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, H * W)
    out = np.full((B, H * W), BACKGROUND, np.float32)
    for b in range(B):
        px, ids = RN.contributing(tri, tind[b], nver)
        q = weights(vertex[b], ids, px, W)
        with np.errstate(all="ignore"):
            d = ((q["w"][0] * q["z"][0] + q["w"][1] * q["z"][1]) + q["w"][2] * q["z"][2]).astype(np.float32)
        out[b, px] = np.where(q["flat"], flat_h(vertex[b], ids), d)
    return out.reshape(B, H, W, 1)


def terms(g, V, tri, tind, nver, W):
    """One face (g [npix] fp32, V [3,nver] fp32, tind [npix]): (ids [3,n], T64 [n,3,3] the terms in float64 before their rounding,
    T32 [n,3,3] fp32) -- axis 1 is the vertex of the triangle, axis 2 the coordinate (x, y, z)."""
    px, ids = RN.contributing(tri, tind, nver)
    q = weights(V, ids, px, W)
    g32 = g[px].astype(np.float32)
    G = g32.astype(np.float64)
    with np.errstate(all="ignore"):
        gux = (q["dot11"] * q["v0x"] - q["dot01"] * q["v1x"]) * q["inv"]
        guy = (q["dot11"] * q["v0y"] - q["dot01"] * q["v1y"]) * q["inv"]
        gvx = (q["dot00"] * q["v1x"] - q["dot01"] * q["v0x"]) * q["inv"]
        gvy = (q["dot00"] * q["v1y"] - q["dot01"] * q["v0y"]) * q["inv"]
        d2, d3 = q["z"][1] - q["z"][0], q["z"][2] - q["z"][0]
        Ax = d2 * gvx + d3 * gux
        Ay = d2 * gvy + d3 * guy
        T64 = np.zeros((len(px), 3, 3))
        for k in range(3):
            c = G * q["w"][k]
            T64[:, k, 0] = -(c * Ax)
            T64[:, k, 1] = -(c * Ay)
            T64[:, k, 2] = c
        zflat = ((g32 * np.float32(1.0)) / np.float32(3.0)).astype(np.float64)    # the flat backward's term, formed in fp32
        f = q["flat"]
        T64[f, :, 0:2] = 0.0
        T64[f, :, 2] = zflat[f, None]
        T32 = T64.astype(np.float32)
    return ids, T64, T32


def model(depth_grad, vertex, tri, tri_ind, H, W):
    """-> RN.Model: per face the exact sums S, the counts n, A = sum |term|, M, the non-finite flags (tests/ref_normal_backward.py);
    RN.check_bound(got, model) is the header's bound in integers."""
    npix = H * W
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    g = np.ascontiguousarray(depth_grad, np.float32).reshape(B, npix)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    R = RN.Model()
    R.shift, R.nver, R.faces = RN.shift_of(npix), nver, []
    for b in range(B):
        ids, _, T32 = terms(g[b], vertex[b], tri, tind[b], nver, W)
        R.faces.append(RN.face_of(ids, T32, nver))
    return R


def sums64(depth_grad, vertex, tri, tri_ind, H, W):
    """The model's terms BEFORE their rounding to fp32, summed in float64 per element -> (S [B,3,nver], largest |term|)."""
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    g = np.ascontiguousarray(depth_grad, np.float32).reshape(B, H * W)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, H * W)
    S = np.zeros((B, 3, nver))
    big = 0.0
    for b in range(B):
        ids, T64, _ = terms(g[b], vertex[b], np.ascontiguousarray(tri, np.float32), tind[b], nver, W)
        for k in range(3):
            for c in range(3):
                np.add.at(S[b, c], ids[k], T64[:, k, c])
        big = max(big, float(np.abs(T64).max()) if T64.size else 0.0)
    return S, big


# ---- the same gradient by torch float64 autograd ---------------------------------------------------------------------------
def torch_grad(depth_grad, vertex, tri, tri_ind, H, W):
    """d/dV of sum(depth_grad * depth) in float64, depth = the interpolation restated with gathers (no den == 0 branch: the caller
    restricts tri_ind to triangles with area) -> [B,3,nver] float64."""
    import torch
    npix = H * W
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    g = np.ascontiguousarray(depth_grad, np.float32).reshape(B, npix)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    out = np.zeros((B, 3, nver), np.float64)
    for b in range(B):
        px, ids = RN.contributing(tri, tind[b], nver)
        if px.size == 0:
            continue
        V = torch.tensor(vertex[b].astype(np.float64), requires_grad=True)
        P1, P2, P3 = (V[:, torch.as_tensor(ids[k])] for k in range(3))               # [3, n]
        pix = torch.as_tensor(np.stack([px % W, px // W]).astype(np.float64))
        v0, v1, v2 = P3[:2] - P1[:2], P2[:2] - P1[:2], pix - P1[:2]
        dot00, dot01, dot02 = (v0 * v0).sum(0), (v0 * v1).sum(0), (v0 * v2).sum(0)
        dot11, dot12 = (v1 * v1).sum(0), (v1 * v2).sum(0)
        den = dot00 * dot11 - dot01 * dot01
        u = (dot11 * dot02 - dot01 * dot12) / den
        v = (dot00 * dot12 - dot01 * dot02) / den
        depth = (1 - u - v) * P1[2] + v * P2[2] + u * P3[2]
        (depth * torch.as_tensor(g[b][px].astype(np.float64))).sum().backward()
        out[b] = V.grad.numpy()
    return out
