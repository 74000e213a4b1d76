"""The soft coverage's float64 model: what fr_coverage_forward must return bit for bit, and what fr_coverage_backward must return
to a derived bound.

Written from the text of include/fr_hotpath.h ("soft coverage"), loop for loop in the order stated there; it shares no code with
the product (the exact-sum and bound machinery is that of tests/ref_normal_backward.py: the backwards form their sums the same
way).  The arithmetic is Python's float -- IEEE binary64, one rounding per operation, nothing contracted -- on the widened fp32
inputs; the one division goes through numpy so that a zero divisor follows IEEE instead of raising.

  pair()      the pair (c, n) of the header: None when inert, else (k, s, Fc, Fn, sigma)
  forward()   the plane, fp32;  forward64() the same function of float64 vertices without the final rounding (what the central
              differences of tests/test_coverage_cpu.py difference)
  terms()     the six x, y terms (and three +0 z terms) of every pixel that writes a record, before and after their rounding
  model()     the exact sums of the fp32 terms per (face, row, vertex): RN.check_bound(got, model) is the header's bound."""
import math

import numpy as np

import ref_normal_backward as RN

NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # (dx, dy): left, right, up, down


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def edge(ax, ay, bx, by, xx, xy):
    return (bx - ax) * (xy - ay) - (by - ay) * (xx - ax)


def pair(P, c, n):
    """P = ((x1, y1), (x2, y2), (x3, y3)) floats, c and n = (x, y) pixel centres -> None (inert) or (k, s, Fc, Fn, sigma)."""
    area = edge(P[0][0], P[0][1], P[1][0], P[1][1], P[2][0], P[2][1])
    if area == 0 or not math.isfinite(area):
        return None
    sigma = 1.0 if area > 0 else -1.0
    best = None
    for k in range(3):
        A, B = P[k], P[(k + 1) % 3]
        fc = sigma * edge(A[0], A[1], B[0], B[1], float(c[0]), float(c[1]))
        fn = sigma * edge(A[0], A[1], B[0], B[1], float(n[0]), float(n[1]))
        if not (fn < 0 and fc > fn):
            continue
        sk = _div(fc, fc - fn)
        if not math.isfinite(sk):
            continue
        if best is None or sk < best[1]:
            best = (k, sk, fc, fn, sigma)
    return best


def clamp01(s):
    return min(max(s, 0.0), 1.0)


def ok_triangles(tri, tind, nver):
    """One face -> (okt [npix] int64: the triangle of an OK pixel, -1 of a not-OK one; ids [3, ntri] int64)."""
    px, ids = RN.contributing(tri, tind, nver)
    okt = np.full(tind.shape[0], -1, np.int64)
    okt[px] = RN.f2i_x86(tind[px])
    tid = np.stack([RN.f2i_x86(tri[k]) for k in range(3)]) if tri.shape[1] else np.zeros((3, 0), np.int64)
    return okt, tid


def _tri_xy(V, tid, t):
    """the x, y of triangle t's three vertices as Python floats (V [3,nver] of any float dtype)"""
    return tuple((float(V[0, tid[k, t]]), float(V[1, tid[k, t]])) for k in range(3))


def _border(okt, H, W):
    """indices of the pixels with an existing neighbour of the other state"""
    ok = (okt >= 0).reshape(H, W)
    d = np.zeros((H, W), bool)
    d[:, 1:] |= ok[:, 1:] != ok[:, :-1]
    d[:, :-1] |= ok[:, :-1] != ok[:, 1:]
    d[1:, :] |= ok[1:, :] != ok[:-1, :]
    d[:-1, :] |= ok[:-1, :] != ok[1:, :]
    return np.flatnonzero(d.reshape(-1))


def _face_forward(V, okt, tid, H, W):
    """-> float64 [npix]: max(0, 1 - a) / min(1, a) before the rounding to fp32"""
    out = np.where(okt >= 0, 1.0, 0.0)
    for i in _border(okt, H, W):
        y, x = divmod(int(i), W)
        a = 0.0
        me = okt[i]
        for dx, dy in NEIGHBOURS:
            nx, ny = x + dx, y + dy
            if nx < 0 or nx >= W or ny < 0 or ny >= H:
                continue
            other = okt[ny * W + nx]
            if me >= 0:
                if other >= 0:
                    continue
                pr = pair(_tri_xy(V, tid, me), (x, y), (nx, ny))
                if pr is not None:
                    a = a + max(0.5 - clamp01(pr[1]), 0.0)
            else:
                if other < 0:
                    continue
                pr = pair(_tri_xy(V, tid, other), (nx, ny), (x, y))
                if pr is not None:
                    a = a + max(clamp01(pr[1]) - 0.5, 0.0)
        out[i] = max(0.0, 1.0 - a) if me >= 0 else min(1.0, a)
    return out


def forward(vertex, tri, tri_ind, H, W):
    """-> cov [B,H,W,1] fp32"""
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    tri = np.ascontiguousarray(tri, np.float32)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, H * W)
    out = np.zeros((B, H * W), np.float32)
    for b in range(B):
        okt, tid = ok_triangles(tri, tind[b], nver)
        out[b] = _face_forward(vertex[b], okt, tid, H, W).astype(np.float32)
    return out.reshape(B, H, W, 1)


def forward64(vertex64, tri, tri_ind, H, W):
    """The same function of float64 vertices [B,3,nver], no rounding of the result -> [B,H*W] float64"""
    vertex64 = np.ascontiguousarray(vertex64, np.float64)
    B, _, nver = vertex64.shape
    tri = np.ascontiguousarray(tri, np.float32)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, H * W)
    out = np.zeros((B, H * W))
    for b in range(B):
        okt, tid = ok_triangles(tri, tind[b], nver)
        out[b] = _face_forward(vertex64[b], okt, tid, H, W)
    return out


def terms(g, cov, V, tri, tind, nver, H, W):
    """One face (g, cov [npix]; V [3,nver]; tind [npix]) -> (ids [3,n], T64 [n,3,3], T32 [n,3,3] fp32, px [n]) of the pixels that
    write a record -- axis 1 is the vertex of the triangle, axis 2 the coordinate (x, y, z)."""
    okt, tid = ok_triangles(tri, tind, nver)
    px, T = [], []
    for i in _border(okt, H, W):
        me = okt[i]
        if me < 0:
            continue
        y, x = divmod(int(i), W)
        P = _tri_xy(V, tid, me)
        slot = [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
        for dx, dy in NEIGHBOURS:
            nx, ny = x + dx, y + dy
            if nx < 0 or nx >= W or ny < 0 or ny >= H or okt[ny * W + nx] >= 0:
                continue
            pr = pair(P, (x, y), (nx, ny))
            if pr is None or not (0.0 < pr[1] < 1.0):
                continue
            k, s, fc, fn, sigma = pr
            j = ny * W + nx
            q = 0.0
            if s < 0.5 and cov[i] > 0:
                q = q + float(g[i])
            if s > 0.5 and cov[j] < 1:
                q = q + float(g[j])
            ka, kb = k, (k + 1) % 3
            (ax, ay), (bx, by) = P[ka], P[kb]
            xc, yc, xn, yn = float(x), float(y), float(nx), float(ny)
            D = fc - fn
            DD = D * D
            dec = (by - yc, xc - bx, yc - ay, ax - xc)
            den = (by - yn, xn - bx, yn - ay, ax - xn)
            ds = [_div(sigma * ((-fn) * dec[v] + fc * den[v]), DD) for v in range(4)]
            slot[ka][0] = slot[ka][0] + q * ds[0]
            slot[ka][1] = slot[ka][1] + q * ds[1]
            slot[kb][0] = slot[kb][0] + q * ds[2]
            slot[kb][1] = slot[kb][1] + q * ds[3]
        t = np.zeros((3, 3))
        t[:, 0:2] = slot
        with np.errstate(all="ignore"):
            if np.all(t.astype(np.float32) == 0):
                continue                                                      # no record
        px.append(int(i))
        T.append(t)
    px = np.asarray(px, np.int64)
    T64 = np.asarray(T, np.float64).reshape(len(px), 3, 3)
    with np.errstate(all="ignore"):
        T32 = T64.astype(np.float32)
    ids = tid[:, okt[px]] if len(px) else np.zeros((3, 0), np.int64)
    return ids, T64, T32, px


def model(cov_grad, cov, vertex, tri, tri_ind, H, W):
    """-> RN.Model: per face the exact sums of the fp32 terms (tests/ref_normal_backward.py)"""
    npix = H * W
    vertex = np.ascontiguousarray(vertex, np.float32)
    B, _, nver = vertex.shape
    g = np.ascontiguousarray(cov_grad, np.float32).reshape(B, npix)
    c = np.ascontiguousarray(cov, np.float32).reshape(B, npix)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, npix)
    tri = np.ascontiguousarray(tri, np.float32)
    R = RN.Model()
    R.shift, R.nver, R.faces, R.records = RN.shift_of(npix), nver, [], []
    for b in range(B):
        ids, _, T32, px = terms(g[b], c[b], vertex[b], tri, tind[b], nver, H, W)
        R.faces.append(RN.face_of(ids, T32, nver))
        R.records.append(px)
    return R


def grad64(g, cov64, vertex64, tri, tri_ind, H, W):
    """The terms BEFORE their rounding to fp32, summed in float64 per element, for float64 vertices and the float64 plane of
    forward64 -> [B,3,nver] float64"""
    vertex64 = np.ascontiguousarray(vertex64, np.float64)
    B, _, nver = vertex64.shape
    tri = np.ascontiguousarray(tri, np.float32)
    tind = np.ascontiguousarray(tri_ind, np.float32).reshape(B, H * W)
    S = np.zeros((B, 3, nver))
    for b in range(B):
        ids, T64, _, _ = terms(np.asarray(g, np.float64).reshape(B, -1)[b], cov64[b], vertex64[b], tri, tind[b], nver, H, W)
        for k in range(3):
            for c in range(3):
                np.add.at(S[b, c], ids[k], T64[:, k, c])
    return S
