"""numpy models of the fine-mesh operators, exactly as include/fr_hotpath.h ("fine mesh") states them: fr_mesh_visible, fr_mesh_lift
and fr_mesh_vertex_normals.  Float64 on the widened fp32 inputs, every operation rounded on its own, sums in the stated order: the
kernels are held to these bit for bit (tests/test_fine_mesh_gpu.py); tests/test_fine_mesh_cpu.py holds the models to their properties.
Written as plain loops over vertices and corners where the order matters -- the test shapes are small."""
import numpy as np

INT_MIN = -2 ** 31


def f2i(a):
    """the x86 conversion of the render backwards: truncation; NaN and anything outside the int32 range -> INT_MIN"""
    a = np.asarray(a, np.float32)
    ok = (a >= np.float32(-2147483648.0)) & (a < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, a, 0)), INT_MIN).astype(np.int64)


def ok_pixels(tri, tind, nver):
    """tind: any shape of float-stored triangle ids -> (ok mask of that shape, ids [3, ...] of the pixel's triangle)"""
    tri = np.asarray(tri, np.float32)
    ntri = tri.shape[1]
    t = f2i(tind)
    cov = (t >= 0) & (t < ntri)
    if ntri == 0:
        return np.zeros(t.shape, bool), np.zeros((3,) + t.shape, np.int64)
    ids = f2i(tri)[:, np.where(cov, t, 0)]
    ok = cov & ((ids >= 0) & (ids < nver)).all(0)
    return ok, ids


def visible(tri, tind, nver):
    """tri [3,ntri], tind [B,H,W] -> uint8 [B,nver]"""
    tind = np.asarray(tind, np.float32)
    B = tind.shape[0]
    out = np.zeros((B, nver), np.uint8)
    for b in range(B):
        ok, ids = ok_pixels(tri, tind[b].reshape(-1), nver)
        out[b, ids[:, ok].reshape(-1)] = 1
    return out


def lift(vertex, tind, vis, fine, coarse, ntri):
    """vertex [B,3,nver] fp32 (a pitched tensor's live columns), tind / fine / coarse [B,H,W], vis uint8 [B,nver]
    -> (vertex_out [B,3,nver] fp32, state uint8 [B,nver])"""
    vertex = np.asarray(vertex, np.float32)
    tind, fine, coarse = (np.asarray(a, np.float32) for a in (tind, fine, coarse))
    B, _, nver = vertex.shape
    H, W = tind.shape[1:3]
    out = vertex.copy()
    state = np.zeros((B, nver), np.uint8)
    tt = f2i(tind)
    on_face = (tt >= 0) & (tt < ntri)
    with np.errstate(all="ignore"):
        for b in range(B):
            for v in range(nver):
                if not vis[b, v]:
                    continue
                state[b, v] = 2
                x, y, z = (np.float64(vertex[b, c, v]) for c in range(3))
                if not (np.isfinite(x) and np.isfinite(y)) or ntri <= 0:
                    continue
                c0, r0 = np.floor(x), np.floor(y)
                fx, fy = x - c0, y - r0
                gx, gy = np.float64(1.0) - fx, np.float64(1.0) - fy
                w = (gx * gy, fx * gy, gx * fy, fx * fy)
                num, den, found = np.float64(0.0), np.float64(0.0), False
                for k in range(4):
                    r, c = r0 + (k >> 1), c0 + (k & 1)
                    if not (0 <= r < H and 0 <= c < W) or w[k] == 0.0:
                        continue
                    r, c = int(r), int(c)
                    if not on_face[b, r, c]:
                        continue
                    d = np.float64(fine[b, r, c]) - np.float64(coarse[b, r, c])
                    num = num + w[k] * d
                    den = den + w[k]
                    found = True
                if found:
                    state[b, v] = 1
                    out[b, 2, v] = np.float32(z + num / den)
    return out, state


def vertex_normals(vertex, tri, adj_start, adj_tri):
    """vertex [B,3,nver] fp32, tri [3,ntri], the CSR table -> normal [B,3,nver] fp32"""
    vertex = np.asarray(vertex, np.float32)
    B, _, nver = vertex.shape
    ids = f2i(np.asarray(tri, np.float32))
    ntri = ids.shape[1]
    out = np.zeros((B, 3, nver), np.float32)
    V = vertex.astype(np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            for v in range(nver):
                n = np.zeros(3, np.float64)
                for e in range(max(int(adj_start[v]), 0), min(int(adj_start[v + 1]), 3 * ntri)):
                    t = int(adj_tri[e])
                    if not 0 <= t < ntri:
                        continue
                    p = ids[:, t]
                    if ((p < 0) | (p >= nver)).any():
                        continue
                    P1, P2, P3 = V[b][:, p[0]], V[b][:, p[1]], V[b][:, p[2]]
                    a, c = P2 - P1, P3 - P1
                    n[0] = n[0] + (a[1] * c[2] - a[2] * c[1])
                    n[1] = n[1] + (a[2] * c[0] - a[0] * c[2])
                    n[2] = n[2] + (a[0] * c[1] - a[1] * c[0])
                s = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                if s > 0 and np.isfinite(s):
                    out[b, :, v] = (n / s).astype(np.float32)
    return out


# ---- shapes the tests share ---------------------------------------------------------------------------------------------------------
def layered_scene(nu=9, nv=7, H=12, W=16, B=3, pitch_pad=5, seed=11):
    """A front nu x nv vertex grid (2 (nu - 1)(nv - 1) triangles) over the image with a smaller 4 x 4 layer behind its middle, B
    faces at different poses (a shift, a scale and a shear each; the last face hangs over the image's edge, where the rasteriser
    drops whole triangles and the layer behind shows).  -> dict: vertex [B,3,nver + pitch_pad] fp32 (the pad columns hold NaN),
    nver, tri [3,T] fp32, H, W."""
    rs = np.random.RandomState(seed)
    n_front, n_back = nu * nv, 16
    nver = n_front + n_back
    tri = np.concatenate([grid_mesh(nu, nv), grid_mesh(4, 4, first=n_front)], 1)
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    ju, jv = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    V = np.full((B, 3, nver + pitch_pad), np.nan, np.float32)
    for b in range(B):
        sx, sy = (W - 3.0) / (nv - 1) * (1 + 0.04 * b), (H - 2.5) / (nu - 1) * (1 - 0.03 * b)
        ox, oy = 1.3 + 0.9 * b, 0.8 + 0.35 * b
        x = ox + sx * iv + 0.11 * b * iu + rs.uniform(-0.2, 0.2, iu.shape)
        y = oy + sy * iu + 0.07 * b * iv + rs.uniform(-0.2, 0.2, iu.shape)
        z = 50.0 + 0.8 * iv - 0.6 * iu + rs.uniform(-0.3, 0.3, iu.shape)
        V[b, 0, :n_front], V[b, 1, :n_front], V[b, 2, :n_front] = x.reshape(-1), y.reshape(-1), z.reshape(-1)
        bx = W / 2.0 - 3.0 + 2.1 * jv + 0.5 * b
        by = H / 2.0 - 3.0 + 1.9 * ju + 0.25 * b
        V[b, 0, n_front:nver], V[b, 1, n_front:nver] = bx.reshape(-1), by.reshape(-1)
        V[b, 2, n_front:nver] = 20.0 + 0.5 * jv.reshape(-1)
    return {"vertex": V, "nver": nver, "tri": tri, "H": H, "W": W}


def fine_of(coarse, seed=3, scale=0.3):
    """a fine depth map for a coarse one: the coarse map plus fp32 noise"""
    rs = np.random.RandomState(seed)
    return (np.asarray(coarse, np.float32) + (scale * rs.standard_normal(np.shape(coarse))).astype(np.float32)).astype(np.float32)
def grid_mesh(nu, nv, first=0):
    """the 2 (nu - 1)(nv - 1) triangles of an nu x nv vertex grid (vertex id = first + iu * nv + iv), float32 [3,T], wound so that
    with x growing along iv and y along iu the render's normal (P2 - P1) x (P3 - P1) has n_z > 0"""
    t = []
    for iu in range(nu - 1):
        for iv in range(nv - 1):
            a = first + iu * nv + iv
            b, c, d = a + 1, a + nv, a + nv + 1
            t.append((a, b, c))
            t.append((b, d, c))
    return np.asarray(t, np.float32).T.copy()
