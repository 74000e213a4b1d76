"""The seeded scene generator of the fuzz tests (tests/test_fuzz_gpu.py, tests/test_fuzz_consumers_gpu.py and the CPU test that
holds the consumers' seed set to its conditions, tests/test_fuzz_scenes_cpu.py): scene type, batch, image size, triangle count,
coordinate scale and special values are all drawn from the seed, so every case is reproducible by its id."""
import copy

import numpy as np

KINDS = ("jittered grid", "soup", "small-triangle soup", "integer coordinates with ties", "specials")
CONSUMER_FACES = 8             # a batch that is a multiple of 8 takes the owners' XCD block map
CONSUMER_PIXELS = 200_000      # B*H*W a consumer case may have: the models run in a few seconds below it
CONSUMER_STRIDE = 100_000      # the seed stride a too large scene is skipped by (as test_fused_rendering_layer skips)
CONSUMER_BASE = 31000          # the consumers' seed base: chosen on the CPU by tests/test_fuzz_scenes_cpu.py (its docstring)
ALBEDO_K = (1, 10, 15)         # the albedo fit's basis widths a case draws from: the smallest, the standard one and the largest served
# the colour sampler's ranges (rendering_layer.ops.SYNTH_LIGHT_RANGES_RGB), stated here on their own as tests/ref_photo_rgb.py does
LIGHT_RANGES_RGB = tuple(((0.3, 0.7), (-0.4, 0.4), (-0.4, 0.4), (0.2, 0.9))[k] if k < 4 else (-0.15, 0.15) for c in range(3) for k in range(9))


def _draw(seed):
    """-> (ver [B,3,nver], tri [3,ntri] float-stored, tex [1 or B,3,nver], H, W, kind: an index into KINDS)"""
    rs = np.random.RandomState(seed)
    B = int(rs.choice([1, 1, 2, 3, 5, 8, 17, 64, 70]))
    H = int(rs.choice([1, 2, 3, 5, 9, 16, 31, 40, 64, 100, 200, 257]))
    W = int(rs.choice([1, 2, 4, 7, 8, 9, 33, 64, 100, 200, 300]))
    if B * H * W > 3_000_000:
        B = max(1, 3_000_000 // (H * W))
    kind = int(rs.randint(0, 5))
    if kind == 0:      # jittered sub-pixel grid (the 3DMM regime), random triangle order
        nu, nv = max(2, int(H * rs.uniform(0.8, 1.6))), max(2, int(W * rs.uniform(0.8, 1.6)))
        gx, gy = np.meshgrid(np.linspace(-2.0, W + 1.0, nv), np.linspace(-2.0, H + 1.0, nu))
        nver = nu * nv
        ver = np.empty((B, 3, nver), np.float32)
        j = rs.uniform(0.0, 0.6)
        for b in range(B):
            ver[b, 0] = (gx + rs.uniform(-j, j, gx.shape)).reshape(-1)
            ver[b, 1] = (gy + rs.uniform(-j, j, gy.shape)).reshape(-1)
            ver[b, 2] = rs.uniform(-5, 5, nver)
        iu, iv = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="ij")
        v00 = (iu * nv + iv).reshape(-1)
        tri = np.concatenate([np.stack([v00, v00 + nv, v00 + 1]), np.stack([v00 + 1, v00 + nv, v00 + nv + 1])], 1)
        tri = tri[:, rs.permutation(tri.shape[1])]
    else:
        nver = int(rs.randint(3, 3000))
        ntri = int(rs.randint(1, 6000))
        ver = np.empty((B, 3, nver), np.float32)
        ver[:, 0] = rs.uniform(-0.2 * W - 1, 1.2 * W + 1, (B, nver))
        ver[:, 1] = rs.uniform(-0.2 * H - 1, 1.2 * H + 1, (B, nver))
        ver[:, 2] = rs.uniform(-50, 50, (B, nver))
        tri = rs.randint(0, nver, (3, ntri))
        if kind >= 2:   # most triangles small: two vertices near the first
            scale = float(rs.choice([0.3, 1.0, 3.0, 12.0]))
            k = min(ntri, nver // 3)
            idx = rs.permutation(nver)[:3 * k].reshape(-1, 3)
            for b in range(B):
                c = ver[b, :2][:, idx[:, 0]]
                ver[b, :2][:, idx[:, 1]] = c + rs.uniform(-scale, scale, c.shape).astype(np.float32)
                ver[b, :2][:, idx[:, 2]] = c + rs.uniform(-scale, scale, c.shape).astype(np.float32)
            tri[:, :k] = idx.T
        if kind == 3:   # integer coordinates: pixel centres on edges and vertices, equal depths (ties)
            ver[:, :2] = np.round(ver[:, :2])
            ver[:, 2] = np.round(ver[:, 2] / 10)
        if kind == 4:   # duplicates, degenerate triangles and special values
            tri[:, ::7] = tri[:, ::7][:, ::-1] if tri[:, ::7].shape[1] > 1 else tri[:, ::7]
            tri[1, ::11] = tri[0, ::11]
            flat = ver.reshape(-1)
            for val in (np.nan, np.inf, -np.inf, 3e9, -3e9, 1e-40, -0.0):
                flat[rs.randint(0, flat.size, 3)] = val
    tri = tri.astype(np.float32)
    if kind == 4:
        tri[rs.randint(0, 3), rs.randint(0, tri.shape[1])] = -1.0
        tri[rs.randint(0, 3), rs.randint(0, tri.shape[1])] = float(nver)
        tri[rs.randint(0, 3), rs.randint(0, tri.shape[1])] = np.nan
        tri[rs.randint(0, 3), rs.randint(0, tri.shape[1])] = 0.75
    tex_b = B if rs.rand() < 0.5 else 1
    tex = rs.uniform(0, 1, (tex_b, 3, nver)).astype(np.float32)
    return ver, tri, tex, H, W, kind


def _scene(seed):
    return _draw(seed)[:5]


def consumer_scene(seed):
    """_scene cut down so that a case with its numpy models runs in a few seconds: at most CONSUMER_FACES faces (the first of `ver`,
    and of `tex` when it is per-face), and a scene that still has more than CONSUMER_PIXELS pixels is skipped by the fixed seed
    stride.  -> (ver, tri, tex, H, W, kind, the seed the scene was drawn from)"""
    s = seed
    while True:
        ver, tri, tex, H, W, kind = _draw(s)
        per_face = tex.shape[0] == ver.shape[0]
        ver = np.ascontiguousarray(ver[:CONSUMER_FACES])
        if per_face:
            tex = np.ascontiguousarray(tex[:CONSUMER_FACES])
        if ver.shape[0] * H * W <= CONSUMER_PIXELS:
            return ver, tri, tex, H, W, kind, s
        s += CONSUMER_STRIDE


class ConsumerCase:
    """Everything a consumer case draws, from its seed alone: the scene (ver, tri, tex, H, W, kind, B, nver, tex_batch), and for the
    consumers g_normal / g_depth / g_tex (each a pair: the two gradient profiles), `old` (a finite tensor to accumulate onto),
    light, target, weight (odd seeds; else None), grad_sse and fine_noise (pixels of the fine depth map that get NaN / Inf on the
    specials kind: (flat indices, values)).  The soft coverage, the colour shading and the albedo fit draw theirs from a later stream
    (_draw_later_consumers), and the coverage has a pass of its own (vertex_altered)."""

    def __init__(self, index, scene=None):
        self.index, self.seed = index, CONSUMER_BASE + index
        self.ver, self.tri, self.tex, self.H, self.W, self.kind, self.drawn_from = scene or consumer_scene(self.seed)
        self.B, self.nver, self.tex_batch = self.ver.shape[0], self.ver.shape[2], self.tex.shape[0]
        B, npix = self.B, self.H * self.W
        rs = np.random.RandomState(self.seed + 500_000_000)
        pair = lambda shape: (lambda g: (g, second_gradient(rs, g)))(uniform_gradient(rs, shape))   # noqa: E731
        self.g_normal, self.g_depth, self.g_tex = pair((B, npix, 3)), pair((B, npix)), pair((B, npix, 3))
        self.old = rs.standard_normal((B, 3, self.nver)).astype(np.float32)
        self.light = rs.uniform(-1, 1, (B, 4)).astype(np.float32)
        self.target = rs.uniform(0, 1, (B, self.H, self.W, 1)).astype(np.float32)
        weight = rs.uniform(0.25, 2.0, (B, self.H, self.W, 1)).astype(np.float32)
        self.weight = weight if self.seed % 2 else None
        self.grad_sse = rs.uniform(-2, 2, B)
        where = rs.randint(0, B * npix, 4)
        self.fine_noise = (where, np.float32([np.nan, np.inf, -np.inf, np.nan])) if self.kind == 4 else (where[:0], np.float32([]))
        self._draw_later_consumers()

    def _draw_later_consumers(self):
        """What the soft coverage, the colour shading and the albedo fit draw, from a stream of their own (the attributes above keep
        their bytes): g_cov (a pair, [B,npix]); light_rgb [B,3,9] uniform in LIGHT_RANGES_RGB -- the colour sampler's ranges, under
        which a channel is unlit on some pixels of some cases and lit on most -- target_rgb [B,H,W,3] and background_rgb (None,
        [1,H,W,3] or [B,H,W,3]: bg_kind 0, 1, 2); K in ALBEDO_K, pc_tex [3 nver,K] fp32, lighting [3,npix] float64, abedo and
        im_gray [B,H,W,1] (on the specials kind im_gray holds a NaN and an Inf somewhere)."""
        B, H, W, npix = self.B, self.H, self.W, self.H * self.W
        rs = np.random.RandomState(self.seed + 700_000_000)
        g = uniform_gradient(rs, (B, npix))
        self.g_cov = (g, second_gradient(rs, g))
        lo, hi = np.asarray(LIGHT_RANGES_RGB, np.float64).T
        self.light_rgb = rs.uniform(lo, hi, (B, 27)).astype(np.float32).reshape(B, 3, 9)
        self.target_rgb = rs.uniform(0, 1, (B, H, W, 3)).astype(np.float32)
        self.bg_kind = int(rs.randint(0, 3))
        bg = rs.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)
        self.background_rgb = (None, bg[:1], bg)[self.bg_kind]
        self.K = int(rs.choice(ALBEDO_K))
        self.pc_tex = (0.05 * rs.standard_normal((3 * self.nver, self.K))).astype(np.float32)
        self.lighting = np.array([0.2, 0.1, 0.9])[:, None] + 0.1 * rs.standard_normal((3, npix))
        self.abedo = rs.uniform(0.2, 0.8, (B, H, W, 1)).astype(np.float32)
        self.im_gray = rs.uniform(0, 1, (B, H, W, 1)).astype(np.float32)
        if self.kind == 4:
            self.im_gray.reshape(-1)[rs.randint(0, B * npix, 2)] = (np.nan, np.inf)

    def vertex_altered(self, tri_ind):
        """The pass the soft coverage needs and no render produces: the rasteriser never lets a triangle with a non-finite area win a
        pixel, so the coverage's exits for such a triangle (area, or s_k, not finite) are never taken on a rendered scene.  -> a copy
        of the case in which up to four (face, triangle) of those that own an OK pixel with a not-OK 4-neighbour (OK by the case's
        own table and `tri_ind` [B,H*W]) have the x or the y of one vertex set to NaN, +Inf, -3e38 and 1e30 in turn; the four
        triangles differ where the scene has that many.  `poisoned` lists them as (face, triangle, vertex, row, value).  The
        consumer is handed `tri_ind` as it is -- the plane of the UNPOISONED scene."""
        import ref_coverage as RC
        import ref_normal_backward as RN
        rs = np.random.RandomState(self.seed + 800_000_000)
        other = copy.copy(self)
        other.ver = self.ver.copy()
        other.poisoned = []
        tind = np.asarray(tri_ind, np.float32).reshape(self.B, -1)
        owners = []
        for b in range(self.B):
            okt, _ = RC.ok_triangles(self.tri, tind[b], self.nver)
            border = RC._border(okt, self.H, self.W)
            owners += [(b, int(t)) for t in np.unique(okt[border][okt[border] >= 0])]
        order = rs.permutation(len(owners))
        ids = RN.f2i_x86(self.tri)
        taken = set()
        for val in (np.nan, np.inf, -3e38, 1e30):
            pick = [owners[i] for i in order if owners[i][1] not in taken] or [owners[i] for i in order]
            if not pick:
                break
            b, t = pick[0]
            taken.add(t)
            v, row = int(ids[rs.randint(0, 3), t]), int(rs.randint(0, 2))
            other.ver[b, row, v] = val
            other.poisoned.append((b, t, v, row, float(val)))
        return other

    def vertex_on_segment(self, tri_ind):
        """The other class no scene holds: two edges that tie on s with 0 < s < 1, where the winning edge decides which vertices the
        backward's terms go to.  (On the lattice scenes every tie is at s = 0, a pixel centre on a vertex: no record is written and
        the forward cannot tell the edges apart.)  It takes a vertex of the OK pixel's triangle exactly ON the segment from the
        pixel's centre c to its not-OK neighbour's n, with c inside the triangle.  -> a copy of the case in which up to four
        triangles that own such a pixel have one vertex moved to c + s0 (n - c), s0 = 0.25, 0.75 in turn (s < 0.5 passes the OK
        pixel's gradient back, s > 0.5 the neighbour's), wherever the move gives an exact tie; `moved` lists them as (face,
        triangle, vertex, pixel, neighbour, s0).  No two of the triangles share a vertex.  The consumer is handed `tri_ind` as it
        is, as in vertex_altered."""
        import ref_coverage as RC
        rs = np.random.RandomState(self.seed + 900_000_000)
        other = copy.copy(self)
        other.ver = self.ver.copy()
        other.moved = []
        H, W = self.H, self.W
        tind = np.asarray(tri_ind, np.float32).reshape(self.B, -1)
        for b in rs.permutation(self.B):
            okt, tid = RC.ok_triangles(self.tri, tind[b], self.nver)
            border = RC._border(okt, H, W)
            fixed = set()
            for i in rs.permutation(border[okt[border] >= 0])[:64]:
                t = int(okt[i])
                if len(other.moved) == 4:
                    return other
                if fixed & set(tid[:, t].tolist()):
                    continue
                y, x = divmod(int(i), W)
                s0 = (0.25, 0.75)[len(other.moved) % 2]
                for (dx, dy), k in ((d, k) for d in RC.NEIGHBOURS for k in range(3)):
                    nx, ny = x + dx, y + dy
                    if nx < 0 or nx >= W or ny < 0 or ny >= H or okt[ny * W + nx] >= 0:
                        continue
                    v = int(tid[k, t])
                    old = other.ver[b, :2, v].copy()
                    other.ver[b, :2, v] = (x + s0 * dx, y + s0 * dy)
                    sk = candidate_s(RC._tri_xy(other.ver[b], tid, t), (x, y), (nx, ny))
                    if sk and sk.count(min(sk)) > 1 and 0.0 < min(sk) < 1.0:
                        other.moved.append((int(b), t, v, int(i), ny * W + nx, s0))
                        fixed |= set(tid[:, t].tolist())
                        break
                    other.ver[b, :2, v] = old
        return other

    def altered(self, tri_ind):
        """The rasteriser skips a triangle with an id outside the mesh and writes whole triangle indices or -1, so on a rendered
        scene the consumers' own tests of the ids and of the plane see nothing, and their two rules -- COUNTED iff
        0 <= (int)tri_ind < ntri with all ids in range, COVERED iff tri_ind >= 0 -- never part.  -> (a copy of the case, a copy of
        tri_ind [B,H*W]) as handed to the CONSUMERS in a second pass:
          the table   a bad id in up to three triangles that win pixels: the third id becomes nver, the second -1, the first NaN;
          the plane   up to three covered pixels become NaN (uncovered by both rules), ntri (covered, not counted) and their own
                      value + 0.5 (the same triangle), and two pixels anywhere become NaN and -0.0 (covered: triangle 0)."""
        rs = np.random.RandomState(self.seed + 600_000_000)
        other = copy.copy(self)
        other.tri = self.tri.copy()
        plane = np.array(tri_ind, np.float32)
        flat = plane.reshape(-1)
        winners = np.unique(flat[flat >= 0]).astype(np.int64)
        if winners.size:
            for t, (k, val) in zip(rs.choice(winners, min(3, winners.size), replace=False), ((2, self.nver), (1, -1.0), (0, np.nan))):
                other.tri[k, t] = val
            covered = np.flatnonzero(flat >= 0)
            for i, val in zip(rs.choice(covered, min(3, covered.size), replace=False), (np.nan, float(self.tri.shape[1]), None)):
                flat[i] = flat[i] + 0.5 if val is None else val
        flat[rs.randint(0, flat.size, 2)] = (np.nan, -0.0)
        return other, plane

    def with_noise(self, fine):
        """`fine` (ref_mesh.fine_of of the coarse plane) with the case's NaN / Inf written into it"""
        fine = np.array(fine, np.float32)
        fine.reshape(-1)[self.fine_noise[0]] = self.fine_noise[1]
        return fine


def clamp_scene():
    """The hand-made scene for the one class the seeds cannot reach (tests/test_fuzz_scenes_cpu.py): a texture with values below the
    shader's clamp of 1e-6 under covered pixels.  Three faces of 12 x 16, 60 vertices on the integer lattice, 90 triangles of
    which every fifth names a vertex twice (a segment: it paints the pixel centres it holds with a zero normal), a texture drawn
    from (-0.4, 1); lights of both signs, so that with the flipped and the unflipped normals every branch of the shader is taken."""
    rs = np.random.RandomState(12)
    B, H, W, nver, ntri = 3, 12, 16, 60, 90
    ver = np.empty((B, 3, nver), np.float32)
    ver[:, 0] = np.round(rs.uniform(-2, W + 1, (B, nver)))
    ver[:, 1] = np.round(rs.uniform(-2, H + 1, (B, nver)))
    ver[:, 2] = rs.uniform(-50, 50, (B, nver))
    tri = rs.randint(0, nver, (3, ntri))
    tri[1, ::5] = tri[0, ::5]
    ver[:, 2, tri[0, ::5]] = 60.0                                              # the segments in front
    tex = rs.uniform(-0.4, 1.0, (B, 3, nver)).astype(np.float32)
    case = ConsumerCase(-1, (ver, tri.astype(np.float32), tex, H, W, 3, None))
    # colour lights of both signs in every channel (the sampler's ranges leave most pixels lit): every entry of
    # ref_photo_rgb.BRANCHES is taken on this scene, the per-channel clamp included
    case.light_rgb = np.random.RandomState(13).uniform(-1, 1, (B, 3, 9)).astype(np.float32)
    return case


def candidate_s(P, c, n):
    """the s_k of the candidate edges of the soft coverage's pair (c, n) for the triangle P = ((x1, y1), (x2, y2), (x3, y3)), by
    ref_coverage's edge function and the header's rule -> list (empty: the pair is inert)"""
    import math

    import ref_coverage as RC
    area = RC.edge(P[0][0], P[0][1], P[1][0], P[1][1], P[2][0], P[2][1])
    if area == 0 or not math.isfinite(area):
        return []
    sigma, out = (1.0 if area > 0 else -1.0), []
    for k in range(3):
        A, B = P[k], P[(k + 1) % 3]
        fc = sigma * RC.edge(A[0], A[1], B[0], B[1], float(c[0]), float(c[1]))
        fn = sigma * RC.edge(A[0], A[1], B[0], B[1], float(n[0]), float(n[1]))
        if fn < 0 and fc > fn and math.isfinite(RC._div(fc, fc - fn)):
            out.append(RC._div(fc, fc - fn))
    return out


def uniform_gradient(rs, shape):
    """the fuzz's first gradient profile: uniform in (-2, 2) with about 30 % exact zeros"""
    return (rs.uniform(-2, 2, shape) * (rs.rand(*shape) < 0.7)).astype(np.float32)


def second_gradient(rs, g):
    """the fuzz's second profile, drawn from the same stream: 12 decades of magnitude, or `g` (the uniform one) with a few Inf /
    NaN / subnormal / +-0 entries placed anywhere, covered or not"""
    if rs.rand() < 0.5:
        return (rs.standard_normal(g.shape) * np.exp(rs.uniform(-14, 14, g.shape))).astype(np.float32)
    g2 = g.copy()
    flat = g2.reshape(-1)
    for val in (np.inf, -np.inf, np.nan, 1e-40, -3e-45, 0.0, -0.0, 1.5e-38):
        flat[rs.randint(0, flat.size, 2)] = val
    return g2
