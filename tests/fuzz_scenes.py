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
    specials kind: (flat indices, values))."""

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
    return ConsumerCase(-1, (ver, tri.astype(np.float32), tex, H, W, 3, None))


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
