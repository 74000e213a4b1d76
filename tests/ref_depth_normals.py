"""numpy float64 model of the depth-map normals (fr_depth_normals_forward / _backward), written from the section "depth-map normals"
of include/fr_hotpath.h alone; it shares no code with the product.  TEST INFRASTRUCTURE ONLY.

Per valid pixel, on the fp32 inputs widened to float64, every operation rounded on its own (numpy's elementwise float64):
    dx = (z_R - z_L) * 0.5 | z_R - z_p | z_p - z_L | 0.0     by which of the left / right neighbours are valid;   dy alike by rows
    s = sqrt((dx dx + dy dy) + 1)      n = (-dx / s, -dy / s, 1 / s)
backward:  d = (g_x n_x + g_y n_y) + g_z n_z,  e_x = -((g_x - n_x d) / s),  e_y alike, and the gather of six terms in the header's order.
The model is held to central finite differences of its own forward and to the renderer's normals by tests/test_depth_normals_cpu.py.

The shapes (CASES) sit where the kernels can go wrong: one pixel, one row, one column, height and width each at tile - 1, tile and
tile + 1 (the tile is read from fr_debug_depth_normals_geom), several ragged tiles (33 x 67), one face and three faces with a mask
each.  The masks: NULL, all valid, all invalid, isolated valid pixels, runs of two, a checkerboard, a disc, a NaN entry, a hole on
a tile corner."""
import collections
import ctypes

import numpy as np

MASKS = ("null", "valid", "invalid", "isolated", "runs2", "checker", "disc", "nan", "corner")
# masks under which NO valid pixel has a valid neighbour: every normal is (0, 0, 1) and every gradient exactly 0
FLAT = ("invalid", "isolated", "checker")

Case = collections.namedtuple("Case", "B H W masks")
Model = collections.namedtuple("Model", "normal valid dx dy s")


def tile():
    """(tile width, tile height) of the launchers, from the library's geometry hook (no GPU)"""
    from conftest import pkg
    out = (ctypes.c_int * 6)()
    pkg("_lib").lib().fr_debug_depth_normals_geom(1, 64, 64, out)
    assert out[0] > 1 and out[1] > 1, list(out)
    return int(out[0]), int(out[1])


def cases():
    tw, th = tile()
    shapes = [(1, 1), (1, tw + 5), (th + 3, 1)] + [(h, w) for h in (th - 1, th, th + 1) for w in (tw - 1, tw, tw + 1)]
    out = []
    for i, (H, W) in enumerate(shapes):                      # three masks per small shape, rotating through all nine kinds
        for j in range(3):
            out.append(Case(1, H, W, (MASKS[(3 * i + j) % len(MASKS)],)))
    for m in MASKS:                                          # several tiles, ragged edges: every mask
        out.append(Case(1, 33, 67, (m,)))
    out.append(Case(3, 33, 67, ("disc", "runs2", "corner")))  # a different mask per face
    out.append(Case(3, th + 1, tw + 1, ("checker", "nan", "valid")))
    return tuple(out)


def case_id(c):
    return "B%d_%dx%d_%s" % (c.B, c.H, c.W, "+".join(c.masks))


def make_mask(kind, H, W, rs):
    """fp32 [H,W]: a triangle index >= 0 (0.0 included) at valid pixels, -1 at invalid ones, NaN where the kind says so"""
    tw, th = tile()
    r, c = np.mgrid[0:H, 0:W]
    ids = rs.randint(0, 1000, (H, W)).astype(np.float32)
    ids[0, 0] = 0.0                                           # index 0 is a valid triangle
    if kind in ("null", "valid"):
        v = np.ones((H, W), bool)
    elif kind == "invalid":
        v = np.zeros((H, W), bool)
    elif kind == "isolated":
        v = np.zeros((H, W), bool)
        v[H // 2, W // 2] = True
        if abs(H // 2 - 0) + abs(W // 2 - (W - 1)) >= 2:
            v[0, W - 1] = True
    elif kind == "runs2":
        v = (r % 3 != 2) & (c % 3 != 2)
    elif kind == "checker":
        v = (r + c) % 2 == 0
    elif kind == "disc":
        v = ((r - (H - 1) / 2.0) / (H / 2.0)) ** 2 + ((c - (W - 1) / 2.0) / (W / 2.0)) ** 2 <= 0.9
    elif kind == "nan":
        v = rs.uniform(size=(H, W)) >= 0.1
    elif kind == "corner":
        v = np.ones((H, W), bool)
        v[max(th - 1, 0):th + 1, max(tw - 1, 0):tw + 1] = False
    else:
        raise ValueError(kind)
    m = np.where(v, ids, np.float32(-1.0)).astype(np.float32)
    if kind == "nan":
        m[H // 2, W // 2] = np.nan
        m[H - 1, 0] = np.nan
    return m


def inputs(case, seed=1):
    """-> dict of fp32 arrays: depth [B,H,W,1] (order 1-100, slopes of order 1: no non-zero output is subnormal), mask [B,H,W,1] or
    None (the case's single mask is "null"), grad_normal [B,H,W,3] standard normal"""
    B, H, W = case.B, case.H, case.W
    rs = np.random.RandomState(seed)
    r, c = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.empty((B, H, W))
    for b in range(B):
        a, bb = rs.uniform(-1.5, 1.5, 2)
        z[b] = 50.0 + a * (c - W / 2.0) * 0.3 + bb * (r - H / 2.0) * 0.3 + 3.0 * np.sin(0.5 * c + b) * np.cos(0.3 * r) \
            + 0.5 * rs.standard_normal((H, W))
    z = np.clip(z, 1.0, 100.0)
    d = {"depth": z.astype(np.float32)[..., None]}
    masks = [make_mask(k, H, W, rs) for k in case.masks]
    d["mask"] = None if case.masks == ("null",) else np.stack(masks)[..., None].astype(np.float32)
    d["grad_normal"] = rs.standard_normal((B, H, W, 3)).astype(np.float32)
    return d


def valid_of(mask, shape):
    if mask is None:
        return np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32).reshape(shape) >= 0


def _sh(a, dr, dc, fill):
    """out[b, r, c] = a[b, r + dr, c + dc], `fill` outside the image"""
    B, H, W = a.shape
    out = np.full_like(a, fill)
    rs, re = max(0, -dr), min(H, H - dr)
    cs, ce = max(0, -dc), min(W, W - dc)
    if rs < re and cs < ce:
        out[:, rs:re, cs:ce] = a[:, rs + dr:re + dr, cs + dc:ce + dc]
    return out


def _diff(z, lo, hi, dr, dc):
    zl, zh = _sh(z, -dr, -dc, 0.0), _sh(z, dr, dc, 0.0)
    return np.where(lo & hi, (zh - zl) * 0.5, np.where(hi, zh - z, np.where(lo, z - zl, 0.0)))


def _nbrs(v):
    return _sh(v, 0, -1, False), _sh(v, 0, 1, False), _sh(v, -1, 0, False), _sh(v, 1, 0, False)    # L, R, U, D


def forward(depth, mask):
    """-> Model(normal [B,H,W,3] float64 BEFORE its rounding to fp32, valid [B,H,W], dx, dy, s)"""
    z = np.asarray(depth, np.float32).astype(np.float64)
    z = z.reshape(z.shape[:3])
    v = valid_of(mask, z.shape)
    L, R, U, D = _nbrs(v)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.where(v, _diff(z, L, R, 0, 1), 0.0)
        dy = np.where(v, _diff(z, U, D, 1, 0), 0.0)
        s = np.sqrt((dx * dx + dy * dy) + 1.0)
        n = np.stack([-dx / s, -dy / s, 1.0 / s], -1)
    return Model(np.where(v[..., None], n, 0.0), v, dx, dy, s)


def backward(grad_normal, depth, mask, m=None):
    """-> (G [B,H,W,1] float64 before rounding, A [B,H,W,1] = the sum of the absolute values of the six terms)"""
    m = forward(depth, mask) if m is None else m
    g = np.asarray(grad_normal, np.float32).astype(np.float64)
    v = m.valid
    L, R, U, D = _nbrs(v)
    with np.errstate(invalid="ignore", over="ignore"):
        nx, ny, nz = -m.dx / m.s, -m.dy / m.s, 1.0 / m.s
        d = (g[..., 0] * nx + g[..., 1] * ny) + g[..., 2] * nz
        ex = np.where(v, -((g[..., 0] - nx * d) / m.s), 0.0)
        ey = np.where(v, -((g[..., 1] - ny * d) / m.s), 0.0)
    wx = ex * np.where(L & R, 0.5, 1.0)
    wy = ey * np.where(U & D, 0.5, 1.0)
    terms = [np.where(R & ~L, -ex, np.where(L & ~R, ex, 0.0)),
             np.where(D & ~U, -ey, np.where(U & ~D, ey, 0.0)),
             np.where(L, _sh(wx, 0, -1, 0.0), 0.0),
             np.where(R, -_sh(wx, 0, 1, 0.0), 0.0),
             np.where(U, _sh(wy, -1, 0, 0.0), 0.0),
             np.where(D, -_sh(wy, 1, 0, 0.0), 0.0)]
    G = ((((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]) + terms[5]
    A = sum(np.abs(t) for t in terms)
    return np.where(v, G, 0.0)[..., None], np.where(v, A, 0.0)[..., None]
