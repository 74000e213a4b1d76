"""GPU: the emit kernel's entry chain and its mask bookkeeping (csrc/fr_render.hip: RenderArgs' leading block, the division-free
workgroup -> (face, segment) decomposition, the XCD remap from host constants, the header check behind the gathers, the predicates
kept as lane masks), through the C ABI and bit for bit against the oracle rasteriser on all four planes."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import assert_render_equal

pytestmark = pytest.mark.gpu
SEG, EMIT_ACTIVE = 504, 252     # triangles per segment, lanes that own two of them (fr_render.hip)


def _capi(ver, tri, tex, H, W, phases=7, ws=None, nver=None, pitched=False):
    """fr_render_depth_forward_phases on dense [B,3,N] rows, or -- pitched -- fr_decode_render_forward without its decode phase on
    rows of fr_decode_render_vertex_pitch(N) floats.  Returns the four planes (pre-filled with 7 so that nothing unwritten passes)."""
    h = pkg("_lib")
    L = h.lib()
    dev = torch.device("cuda:0")
    B, _, N = ver.shape
    nver = N if nver is None else nver
    ntri, tb = tri.shape[1], tex.shape[0]
    tri_t = torch.as_tensor(np.ascontiguousarray(tri, np.float32), device=dev)
    tex_t = torch.as_tensor(np.ascontiguousarray(tex, np.float32), device=dev)
    outs = [torch.full((B, H, W, c), 7.0, device=dev) for c in (1, 3, 3, 1)]
    nws = L.fr_render_depth_workspace_bytes(B, nver, ntri, H, W)
    if ws is None:
        ws = torch.zeros((nws + 64,), dtype=torch.uint8, device=dev)
    assert ws.numel() >= nws
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if pitched:
        pitch = L.fr_decode_render_vertex_pitch(N)
        nvb = L.fr_decode_render_vertex_bytes(B, N)
        rows = np.full((B, 3, pitch), np.nan, np.float32)      # the pad floats are never read: a NaN there must not matter
        rows[:, :, :N] = ver
        buf = torch.zeros((nvb // 4 + 64,), dtype=torch.float32, device=dev)
        off = (-buf.data_ptr() % 128) // 4
        vt = buf[off:off + B * 3 * pitch]
        vt.copy_(torch.as_tensor(rows.reshape(-1), device=dev))
        rc = L.fr_decode_render_forward(None, None, None, h.ptr(tri_t), h.ptr(tex_t), B, N, 0, 0, ntri, H, W, tb, float(max(H, W)),
                                        h.ptr(vt), nvb, h.ptr(outs[0]), h.ptr(outs[1]), h.ptr(outs[2]), h.ptr(outs[3]), h.ptr(ws),
                                        nws, st, phases)
    else:
        ver_t = torch.as_tensor(np.ascontiguousarray(ver, np.float32), device=dev)
        rc = L.fr_render_depth_forward_phases(h.ptr(ver_t), h.ptr(tri_t), h.ptr(tex_t), B, nver, ntri, H, W, 3, tb, h.ptr(outs[0]),
                                              h.ptr(outs[1]), h.ptr(outs[2]), h.ptr(outs[3]), h.ptr(ws), nws, st, phases)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


# ---- a small jittered grid mesh, another pose per face --------------------------------------------------------------------------
NU = NV = 29                                  # 841 vertices, 1,568 triangles: enough for the largest list below (1,513)


def _grid_tris(rs):
    iu, iv = np.meshgrid(np.arange(NU - 1), np.arange(NV - 1), indexing="ij")
    v00 = (iu * NV + iv).reshape(-1)
    tri = np.concatenate([np.stack([v00, v00 + NV, v00 + 1]), np.stack([v00 + 1, v00 + NV, v00 + NV + 1])], 1)
    return tri[:, rs.permutation(tri.shape[1])].astype(np.float32)


def _posed_grid(rs, B, H, W):
    """The grid, jittered, under a different rotation / scale / offset per face: handing a workgroup another face's vertices or
    another segment's triangles changes pixels."""
    gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, NV), np.linspace(-1.0, 1.0, NU))
    ver = np.empty((B, 3, NU * NV), np.float32)
    for b in range(B):
        ang = 0.7 * b + rs.uniform(0, 0.3)
        s = (0.45 + 0.07 * (b % 4)) * min(H, W)
        x = gx + rs.uniform(-0.02, 0.02, gx.shape)
        y = gy + rs.uniform(-0.02, 0.02, gy.shape)
        ver[b, 0] = (s * (np.cos(ang) * x - np.sin(ang) * y) + 0.5 * W + rs.uniform(-2, 2)).reshape(-1)
        ver[b, 1] = (s * (np.sin(ang) * x + np.cos(ang) * y) + 0.5 * H + rs.uniform(-2, 2)).reshape(-1)
        ver[b, 2] = rs.uniform(-5, 5, NU * NV)
    return ver


_DECOMP = {}


def _decomp_scene(B, T, H, W):
    key = (B, T, H, W)
    if key not in _DECOMP:
        rs = np.random.RandomState(1000 * B + T + H)
        tb = 1 if (B + T) % 2 else B          # the texture shared by the batch (face 0's workgroups fill the table) or one per face
        _DECOMP[key] = (_posed_grid(rs, B, H, W), _grid_tris(rs)[:, :T].copy(),
                        rs.uniform(0, 1, (tb, 3, NU * NV)).astype(np.float32))
    return _DECOMP[key]


@pytest.mark.parametrize("T", [1, 503, 504, 505, 1008, 1009, 1513])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 8, 9])
def test_workgroup_to_face_and_segment(oracle, B, T):
    """nseg = ceil(T / 504) is 1 .. 4 and the emit grid B * nseg takes 1, 2, 3, 5, 8, 9, 15, 16, 27, 36 and eight more values (7 and
    17 are no product of these B and nseg; 15 | 16 and 8 | 9 sit on either side of a multiple of 8, where the XCD remap's runs
    change length), with nseg = 1, where the reciprocal is 2^31, among them.  Every workgroup must find its own face and segment:
    each face has another pose."""
    nseg = (T + SEG - 1) // SEG
    assert 1 <= nseg <= 4
    for H, W in ((32, 32), (40, 48)):
        ver, tri, tex = _decomp_scene(B, T, H, W)
        want = oracle.render_depth(ver, tri, tex, H, W)
        if T >= 503:
            assert (want[3] >= 0).mean() > 0.05, "the mesh covers part of the image"
        assert_render_equal(_capi(ver, tri, tex, H, W), want, "B=%d T=%d nseg=%d %dx%d" % (B, T, nseg, H, W))


# ---- mask paths: one 504-triangle segment each, every FR_EMIT_FILTER ---------------------------------------------------------------
MH = MW = 32


def _tri_soup(tris, zs, faces=2):
    """[(p1, p2, p3)] with own vertices per triangle -> (vertex [faces,3,3T] (face f shifted by f px in x), tri, texture)."""
    nt = len(tris)
    P = np.array(tris, np.float64).reshape(nt * 3, 2)
    ver = np.zeros((faces, 3, 3 * nt), np.float32)
    for f in range(faces):
        ver[f, 0], ver[f, 1], ver[f, 2] = P[:, 0] + f, P[:, 1], np.asarray(zs).reshape(-1)
    tri = np.arange(3 * nt, dtype=np.float32).reshape(nt, 3).T.copy()
    return ver, tri


def _single(c, r=0.3):       # holds the pixel centre c and no other: a single-pixel bbox that every filter keeps
    return ((c[0] - r, c[1] - r), (c[0] + r, c[1] - r), (c[0], c[1] + r))


def _multi(c):               # a 2 x 2 pixel bbox around c .. c+1
    return ((c[0] - 0.2, c[1] - 0.2), (c[0] + 1.2, c[1] - 0.1), (c[0] + 0.1, c[1] + 1.2))


def _miss(c, k):             # no survivor: off the screen, or no pixel centre in the bbox
    return _single((-5.0 - c[0], c[1])) if k % 2 else ((c[0] + 0.2, c[1] + 0.2), (c[0] + 0.6, c[1] + 0.3), (c[0] + 0.3, c[1] + 0.7))


def _mask_scene(kind):
    rs = np.random.RandomState({"all_single": 1, "none": 2, "edges": 3, "mixed": 4}[kind])
    cells = [(2 + i % 26, 2 + i // 26) for i in range(SEG)]            # 504 distinct pixel centres, a margin for the shifted face
    if kind == "all_single":
        tris = [_single(c) for c in cells]
    elif kind == "none":
        tris = [_miss(c, k) for k, c in enumerate(cells)]
    elif kind == "edges":
        # list order is the lane order here (FR_EMIT_ORDER = 0): position p is lane p % 252's triangle p // 252.  Survivors at the
        # wave edge (lanes 63, 64, 65) and at the last owning lane and its neighbour position (251 | 252 = lane 0's second triangle),
        # for both triangles of those lanes
        keep = {63, 64, 65, 251, 252, EMIT_ACTIVE + 63, EMIT_ACTIVE + 64, EMIT_ACTIVE + 65, SEG - 1}
        tris = [_single(c) if k in keep else _miss(c, k) for k, c in enumerate(cells)]
    else:
        # every triangle survives, about half of them with a multi-pixel bbox, interleaved: the single-pixel ones fill the queue
        # from slot 0 up, the others from slot 503 down, and the two ends meet (504 survivors = the queue's capacity)
        pick = rs.rand(SEG) < 0.5
        tris = [_multi(c) if pick[k] else _single(c) for k, c in enumerate(cells)]
    ver, tri = _tri_soup(tris, rs.uniform(1, 50, (SEG, 3)))
    tex = rs.uniform(0, 1, (1 if kind in ("all_single", "edges") else 2, 3, ver.shape[2])).astype(np.float32)
    return ver, tri, tex


_MASK_WANT = {}


@pytest.mark.parametrize("filt", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["all_single", "none", "edges", "mixed"])
def test_mask_paths(oracle, kind, filt):
    ver, tri, tex = _mask_scene(kind)
    assert tri.shape[1] == SEG
    if kind not in _MASK_WANT:
        _MASK_WANT[kind] = oracle.render_depth(ver, tri, tex, MH, MW)
    want = _MASK_WANT[kind]
    covered = int((want[3][0] >= 0).sum())
    if kind == "all_single":
        assert covered == SEG                     # every triangle owns its pixel: all 504 survive and hit
    elif kind == "none":
        assert covered == 0
    elif kind == "edges":
        assert covered == 9 and sorted(set(want[3][0].reshape(-1).astype(int)) - {-1}) == [63, 64, 65, 251, 252, 315, 316, 317, 503]
    else:
        assert covered > SEG
    with pkg("_lib").options(FR_EMIT_FILTER=filt, FR_EMIT_ORDER=0):
        assert_render_equal(_capi(ver, tri, tex, MH, MW), want, "%s FR_EMIT_FILTER=%d" % (kind, filt))


# ---- the table header: packed for another nver -> pure background ---------------------------------------------------------------------
def test_header_of_another_nver_gives_background_then_the_scene(oracle):
    """Pack the table for (nver', ntri) with nver' < nver, then emit + resolve with nver: every stale offset stays inside the vertex
    rows, the header's nver does not match, every triangle is invalid and the planes are what the oracle gives for an empty
    list.  With the right header the scene is back."""
    rs = np.random.RandomState(31)
    B, H, W, T = 3, 32, 32, 1009
    ver, tri, tex = _posed_grid(rs, B, H, W), _grid_tris(rs)[:, :T].copy(), rs.uniform(0, 1, (B, 3, NU * NV)).astype(np.float32)
    N, Np = NU * NV, NU * NV - 1
    tri = np.minimum(tri, Np - 1)                    # every id is valid for nver' = N - 1 too
    h = pkg("_lib")
    nws = h.lib().fr_render_depth_workspace_bytes(B, N, T, H, W)
    assert nws == h.lib().fr_render_depth_workspace_bytes(B, Np, T, H, W)   # same table position: only the header differs
    ws = torch.zeros((nws + 64,), dtype=torch.uint8, device="cuda:0")
    _capi(ver[:, :, :Np].copy(), tri, tex[:, :, :Np].copy(), H, W, phases=4, ws=ws)            # pack for nver' = N - 1
    empty = oracle.render_depth(ver, np.zeros((3, 0), np.float32), tex, H, W)
    assert (empty[3] == -1).all() and not empty[1].any() and not empty[2].any()
    assert_render_equal(_capi(ver, tri, tex, H, W, phases=3, ws=ws), empty, "header of another nver")
    want = oracle.render_depth(ver, tri, tex, H, W)
    assert (want[3] >= 0).mean() > 0.3
    _capi(ver, tri, tex, H, W, phases=4, ws=ws)                                                  # the right header
    assert_render_equal(_capi(ver, tri, tex, H, W, phases=3, ws=ws), want, "right header")


# ---- vertex rows at a pitch: the host's 64-bit face stride ------------------------------------------------------------------------------
@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "pitch32"])
def test_face_stride_with_dense_and_padded_rows(oracle, pitched):
    rs = np.random.RandomState(41)
    B, H, W, T = 3, 40, 48, 1513
    ver, tri, tex = _posed_grid(rs, B, H, W), _grid_tris(rs)[:, :T].copy(), rs.uniform(0, 1, (B, 3, NU * NV)).astype(np.float32)
    assert pkg("_lib").lib().fr_decode_render_vertex_pitch(NU * NV) == 864 != NU * NV
    want = oracle.render_depth(ver, tri, tex, H, W)
    assert (want[3] >= 0).mean() > 0.3
    assert_render_equal(_capi(ver, tri, tex, H, W, pitched=pitched), want, "pitched" if pitched else "dense")
