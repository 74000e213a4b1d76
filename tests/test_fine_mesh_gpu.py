"""GPU: fr_mesh_visible, fr_mesh_lift and fr_mesh_vertex_normals (csrc/fr_mesh.hip) held BIT FOR BIT to their numpy models
(tests/ref_mesh.py, pinned on the CPU by tests/test_fine_mesh_cpu.py): the uint8 planes and the fp32 bits; the operators of
rendering_layer/ops.py, FaceRecNet.fine_mesh and the mesh export of examples/coarse_loop.py.  Outputs are pre-filled with a
sentinel, so an element the kernels did not write shows."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_mesh as RM
from conftest import ROOT, pkg
from raw_calls import SENT, raw_lift, raw_normals, raw_visible

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _h():
    return pkg("_lib")


def _ops():
    return pkg("rendering_layer.ops")


def _mesh_io():
    return pkg("utils.mesh_io")


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_padded(out, want, nver):
    """the live columns carry the model's bits, the pad columns still the sentinel"""
    got = out.cpu().numpy()
    assert np.array_equal(_u32(got[:, :, :nver]), _u32(want))
    assert (_u32(got[:, :, nver:]) == SENT).all()


class Scene:
    """a scene of ref_mesh rendered by the project's own render_depth; the models, computed once and never changed; one run of the
    three kernels on pitched tensors"""

    def __init__(self, S, out_pad=3):
        self.nver, self.H, self.W = S["nver"], S["H"], S["W"]
        self.V = S["vertex"]                                                   # [B,3,pitch], the pad columns NaN
        self.dense = np.ascontiguousarray(self.V[:, :, :self.nver])
        self.tri = S["tri"]
        B = self.V.shape[0]
        outs = _ops().render_depth(_t(self.dense), _t(self.tri), torch.zeros((1, 3, self.nver), device=DEV),
                                   torch.zeros((B, self.H, self.W, 3), device=DEV))
        self.tind = outs[3].reshape(B, self.H, self.W).cpu().numpy()
        self.coarse = outs[0].clamp_min(1e-6).reshape(B, self.H, self.W).cpu().numpy()
        self.fine = RM.fine_of(self.coarse)
        self.adj = _mesh_io().vertex_adjacency(self.tri, self.nver)
        ntri = self.tri.shape[1]
        # the models
        self.m_vis = RM.visible(self.tri, self.tind, self.nver)
        self.m_out, self.m_state = RM.lift(self.dense, self.tind, self.m_vis, self.fine, self.coarse, ntri)
        self.m_nrm = RM.vertex_normals(self.m_out, self.tri, *self.adj)
        # the kernels
        self.out_pitch = self.nver + out_pad
        self.g_vis = raw_visible(_t(self.tri), _t(self.tind), self.nver)
        self.g_out, self.g_state = raw_lift(_t(self.V), self.nver, _t(self.tind), self.g_vis, _t(self.fine), _t(self.coarse), ntri,
                                            self.out_pitch)
        self.g_nrm = raw_normals(self.g_out, self.nver, _t(self.tri), self.adj, self.nver + 1)
        torch.cuda.synchronize()


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        if name == "layered":
            _SCENES[name] = Scene(RM.layered_scene())                            # 9 x 7 front grid (96 triangles) + a layer behind
        else:
            _SCENES[name] = Scene(RM.layered_scene(nu=20, nv=16, H=30, W=36, B=2, pitch_pad=7))   # 336 vertices
    return _SCENES[name]


# ---- 1. the three kernels against the models ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layered", "two_blocks"])
def test_kernels_bit_for_bit(name):
    s = _scene(name)
    B = s.V.shape[0]
    if name == "layered":
        assert (B, s.tri.shape[1], s.H, s.W) == (3, 96 + 18, 12, 16) and s.V.shape[2] > s.nver and s.out_pitch > s.nver
    else:
        assert B == 2 and s.nver > 300 and s.nver % 256 != 0                    # a face's vertices cross a 256-lane block; B = 2:
    print("%s: state counts %s, visible %d of %d" % (name, np.bincount(s.m_state.reshape(-1), minlength=3).tolist(),
                                                      int(s.m_vis.sum()), s.m_vis.size))
    assert np.array_equal(s.g_vis.cpu().numpy(), s.m_vis)
    assert np.array_equal(s.g_state.cpu().numpy(), s.m_state)
    _check_padded(s.g_out, s.m_out, s.nver)
    _check_padded(s.g_nrm, s.m_nrm, s.nver)
    assert (s.m_state == 0).any() and (s.m_state == 1).any()                    # hidden vertices exist, and lifted ones
    moved = _u32(s.m_out[:, 2]) != _u32(s.dense[:, 2])
    assert moved.any() and not (moved & (s.m_state != 1)).any()
    assert np.array_equal(_u32(s.m_out[:, :2]), _u32(s.dense[:, :2]))
    assert np.isfinite(s.m_nrm).all() and (np.abs(np.linalg.norm(s.m_nrm.astype(np.float64), axis=1) - 1) < 1e-6).all()


# ---- 2. edges of the lift, hand-made ---------------------------------------------------------------------------------------------------
def test_lift_edges():
    H, W, ntri = 6, 8, 5
    nan, inf = np.nan, np.inf
    #         0    1    2    3     4     5     6    7    8     9     10   11    12   13
    xs = [3.0, 7.0, 7.5, -3.0, 9.25, 2.5, nan, 1.5, 1e30, 0.25, 5.5, 2.0, -0.5, 6.0]
    ys = [2.0, 5.0, 5.5, 2.0, 2.0, -0.5, 1.0, inf, 2.0, 4.5, 0.5, 0.0, 1.25, 3.0]
    nver = len(xs)
    V = np.stack([xs, ys, np.linspace(10, 23, nver)]).astype(np.float32)[None]
    tind = np.zeros((1, H, W), np.float32)
    tind[0, 4:6, 0:2] = -1                                                      # vertex 9's four corners: all background
    tind[0, 0, 5], tind[0, 1, 5] = nan, ntri                                    # two of vertex 10's corners are no triangle
    tind[0, 0, 6] = 4
    vis = np.ones((1, nver), np.uint8)
    vis[0, 13] = 0                                                              # hidden: state 0 whatever lies around it
    coarse = np.full((1, H, W), 15.0, np.float32)
    fine = RM.fine_of(coarse, seed=5)
    # vertex 0 at integer coordinates: only corner (2, 3) has a weight; NaN at the three zero-weight corners must not reach it
    fine[0, 2, 4] = fine[0, 3, 3] = fine[0, 3, 4] = nan
    fine[0, 0, 5] = fine[0, 1, 5] = nan                                         # not corners (tri_ind): never read
    fine[0, 4:6, 0:2] = nan
    m_out, m_state = RM.lift(V, tind, vis, fine, coarse, ntri)
    want_state = [1, 1, 1, 2, 2, 1, 2, 2, 2, 2, 1, 1, 1, 0]
    #             0: integer; 1: the last row and column, fx = fy = 0; 2: only (5, 7) is inside; 3, 4: outside; 5: row -1 is outside,
    #             row 0 counts; 6, 7: NaN x, inf y; 8: beyond the int range; 9: four background corners; 10: two of four corners;
    #             11: on the top edge; 12: column -1 is outside, column 0 counts; 13: hidden
    assert m_state[0].tolist() == want_state
    assert np.isfinite(m_out[0, 2, [0, 1, 2, 5, 10, 11, 12]]).all()
    assert m_out[0, 2, 0] == np.float32(np.float64(V[0, 2, 0]) + (np.float64(fine[0, 2, 3]) - 15.0))
    assert m_out[0, 2, 1] == np.float32(np.float64(V[0, 2, 1]) + (np.float64(fine[0, 5, 7]) - 15.0))
    g_out, g_state = raw_lift(_t(V), nver, _t(tind), _t(vis, np.uint8), _t(fine), _t(coarse), ntri, nver + 2)
    assert g_state.cpu().numpy()[0].tolist() == want_state
    _check_padded(g_out, m_out, nver)


# ---- 3. hand-made tri_ind ---------------------------------------------------------------------------------------------------------------
def test_what_marks_a_vertex_and_what_counts_as_a_corner():
    """-1, NaN, ntri and a triangle with a bad vertex id mark no vertex; -1, NaN and ntri are no corner of the lift either.  (The lift
    is not given the triangle list: a pixel whose triangle has a bad id is on the face for it, as for the render's mask.)"""
    nver, H, W = 8, 4, 5
    nan = np.nan
    tri = np.float32([[0, 3, 6, 1, 2], [1, 4, nver, -1, nan], [2, 5, 7, 2, 3]])  # triangles 2, 3, 4 have a bad id
    ntri = tri.shape[1]
    tind = np.full((2, H, W), -1, np.float32)
    tind[0, 0, :] = [nan, ntri, 2, 3, 4]
    tind[0, 2, 2] = 1
    tind[1, 3, 4] = 0
    tind[1, 1, 1] = ntri + 3
    tind[1, 0, 0] = -2.5
    m_vis = RM.visible(tri, tind, nver)
    assert m_vis.tolist() == [[0, 0, 0, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0, 0, 0]]
    g_vis = raw_visible(_t(tri), _t(tind), nver)
    assert np.array_equal(g_vis.cpu().numpy(), m_vis)
    # the lift over the same planes: every vertex visible, placed between pixels (0, 0) and (0, 1) / on the listed values
    V = np.zeros((2, 3, nver), np.float32)
    V[:, 0] = [0.5, 1.5, 2.5, 3.5, 2.0, 1.0, 0.0, 3.0]
    V[:, 1] = [0.0, 0.0, 0.0, 0.0, 2.0, 1.0, 3.0, 2.5]
    V[:, 2] = 30.0
    vis = np.ones((2, nver), np.uint8)
    coarse = np.full((2, H, W), 30.0, np.float32)
    fine = RM.fine_of(coarse, seed=9)
    m_out, m_state = RM.lift(V, tind, vis, fine, coarse, ntri)
    assert m_state[0].tolist() == [2, 1, 1, 1, 1, 2, 2, 2]                      # 0: corners NaN, ntri; 1: ntri (no) and 2 (yes)
    assert m_state[1].tolist() == [2] * 8
    g_out, g_state = raw_lift(_t(V), nver, _t(tind), _t(vis, np.uint8), _t(fine), _t(coarse), ntri, nver)
    assert np.array_equal(g_state.cpu().numpy(), m_state)
    _check_padded(g_out, m_out, nver)


def test_an_empty_triangle_table():
    nver, H, W = 5, 3, 4
    tri = np.zeros((3, 0), np.float32)
    tind = np.zeros((2, H, W), np.float32)
    g_vis = raw_visible(_t(tri), _t(tind), nver)
    assert not g_vis.cpu().numpy().any()
    V = np.random.RandomState(0).uniform(0, 3, (2, 3, nver)).astype(np.float32)
    vis = np.uint8([[1, 0, 1, 1, 0], [0, 0, 0, 0, 1]])
    plane = np.ones((2, H, W), np.float32)
    g_out, g_state = raw_lift(_t(V), nver, _t(tind), _t(vis, np.uint8), _t(plane * 2), _t(plane), 0, nver)
    assert np.array_equal(g_state.cpu().numpy(), vis * 2)                       # visible without a corner: 2
    _check_padded(g_out, V, nver)
    g_n = raw_normals(_t(V), nver, _t(tri), (np.zeros(nver + 1, np.int32), np.zeros(0, np.int32)), nver)
    assert not g_n.cpu().numpy().view(np.uint32).any()


# ---- 4. normals: nothing to sum, or a sum that vanishes ---------------------------------------------------------------------------------
def test_normals_that_are_exactly_zero():
    V = np.float32([[0, 1, 2, 5, 7, 3], [0, 1, 2, 5, 7, 3], [0, 1, 2, 5, 7, 4]])[None]   # 0, 1, 2 on a line; 3, 4 unnamed
    tri = np.float32([[0, 1, 0], [1, 2, 1], [2, 0, 5]])                         # a zero-area fan, and one real triangle (0, 1, 5)
    s, t = _mesh_io().vertex_adjacency(tri, 6)
    want = RM.vertex_normals(V, tri, s, t)
    assert not want[0, :, [2, 3, 4]].view(np.uint32).any()                      # 2: only the fan; 3, 4: no triangle
    assert np.abs(want[0, :, [0, 1, 5]]).sum() > 0
    got = raw_normals(_t(V), 6, _t(tri), (s, t), 6)
    assert np.array_equal(_u32(got.cpu().numpy()), _u32(want))


# ---- 5. the same bits wherever the launch puts a face -----------------------------------------------------------------------------------
def test_a_face_alone_and_at_index_two_of_three():
    s = _scene("layered")
    ntri = s.tri.shape[1]
    one = lambda a: np.ascontiguousarray(a[2:3])                                 # noqa: E731
    vis = raw_visible(_t(s.tri), _t(one(s.tind)), s.nver)
    out, state = raw_lift(_t(one(s.V)), s.nver, _t(one(s.tind)), vis, _t(one(s.fine)), _t(one(s.coarse)), ntri, s.out_pitch)
    nrm = raw_normals(out, s.nver, _t(s.tri), s.adj, s.nver + 1)
    assert torch.equal(vis[0], s.g_vis[2]) and torch.equal(state[0], s.g_state[2])
    assert torch.equal(out[0].view(torch.int32), s.g_out[2].view(torch.int32))
    assert torch.equal(nrm[0].view(torch.int32), s.g_nrm[2].view(torch.int32))


def test_two_streams():
    s = _scene("layered")
    ntri = s.tri.shape[1]
    ins = [_t(s.tri), _t(s.tind), _t(s.V), _t(s.fine), _t(s.coarse)]
    torch.cuda.synchronize()
    got = []
    for st in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(st):
            vis = raw_visible(ins[0], ins[1], s.nver)
            out, state = raw_lift(ins[2], s.nver, ins[1], vis, ins[3], ins[4], ntri, s.out_pitch)
            got.append((vis, state, out, raw_normals(out, s.nver, ins[0], s.adj, s.nver + 1)))
    torch.cuda.synchronize()
    for vis, state, out, nrm in got:
        assert torch.equal(vis, s.g_vis) and torch.equal(state, s.g_state)
        assert torch.equal(out.view(torch.int32), s.g_out.view(torch.int32))
        assert torch.equal(nrm.view(torch.int32), s.g_nrm.view(torch.int32))


# ---- 6. the operators and FaceRecNet.fine_mesh ------------------------------------------------------------------------------------------
IM = 40


@pytest.fixture(scope="module")
def small_face(small_assets):
    """the small fixture mesh decoded as __graft_entry__.smoke() decodes it, and its coarse depth map"""
    A = small_assets
    netm = pkg("nets.network")
    rs = np.random.RandomState(0)
    B = 2
    P = np.zeros((B, 7 + A["ndim_shape"] + A["ndim_exp"]), np.float32)
    P[:, 0:3] = rs.uniform(-0.5, 0.5, (B, 3))
    P[:, 3:5] = rs.uniform(17, 23, (B, 2))
    P[:, 6] = rs.uniform(1.6e-4, 2.2e-4, B)
    P[:, 7:7 + A["ndim_shape"]] = rs.uniform(0, 1e4, (B, A["ndim_shape"]))
    P[:, 7 + A["ndim_shape"]:] = rs.uniform(-1.5, 1.5, (B, A["ndim_exp"]))
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=IM, device=torch.device(DEV))
    V = net.vertices_transform(torch.as_tensor(P, device=DEV))
    coarse = net.rendering_layer(V, net.tri, net.vertex_code)[3]
    return net, V, coarse


def test_fine_mesh_with_equal_maps_returns_the_vertices(small_face):
    net, V, coarse = small_face
    m = net.fine_mesh(V, coarse, coarse)
    assert set(m) == {"vertices", "state", "normals"}
    assert torch.equal(m["vertices"].view(torch.int32), V.contiguous().view(torch.int32))
    assert m["state"].dtype == torch.uint8 and tuple(m["state"].shape) == (2, net.nvert)
    assert not m["vertices"].requires_grad and not m["normals"].requires_grad
    st = m["state"].cpu().numpy()
    assert (st == 1).sum() > 50 and (st == 0).any()
    assert net.adjacency() is net.adjacency()                                  # built once
    assert net.fine_mesh(V, coarse, coarse, with_normals=False)["normals"] is None
    # the operators against the models, through the public surface
    ops = _ops()
    tri = net.tri.cpu().numpy()
    tind = ops.render_depth(V, net.tri, net.vertex_code, torch.zeros((2, IM, IM, 3), device=DEV))[3]
    vis = ops.mesh_visible(net.tri, tind, net.nvert)
    m_vis = RM.visible(tri, tind.cpu().numpy()[..., 0], net.nvert)
    assert np.array_equal(vis.cpu().numpy(), m_vis)
    fine = _t(RM.fine_of(coarse.cpu().numpy(), scale=0.05))
    out, state = ops.mesh_lift(V, tind, vis, fine, coarse, ntri=tri.shape[1])
    m_out, m_state = RM.lift(V.cpu().numpy(), tind.cpu().numpy()[..., 0], m_vis, fine.cpu().numpy()[..., 0],
                             coarse.cpu().numpy()[..., 0], tri.shape[1])
    assert np.array_equal(state.cpu().numpy(), m_state) and np.array_equal(_u32(out.cpu().numpy()), _u32(m_out))
    assert np.array_equal(st, RM.lift(V.cpu().numpy(), tind.cpu().numpy()[..., 0], m_vis, coarse.cpu().numpy()[..., 0],
                                      coarse.cpu().numpy()[..., 0], tri.shape[1])[1])
    nrm = ops.vertex_normals(out, net.tri, _mesh_io().vertex_adjacency(tri, net.nvert))
    assert np.array_equal(_u32(nrm.cpu().numpy()), _u32(RM.vertex_normals(m_out, tri, *_mesh_io().vertex_adjacency(tri, net.nvert))))
    assert torch.equal(nrm.view(torch.int32), ops.vertex_normals(out, net.tri, net.adjacency()).view(torch.int32))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_bump_moves_only_the_lifted_vertices_near_it(small_face, sign):
    net, V, coarse = small_face
    tind = _ops().render_depth(V, net.tri, net.vertex_code, torch.zeros((2, IM, IM, 3), device=DEV))[3].cpu().numpy()[..., 0]
    rows, cols = np.nonzero(tind[0] >= 0)
    r_c, c_c, rad = float(rows.mean()), float(cols.mean()), 3.0                # a disc inside face 0
    rr, cc = np.meshgrid(np.arange(IM), np.arange(IM), indexing="ij")
    disc = (rr - r_c) ** 2 + (cc - c_c) ** 2 <= rad * rad
    assert (tind[0][disc] >= 0).all()
    bump = np.zeros((2, IM, IM, 1), np.float32)
    bump[0, disc, 0] = sign * 0.25
    m = net.fine_mesh(V, coarse + _t(bump), coarse)
    Vn, out, st = V.cpu().numpy(), m["vertices"].cpu().numpy(), m["state"].cpu().numpy()
    assert np.array_equal(_u32(out[:, :2]), _u32(Vn[:, :2])) and np.array_equal(_u32(out[1]), _u32(Vn[1]))
    dz = out[0, 2].astype(np.float64) - Vn[0, 2]
    moved = dz != 0
    # a vertex reads the four pixels around it: one of them lies in the disc only if the vertex is within rad + sqrt(2) of its centre
    near = (Vn[0, 1] - r_c) ** 2 + (Vn[0, 0] - c_c) ** 2 < (rad + 1.5) ** 2
    print("bump %+.2f: %d vertices moved, %d lifted and near" % (sign * 0.25, moved.sum(), (near & (st[0] == 1)).sum()))
    assert moved.sum() >= 3 and not (moved & ~((st[0] == 1) & near)).any()
    assert (np.sign(dz[moved]) == sign).all() and np.abs(dz).max() <= 0.25 * (1 + 1e-6)
    inside = ((Vn[0, 1] - r_c) ** 2 + (Vn[0, 0] - c_c) ** 2 < (rad - 1.5) ** 2) & (st[0] == 1)
    assert np.allclose(dz[inside], sign * 0.25, rtol=1e-5)                     # every corner in the disc: the whole bump


def test_operator_shape_checks():
    ops = _ops()
    tri, tind = _t(RM.grid_mesh(3, 3)), torch.zeros((2, 4, 5, 1), device=DEV)
    V = torch.zeros((2, 3, 9), device=DEV)
    vis = ops.mesh_visible(tri, tind, 9)
    for bad in (lambda: ops.mesh_visible(tri.t(), tind, 9), lambda: ops.mesh_visible(tri, tind[..., 0, 0], 9),
                lambda: ops.mesh_lift(V[:, :2], tind, vis, tind, tind), lambda: ops.mesh_lift(V, tind[:1], vis, tind, tind),
                lambda: ops.mesh_lift(V, tind, vis[:, :8], tind, tind), lambda: ops.mesh_lift(V, tind, vis.float(), tind, tind),
                lambda: ops.mesh_lift(V, tind, vis, tind[:, :3], tind), lambda: ops.mesh_lift(V, tind, vis, tind, tind[:, :, :4]),
                lambda: ops.vertex_normals(V, tri, (np.zeros(10, np.int32), np.zeros(23, np.int32))),
                lambda: ops.vertex_normals(V[:, :, :8], tri, ops.MeshAdjacency(*_mesh_io().vertex_adjacency(tri.cpu().numpy(), 9), 9, 8, DEV))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.mesh_visible(tri.cpu(), tind.cpu(), 9)


# ---- 7. the program -----------------------------------------------------------------------------------------------------------------------
def _read_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        p = line.split()
        if not p or p[0] == "#":
            continue
        assert p[0] in ("v", "vn", "f"), line
        if p[0] == "f":
            f.append([int(q.split("/")[0]) for q in p[1:]])
        else:
            (v if p[0] == "v" else vn).append([float(q) for q in p[1:]])
    return np.array(v), np.array(vn), np.array(f)


def test_export_mesh_program(small_assets, tmp_path):
    out = str(tmp_path / "meshes")
    B, S = 8, 120
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/coarse_loop.py", "--phase", "test", "--small", "--batch", str(B), "--im-size", str(S),
                        "--steps", "4", "--warmup", "1", "--synth-data", "--export-mesh", out, "--export-count", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    print({k: d[k] for k in ("vertex_rmse_coarse", "vertex_rmse_fine", "vertex_rmse_vertices", "depth_rmse")})
    assert np.isfinite(d["vertex_rmse_coarse"]) and np.isfinite(d["vertex_rmse_fine"]) and np.isfinite(d["depth_rmse"])
    assert d["export_count"] == 2 and d["depth_identical_to_one_batch_at_a_time"] is True
    assert sorted(os.listdir(out)) == ["face_%06d_%s.obj" % (i, k) for i in (0, 1) for k in ("coarse", "fine")]
    nver, T = small_assets["vertex"].shape[1], small_assets["tri"].shape[1]
    for i in (0, 1):
        vc, nc, fc = _read_obj(os.path.join(out, "face_%06d_coarse.obj" % i))
        vf, nf, ff = _read_obj(os.path.join(out, "face_%06d_fine.obj" % i))
        assert vc.shape == vf.shape == nc.shape == nf.shape == (nver, 3) and fc.shape == (T, 3) and np.array_equal(fc, ff)
        assert fc.min() >= 1 and fc.max() <= nver and np.isfinite(vc).all() and np.isfinite(vf).all()
        assert np.array_equal(vc[:, :2], vf[:, :2])                             # x and y do not move
        assert np.array_equal(fc - 1, small_assets["tri"].T.astype(int)[:, ::-1])   # flip_y: the winding reversed
