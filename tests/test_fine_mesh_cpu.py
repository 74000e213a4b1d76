"""CPU: the fine-mesh entry points (fr_mesh_visible, fr_mesh_lift, fr_mesh_vertex_normals) exist and validate before any HIP call in
the order include/fr_hotpath.h states; utils/mesh_io.vertex_adjacency against a brute-force loop; the numpy models of the GPU tests
(tests/ref_mesh.py) against the properties they must have; the OBJ and PLY writers read back."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import ref_mesh as RM

NEW = ("fr_mesh_visible", "fr_mesh_lift", "fr_mesh_vertex_normals")


def _L():
    return pkg("_lib").lib()


def _mesh_io():
    return pkg("utils.mesh_io")


def test_symbols_exported_and_bound():
    L, lib = _L(), pkg("_lib")
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTS and name in lib.SIGNATURES
    assert lib.SIGNATURES["fr_mesh_visible"] == "i:ppiiiiipp"
    assert lib.SIGNATURES["fr_mesh_lift"] == "i:pippppiiiiipipp"
    assert lib.SIGNATURES["fr_mesh_vertex_normals"] == "i:pipppiiipip"
    assert "fr_mesh.hip" in lib.SOURCES
    assert b"fr_hotpath 0.4 " in L.fr_version()                                 # the ABI version is unchanged


def _gpu_visible():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_visible(), reason="the made-up pointers of this test must never reach a launch: CPU machines only")
def test_validates_before_any_hip_call():
    """The header's order: (1) sizes / pitches, (2) the empty batch or mesh, (3) pointers, (4) what the kernels do not serve.  No call
    here is legal throughout: each stops at a check."""
    L = _L()
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(4)
    B, nver, ntri, H, W = 2, 10, 5, 8, 9

    def vis(tri=one, ti=one, B=B, nver=nver, ntri=ntri, H=H, W=W, out=one):
        return L.fr_mesh_visible(tri, ti, B, nver, ntri, H, W, out, nul)

    def lift(v=one, vp=nver, ti=one, vs=one, f=one, c=one, B=B, nver=nver, ntri=ntri, H=H, W=W, out=one, op=nver, st=one):
        return L.fr_mesh_lift(v, vp, ti, vs, f, c, B, nver, ntri, H, W, out, op, st, nul)

    def nrm(v=one, vp=nver, tri=one, a0=one, a1=one, B=B, nver=nver, ntri=ntri, out=one, op=nver):
        return L.fr_mesh_vertex_normals(v, vp, tri, a0, a1, B, nver, ntri, out, op, nul)
    # (1)
    for k in ("B", "nver", "ntri", "H", "W"):
        assert vis(**{k: -1}) == -1 and lift(**{k: -1}) == -1, k
    for k in ("B", "nver", "ntri"):
        assert nrm(**{k: -1}) == -1, k
    assert lift(vp=nver - 1) == -1 and lift(op=nver - 1) == -1 and nrm(vp=nver - 1) == -1 and nrm(op=nver - 1) == -1
    # (1) comes before (2): a scalar error is reported for an empty batch too
    assert vis(B=0, H=-1) == -1 and lift(B=0, vp=nver - 1) == -1 and nrm(B=0, op=nver - 1) == -1
    # (2) comes before (3) and (4): nothing is looked at
    assert vis(tri=nul, ti=nul, out=nul, B=0) == 0 and vis(tri=nul, ti=nul, out=nul, nver=0) == 0
    assert lift(v=nul, ti=nul, vs=nul, f=nul, c=nul, out=nul, st=nul, B=0, ntri=1 << 24) == 0
    assert lift(v=nul, ti=nul, vs=nul, f=nul, c=nul, out=nul, st=nul, nver=0, vp=0, op=0) == 0
    assert nrm(v=nul, tri=nul, a0=nul, a1=nul, out=nul, B=0, ntri=1 << 24) == 0
    assert nrm(v=nul, tri=nul, a0=nul, a1=nul, out=nul, nver=0, vp=0, op=0) == 0
    # (3)
    for k in ("tri", "ti", "out"):
        assert vis(**{k: nul}) == -1, k
    for k in ("v", "ti", "vs", "f", "c", "out", "st"):
        assert lift(**{k: nul}) == -1, k
    for k in ("v", "tri", "a0", "a1", "out"):
        assert nrm(**{k: nul}) == -1, k
    # (3) comes before (4)
    assert vis(out=nul, ntri=1 << 24) == -1 and lift(st=nul, ntri=1 << 24) == -1 and nrm(out=nul, ntri=1 << 24) == -1
    # (4)
    assert vis(ntri=1 << 24) == -4 and lift(ntri=1 << 24) == -4 and nrm(ntri=1 << 24) == -4   # float-stored ids stop being exact
    assert vis(H=1 << 16, W=1 << 15) == -4 and lift(H=1 << 16, W=1 << 15) == -4               # 2^31 pixels per face
    assert vis(B=1 << 11, H=1 << 15, W=1 << 13) == -4                                          # 2^31 workgroups of 256 pixels
    assert lift(B=1 << 16, nver=1 << 23, vp=1 << 23, op=1 << 23) == -4                          # 2^31 workgroups of 256 vertices
    assert nrm(B=1 << 16, nver=1 << 23, vp=1 << 23, op=1 << 23) == -4


# ---- vertex_adjacency ---------------------------------------------------------------------------------------------------------------
def _brute_adjacency(tri, nver):
    rows = [[] for _ in range(nver)]
    for t in range(tri.shape[1]):
        for v in sorted(set(int(x) for x in tri[:, t])):
            if 0 <= v < nver:
                rows[v].append(t)
    return rows


def test_vertex_adjacency_against_a_brute_force_loop():
    rs = np.random.RandomState(2)
    nver, T = 40, 70
    tri = rs.randint(0, nver - 1, (3, T))                                       # vertex 39: no triangle names it
    tri[1, 5] = tri[0, 5]                                                        # triangle 5 names a vertex twice
    tri[:, 9] = 7                                                                # triangle 9 names one three times
    assert not (tri == nver - 1).any()
    want = _brute_adjacency(tri, nver)
    for t_in in (tri.astype(np.float32), tri.astype(np.int32)):
        adj_start, adj_tri = _mesh_io().vertex_adjacency(t_in, nver)
        assert adj_start.dtype == np.int32 and adj_tri.dtype == np.int32
        assert adj_start.shape == (nver + 1,) and adj_tri.shape == (3 * T,)
        assert adj_start[0] == 0 and adj_start[-1] == sum(len(r) for r in want) < 3 * T
        for v in range(nver):
            got = adj_tri[adj_start[v]:adj_start[v + 1]].tolist()
            assert got == want[v] == sorted(set(want[v])), v
        assert adj_start[nver - 1] == adj_start[nver]                            # the unnamed vertex: an empty row
        assert want[int(tri[0, 5])].count(5) == 1 and want[7].count(9) == 1


def test_vertex_adjacency_edges():
    io = _mesh_io()
    s, t = io.vertex_adjacency(np.zeros((3, 0), np.float32), 4)
    assert s.tolist() == [0] * 5 and t.shape == (0,)
    s, t = io.vertex_adjacency(np.float32([[0, 1], [1, np.nan], [9, 2]]), 3)     # ids outside the mesh are listed nowhere
    assert s.tolist() == [0, 1, 3, 4] and t[:4].tolist() == [0, 0, 1, 1]
    with pytest.raises(ValueError):
        io.vertex_adjacency(np.zeros((2, 4)), 3)


def test_adjacency_table_is_checked_on_the_host():
    ops = pkg("rendering_layer.ops")
    tri = RM.grid_mesh(3, 3)
    s, t = _mesh_io().vertex_adjacency(tri, 9)
    A = ops.MeshAdjacency(s, t, 9, 8, "cpu")
    assert A.adj_start.dtype.is_floating_point is False and A.adj_tri.numel() == 24
    bad = s.copy()
    bad[3] = bad[4] + 1
    for a0, a1, nv, nt in ((bad, t, 9, 8), (s[:-1], t, 9, 8), (s, t[:-1], 9, 8), (s + 1, t, 9, 8), (s, t + 8, 9, 8), (s, t - 1, 9, 8),
                           (s.astype(np.float32), t, 9, 8), (s, t, 9, 7)):
        with pytest.raises(ValueError):
            ops.MeshAdjacency(a0, a1, nv, nt, "cpu")


# ---- the numpy models ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle):
    """RM.layered_scene rendered by the reference model's own forward: tind, coarse [B,H,W]; the model's visible plane"""
    S = RM.layered_scene()
    nver = S["nver"]
    V = np.ascontiguousarray(S["vertex"][:, :, :nver])
    outs = oracle.render_depth(V, S["tri"], np.zeros((1, 3, nver), np.float32), S["H"], S["W"])
    S["dense"] = V
    S["tind"] = outs[3].reshape(-1, S["H"], S["W"])
    S["coarse"] = np.maximum(outs[0].reshape(-1, S["H"], S["W"]), np.float32(1e-6))
    S["visible"] = RM.visible(S["tri"], S["tind"], nver)
    return S


def _expected_state(V, tind, vis):
    """state by its definition, vectorised and without the model's loop: 0 hidden; 1 where one of the four pixels around the vertex
    is on the face with a weight that is not 0; else 2"""
    B, _, nver = V.shape
    H, W = tind.shape[1:]
    x, y = V[:, 0].astype(np.float64), V[:, 1].astype(np.float64)
    c0, r0 = np.floor(x), np.floor(y)
    fx, fy = x - c0, y - r0
    found = np.zeros((B, nver), bool)
    for dr, dc, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        r, c = r0 + dr, c0 + dc
        inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        ri, ci = np.where(inside, r, 0).astype(int), np.where(inside, c, 0).astype(int)
        found |= inside & (w != 0) & (tind[np.arange(B)[:, None], ri, ci] >= 0)
    return np.where(vis == 0, 0, np.where(found, 1, 2)).astype(np.uint8)


def test_the_scene_has_hidden_and_lifted_vertices(scene):
    vis = scene["visible"]
    assert (scene["tind"] >= 0).mean() > 0.3
    assert vis[:, :63].any() and not vis[:, 63:].all() and not vis.all()       # the layer behind is hidden somewhere
    # a vertex is visible exactly when a pixel's winner names it: brute force over the pixels
    ids = RM.f2i(scene["tri"])
    for b in range(vis.shape[0]):
        named = np.zeros(scene["nver"], np.uint8)
        for t in scene["tind"][b].reshape(-1):
            if t >= 0:
                named[ids[:, int(t)]] = 1
        assert np.array_equal(named, vis[b]), b


def test_equal_maps_leave_the_vertices_alone(scene):
    out, state = RM.lift(scene["dense"], scene["tind"], scene["visible"], scene["coarse"], scene["coarse"], scene["tri"].shape[1])
    assert np.array_equal(out.view(np.uint32), scene["dense"].view(np.uint32))
    want = _expected_state(scene["dense"], scene["tind"], scene["visible"])
    assert np.array_equal(state, want)
    assert set(np.unique(state).tolist()) <= {0, 1, 2} and (state == 0).any() and (state == 1).any()


def test_a_constant_offset_moves_the_lifted_vertices_by_it(scene):
    """fine = coarse + 0.5: the differences are 0.5 up to the rounding of coarse + 0.5 (coarse ~ 50, so |d - 0.5| <= 2^-19); the
    quotient of the two chains carries a few 2^-53 of relative error ahead of one fp32 rounding.  With an offset that IS exact per
    pixel the result is fl32(z + 0.5) or a neighbour of it."""
    coarse = np.round(scene["coarse"] * 4) / 4                                  # multiples of 1/4: coarse + 0.5 is exact in fp32
    fine = (coarse + np.float32(0.5)).astype(np.float32)
    assert np.array_equal(fine.astype(np.float64) - coarse.astype(np.float64), np.full(coarse.shape, 0.5))
    out, state = RM.lift(scene["dense"], scene["tind"], scene["visible"], fine, coarse, scene["tri"].shape[1])
    V = scene["dense"]
    assert np.array_equal(out[:, :2].view(np.uint32), V[:, :2].view(np.uint32))
    on = state == 1
    assert on.sum() > 50
    z, got = V[:, 2][on], out[:, 2][on]
    want = (z.astype(np.float64) + 0.5).astype(np.float32)
    near = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    assert near.all()
    assert np.array_equal(out[:, 2][~on].view(np.uint32), V[:, 2][~on].view(np.uint32))


def test_a_nan_in_the_fine_map_stays_in_its_stencil(scene):
    fine = RM.fine_of(scene["coarse"])
    ntri = scene["tri"].shape[1]
    clean, st0 = RM.lift(scene["dense"], scene["tind"], scene["visible"], fine, scene["coarse"], ntri)
    b, r, c = 0, 5, 7
    assert scene["tind"][b, r, c] >= 0
    fine2 = fine.copy()
    fine2[b, r, c] = np.nan
    out, st1 = RM.lift(scene["dense"], scene["tind"], scene["visible"], fine2, scene["coarse"], ntri)
    assert np.array_equal(st0, st1)
    x, y = scene["dense"][:, 0], scene["dense"][:, 1]
    reads = (np.arange(3)[:, None] == b) & (np.floor(x) >= c - 1) & (np.floor(x) <= c) & (np.floor(y) >= r - 1) & (np.floor(y) <= r)
    hit = np.isnan(out[:, 2])
    assert hit.any() and not (hit & ~reads).any()
    assert np.array_equal(out[:, 2][~hit].view(np.uint32), clean[:, 2][~hit].view(np.uint32))


def test_normals_of_a_tilted_plane():
    """x and y on a grid of 1/64, the plane's coefficients dyadic: every vertex lies on the plane exactly in fp32, so every facet's
    normal is the plane's up to float64 rounding and so is every vertex's, border included"""
    nu, nv = 7, 6
    tri = RM.grid_mesh(nu, nv)
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    rs = np.random.RandomState(1)
    x = np.round((1.5 * iv + rs.uniform(-0.3, 0.3, iv.shape)).reshape(-1) * 64) / 64
    y = np.round((1.25 * iu + rs.uniform(-0.3, 0.3, iv.shape)).reshape(-1) * 64) / 64
    a, b, c = 0.5, -0.75, 9.0
    V64 = np.stack([x, y, a * x + b * y + c])[None]
    V = V64.astype(np.float32)
    assert np.array_equal(V.astype(np.float64), V64)
    s, t = _mesh_io().vertex_adjacency(tri, nu * nv)
    n = RM.vertex_normals(V, tri, s, t)[0].astype(np.float64)
    want = np.array([-a, -b, 1.0]) / np.sqrt(a * a + b * b + 1)                 # the winding of grid_mesh gives n_z > 0
    inner = ((iu > 0) & (iu < nu - 1) & (iv > 0) & (iv < nv - 1)).reshape(-1)
    assert inner.sum() == (nu - 2) * (nv - 2)
    assert np.abs(n[:, inner] - want[:, None]).max() <= 1e-6
    assert np.abs(np.linalg.norm(n, axis=0) - 1).max() <= 1e-6


def test_normals_without_a_triangle_or_without_area():
    V = np.float32([[[0, 1, 2, 5, 7]], [[0, 1, 2, 5, 7]], [[0, 1, 2, 5, 7]]]).reshape(1, 3, 5)   # vertices 0, 1, 2 on a line
    tri = np.float32([[0, 1], [1, 2], [2, 0]])                                  # a zero-area fan; vertices 3 and 4 unnamed
    s, t = _mesh_io().vertex_adjacency(tri, 5)
    n = RM.vertex_normals(V, tri, s, t)
    assert not n.view(np.uint32).any()                                           # exactly +0 everywhere


# ---- writers ------------------------------------------------------------------------------------------------------------------------
def _read_obj(path):
    v, vn, f, fn = [], [], [], []
    for line in open(path):
        p = line.split()
        if not p or p[0] == "#":
            continue
        if p[0] == "v":
            v.append([float(q) for q in p[1:]])
        elif p[0] == "vn":
            vn.append([float(q) for q in p[1:]])
        elif p[0] == "f":
            f.append([int(q.split("/")[0]) for q in p[1:]])
            fn.append([int(q.split("/")[-1]) for q in p[1:]])
        else:
            raise AssertionError("unexpected OBJ line: " + line)
    return np.array(v), np.array(vn), np.array(f), np.array(fn)


def _read_ply(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    end = lines.index("end_header")
    nv = int([q for q in lines[:end] if q.startswith("element vertex")][0].split()[2])
    nf = int([q for q in lines[:end] if q.startswith("element face")][0].split()[2])
    props = [q.split()[2] for q in lines[:end] if q.startswith("property") and "list" not in q]
    body = lines[end + 1:]
    v = np.array([[float(q) for q in body[i].split()] for i in range(nv)])
    f = np.array([[int(q) for q in body[nv + i].split()] for i in range(nf)])
    assert v.shape == (nv, len(props)) and (f[:, 0] == 3).all() and not "".join(body[nv + nf:]).strip()
    return props, v, f[:, 1:]


def _small_face():
    tri = RM.grid_mesh(3, 4)
    rs = np.random.RandomState(8)
    V = rs.uniform(0, 30, (3, 12)).astype(np.float32)
    N = rs.standard_normal((3, 12)).astype(np.float32)
    C = rs.uniform(0, 1, (3, 12)).astype(np.float32)
    return V, tri, N, C


def test_obj_reads_back(tmp_path):
    io = _mesh_io()
    V, tri, N, C = _small_face()
    p = str(tmp_path / "a.obj")
    io.write_obj(p, V, tri)
    v, vn, f, _ = _read_obj(p)
    assert np.array_equal(v.astype(np.float32), V.T) and vn.size == 0          # %.9g round-trips an fp32 value
    assert np.array_equal(f - 1, tri.T.astype(int))                             # 1-based in the file
    io.write_obj(p, V, tri.astype(np.int64), normals=N, colors=C)
    v, vn, f, fn = _read_obj(p)
    assert v.shape == (12, 6) and np.array_equal(v[:, :3].astype(np.float32), V.T) and np.allclose(v[:, 3:], C.T, atol=1e-5)
    assert np.array_equal(vn.astype(np.float32), N.T) and np.array_equal(f, fn) and np.array_equal(f - 1, tri.T.astype(int))


def test_ply_reads_back(tmp_path):
    io = _mesh_io()
    V, tri, N, C = _small_face()
    p = str(tmp_path / "a.ply")
    io.write_ply(p, V, tri)
    props, v, f = _read_ply(p)
    assert props == ["x", "y", "z"] and np.array_equal(v.astype(np.float32), V.T)
    assert np.array_equal(f, tri.T.astype(int))                                 # 0-based in the file
    io.write_ply(p, V, tri, normals=N, colors=C)
    props, v, f = _read_ply(p)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(v[:, 3:6].astype(np.float32), N.T) and np.array_equal(v[:, 6:], np.round(C.T * 255))


def test_flip_y_flips_y_and_the_winding(tmp_path):
    io = _mesh_io()
    V, tri, N, _ = _small_face()
    for write, read, base in ((io.write_obj, lambda q: _read_obj(q)[:3], 1), (io.write_ply, lambda q: _read_ply(q)[1:], 0)):
        p = str(tmp_path / "f")
        write(p, V, tri, normals=N, flip_y=40)
        got = read(p)
        v, f = got[0], got[-1]
        assert np.array_equal(v[:, 0].astype(np.float32), V[0]) and np.array_equal(v[:, 2].astype(np.float32), V[2])
        assert np.allclose(v[:, 1], (40.0 - V[1].astype(np.float64)) - 1.0, rtol=1e-8)
        assert np.array_equal(f - base, tri.T.astype(int)[:, ::-1])
        nrm = got[1] if base == 1 else v[:, 3:6]
        assert np.array_equal(nrm[:, 1].astype(np.float32), -N[1]) and np.array_equal(nrm[:, 0].astype(np.float32), N[0])
    # upright and still pointing out: a facet's normal from the FILE's vertices and winding is the mirror image of the original's
    io.write_obj(str(tmp_path / "g.obj"), V, tri, flip_y=40)
    v, _, f, _ = _read_obj(str(tmp_path / "g.obj"))
    P = v[f - 1]
    n_file = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    Q = V.T.astype(np.float64)[tri.T.astype(int)]
    n_orig = np.cross(Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0])
    assert np.allclose(n_file, n_orig * np.array([1.0, -1.0, 1.0]), atol=1e-9)
    with pytest.raises(ValueError):
        io.write_obj(str(tmp_path / "h.obj"), V, np.float32([[0], [1], [12]]))
