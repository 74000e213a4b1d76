"""GPU: the render backward (render_backward_kernel<PACKED>, bwd_records_kernel in csrc/fr_render_bwd.hip; fr_render_depth_backward and
fr_render_depth_backward_ws) held to its integer model (tests/ref_render_bwd_model.py, pinned on the CPU by
tests/test_render_bwd_model_cpu.py) BIT FOR BIT, at every launch geometry the launcher chooses from and at the values
where a fixed-point scatter goes wrong.

Every case calls both entry points through the C ABI, and the workspace one twice more: with a workspace one byte too
small and with one misaligned by 8 bytes (both run as the plain variant).  Per face:
  * fixed-point face: vertex_grad bit-equal to the model (x and y rows +0; the output is pre-filled with NaN, so all of it
    was written); all four calls bit-equal;
  * bad face (Inf / NaN among the counted gradients): fp32 atomics in an unknown order, so no bits -- the class of every
    vertex equals the model's and a finite vertex is within n_v * ulp_fp32(sum |terms|) of the float64 sum (each of the
    n_v additions rounds a partial sum that is at most sum |terms|: the standard bound of a sequential sum);
  * the launch geometry the case was written for, read from fr_debug_render_bwd_geom (the launcher's own function), never
    recomputed here."""
import ctypes

import numpy as np
import pytest
import torch

import ref_render_bwd_model as R
from conftest import pkg
from gpu_util import ops

pytestmark = pytest.mark.gpu
FMAX = float(np.finfo(np.float32).max)
GEOM_KEYS = ("splits", "range", "shift", "chunks", "lds", "xcd")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda:0")


def geom(B, nver, H, W):
    out = (ctypes.c_int * 6)()
    pkg("_lib").lib().fr_debug_render_bwd_geom(B, nver, H, W, out)
    return dict(zip(GEOM_KEYS, out))


def launch_all(g, tri, ti, nver, H, W):
    """the four calls -> [plain, ws, ws one byte short, ws misaligned by 8], device tensors [B,3,nver] pre-filled with NaN"""
    h = pkg("_lib")
    L = h.lib()
    B, ntri = g.shape[0], tri.shape[1]
    gt, trit, tit = _t(g), _t(tri), _t(ti)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nws = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    assert nws >= 16 * B * H * W
    ws = torch.empty((nws + 16,), dtype=torch.uint8, device="cuda:0")
    assert ws.data_ptr() % 16 == 0
    outs = [torch.full((B, 3, nver), float("nan"), device="cuda:0") for _ in range(4)]
    assert L.fr_render_depth_backward(h.ptr(gt), h.ptr(trit), h.ptr(tit), h.ptr(outs[0]), B, nver, ntri, H, W, st) == 0
    for out, p, nbytes in ((outs[1], ws.data_ptr(), nws), (outs[2], ws.data_ptr(), nws - 1), (outs[3], ws.data_ptr() + 8, nws)):
        assert L.fr_render_depth_backward_ws(h.ptr(gt), h.ptr(trit), h.ptr(tit), h.ptr(out), B, nver, ntri, H, W,
                                             ctypes.c_void_p(p), ctypes.c_size_t(nbytes), st) == 0
    torch.cuda.synchronize()
    return outs


def check(g, tri, ti, nver, H, W, want_geom, n_bad=0):
    """runs the case through the four calls and holds every face to the model; returns the model"""
    g = np.ascontiguousarray(g, np.float32).reshape(-1, H, W, 1)
    ti = np.ascontiguousarray(ti, np.float32).reshape(-1, H, W, 1)
    B = g.shape[0]
    got_geom = geom(B, nver, H, W)
    assert {k: got_geom[k] for k in want_geom} == want_geom, got_geom
    M = R.model(g, tri, ti, nver, H, W)
    assert int(M.bad.sum()) == n_bad, M.bad
    outs = launch_all(g, tri, ti, nver, H, W)
    fixed = np.flatnonzero(~M.bad)
    got = outs[0].cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[fixed], M.bits[fixed])
    if n_bad == 0:
        for o in outs[1:]:
            assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))
        return M
    for o in outs:
        bits = o.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(bits[fixed], M.bits[fixed])
        z = bits.view(np.float32)
        for b in np.flatnonzero(M.bad):
            assert not bits[b, :2].any()
            R.assert_bad_face(z[b, 2], M, b)
    return M


GRADS = {
    "unit": lambda rs, sh: rs.standard_normal(sh),
    "decades12": lambda rs, sh: rs.standard_normal(sh) * np.exp(rs.uniform(-14, 14, sh)),
}


def synth_scene(rs, B, nver, ntri, H, W, cover=0.85):
    """random ids and a directly drawn tri_ind; the last pixel of every face is covered (the tail of the pixel loops)"""
    tri = rs.randint(0, nver, (3, ntri)).astype(np.float32)
    tri[:, 0] = [0, nver // 2, nver - 1]
    ti = np.where(rs.rand(B, H * W) < cover, rs.randint(0, ntri, (B, H * W)), -1).astype(np.float32)
    ti[:, -1] = rs.randint(0, ntri, B)
    return tri, ti


def nonzero(g):
    g = g.astype(np.float32)
    g[g == 0] = 1.0
    return g


# ---- geometry: the full mesh ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_faces(oracle, full_assets, synth):
    """tri_ind of eight decoded faces from the product's forward (53,215 vertices, 105,840 triangles, 200 x 200), the
    first two checked against the oracle; batches are assembled from them"""
    A = full_assets
    P = synth.sample_params_batch(8, beta=0.7, seed=31)
    V = oracle.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], 200.0)
    tind = ops().render_depth(_t(V), _t(A["tri"]), _t(A["vertex"]), torch.zeros((8, 200, 200, 3), device="cuda:0"))[3]
    tind = tind.cpu().numpy().reshape(8, -1)
    want = oracle.render_depth(V[:2], A["tri"], A["vertex"], 200, 200)[3]
    np.testing.assert_array_equal(tind[:2], want.reshape(2, -1))
    assert V.shape[2] == 53215 and A["tri"].shape[1] == 105840
    assert np.all((tind >= 0).mean(axis=1) > 0.2)
    return A["tri"], tind, V.shape[2]


FULL_MESH = {   # B: the geometry the case is written for
    1: dict(splits=256, range=208, lds=1808, xcd=0),
    3: dict(splits=86, range=619, xcd=0),
    8: dict(splits=32, range=1663, xcd=1),                       # the XCD block map with several owners
    64: dict(splits=4, range=13304, lds=106576, xcd=1),          # the product batch: above 64 KiB, the full-LDS opt-in
    65: dict(splits=4, range=13304, lds=106576, xcd=0),          # the same owners through the other block map
    70: dict(splits=4, range=13304, lds=106576, xcd=0),
}


@pytest.mark.parametrize("profile", sorted(GRADS))
@pytest.mark.parametrize("B", sorted(FULL_MESH))
def test_full_mesh_batches(mesh_faces, B, profile):
    tri, tind, nver = mesh_faces
    rs = np.random.RandomState(100 * B + len(profile))
    ti = tind[(np.arange(B) + B) % 8]
    g = nonzero(GRADS[profile](rs, (B, 200 * 200)))
    M = check(g, tri, ti, nver, 200, 200, dict(FULL_MESH[B], shift=0, chunks=40))
    assert np.count_nonzero(M.bits[:, 2]) > B * 20000


# ---- geometry: owner ranges, vertex counts, pixel counts ------------------------------------------------------------
SYNTH = [   # id, B, nver, ntri, H, W, geometry
    ("largest_owner_range", 256, 16384, 3000, 32, 32, dict(splits=1, range=16384, lds=131216, xcd=1, chunks=1)),
    ("short_last_owner", 256, 16385, 3000, 32, 32, dict(splits=2, range=8193, xcd=1)),
    ("owners_clamped_nver3", 1, 3, 7, 9, 13, dict(splits=3, range=1, lds=152)),
    ("owners_clamped_nver10", 1, 10, 30, 9, 13, dict(splits=10, range=1)),
    ("ranges_3_3_3_1", 64, 10, 30, 9, 13, dict(splits=4, range=3, xcd=1)),
    ("one_vertex_one_triangle", 1, 1, 1, 5, 4, dict(splits=1, range=1)),
    ("nver_above_65536", 16, 70000, 100000, 64, 64, dict(splits=16, range=4375, xcd=1, chunks=4)),
    ("npix_1", 3, 500, 900, 1, 1, dict(splits=84, range=6, chunks=1)),
    ("npix_1023_column", 3, 500, 900, 1023, 1, dict(chunks=1)),
    ("npix_1024_row", 3, 500, 900, 1, 1024, dict(chunks=1)),
    ("npix_1025", 3, 500, 900, 25, 41, dict(chunks=2)),
    ("npix_8191_column", 3, 500, 900, 8191, 1, dict(chunks=8)),
    ("npix_8192", 3, 500, 900, 64, 128, dict(chunks=8)),
    ("npix_8193_row", 3, 500, 900, 1, 8193, dict(chunks=9)),
    ("npix_40000", 3, 500, 900, 200, 200, dict(chunks=40)),
    ("shift0_2pow20", 2, 300, 700, 1024, 1024, dict(shift=0, chunks=1024, splits=100)),
    ("shift1_one_row_more", 2, 300, 700, 1025, 1024, dict(shift=1, chunks=1025)),
    ("shift2_above_2pow21", 2, 300, 700, 1025, 2048, dict(shift=2, chunks=2050)),
]


# (the three images above 2^20 pixels are kept to one case each: the 12-decade gradients)
SYNTH_CASES = [(c, p) for c in SYNTH for p in sorted(GRADS) if p == "decades12" or not c[0].startswith("shift")]


@pytest.mark.parametrize("case,profile", SYNTH_CASES, ids=["%s-%s" % (c[0], p) for c, p in SYNTH_CASES])
def test_launch_geometries(case, profile):
    name, B, nver, ntri, H, W, want_geom = case
    rs = np.random.RandomState(len(name) * 1000 + B + len(profile))
    tri, ti = synth_scene(rs, B, nver, ntri, H, W)
    if ntri == 1:
        tri[:] = 0
    g = nonzero(GRADS[profile](rs, (B, H * W)) * np.exp(rs.uniform(-3, 3, (B, 1))))      # faces of different scale
    M = check(g, tri, ti, nver, H, W, want_geom)
    assert M.bits[:, 2].any(axis=1).all()                       # every face received something
    if name.startswith("shift"):
        assert M.shift == want_geom["shift"]


# ---- values -------------------------------------------------------------------------------------------------------
VB, VNVER, VNTRI, VH, VW = 3, 700, 1500, 64, 50
VGEOM = dict(splits=78, range=9, shift=0, chunks=4, xcd=0)      # several owners per face; faces differ


def value_scene(seed, nver=VNVER):
    rs = np.random.RandomState(seed)
    tri, ti = synth_scene(rs, VB, nver, VNTRI, VH, VW)
    return rs, tri, ti, rs.standard_normal((VB, VH * VW))


def covered_pixels(ti, b, ntri=VNTRI):
    return np.flatnonzero((ti[b] >= 0) & (ti[b] < ntri))


def test_subnormal_gradients_and_the_lowest_normal_binade():
    """face 0: every gradient subnormal (e = -127: every term is on the grid, the sum is exact); face 1: one normal value
    among subnormals; face 2: the largest |g| in the lowest normal binade.  (A flushed denormal in c = g / 3.0f or in the
    conversion would show here.)"""
    rs, tri, ti, n = value_scene(1)
    g = (n * 1e-41).astype(np.float32)
    g[1, covered_pixels(ti, 1)[5]] = 3e-30
    g[2, covered_pixels(ti, 2)[::40]] = 1.9e-38
    assert np.all(np.abs(g[0]) < 1.1754944e-38) and np.count_nonzero(g[0]) > 3000
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    assert M.e.tolist() == [-127, -99, -126]
    X, nv = R.exact(g[:1], tri, ti[:1], VNVER, VH, VW)
    assert R.bound_ratio(M.bits.view(np.float32)[0, 2], X[0], nv[0], -127, 0) == 0.0
    assert np.count_nonzero(M.bits[:, 2]) > 3 * 600


def test_flt_max_with_finite_sums_and_an_overflowing_vertex():
    rs, tri, ti, n = value_scene(2)
    g = (n * 1e30).astype(np.float32)
    for b in range(VB):
        g[b, covered_pixels(ti, b)[7 + b]] = FMAX * (-1) ** b
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    assert M.e.tolist() == [127] * 3 and np.isfinite(M.bits.view(np.float32)).all()
    # four pixels of triangle 0 (vertices 0, nver / 2, nver - 1: first, middle and last owner) at FLT_MAX on face 1, and at
    # -FLT_MAX on face 2: 4 * FLT_MAX / 3 overflows and the model says which infinity
    for b, s in ((1, 1.0), (2, -1.0)):
        px = covered_pixels(ti, b)[20:24]
        ti[b, px] = 0
        g[b, px] = s * FMAX
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    z = M.bits.view(np.float32)[:, 2]
    assert np.isposinf(z[1, [0, VNVER // 2, VNVER - 1]]).all() and np.isneginf(z[2, [0, VNVER // 2, VNVER - 1]]).all()
    assert np.isfinite(z[0]).all() and np.isinf(z).sum() == 6


def test_an_all_zero_face_between_faces_that_are_not():
    rs, tri, ti, n = value_scene(3)
    g = n.astype(np.float32)
    g[1] = np.where(rs.rand(VH * VW) < 0.5, 0.0, -0.0)
    g[1, ti[1] < 0] = 7.0                                       # uncovered pixels do not count
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    assert M.m[1] == 0 and not M.bits[1].any() and M.bits[0, 2].any() and M.bits[2, 2].any()


def test_one_gradient_2_pow_45_times_the_rest():
    """the small terms round to q == 0 and vanish: the model says exactly which vertices become 0, and the derived bound
    still holds against the exact sum"""
    rs, tri, ti, n = value_scene(4)
    g = n.astype(np.float32)
    for b in range(VB):
        g[b, covered_pixels(ti, b)[11 * (b + 1)]] = np.ldexp(1.5, 45 + b)
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    z = M.bits.view(np.float32)[:, 2]
    X, nv = R.exact(g, tri, ti, VNVER, VH, VW)
    for b in range(VB):
        vanished = (z[b] == 0) & (nv[b] > 0) & np.array([x != 0 for x in X[b]])
        assert vanished.sum() > 500 and 1 <= np.count_nonzero(z[b]) <= 3
        assert 0 < R.bound_ratio(z[b], X[b], nv[b], M.e[b], 0) <= 1


def test_the_largest_gradient_on_a_pixel_that_contributes_nothing():
    """the face's largest |g| sits on a pixel whose triangle has a vertex id that is NaN (face 0), -1 (face 1) or nver
    (face 2): it sets the scale and adds nothing, identically in both variants"""
    rs, tri, ti, n = value_scene(5)
    tri[1, 1], tri[0, 2], tri[2, 3], tri[1, 4] = np.nan, -1.0, float(VNVER), 1e10
    g = n.astype(np.float32)
    for b in range(VB):
        px = covered_pixels(ti, b)[30:34]
        ti[b, px] = [1, 2, 3, 4]
        g[b, px[b]] = -3.0e6
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    assert M.m.tolist() == [int(np.float32(3.0e6).view(np.uint32))] * 3 and M.e.tolist() == [21] * 3
    assert np.abs(M.bits.view(np.float32)).max() < 100


def test_inf_and_nan_where_they_do_not_count_and_where_they_do():
    """Inf / NaN on an uncovered pixel and on a pixel with tri_ind >= ntri: the face stays on the fixed-point path.  Inf on
    a covered pixel whose triangle has a bad vertex id: it adds nothing, but the face is bad."""
    rs, tri, ti, n = value_scene(6)
    tri[2, 1] = float(VNVER)
    g = n.astype(np.float32)
    for b in range(VB):
        unc = np.flatnonzero(ti[b] < 0)
        g[b, unc[:4]] = [np.inf, -np.inf, np.nan, FMAX]
        px = covered_pixels(ti, b)[40:43]
        ti[b, px] = [VNTRI, VNTRI + 7, 3e9]
        g[b, px] = [np.nan, np.inf, -np.inf]
    px = covered_pixels(ti, 2)[50]
    ti[2, px] = 1
    g[2, px] = np.inf
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM, n_bad=1)
    assert M.bad.tolist() == [False, False, True] and np.all(M.cls[2] == R.FINITE)


def test_tri_ind_and_vertex_ids_that_are_not_integers():
    """tri_ind -0.5, -0.0 and 0.75 select triangle 0 and ntri - 0.5 the last one; ntri, 3e9, -3e9, NaN, +-Inf nothing;
    ids 0.75 and nver - 0.25 are vertices 0 and nver - 1"""
    rs, tri, ti, n = value_scene(7)
    tri[:, 0] = [0.75, 5.5, VNVER - 0.25]
    tri[:, VNTRI - 1] = [VNVER - 0.25, 0.75, 3.999]
    g = nonzero(n * np.exp(rs.uniform(-14, 5, n.shape)))
    special = np.array([-0.5, -0.0, 0.75, VNTRI - 0.5, VNTRI, 3e9, -3e9, np.nan, np.inf, -np.inf], np.float32)
    assert special[3] == VNTRI - 0.5
    for b in range(VB):
        px = np.arange(100 * (b + 1), 100 * (b + 1) + 10)
        ti[b, px] = np.roll(special, b)
        g[b, px] = rs.uniform(1, 2, 10) * 2.0 ** 20             # large enough to be seen in vertices 0 and nver - 1
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    z = M.bits.view(np.float32)[:, 2]
    assert np.all(np.abs(z[:, [0, 5, VNVER - 1]]) > 2.0 ** 18)


def test_a_bad_face_leaves_its_neighbours_bits_alone():
    rs, tri, ti, n = value_scene(8)
    g = nonzero(n)
    clean = check(g, tri, ti, VNVER, VH, VW, VGEOM)
    px = covered_pixels(ti, 1)
    g[1, px[3]], g[1, px[9]], g[1, px[200]] = np.inf, np.nan, -np.inf
    M = check(g, tri, ti, VNVER, VH, VW, VGEOM, n_bad=1)
    np.testing.assert_array_equal(M.bits[[0, 2]], clean.bits[[0, 2]])
    assert (M.cls[1] != R.FINITE).sum() >= 3 and (M.cls[1] == R.FINITE).sum() > 600


# ---- independence --------------------------------------------------------------------------------------------------
def test_a_faces_bits_do_not_depend_on_the_batch_its_position_or_its_neighbours(mesh_faces):
    """one face's (g, tri_ind) at positions 0, 3 and last of batches of 1, 7, 8 and 64 filled with other faces: 256 / 37 /
    32 / 4 owners per face and both block maps, so this is also the check that the result does not depend on `splits`"""
    tri, tind, nver = mesh_faces
    rs = np.random.RandomState(77)
    npix = 200 * 200
    probe_g = nonzero(rs.standard_normal(npix) * np.exp(rs.uniform(-14, 14, npix)))
    probe_ti = tind[5]
    want = R.model(probe_g, tri, probe_ti, nver, 200, 200).bits[0]
    fill_g = nonzero(rs.standard_normal((64, npix)) * np.exp(rs.uniform(-20, 20, (64, 1))))
    owners = {1: 256, 7: 37, 8: 32, 64: 4}
    seen = 0
    for B in (1, 7, 8, 64):
        g0 = geom(B, nver, 200, 200)
        assert g0["splits"] == owners[B] and g0["xcd"] == (1 if B % 8 == 0 else 0)
        for pos in sorted({0, min(3, B - 1), B - 1}):
            g = fill_g[:B].copy()
            ti = tind[(np.arange(B) * 3 + pos) % 8].copy()
            g[pos], ti[pos] = probe_g, probe_ti
            for o in launch_all(g.reshape(B, 200, 200, 1), tri, ti.reshape(B, 200, 200, 1), nver, 200, 200):
                np.testing.assert_array_equal(o[pos].cpu().numpy().view(np.uint32), want, err_msg="B %d pos %d" % (B, pos))
            seen += 1
    assert seen == 10
