"""GPU: fr_attr_interp_forward / _backward (csrc/fr_attr_interp.hip) and fr_mesh_vertex_normals_backward (csrc/fr_mesh.hip) held to
their float64 models (tests/ref_attr_interp.py, pinned on the CPU by tests/test_attr_interp_cpu.py), the promises the header makes
about their typed scratch tensors, and the opt-in Python surface (attr_interpolate, vertex_normals(grad=True), smooth_planes).

forward, vertex-normal backward:  bit for bit.
interpolation backward, each output:  |got - S| <= 2^-24 |S| + n_v 2^(shift - 39) M    S the exact sum of the model's fp32 terms of
                                      that output, n_v their number, M the face's largest |term| of that output -- in integers
                                      (ref_normal_backward.check_bound); an element without terms is +0.
The shapes and scenes are those of tests/test_depth_interp_gpu.py (tri_ind from the product's own forward); the launch geometry a
case is written for is read from fr_debug_attr_interp_bwd_geom (the launcher's own function)."""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import ref_attr_interp as RA
import ref_normal_backward as RN
import workspace_cases as WC
from conftest import pkg
from gpu_util import ops, net_mod, assert_bits_equal
from raw_calls import dfwd
from test_depth_interp_gpu import scene as depth_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((3, 33, 40), (3, 8, 9), (1, 64, 64), (8, 64, 64))                  # (B, H, W): 33 x 40 = one full 1,024-pixel chunk and a
                                                                              # ragged one; 8 x 9 less than one; B = 8 the XCD map


def _h():
    return pkg("_lib")


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def _stream(stream=None):
    return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def geom(B, nver, H, W):
    out = (ctypes.c_int * 6)()
    _h().lib().fr_debug_attr_interp_bwd_geom(B, nver, H, W, out)
    return dict(zip(("splits", "range", "shift", "chunks", "lds", "xcd"), out))


def _pitched(x, nver, pad):
    """[B,3,nver] -> [B,3,nver + pad] with NaN in the pad columns"""
    p = _nan(x.shape[0], 3, nver + pad)
    p[:, :, :nver] = x
    return p


# ---- the raw calls, on torch's current stream unless one is given; outputs pre-filled with NaN --------------------------------------
def afwd(V, A, tri, ti, H, W, nver=None, stream=None):
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if nver is None else nver
    out = _nan(B, H, W, 3)
    rc = L.fr_attr_interp_forward(h.ptr(V), int(V.shape[2]), h.ptr(A), int(A.shape[2]), h.ptr(tri), h.ptr(ti), B, nver, int(tri.shape[1]),
                                  H, W, h.ptr(out), _stream(stream))
    assert rc == 0, rc
    return out


def scratch(B, H, W, fill=0xA5):
    """(records int32 [2,B,3,HW,4], partial uint32 [2,B,chunks,2]) as the header states them, filled with a byte"""
    rec = torch.full((2, B, 3, H * W, 4 * 4), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
    part = torch.full((2, B, (H * W + 1023) // 1024, 2 * 4), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
    assert rec.shape == (2, B, 3, H * W, 4) and part.shape == (2, B, (H * W + 1023) // 1024, 2)
    return rec, part


def abwd(g, V, A, tri, ti, H, W, want=(True, True), out=(None, None), accumulate=(0, 0), nver=None, stream=None, rec=None, part=None):
    """-> (attr_grad, vertex_grad); an output that is not wanted is None"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if nver is None else nver
    if rec is None:
        rec, part = scratch(B, H, W)
    outs = [(o if o is not None else _nan(B, 3, nver)) if w else None for o, w in zip(out, want)]
    rc = L.fr_attr_interp_backward(h.ptr(g), h.ptr(V), int(V.shape[2]), h.ptr(A), int(A.shape[2]), h.ptr(tri), h.ptr(ti),
                                   h.ptr(outs[0]), accumulate[0], h.ptr(outs[1]), accumulate[1], B, nver, int(tri.shape[1]), H, W,
                                   ctypes.c_void_p(rec.data_ptr()), ctypes.c_void_p(part.data_ptr()), _stream(stream))
    assert rc == 0, rc
    return outs


def vnbwd(g, V, tri, adj, nver=None, out=None, accumulate=0, out_pitch=None):
    """fr_mesh_vertex_normals_backward with an h of its own -> vertex_grad [B,3,out_pitch]"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if nver is None else nver
    out_pitch = nver if out_pitch is None else out_pitch
    hbuf = torch.full((B, 3, nver), float("nan"), dtype=torch.float64, device=DEV)
    if out is None:
        out = _nan(B, 3, out_pitch)
    a0, a1 = _t(adj[0], np.int32), _t(adj[1], np.int32)
    rc = L.fr_mesh_vertex_normals_backward(h.ptr(g), int(g.shape[2]), h.ptr(V), int(V.shape[2]), h.ptr(tri), h.ptr(a0), h.ptr(a1), B,
                                           nver, int(tri.shape[1]), h.ptr(hbuf), h.ptr(out), out_pitch, accumulate, _stream())
    assert rc == 0, rc
    return out


# ---- scenes: the depth-interp ones, with a random attribute and a three-channel gradient (neither with a zero) ---------------------
_SCENES = {}


def scene(small_assets, B, H, W):
    key = (B, H, W)
    if key not in _SCENES:
        sc = dict(depth_scene(small_assets, B, H, W))
        rs = np.random.RandomState(7 * B + H)
        sc["A"] = rs.uniform(-1, 1, sc["V"].shape).astype(np.float32)
        sc["A"][sc["A"] == 0] = 0.5
        sc["g3"] = rs.standard_normal((B, H * W, 3)).astype(np.float32)
        sc["g3"][sc["g3"] == 0] = 1.0
        sc["model"] = RA.model(sc["g3"], sc["V"], sc["A"], sc["tri"], sc["tind"], H, W)          # computed once, never written
        _SCENES[key] = sc
    return _SCENES[key]


def _dev(sc):
    return _t(sc["g3"]), _t(sc["V"]), _t(sc["A"]), _t(sc["tri"]), _t(sc["tind"])


# ---- forward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_is_the_model_bit_for_bit(small_assets, B, H, W):
    sc = scene(small_assets, B, H, W)
    gm = geom(B, 480, H, W)
    assert sc["nver"] == 480 and gm["xcd"] == (1 if B == 8 else 0) and gm["chunks"] == (H * W + 1023) // 1024
    cov = sc["tind"] >= 0
    assert cov.any() and not cov.all()
    want = RA.forward(sc["V"], sc["A"], sc["tri"], sc["tind"], H, W)
    _, V, A, tri, ti = _dev(sc)
    got = afwd(V, A, tri, ti, H, W)
    assert_bits_equal(got.cpu().numpy(), want, "interpolated attribute")
    assert not bool(_bits(got).view(B, H * W, 3)[torch.as_tensor(~cov)].any())                   # (+0, +0, +0) off the face
    assert _same(afwd(_pitched(V, 480, 22), _pitched(A, 480, 9), tri, ti, H, W, nver=480), got)   # pitched vertex and attribute rows
    # a constant attribute comes out as that constant wherever the pixel is OK (no triangle of the scene is without area)
    const = torch.tensor([0.75, -1.3, 2.0], device=DEV).view(1, 3, 1).expand(B, 3, 480).contiguous()
    plane = afwd(V, const, tri, ti, H, W).view(B, H * W, 3)[torch.as_tensor(cov)]
    assert _same(plane, const[0, :, 0].expand(plane.shape[0], 3))
    # the vertices as their own attribute: channel 2 is the interpolated depth on the face
    own = afwd(V, V, tri, ti, H, W).view(B, H * W, 3)[..., 2][torch.as_tensor(cov)]
    assert _same(own, dfwd(V, tri, ti, H, W).view(B, H * W)[torch.as_tensor(cov)])


def _hand_made(small_assets):
    """[2,8,9]: -1, NaN, ntri, 3e9, a triangle with an id >= nver, a triangle with two coincident vertices (den == 0)"""
    sc = scene(small_assets, 3, 8, 9)
    V, A = sc["V"][:2].copy(), sc["A"][:2].copy()
    nver, H, W = sc["nver"], 8, 9
    tri = sc["tri"].copy()
    ntri = tri.shape[1]
    bad_t, flat_t = 7, 11
    tri[1, bad_t] = nver
    p1, p2 = int(tri[0, flat_t]), int(tri[1, flat_t])
    V[:, 0:2, p2] = V[:, 0:2, p1]
    rs = np.random.RandomState(8)
    tind = rs.randint(0, ntri, (2, H * W)).astype(np.float32)
    tind[:, 0:6] = (-1, np.nan, ntri, bad_t, flat_t, ntri + 5)
    tind[1, 40:44] = (flat_t, bad_t, -1, 3e9)
    g = rs.standard_normal((2, H * W, 3)).astype(np.float32)
    return dict(V=V, A=A, tri=tri, tind=tind, g=g, H=H, W=W, nver=nver, flat_t=flat_t)


def test_forward_and_backward_on_a_hand_made_tri_ind(small_assets):
    hm = _hand_made(small_assets)
    V, A, tri, tind, g, H, W, nver = (hm[k] for k in ("V", "A", "tri", "tind", "g", "H", "W", "nver"))
    want = RA.forward(V, A, tri, tind, H, W)
    w = want.reshape(2, -1, 3)
    assert not w[:, [0, 1, 2, 3, 5]].view(np.uint32).any() and not w[1, [41, 42, 43]].view(np.uint32).any()
    for b in range(2):
        a = A[b][:, [int(tri[k, hm["flat_t"]]) for k in range(3)]]
        flat = ((a[:, 0] + a[:, 1]) + a[:, 2]) / np.float32(3)
        assert np.array_equal(w[b, 4], flat) and np.array_equal(w[1, 40], w[1, 4])
    got = afwd(_t(V), _t(A), _t(tri), _t(tind), H, W)
    assert_bits_equal(got.cpu().numpy(), want, "hand-made tri_ind")
    Ra, Rv = RA.model(g, V, A, tri, tind, H, W)
    ga, gv = abwd(_t(g), _t(V), _t(A), _t(tri), _t(tind), H, W)
    assert RN.check_bound(ga.cpu().numpy(), Ra) <= 1.0 and RN.check_bound(gv.cpu().numpy(), Rv) <= 1.0
    pa, pv = abwd(_t(g), _pitched(_t(V), nver, 22), _pitched(_t(A), nver, 9), _t(tri), _t(tind), H, W, nver=nver)
    assert _same(pa, ga) and _same(pv, gv)


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_backward_within_the_bound_of_the_exact_sums(small_assets, B, H, W):
    sc = scene(small_assets, B, H, W)
    gm = geom(B, 480, H, W)
    assert gm["lds"] <= 160 * 1024 and gm["shift"] == 0 and gm["xcd"] == (1 if B == 8 else 0)
    Ra, Rv = sc["model"]
    assert not any(F.bad for F in Ra.faces + Rv.faces)
    g, V, A, tri, ti = _dev(sc)
    ga, gv = abwd(g, V, A, tri, ti, H, W)
    wa = RN.check_bound(ga.cpu().numpy(), Ra)                                 # ... and exactly +0 where no OK pixel names the vertex
    wv = RN.check_bound(gv.cpu().numpy(), Rv)
    print("B=%d %dx%d: %d owners of %d vertices, worst error / bound: attr %.3f, vertex %.3f" % (B, H, W, gm["splits"], gm["range"], wa, wv))
    assert wa <= 1.0 and wv <= 1.0
    assert not bool(_bits(gv[:, 2]).any())                                    # the z row: +0
    assert all(float(ga[:, c].abs().max()) > 0 for c in range(3)) and float(gv[:, 0].abs().max()) > 0 and float(gv[:, 1].abs().max()) > 0
    # each output requested alone: the bits it has when both are requested
    a_only, none = abwd(g, V, A, tri, ti, H, W, want=(True, False))
    none2, v_only = abwd(g, V, A, tri, ti, H, W, want=(False, True))
    assert none is None and none2 is None and _same(a_only, ga) and _same(v_only, gv)
    # accumulate: one fp32 add per element, per output
    gen = torch.Generator().manual_seed(B + H)
    olda, oldv = torch.randn(ga.shape, generator=gen).to(DEV), torch.randn(gv.shape, generator=gen).to(DEV)
    acca, accv = abwd(g, V, A, tri, ti, H, W, out=(olda.clone(), oldv.clone()), accumulate=(1, 1))
    assert _same(acca, olda + ga) and _same(accv, oldv + gv)
    mixa, mixv = abwd(g, V, A, tri, ti, H, W, out=(olda.clone(), oldv.clone()), accumulate=(0, 1))
    assert _same(mixa, ga) and _same(mixv, oldv + gv)


def test_a_faces_bits_do_not_depend_on_its_batch(small_assets):
    sc = scene(small_assets, 8, 64, 64)
    H = W = 64
    g, V, A, tri, ti = _dev(sc)
    ga, gv = abwd(g, V, A, tri, ti, H, W)
    ga2, gv2 = abwd(g, V, A, tri, ti, H, W)
    assert _same(ga, ga2) and _same(gv, gv2)
    assert len({geom(n, 480, H, W)["range"] for n in (1, 8)}) == 2
    for b in (0, 5, 7):
        pa, pv = abwd(g[b:b + 1].contiguous(), V[b:b + 1].contiguous(), A[b:b + 1].contiguous(), tri, ti[b:b + 1].contiguous(), H, W)
        assert _same(pa, ga[b:b + 1]) and _same(pv, gv[b:b + 1]), b


def test_a_nan_gradient_stays_in_its_face(small_assets):
    sc = scene(small_assets, 3, 33, 40)
    H, W = 33, 40
    g, V, A, tri, ti = _dev(sc)
    ga, gv = abwd(g, V, A, tri, ti, H, W)
    gn = sc["g3"].copy()
    px = int(np.flatnonzero(sc["tind"][1] >= 0)[5])
    gn[1, px, 1] = np.nan
    na, nv = abwd(_t(gn), V, A, tri, ti, H, W)
    for got, clean in ((na, ga), (nv, gv)):
        assert _same(got[0], clean[0]) and _same(got[2], clean[2])            # faces 0 and 2 keep their bits
    ids = sorted({int(sc["tri"][k, int(sc["tind"][1, px])]) for k in range(3)})
    Ra, Rv = RA.model(gn, sc["V"], sc["A"], sc["tri"], sc["tind"], H, W)
    assert [F.bad for F in Ra.faces] == [False, True, False] and [F.bad for F in Rv.faces] == [False, True, False]
    assert RN.check_bad_faces(na.cpu().numpy(), Ra) == 1 and RN.check_bad_faces(nv.cpu().numpy(), Rv) == 1
    bad_a = ~np.isfinite(na[1].cpu().numpy())
    assert bad_a[1, ids].all() and not bad_a[0].any() and not bad_a[2].any()  # channel 1 of the triangle's three vertices, nothing else
    bad_v = ~np.isfinite(nv[1].cpu().numpy())
    assert bad_v[0:2, ids].all() and not bad_v[2].any() and not bool(_bits(nv[1, 2]).any())


# ---- the scratch tensors' three promises ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ("even", "ragged"))
def test_scratch_needs_nothing_cleared_keeps_to_its_shape_and_its_alignment(shape):
    """records and partial placed at exactly their stated alignment (16 and 8 bytes, and no larger power of two) between guard
    bytes, under three fills: the outputs keep their bits and the guards theirs"""
    sc = WC.scene(shape, owner=True)
    B, H, W, nver = sc["B"], sc["H"], sc["W"], sc["nver"]
    assert (B, H, W, nver) == ((1, 32, 32, 64) if shape == "even" else (3, 17, 31, 257))
    gm = geom(B, nver, H, W)
    assert shape == "even" or (H * W % 1024 and nver % gm["range"] and gm["splits"] > 1)
    g, V, A, tri, ti = (WC._t(sc[k]) for k in ("g3", "V", "tex", "tri", "tind"))  # (copies: the shared inputs are read-only arrays)
    rec_bytes, part_bytes = 2 * B * 3 * H * W * 16, 2 * B * ((H * W + 1023) // 1024) * 8
    want = None
    for tag, fill in WC.FILLS:
        gb = WC.GUARD_BYTES[tag]
        rw, ro = WC.place(rec_bytes, 16, guard_byte=gb)
        pw, po = WC.place(part_bytes, 8, guard_byte=gb)
        rw[ro:ro + rec_bytes] = fill
        pw[po:po + part_bytes] = fill
        rec, part = rw[ro:ro + rec_bytes].view(torch.int32), pw[po:po + part_bytes].view(torch.int32)
        assert rec.data_ptr() % 32 == 16 and part.data_ptr() % 16 == 8
        ga, gv = abwd(g, V, A, tri, ti, H, W, rec=rec, part=part)
        torch.cuda.synchronize()
        got = {"attr_grad": ga, "vertex_grad": gv}
        assert WC.guard_damage(rw, ro, rec_bytes, gb) is None, (tag, WC.guard_damage(rw, ro, rec_bytes, gb))
        assert WC.guard_damage(pw, po, part_bytes, gb) is None, (tag, WC.guard_damage(pw, po, part_bytes, gb))
        if want is None:
            want = got
            Ra, Rv = RA.model(sc["g3"], sc["V"], sc["tex"], sc["tri"], sc["tind"], H, W)
            assert RN.check_bound(ga.cpu().numpy(), Ra) <= 1.0 and RN.check_bound(gv.cpu().numpy(), Rv) <= 1.0
            assert float(ga.abs().max()) > 0 and float(gv.abs().max()) > 0
        assert WC.bit_difference(got, want) is None, (tag, WC.bit_difference(got, want))


# ---- the vertex normals' backward -------------------------------------------------------------------------------------------------------------
def test_vertex_normal_backward_is_the_model_bit_for_bit(small_assets):
    """two faces of the small mesh; vertex 100 written out of every triangle that names it (those triangles then name another
    vertex twice, and 100 has no triangle: its forward normal is (0, 0, 0)), triangle 3 given an id out of range"""
    mesh_io = pkg("utils.mesh_io")
    sc = scene(small_assets, 3, 33, 40)
    V = sc["V"][:2]
    nver = sc["nver"]
    tri = sc["tri"].copy()
    lone = 100
    hit = np.flatnonzero((tri == lone).any(axis=0))
    assert hit.size >= 2
    for t in hit:
        for k in range(3):
            if tri[k, t] == lone:
                tri[k, t] = tri[(k + 1) % 3, t]
    tri[2, 3] = nver
    adj = mesh_io.vertex_adjacency(tri, nver)
    rs = np.random.RandomState(3)
    g = rs.standard_normal(V.shape).astype(np.float32)
    want, _, hh = RA.normals_backward(g, V, tri, adj[0], adj[1])
    assert not want[:, :, lone].view(np.uint32).any() and not hh[:, :, lone].any()
    fwd = ops().vertex_normals(_t(V), _t(tri), adj)
    assert not bool(_bits(fwd[:, :, lone]).any()) and float(fwd.abs().max()) > 0
    got = vnbwd(_t(g), _t(V), _t(tri), adj)
    assert_bits_equal(got.cpu().numpy(), want, "vertex-normal backward")
    assert all(float(got[:, c].abs().max()) > 0 for c in range(3))
    # pitched rows on all three tensors: the pad columns of the output stay as they were
    po = vnbwd(_pitched(_t(g), nver, 5), _pitched(_t(V), nver, 22), _t(tri), adj, nver=nver, out_pitch=nver + 3)
    assert _same(po[:, :, :nver], got) and bool(torch.isnan(po[:, :, nver:]).all())
    # accumulate: fl32(old + out)
    old = rs.standard_normal(V.shape).astype(np.float32)
    acc = vnbwd(_t(g), _t(V), _t(tri), adj, out=_t(old), accumulate=1)
    assert_bits_equal(acc.cpu().numpy(), RA.normals_backward(g, V, tri, adj[0], adj[1], old=old)[0], "accumulate")
    assert _same(acc, _t(old) + got)


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------------
class _Py:
    pass


@pytest.fixture(scope="module")
def py(small_assets):
    """the small mesh decoded at 64 x 64, two faces, its render's tri_ind; random weights for the planes"""
    s = _Py()
    s.B, s.S = 2, 64
    A = small_assets
    s.net = net_mod().FaceRecNet(mesh_data=A, batch_size=s.B, im_size=s.S, device=torch.device(DEV))
    rs = np.random.RandomState(0)
    P = np.zeros((s.B, 7 + A["ndim_shape"] + A["ndim_exp"]), np.float32)
    P[:, 0:3] = rs.uniform(-0.4, 0.4, (s.B, 3))
    P[:, 3:5] = rs.uniform(29, 35, (s.B, 2))
    P[:, 6] = rs.uniform(2.8e-4, 3.4e-4, s.B)
    P[:, 7:7 + A["ndim_shape"]] = rs.uniform(0, 1e4, (s.B, A["ndim_shape"]))
    P[:, 7 + A["ndim_shape"]:] = rs.uniform(-1.5, 1.5, (s.B, A["ndim_exp"]))
    s.V = s.net.vertices_transform(_t(P)).detach()
    gen = torch.Generator().manual_seed(9)
    s.w3 = torch.randn((s.B, s.S, s.S, 3), generator=gen).to(DEV)
    s.wv = torch.randn(tuple(s.V.shape), generator=gen).to(DEV)
    s.image = torch.zeros((s.B, s.S, s.S, 3), device=DEV)
    s.tind = ops().render_depth(s.V, s.net.tri, s.net.vertex_code, s.image)[3].detach()
    s.attr = torch.rand(tuple(s.V.shape), generator=gen).to(DEV) + 0.1
    return s


def test_attr_interpolate_is_the_raw_calls(py):
    o, s = ops(), py
    V, A = s.V.clone().requires_grad_(True), s.attr.clone().requires_grad_(True)
    out = o.attr_interpolate(V, A, s.net.tri, s.tind)
    assert _same(out, afwd(s.V, s.attr, s.net.tri, s.tind, s.S, s.S))
    (out * s.w3).sum().backward()
    ga, gv = abwd(s.w3.reshape(s.B, -1, 3).contiguous(), s.V, s.attr, s.net.tri, s.tind, s.S, s.S)
    assert _same(A.grad, ga) and _same(V.grad, gv)
    # only the gradients autograd needs
    A2 = s.attr.clone().requires_grad_(True)
    (o.attr_interpolate(s.V, A2, s.net.tri, s.tind) * s.w3).sum().backward()
    assert _same(A2.grad, ga)
    V2 = s.V.clone().requires_grad_(True)
    (o.attr_interpolate(V2, s.attr, s.net.tri, s.tind) * s.w3).sum().backward()
    assert _same(V2.grad, gv)
    # a shared attribute: expanded first, its gradient torch's sum over the faces
    for shared in (s.attr[0].clone(), s.attr[0:1].clone()):
        shared.requires_grad_(True)
        out1 = o.attr_interpolate(s.V, shared, s.net.tri, s.tind)
        rep = s.attr[0:1].expand(s.B, -1, -1).contiguous()
        assert _same(out1, afwd(s.V, rep, s.net.tri, s.tind, s.S, s.S))
        (out1 * s.w3).sum().backward()
        per_face = abwd(s.w3.reshape(s.B, -1, 3).contiguous(), s.V, rep, s.net.tri, s.tind, s.S, s.S, want=(True, False))[0]
        assert tuple(shared.grad.shape) == tuple(shared.shape)
        assert torch.allclose(shared.grad.reshape(3, -1), per_face.sum(0), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        o.attr_interpolate(s.V, s.attr, s.net.tri, s.tind.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        o.attr_interpolate(s.V, s.attr[:, :, :-1], s.net.tri, s.tind)


def test_vertex_normals_grad_flag(py):
    o, s = ops(), py
    adj = s.net.adjacency()
    V = s.V.clone().requires_grad_(True)
    plain = o.vertex_normals(V, s.net.tri, adj)
    assert not plain.requires_grad and plain.grad_fn is None                  # the default: outside autograd, as before
    n = o.vertex_normals(V, s.net.tri, adj, grad=True)
    assert n.requires_grad and _same(n, plain)
    (n * s.wv).sum().backward()
    raw = vnbwd(s.wv, s.V, s.net.tri, (adj.adj_start.cpu().numpy(), adj.adj_tri.cpu().numpy()))
    assert _same(V.grad, raw) and all(float(raw[:, c].abs().max()) > 0 for c in range(3))


def test_smooth_planes_reach_the_vertices_and_alpha(py):
    o, s, net = ops(), py, py.net
    gen = torch.Generator().manual_seed(4)
    alpha = (0.3 * torch.randn((s.B, int(net.pc_tex.shape[1])), generator=gen)).to(DEV).requires_grad_(True)
    light = torch.zeros((s.B, 3, 9), device=DEV)
    light[:, :, 0] = 0.8
    light[:, :, 1:4] = 0.3 * torch.randn((s.B, 3, 3), generator=gen).to(DEV)
    target = torch.rand((s.B, s.S, s.S, 3), generator=gen).to(DEV)
    V = s.V.clone().requires_grad_(True)
    tex = o.synth_texture(net.mu_tex, net.pc_tex, alpha)
    tex_img, normal = net.smooth_planes(V, tex, s.tind)
    assert tuple(tex_img.shape) == tuple(normal.shape) == (s.B, s.S, s.S, 3)
    assert _same(tex_img, afwd(s.V, tex.detach(), net.tri, s.tind, s.S, s.S))
    assert _same(normal, afwd(s.V, o.vertex_normals(s.V, net.tri, net.adjacency()), net.tri, s.tind, s.S, s.S))
    flat = o.render_depth(s.V, net.tri, tex.detach(), s.image)
    assert not _same(tex_img, flat[1]) and not _same(normal, flat[2])
    sse, count = o.photo_loss_rgb(tex_img, normal, s.tind, light, target)
    (sse.sum() / (3 * count.sum()).clamp_min(1)).backward()
    assert bool(torch.isfinite(V.grad).all()) and all(float(V.grad[:, c].abs().max()) > 0 for c in range(3))
    assert bool(torch.isfinite(alpha.grad).all()) and float(alpha.grad.abs().max()) > 0
    # one plane alone costs nothing for the other; the layouts are synth_shade's too
    only_tex, none = net.smooth_planes(s.V, tex.detach(), s.tind, normals=False)
    none2, only_n = net.smooth_planes(s.V, tex.detach(), s.tind, tex=False)
    assert none is None and none2 is None and _same(only_tex, tex_img) and _same(only_n, normal)
    im_rgb, im_gray, mask = o.synth_shade_rgb(only_tex, only_n, s.tind, light)
    assert bool(torch.isfinite(im_rgb).all()) and float(im_rgb.abs().max()) > 0 and _same(mask, (s.tind >= 0).float())


def test_two_threads_two_streams(py):
    """two host threads, each forward and backward through the autograd nodes on a stream of its own (the scratch comes from the
    stream-scoped pool): the serial bits"""
    o, s = ops(), py
    adj = s.net.adjacency()

    def job(i):
        V = (s.V + 0.01 * i).requires_grad_(True)
        n = o.attr_interpolate(V, o.vertex_normals(V, s.net.tri, adj, grad=True), s.net.tri, s.tind)
        (n * s.w3 * (i + 1)).sum().backward()
        return n.detach(), V.grad
    refs = [job(i) for i in range(2)]
    streams = [torch.cuda.Stream(device=DEV) for _ in refs]
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(refs))

    def worker(i):
        bad = []
        barrier.wait(timeout=60)
        with torch.cuda.stream(streams[i]):
            for it in range(6):
                n, gV = job(i)
                streams[i].synchronize()
                if not (_same(n, refs[i][0]) and _same(gV, refs[i][1])):
                    bad.append("thread %d iteration %d" % (i, it))
        return bad

    ex = ThreadPoolExecutor(max_workers=len(refs))
    try:
        futs = [ex.submit(worker, i) for i in range(len(refs))]
        bad = sum((f.result(timeout=180) for f in futs), [])
    finally:
        ex.shutdown(wait=False, cancel_futures=True)
    assert not bad, bad[:10]
