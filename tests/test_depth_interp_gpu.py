"""GPU: fr_depth_interp_forward / fr_depth_interp_backward (csrc/fr_depth_interp.hip) held to their float64 model
(tests/ref_depth_interp.py, pinned on the CPU by tests/test_depth_interp_cpu.py), and the opt-in `depth_interp` flag of the Python
surface.

forward:   bit for bit.
backward:  |got - S| <= 2^-24 |S| + n_v 2^(shift - 39) M     S the exact sum of the model's fp32 terms, n_v their number, M the
                                                             face's largest |term| -- evaluated in integers
                                                             (ref_normal_backward.check_bound); an element without terms is +0.
tri_ind always comes from the product's own forward (or is made by hand where the case says so); the launch geometry a case is
written for is read from fr_debug_depth_interp_bwd_geom (the launcher's own function)."""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import ref_depth_interp as RD
import ref_normal_backward as RN
from conftest import pkg
from gpu_util import ops, net_mod, assert_bits_equal
from raw_calls import dbwd, dfwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _h():
    return pkg("_lib")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def _stream(stream=None):
    return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def geom(B, nver, H, W):
    out = (ctypes.c_int * 6)()
    _h().lib().fr_debug_depth_interp_bwd_geom(B, nver, H, W, out)
    return dict(zip(("splits", "range", "shift", "chunks", "lds", "xcd"), out))


# ---- scenes: the synthetic mesh placed on an H x W screen, a pose per face ---------------------------------------------------------
def make_scene(A, B, H, W, seed):
    """-> dict of numpy arrays: V [B,3,nver] (the mean shape scaled to ~0.7 of the screen, turned a little about two axes and
    jittered per face), tri, tind [B,H*W] (the product's forward), g [B,H*W] (no zero)"""
    rs = np.random.RandomState(seed)
    N = A["mu"].shape[0] // 3
    mu = A["mu"].reshape(3, N).astype(np.float64)
    V = np.zeros((B, 3, N), np.float32)
    for b in range(B):
        ay, ax = rs.uniform(-0.4, 0.4, 2)
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        P = (Rx @ Ry @ mu) * np.array([[0.35 * W / 7.0e4], [0.35 * H / 8.0e4], [1e-4]])
        P += np.array([[W / 2.0], [H / 2.0], [20.0]]) + rs.uniform(-0.05, 0.05, (3, N))
        V[b] = P
    tri = A["tri"]
    outs = ops().render_depth(_t(V), _t(tri), _t(A["vertex"]), torch.zeros((B, H, W, 3), device=DEV))
    tind = outs[3].cpu().numpy().reshape(B, H * W)
    g = rs.standard_normal((B, H * W)).astype(np.float32)
    g[g == 0] = 1.0
    return dict(V=V, tri=tri, tind=tind, g=g, flat=outs[0].cpu().numpy(), H=H, W=W, B=B, nver=N)


_SCENES = {}
SHAPES = ((3, 33, 40), (3, 8, 9), (1, 64, 64), (3, 64, 64), (8, 64, 64))      # (B, H, W): 33 x 40 = one full 1,024-pixel chunk and
                                                                              # a ragged one; 8 x 9 less than one; B = 8 the XCD map


def scene(small_assets, B, H, W):
    key = (B, H, W)
    if key not in _SCENES:
        _SCENES[key] = make_scene(small_assets, B, H, W, 100 * B + H)
    return _SCENES[key]


# ---- forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_is_the_model_bit_for_bit(small_assets, B, H, W):
    sc = scene(small_assets, B, H, W)
    assert sc["nver"] == 480
    cov = sc["tind"] >= 0
    assert cov.any() and not cov.all()
    assert geom(B, 480, H, W)["xcd"] == (1 if B == 8 else 0) and geom(B, 480, H, W)["chunks"] == (H * W + 1023) // 1024
    want = RD.forward(sc["V"], sc["tri"], sc["tind"], H, W)
    got = dfwd(_t(sc["V"]), _t(sc["tri"]), _t(sc["tind"]), H, W).cpu().numpy()
    assert_bits_equal(got, want, "interpolated depth")
    # the plane does differ from the flat h where a triangle wins, and is the background where none does
    assert (got.reshape(B, -1)[cov] != sc["flat"].reshape(B, -1)[cov]).mean() > 0.9
    assert_bits_equal(got.reshape(B, -1)[~cov], sc["flat"].reshape(B, -1)[~cov], "background")


def test_forward_on_a_hand_made_tri_ind(small_assets):
    """[2,8,9,1]: -1, NaN, ntri and a triangle with an id >= nver give the background; a triangle with two coincident vertices
    (den == 0) gives the flat h; vertex rows of pitch nver + 22 give the dense result"""
    sc = scene(small_assets, 3, 8, 9)
    V = sc["V"][:2].copy()
    nver, H, W = sc["nver"], 8, 9
    tri = sc["tri"].copy()
    ntri = tri.shape[1]
    bad_t, flat_t = 7, 11
    tri[1, bad_t] = nver                                                      # an id >= nver
    p1, p2 = int(tri[0, flat_t]), int(tri[1, flat_t])
    V[:, 0:2, p2] = V[:, 0:2, p1]                                             # two coincident vertices (z differs): den == 0
    rs = np.random.RandomState(8)
    tind = rs.randint(0, ntri, (2, H * W)).astype(np.float32)
    tind[:, 0:6] = (-1, np.nan, ntri, bad_t, flat_t, ntri + 5)
    tind[1, 40:44] = (flat_t, bad_t, -1, 3e9)
    want = RD.forward(V, tri, tind, H, W)
    bg = RD.BACKGROUND.view(np.uint32)
    w = want.reshape(2, -1)
    assert np.all(w[:, [0, 1, 2, 3, 5]].view(np.uint32) == bg) and np.all(w[1, [41, 42, 43]].view(np.uint32) == bg)
    for b in range(2):
        z = V[b, 2, [int(tri[k, flat_t]) for k in range(3)]]
        assert w[b, 4] == np.float32(np.float32(np.float32(z[0] + z[1]) + z[2]) / np.float32(3)) and w[1, 40] == w[1, 4]
    got = dfwd(_t(V), _t(tri), _t(tind), H, W)
    assert_bits_equal(got.cpu().numpy(), want, "hand-made tri_ind")
    pitch = nver + 22
    Vp = torch.full((2, 3, pitch), float("nan"), device=DEV)
    Vp[:, :, :nver] = _t(V)
    assert _same(dfwd(Vp, _t(tri), _t(tind), H, W, pitch=(pitch, nver)), got)
    # the backward on the same plane: the model's bound, the flat term on the den == 0 pixels, and the pitched rows' bits
    g = rs.standard_normal((2, H * W)).astype(np.float32)
    R = RD.model(g, V, tri, tind, H, W)
    gb = dbwd(_t(g), _t(V), _t(tri), _t(tind), H, W)
    assert RN.check_bound(gb.cpu().numpy(), R) <= 1.0
    assert _same(dbwd(_t(g), Vp, _t(tri), _t(tind), H, W, pitch=(pitch, nver)), gb)


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def _backward_case(sc):
    B, H, W = sc["B"], sc["H"], sc["W"]
    g, V, tri, ti = _t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    R = RD.model(sc["g"], sc["V"], sc["tri"], sc["tind"], H, W)
    assert not any(F.bad for F in R.faces)
    got = dbwd(g, V, tri, ti, H, W)
    worst = RN.check_bound(got.cpu().numpy(), R)                             # ... and exactly +0 where no ok pixel names the vertex
    assert worst <= 1.0
    touched = np.zeros((B, sc["nver"]), bool)
    for b, F in enumerate(R.faces):
        touched[b, F.elem % sc["nver"]] = True
    assert touched.any()
    assert float(got[:, 0].abs().max()) > 0 and float(got[:, 1].abs().max()) > 0 and float(got[:, 2].abs().max()) > 0
    old = torch.randn(got.shape, generator=torch.Generator().manual_seed(B + H)).to(DEV)
    acc = dbwd(g, V, tri, ti, H, W, out=old.clone(), accumulate=1)
    assert _same(acc, old + got)                                              # one fp32 add per element
    return worst, touched


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_backward_within_the_bound_of_the_exact_sums(small_assets, B, H, W):
    gm = geom(B, 480, H, W)
    assert gm["lds"] <= 160 * 1024 and gm["shift"] == 0
    worst, touched = _backward_case(scene(small_assets, B, H, W))
    assert (H, W) != (8, 9) or not touched.all()                             # vertices no ok pixel names: held to +0 by check_bound
    print("B=%d %dx%d: %d owners of %d vertices, worst error / bound = %.3f" % (B, H, W, gm["splits"], gm["range"], worst))


def test_backward_with_several_owners_per_face_of_a_larger_mesh(synth):
    """make_assets on a grid chosen so that, at B = 8 (the XCD block map), a face has several owners of more than a triangle's
    vertices each: the mesh's triangles straddle the owner boundaries"""
    gu, gv, B, H, W = 40, 50, 8, 33, 40
    gm = geom(B, gu * gv, H, W)
    assert gm["splits"] >= 2 and gm["range"] > gv and gm["xcd"] == 1, gm      # an owner holds more than a row of the grid
    A = synth.make_assets(grid_u=gu, grid_v=gv, n_shape=2, n_exp=2, patch=(3, 4, 2, 3))
    sc = make_scene(A, B, H, W, 77)
    owners = (sc["tri"].astype(np.int64) // gm["range"])
    assert (owners.max(axis=0) != owners.min(axis=0)).any()
    worst, _ = _backward_case(sc)
    print("%d owners of %d vertices: worst error / bound = %.3f" % (gm["splits"], gm["range"], worst))


def test_backward_is_bit_reproducible_whatever_the_launch_geometry(small_assets):
    """Two calls: the same bits.  The owner passes (csrc/fr_owner_scatter.h owner_rows3, shared with fr_render_nbwd.hip) read no
    entry of the option table -- their geometry is a function of (B, nver, H, W) alone -- so the geometry is moved the only way it
    can be: a face computed alone (B = 1), among three and among eight (the XCD block map) -- three different owner ranges --
    gives the same bits; and the backward knobs that do exist (the decode backward's) change nothing."""
    sc = scene(small_assets, 8, 64, 64)
    H = W = 64
    g, V, tri, ti = _t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    first = dbwd(g, V, tri, ti, H, W)
    assert _same(dbwd(g, V, tri, ti, H, W), first)
    assert len({geom(n, 480, H, W)["range"] for n in (1, 3, 8)}) == 3
    for n in (1, 3):
        for b0 in (0, 8 - n):
            part = dbwd(g[b0:b0 + n].contiguous(), V[b0:b0 + n].contiguous(), tri, ti[b0:b0 + n].contiguous(), H, W)
            assert _same(part, first[b0:b0 + n]), (n, b0)
    with _h().options(FR_BWD_CHUNKS=64, FR_BWD_CB=2):
        assert _same(dbwd(g, V, tri, ti, H, W), first)
    assert _same(dfwd(V, tri, ti, H, W), dfwd(V, tri, ti, H, W))


def test_a_nan_gradient_reaches_exactly_its_triangle(small_assets):
    sc = scene(small_assets, 3, 33, 40)
    g = sc["g"].copy()
    px = int(np.flatnonzero(sc["tind"][1] >= 0)[5])
    g[1, px] = np.nan
    ids = {int(sc["tri"][k, int(sc["tind"][1, px])]) for k in range(3)}
    clean = dbwd(_t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"]), 33, 40)
    got = dbwd(_t(g), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"]), 33, 40)
    assert _same(got[0], clean[0]) and _same(got[2], clean[2])                # faces 0 and 2 keep their bits
    R = RD.model(g, sc["V"], sc["tri"], sc["tind"], 33, 40)
    assert [F.bad for F in R.faces] == [False, True, False]
    nonfinite = ~np.isfinite(got[1].cpu().numpy())
    np.testing.assert_array_equal(nonfinite, R.dense(1, "nonfinite"))
    assert set(np.flatnonzero(nonfinite.any(axis=0)).tolist()) == ids and len(ids) == 3
    assert nonfinite[:, sorted(ids)].all()                                    # all three rows of the three vertices


# ---- Python surface ------------------------------------------------------------------------------------------------------------------------
class _Py:
    pass


@pytest.fixture(scope="module")
def py(small_assets):
    """the small mesh decoded at 64 x 64, two faces; random weights for every output"""
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
    s.P = _t(P)
    s.V = s.net.vertices_transform(s.P).detach()
    gen = torch.Generator().manual_seed(9)
    s.wn = torch.randn((s.B, s.S, s.S, 3), generator=gen).to(DEV)
    s.wd = torch.randn((s.B, s.S, s.S, 1), generator=gen).to(DEV)
    s.w7 = torch.randn((s.B, s.S, s.S, 7), generator=gen).to(DEV)
    s.im = torch.rand((s.B, s.S, s.S, 1), generator=gen).to(DEV)
    s.image = torch.zeros((s.B, s.S, s.S, 3), device=DEV)
    return s


def test_render_depth_depth_interp_flag(py):
    o, s = ops(), py

    def run(use_depth, use_normal, **kw):
        V = s.V.clone().requires_grad_(True)
        outs = o.render_depth(V, s.net.tri, s.net.vertex_code, s.image, **kw)
        loss = 0
        if use_depth:
            loss = loss + (outs[0].clamp_min(0) * s.wd).sum()
        if use_normal:
            loss = loss + (outs[2] * s.wn).sum()
        loss.backward()
        return [t.detach() for t in outs], V.grad
    outs0, g0 = run(True, False)
    outsF, gF = run(True, False, depth_interp=False)
    outs1, g1 = run(True, False, depth_interp=True)
    for a, b, c in zip(outs0[1:], outsF[1:], outs1[1:]):
        assert _same(a, b) and _same(a, c)                                    # outputs 2-4: the default call's bits
    assert _same(outs0[0], outsF[0]) and _same(g0, gF)                        # off: as before
    want = o.depth_interpolate(s.V, s.net.tri, outs0[3])
    assert _same(outs1[0], want) and not _same(outs1[0], outs0[0])
    assert not bool(_bits(g0[:, 0:2]).any())                                  # the flat depth: x and y rows exactly +0
    assert float(g1[:, 0].abs().max()) > 0 and float(g1[:, 1].abs().max()) > 0 and float(g1[:, 2].abs().max()) > 0
    # the node's gradient is depth_interpolate's own
    V = s.V.clone().requires_grad_(True)
    (o.depth_interpolate(V, s.net.tri, outs0[3]).clamp_min(0) * s.wd).sum().backward()
    assert _same(V.grad, g1)
    # with normal_grad as well: the two parts computed separately, one fp32 add per element
    _, gn = run(False, True, normal_grad=True)
    _, gboth = run(True, True, normal_grad=True, depth_interp=True)
    assert _same(gboth, g1 + gn)
    # texture_grad rides along; an output nobody used costs no backward
    tex = s.net.vertex_code.clone().requires_grad_(True)
    V = s.V.clone().requires_grad_(True)
    outs = o.render_depth(V, s.net.tri, tex, s.image, depth_interp=True, texture_grad=True)
    (outs[1] * s.wn).sum().backward()
    assert V.grad is None and float(tex.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        o.depth_interpolate(s.V, s.net.tri, outs0[3].clone().requires_grad_(True))


def test_coarse_net_input_depth_interp_flag(py):
    s, net = py, py.net

    def run(**kw):
        V = s.V.clone().requires_grad_(True)
        ni, di = net.coarse_net_input(V, im_gray=s.im, **kw)
        ((ni * s.w7).sum() + (di * s.wd).sum()).backward()
        return ni.detach(), di.detach(), V.grad
    off, on = run(), run(depth_interp=True)
    assert _same(run(depth_interp=False)[1], off[1])
    assert _same(on[0], off[0])                                               # net_input: bit for bit, the mask channel included
    assert not _same(on[1], off[1])
    tind = ops().render_depth(s.V, net.tri, net.vertex_code, s.image)[3]
    assert _same(on[1], ops().depth_interpolate(s.V, net.tri, tind).clamp_min(1e-6))
    assert not bool(_bits(off[2][:, 0:2]).any()) and float(on[2][:, 0].abs().max()) > 0 and float(on[2][:, 1].abs().max()) > 0
    # the unfused route agrees
    pncc, normal, mask, di = net.rendering_layer(s.V, net.tri, net.vertex_code, im_gray=s.im, depth_interp=True)
    assert _same(di, on[1]) and _same(mask, off[0][..., 0:1])


def test_decode_rendering_layer_depth_interp_turns_the_head(py):
    s, net = py, py.net

    def run(**kw):
        p = s.P.clone().requires_grad_(True)
        ni, di = net.decode_rendering_layer(p, im_gray=s.im, pose_grad=True, **kw)
        (di * s.wd).sum().backward()
        return ni.detach(), di.detach(), p.grad, type(di.grad_fn).__name__
    on, off = run(depth_interp=True), run()
    assert _same(on[0], off[0]) and not _same(on[1], off[1])
    assert off[3].startswith("_DecodeRenderingLayer") and not on[3].startswith("_DecodeRenderingLayer")   # the two-step route
    ang = on[2][:, 0:3]
    assert bool(torch.isfinite(on[2]).all()) and bool((ang != 0).all())
    assert not _same(ang, off[2][:, 0:3])


def test_face_recon_model_depth_interp_trains(small_assets):
    netm, Ls, cn = net_mod(), pkg("nets.losses"), pkg("nets.coarse_net")
    B, S = 2, 64
    face = netm.FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S)
    face.init_pred_params[..., 6] = 3e-4
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    label = torch.as_tensor(pkg("utils.synth").sample_params_batch(B, im_size=S, n_shape=face.ndim_shape, n_exp=face.ndim_exp,
                                                                   beta=0.7, seed=5), device=DEV)
    maps = {}
    for flag in (False, True):
        torch.manual_seed(3)
        model = cn.FaceReconModel(face, nIter=1, fine=True, pose_grad=True, **({"depth_interp": True} if flag else {})).to(DEV).train()
        out = model(im)
        maps[flag] = out["coarse_depth_map"].detach()
        L = Ls.get_loss(face, out["pred_params"], label, im, out["vertices_proj"], out["coarse_depth_map"], out["pred_depth_map"])
        L["total_loss"].backward()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert bool(torch.isfinite(L["total_loss"])) and grads and all(bool(torch.isfinite(g).all()) for g in grads)
        assert float(model.coarse.iters[0].fc.weight.grad.abs().max()) > 0
    assert maps[True].shape == maps[False].shape and not _same(maps[True], maps[False])
    assert bool(torch.isfinite(maps[True]).all())


# ---- threads ------------------------------------------------------------------------------------------------------------------------------
def test_four_threads_four_streams(small_assets):
    """four host threads, each forward and backward on a stream of its own with a workspace per call, at 33 x 40: the serial bits
    (the pattern of tests/test_fine_losses_gpu.py)"""
    sc = scene(small_assets, 3, 33, 40)
    H, W = 33, 40
    g, V, tri, ti = _t(sc["g"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    jobs = [(g * (i + 1), V + 0.01 * i) for i in range(4)]
    refs = [(dfwd(v, tri, ti, H, W), dbwd(gi, v, tri, ti, H, W)) for gi, v in jobs]
    streams = [torch.cuda.Stream(device=DEV) for _ in jobs]
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(jobs))

    def worker(i):
        bad = []
        barrier.wait(timeout=60)
        gi, v = jobs[i]
        with torch.cuda.stream(streams[i]):
            for it in range(10):
                d = dfwd(v, tri, ti, H, W, stream=streams[i])
                vg = dbwd(gi, v, tri, ti, H, W, stream=streams[i])
                streams[i].synchronize()
                if not (_same(d, refs[i][0]) and _same(vg, refs[i][1])):
                    bad.append("thread %d iteration %d" % (i, it))
        return bad

    ex = ThreadPoolExecutor(max_workers=len(jobs))
    try:
        futs = [ex.submit(worker, i) for i in range(len(jobs))]
        bad = sum((f.result(timeout=180) for f in futs), [])
    finally:
        ex.shutdown(wait=False, cancel_futures=True)
    assert not bad, bad[:10]
