"""GPU: the fine-depth losses (csrc/fr_fine_losses.hip; ops.fine_depth_losses; get_loss(fine_fused=True)).

  1  the forward: the tile partials, the two state sums and the two fp32 outputs bit for bit against the model
     (tests/ref_fine_losses.py), and each sum within n 2^-53 sum |term| of its fsum value whatever the association;
  2  the backward: grad_pred and grad_coarse bit for bit, at three (g_f, g_s) pairs, each scalar also NULL, grad_coarse also NULL;
  3  two runs into differently pre-filled buffers;
  4  a NaN in one face;
  5  the operator against the raw calls, and the objective's flag on and off;
  6  two host threads on two streams.
The shapes come from the kernels' own tile (fr_debug_fine_losses_geom), not from a re-derivation.  Outputs are pre-filled with NaN,
the state with 0xFF bytes."""
import ctypes
import functools
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import assert_bits_equal
import ref_fine_losses as RF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53
CASES = [(s, False) for s in RF.shapes()] + [((3, 33, 67), True), ((2, 200, 200), True)]


def _cid(case):
    return RF.case_id(case[0]) + ("-wide" if case[1] else "")


def _h():
    return pkg("_lib")


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_bits64_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (_bits64(got) != _bits64(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d float64 values differ in their bits, first at %s: got %r want %r" % (
        what, int(bad.sum()), got.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def raw_forward(z, c, fill=0xFF, stream=None, state=None):
    """fr_fine_losses_forward through the raw C ABI -> (fidelity fp32, smoothness fp32, state as float64 [2 + 2P])"""
    h = _h()
    L = h.lib()
    B, H, W = z.shape
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)
    zt, ct = torch.tensor(z, device=DEV), torch.tensor(c, device=DEV)      # (the shared inputs are read-only: copies)
    nst = L.fr_fine_losses_state_bytes(B, H, W)
    g = RF.geom(B, H, W)
    assert nst == (2 + 2 * g[3] * g[4] * B) * 8
    if state is None:
        state = torch.full((nst,), fill, dtype=torch.uint8, device=DEV)
    assert state.dtype == torch.uint8 and state.numel() == nst
    out = torch.full((2,), float("nan") if fill else 0.0, dtype=torch.float32, device=DEV)
    rc = L.fr_fine_losses_forward(h.ptr(zt), h.ptr(ct), B, H, W, h.ptr(out[0:]), h.ptr(out[1:]), h.ptr(state), nst, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[0], o[1], state.view(torch.float64).cpu().numpy()


def raw_backward(z, c, g_f, g_s, want_coarse=True, fill=float("nan"), stream=None):
    """fr_fine_losses_backward through the raw C ABI -> (grad_pred, grad_coarse or None); g_f / g_s None = a NULL pointer"""
    h = _h()
    L = h.lib()
    B, H, W = z.shape
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)
    zt, ct = torch.tensor(z, device=DEV), torch.tensor(c, device=DEV)      # (the shared inputs are read-only: copies)
    gf = torch.tensor(g_f, dtype=torch.float32, device=DEV) if g_f is not None else None
    gs = torch.tensor(g_s, dtype=torch.float32, device=DEV) if g_s is not None else None
    gp = torch.full((B, H, W), fill, dtype=torch.float32, device=DEV)
    gc = torch.full((B, H, W), fill, dtype=torch.float32, device=DEV) if want_coarse else None
    rc = L.fr_fine_losses_backward(h.ptr(gf), h.ptr(gs), h.ptr(zt), h.ptr(ct), B, H, W, h.ptr(gp), h.ptr(gc), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return gp.cpu().numpy(), (gc.cpu().numpy() if want_coarse else None)


@functools.lru_cache(maxsize=None)
def rig(case):
    """(z, c, planted, the model's forward) of a case: computed once, shared by every test, never written"""
    (B, H, W), wide = case
    z, c, planted = RF.inputs(B, H, W, wide=wide)
    for a in (z, c, planted):
        a.setflags(write=False)
    return z, c, planted, RF.forward(z, c)


# ---- 1: the forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_forward_bits_and_bound(case):
    z, c, planted, want = rig(case)
    n = z.size
    fid, sm, state = raw_forward(z, c)
    P = want["part_f"].size
    assert state.size == 2 + 2 * P
    assert_bits64_equal(state[2:2 + P], want["part_f"], "fidelity partials")
    assert_bits64_equal(state[2 + P:], want["part_s"], "smoothness partials")
    assert_bits64_equal(state[:2], [want["S_f"], want["S_s"]], "S_f, S_s")
    assert_bits_equal(fid, want["fidelity"], "fidelity")
    assert_bits_equal(sm, want["smoothness"], "smoothness")
    tf, ts = RF.terms(z, c)
    for name, S, exact, tot in (("S_f", state[0], want["fsum_f"], float(tf.sum())), ("S_s", state[1], want["fsum_s"], float(ts.sum()))):
        bound = n * U * tot
        print("%s %s: %.17g, fsum %.17g, |difference| / (n u sum|term|) = %.3g" % (_cid(case), name, S, exact,
                                                                                   abs(S - exact) / max(bound, 1e-300)))
        assert abs(S - exact) <= bound
    share = float((RF.laplacian(z) == 0).sum()) / n
    print("%s: share of pixels with L == 0 on the model: %.3f" % (_cid(case), share))
    assert (RF.laplacian(z)[planted] == 0).all()
    if z.shape[0] == 3:
        assert share >= 0.1                  # the s(0) = 0 branch is exercised: the all-zero face alone is a third
    # 3: a second run into a state of zeros and outputs of zeros
    fid2, sm2, state2 = raw_forward(z, c, fill=0x00)
    assert_bits64_equal(state2, state, "second run's state")
    assert_bits_equal(fid2, fid, "second run's fidelity")
    assert_bits_equal(sm2, sm, "second run's smoothness")


# ---- 2: the backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_backward_bits(case):
    z, c, _, _ = rig(case)
    for g_f, g_s in RF.GRADS:
        want_p, want_c = RF.backward(z, c, g_f, g_s)
        gp, gc = raw_backward(z, c, g_f, g_s)
        assert_bits_equal(gp, want_p, "grad_pred at (%g, %g)" % (g_f, g_s))
        assert_bits_equal(gc, want_c, "grad_coarse at (%g, %g)" % (g_f, g_s))
    g_f, g_s = RF.GRADS[1]
    want_p, want_c = RF.backward(z, c, g_f, g_s)
    # 3: another pre-fill, and grad_coarse not wanted
    gp, gc = raw_backward(z, c, g_f, g_s, want_coarse=False, fill=0.0)
    assert gc is None
    assert_bits_equal(gp, want_p, "grad_pred without grad_coarse, into zeros")
    # each scalar NULL: that term is absent
    for gf_, gs_ in ((None, g_s), (g_f, None), (None, None)):
        wp, wc = RF.backward(z, c, gf_, gs_)
        gp, gc = raw_backward(z, c, gf_, gs_)
        assert_bits_equal(gp, wp, "grad_pred at (%r, %r)" % (gf_, gs_))
        assert_bits_equal(gc, wc, "grad_coarse at (%r, %r)" % (gf_, gs_))
    if z.shape[0] == 3:
        assert not want_c[2].any()                                   # c == z on face 2: a zero fidelity gradient there
    # the zero-L regions: where every sign of a pixel's ring is zero, the smoothness part is exactly absent
    T = RF.T_plane(z)
    only_s, _ = raw_backward(z, c, None, 1.0)
    assert_bits_equal(only_s, T.astype(np.float32), "T itself")


# ---- 4: non-finite --------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_face():
    B, H, W = 3, 33, 67
    z = RF.inputs(B, H, W, seed=3)[0].copy()
    z[1] = RF.inputs(B, H, W, seed=4)[0][0]                          # three random faces
    c = RF.inputs(B, H, W, seed=3)[1]
    clean_p, clean_c = raw_backward(z, c, 1.0, 1.0)
    assert np.isfinite(clean_p).all() and np.isfinite(clean_c).all()
    bad = z.copy()
    bad[1, 16, 32] = np.nan                                          # on a tile corner: its ring lies in four tiles
    gp, gc = raw_backward(bad, c, 1.0, 1.0)
    assert_bits_equal(gp[[0, 2]], clean_p[[0, 2]], "grad_pred of the other faces")
    assert_bits_equal(gc[[0, 2]], clean_c[[0, 2]], "grad_coarse of the other faces")
    assert np.argwhere(~np.isfinite(gp)).tolist() == [[1, 16, 32]]
    assert np.argwhere(~np.isfinite(gc)).tolist() == [[1, 16, 32]]
    changed = np.argwhere(gp[1].view(np.uint32) != clean_p[1].view(np.uint32))
    assert len(changed) > 1 and (np.abs(changed - np.array([16, 32])).max(axis=1) <= 2).all()
    want_p, want_c = RF.backward(bad, c, 1.0, 1.0)
    assert_bits_equal(gp, want_p, "grad_pred with the NaN")
    assert_bits_equal(gc, want_c, "grad_coarse with the NaN")
    fid, sm, _ = raw_forward(bad, c)
    assert not np.isfinite(fid) and not np.isfinite(sm)
    fid, sm, _ = raw_forward(z, c)
    assert np.isfinite(fid) and np.isfinite(sm)


# ---- 5: the operator and the objective ------------------------------------------------------------------------------------------------
def test_operator_equals_the_raw_calls():
    ops = pkg("rendering_layer.ops")
    case = ((3, 33, 67), True)
    z, c, _, _ = rig(case)
    fid, sm, _ = raw_forward(z, c)
    for chan in (True, False):                                       # [B,H,W,1] as the objective passes it, and [B,H,W]
        shape = z.shape + (1,) if chan else z.shape
        zt = torch.tensor(z, device=DEV).reshape(shape).requires_grad_(True)
        ct = torch.tensor(c, device=DEV).reshape(shape).requires_grad_(True)
        f, s = ops.fine_depth_losses(zt, ct)
        assert f.dim() == 0 and s.dim() == 0 and f.dtype == torch.float32 and s.dtype == torch.float32
        assert_bits_equal(f.detach().cpu().numpy(), fid, "operator fidelity")
        assert_bits_equal(s.detach().cpu().numpy(), sm, "operator smoothness")
        (f * -0.37 + s * 1e-3).backward()
        gp, gc = raw_backward(z, c, -0.37, 1e-3)
        assert zt.grad.shape == zt.shape and ct.grad.shape == ct.shape
        assert_bits_equal(zt.grad.cpu().numpy().reshape(z.shape), gp, "operator grad_pred")
        assert_bits_equal(ct.grad.cpu().numpy().reshape(z.shape), gc, "operator grad_coarse")
        with pytest.raises(RuntimeError):
            (f * -0.37 + s * 1e-3).backward()                        # a second backward through the same node
    # one output unused: its gradient is NULL, its term absent; a constant coarse gets no gradient
    zt = torch.tensor(z, device=DEV).requires_grad_(True)
    ct = torch.tensor(c, device=DEV)
    f, s = ops.fine_depth_losses(zt, ct)
    s.backward()
    assert_bits_equal(zt.grad.cpu().numpy(), raw_backward(z, c, None, 1.0)[0], "smoothness alone")
    zt.grad = None
    f, s = ops.fine_depth_losses(zt, ct)
    f.backward()
    assert_bits_equal(zt.grad.cpu().numpy(), raw_backward(z, c, 1.0, None)[0], "fidelity alone")
    # two forwards in flight before their backwards: nothing of the first is lost to the second
    z1 = torch.tensor(z, device=DEV).requires_grad_(True)
    z2 = torch.as_tensor(z[::-1].copy(), device=DEV).requires_grad_(True)
    f1, s1 = ops.fine_depth_losses(z1, ct)
    f2, s2 = ops.fine_depth_losses(z2, ct)
    (f1 + s1).backward()
    (f2 + s2).backward()
    assert_bits_equal(f1.detach().cpu().numpy(), fid, "first of two in flight")
    assert_bits_equal(z1.grad.cpu().numpy(), raw_backward(z, c, 1.0, 1.0)[0], "first of two in flight, gradient")
    assert_bits_equal(z2.grad.cpu().numpy(), raw_backward(z[::-1].copy(), c, 1.0, 1.0)[0], "second of two in flight, gradient")
    # an empty batch takes the torch route
    e = torch.zeros((0, 5, 5, 1), device=DEV)
    f, s = ops.fine_depth_losses(e, e)
    assert f.dim() == 0 and s.dim() == 0 and float(s) == 0.0


def _same(a, b):
    return bool((a.detach().view(torch.int32) == b.detach().view(torch.int32)).all())


def test_get_loss_flag_on_and_off(small_assets):
    """the objective on the small synthetic assets with fine_fused on and off: the two terms, the total and the gradients reaching
    pred_depth_map and the CoarseNet parameters to the 1e-5 relative the project uses for its fp32 product route
    (tests/test_losses_gpu.py); the other four entries bit-equal"""
    netm, Ls, cn = pkg("nets.network"), pkg("nets.losses"), pkg("nets.coarse_net")
    A = small_assets
    B, S = 3, 40
    face = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
    torch.manual_seed(11)
    model = cn.FaceReconModel(face, nIter=1, fine=False).to(DEV).train()
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    noise = 0.05 * torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(2)).to(DEV)
    label = torch.as_tensor(pkg("utils.synth").sample_params_batch(B, im_size=S, n_shape=face.ndim_shape, n_exp=face.ndim_exp,
                                                                   beta=0.7, seed=5), device=DEV)
    with pytest.raises(ValueError):
        Ls.get_loss(face, label, label, im, None, None, None, fine_fused=True)

    # ONE forward of the net, two objectives on its tensors: the other terms then see the same bits on both routes
    out = model(im)
    # a stand-in for FineNet that keeps both paths of the fidelity gradient alive: into pred_depth_map and into the coarse map
    pd = 0.9 * out["coarse_depth_map"] + noise
    names, params = zip(*model.named_parameters())

    def run(**kw):
        L = Ls.get_loss(face, out["pred_params"], label, im, out["vertices_proj"], out["coarse_depth_map"], pd, **kw)
        g = torch.autograd.grad(L["total_loss"], (pd,) + params, retain_graph=True, allow_unused=True)
        torch.cuda.synchronize()
        return L, g[0], {n: t for n, t in zip(names, g[1:]) if t is not None}

    off, gpd_off, g_off = run()
    on, gpd_on, g_on = run(fine_fused=True)
    for k in ("fidelity_loss", "smoothness_loss", "total_loss"):
        a, b = float(on[k].detach()), float(off[k].detach())
        print("%s: fused %.9g, torch %.9g, relative difference %.3g" % (k, a, b, abs(a - b) / abs(b)))
        assert on[k].dim() == 0 and on[k].dtype == torch.float32
        assert abs(a - b) <= 1e-5 * abs(b)
    for k in ("pose_loss", "geometry_loss", "spherical_harmonics_loss"):
        assert _same(on[k], off[k]), k
    assert set(on) == set(off) and len(on) == 6
    rel = float((gpd_on - gpd_off).abs().max() / gpd_off.abs().max())
    print("gradient reaching pred_depth_map: largest difference / largest entry = %.3g" % rel)
    assert float(gpd_off.abs().max()) > 0 and rel <= 1e-5
    assert set(g_on) == set(g_off) and len(g_on) > 0
    worst = 0.0
    for n in g_off:
        scale = float(g_off[n].abs().max())
        if scale == 0.0:
            assert not g_on[n].any(), n
            continue
        worst = max(worst, float((g_on[n] - g_off[n]).abs().max()) / scale)
    print("gradients reaching %d parameter tensors: largest difference / largest entry of its tensor = %.3g" % (len(g_off), worst))
    assert worst <= 1e-5
    # beside the other flags
    assert max(float(g.abs().max()) for g in g_off.values()) > 0
    both = Ls.get_loss(face, label, label, im, out["vertices_proj"].detach(), torch.zeros((B, S, S, 1), device=DEV),
                       torch.ones((B, S, S, 1), device=DEV), fine_fused=True, sfs_fused=True, geometry_gram=True, sfs_fine=True)
    assert float(both["fidelity_loss"]) == 1.0


# ---- 6: threads -----------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams():
    """two host threads, a stream and a state each: the single-thread bits (the pattern of tests/test_geometry_gram_gpu.py)"""
    jobs = [rig(((3, 33, 67), True))[:2], rig(((2, 200, 200), False))[:2]]
    grads = [(1.0, 1.0), (-0.37, 1e-3)]
    refs = [(raw_forward(z, c), raw_backward(z, c, *g)) for (z, c), g in zip(jobs, grads)]
    streams = [torch.cuda.Stream(device=DEV) for _ in jobs]
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(jobs))

    def worker(i):
        bad = []
        barrier.wait(timeout=60)
        (z, c), g = jobs[i], grads[i]
        with torch.cuda.stream(streams[i]):
            for it in range(10):
                fid, sm, state = raw_forward(z, c, stream=streams[i])
                gp, gc = raw_backward(z, c, *g, stream=streams[i])
                (rf, rs, rstate), (rp, rc) = refs[i]
                same = (fid.view(np.uint32) == rf.view(np.uint32) and sm.view(np.uint32) == rs.view(np.uint32)
                        and np.array_equal(_bits64(state), _bits64(rstate)) and np.array_equal(gp.view(np.uint32), rp.view(np.uint32))
                        and np.array_equal(gc.view(np.uint32), rc.view(np.uint32)))
                if not same:
                    bad.append("thread %d iteration %d" % (i, it))
        return bad

    ex = ThreadPoolExecutor(max_workers=len(jobs))
    try:
        futs = [ex.submit(worker, i) for i in range(len(jobs))]
        bad = sum((f.result(timeout=180) for f in futs), [])
    finally:
        ex.shutdown(wait=False, cancel_futures=True)
    assert not bad, bad[:10]
