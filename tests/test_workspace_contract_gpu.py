"""GPU: the three promises include/fr_hotpath.h makes about every caller-owned workspace, state, packed basis and image -- the call
needs none of the buffer cleared, writes nothing outside the stated bytes, and the stated alignment is enough -- held for every
(entry point, buffer) pair of tests/workspace_cases.py at its "even" and its "ragged" shape.

The buffer is the middle of one uint8 tensor, [4096 guard | nbytes | 4096 guard], with nbytes exactly the size function's answer (the
byte count the call is given) and a start that is a multiple of the stated alignment and of no larger power of two.  Each case runs
under four fills of the middle -- Z zeros, F 0xFF bytes (NaN in fp32 and fp64, -1 in signed integers, the maximum in unsigned
counters), H 0x7F bytes (a huge finite float, a huge positive integer) and L, leftovers: what the call that shares the buffer's pool
kind (or the same entry point at a larger shape) left there, not refilled -- and then
  a. every output of F, H and L equals Z's bit for bit;
  b. both guards still hold their fill (another byte under each of the four, so a read past either end shows under a.), and
     under L the bytes between the small nbytes and the end of the larger buffer are what they were just before the small call;
  c. Z's outputs are finite and not all zero, at least 30 % of the pixels are covered, every solve reports ok = 1 on every unit;
  d. Z's result passes the existing reference check of its kernel's own test module, with that module's bound (no tolerance is
     introduced here).
Entries with no (raw call, shape-free reference check) pair to anchor to, held by a. - c. alone: rendering_layer_forward and
rendering_layer_forward_phases (tests/test_fused_layer_gpu.py goes through the operator surface), decode_pose_backward (its module has
no check outside its test functions), decode_render_backward and decode_render_backward_pose (tests/test_decode_layer_gpu.py takes
its tolerance from a list inside the test function), the three albedo_lse_forward cases with the albedo basis's consumer
(tests/test_albedo_lse_gpu.py judges them inside test functions; the basis itself is anchored), and landmark_forward /
landmark_backward behind the basis image (the image itself is anchored).

The second half runs every op of the Python surface that takes a hold on a pooled buffer (_lib.StreamBuffers) over a pool whose
buffers were filled with 0xFF behind its back, and again after the op that shares its pool kind has used the buffer at a larger
shape."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import pkg
import workspace_cases as WC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@contextlib.contextmanager
def _a_device_fault_ends_the_session():
    """nothing more is launched on a device that has faulted: every later test of the process would only report the dead context"""
    try:
        yield
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("device fault: %s" % str(e).splitlines()[0], returncode=3)
        raise


def _np(outs):
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in outs.items()}


def _run_filled(c, shape, tag, fill):
    """-> (outputs as the call returned them, guard damage or None)"""
    n, gb = c.nbytes(shape), WC.GUARD_BYTES[tag]
    whole, off = WC.place(n, c.align, guard_byte=gb)
    whole[off:off + n] = fill
    outs = c.run(shape, whole[off:off + n])
    torch.cuda.synchronize()
    return outs, WC.guard_damage(whole, off, n, gb)


def _run_leftovers(c, shape):
    """-> (outputs, guard damage or None, True if the bytes behind the small buffer survived the small call)"""
    oc, oshape = (WC.CASES[c.other[0]], c.other[1]) if c.other is not None else (c, "large")
    n, nother = c.nbytes(shape), oc.nbytes(oshape)
    nbig = max(n, nother)
    whole, off = WC.place(nbig, max(c.align, oc.align), guard_byte=WC.GUARD_BYTES["L"])
    oc.run(oshape, whole[off:off + nother])
    before = whole[off + n:off + nbig].clone()
    outs = c.run(shape, whole[off:off + n])
    torch.cuda.synchronize()
    return outs, WC.guard_damage(whole, off, nbig, WC.GUARD_BYTES["L"]), bool(torch.equal(before, whole[off + n:off + nbig]))


@pytest.mark.parametrize("shape", WC.SHAPES)
@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_buffer_contract(name, shape):
    with _a_device_fault_ends_the_session():
        _buffer_contract(WC.CASES[name], shape)


def _buffer_contract(c, shape):
    raw, damage = _run_filled(c, shape, *WC.FILLS[0])
    z = _np(raw)
    assert damage is None, "Z: " + damage
    # c. not vacuous
    for k, v in z.items():
        assert v.size and np.isfinite(v.astype(np.float64)).all(), "%s is not finite" % k
        assert v.any(), "%s is all zero" % k
    if c.cover is not None:
        assert c.cover(shape) >= 0.30, c.cover(shape)
    if "tri_ind" in z:                                                       # a render: the GPU's own plane, not the reference's
        assert (z["tri_ind"] >= 0).mean() >= 0.30, float((z["tri_ind"] >= 0).mean())
    for k in c.ok:
        assert (z[k] == 1).all(), (k, z[k])
    # d. anchored
    if c.anchor is not None:
        c.anchor(shape, raw)
    # a. no read before write, b. no write outside
    for tag, fill in WC.FILLS[1:]:
        outs, damage = _run_filled(c, shape, tag, fill)
        assert damage is None, "%s: %s" % (tag, damage)
        diff = WC.bit_difference(_np(outs), z)
        assert diff is None, "%s (0x%02X bytes) against zeros: %s" % (tag, fill, diff)
    outs, damage, tail_kept = _run_leftovers(c, shape)
    assert damage is None, "L: " + damage
    assert tail_kept, "L: the call wrote behind its stated bytes, into the larger buffer's tail"
    diff = WC.bit_difference(_np(outs), z)
    assert diff is None, "L (leftovers of %s) against zeros: %s" % (c.other or "the same call at the large shape", diff)


# ---- the pooled path: every op of the Python surface that takes a hold ------------------------------------------------------------------
def _ops():
    return pkg("rendering_layer.ops")


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.array(a, dtype), device=DEV)                    # (a copy: the shared inputs are read-only arrays)


def _poison(pools):
    """fills every pooled buffer with 0xFF under its entry's lock and clears the entry's note (what R2 does on replacement)
    -> the kinds found"""
    kinds = set()
    for pool in pools:
        for key, ent in pool.snapshot().items():
            with ent.lock:
                ent.buf.fill_(0xFF)
                ent.note = None
            kinds.add(key[0])
    return kinds


def _pooled(op, bigger, kinds, extra_pools=()):
    with _a_device_fault_ends_the_session():
        _pooled_body(op, bigger, kinds, extra_pools)


def _pooled_body(op, bigger, kinds, extra_pools):
    o = _ops()
    pools = [o._RENDER_POOL, o._KINDS_POOL] + list(extra_pools)
    o.clear_workspace_cache()
    for p in extra_pools:
        p.clear()
    first = _np(op())
    torch.cuda.synchronize()
    for k, v in first.items():
        assert np.isfinite(v.astype(np.float64)).all() and v.any(), k
    found = _poison(pools)
    assert set(kinds) <= found, (kinds, found)
    second = _np(op())
    diff = WC.bit_difference(second, first)
    assert diff is None, "after the pool's buffers were filled with 0xFF: " + diff
    bigger()
    third = _np(op())
    torch.cuda.synchronize()
    diff = WC.bit_difference(third, first)
    assert diff is None, "after the op that shares the pool kind ran at a larger shape: " + diff


def _render_inputs(shape):
    sc = WC.scene(shape)
    return _t(sc["V"]), _t(sc["tri"]), _t(sc["tex"]), _t(sc["im"]), torch.zeros((sc["B"], sc["H"], sc["W"], 3), device=DEV)


def test_pooled_render():
    o = _ops()
    V, tri, tex, im, image = _render_inputs("ragged")
    Vb, trib, texb, imb, _ = _render_inputs("large")

    def op():
        return dict(zip(("depth", "tex_img", "normal", "tri_ind"), o.render_depth(V, tri, tex, image)))

    _pooled(op, lambda: o.rendering_layer_fused(Vb, trib, texb, imb), ["render"])


def _layer_op(shape, pose_grad):
    o = _ops()
    rig = WC._lrig(shape)
    P0, im = _t(WC.layer_params(shape)), _t(WC.scene(shape)["im"])
    g = torch.Generator().manual_seed(3)
    gn, gd = torch.randn((P0.shape[0],) + tuple(im.shape[1:3]) + (7,), generator=g).to(DEV), torch.randn(im.shape, generator=g).to(DEV)

    def op():
        P = P0.clone().requires_grad_(True)
        net_in, depth_img = o.decode_rendering_layer(P, None, im, rig.net.tri, rig.net.vertex_code, rig.net._basis, rig.im_size,
                                                     pose_grad=pose_grad)
        ((net_in * gn).sum() + (depth_img * gd).sum()).backward()
        return {"net_input": net_in.detach(), "depth_img": depth_img.detach(), "grad_params": P.grad}
    return op


def test_pooled_hand_and_bwd():
    _pooled(_layer_op("ragged", False), _layer_op("large", True), ["render", "hand", "bwd"])


def test_pooled_coverage_bwd():
    o = _ops()

    def make(shape):
        sc = WC.scene(shape, True)
        V0, tri, ti, g = _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"]), _t(sc["g1"])

        def op():
            V = V0.clone().requires_grad_(True)
            cov = o.soft_coverage(V, tri, ti)
            (cov * g.reshape(cov.shape)).sum().backward()
            return {"cov": cov.detach(), "vertex_grad": V.grad}
        return op
    _pooled(make("ragged"), make("large"), ["coverage_bwd"])


def test_pooled_fine_losses():
    o = _ops()

    def make(shape):
        z, c = (_t(a) for a in WC._fine_in(shape))
        return lambda: dict(zip(("fidelity", "smoothness"), o.fine_depth_losses(z, c)))
    _pooled(make("ragged"), make("large"), ["fine_losses"])


def test_pooled_sfs_lighting():
    o = _ops()

    def make(shape):
        d = {k: _t(v) for k, v in WC.sfs_inputs(shape)[0].items()}
        return lambda: {"lighting": o.sfs_lighting(d["abedo"], d["normal"], d["im_gray"])}
    _pooled(make("ragged"), make("large"), ["sfs_lighting"])


def test_pooled_albedo_lse():
    o = _ops()

    def make(shape, K):
        a = WC._albedo_dev(shape, K)
        return lambda: dict(zip(("alpha", "stats"), o.albedo_lse(a["basis"], a["tri_ind"], a["lighting"], a["normal"], a["abedo"],
                                                                 a["im_gray"])))
    _pooled(make("ragged", 15), make("large", 9), ["albedo_lse"])


def test_pooled_synth_texture_backward():
    o = _ops()

    def make(shape):
        B, N, K = WC._synth_args(shape)
        rs = np.random.RandomState(N)
        pc, g = _t(0.05 * rs.standard_normal((3 * N, K))), _t(rs.standard_normal((B, 3, N)))
        return lambda: {"grad_alpha": o.synth_texture_backward(pc, g)}
    _pooled(make("ragged"), make("large"), ["synth_texture_backward"])


@pytest.mark.parametrize("rgb", [False, True], ids=["photo_loss", "photo_loss_rgb"])
def test_pooled_photo_loss(rgb):
    import ref_photo_loss as RP
    import ref_photo_rgb as RC
    o = _ops()

    def make(shape, colour):
        B, H, W = WC._bhw(shape)
        p = [_t(a) for a in (RC.hand_planes_rgb if colour else RP.hand_planes)(B, H, W, seed=5 + H)]
        fn = o.photo_loss_rgb if colour else o.photo_loss
        return lambda: dict(zip(("sse", "count"), fn(p[0], p[1], p[2], p[3], p[4], p[5], 1.75, -0.125)))
    _pooled(make("ragged", rgb), make("large", rgb), ["photo_loss_rgb" if rgb else "photo_loss"])


@pytest.mark.parametrize("which", ["light", "albedo"])
def test_pooled_photo_solve_rgb(which):
    o = _ops()

    def make(shape, K, what):
        s = WC.solve_inputs(shape, K)
        basis, ti, n, tg, tex, light = (_t(s["basis"], np.float64), _t(s["tri_ind"]), _t(s["normal"]), _t(s["target"]), _t(s["tex"]),
                                        _t(s["light"]))
        if what == "light":
            return lambda: dict(zip(("light", "stats"), o.photo_light_lse_rgb(tex, n, ti, tg)))
        return lambda: dict(zip(("alpha", "stats"), o.albedo_lse_rgb(basis, ti, n, light, tg, ridge=1e-6)))
    _pooled(make("ragged", 15, which), make("large", 9, "albedo" if which == "light" else "light"), ["photo_solve_rgb"])


def test_pooled_landmark_solve():
    o = _ops()

    def make(shape):
        c = WC._lm_case(shape)
        A = c["A"]
        lb = o.landmark_basis(_t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"]), c["idx"])
        P, target, ridge, center, damp = _t(c["P"]), _t(c["target"]), _t(c["ridge"]), _t(c["center"]), _t(c["damp"], np.float64)
        return lambda: dict(zip(("delta", "cost", "ok"), o.landmark_solve_step(P, lb, target, ridge=ridge, center=center, damp=damp,
                                                                               fit_pose=False, fit_coef=True)))
    _pooled(make("ragged"), make("large"), ["landmark_solve"])


def test_pooled_network_backward_workspace():
    """nets/network.py's decode backward: PackedBasis.backward_workspace's own pool.  Its kind is the byte count, so the entry points
    that share a buffer are the two fused backwards at one batch size (from the forward's output, and from mu); a larger batch takes
    a buffer of its own, and is run as well"""
    net = WC._brig("ragged").net
    basis = net._basis
    P0, _, _, G0 = WC.decode_inputs("ragged")
    Pt, Gt = _t(P0), _t(G0)

    def op(from_mu=False, reps=1):
        basis.backward_from_mu = from_mu
        try:
            P = Pt.repeat(reps, 1).requires_grad_(True)
            net.vertices_transform(P).backward(Gt.repeat(reps, 1, 1))
            return {"grad_params": P.grad}
        finally:
            basis.backward_from_mu = False
    nws = WC.lib().fr_decode_backward_workspace_bytes(Pt.shape[0], *WC.asset_dims("ragged"))
    _pooled(op, lambda: (op(from_mu=True), op(reps=2)), [nws], extra_pools=[basis._bwd_ws])
