"""GPU: the photometric loss (csrc/fr_photo.hip; rendering_layer.ops.photo_loss, nets.losses.photometric_loss) and the albedo
blend's adjoint (fr_synth_texture_backward; ops.synth_texture as an autograd node).  The forward's six sums, grad_tex_img, grad_light
and the blend's adjoint are held to the numpy model of tests/ref_photo_loss.py bit for bit; grad_normal within the header's bound
(the device's float64 division and square root are not assumed to round as the host's); the loss is the shader's image to the bit;
faces are independent; calls are reproducible across streams and host threads; the chain through the public operators is the hand
composition of its links; the callers run as programs."""
import ctypes
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
from gpu_util import assert_bits_equal, net_mod, ops
import ref_photo_loss as RP
from raw_calls import GAIN, OFFSET, PhotoCall as Call, assert_f64_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
# one partial tile; two full tiles plus 49 pixels; sixteen full tiles; 257 tiles: one more than the finish workgroup's 256 threads, so
# thread 0 chains two partials
SHAPES = [(1, 5, 6), (3, 33, 17), (2, 64, 64), (1, 257, 256)]
LIGHT = ((0.3, 0.7), (-0.4, 0.4), (-0.4, 0.4), (0.2, 0.9))


def _dev():
    return torch.device("cuda:0")


def _cpu(t):
    return t.detach().cpu().numpy()


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _grad_up(B):
    return np.array([1.0, -0.75, 2.5])[:B]


@pytest.fixture(scope="module")
def cases():
    """the hand planes of every shape and their model values, computed once"""
    out = {}
    for B, H, W in SHAPES:
        planes = RP.hand_planes(B, H, W, seed=(H * W + B) % 65792)      # (the largest shape takes seed 1: its planes reach s < 0)
        for weighted in (False, True):
            w = planes[5] if weighted else None
            sums = RP.forward(*planes[:5], w, GAIN, OFFSET)
            grads = RP.backward(*planes[:5], _grad_up(B), w, GAIN, OFFSET, sums=sums)
            out[(B, H, W, weighted)] = (planes, sums, grads)
    return out


def test_the_planes_reach_every_branch(cases):
    for (B, H, W, weighted), (planes, sums, _) in cases.items():
        if B * H * W > 500:
            assert RP.reaches_every_branch(*planes[:4]), (B, H, W)
        assert np.isfinite(sums).all() and (sums[:, 0] > 0).all()
    assert RP.geom(1, 5, 6)[1] == 1 and RP.geom(3, 33, 17)[1] == 3 and RP.geom(2, 64, 64)[1] == 16
    assert RP.geom(1, 257, 256)[1] == RP.geom(1, 257, 256)[2] + 1


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "weight"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-%dx%d" % s)
def test_forward_sums_bit_exact_against_the_model(cases, shape, weighted):
    planes, want, _ = cases[shape + (weighted,)]
    c = Call(planes, weighted)
    sums = c.forward()
    torch.cuda.synchronize()
    assert_f64_bits_equal(_cpu(sums), want, "sums at %s" % (shape,))
    assert np.array_equal(_cpu(sums)[:, 1], (planes[2][..., 0] >= 0).reshape(shape[0], -1).sum(1).astype(np.float64))
    # the operator returns the same two columns
    sse, cnt = ops().photo_loss(*c.t[:5], c.t[5], GAIN, OFFSET)
    torch.cuda.synchronize()
    assert sse.dtype == torch.float64 and cnt.dtype == torch.float64 and not cnt.requires_grad
    assert_f64_bits_equal(_cpu(sse), want[:, 0], "sse")
    assert_f64_bits_equal(_cpu(cnt), want[:, 1], "count")


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "weight"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-%dx%d" % s)
def test_backward_against_the_model(cases, shape, weighted):
    planes, sums_want, (gt_w, gn_w, gl_w, A) = cases[shape + (weighted,)]
    B = shape[0]
    c = Call(planes, weighted)
    sums = c.forward()
    gt, gn, gl = c.backward(sums, _grad_up(B))      # (every output pre-filled with NaN)
    torch.cuda.synchronize()
    gt, gn, gl = _cpu(gt), _cpu(gn), _cpu(gl)
    assert_bits_equal(gt, gt_w, "grad_tex_img at %s" % (shape,))
    assert_bits_equal(gl, gl_w, "grad_light at %s" % (shape,))
    bound = 2.0 ** -24 * np.abs(gn_w.astype(np.float64)) + 2.0 ** -40 * A[..., None]
    err = np.abs(gn.astype(np.float64) - gn_w.astype(np.float64))
    assert np.isfinite(gn).all()
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print("grad_normal at %s: worst |got - want| / bound = %.3g; %d of %d elements differ in their bits" % (
        shape, worst, int((gn.view(np.uint32) != gn_w.view(np.uint32)).sum()), gn.size))
    assert (err <= bound).all()
    # every element was written, and every uncovered pixel is 0
    covered = planes[2][..., 0] >= 0
    assert np.isfinite(gt).all() and np.isfinite(gl).all()
    assert not gt[~covered].any() and not gn[~covered].any() and gt[covered].any() and gn[covered].any()
    # an output passed as NULL is not touched; the others keep their bits
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        part = [_cpu(o) for o in c.backward(sums, _grad_up(B), want=want)]
        torch.cuda.synchronize()
        for o, full, w in zip(part, (gt, gn, gl), want):
            if w:
                assert np.array_equal(o.view(np.uint32), full.view(np.uint32))
            else:
                assert np.isnan(o).all()


def test_the_loss_is_the_shaders_image(cases):
    """target = synth_shade of the same planes: sse is exactly 0, and so is every gradient"""
    planes, _, _ = cases[(3, 33, 17, True)]
    tex, nrm, ti, light, _, weight = planes
    for weighted in (False, True):
        im, mask = ops().synth_shade(_t(tex), _t(nrm), _t(ti), _t(light), gain=GAIN, offset=OFFSET)
        c = Call((tex, nrm, ti, light, _cpu(im), weight), weighted)
        sums = c.forward()
        gt, gn, gl = c.backward(sums, _grad_up(3))
        torch.cuda.synchronize()
        s = _cpu(sums)
        assert not s[:, 0].any() and not s[:, 2:].any() and np.array_equal(s[:, 1], _cpu(mask).reshape(3, -1).sum(1).astype(np.float64))
        assert not _cpu(gt).any() and not _cpu(gn).any() and not _cpu(gl).any()


def test_faces_are_independent_and_a_nan_stays_in_its_face(cases):
    planes, _, _ = cases[(3, 33, 17, True)]
    B = 3
    whole = Call(planes, True)
    sums = whole.forward()
    grads = whole.backward(sums, _grad_up(B))
    torch.cuda.synchronize()
    sums, grads = _cpu(sums), [_cpu(g) for g in grads]
    for b in range(B):
        one = Call(tuple(p[b:b + 1] for p in planes), True)
        s1 = one.forward()
        g1 = one.backward(s1, _grad_up(B)[b:b + 1])
        torch.cuda.synchronize()
        assert_f64_bits_equal(_cpu(s1), sums[b:b + 1], "face %d alone" % b)
        for a, w in zip(g1, grads):
            assert np.array_equal(_cpu(a).view(np.uint32), w[b:b + 1].view(np.uint32)), b
    # a NaN in one covered pixel of the last face
    bad = [p.copy() for p in planes]
    bad[2][B - 1, 2, 2, 0] = 3
    bad[0][B - 1, 2, 2, 1] = np.nan
    clean = [p.copy() for p in planes]
    clean[2][B - 1, 2, 2, 0] = 3
    res = []
    for pl in (clean, bad):
        c = Call(tuple(pl), True)
        s = c.forward()
        g = c.backward(s, _grad_up(B))
        torch.cuda.synchronize()
        res.append((_cpu(s), [_cpu(x) for x in g]))
    (s0, g0), (s1, g1) = res
    assert np.isnan(s1[B - 1, 0]) and np.isfinite(s0).all() and s1[B - 1, 1] == s0[B - 1, 1]
    assert_f64_bits_equal(s1[:B - 1], s0[:B - 1], "the other faces' sums")
    for a, w in zip(g1, g0):
        assert np.array_equal(a[:B - 1].view(np.uint32), w[:B - 1].view(np.uint32))
    want = RP.forward(*bad[:5], bad[5], GAIN, OFFSET)
    assert_f64_bits_equal(s1, want, "the model with the NaN")
    gt_w, _, gl_w, _ = RP.backward(*bad[:5], _grad_up(B), bad[5], GAIN, OFFSET, sums=want)
    assert_bits_equal(g1[0], gt_w, "grad_tex_img with the NaN")
    assert_bits_equal(g1[2], gl_w, "grad_light with the NaN")


def test_calls_are_reproducible_across_streams_and_threads(cases):
    planes, want, _ = cases[(3, 33, 17, True)]
    B = 3

    def run(stream):
        c = Call(planes, True)
        s = c.forward(stream)
        g = c.backward(s, _grad_up(B), stream=stream)
        (stream or torch.cuda.current_stream(_dev())).synchronize()
        return [_cpu(s).view(np.uint64)] + [_cpu(x).view(np.uint32) for x in g]
    first = run(None)
    assert_f64_bits_equal(first[0].view(np.float64), want, "sums")
    again = run(None)
    side = run(torch.cuda.Stream(device=_dev()))
    streams = [torch.cuda.Stream(device=_dev()) for _ in range(4)]
    with ThreadPoolExecutor(max_workers=4) as pool:
        threaded = list(pool.map(run, streams))
    for other in [again, side] + threaded:
        for a, b in zip(first, other):
            assert np.array_equal(a, b)


# ---- the blend's adjoint ------------------------------------------------------------------------------------------------------------------
def _adjoint(pc, g):
    got = ops().synth_texture_backward(_t(pc) if pc is not None else None, _t(g))
    torch.cuda.synchronize()
    return _cpu(got)


@pytest.mark.parametrize("K", [3, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_blend_adjoint_bit_exact_on_the_small_assets(small_assets, K, B):
    pc = np.ascontiguousarray(small_assets["pc_tex"][:, :K])
    N = pc.shape[0] // 3
    assert N == 480 and 3 * N > 5 * RP.TX_ROWS and (3 * N) % RP.TX_ROWS != 0      # full row tiles and a partial one
    rs = np.random.RandomState(10 * K + B)
    g = (rs.standard_normal((B, 3, N)) * np.exp2(rs.randint(-6, 6, (B, 3, N)))).astype(F)
    assert_bits_equal(_adjoint(pc, g), RP.texture_backward(pc, g), "K = %d, B = %d" % (K, B))


@pytest.mark.parametrize("K", [17, 33])
@pytest.mark.parametrize("B", [8, 9, 17])
def test_blend_adjoint_bit_exact_across_column_chunks_and_face_groups(K, B):
    """K = 17 and 33 run the second and third 16-column chunk, B = 8, 9 and 17 a full group of eight faces, a second group of one
    face and a third; N = 515: 3N = 6 x 256 + 9 rows leaves a ragged last row tile"""
    N = 515
    rs = np.random.RandomState(100 * K + B)
    pc = rs.standard_normal((3 * N, K)).astype(F)
    g = rs.standard_normal((B, 3, N)).astype(F)
    assert_bits_equal(_adjoint(pc, g), RP.texture_backward(pc, g), "K = %d, B = %d" % (K, B))


def test_blend_adjoint_bit_exact_beyond_one_round_of_the_finish_step():
    """3N = 16,500 rows are 65 row tiles: one more than the finish step's 64 lanes, so lane 0 chains two partials"""
    N, K, B = 5500, 3, 2
    assert -(-3 * N // RP.TX_ROWS) == 65
    rs = np.random.RandomState(7)
    pc = rs.standard_normal((3 * N, K)).astype(F)
    g = rs.standard_normal((B, 3, N)).astype(F)
    assert_bits_equal(_adjoint(pc, g), RP.texture_backward(pc, g), "65 row tiles")


def test_blend_adjoint_of_no_columns_is_empty():
    dev = _dev()
    mu = torch.rand((3, 40), device=dev)
    alpha = torch.zeros((2, 0), device=dev, requires_grad=True)
    tex = ops().synth_texture(mu, None, alpha)
    assert tex.requires_grad
    tex.sum().backward()
    torch.cuda.synchronize()
    assert tuple(alpha.grad.shape) == (2, 0)
    assert tuple(_adjoint(None, np.zeros((2, 3, 40), F)).shape) == (2, 0)


def test_synth_texture_node_keeps_the_forward_bits(small_assets):
    dev = _dev()
    mu, pc = _t(small_assets["mu_tex"]), _t(np.ascontiguousarray(small_assets["pc_tex"][:, :10]))
    alpha = torch.as_tensor(np.random.RandomState(4).uniform(-2, 2, (3, 10)).astype(F), device=dev)
    plain = ops().synth_texture(mu, pc, alpha)
    a = alpha.clone().requires_grad_(True)
    node = ops().synth_texture(mu, pc, a)
    assert node.requires_grad and not plain.requires_grad and torch.equal(plain, node.detach())
    g = torch.as_tensor(np.random.RandomState(5).standard_normal(tuple(node.shape)).astype(F), device=dev)
    node.backward(g)
    torch.cuda.synchronize()
    assert_bits_equal(_cpu(a.grad), RP.texture_backward(_cpu(pc), _cpu(g)), "alpha.grad")
    with pytest.raises(ValueError, match="out="):
        ops().synth_texture(mu, pc, a, out=torch.empty_like(plain))
    with torch.no_grad():
        assert torch.equal(ops().synth_texture(mu, pc, a, out=torch.empty_like(plain)), plain)


# ---- the chain through the public operators ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_chain(small_assets):
    """the small_render recipe of tests/test_synth_batch_gpu.py: small assets at 32 x 32, B = 3, sampled on the device"""
    dev, B, S = _dev(), 3, 32
    net = net_mod().FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S, device=dev)
    K = int(net.pc_tex.shape[1])
    P, light, alpha = ops().synth_params(5, 0, B, net.ndim_shape, net.ndim_exp, K, S, light_ranges=LIGHT, alpha_ranges=1.0,
                                         focal=1e-3 * S / 200.0, device=dev)
    torch.cuda.synchronize()
    return dict(net=net, P=P, light=light, alpha=alpha, B=B, S=S)


def test_chain_is_the_hand_composition_of_its_links(small_chain):
    r = small_chain
    net, B, S, dev = r["net"], r["B"], r["S"], _dev()
    o = ops()
    image = torch.zeros((B, S, S, 1), device=dev)
    target = torch.as_tensor(np.random.RandomState(9).uniform(0, 1, (B, S, S, 1)).astype(F), device=dev)
    gvec = torch.as_tensor(_grad_up(B), device=dev)
    # one graph
    P = r["P"].clone().requires_grad_(True)
    light = r["light"].clone().requires_grad_(True)
    alpha = r["alpha"].clone().requires_grad_(True)
    ver = net.vertices_transform(P)
    tex = o.synth_texture(net.mu_tex, net.pc_tex, alpha)
    _, tex_img, normal, tri_ind = o.render_depth(ver, net.tri, tex, image, normal_grad=True, texture_grad=True)
    sse, cnt = o.photo_loss(tex_img, normal, tri_ind, light, target, None, GAIN, OFFSET)
    (sse * gvec).sum().backward()
    torch.cuda.synchronize()
    cov = float((tri_ind >= 0).float().mean())
    assert 0.1 < cov < 0.95, cov
    ns = net.ndim_shape
    for name, g in (("alpha", alpha.grad), ("light", light.grad), ("params", P.grad)):
        assert g is not None and bool(torch.isfinite(g).all()), name
    assert bool(alpha.grad.abs().sum() > 0) and bool(light.grad.abs().sum() > 0) and bool(P.grad[:, 7:7 + ns].abs().sum() > 0)
    # the same links, one at a time, on leaves
    tex_img_l, normal_l, light_l = (t.detach().clone().requires_grad_(True) for t in (tex_img, normal, light))
    sse2, _ = o.photo_loss(tex_img_l, normal_l, tri_ind, light_l, target, None, GAIN, OFFSET)
    g_tex_img, g_normal, g_light = torch.autograd.grad((sse2 * gvec).sum(), [tex_img_l, normal_l, light_l])
    ver_l, tex_l = ver.detach().clone().requires_grad_(True), tex.detach().clone().requires_grad_(True)
    _, tex_img2, normal2, tri_ind2 = o.render_depth(ver_l, net.tri, tex_l, image, normal_grad=True, texture_grad=True)
    g_ver, g_tex = torch.autograd.grad([tex_img2, normal2], [ver_l, tex_l], [g_tex_img, g_normal])
    g_alpha = o.synth_texture_backward(net.pc_tex, g_tex)
    P2 = r["P"].clone().requires_grad_(True)
    (g_P,) = torch.autograd.grad(net.vertices_transform(P2), P2, g_ver)
    torch.cuda.synchronize()
    assert torch.equal(sse2, sse) and torch.equal(tri_ind2, tri_ind)
    assert_bits_equal(_cpu(light.grad), _cpu(g_light), "light")
    assert_bits_equal(_cpu(alpha.grad), _cpu(g_alpha), "alpha")
    assert_bits_equal(_cpu(P.grad), _cpu(g_P), "params")
    # the photometric_loss of nets/losses.py is this chain's mean
    losses = pkg("nets.losses")
    L = losses.photometric_loss(net, ver.detach(), target, light.detach(), alpha.detach(), gain=GAIN, offset=OFFSET)
    assert L.dtype == torch.float64 and torch.equal(L, sse.detach().sum() / cnt.sum().clamp_min(1))


def test_chain_is_exactly_zero_at_the_truth(small_chain):
    """the image shaded from the same parameters: the loss and every gradient are exactly 0"""
    r = small_chain
    net, B, S, dev = r["net"], r["B"], r["S"], _dev()
    o, losses = ops(), pkg("nets.losses")
    with torch.no_grad():
        ver0 = net.vertices_transform(r["P"])
        _, tex_img, normal, tri_ind = o.render_depth(ver0, net.tri, o.synth_texture(net.mu_tex, net.pc_tex, r["alpha"]),
                                                     torch.zeros((B, S, S, 1), device=dev))
        im, _ = o.synth_shade(tex_img, normal, tri_ind, r["light"], gain=GAIN, offset=OFFSET)
    P = r["P"].clone().requires_grad_(True)
    light = r["light"].clone().requires_grad_(True)
    alpha = r["alpha"].clone().requires_grad_(True)
    L = losses.photometric_loss(net, net.vertices_transform(P), im, light, alpha, gain=GAIN, offset=OFFSET)
    L.backward()
    torch.cuda.synchronize()
    assert float(L.detach()) == 0.0
    for g in (P.grad, light.grad, alpha.grad):
        assert g is not None and not bool(g.any())
    # ... and away from it, it is not
    L2 = losses.photometric_loss(net, net.vertices_transform(P), im, light.detach() + 0.1, alpha, gain=GAIN, offset=OFFSET)
    assert float(L2.detach()) > 0


# ---- programs ---------------------------------------------------------------------------------------------------------------------------
def _program(cmd, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _record(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]
    return json.loads(lines[0])


def test_train_program_with_the_photometric_term():
    d = _record(_program(["examples/coarse_loop.py", "--small", "--train", "--steps", "2", "--warmup", "0", "--synth-data", "--photo-loss",
                          "--normal-grad", "--pose-grad"]))
    assert d["train"] is True and d["steps"] == 2 and d["params_finite"] is True
    assert np.isfinite(d["photometric_loss"]) and d["photometric_loss"] >= 0 and d["losses"]["photometric_loss"] == d["photometric_loss"]
    assert all(np.isfinite(v) for v in d["losses"].values()), d["losses"]


def test_photo_loss_flag_needs_synthetic_data():
    p = _program(["examples/coarse_loop.py", "--small", "--train", "--steps", "1", "--warmup", "0", "--photo-loss"], timeout=120)
    assert p.returncode == 2 and "--photo-loss needs --synth-data" in p.stderr and not p.stdout.strip()


def test_photo_fit_descends():
    d = _record(_program(["examples/photo_fit.py", "--small"]))
    print("photo_fit --small:", json.dumps(d))
    assert d["finite"] is True and np.isfinite(d["first"]) and np.isfinite(d["last"])
    assert d["last"] < d["first"]
