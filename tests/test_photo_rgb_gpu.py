"""GPU: colour shading (csrc/fr_shade.h, fr_synth.hip, fr_photo.hip; rendering_layer.ops.synth_light_rgb / synth_shade_rgb /
photo_loss_rgb, nets.losses.photometric_loss with a [B,3,9] lighting).  The shader's image and its gray, the sampler, the forward's 29
sums, grad_tex_img and grad_light are held to the numpy model of tests/ref_photo_rgb.py bit for bit; grad_normal within the gray
header's bound evaluated with the colour g~ (the device's float64 division and square root are not assumed to round as the host's);
the loss is the shader's image to the bit; faces are independent; calls are reproducible across streams and host threads; the chain
through the public operators is the hand composition of its links; the callers run as programs."""
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
import ref_photo_rgb as RC
from raw_calls import GAIN, OFFSET, PhotoRgbCall as Call, assert_f64_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = RC.SHAPES
assert SHAPES == [(1, 5, 6), (3, 33, 17), (2, 64, 64), (1, 257, 256)]
IDS = lambda s: "B%d-%dx%d" % s   # noqa: E731


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
    for shape in SHAPES:
        planes = RC.hand_planes_rgb(*shape, seed=RC.SEEDS[shape])
        for weighted in (False, True):
            w = planes[5] if weighted else None
            sums = RC.forward(*planes[:5], w, GAIN, OFFSET)
            grads = RC.backward(*planes[:5], _grad_up(shape[0]), w, GAIN, OFFSET, sums=sums)
            out[shape + (weighted,)] = (planes, sums, grads)
    return out


def test_the_planes_reach_every_branch(cases):
    for (B, H, W, weighted), (planes, sums, _) in cases.items():
        assert RC.reaches_every_branch(*planes[:4], planes[5]), (B, H, W)
        assert np.isfinite(sums).all() and (sums[:, 0] > 0).all()
    assert RC.geom_rgb(1, 5, 6)[1] == 1 and RC.geom_rgb(3, 33, 17)[1] == 3 and RC.geom_rgb(2, 64, 64)[1] == 16
    assert RC.geom_rgb(1, 257, 256)[1] == RC.geom_rgb(1, 257, 256)[2] + 1 and RC.geom_rgb(1, 5, 6)[3] == 29


# ---- the shader and the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shader_bit_exact_with_every_background(cases, shape):
    planes, _, _ = cases[shape + (False,)]
    tex, nrm, ti, light = planes[:4]
    B, H, W = shape
    rs = np.random.RandomState(B + H)
    for bg in (None, rs.uniform(-1, 1, (1, H, W, 3)).astype(F), rs.uniform(-1, 1, (B, H, W, 3)).astype(F)):
        want = RC.shade(tex, nrm, ti, light, bg, GAIN, OFFSET)
        got = ops().synth_shade_rgb(_t(tex), _t(nrm), _t(ti), _t(light), background=_t(bg), gain=GAIN, offset=OFFSET)
        torch.cuda.synchronize()
        for g, w, name in zip(got, want, ("im_rgb", "im_gray", "mask")):
            assert tuple(g.shape) == w.shape
            assert_bits_equal(_cpu(g), w, "%s at %s, background %s" % (name, shape, None if bg is None else bg.shape))
        # out=: the caller's tensors are written, every element
        out = (torch.full((B, H, W, 3), float("nan"), device=_dev()), torch.full((B, H, W, 1), float("nan"), device=_dev()),
               torch.full((B, H, W, 1), float("nan"), device=_dev()))
        again = ops().synth_shade_rgb(_t(tex), _t(nrm), _t(ti), _t(light), background=_t(bg), gain=GAIN, offset=OFFSET, out=out)
        torch.cuda.synchronize()
        assert all(a is b for a, b in zip(again, out)) and all(torch.equal(a, b) for a, b in zip(again, got))
    # im_gray is optional at the C level: a NULL plane is not written and the others keep their bits
    L = pkg("_lib").lib()
    t = [_t(tex), _t(nrm), _t(ti), _t(light)]
    rgb, mask = torch.full((B, H, W, 3), float("nan"), device=_dev()), torch.full((B, H, W, 1), float("nan"), device=_dev())
    rc = L.fr_synth_shade_rgb(*[_p(x) for x in t], None, 0, B, H, W, GAIN, OFFSET, _p(rgb), None, _p(mask),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = RC.shade(tex, nrm, ti, light, None, GAIN, OFFSET)
    assert rc == 0
    assert_bits_equal(_cpu(rgb), want[0], "im_rgb without a gray plane")
    assert_bits_equal(_cpu(mask), want[2], "mask without a gray plane")


@pytest.mark.parametrize("seed, first, B", [(5, 0, 3), (2 ** 63 + 11, 2 ** 64 - 2, 4), (77, 1000, 65)])
def test_sampler_bit_exact_and_beside_the_existing_streams(seed, first, B):
    o = ops()
    ns, ne, K, S = 9, 5, 3, 32
    before = o.synth_params(seed, first, B, ns, ne, K, S, device=_dev())
    light = o.synth_light_rgb(seed, first, B, device=_dev())
    after = o.synth_params(seed, first, B, ns, ne, K, S, device=_dev())
    torch.cuda.synchronize()
    assert_bits_equal(_cpu(light), RC.sample_light(seed, first, B), "light [B,3,9]")
    for a, b, name in zip(before, after, ("params", "light", "alpha")):
        assert_bits_equal(_cpu(a), _cpu(b), name)                              # the existing sampler's outputs do not move
    import ref_synth_batch as RS   # ... and are still that sampler's own model
    want = RS.sample(seed, first, B, ns, ne, K, S, 0.7, o.SYNTH_LIGHT_RANGES, [(-1.0, 1.0)] * K, focal=1e-3)
    for a, w, name in zip(after, want[:3], ("params", "light", "alpha")):
        assert_bits_equal(_cpu(a), w, name + " against the existing sampler's model")
    # channel 0's first four coefficients share the gray lighting's ranges, and are other draws
    assert not (_cpu(light)[:, 0, :4] == want[1]).any()
    lo, hi = np.asarray(RC.LIGHT_RANGES_RGB, F).T
    assert tuple(light.shape) == (B, 3, 9) and (_cpu(light).reshape(B, 27) >= lo).all() and (_cpu(light).reshape(B, 27) <= hi).all()
    # other ranges, and a caller's tensor
    out = torch.full((B, 3, 9), float("nan"), device=_dev())
    rg = [(-1.0 - 0.1 * j, 2.0 + j) for j in range(27)]
    assert o.synth_light_rgb(seed, first, B, ranges=rg, out=out) is out
    torch.cuda.synchronize()
    assert_bits_equal(_cpu(out), RC.sample_light(seed, first, B, rg), "light with other ranges")


# ---- the loss -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "weight"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_sums_bit_exact_against_the_model(cases, shape, weighted):
    planes, want, _ = cases[shape + (weighted,)]
    c = Call(planes, weighted)
    sums = c.forward()
    torch.cuda.synchronize()
    assert_f64_bits_equal(_cpu(sums), want, "sums at %s" % (shape,))
    assert np.array_equal(_cpu(sums)[:, 1], (planes[2][..., 0] >= 0).reshape(shape[0], -1).sum(1).astype(np.float64))
    # the operator returns the same two columns
    sse, cnt = ops().photo_loss_rgb(*c.t[:5], c.t[5], GAIN, OFFSET)
    torch.cuda.synchronize()
    assert sse.dtype == torch.float64 and cnt.dtype == torch.float64 and not cnt.requires_grad
    assert_f64_bits_equal(_cpu(sse), want[:, 0], "sse")
    assert_f64_bits_equal(_cpu(cnt), want[:, 1], "count")


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "weight"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
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
    # the gray header's bound with the colour g~
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
    """target = synth_shade_rgb of the same planes: sse is exactly 0, and so is every gradient"""
    planes, _, _ = cases[(3, 33, 17, True)]
    tex, nrm, ti, light, _, weight = planes
    for weighted in (False, True):
        im, _, mask = ops().synth_shade_rgb(_t(tex), _t(nrm), _t(ti), _t(light), gain=GAIN, offset=OFFSET)
        c = Call((tex, nrm, ti, light, _cpu(im), weight), weighted)
        sums = c.forward()
        gt, gn, gl = c.backward(sums, _grad_up(3))
        torch.cuda.synchronize()
        s = _cpu(sums)
        assert not s[:, 0].any() and not s[:, 2:].any() and np.array_equal(s[:, 1], _cpu(mask).reshape(3, -1).sum(1).astype(np.float64))
        assert not _cpu(gt).any() and not _cpu(gn).any() and not _cpu(gl).any()


def _run(planes, g, weighted=True):
    c = Call(tuple(planes), weighted)
    s = c.forward()
    grads = c.backward(s, g)
    torch.cuda.synchronize()
    return _cpu(s), [_cpu(x) for x in grads]


def test_faces_are_independent_and_a_nan_stays_in_its_face(cases):
    planes, _, _ = cases[(3, 33, 17, True)]
    B = 3
    sums, grads = _run(planes, _grad_up(B))
    for b in range(B):
        s1, g1 = _run([p[b:b + 1] for p in planes], _grad_up(B)[b:b + 1])
        assert_f64_bits_equal(s1, sums[b:b + 1], "face %d alone" % b)
        for a, w in zip(g1, grads):
            assert np.array_equal(a.view(np.uint32), w[b:b + 1].view(np.uint32)), b
    # a NaN in one covered pixel of the last face (the planes of hand_planes_rgb(nan=True))
    bad = [p.copy() for p in planes]
    bad[2][B - 1, 2, 3, 0] = 3
    bad[0][B - 1, 2, 3, 1] = np.nan
    clean = [p.copy() for p in planes]
    clean[2][B - 1, 2, 3, 0] = 3
    (s0, g0), (s1, g1) = _run(clean, _grad_up(B)), _run(bad, _grad_up(B))
    assert np.isnan(s1[B - 1, 0]) and np.isfinite(s0).all() and s1[B - 1, 1] == s0[B - 1, 1]
    assert_f64_bits_equal(s1[:B - 1], s0[:B - 1], "the other faces' sums")
    for a, w in zip(g1, g0):
        assert np.array_equal(a[:B - 1].view(np.uint32), w[:B - 1].view(np.uint32))
    want = RC.forward(*bad[:5], bad[5], GAIN, OFFSET)
    assert_f64_bits_equal(s1, want, "the model with the NaN")
    # the NaN is in channel 1: it reaches that channel's lighting sums where the channel is lit, and no other channel's
    lit1 = RC.shade_terms(*bad[:4], GAIN, OFFSET)["s"][B - 1, 2, 3, 1] > 0
    assert np.isnan(s1[B - 1, 2 + 9:2 + 18]).all() == bool(lit1) and np.isfinite(s1[B - 1, 2:2 + 9]).all() and np.isfinite(s1[B - 1, 2 + 18:]).all()
    gt_w, _, gl_w, _ = RC.backward(*bad[:5], _grad_up(B), bad[5], GAIN, OFFSET, sums=want)
    assert_bits_equal(g1[0], gt_w, "grad_tex_img with the NaN")
    assert_bits_equal(g1[2], gl_w, "grad_light with the NaN")
    # a NaN in light[1], and one in grad_sse[1]: face 1 alone
    nl = [p.copy() for p in planes]
    nl[3][1, 2, 4] = np.nan
    s2, g2 = _run(nl, _grad_up(B))
    assert np.isnan(s2[1, 0]) and s2[1, 1] == sums[1, 1]
    gnan = _grad_up(B).copy()
    gnan[1] = np.nan
    s3, g3 = _run(planes, gnan)
    assert_f64_bits_equal(s3, sums, "the forward does not read grad_sse")
    for other in (0, 2):
        assert_f64_bits_equal(s2[other:other + 1], sums[other:other + 1], "face %d beside a NaN light" % other)
        for a, b_, w in zip(g2, g3, grads):
            assert np.array_equal(a[other].view(np.uint32), w[other].view(np.uint32))
            assert np.array_equal(b_[other].view(np.uint32), w[other].view(np.uint32))
    assert np.isnan(g3[2][1]).all() and np.isnan(g2[1][1]).any()          # grad_light under a NaN grad_sse; grad_normal under a NaN light


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
    second = run(torch.cuda.Stream(device=_dev()))
    with ThreadPoolExecutor(max_workers=2) as pool:
        threaded = list(pool.map(run, [torch.cuda.Stream(device=_dev()) for _ in range(2)]))
    for other in [again, side, second] + threaded:
        for a, b in zip(first, other):
            assert np.array_equal(a, b)


# ---- the chain through the public operators ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_chain(small_assets):
    """small assets at 32 x 32, B = 3, sampled on the device"""
    dev, B, S = _dev(), 3, 32
    net = net_mod().FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S, device=dev)
    K = int(net.pc_tex.shape[1])
    P, _, alpha = ops().synth_params(5, 0, B, net.ndim_shape, net.ndim_exp, K, S, alpha_ranges=1.0, focal=1e-3 * S / 200.0, device=dev)
    light = ops().synth_light_rgb(5, 0, B, device=dev)
    torch.cuda.synchronize()
    return dict(net=net, P=P, light=light, alpha=alpha, B=B, S=S)


def test_chain_is_the_hand_composition_of_its_links(small_chain):
    r = small_chain
    net, B, S, dev = r["net"], r["B"], r["S"], _dev()
    o = ops()
    image = torch.zeros((B, S, S, 1), device=dev)
    target = torch.as_tensor(np.random.RandomState(9).uniform(0, 1, (B, S, S, 3)).astype(F), device=dev)
    gvec = torch.as_tensor(_grad_up(B), device=dev)
    # one graph
    P = r["P"].clone().requires_grad_(True)
    light = r["light"].clone().requires_grad_(True)
    alpha = r["alpha"].clone().requires_grad_(True)
    ver = net.vertices_transform(P)
    tex = o.synth_texture(net.mu_tex, net.pc_tex, alpha)
    _, tex_img, normal, tri_ind = o.render_depth(ver, net.tri, tex, image, normal_grad=True, texture_grad=True)
    sse, cnt = o.photo_loss_rgb(tex_img, normal, tri_ind, light, target, None, GAIN, OFFSET)
    (sse * gvec).sum().backward()
    torch.cuda.synchronize()
    cov = float((tri_ind >= 0).float().mean())
    assert 0.1 < cov < 0.95, cov
    ns = net.ndim_shape
    for name, g in (("alpha", alpha.grad), ("light", light.grad), ("params", P.grad)):
        assert g is not None and bool(torch.isfinite(g).all()), name
    assert tuple(light.grad.shape) == (B, 3, 9) and bool((light.grad.abs().sum(dim=(0, 2)) > 0).all())
    assert bool(alpha.grad.abs().sum() > 0) and bool(P.grad[:, 7:7 + ns].abs().sum() > 0)
    # the same links, one at a time, on leaves
    tex_img_l, normal_l, light_l = (t.detach().clone().requires_grad_(True) for t in (tex_img, normal, light))
    sse2, _ = o.photo_loss_rgb(tex_img_l, normal_l, tri_ind, light_l, target, None, GAIN, OFFSET)
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
    # the loss and its gradients are the numpy model's on these planes
    planes = (_cpu(tex_img), _cpu(normal), _cpu(tri_ind), _cpu(light), _cpu(target), None)
    want = RC.forward(*planes[:5], None, GAIN, OFFSET)
    assert_f64_bits_equal(_cpu(sse), want[:, 0], "sse on the rendered planes")
    gt_w, _, gl_w, _ = RC.backward(*planes[:5], _grad_up(B), None, GAIN, OFFSET, sums=want)
    assert_bits_equal(_cpu(g_tex_img), gt_w, "grad_tex_img on the rendered planes")
    assert_bits_equal(_cpu(g_light), gl_w, "grad_light on the rendered planes")
    # the photometric_loss of nets/losses.py picks the route by light's shape: the colour chain's mean over pixels and channels
    losses = pkg("nets.losses")
    L = losses.photometric_loss(net, ver.detach(), target, light.detach(), alpha.detach(), gain=GAIN, offset=OFFSET)
    assert L.dtype == torch.float64 and torch.equal(L, sse.detach().sum() / (3 * cnt.sum()).clamp_min(1))
    gray_light = torch.zeros((B, 4), device=dev)
    Lg = losses.photometric_loss(net, ver.detach(), image, gray_light, alpha.detach(), gain=GAIN, offset=OFFSET)
    sse_g, cnt_g = o.photo_loss(tex_img.detach(), normal.detach(), tri_ind, gray_light, image, None, GAIN, OFFSET)
    assert torch.equal(Lg, sse_g.sum() / cnt_g.sum().clamp_min(1))
    for bad_light, picture in ((light.detach(), image), (light.detach(), image[..., 0]), (gray_light, target), (light.detach()[:, :, :4], target)):
        with pytest.raises(ValueError, match="im_rgb"):
            losses.photometric_loss(net, ver.detach(), picture, bad_light, alpha.detach())


def test_chain_is_exactly_zero_at_the_truth(small_chain):
    """the colour image shaded from the same parameters: the loss and every gradient are exactly 0"""
    r = small_chain
    net, B, S, dev = r["net"], r["B"], r["S"], _dev()
    o, losses = ops(), pkg("nets.losses")
    image = torch.zeros((B, S, S, 1), device=dev)
    with torch.no_grad():
        ver0 = net.vertices_transform(r["P"])
        _, tex_img, normal, tri_ind = o.render_depth(ver0, net.tri, o.synth_texture(net.mu_tex, net.pc_tex, r["alpha"]), image)
        im, _, _ = o.synth_shade_rgb(tex_img, normal, tri_ind, r["light"], gain=GAIN, offset=OFFSET)
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


def test_colour_batches_carry_the_image_they_depict(small_assets):
    """pipeline.SynthBatches(colour=True): the gray stream's params, alpha, depth, mask and tri_ind; light [B,3,9] from the colour
    sampler; im_rgb the shader's image of the batch's own planes, im_gray its gray; the default stream is unchanged beside it"""
    dev, B, S = _dev(), 3, 32
    pipe = pkg("pipeline")
    net = net_mod().FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S, device=dev)
    kw = dict(slots=1, focal=1e-3 * S / 200.0, gain=GAIN, offset=OFFSET)
    gray_s, col_s = pipe.SynthBatches(net, B, 21, **kw), pipe.SynthBatches(net, B, 21, colour=True, **kw)
    for n in range(2):
        g = {k: v.clone() for k, v in gray_s.next().items()}
        c = {k: v.clone() for k, v in col_s.next().items()}
        torch.cuda.synchronize()
        assert set(c) == set(g) | {"im_rgb"} and tuple(c["light"].shape) == (B, 3, 9) and tuple(g["light"].shape) == (B, 4)
        for k in ("params", "alpha", "depth", "mask", "tri_ind"):
            assert torch.equal(c[k], g[k]), k
        assert_bits_equal(_cpu(c["light"]), RC.sample_light(21, n * B, B), "batch %d: light" % n)
        assert_bits_equal(_cpu(c["im_gray"]), RC.gray_of(_cpu(c["im_rgb"]))[..., None], "batch %d: im_gray is the gray of im_rgb" % n)
        assert not torch.equal(c["im_gray"], g["im_gray"]) and bool((c["im_rgb"][..., 0] != c["im_rgb"][..., 2]).any())
    gray_s.synchronize()
    col_s.synchronize()


# ---- programs ---------------------------------------------------------------------------------------------------------------------------
def _program(cmd, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _record(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]
    return json.loads(lines[0])


def test_train_program_with_colour_batches_and_the_colour_term():
    d = _record(_program(["examples/coarse_loop.py", "--small", "--train", "--steps", "2", "--warmup", "0", "--synth-data",
                          "--synth-colour", "--photo-loss", "--normal-grad", "--pose-grad"]))
    assert d["train"] is True and d["steps"] == 2 and d["params_finite"] is True
    assert np.isfinite(d["photometric_loss"]) and d["photometric_loss"] >= 0 and d["losses"]["photometric_loss"] == d["photometric_loss"]
    assert all(np.isfinite(v) for v in d["losses"].values()), d["losses"]


def test_synth_colour_flag_needs_synthetic_data():
    p = _program(["examples/coarse_loop.py", "--small", "--train", "--steps", "1", "--warmup", "0", "--synth-colour"], timeout=120)
    assert p.returncode == 2 and "--synth-colour needs --synth-data" in p.stderr and not p.stdout.strip()


def test_photo_fit_descends_in_colour():
    d = _record(_program(["examples/photo_fit.py", "--small", "--colour"]))
    print("photo_fit --small --colour:", json.dumps(d))
    assert d["colour"] is True and d["finite"] is True and np.isfinite(d["first"]) and np.isfinite(d["last"])
    assert d["last"] < d["first"]
