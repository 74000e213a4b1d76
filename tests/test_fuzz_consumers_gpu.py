"""Seeded differential fuzzing of every consumer of the rasteriser's tri_ind plane -- the normal backward (raw and post mode), the
texture backward (shared and per-face texture), the interpolated depth (forward and backward), mesh_visible / mesh_lift,
synth_shade / photo_loss, the soft coverage (forward and backward), synth_shade_rgb / photo_loss_rgb, and the per-face albedo fit
(basis build and moments) -- on the scenes of the rasteriser fuzz (tests/fuzz_scenes.py: jittered sub-pixel grids, triangle soup,
small-triangle soup, integer coordinates with ties, and the specials: duplicated and degenerate triangles, NaN / Inf / 3e9 /
subnormal / -0.0 coordinates, triangle ids of -1, nver, NaN and 0.75), cut down to at most 8 faces and 200,000 pixels.

A case renders its scene once and holds the planes to the CPU oracle; every consumer and its numpy model (tests/ref_*.py) is then
handed the ORACLE's tri_ind and normal planes, so a consumer's failure is not a forward failure in disguise.  No bound here is new
or measured: each is the one include/fr_hotpath.h states for the kernel and the model already implements -- bits where the header
says bit for bit, the integer bound of ref_normal_backward.check_bound for the owner-scatter sums, the header's class rule
(ref_normal_backward.check_bad_faces, ref_texture_backward.assert_bad_scope) for a face or scope with a non-finite term.
A second pass hands the consumers what no rendered scene holds (fuzz_scenes.ConsumerCase.altered): bad ids in triangles that do win
pixels, and NaN / ntri / fractional / -0.0 entries in the plane.  Without it an `ok` test that ignores an id, or a NaN tri_ind taken as
covered, passes every case.  The soft coverage has a third pass (ConsumerCase.vertex_altered): NaN, Inf and huge coordinates in
vertices of triangles that own a border pixel, under the oracle's plane of the unpoisoned scene -- the rasteriser never lets such a
triangle win, so no render reaches the coverage's exits for a non-finite area or quotient -- and a fourth
(ConsumerCase.vertex_on_segment): a vertex exactly on the segment between an OK pixel's centre and its neighbour's, so that two
edges tie on s inside (0, 1) and the "lowest k" rule shows in the backward.
NOT covered: the owner-scatter geometry with shift > 0 (more than 2^20 pixels per face).  The numpy models cannot afford such a
plane, and CONSUMER_PIXELS keeps every case far below it; tests/test_render_backward_exact_gpu.py reaches it for the render
backward alone.  tests/test_fuzz_scenes_cpu.py holds the seed set to reaching every class of input this file exists
for, and names the seed base."""
import collections
import os

import numpy as np
import pytest
import torch

import fuzz_scenes as FS
import ref_albedo_lse as RA
import ref_coverage as RC
import ref_depth_interp as RD
import ref_mesh as RM
import ref_normal_backward as RN
import ref_photo_loss as RP
import ref_photo_rgb as RPR
import ref_synth_batch as RS
import ref_texture_backward as RT
from gpu_util import assert_bits_equal, assert_render_equal, ops, render_gpu
from raw_calls import (GAIN, OFFSET, SENT, PhotoCall, PhotoRgbCall, assert_f64_bits_equal, cbwd, cfwd, dbwd, dfwd, nbwd, raw_basis,
                       raw_fit, raw_lift, raw_visible, tbwd)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N_RENDER = int(os.environ.get("FR_FUZZ_CASES", "160"))
N_CASES = max(1, N_RENDER * 3 // 10)


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _finite_faces(*models):
    return np.array([not any(R.faces[b].bad for R in models) for b in range(len(models[0].faces))])


def _twice(call, R, what, post=False):
    """two launches of an owner-scatter backward -> the first result: bit-equal on the finite faces, and each within the model:
    the integer bound there, the header's class rule on the faces with a non-finite term"""
    first, second = call().cpu().numpy(), call().cpu().numpy()
    fin = _finite_faces(R)
    assert_bits_equal(first[fin], second[fin], what + ": two launches")
    assert RN.check_bound(first, R, post=post) <= 1.0, what
    for out in (first, second):
        RN.check_bad_faces(out, R)
    return first


def check_normal_backward(c, ti, what, profiles=(0, 1)):
    """-> (the raw-mode result and its model on the first gradient profile)"""
    V, tri, tind = _t(c.ver), _t(c.tri), _t(ti)
    keep = None
    for mode in (0, 1):
        for k in profiles:
            g = c.g_normal[k]
            R = RN.model(g, c.ver, c.tri, ti, c.H, c.W, mode)
            gt = _t(g)
            got = _twice(lambda: nbwd(gt, V, tri, tind, c.H, c.W, mode), R,
                         "%s: normal backward, profile %d, %s" % (what, k, "post" if mode else "raw"), post=mode == 1)
            if k == profiles[0] and mode == c.seed % 2:                       # once per case: accumulate onto a finite tensor
                acc = nbwd(gt, V, tri, tind, c.H, c.W, mode, out=_t(c.old), accumulate=1).cpu().numpy()
                fin = _finite_faces(R)
                assert_bits_equal(acc[fin], (c.old + got)[fin], what + ": normal backward, accumulate")
            if k == 0 and mode == 0:
                keep = (got, R)
    return keep


def check_depth_interp(c, ti, what, profiles=(0, 1)):
    V, tri, tind = _t(c.ver), _t(c.tri), _t(ti)
    want = RD.forward(c.ver, c.tri, ti, c.H, c.W)
    assert_bits_equal(dfwd(V, tri, tind, c.H, c.W).cpu().numpy(), want, what + ": interpolated depth")
    keep = None
    for k in profiles:
        g = c.g_depth[k]
        R = RD.model(g, c.ver, c.tri, ti, c.H, c.W)
        gt = _t(g)
        got = _twice(lambda: dbwd(gt, V, tri, tind, c.H, c.W), R, "%s: interpolated depth backward, profile %d" % (what, k))
        if k == 0:
            keep = (got, R)
    return keep


def check_texture_backward(c, ti, what, profiles=(0, 1)):
    tri, tind = _t(c.tri), _t(ti)
    keep = None
    for k in profiles:
        g = c.g_tex[k]
        M = RT.model(g, c.tri, ti, c.nver, c.H, c.W, c.tex_batch)
        got = tbwd(_t(g), tri, tind, c.nver, c.H, c.W, c.tex_batch).cpu().numpy()
        for s in range(c.tex_batch):
            if M.bad[s]:
                RT.assert_bad_scope(got[s], M, s)
            else:
                assert_bits_equal(got[s], M.value()[s], "%s: texture backward, profile %d, scope %d of %d" % (what, k, s, c.tex_batch))
        if k == 0:
            keep = (got, M)
    return keep


def check_mesh(c, planes, what):
    ntri = c.tri.shape[1]
    tind = planes[3].reshape(c.B, c.H, c.W)
    coarse = planes[0].reshape(c.B, c.H, c.W)
    fine = c.with_noise(RM.fine_of(coarse))
    m_vis = RM.visible(c.tri, tind, c.nver)
    m_out, m_state = RM.lift(c.ver, tind, m_vis, fine, coarse, ntri)
    g_vis = raw_visible(_t(c.tri), _t(tind), c.nver)
    g_out, g_state = raw_lift(_t(c.ver), c.nver, _t(tind), g_vis, _t(fine), _t(coarse), ntri, c.nver + 3)
    assert np.array_equal(g_vis.cpu().numpy(), m_vis), what + ": mesh_visible"
    assert np.array_equal(g_state.cpu().numpy(), m_state), what + ": mesh_lift state"
    g_out = g_out.cpu().numpy()
    assert_bits_equal(g_out[:, :, :c.nver], m_out, what + ": mesh_lift")
    assert (g_out[:, :, c.nver:].view(np.uint32) == SENT).all(), what + ": mesh_lift wrote a pad column"


# One shading model as check_shade_and_photo_loss sees it: the op pair (`shader`, whose outputs are `planes`, and `loss`, called raw
# through `call`), the numpy models (`ref`: the loss's module; `shade`: the shader's function) and the names of the case's light,
# target and background fields (background None: the case has none for this model, the shader runs without).
ShadeModel = collections.namedtuple("ShadeModel", "shader planes loss call ref shade light target background")
GRAY = ShadeModel("synth_shade", ("im_gray", "mask"), "photo_loss", PhotoCall, RP, RS.shade, "light", "target", None)
RGB = ShadeModel("synth_shade_rgb", ("im_rgb", "im_gray", "mask"), "photo_loss_rgb", PhotoRgbCall, RPR, RPR.shade, "light_rgb",
                 "target_rgb", "background_rgb")


def check_shade_and_photo_loss(m, c, planes, what):
    """the shader and the photometric loss of the model m (GRAY or RGB) on the case's light, target and background for that model, its
    weight and grad_sse"""
    tex_img, normal, ti = planes[1], planes[2], planes[3]
    weighted = c.weight is not None
    light, target = getattr(c, m.light), getattr(c, m.target)
    bg = getattr(c, m.background) if m.background else None
    got = getattr(ops(), m.shader)(_t(tex_img), _t(normal), _t(ti), _t(light), background=None if bg is None else _t(bg),
                                   gain=GAIN, offset=OFFSET)
    for g, w, name in zip(got, m.shade(tex_img, normal, ti, light, bg, GAIN, OFFSET), m.planes):
        assert_bits_equal(g.cpu().numpy(), w, "%s: %s %s" % (what, m.shader, name))
    what = "%s: %s" % (what, m.loss)

    def run(nrm):
        call = m.call((tex_img, nrm, ti, light, target, c.weight), weighted)
        sums = call.forward()
        grads = call.backward(sums, c.grad_sse)
        return sums.cpu().numpy(), [g.cpu().numpy() for g in grads]
    sums, (gt, gn, gl) = run(normal)
    want = m.ref.forward(tex_img, normal, ti, light, target, c.weight, GAIN, OFFSET)
    assert_f64_bits_equal(sums, want, what + " sums")
    gt_w, gn_w, gl_w, A = m.ref.backward(tex_img, normal, ti, light, target, c.grad_sse, c.weight, GAIN, OFFSET, sums=want)
    assert_bits_equal(gt, gt_w, what + " grad_tex_img")
    assert_bits_equal(gl, gl_w, what + " grad_light")
    # grad_normal: the header's bound (the gray one, with the model's own g~) where the model is finite; where it is not, the same NaN
    # or the same Inf
    fin = np.isfinite(gn_w)
    assert np.array_equal(np.isnan(gn), np.isnan(gn_w)), what + " grad_normal NaNs"
    assert np.array_equal(gn[~fin & ~np.isnan(gn_w)], gn_w[~fin & ~np.isnan(gn_w)]), what + " grad_normal Infs"
    bound = 2.0 ** -24 * np.abs(gn_w.astype(np.float64)) + 2.0 ** -40 * np.broadcast_to(A[..., None], gn_w.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(gn.astype(np.float64) - gn_w.astype(np.float64))
        assert (err[fin] <= bound[fin]).all(), (what + " grad_normal", float(np.nanmax(err[fin] / bound[fin])))
    covered = ti[..., 0] >= 0
    assert not gt[~covered].view(np.uint32).any() and not gn[~covered].view(np.uint32).any()
    # a NaN normal reaches its own pixel and its own face's sums, and nothing else changes by a bit: the same call with those
    # normals replaced by finite ones
    sick = covered & np.isnan(normal).any(-1)
    if sick.any():
        clean_sums, (gt2, gn2, gl2) = run(np.where(sick[..., None], np.float32(0.5), normal))
        well = ~sick.reshape(c.B, -1).any(1)
        assert_f64_bits_equal(sums[well], clean_sums[well], what + ", the faces without a NaN normal")
        assert_f64_bits_equal(sums[:, 1], clean_sums[:, 1], what + " cnt")
        assert_bits_equal(gl[well], gl2[well], what + " grad_light, the faces without a NaN normal")
        assert_bits_equal(gt[~sick], gt2[~sick], what + " grad_tex_img, the pixels without a NaN normal")
        assert_bits_equal(gn[~sick], gn2[~sick], what + " grad_normal, the pixels without a NaN normal")
        assert np.isnan(sums[~well, 0]).all() and np.isfinite(clean_sums[:, 1]).all()


def check_coverage(c, ti, what, profiles=(0, 1)):
    """The soft coverage on the case's table and plane, then on poisoned vertices (ConsumerCase.vertex_altered) and on vertices moved
    onto a segment between two centres (ConsumerCase.vertex_on_segment), both under the same plane.
    The forward bit for bit; the backward -- handed the model's plane, which the forward's has just been held to -- through _twice;
    the z row exactly +0 on the finite faces; once per case accumulate = 1, and both kernels on a padded vertex pitch with NaN in
    the pad.  -> (the result and its model on the first profile, the model's plane)"""
    H, W, nver = c.H, c.W, c.nver
    tri, tind = _t(c.tri), _t(ti)

    def run(case, label, profiles, extras):
        V = _t(case.ver)
        want = RC.forward(case.ver, c.tri, ti, H, W)
        got_cov = cfwd(V, tri, tind, H, W).cpu().numpy()
        assert_bits_equal(got_cov, want, label + ": soft coverage")
        cov, keep = _t(want), None
        for k in profiles:
            R = RC.model(case.g_cov[k], want, case.ver, c.tri, ti, H, W)
            gt = _t(case.g_cov[k])
            got = _twice(lambda: cbwd(gt, cov, V, tri, tind, H, W), R, "%s: soft coverage backward, profile %d" % (label, k))
            fin = _finite_faces(R)
            assert not got[fin][:, 2].view(np.uint32).any(), label + ": soft coverage backward, the z row"
            if extras and k == profiles[0]:
                acc = cbwd(gt, cov, V, tri, tind, H, W, out=_t(c.old), accumulate=1).cpu().numpy()
                assert_bits_equal(acc[fin], (c.old + got)[fin], label + ": soft coverage backward, accumulate")
                pitch = nver + 5
                Vp = torch.full((c.B, 3, pitch), float("nan"), device=DEV)
                Vp[:, :, :nver] = V
                assert_bits_equal(cfwd(Vp, tri, tind, H, W, pitch=(pitch, nver)).cpu().numpy(), want, label + ": soft coverage, padded pitch")
                padded = cbwd(gt, cov, Vp, tri, tind, H, W, pitch=(pitch, nver)).cpu().numpy()
                assert_bits_equal(padded[fin], got[fin], label + ": soft coverage backward, padded pitch")
            if k == 0:
                keep = (got, R)
        return got_cov, keep, want

    clean, keep, want = run(c, what, profiles, True)
    v = c.vertex_altered(ti)
    sick, _, _ = run(v, what + ", poisoned vertices", (c.seed % 2,), False)
    # a pixel is out of the poison's reach when neither its own triangle nor a 4-neighbour's names a poisoned vertex: its bits stay
    marked = (v.ver.view(np.uint32) != c.ver.view(np.uint32)).any(axis=1)      # [B,nver]
    reach = np.zeros((c.B, H + 2, W + 2), bool)
    for b in range(c.B):
        okt, tid = RC.ok_triangles(c.tri, ti[b], nver)
        hit = ((okt >= 0) & marked[b][np.clip(tid[:, np.maximum(okt, 0)], 0, nver - 1)].any(axis=0)).reshape(H, W)
        for dy, dx in ((1, 1), (1, 0), (1, 2), (0, 1), (2, 1)):
            reach[b, dy:dy + H, dx:dx + W] |= hit
    far = ~reach[:, 1:-1, 1:-1]
    assert_bits_equal(sick.reshape(c.B, H, W)[far], clean.reshape(c.B, H, W)[far], what + ": soft coverage away from the poisoned vertices")
    # ... and with vertices moved onto the segment between two centres (ConsumerCase.vertex_on_segment): two edges tie on s inside
    # (0, 1), and the lowest k decides which vertices the terms go to
    run(c.vertex_on_segment(ti), what + ", vertices on a segment", (0, 1), False)
    return keep, want


def check_albedo_fit(c, planes, what):
    """The per-face albedo fit on the case's table (bad ids: +0 basis rows) and plane (counted iff 0 <= (int)tri_ind < ntri), with the
    oracle's normal as it comes.  The basis bit for bit; the count exact; every moment the model (fsum of the rounded products) has
    finite within gamma(H W) sum |x_i x_j| of it -- tests/test_albedo_lse_gpu.py::test_moments_and_solve's bound.  A non-finite x
    stays in its face (test_poisoned_face's rule): where the model's moment is not finite the kernel's is the same NaN or the same Inf
    -- a sum of products holding a NaN, or Infs of both signs, is NaN in any order, and one holding Infs of one sign is that Inf --
    the count is unchanged and the face fails.  The moments are symmetric and repeat on a second launch.  alpha is not asserted
    (most scenes are rank-deficient by construction; the solve has its own tests), the failure flag is: on a face whose moments are
    all finite it is ref_albedo_lse.solve_ref's on the kernel's own moments.  The ridge is 0 on even seeds, 1e-6 on odd ones."""
    B, H, W, K = c.B, c.H, c.W, c.K
    tind, normal = planes[3].reshape(B, H, W, 1), planes[2]
    basis_w = RA.basis_ref(c.tri, c.pc_tex)
    basis = raw_basis(_t(c.tri), _t(c.pc_tex), c.nver)
    assert_f64_bits_equal(basis.cpu().numpy(), basis_w, what + ": albedo basis")
    inp = dict(basis=basis, tri_ind=_t(tind), lighting=_t(c.lighting.reshape(3, H, W), np.float64), normal=_t(normal),
               abedo=_t(c.abedo), im_gray=_t(c.im_gray))
    ridge = (0.0, 1e-6)[c.seed % 2]
    alpha, stats, M = raw_fit(inp, ridge)
    x, counted = RA.pixel_x(basis_w, tind, c.lighting, normal, c.abedo, c.im_gray)
    with np.errstate(invalid="ignore"):                                       # (Infs of both signs in one sum)
        RM, RS_ = RA.moments_fsum(x)
    assert np.array_equal(stats[:, 0], counted.sum(1).astype(np.float64)), what + ": albedo fit count"
    fin = np.isfinite(RM)
    with np.errstate(invalid="ignore"):
        err = np.abs(M - RM)
    assert (err[fin] <= (RA.gamma(H * W) * RS_)[fin]).all(), what + ": albedo fit moments"
    assert np.array_equal(np.isnan(M), np.isnan(RM)), what + ": albedo fit, the NaN moments"
    assert np.array_equal(M[~fin & ~np.isnan(RM)], RM[~fin & ~np.isnan(RM)]), what + ": albedo fit, the Inf moments"
    assert_f64_bits_equal(M, np.transpose(M, (0, 2, 1)), what + ": albedo fit, symmetry")
    assert_f64_bits_equal(raw_fit(inp, ridge)[2], M, what + ": albedo fit, two launches")
    for b in range(B):
        if fin[b].all():
            assert stats[b, 3] == RA.solve_ref(M[b], K, ridge, stats[b, 0])[3], "%s: albedo fit, face %d's failure flag" % (what, b)
        else:
            assert stats[b, 3] == 0.0 and not alpha[b].view(np.uint32).any(), "%s: albedo fit, poisoned face %d" % (what, b)


def check_operator_surface(c, normal_part, depth_part, tex_part, cov_part, what):
    """the wiring, not the arithmetic: render_depth with the three flags and all three gradients arriving in one backward"""
    B, H, W = c.B, c.H, c.W
    v = _t(c.ver).requires_grad_(True)
    tx = _t(c.tex).requires_grad_(True)
    tri = _t(c.tri)
    outs = ops().render_depth(v, tri, tx, torch.zeros((B, H, W, 3), device=DEV), normal_grad=True, texture_grad=True,
                              depth_interp=True)
    gd, gt, gn = _t(c.g_depth[0].reshape(B, H, W, 1)), _t(c.g_tex[0].reshape(B, H, W, 3)), _t(c.g_normal[0].reshape(B, H, W, 3))
    torch.autograd.backward([outs[0], outs[1], outs[2]], [gd, gt, gn])
    ti = outs[3].detach()
    raw = dbwd(gd, v.detach(), tri, ti, H, W)
    nbwd(gn, v.detach(), tri, ti, H, W, 0, out=raw, accumulate=1)
    fin = _finite_faces(normal_part[1], depth_part[1])
    assert_bits_equal(v.grad.cpu().numpy()[fin], raw.cpu().numpy()[fin], what + ": ver.grad through render_depth")
    with np.errstate(invalid="ignore"):                                        # (a face with Inf terms of both signs is not in `fin`)
        want = (depth_part[0] + normal_part[0])[fin]                           # the same two results, one fp32 add per element
    assert_bits_equal(v.grad.cpu().numpy()[fin], want, what + ": ver.grad against the raw calls on the oracle's planes")
    good = ~tex_part[1].bad                                                    # (a scope with a non-finite term has no bits to repeat)
    assert tuple(tx.grad.shape) == tuple(c.tex.shape)
    assert_bits_equal(tx.grad.cpu().numpy()[good], tex_part[0][good], what + ": texture.grad through render_depth")
    # ops.soft_coverage under autograd on the rendered tri_ind: the model's plane, and the raw backward's bits on the finite faces
    (got, R), want = cov_part
    v2 = _t(c.ver).requires_grad_(True)
    cov = ops().soft_coverage(v2, tri, ti)
    assert_bits_equal(cov.detach().cpu().numpy(), want, what + ": ops.soft_coverage")
    cov.backward(_t(c.g_cov[0].reshape(B, H, W, 1)))
    assert_bits_equal(v2.grad.cpu().numpy()[_finite_faces(R)], got[_finite_faces(R)], what + ": ver.grad through ops.soft_coverage")


def run_case(c, oracle, what):
    want = oracle.render_depth(c.ver, c.tri, c.tex, c.H, c.W)
    assert_render_equal(render_gpu(c.ver, c.tri, c.tex, c.H, c.W), want, what)
    ti = want[3].reshape(c.B, c.H * c.W)
    normal_part = check_normal_backward(c, ti, what)
    depth_part = check_depth_interp(c, ti, what)
    tex_part = check_texture_backward(c, ti, what)
    check_mesh(c, want, what)
    check_shade_and_photo_loss(GRAY, c, want, what)
    cov_part = check_coverage(c, ti, what)
    check_shade_and_photo_loss(RGB, c, want, what)
    check_albedo_fit(c, want, what)
    check_operator_surface(c, normal_part, depth_part, tex_part, cov_part, what)
    # a second pass on what the rasteriser never emits (fuzz_scenes.ConsumerCase.altered): bad ids in triangles that DO win pixels,
    # and NaN / ntri / fractional / -0.0 entries in the plane -- the pixels on which the consumers' two rules part.  Every consumer
    # must treat them as its header paragraph and its model do; one gradient profile, by the seed's parity
    a, ti2 = c.altered(ti)
    what, one = what + ", altered table and plane", (c.seed % 2,)
    planes2 = (want[0], want[1], want[2], ti2.reshape(want[3].shape))
    check_normal_backward(a, ti2, what, one)
    check_depth_interp(a, ti2, what, one)
    check_texture_backward(a, ti2, what, one)
    check_mesh(a, planes2, what)
    check_shade_and_photo_loss(GRAY, a, planes2, what)
    check_coverage(a, ti2, what, one)
    check_shade_and_photo_loss(RGB, a, planes2, what)
    check_albedo_fit(a, planes2, what)


@pytest.mark.parametrize("seed", range(N_CASES))
def test_consumers_of_tri_ind(oracle, seed):
    c = FS.ConsumerCase(seed)
    run_case(c, oracle, "consumer fuzz %d (scene %d, %s)" % (seed, c.drawn_from, FS.KINDS[c.kind]))


def test_consumers_on_the_texture_clamp_scene(oracle):
    """the class no seed reaches (tests/test_fuzz_scenes_cpu.py): tex_img below the shader's clamp under covered pixels"""
    run_case(FS.clamp_scene(), oracle, "the texture clamp scene")
