"""The reference's training objective (nets/network.py:336-392, 420-462) on PyTorch-ROCm -- the caller of the hot path in
BASELINE.json config 4.  Stock torch ops, except where the objective itself calls the hot path:

  * the geometry loss's basis product [pc_shape | pc_exp] . coeff (network.py:347-353) runs on the MFMA decode kernel
    (FaceRecNet.geometry_product) -- or, opt-in (geometry_gram=True), on no pass of the basis at all: the loss is a quadratic
    form in the coefficient differences, evaluated from the basis's Gram matrix (FaceRecNet.geometry_loss(gram=True)) -- and
  * the shape-from-shading model issues two more render_depth calls (network.py:423, 454 through compute_abedo_image), and
  * opt-in (fine_fused=True), the fidelity and the smoothness term of the fine depth map are one kernel pass per direction
    (rendering_layer/ops.py::fine_depth_losses) instead of a chain of elementwise ops, a convolution and two reductions, and
  * opt-in (photo_light / photo_alpha), a photometric term compares the face rendered and shaded under a given lighting and albedo
    with the picture itself (photometric_loss: synth_texture -> render_depth -> rendering_layer/ops.py::photo_loss), with a
    gradient to the geometry, the lighting and the albedo coefficients, and
  * opt-in (silhouette_mask), a silhouette term compares the soft coverage of the rendered face with a target mask
    (silhouette_loss: FaceRecNet.soft_mask -> rendering_layer/ops.py::soft_coverage), with a gradient to x and y of the vertices.

Names and weights follow the reference: pose MSE (lambda 1e-3), geometry MSE through the basis (1e-6), spherical
harmonics / SfS MSE (1e-3), fidelity MSE between the coarse and the fine depth map (100), Laplacian-L1 smoothness (1e-5)
(network.py:27-31, 373).

Batch sharding: every term but one is a mean / sum over independent faces, so a data-parallel shard
computes its share and DDP averages the gradients.  The exception is the SfS lighting estimate: the reference solves ONE
per-pixel least squares over the whole batch (network.py:430-434: (Y Y^T)^+ Y (I/(albedo+1))^T with Y = [3 x B] normals
of that pixel), so under batch sharding each rank's lighting is estimated from its own B/world faces -- a different
(noisier) estimator, not a bug; `get_spherical_harmonics_model(..., gather=True)` all-gathers the per-pixel normal,
intensity and albedo planes first and reproduces the single-process estimate (one all-gather of 4 floats per pixel per
face, no gradient through the gathered remote shards, like the reference's py_func pinv has none).  That route stays on
stock torch, every rank repeats the pinv and the matmuls over all faces, and rank i never receives the part of rank j's
loss that passes through the shared lighting into rank i's normals.  `fused_gather=True` (with gather and fused; opt-in)
exchanges the per-pixel SUMS instead -- nine float64 planes per rank forward, three backward -- around the fused kernels
(rendering_layer/ops.py::sfs_intensity_sharded): the same whole-batch estimate on every rank, bit for bit, and a
DDP-averaged gradient equal to the single-process one.
"""
import torch
import torch.nn.functional as F

LAMBDA_POSE = 1e-3   # network.py:27
LAMBDA_GEO = 1e-6    # :28
LAMBDA_SH = 1e-3     # :29
LAMBDA_F = 100.0     # :30
LAMBDA_SM = 1e-5     # :31

_LAPLACE_K = ((0.5, 1.0, 0.5), (1.0, -6.0, 1.0), (0.5, 1.0, 0.5))  # network.py:383-385


def laplace_transform(x):
    """2-D Laplacian of (H,W) or (B,H,W) maps with the reference's 3x3 kernel, zero 'SAME' padding (network.py:381-392)."""
    single = x.dim() == 2
    xx = x[None] if single else x
    k = torch.tensor(_LAPLACE_K, dtype=xx.dtype, device=xx.device)[None, None]
    y = F.conv2d(xx[:, None], k, padding=1)[:, 0]
    return y[0] if single else y


def _pinv_sym3(A, rtol=1e-15):
    """Moore-Penrose inverse of a batch of symmetric 3x3 matrices (the reference calls np.linalg.pinv on Y Y^T through
    tf.py_func, network.py:431: cutoff 1e-15 x the largest singular value, no gradient)."""
    return torch.linalg.pinv(A.detach(), rtol=rtol, hermitian=True)


def _ops():
    """rendering_layer/ops.py, loaded by path under the name nets/network.py uses: one module, however this file was imported"""
    import importlib.util
    import os
    import sys
    mod = sys.modules.get("_fr_hotpath_ops")
    if mod is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rendering_layer", "ops.py")
        spec = importlib.util.spec_from_file_location("_fr_hotpath_ops", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["_fr_hotpath_ops"] = mod
        spec.loader.exec_module(mod)
    return mod


def _world_size():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _all_gather_batch(t):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return t
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t.detach().contiguous())
    parts[dist.get_rank()] = t  # keep the local shard differentiable
    return torch.cat(parts, dim=-1)


def spherical_harmonics_intensity(abedo_image, normal_map, im_gray, abedo_image_new, normal_map_new, gather=False, fused=False,
                                  rcond=1e-15, tex_grad=False, fused_gather=False):
    """The linear-algebra core of get_spherical_harmonics_model (network.py:424-460) on already rendered maps:
    per pixel, lighting l = (Y Y^T)^+ Y (I / (albedo + 1))^T over the batch (Y = [3 x B] normals), then the recovered
    intensity albedo_new * (l^T Y_new).  All inputs [B,H,W,c]; returns [B,H,W,1].
    rcond: the pseudo-inverse's cutoff relative to the largest eigenvalue (the reference's 1e-15).
    fused=True: the whole expression is one kernel pass (rendering_layer/ops.py::sfs_intensity, fr_sfs_intensity_forward): float64
    sums in a fixed order, gradients to the two normal maps with the pseudo-inverse held constant -- the same autograd semantics
    as this torch route, whose pinv is detached.  The albedos and im_gray are constants of that call (they are detached here; in
    this model neither has a path to a parameter).  gather=True under a world size above 1 stays on the torch route even with
    fused=True: the per-pixel sums would have to cross ranks, which that kernel does not do (fused_gather below does).
    tex_grad=True: on the fused route abedo_image_new is no longer detached and receives its gradient, the lighting held constant
    (sfs_intensity(abedo_grad=True)); the torch route differentiates abedo_image_new anyway, so the flag changes nothing there.
    fused_gather=True (requires gather and fused, else ValueError): the whole-batch estimate on the fused kernels at any world
    size (sfs_intensity_sharded): the ranks all-gather nine float64 planes of per-pixel sums in the forward and three in the
    backward instead of their maps, and the backward uses the total q, so the DDP-averaged gradient is the single-process
    gradient (the torch gather route keeps only the local shard differentiable).  Every rank must make the same call and run the
    backward (it holds a collective); with no process group it equals fused=True bit for bit.  Works with tex_grad."""
    if fused_gather:
        if not (gather and fused):
            raise ValueError("fused_gather=True needs gather=True and fused=True")
        return _ops().sfs_intensity_sharded(abedo_image.detach(), normal_map, im_gray.detach(),
                                            abedo_image_new if tex_grad else abedo_image_new.detach(), normal_map_new,
                                            rcond=rcond, abedo_grad=bool(tex_grad))
    if fused and tex_grad and not (gather and _world_size() > 1):
        return _ops().sfs_intensity(abedo_image.detach(), normal_map, im_gray.detach(), abedo_image_new, normal_map_new,
                                    rcond=rcond, abedo_grad=True)
    if fused and not (gather and _world_size() > 1):
        return _ops().sfs_intensity(abedo_image.detach(), normal_map, im_gray.detach(), abedo_image_new.detach(), normal_map_new,
                                    rcond=rcond)
    abedo = abedo_image.permute(1, 2, 3, 0)            # (H,W,1,B)
    Yz0 = normal_map.permute(1, 2, 3, 0)               # (H,W,3,B)
    I = im_gray.permute(1, 2, 3, 0)                    # (H,W,1,B)
    rhs = I / (abedo + 1.0)
    Yl, rl = (Yz0, rhs) if not gather else (_all_gather_batch(Yz0), _all_gather_batch(rhs))
    Yz0_nec_inv = _pinv_sym3(Yl @ Yl.transpose(-1, -2), rcond)                                  # (H,W,3,3)
    lighting_lse = (Yz0_nec_inv @ Yl) @ rl.transpose(-1, -2)                               # (H,W,3,1)
    Yz = normal_map_new.permute(1, 2, 3, 0)
    intensity = abedo_image_new.permute(1, 2, 3, 0) * (lighting_lse.transpose(-1, -2) @ Yz)  # Eqn (8), (H,W,1,B)
    return intensity.permute(3, 0, 1, 2)


def get_spherical_harmonics_model(face_net, vertices_proj, im_gray, gather=False, normal_grad=False, fused=False, rcond=1e-15,
                                  tex_grad=False, fused_gather=False, fine_depth=None, alpha_lse=False, alpha_ridge=1e-6):
    """Recovered intensity (B,H,W,1) of the first-order spherical-harmonics shading model (network.py:420-462): two
    more render_depth calls (mean albedo, then mean + pc_tex . param_tex) feed spherical_harmonics_intensity.
    normal_grad=False (default): as the reference, both renders hand autograd constant normal maps, so the term has no gradient
    with respect to any parameter.  normal_grad=True: both renders carry the normal map's gradient to the vertices
    (render_depth(normal_grad=True)) and the term moves the geometry.  fused / rcond: as spherical_harmonics_intensity.
    tex_grad=True: the second render, the one of texture_new, carries the albedo image's gradient to the texture
    (render_depth(texture_grad=True)), hence to face_net.param_tex where that requires grad; the render of the mean texture
    stays a constant.
    fused_gather=True (requires gather and fused, else ValueError): as spherical_harmonics_intensity; works with normal_grad and
    tex_grad.
    fine_depth ([B,H,W,1], default None): the predicted fine depth map.  When given, the shaded normals are ITS normals on the pixel
    grid -- depth_normals(fine_depth, mask = tri_ind of the second render) -- instead of the second render's normal map, which is
    the coarse mesh's a second time (the reference's own complaint, network.py:451-453); the term then constrains the fine depth
    and its gradient reaches fine_depth.  The lighting still comes from the first render and abedo_new from the second.  Works with
    every flag above (the gradient of the shaded normals is local to the rank).
    alpha_lse=True (default off; alpha_ridge: its ridge, relative to the mean diagonal of a face's Gram matrix): texture_new is no
    longer mean + pc_tex . param_tex, one albedo for every face, but PER FACE mean + pc_tex . alpha_b with alpha_b the least-squares
    fit of that face's own SfS residual given the lighting -- the estimate the reference wanted and gave up (network.py:436-455).
    The first render also returns its tri_ind, the map from pixels to rows of the texture basis; the shaded normals are chosen
    (the render's own, or depth_normals(fine_depth, mask = that tri_ind)); sfs_lighting gives l; albedo_lse fits alpha_b
    (rendering_layer/ops.py); the second render and spherical_harmonics_intensity then run as above.  alpha_b is a fitted
    quantity held constant in the backward, like the lighting's pseudo-inverse.  Works with fused, rcond, normal_grad and
    fine_depth; each rank fits its own faces (no collective).  ValueError unless fused (the lighting must be the fused solve's),
    with tex_grad (param_tex is no longer what the term uses), and with gather or fused_gather (the whole-batch lighting across
    ranks is not served)."""
    fn = face_net
    if fused_gather and not (gather and fused):
        raise ValueError("fused_gather=True needs gather=True and fused=True")
    if alpha_lse:
        if not fused:
            raise ValueError("alpha_lse=True needs fused=True (the fit uses the fused solve's lighting)")
        if tex_grad:
            raise ValueError("alpha_lse=True excludes tex_grad=True (param_tex is no longer what the term uses)")
        if gather or fused_gather:
            raise ValueError("alpha_lse=True excludes gather / fused_gather (the whole-batch lighting across ranks is not served)")
    if fn.mu_tex is None or fn.pc_tex is None or fn.param_tex is None:
        raise ValueError("the asset dict has no texture model (mu_tex / pc_tex / param_tex)")
    kw = {"normal_grad": True} if normal_grad else {}
    if alpha_lse:
        return _sfs_model_alpha_lse(fn, vertices_proj, im_gray, kw, normal_grad, rcond, fine_depth, alpha_ridge)
    abedo_image, normal_map = fn.compute_abedo_image(vertices_proj, fn.tri, fn.mu_tex, **kw)   # (B,H,W,1), (B,H,W,3)
    texture_new = fn.mu_tex + (fn.pc_tex @ fn.param_tex).reshape(3, -1)                    # network.py:446-448
    kw_new = dict(kw, texture_grad=True) if tex_grad else kw
    if fine_depth is None:
        abedo_new, normal_new = fn.compute_abedo_image(vertices_proj, fn.tri, texture_new, **kw_new)
    else:
        abedo_new, _, tri_ind_new = fn.compute_abedo_image(vertices_proj, fn.tri, texture_new, with_tri_ind=True, **kw_new)
        normal_new = _ops().depth_normals(fine_depth, mask=tri_ind_new.detach())
    if fused and not normal_grad:
        # the renders' normal maps are constants to autograd in this mode (their node drops the gradient): say so, and the fused
        # node runs no backward at all -- unless the shaded normals are the fine depth map's, which are not constants
        normal_map = normal_map.detach()
        if fine_depth is None:
            normal_new = normal_new.detach()
    if not (fused or rcond != 1e-15):
        return spherical_harmonics_intensity(abedo_image, normal_map, im_gray, abedo_new, normal_new, gather=gather)
    kw_tex = {"tex_grad": True} if tex_grad else {}
    if fused_gather:
        kw_tex["fused_gather"] = True
    return spherical_harmonics_intensity(abedo_image, normal_map, im_gray, abedo_new, normal_new, gather=gather, fused=fused,
                                         rcond=rcond, **kw_tex)


def _sfs_model_alpha_lse(fn, vertices_proj, im_gray, kw, normal_grad, rcond, fine_depth, ridge):
    """get_spherical_harmonics_model(alpha_lse=True, fused=True): the steps of its docstring, in order"""
    ops = _ops()
    abedo_image, normal_map, tri_ind = fn.compute_abedo_image(vertices_proj, fn.tri, fn.mu_tex, with_tri_ind=True, **kw)
    tri_ind = tri_ind.detach()
    shaded = normal_map if fine_depth is None else ops.depth_normals(fine_depth, mask=tri_ind)
    lighting = ops.sfs_lighting(abedo_image, normal_map, im_gray, rcond=rcond)
    alpha, _ = ops.albedo_lse(fn.albedo_basis(), tri_ind, lighting, shaded, abedo_image, im_gray, ridge=ridge)
    texture_new = fn.mu_tex[None] + (alpha @ fn.pc_tex.t()).reshape(alpha.shape[0], 3, -1)     # [B,3,N]: one albedo per face
    if fine_depth is None:
        abedo_new, normal_new = fn.compute_abedo_image(vertices_proj, fn.tri, texture_new, **kw)
    else:
        abedo_new, _, tri_ind_new = fn.compute_abedo_image(vertices_proj, fn.tri, texture_new, with_tri_ind=True, **kw)
        normal_new = ops.depth_normals(fine_depth, mask=tri_ind_new.detach())
    if not normal_grad:
        normal_map = normal_map.detach()
        if fine_depth is None:
            normal_new = normal_new.detach()
    return spherical_harmonics_intensity(abedo_image, normal_map, im_gray, abedo_new, normal_new, fused=True, rcond=rcond)


def photometric_loss(face_net, vertices_proj, im_gray, light, alpha, weight=None, gain=1.0, offset=0.0):
    """The analysis-by-synthesis term: the mean over the covered pixels of weight (I^ - im_gray)^2, with I^ the face of
    vertices_proj [B,3,N] rendered with the per-face albedo mu_tex + pc_tex . alpha_b and shaded under the first-order lighting
    light [B,4] -- the image pipeline.SynthBatches makes of the same quantities, bit for bit (gain, offset: that stream's).
    synth_texture -> render_depth(normal_grad=True, texture_grad=True) -> photo_loss (rendering_layer/ops.py): the gradient reaches
    vertices_proj (x, y and z, through the normal map; tri_ind held fixed), light and alpha, wherever they require grad.  im_gray
    [B,H,W,1] and weight (None = 1) are constants.  -> a 0-dim float64 tensor, sse.sum() / count.sum().clamp_min(1); each rank
    takes the mean over its own faces (no collective).
    COLOUR (opt-in, chosen by light's shape): with light [B,3,9] -- per-channel albedo under a second-order lighting per channel, the
    image pipeline.SynthBatches(colour=True) makes -- the picture in im_gray's place is the colour one, im_rgb [B,H,W,3] (a
    constant), the term compares in colour through rendering_layer/ops.py::photo_loss_rgb, and is
    sse.sum() / (3 count.sum()).clamp_min(1): the mean over the covered pixels' channels.  ValueError where the lighting and the
    picture do not go together (a [B,3,9] lighting with a one-channel picture, a [B,4] lighting with a three-channel one).  With
    light [B,4] every bit is the gray route's."""
    fn = face_net
    if fn.mu_tex is None or fn.pc_tex is None:
        raise ValueError("the asset dict has no texture model (mu_tex / pc_tex)")
    colour = light.dim() == 3
    channels = int(im_gray.shape[-1]) if im_gray.dim() == 4 else 1
    if colour and (tuple(light.shape[1:]) != (3, 9) or channels != 3):
        raise ValueError("the colour route (light [B,3,9]) needs the colour picture im_rgb [B,H,W,3]; got light %s and a picture %s"
                         % (tuple(light.shape), tuple(im_gray.shape)))
    if not colour and channels == 3:
        raise ValueError("a colour picture im_rgb [B,H,W,3] goes with a colour lighting [B,3,9]; light is %s" % (tuple(light.shape),))
    ops = _ops()
    tex = ops.synth_texture(fn.mu_tex, fn.pc_tex, alpha)
    _, tex_img, normal, tri_ind = ops.render_depth(vertices_proj.float(), fn.tri, tex, im_gray, normal_grad=True, texture_grad=True)
    if colour:
        sse, count = ops.photo_loss_rgb(tex_img, normal, tri_ind.detach(), light, im_gray.detach(), weight, gain, offset)
        return sse.sum() / (3 * count.sum()).clamp_min(1)
    sse, count = ops.photo_loss(tex_img, normal, tri_ind.detach(), light, im_gray.detach(), weight, gain, offset)
    return sse.sum() / count.sum().clamp_min(1)


def photometric_loss_smooth(face_net, vertices_proj, picture, light, alpha, weight=None, gain=1.0, offset=0.0):
    """photometric_loss over SMOOTH planes (opt-in; photometric_loss itself is unchanged): the render gives tri_ind alone, held
    fixed, and the two planes shaded are FaceRecNet.smooth_planes -- the per-face albedo and the vertex normals interpolated at the
    pixel, not the winning facet's.  The gradient reaches vertices_proj through x and y (both planes) and through the vertex
    normals (x, y and z), and light and alpha as there.  `picture` is im_gray [B,H,W,1] with light [B,4] or im_rgb [B,H,W,3] with
    light [B,3,9]; it should itself be shaded from smooth planes (examples/photo_fit.py --smooth does so).  -> a 0-dim float64
    tensor, normalised as photometric_loss."""
    fn = face_net
    if fn.mu_tex is None or fn.pc_tex is None:
        raise ValueError("the asset dict has no texture model (mu_tex / pc_tex)")
    colour = light.dim() == 3
    channels = int(picture.shape[-1]) if picture.dim() == 4 else 1
    if colour != (channels == 3) or (colour and tuple(light.shape[1:]) != (3, 9)):
        raise ValueError("light [B,4] goes with a one-channel picture and light [B,3,9] with im_rgb [B,H,W,3]; got light %s and a "
                         "picture %s" % (tuple(light.shape), tuple(picture.shape)))
    ops = _ops()
    tex = ops.synth_texture(fn.mu_tex, fn.pc_tex, alpha)
    ver = vertices_proj.float()
    with torch.no_grad():
        B, H, W = int(picture.shape[0]), int(picture.shape[1]), int(picture.shape[2])
        image = torch.zeros((B, H, W, 3), dtype=torch.float32, device=ver.device)
        tri_ind = ops.render_depth(ver.detach(), fn.tri, fn.vertex_code, image)[3]
    tex_img, normal = fn.smooth_planes(ver, tex, tri_ind)
    if colour:
        sse, count = ops.photo_loss_rgb(tex_img, normal, tri_ind, light, picture.detach(), weight, gain, offset)
        return sse.sum() / (3 * count.sum()).clamp_min(1)
    sse, count = ops.photo_loss(tex_img, normal, tri_ind, light, picture.detach(), weight, gain, offset)
    return sse.sum() / count.sum().clamp_min(1)


def silhouette_loss(face_net, vertices_proj, target_mask):
    """The mean squared difference between the soft silhouette of the face of vertices_proj [B,3,N] (FaceRecNet.soft_mask: one
    render for tri_ind, then rendering_layer/ops.py::soft_coverage) and target_mask ([B,H,W,1] or [B,H,W], e.g. the `mask` of
    pipeline.SynthBatches; a constant: it gets no gradient).  The gradient reaches the x and y rows of vertices_proj -- the only
    term that tells a fit where the face is in the picture.  Stock torch on one plane after the kernel; each rank takes the mean
    over its own faces (no collective)."""
    cov = face_net.soft_mask(vertices_proj)
    target = target_mask.detach().to(cov.dtype).reshape(cov.shape)
    return F.mse_loss(cov, target)


def landmark_loss(face_net, pred_params, idx, target, weight=None, pose_grad=True, lines=None, line_target=None, line_weight=None):
    """The landmark term: the mean over faces of sse_b / max(sum_k w_k, 1), with sse_b the weighted squared pixel distance between
    the projections of the vertices `idx` under pred_params ((B,d) or (B,1,1,d)) and target [B,K,2] (x, y; a constant).  weight:
    None (= 1), [K] or [B,K] (e.g. the `landmark_visible` of pipeline.SynthBatches); a landmark of weight 0 is skipped entirely and
    may carry a NaN target.  FaceRecNet.landmark_basis(idx) -> rendering_layer/ops.py::landmark_sse: the dense basis is not read and
    no [B,3,N] tensor exists; one launch each way.  The gradient reaches pred_params -- the angles too unless pose_grad=False.
    -> a 0-dim float64 tensor; each rank takes the mean over its own faces (no collective).
    lines [C,M] with line_target [B,C,2] (default None: the code path and every bit are today's; one without the other is a
    ValueError) and line_weight (None = 1, [C] or [B,C]): contour landmarks that slide.  Each line of candidate vertex ids is held to
    its 2D point through the candidate that projects nearest to it under pred_params (FaceRecNet.landmark_contour_basis(idx, lines)
    -> rendering_layer/ops.py::landmark_contour_sse); the selection is a constant of the step.  idx, target and weight then belong
    to the fixed landmarks (idx may be empty with target None), and the divisor is the sum of both kinds' weights."""
    fn = face_net
    B = pred_params.shape[0]
    pred = pred_params.reshape(B, fn.ndim)
    if (lines is None) != (line_target is None) or (lines is None and line_weight is not None):
        raise ValueError("lines and line_target go together: the candidate vertices of every contour point and the 2D points")

    def weight_sum(w, count, dev):
        if w is None:
            return torch.full((B,), float(count), dtype=torch.float64, device=dev)
        w = w.detach().to(device=dev, dtype=torch.float64)
        return w.sum().expand(B) if w.dim() == 1 else w.sum(dim=1)
    if lines is not None:
        lb = fn.landmark_contour_basis(idx, lines)
        sse = _ops().landmark_contour_sse(pred, lb, line_target, line_weight=line_weight, fixed_target=target, fixed_weight=weight,
                                          im_size=fn.im_size, pose_grad=pose_grad)
        wsum = weight_sum(weight, lb.n_fixed, sse.device) + weight_sum(line_weight, lb.C, sse.device)
        return (sse / wsum.clamp_min(1.0)).mean()
    lb = fn.landmark_basis(idx)
    sse = _ops().landmark_sse(pred, lb, target, weight=weight, im_size=fn.im_size, pose_grad=pose_grad)
    if weight is None:
        wsum = torch.full((B,), float(lb.K), dtype=torch.float64, device=sse.device)
    else:
        w = weight.detach().to(device=sse.device, dtype=torch.float64)
        wsum = w.sum().expand(B) if w.dim() == 1 else w.sum(dim=1)
    return (sse / wsum.clamp_min(1.0)).mean()


def combine_losses(losses):
    """total = 1e-3 pose + 1e-6 geometry + 1e-3 SfS + 100 fidelity + 1e-5 smoothness (network.py:27-31, 373)"""
    return (LAMBDA_POSE * losses['pose_loss'] + LAMBDA_GEO * losses['geometry_loss'] +
            LAMBDA_SH * losses['spherical_harmonics_loss'] + LAMBDA_F * losses['fidelity_loss'] +
            LAMBDA_SM * losses['smoothness_loss'])


def get_loss(face_net, pred_params, params_label, im_gray, vertices_proj, coarse_depth_map, pred_depth_map,
             gather_sfs=False, sfs_normal_grad=False, sfs_fused=False, sfs_rcond=1e-15, sfs_tex_grad=False,
             sfs_fused_gather=False, sfs_fine=False, fine_fused=False, sfs_alpha_lse=False, sfs_alpha_ridge=1e-6,
             silhouette_mask=None, lambda_silhouette=1.0,
             landmark_target=None, landmark_idx=None, landmark_weight=None, lambda_landmark=1.0, landmark_lines=None,
             landmark_line_target=None, landmark_line_weight=None, photo_target_rgb=None,
             photo_light=None, photo_alpha=None, photo_weight=None, photo_gain=1.0, photo_offset=0.0, lambda_photo=1.0,
             geometry_gram=False):
    """dict of the reference's six scalars (network.py:336-378).  pred_params / params_label: (B,d) or (B,1,1,d).
    sfs_normal_grad / sfs_fused / sfs_rcond (defaults: off, off, the reference's 1e-15): the normal_grad / fused / rcond of
    get_spherical_harmonics_model.  With them off spherical_harmonics_loss is a reported scalar with no gradient, as in the
    reference; sfs_normal_grad=True lets it reach the vertices through the two SfS renders.
    sfs_tex_grad=True (default off): the term also reaches the albedo coefficients face_net.param_tex, where that tensor requires
    grad (FaceReconModel(learn_tex=True)), through the render of texture_new.
    sfs_fused_gather=True (default off; needs gather_sfs and sfs_fused, else ValueError): the whole-batch lighting estimate on
    the fused kernels under any world size, the ranks exchanging per-pixel sums (get_spherical_harmonics_model(fused_gather=True)).
    sfs_fine=True (default off): the term shades the normals of pred_depth_map instead of the coarse mesh's a second time
    (get_spherical_harmonics_model(fine_depth=pred_depth_map)), so spherical_harmonics_loss has a gradient with respect to
    pred_depth_map on either route; ValueError when pred_depth_map is None.
    geometry_gram=True (default off): geometry_loss comes from the Gram matrix of the basis (FaceRecNet.geometry_loss(gram=True)):
    the same quantity, from float64 chains over 228 numbers per face instead of two passes over the basis; the second packed image
    of the basis is then never built.  Each rank takes the mean over its own faces, as on the default route: no collective.
    fine_fused=True (default off): fidelity_loss and smoothness_loss come from one autograd node (rendering_layer/ops.py::
    fine_depth_losses, fr_fine_losses_forward / _backward): the same two quantities as float64 sums in a fixed association, one
    kernel pass and a finish launch forward, one gather pass backward -- no convolution, no plane-sized intermediate.  The gradient
    reaches pred_depth_map and, where it requires grad, coarse_depth_map, as on the default route; ValueError when pred_depth_map
    is None.  Each rank sums over its own faces: no collective.
    sfs_alpha_lse=True / sfs_alpha_ridge (default off, 1e-6): the alpha_lse / alpha_ridge of get_spherical_harmonics_model -- the
    term's albedo is fitted per face instead of shared; needs sfs_fused, excludes sfs_tex_grad, gather_sfs and sfs_fused_gather
    (ValueError).
    photo_light [B,4] / photo_alpha [B,K] (default None: the term is absent, the dict and every bit are today's; one without the
    other is a ValueError): adds losses['photometric_loss'] = photometric_loss(face_net, vertices_proj, im_gray, photo_light,
    photo_alpha, photo_weight, photo_gain, photo_offset) -- the rendered and shaded face against im_gray itself -- and lambda_photo
    times it to total_loss.  Its gradient reaches vertices_proj, and photo_light / photo_alpha where they require grad.
    photo_target_rgb [B,H,W,3] (default None): the colour picture; photometric_loss then gets it in im_gray's place.  It goes with a
    colour photo_light [B,3,9] (ValueError otherwise), and the term compares in colour.
    silhouette_mask [B,H,W,1] (default None: the term is absent, the dict and every bit are today's): adds
    losses['silhouette_loss'] = silhouette_loss(face_net, vertices_proj, silhouette_mask) and lambda_silhouette times it to
    total_loss.  Its gradient reaches the x and y rows of vertices_proj; the mask is a constant.
    landmark_target [B,K,2] with landmark_idx (K vertex ids) (default None: the term is absent, the dict and every bit are today's;
    one without the other is a ValueError): adds losses['landmark_loss'] = landmark_loss(face_net, pred_params, landmark_idx,
    landmark_target, landmark_weight) and lambda_landmark times it to total_loss.  Its gradient reaches pred_params directly, the
    angles included; it does not go through vertices_proj.
    landmark_lines [C,M] with landmark_line_target [B,C,2] and landmark_line_weight (default None: absent; one of the first two
    without the other is a ValueError): the lines / line_target / line_weight of landmark_loss -- contour landmarks that slide, with
    or without fixed ones beside them."""
    fn = face_net
    if (landmark_target is None) != (landmark_idx is None):
        raise ValueError("landmark_target and landmark_idx go together: the 2D points and the vertices they belong to")
    if (landmark_lines is None) != (landmark_line_target is None) or (landmark_lines is None and landmark_line_weight is not None):
        raise ValueError("landmark_lines and landmark_line_target go together: the candidate vertices and the 2D points")
    if (photo_light is None) != (photo_alpha is None):
        raise ValueError("photo_light and photo_alpha go together: the photometric term needs the lighting and the albedo coefficients")
    if photo_target_rgb is not None and photo_light is None:
        raise ValueError("photo_target_rgb needs photo_light [B,3,9] and photo_alpha: it is the colour photometric term's picture")
    if fine_fused and pred_depth_map is None:
        raise ValueError("fine_fused=True needs pred_depth_map (the fine depth map the two terms are taken of)")
    B = pred_params.shape[0]
    pred = pred_params.reshape(B, fn.ndim)
    label = params_label.reshape(B, fn.ndim).to(pred.dtype)
    losses = {}
    losses['pose_loss'] = F.mse_loss(pred[:, :fn.ndim_pose], label[:, :fn.ndim_pose])
    # geometry: MSE(basis . label^T, basis . pred^T) == mean over (3N x B) of (basis . (pred - label)^T)^2 up to fp32
    # rounding of the two products; the difference form needs one pass of the basis instead of two
    if geometry_gram:
        losses['geometry_loss'] = fn.geometry_loss(pred[:, fn.ndim_pose:] - label[:, fn.ndim_pose:], gram=True)
    else:
        g = fn.geometry_product(pred[:, fn.ndim_pose:] - label[:, fn.ndim_pose:])
        losses['geometry_loss'] = (g * g).mean()
    kw_tex = {"tex_grad": True} if sfs_tex_grad else {}
    if sfs_fused_gather:
        kw_tex["fused_gather"] = True
    if sfs_fine:
        if pred_depth_map is None:
            raise ValueError("sfs_fine=True needs pred_depth_map (the fine depth map whose normals the term shades)")
        kw_tex["fine_depth"] = pred_depth_map
    if sfs_alpha_lse:
        kw_tex.update(alpha_lse=True, alpha_ridge=sfs_alpha_ridge)
    intensity_recover = get_spherical_harmonics_model(fn, vertices_proj, im_gray, gather=gather_sfs, normal_grad=sfs_normal_grad,
                                                      fused=sfs_fused, rcond=sfs_rcond, **kw_tex)
    losses['spherical_harmonics_loss'] = F.mse_loss(intensity_recover, im_gray)
    if fine_fused:
        losses['fidelity_loss'], losses['smoothness_loss'] = _ops().fine_depth_losses(pred_depth_map, coarse_depth_map)
    else:
        losses['fidelity_loss'] = F.mse_loss(pred_depth_map, coarse_depth_map)
        filtered_depth = laplace_transform(pred_depth_map[..., 0])
        losses['smoothness_loss'] = filtered_depth.abs().sum()    # tf.contrib.layers.l1_regularizer(1.0), network.py:367
    losses['total_loss'] = combine_losses(losses)
    if photo_light is not None:
        picture = im_gray if photo_target_rgb is None else photo_target_rgb
        losses['photometric_loss'] = photometric_loss(fn, vertices_proj, picture, photo_light, photo_alpha, weight=photo_weight,
                                                      gain=photo_gain, offset=photo_offset)
        losses['total_loss'] = losses['total_loss'] + (lambda_photo * losses['photometric_loss']).to(losses['total_loss'].dtype)
    if silhouette_mask is not None:
        losses['silhouette_loss'] = silhouette_loss(fn, vertices_proj, silhouette_mask)
        losses['total_loss'] = losses['total_loss'] + (lambda_silhouette * losses['silhouette_loss']).to(losses['total_loss'].dtype)
    if landmark_lines is not None:
        losses['landmark_loss'] = landmark_loss(fn, pred_params, landmark_idx, landmark_target, weight=landmark_weight,
                                                lines=landmark_lines, line_target=landmark_line_target,
                                                line_weight=landmark_line_weight)
        losses['total_loss'] = losses['total_loss'] + (lambda_landmark * losses['landmark_loss']).to(losses['total_loss'].dtype)
    elif landmark_target is not None:
        losses['landmark_loss'] = landmark_loss(fn, pred_params, landmark_idx, landmark_target, weight=landmark_weight)
        losses['total_loss'] = losses['total_loss'] + (lambda_landmark * losses['landmark_loss']).to(losses['total_loss'].dtype)
    return losses
