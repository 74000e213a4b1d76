"""Operator surface of the rendering layer -- the MI355X drop-in for the reference's rendering_layer/ops.py.

Same names and argument meaning as the reference module (rendering_layer/ops.py:12,23,78-95):

    OP_NAMES                       ['render_depth']
    compile(op=None)               build the native library (hipcc --offload-arch=gfx950, not nvcc + g++)
    render_depth(ver, tri, texture, image, **kwargs)
                                   -> (depth [B,H,W,1], texture_image [B,H,W,3], normal [B,H,W,3], tri_ind [B,H,W,1])
    gradient                       flows to `ver` only (d depth / d vertex z); tri, texture, image get None
                                   (opt-in: normal_grad=True, texture_grad=True, depth_interp=True -- see render_depth)

Tensors are torch.Tensors on an MI355X instead of tf.Tensors; the op is a torch.autograd.Function calling the
C ABI of include/fr_hotpath.h through ctypes on torch's current HIP stream.  Like the reference, importing the
module loads the native library and builds it first if the .so is missing (reference ops.py:63-72) -- but there
is no fallback path: no library or no GPU tensor => an exception.
"""
import collections
import ctypes
import importlib.util
import os
import sys
import weakref

import torch

# Register ops for compilation here (reference ops.py:12)
OP_NAMES = ['render_depth']

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host():
    """The ctypes host module (3dfacerecon_amd/_lib.py), loaded by path so that this file works both as
    `3dfacerecon_amd.rendering_layer.ops` and as the reference-style top-level `rendering_layer.ops`."""
    name = "_fr_hotpath_host"
    mod = sys.modules.get(name)
    if mod is None:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_PKG_DIR, "_lib.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod


def compile(op=None):
    """Build the native op library.  `op` is accepted for signature compatibility (reference ops.py:23-27);
    all ops of OP_NAMES live in one shared library."""
    if op is not None and op not in OP_NAMES:
        raise ValueError("unknown op %r (known: %s)" % (op, OP_NAMES))
    return _host().compile(force=True, verbose=True)


# build-on-import fallback, then load (reference ops.py:63-72).  A missing hipcc or a failing build raises here.
_host().lib()


# The buffers that live from call to call (_lib.StreamBuffers: its docstring has the rules).  Two pools, so that a small scratch
# kind cycling through never evicts a 330 MB render workspace and the triangle table packed into it.
WS_CACHE_MAX = 4
_RENDER_POOL = _host().stream_buffers("render", WS_CACHE_MAX, 16)
# What the autograd nodes and fits below keep per kind and stream: the pitched vertex hand-off of the decode -> rendering-layer
# forward ("hand"), the workspace of its backward ("bwd"), the partial sums of the losses and fits.
_KINDS_POOL = _host().stream_buffers("scratch", 8, 256)


def clear_workspace_cache():
    """Releases every pooled render workspace and scratch buffer (their memory returns to torch's caching allocator), with the
    record of which triangle list each workspace's table was packed from.  The pools are process-wide: this reaches what every
    load of this file uses -- the package's, and the one nets/network.py (FaceRecNet) and nets/losses.py load by path."""
    _RENDER_POOL.clear()
    _KINDS_POOL.clear()


# A render workspace's entry remembers in `note` which triangle list its pre-validated triangle table (pack_tri_kernel) was built
# from -- (a weak reference to the tensor OBJECT, (its torch version counter, its data_ptr, the option epoch) + the geometry) --
# so a loop that renders with the same `tri` tensor every call (the reference makes it a tf.constant, network.py:178) packs it
# once, not once per call.  A new tensor is never mistaken for an old one whose memory the caching allocator handed out again
# (object identity, not data_ptr); the version counter sees in-place torch writes; a caller that rewrites the tensor's memory
# behind torch's back must call clear_workspace_cache().
def _render_phases(ent, cached, tri_c, geom):
    """-> (phases, pending): phases = 7 (pack + emit + resolve), or 3 when the entry's triangle table was packed from this very
    list for this geometry under the launcher options in force now; `pending` is the record _table_packed() commits once the
    call that packs the table has RETURNED 0 (a failed or unsupported call leaves no claim about the table behind)."""
    # an inference tensor (created under torch.inference_mode()) has no version counter: in-place writes to it cannot be
    # seen, so its table is never reused -- packed every call, like a caller that passes a new tensor each time
    if tri_c.is_inference():
        ent.note = None
        return 7, None
    # (the option epoch: FR_RENDER_IMPL / FR_RENDER_ROWS / FR_EMIT_ORDER decide whether and how the table is written, and
    # can only change through _lib.set_option, which bumps it)
    key = (tri_c._version, tri_c.data_ptr(), _host().option_epoch()) + geom
    if cached and ent.note is not None and ent.note[0]() is tri_c and ent.note[1] == key:
        return 3, None
    ent.note = None   # whatever this call does, the old record no longer describes the table
    return 7, ((weakref.ref(tri_c), key) if cached else None)


def _table_packed(ent, pending):
    if pending is not None:
        ent.note = pending


def _render_with_workspace(dev, ws_bytes, tri_c, geom, call):
    """The step every render forward makes as one, inside a hold on the stream's workspace (decide the phases -> launch -> record
    the table: one thread's pack must not land between another's choice to skip it and that thread's launch): choose the phases,
    make the call -- call(workspace buffer, phases) -> rc -- and, where it returned 0, record the table it packed.  -> rc"""
    with _RENDER_POOL.hold("render", dev, ws_bytes) as ent:
        phases, pending = _render_phases(ent, ent.pooled, tri_c, geom)
        rc = call(ent.buf, phases)
        if rc == 0:
            _table_packed(ent, pending)
    return rc


def _check_ver(ver):
    if ver.dim() != 3 or ver.shape[1] != 3:
        raise ValueError("The vertex is not Batch x 3 x nver")


def _check_tri(tri):
    if tri.dim() != 2 or tri.shape[0] != 3:
        raise ValueError("The tri is not 3 x ntri")


def _check_plane(op, name, t, B, H, W, c, dev=None, anchor=None, flat=False):
    """ValueError unless `t` is a pixel plane [B,H,W,c] (flat: or [B,H,W]) and -- where `dev` is given -- on `dev`, the device of
    the op's argument `anchor`"""
    shapes = ((B, H, W, c), (B, H, W)) if flat else ((B, H, W, c),)
    if tuple(t.shape) not in shapes:
        raise ValueError("%s: %s must be %s (got %s)" % (op, name, " or ".join(str(list(s)) for s in shapes), tuple(t.shape)))
    if dev is not None and t.device != dev:
        raise ValueError("%s: %s is on %s, %s on %s" % (op, name, t.device, anchor, dev))


def _check_forward_shapes(ver, tri, texture, image):
    # the OP_REQUIRES checks of RenderDepthOp::Compute (render_depth_op.cc:397-418), same messages
    if image.dim() != 4 or ver.dim() != 3 or tri.dim() != 2 or texture.dim() not in (2, 3):
        raise ValueError("render_depth expects ver [B,3,nver], tri [3,ntri], texture [B,3,nver], image [B,H,W,C]")
    B = image.shape[0]
    if ver.shape[0] != B:
        raise ValueError("The vertex's batch is not the same as image batch")
    _check_ver(ver)
    _check_tri(tri)
    if texture.shape[-2] != 3:
        raise ValueError("The texture channel must be equal to image channel namely 3")
    if texture.shape[-1] != ver.shape[2]:
        raise ValueError("The texture is not Batch x 3 x nver")
    if texture.dim() == 3 and texture.shape[0] not in (1, B):
        raise ValueError("The texture's batch is neither 1 nor the image batch")


def _backward_call(h, g, tri_c, tri_ind, vertex_grad, B, nver, ntri, H, W, dev):
    """fr_render_depth_backward_ws with its workspace (one 16-byte record per pixel)."""
    L = h.lib()
    nws = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    ws = h.byte_buffer(nws, dev)
    rc = L.fr_render_depth_backward_ws(h.ptr(g), h.ptr(tri_c), h.ptr(tri_ind), h.ptr(vertex_grad), B, nver, ntri, H, W,
                                       h.ptr(ws), nws, h.stream_ptr(dev))
    h.check(rc, "fr_render_depth_backward")


def _normal_backward_call(h, g, g_offset, g_stride, ver_c, tri_c, tri_ind, vertex_grad, B, nver, ntri, H, W, mode, accumulate,
                          dev):
    """fr_render_normal_backward with its workspace (48 bytes per pixel): the gradient read at `g_offset` floats into `g`,
    `g_stride` floats between pixels; accumulate=1 completes a vertex_grad the depth backward has written on this stream."""
    L = h.lib()
    nws = L.fr_render_normal_backward_workspace_bytes(B, nver, H, W)
    ws = h.byte_buffer(nws, dev)
    rc = L.fr_render_normal_backward(ctypes.c_void_p(g.data_ptr() + 4 * g_offset), g_stride, h.ptr(ver_c), nver, h.ptr(tri_c),
                                     h.ptr(tri_ind), h.ptr(vertex_grad), B, nver, ntri, H, W, mode, accumulate, h.ptr(ws), nws,
                                     h.stream_ptr(dev))
    h.check(rc, "fr_render_normal_backward")


def _texture_backward_call(h, g, g_offset, g_stride, tri_c, tri_ind, texture_grad, B, nver, ntri, H, W, tex_batch, accumulate, dev):
    """fr_render_texture_backward with its workspace (24 bytes per pixel, plus the slabs of a shared texture): the gradient read
    at `g_offset` floats into `g`, `g_stride` floats between pixels; texture_grad is dense [tex_batch,3,nver]."""
    L = h.lib()
    nws = L.fr_render_texture_backward_workspace_bytes(B, nver, H, W, tex_batch)
    ws = h.byte_buffer(nws, dev)
    rc = L.fr_render_texture_backward(ctypes.c_void_p(g.data_ptr() + 4 * g_offset), g_stride, h.ptr(tri_c), h.ptr(tri_ind),
                                      h.ptr(texture_grad), B, nver, ntri, H, W, tex_batch, accumulate, h.ptr(ws), nws,
                                      h.stream_ptr(dev))
    h.check(rc, "fr_render_texture_backward")


def _depth_interp_forward_call(h, ver_c, tri_c, tri_ind, B, nver, ntri, H, W, dev):
    """fr_depth_interp_forward on the dense vertex tensor -> the interpolated plane [B,H,W,1]."""
    depth = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)
    rc = h.lib().fr_depth_interp_forward(h.ptr(ver_c), nver, h.ptr(tri_c), h.ptr(tri_ind), B, nver, ntri, H, W, h.ptr(depth),
                                         h.stream_ptr(dev))
    h.check(rc, "fr_depth_interp_forward")
    return depth


def _depth_interp_backward_call(h, g, ver_c, tri_c, tri_ind, vertex_grad, B, nver, ntri, H, W, accumulate, dev):
    """fr_depth_interp_backward with its workspace (48 bytes per pixel): all three rows of vertex_grad."""
    if B * H * W == 0:   # the entry point writes nothing for an empty image
        if not accumulate:
            vertex_grad.zero_()
        return
    L = h.lib()
    nws = L.fr_depth_interp_backward_workspace_bytes(B, nver, H, W)
    ws = h.byte_buffer(nws, dev)
    rc = L.fr_depth_interp_backward(h.ptr(g), h.ptr(ver_c), nver, h.ptr(tri_c), h.ptr(tri_ind), h.ptr(vertex_grad), B, nver, ntri,
                                    H, W, accumulate, h.ptr(ws), nws, h.stream_ptr(dev))
    h.check(rc, "fr_depth_interp_backward")


def _texture_grad_of(ctx, texture_image_grad):
    """The `texture` gradient of a render_depth node built with texture_grad=True, in the input's own shape ([3,N], [1,3,N] or
    [B,3,N]); None -- and no launch -- when nothing downstream used tex_img or the texture needs no gradient."""
    if texture_image_grad is None or not ctx.needs_input_grad[2]:
        return None
    h = _host()
    tri_c, tri_ind = ctx.saved_tensors[:2]
    B, nver, ntri, H, W = ctx.dims
    dev = tri_c.device
    shape = ctx.tex_shape
    tex_batch = 1 if len(shape) == 2 else int(shape[0])
    texture_grad = torch.empty((tex_batch, 3, nver), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _texture_backward_call(h, h.require_gpu_f32(texture_image_grad, "texture_image_grad"), 0, 3, tri_c, tri_ind, texture_grad,
                               B, nver, ntri, H, W, tex_batch, 0, dev)
    return texture_grad.reshape(shape)


class _RenderDepth(torch.autograd.Function):
    """RenderDepth / RenderDepthGrad (render_depth_op.cc:535-589) as one autograd node.
    normal_grad: the node also keeps `ver` ([B,3,nver] fp32: 41 MB at 64 faces of the full mesh) and, where a gradient of `normal`
    arrives, its backward runs fr_render_normal_backward (raw mode) behind the depth backward: all three rows of the vertex
    gradient are filled.  texture_grad: the same saved tensors (the texture's shape is all the node adds); a gradient arriving at
    `tex_img` reaches `texture` through fr_render_texture_backward.  depth_interp: the first output is the interpolated plane
    (fr_depth_interp_forward over this call's tri_ind; the flat plane is not returned), the node keeps `ver`, and a gradient of
    `depth` runs fr_depth_interp_backward in place of the flat backward."""

    @staticmethod
    def forward(ctx, ver, tri, texture, image, normal_grad, texture_grad, depth_interp):
        h = _host()
        _check_forward_shapes(ver, tri, texture, image)
        ver_c = h.require_gpu_f32(ver, "ver")
        tri_c = h.require_gpu_f32(tri, "tri")
        tex_c = h.require_gpu_f32(texture, "texture")
        if not image.is_cuda:
            raise RuntimeError("image is on %s: the fr_hotpath kernels run on an MI355X only" % image.device)
        B, H, W = int(image.shape[0]), int(image.shape[1]), int(image.shape[2])
        nver, ntri = int(ver_c.shape[2]), int(tri_c.shape[1])
        tex_batch = 1 if tex_c.dim() == 2 else int(tex_c.shape[0])
        if tex_batch not in (1, B):
            raise ValueError("The texture's batch is neither 1 nor the image batch")
        dev = ver_c.device
        opts = dict(dtype=torch.float32, device=dev)
        depth = torch.empty((B, H, W, 1), **opts)
        tex_img = torch.empty((B, H, W, 3), **opts)
        normal = torch.empty((B, H, W, 3), **opts)
        tri_ind = torch.empty((B, H, W, 1), **opts)
        L = h.lib()
        with torch.cuda.device(dev):
            ws_bytes = L.fr_render_depth_workspace_bytes(B, nver, ntri, H, W)
            if ws_bytes:
                rc = _render_with_workspace(dev, ws_bytes, tri_c, (B, nver, ntri, H, W), lambda ws, phases: (
                    L.fr_render_depth_forward_phases(h.ptr(ver_c), h.ptr(tri_c), h.ptr(tex_c), B, nver, ntri, H, W, 3, tex_batch,
                                                     h.ptr(depth), h.ptr(tex_img), h.ptr(normal), h.ptr(tri_ind), h.ptr(ws), ws_bytes,
                                                     h.stream_ptr(dev), phases)))
            else:
                rc = L.fr_render_depth_forward(h.ptr(ver_c), h.ptr(tri_c), h.ptr(tex_c), B, nver, ntri, H, W, 3, tex_batch,
                                               h.ptr(depth), h.ptr(tex_img), h.ptr(normal), h.ptr(tri_ind), None, 0,
                                               h.stream_ptr(dev))
        h.check(rc, "fr_render_depth_forward")
        if depth_interp:
            with torch.cuda.device(dev):
                depth = _depth_interp_forward_call(h, ver_c, tri_c, tri_ind, B, nver, ntri, H, W, dev)
        if normal_grad or depth_interp:
            ctx.save_for_backward(tri_c, tri_ind, ver_c)
        else:
            ctx.save_for_backward(tri_c, tri_ind)
        if texture_grad:
            ctx.tex_shape = tuple(texture.shape)
        ctx.normal_grad, ctx.texture_grad, ctx.depth_interp = bool(normal_grad), bool(texture_grad), bool(depth_interp)
        ctx.dims = (B, nver, ntri, H, W)
        ctx.set_materialize_grads(False)  # an unused depth output (the SfS renders, network.py:423, 454) costs no backward
        return depth, tex_img, normal, tri_ind

    @staticmethod
    def backward(ctx, depth_grad, texture_image_grad, normal_grad, tri_ind_grad):
        # by default only depth_grad is used; vertex has gradients, tri / texture / image do not (reference ops.py:86-95)
        h = _host()
        tri_c, tri_ind = ctx.saved_tensors[:2]
        B, nver, ntri, H, W = ctx.dims
        dev = tri_c.device
        if not ctx.normal_grad:
            normal_grad = None
        vertex_grad = None   # nothing downstream used `depth` (or `normal`): the vertices get no gradient (reference ops.py:95)
        if depth_grad is not None or normal_grad is not None:
            vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                if depth_grad is not None and ctx.depth_interp:
                    _depth_interp_backward_call(h, h.require_gpu_f32(depth_grad, "depth_grad"), ctx.saved_tensors[2], tri_c, tri_ind,
                                                vertex_grad, B, nver, ntri, H, W, 0, dev)
                elif depth_grad is not None:
                    _backward_call(h, h.require_gpu_f32(depth_grad, "depth_grad"), tri_c, tri_ind, vertex_grad, B, nver, ntri, H, W,
                                   dev)
                if normal_grad is not None:
                    _normal_backward_call(h, h.require_gpu_f32(normal_grad, "normal_grad"), 0, 3, ctx.saved_tensors[2], tri_c,
                                          tri_ind, vertex_grad, B, nver, ntri, H, W, 0, 1 if depth_grad is not None else 0, dev)
        texture_grad = _texture_grad_of(ctx, texture_image_grad) if ctx.texture_grad else None
        return vertex_grad, None, texture_grad, None, None, None, None


class _RenderingLayerFused(torch.autograd.Function):
    """render_depth + the post-processing of FaceRecNet.rendering_layer (nets/network.py:185-199) as one kernel pass:
    (ver, tri, texture, im_gray) -> (net_input [B,H,W,7], depth_img [B,H,W,1], depth, tri_ind).
    normal_grad: the node also keeps `ver` ([B,3,nver] fp32: 41 MB at 64 faces of the full mesh) and its backward completes the
    depth backward's tensor with fr_render_normal_backward (post mode on channels 4-6 of the net_input gradient, accumulate=1)."""

    @staticmethod
    def forward(ctx, ver, tri, texture, im_gray, normal_grad):
        h = _host()
        image = im_gray
        _check_forward_shapes(ver, tri, texture, image)
        ver_c = h.require_gpu_f32(ver, "ver")
        tri_c = h.require_gpu_f32(tri, "tri")
        tex_c = h.require_gpu_f32(texture, "texture")
        img_c = h.require_gpu_f32(im_gray, "im_gray")
        if img_c.shape[-1] != 1:
            raise ValueError("im_gray must be [B,H,W,1]")
        B, H, W = int(img_c.shape[0]), int(img_c.shape[1]), int(img_c.shape[2])
        nver, ntri = int(ver_c.shape[2]), int(tri_c.shape[1])
        tex_batch = 1 if tex_c.dim() == 2 else int(tex_c.shape[0])
        dev = ver_c.device
        opts = dict(dtype=torch.float32, device=dev)
        net_in = torch.empty((B, H, W, 7), **opts)
        depth_img = torch.empty((B, H, W, 1), **opts)
        depth = torch.empty((B, H, W, 1), **opts)
        tri_ind = torch.empty((B, H, W, 1), **opts)
        L = h.lib()
        with torch.cuda.device(dev):
            ws_bytes = L.fr_render_depth_workspace_bytes(B, nver, ntri, H, W)
            # the same "pack once while the same `tri` tensor is passed" rule as render_depth (the table is the same table)
            rc = _render_with_workspace(dev, ws_bytes, tri_c, (B, nver, ntri, H, W), lambda ws, phases: (
                L.fr_rendering_layer_forward_phases(h.ptr(ver_c), h.ptr(tri_c), h.ptr(tex_c), h.ptr(img_c), B, nver, ntri, H, W,
                                                    tex_batch, h.ptr(net_in), h.ptr(depth_img), h.ptr(depth), h.ptr(tri_ind),
                                                    h.ptr(ws), ws_bytes, h.stream_ptr(dev), phases)))
        if rc == -4:
            raise NotImplementedError("fused rendering layer: shape only covered by the fallback rasteriser")
        h.check(rc, "fr_rendering_layer_forward")
        if normal_grad:
            ctx.save_for_backward(tri_c, tri_ind, depth, img_c, ver_c)
        else:
            ctx.save_for_backward(tri_c, tri_ind, depth, img_c)
        ctx.normal_grad = bool(normal_grad)
        ctx.dims = (B, nver, ntri, H, W)
        ctx.mark_non_differentiable(tri_ind)
        return net_in, depth_img, depth, tri_ind

    @staticmethod
    def backward(ctx, g_net_in, g_depth_img, g_depth, g_tri_ind):
        # only the mask channel and the depth image depend on the vertices (through depth, hence vertex z):
        #   mask = clip(depth, 1e-6, 1) * im  ->  g * im where 1e-6 <= depth <= 1;   depth_img = max(depth, 1e-6)
        # (normal_grad adds the normal channels: all three rows, through the saved vertices)
        h = _host()
        tri_c, tri_ind, depth, img = ctx.saved_tensors[:4]
        B, nver, ntri, H, W = ctx.dims
        dg = torch.zeros_like(depth)
        if g_net_in is not None:
            dg = dg + g_net_in[..., 0:1] * img * ((depth >= 1e-6) & (depth <= 1.0)).to(depth.dtype)
        if g_depth_img is not None:
            dg = dg + g_depth_img * (depth >= 1e-6).to(depth.dtype)
        if g_depth is not None:
            dg = dg + g_depth
        dg = dg.contiguous()
        vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=depth.device)
        with torch.cuda.device(depth.device):
            _backward_call(h, dg, tri_c, tri_ind, vertex_grad, B, nver, ntri, H, W, depth.device)
            if ctx.normal_grad and g_net_in is not None:
                # channels 4-6 of g_net_input are the gradient of the normalised map: post mode, read in place at stride 7
                gn = h.require_gpu_f32(g_net_in, "net_input_grad")
                _normal_backward_call(h, gn, 4, 7, ctx.saved_tensors[4], tri_c, tri_ind, vertex_grad, B, nver, ntri, H, W, 1, 1,
                                      depth.device)
        return vertex_grad, None, None, None, None


class _DecodeRenderingLayer(torch.autograd.Function):
    """vertices_transform -> coarse_net_input as ONE autograd node (include/fr_hotpath.h, "differentiable decode ->
    rendering-layer step"): (params, R, im_gray) -> (net_input [B,H,W,7], depth_img [B,H,W,1]).  Forward:
    fr_decode_rendering_layer_forward, the vertices in a pitched per-stream scratch buffer that is not kept.  Backward:
    fr_decode_render_backward -- the pixel gradient is formed inside the render backward's records pass, only the z row of the
    vertex gradient exists, and the decode backward takes d f from mu: the node saves params, R, tri_ind, depth and im_gray, no
    [B,3,N]-sized tensor.  Raises NotImplementedError where either entry point answers FR_ERR_UNSUPPORTED.
    pose_grad=True: the hand-off is a tensor of the node's own and IS kept ([B,3,pitch] floats: 41 MB at 64 faces of the full
    mesh); the backward is fr_decode_render_backward_pose, which also fills the angle columns (R evaluated in-kernel) or returns
    dL/dR for a caller-computed R.  The default leaves the angles at 0 and R without a gradient."""

    @staticmethod
    def forward(ctx, params, R, im_gray, tri, texture, basis, im_size, pose_grad=False):
        h = _host()
        L = h.lib()
        p = h.require_gpu_f32(params, "pred_params")
        img_c = h.require_gpu_f32(im_gray, "im_gray")
        tri_c = h.require_gpu_f32(tri, "tri")
        tex_c = h.require_gpu_f32(texture, "texture")
        N, ns, ne = basis.nvert, basis.ndim_shape, basis.ndim_exp
        if p.dim() != 2 or p.shape[1] != 7 + ns + ne:
            raise ValueError("pred_params must be (B,%d)" % (7 + ns + ne))
        B = int(p.shape[0])
        if img_c.dim() != 4 or img_c.shape[0] != B or img_c.shape[-1] != 1:
            raise ValueError("im_gray must be [B,H,W,1]")
        _check_tri(tri_c)
        if tex_c.dim() not in (2, 3) or tex_c.shape[-2] != 3 or tex_c.shape[-1] != N:
            raise ValueError("The texture is not Batch x 3 x nver")
        tex_batch = 1 if tex_c.dim() == 2 else int(tex_c.shape[0])
        if tex_batch not in (1, B):
            raise ValueError("The texture's batch is neither 1 nor the image batch")
        H, W, ntri = int(img_c.shape[1]), int(img_c.shape[2]), int(tri_c.shape[1])
        dev = p.device
        if L.fr_decode_render_backward_workspace_bytes(max(B, 1), N, ns, ne, H, W) == 0:
            raise NotImplementedError("decode -> rendering layer: basis / mesh not served by the fused decode backward")
        opts = dict(dtype=torch.float32, device=dev)
        net_in = torch.empty((B, H, W, 7), **opts)
        depth_img = torch.empty((B, H, W, 1), **opts)
        depth = torch.empty((B, H, W, 1), **opts)
        tri_ind = torch.empty((B, H, W, 1), **opts)
        with torch.cuda.device(dev):
            ws_bytes = L.fr_render_depth_workspace_bytes(B, N, ntri, H, W)
            hand_bytes = L.fr_decode_render_vertex_bytes(B, N)
            hand = h.byte_buffer(hand_bytes, dev, 256) if pose_grad else None

            def launch(ws, phases, hand):
                return L.fr_decode_rendering_layer_forward(h.ptr(p), h.ptr(basis.image), h.ptr(R), h.ptr(tri_c), h.ptr(tex_c),
                                                           h.ptr(img_c), B, N, ns, ne, ntri, H, W, tex_batch, float(im_size),
                                                           h.ptr(hand), hand_bytes, h.ptr(net_in), h.ptr(depth_img), h.ptr(depth),
                                                           h.ptr(tri_ind), h.ptr(ws), ws_bytes, h.stream_ptr(dev), 8 | phases)

            def call(ws, phases):
                if pose_grad:
                    return launch(ws, phases, hand)
                # (the one nested hold: the pooled hand-off is taken inside the hold on the render workspace -- threads that
                # share the stream share both buffers)
                with _KINDS_POOL.hold("hand", dev, hand_bytes) as ent:
                    return launch(ws, phases, ent.buf)
            rc = _render_with_workspace(dev, ws_bytes, tri_c, (B, N, ntri, H, W), call)
        if rc == -4:
            raise NotImplementedError("decode -> rendering layer: shape only covered by the fallback rasteriser")
        h.check(rc, "fr_decode_rendering_layer_forward")
        ctx.save_for_backward(p, R if R is not None else p.new_empty(0), tri_ind, depth, img_c)
        ctx.has_R = R is not None
        ctx.hand = (hand, hand_bytes) if pose_grad else None   # (an intermediate of this node alone: no other node can reach it)
        ctx.tri, ctx.basis, ctx.im_size = tri_c, basis, float(im_size)   # (tri: a constant of the model, no gradient)
        ctx.dims = (B, N, ns, ne, ntri, H, W)
        ctx.set_materialize_grads(False)
        return net_in, depth_img

    @staticmethod
    def backward(ctx, g_net_in, g_depth_img):
        if g_net_in is None and g_depth_img is None:
            return (None,) * 8
        h = _host()
        L = h.lib()
        p, R, tri_ind, depth, img = ctx.saved_tensors
        B, N, ns, ne, ntri, H, W = ctx.dims
        basis = ctx.basis
        dev = p.device
        gn = h.require_gpu_f32(g_net_in, "net_input_grad") if g_net_in is not None else None
        gd = h.require_gpu_f32(g_depth_img, "depth_img_grad") if g_depth_img is not None else None
        gp = torch.empty_like(p)
        with torch.cuda.device(dev):
            image_t = basis.image_t()
            gR = None
            if ctx.hand is not None:
                if ctx.has_R and ctx.needs_input_grad[1]:
                    gR = torch.empty_like(R)
                nws = L.fr_decode_render_backward_pose_workspace_bytes(B, N, ns, ne, H, W)
                with _KINDS_POOL.hold("bwd", dev, nws) as ent:
                    rc = L.fr_decode_render_backward_pose(None, h.ptr(gd), h.ptr(gn), h.ptr(img), h.ptr(depth), h.ptr(ctx.tri),
                                                          h.ptr(tri_ind), h.ptr(p), h.ptr(basis.mu), h.ptr(image_t),
                                                          h.ptr(R) if ctx.has_R else None, B, N, ns, ne, ntri, H, W, ctx.im_size,
                                                          h.ptr(gp), h.ptr(ent.buf), nws, h.stream_ptr(dev), h.ptr(ctx.hand[0]),
                                                          ctx.hand[1], h.ptr(gR))
                h.check(rc, "fr_decode_render_backward_pose")
                return gp, gR, None, None, None, None, None, None
            nws = L.fr_decode_render_backward_workspace_bytes(B, N, ns, ne, H, W)
            with _KINDS_POOL.hold("bwd", dev, nws) as ent:
                rc = L.fr_decode_render_backward(None, h.ptr(gd), h.ptr(gn), h.ptr(img), h.ptr(depth), h.ptr(ctx.tri),
                                                 h.ptr(tri_ind), h.ptr(p), h.ptr(basis.mu), h.ptr(image_t),
                                                 h.ptr(R) if ctx.has_R else None, B, N, ns, ne, ntri, H, W, ctx.im_size, h.ptr(gp),
                                                 h.ptr(ent.buf), nws, h.stream_ptr(dev))
        h.check(rc, "fr_decode_render_backward")
        return gp, None, None, None, None, None, None, None


def decode_rendering_layer(params, R, im_gray, tri, texture, basis, im_size, pose_grad=False, normal_grad=False):
    """One-node decode -> rendering layer: (params [B,d], R [B,3,3] or None, im_gray [B,H,W,1]) -> (net_input [B,H,W,7],
    depth_img [B,H,W,1]); `basis` is the network's PackedBasis.  Raises NotImplementedError where the fused entry points do not
    serve the shape (the caller composes vertices_transform and rendering_layer_fused instead).
    pose_grad=True: the backward also gives the three angles their gradient (R None) or R its own (fr_decode_render_backward_pose);
    the node then retains the forward's vertex hand-off, one [B,3,pitch] fp32 buffer -- 41 MB at 64 faces of the full mesh.
    normal_grad=True is not served here: the one-call backward is z-only by construction (only the z plane of the vertex gradient
    exists in it), so it raises NotImplementedError like any other unserved call and the caller takes the two-step route
    (FaceRecNet.decode_rendering_layer does: vertices_transform, then rendering_layer_fused(normal_grad=True))."""
    if normal_grad:
        raise NotImplementedError("decode -> rendering layer: normal gradients need the dense vertex gradient (two-step route)")
    return _DecodeRenderingLayer.apply(params, R, im_gray, tri, texture, basis, im_size, bool(pose_grad))


def _sfs_inputs(op, h, abedo, normal, im_gray, abedo_new, normal_new, abedo_grad):
    """The argument checks and conversions of `op` (sfs_intensity, sfs_intensity_sharded) -> (a_c, n_c, i_c, a2_c, n2_c, B, H, W)"""
    for t, name in ((abedo, "abedo"), (im_gray, "im_gray")) + (() if abedo_grad else ((abedo_new, "abedo_new"),)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError("%s: %s requires grad, but the albedos and im_gray are constants of this model "
                             "(detach it)" % (op, name))
    a_c = h.require_gpu_f32(abedo, "abedo")
    n_c = h.require_gpu_f32(normal, "normal")
    i_c = h.require_gpu_f32(im_gray, "im_gray")
    a2_c = h.require_gpu_f32(abedo_new, "abedo_new")
    n2_c = n_c if normal_new is normal else h.require_gpu_f32(normal_new, "normal_new")
    if n_c.dim() != 4 or n_c.shape[3] != 3:
        raise ValueError("%s expects normal [B,H,W,3]" % op)
    B, H, W = int(n_c.shape[0]), int(n_c.shape[1]), int(n_c.shape[2])
    for t, name, c in ((a_c, "abedo", 1), (i_c, "im_gray", 1), (a2_c, "abedo_new", 1), (n2_c, "normal_new", 3)):
        _check_plane(op, name, t, B, H, W, c, n_c.device, "normal")
    return a_c, n_c, i_c, a2_c, n2_c, B, H, W


def _sfs_grad_buffers(ctx):
    """-> (grad_normal, grad_normal_new, grad_abedo_new) of an SfS node's backward, None where the input needs none; None where
    no input needs any (then nothing is launched)"""
    B, H, W, _ = ctx.dims
    dev = ctx.saved_tensors[0].device
    want_n, want_n2 = ctx.needs_input_grad[1], ctx.needs_input_grad[4]
    want_a2 = ctx.abedo_grad and ctx.needs_input_grad[3]
    if not (want_n or want_n2 or want_a2):
        return None
    gn = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if want_n else None
    gn2 = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if want_n2 else None
    ga2 = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev) if want_a2 else None
    return gn, gn2, ga2


class _SfsIntensity(torch.autograd.Function):
    """fr_sfs_intensity_forward / _backward (include/fr_hotpath.h, "shape-from-shading term") as one autograd node: the per-pixel
    lighting solve over the batch and the shading, P held constant in the backward.  abedo_grad: `abedo_new` may require grad and
    the backward also returns grad_abedo_new (fr_sfs_intensity_backward_tex); `abedo` and `im_gray` stay constants."""

    @staticmethod
    def forward(ctx, abedo, normal, im_gray, abedo_new, normal_new, rcond, abedo_grad):
        h = _host()
        ctx.abedo_grad = bool(abedo_grad)
        a_c, n_c, i_c, a2_c, n2_c, B, H, W = _sfs_inputs("sfs_intensity", h, abedo, normal, im_gray, abedo_new, normal_new, abedo_grad)
        dev = n_c.device
        L = h.lib()
        nst = L.fr_sfs_state_bytes(H, W)
        state = torch.empty((max(nst, 16) // 8,), dtype=torch.float64, device=dev)   # per call: the backward reads it
        intensity = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = L.fr_sfs_intensity_forward(h.ptr(a_c), h.ptr(n_c), h.ptr(i_c), h.ptr(a2_c), h.ptr(n2_c), B, H, W, float(rcond),
                                            h.ptr(intensity), h.ptr(state), nst, h.stream_ptr(dev))
        h.check(rc, "fr_sfs_intensity_forward")
        ctx.save_for_backward(a_c, i_c, a2_c, n2_c, state)
        ctx.dims = (B, H, W, nst)
        return intensity

    @staticmethod
    def backward(ctx, g):
        h = _host()
        a_c, i_c, a2_c, n2_c, state = ctx.saved_tensors
        B, H, W, nst = ctx.dims
        dev = a_c.device
        grads = _sfs_grad_buffers(ctx)
        if grads is None:
            return (None,) * 7
        gn, gn2, ga2 = grads
        g_c = h.require_gpu_f32(g, "grad_intensity")
        with torch.cuda.device(dev):
            if ga2 is not None:
                rc = h.lib().fr_sfs_intensity_backward_tex(h.ptr(g_c), h.ptr(a_c), h.ptr(i_c), h.ptr(a2_c), h.ptr(n2_c),
                                                           h.ptr(state), nst, B, H, W, h.ptr(gn), h.ptr(gn2), h.ptr(ga2),
                                                           h.stream_ptr(dev))
            else:
                rc = h.lib().fr_sfs_intensity_backward(h.ptr(g_c), h.ptr(a_c), h.ptr(i_c), h.ptr(a2_c), h.ptr(n2_c), h.ptr(state),
                                                       nst, B, H, W, h.ptr(gn), h.ptr(gn2), h.stream_ptr(dev))
        h.check(rc, "fr_sfs_intensity_backward")
        return None, gn, None, ga2, gn2, None, None


def sfs_intensity(abedo, normal, im_gray, abedo_new, normal_new, rcond=1e-15, abedo_grad=False):
    """The shape-from-shading intensity (nets/network.py:424-460) on rendered maps in ONE kernel pass: per pixel the lighting
    l = pinv(sum_b n n^T) sum_b n I / (abedo + 1) over the batch, then abedo_new * (l . normal_new) -> [B,H,W,1].  float64 sums in
    a fixed order (a function of B alone), bit-reproducible; `rcond` is the eigenvalue cutoff of the pseudo-inverse.
    Gradients go to `normal` and `normal_new` only, with the pseudo-inverse held constant (what a detached pinv gives the torch
    route); autograd adds the two when one tensor is passed for both.  An albedo or im_gray that requires grad is refused: they are
    constants of this model.  The node keeps a state tensor of ten float64 planes (3.2 MB at 200 x 200) for its backward.
    abedo_grad=True: `abedo_new` may require grad and receives g * (l . normal_new), the lighting held as the state holds it
    (fr_sfs_intensity_backward_tex); `abedo` and `im_gray` are still refused.  Same intensity, bit for bit."""
    return _SfsIntensity.apply(abedo, normal, im_gray, abedo_new, normal_new, float(rcond), bool(abedo_grad))


def _dist():
    """utils/dist.py, loaded by path like _host() (the module holds no state of its own: the process group is torch's)."""
    name = "_fr_hotpath_dist"
    mod = sys.modules.get(name)
    if mod is None:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_PKG_DIR, "utils", "dist.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod


def _sfs_exchange(exchange, local, planes, H, W):
    """local [planes,H,W] float64 -> the stacked parts [nparts,planes,H,W], contiguous on local's device"""
    parts = (exchange if exchange is not None else _dist().all_gather_stack)(local)
    if (not isinstance(parts, torch.Tensor) or parts.dtype != torch.float64 or parts.dim() != 4 or parts.shape[0] < 1
            or tuple(parts.shape[1:]) != (planes, H, W) or parts.device != local.device):
        raise ValueError("sfs_intensity_sharded: exchange must return a float64 tensor [nparts,%d,%d,%d] on %s (got %s)"
                         % (planes, H, W, local.device, getattr(parts, "shape", type(parts))))
    return parts.detach().contiguous()


class _SfsIntensitySharded(torch.autograd.Function):
    """fr_sfs_moments -> exchange -> fr_sfs_solve_shade, and fr_sfs_backward_q -> exchange -> fr_sfs_backward_apply (include/
    fr_hotpath.h, "shape-from-shading term across ranks") as one autograd node."""

    @staticmethod
    def forward(ctx, abedo, normal, im_gray, abedo_new, normal_new, rcond, abedo_grad, exchange):
        h = _host()
        ctx.abedo_grad = bool(abedo_grad)
        ctx.exchange = exchange
        a_c, n_c, i_c, a2_c, n2_c, B, H, W = _sfs_inputs("sfs_intensity_sharded", h, abedo, normal, im_gray, abedo_new, normal_new,
                                                         abedo_grad)
        dev = n_c.device
        L = h.lib()
        nst = L.fr_sfs_state_bytes(H, W)
        state = torch.empty((max(nst, 16) // 8,), dtype=torch.float64, device=dev)   # per call: the backward reads it
        intensity = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)
        ctx.dims = (B, H, W, nst)
        ctx.save_for_backward(a_c, i_c, a2_c, n2_c, state)
        if H * W == 0:   # (the same on every rank: nobody calls the exchange)
            return intensity
        mine = torch.empty((9, H, W), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = L.fr_sfs_moments(h.ptr(a_c), h.ptr(n_c), h.ptr(i_c), B, H, W, h.ptr(mine), mine.numel() * 8, h.stream_ptr(dev))
        h.check(rc, "fr_sfs_moments")
        parts = _sfs_exchange(exchange, mine, 9, H, W)
        with torch.cuda.device(dev):
            rc = L.fr_sfs_solve_shade(h.ptr(parts), int(parts.shape[0]), h.ptr(a2_c), h.ptr(n2_c), B, H, W, float(rcond),
                                      h.ptr(intensity), h.ptr(state), nst, h.stream_ptr(dev))
        h.check(rc, "fr_sfs_solve_shade")
        return intensity

    @staticmethod
    def backward(ctx, g):
        h = _host()
        a_c, i_c, a2_c, n2_c, state = ctx.saved_tensors
        B, H, W, nst = ctx.dims
        dev = a_c.device
        grads = _sfs_grad_buffers(ctx)
        if grads is None:
            return (None,) * 8
        gn, gn2, ga2 = grads
        g_c = h.require_gpu_f32(g, "grad_intensity")
        if H * W == 0:
            return None, gn, None, ga2, gn2, None, None, None
        L = h.lib()
        parts = None
        if gn is not None:   # the one collective of the backward: issued by every rank or by none (same graph on every rank)
            mine = torch.empty((3, H, W), dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                rc = L.fr_sfs_backward_q(h.ptr(g_c), h.ptr(a2_c), h.ptr(n2_c), B, H, W, h.ptr(mine), mine.numel() * 8,
                                         h.stream_ptr(dev))
            h.check(rc, "fr_sfs_backward_q")
            parts = _sfs_exchange(ctx.exchange, mine, 3, H, W)
        with torch.cuda.device(dev):
            rc = L.fr_sfs_backward_apply(h.ptr(g_c), h.ptr(a_c), h.ptr(i_c), h.ptr(a2_c), h.ptr(n2_c), h.ptr(state), nst,
                                         h.ptr(parts), int(parts.shape[0]) if parts is not None else 1, B, H, W, h.ptr(gn),
                                         h.ptr(gn2), h.ptr(ga2), h.stream_ptr(dev))
        h.check(rc, "fr_sfs_backward_apply")
        return None, gn, None, ga2, gn2, None, None, None


def sfs_intensity_sharded(abedo, normal, im_gray, abedo_new, normal_new, rcond=1e-15, abedo_grad=False, exchange=None):
    """sfs_intensity with the batch spread over several ranks: this rank passes its OWN faces' maps ([B,H,W,c]; B may differ from
    rank to rank and may be 0, H and W may not) and receives its own faces' intensity, computed with the lighting of ALL ranks'
    faces.  The ranks exchange sums, not maps: nine float64 planes per rank in the forward (M and r), three in the backward (q);
    the totals are formed in rank order, so every rank holds the same lighting, bit for bit, and the result does not depend on
    which rank computes it (fr_sfs_moments / fr_sfs_solve_shade / fr_sfs_backward_q / fr_sfs_backward_apply).
    exchange(local [k,H,W] float64) -> [nparts,k,H,W] float64 on the same device, the ranks' planes stacked in rank order;
    default: utils/dist.py all_gather_stack on the default process group.  It is called ONCE in the forward (k = 9) and once in the
    backward (k = 3), the latter only when `normal` needs a gradient.  With no process group and no `exchange` the node equals
    sfs_intensity bit for bit.  Same argument checks and refusals as sfs_intensity; abedo_grad as there.
    Gradient semantics.  The backward uses the TOTAL q = sum over ranks r of q_r: rank i returns u_b * (P sum_r q_r) for its own
    faces b, i.e. also the part of every OTHER rank's loss that passes through the shared lighting into rank i's normals.  With
    each rank's loss the mean over its own faces and DDP's averaging of the ranks' gradients, that is the single-process gradient
    of the mean loss over all ranks' faces (the gather=True torch route drops the cross-rank part).  grad_normal_new and
    grad_abedo_new are local.  P is held constant, as in sfs_intensity.
    Every rank must build the same graph: the backward issues a collective when, and only when, `normal` needs a gradient, so
    `normal` must require grad on all ranks or on none, and every rank must run the backward.  With a real collective behind
    `exchange` the node cannot be captured into a HIP graph (the collective and, under gloo, its host staging are not capturable
    work of this stream)."""
    return _SfsIntensitySharded.apply(abedo, normal, im_gray, abedo_new, normal_new, float(rcond), bool(abedo_grad), exchange)


class _DepthNormals(torch.autograd.Function):
    """fr_depth_normals_forward / _backward (include/fr_hotpath.h, "depth-map normals") as one autograd node."""

    @staticmethod
    def forward(ctx, depth, mask):
        h = _host()
        if isinstance(mask, torch.Tensor) and mask.requires_grad:
            raise ValueError("depth_normals: mask requires grad, but the mask is a constant of this operator (detach it)")
        d_c = h.require_gpu_f32(depth, "depth")
        if d_c.dim() == 4 and d_c.shape[3] == 1:
            B, H, W = int(d_c.shape[0]), int(d_c.shape[1]), int(d_c.shape[2])
        elif d_c.dim() == 3:
            B, H, W = (int(v) for v in d_c.shape)
        else:
            raise ValueError("depth_normals expects depth [B,H,W,1] or [B,H,W] (got %s)" % (tuple(d_c.shape),))
        m_c = None
        if mask is not None:
            m_c = h.require_gpu_f32(mask, "mask")
            _check_plane("depth_normals", "mask", m_c, B, H, W, 1, d_c.device, "depth", flat=True)
        dev = d_c.device
        normal = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = h.lib().fr_depth_normals_forward(h.ptr(d_c), h.ptr(m_c), B, H, W, h.ptr(normal), h.stream_ptr(dev))
        h.check(rc, "fr_depth_normals_forward")
        ctx.save_for_backward(d_c, m_c)
        ctx.dims = (B, H, W)
        ctx.depth_shape = tuple(depth.shape)
        return normal

    @staticmethod
    def backward(ctx, g):
        h = _host()
        d_c, m_c = ctx.saved_tensors
        B, H, W = ctx.dims
        if not ctx.needs_input_grad[0]:
            return None, None
        dev = d_c.device
        g_c = h.require_gpu_f32(g, "grad_normal")
        gd = torch.empty(ctx.depth_shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = h.lib().fr_depth_normals_backward(h.ptr(g_c), h.ptr(d_c), h.ptr(m_c), B, H, W, h.ptr(gd), h.stream_ptr(dev))
        h.check(rc, "fr_depth_normals_backward")
        return gd, None


def depth_normals(depth, mask=None):
    """The normal map [B,H,W,3] of a depth map [B,H,W,1] (or [B,H,W]) on the pixel grid, in the renderer's conventions: per valid
    pixel (-dz/dx, -dz/dy, 1) normalised, x = column, y = row, n_z > 0; central differences inside the mask, one-sided ones at its
    edges, a zero slope where a pixel has no valid neighbour on an axis; (0, 0, 0) at invalid pixels (fr_depth_normals_forward:
    float64 arithmetic, one kernel pass).  `mask` ([B,H,W,1] or [B,H,W], e.g. a render's tri_ind): a pixel is valid iff mask >= 0
    (NaN is invalid); None: every pixel is.  The gradient goes to `depth`, in depth's own shape (fr_depth_normals_backward: a
    gather, bit-reproducible); `mask` gets None, and a mask that requires grad is refused.  The node saves `depth` and `mask`."""
    return _DepthNormals.apply(depth, mask)


class _DepthInterpolate(torch.autograd.Function):
    """fr_depth_interp_forward / _backward (include/fr_hotpath.h, "interpolated depth") as one autograd node."""

    @staticmethod
    def forward(ctx, ver, tri, tri_ind):
        h = _host()
        if isinstance(tri_ind, torch.Tensor) and tri_ind.requires_grad:
            raise ValueError("depth_interpolate: tri_ind requires grad, but the winning triangles are held fixed (detach it)")
        ver_c = h.require_gpu_f32(ver, "ver")
        tri_c = h.require_gpu_f32(tri, "tri")
        ti_c = h.require_gpu_f32(tri_ind, "tri_ind")
        _check_ver(ver_c)
        _check_tri(tri_c)
        if ti_c.dim() != 4 or ti_c.shape[0] != ver_c.shape[0] or ti_c.shape[3] != 1:
            raise ValueError("depth_interpolate expects tri_ind [B,H,W,1] with the vertex's batch (got %s)" % (tuple(ti_c.shape),))
        if tri_c.device != ver_c.device or ti_c.device != ver_c.device:
            raise ValueError("depth_interpolate: ver, tri and tri_ind must be on one device")
        B, H, W = int(ti_c.shape[0]), int(ti_c.shape[1]), int(ti_c.shape[2])
        nver, ntri = int(ver_c.shape[2]), int(tri_c.shape[1])
        dev = ver_c.device
        with torch.cuda.device(dev):
            depth = _depth_interp_forward_call(h, ver_c, tri_c, ti_c, B, nver, ntri, H, W, dev)
        ctx.save_for_backward(ver_c, tri_c, ti_c)
        ctx.dims = (B, nver, ntri, H, W)
        return depth

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        h = _host()
        ver_c, tri_c, ti_c = ctx.saved_tensors
        B, nver, ntri, H, W = ctx.dims
        dev = ver_c.device
        vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _depth_interp_backward_call(h, h.require_gpu_f32(g, "depth_grad"), ver_c, tri_c, ti_c, vertex_grad, B, nver, ntri, H, W,
                                        0, dev)
        return vertex_grad, None, None


def depth_interpolate(ver, tri, tri_ind):
    """The interpolated depth [B,H,W,1] of a render's winners: per pixel whose tri_ind ([B,H,W,1], e.g. render_depth's fourth
    output) names a triangle of `tri` [3,ntri], the z of that triangle's plane at the pixel by the barycentric weights of
    get_point_weight (fr_depth_interp_forward: float64, one gather pass); the op's background elsewhere, the flat centroid depth
    for a triangle without area.  Which triangle wins is not re-decided.  The gradient goes to `ver` [B,3,nver] only, to all three
    rows: moving a vertex sideways slides the plane under the pixel (fr_depth_interp_backward: bit-reproducible); a tri_ind that
    requires grad is refused.  The node saves `ver`, `tri` and `tri_ind`."""
    return _DepthInterpolate.apply(ver, tri, tri_ind)


def _attr_interp_scratch(B, H, W):
    """(int32 elements of `records`, uint32 elements of `partial`) of fr_attr_interp_backward (include/fr_hotpath.h)"""
    npix = H * W
    return 2 * B * 3 * npix * 4, 2 * B * ((npix + 1023) // 1024) * 2


class _AttrInterpolate(torch.autograd.Function):
    """fr_attr_interp_forward / _backward (include/fr_hotpath.h, "smooth planes") as one autograd node."""

    @staticmethod
    def forward(ctx, ver, attr, tri, tri_ind):
        h = _host()
        if isinstance(tri_ind, torch.Tensor) and tri_ind.requires_grad:
            raise ValueError("attr_interpolate: tri_ind requires grad, but the winning triangles are held fixed (detach it)")
        ver_c = h.require_gpu_f32(ver, "ver")
        attr_c = h.require_gpu_f32(attr, "attr")
        tri_c = h.require_gpu_f32(tri, "tri")
        ti_c = h.require_gpu_f32(tri_ind, "tri_ind")
        _check_ver(ver_c)
        _check_tri(tri_c)
        if tuple(attr_c.shape) != tuple(ver_c.shape):
            raise ValueError("attr_interpolate expects attr [B,3,nver] like ver %s (got %s)" % (tuple(ver_c.shape), tuple(attr_c.shape)))
        if ti_c.dim() != 4 or ti_c.shape[0] != ver_c.shape[0] or ti_c.shape[3] != 1:
            raise ValueError("attr_interpolate expects tri_ind [B,H,W,1] with the vertex's batch (got %s)" % (tuple(ti_c.shape),))
        if tri_c.device != ver_c.device or ti_c.device != ver_c.device or attr_c.device != ver_c.device:
            raise ValueError("attr_interpolate: ver, attr, tri and tri_ind must be on one device")
        B, H, W = int(ti_c.shape[0]), int(ti_c.shape[1]), int(ti_c.shape[2])
        nver, ntri = int(ver_c.shape[2]), int(tri_c.shape[1])
        dev = ver_c.device
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = h.lib().fr_attr_interp_forward(h.ptr(ver_c), nver, h.ptr(attr_c), nver, h.ptr(tri_c), h.ptr(ti_c), B, nver, ntri, H, W,
                                                h.ptr(out), h.stream_ptr(dev))
        h.check(rc, "fr_attr_interp_forward")
        ctx.save_for_backward(ver_c, attr_c, tri_c, ti_c)
        ctx.dims = (B, nver, ntri, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        need_ver, need_attr = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_ver or need_attr):
            return None, None, None, None
        h = _host()
        ver_c, attr_c, tri_c, ti_c = ctx.saved_tensors
        B, nver, ntri, H, W = ctx.dims
        dev = ver_c.device
        if B * H * W == 0 or nver == 0:   # the entry point writes nothing for an empty image
            z = lambda need: torch.zeros((B, 3, nver), dtype=torch.float32, device=dev) if need else None   # noqa: E731
            return z(need_ver), z(need_attr), None, None
        vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev) if need_ver else None
        attr_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev) if need_attr else None
        g_c = h.require_gpu_f32(g, "grad")
        nrec, npart = _attr_interp_scratch(B, H, W)
        # (both are dead once the launches are enqueued: one buffer per stream, under the pool's hold; `partial` behind `records`,
        # whose byte count is a multiple of 16)
        with torch.cuda.device(dev), _KINDS_POOL.hold("attr_interp_bwd", dev, 4 * (nrec + npart)) as ent:
            base = ent.buf.data_ptr()
            rc = h.lib().fr_attr_interp_backward(h.ptr(g_c), h.ptr(ver_c), nver, h.ptr(attr_c), nver, h.ptr(tri_c), h.ptr(ti_c),
                                                 h.ptr(attr_grad), 0, h.ptr(vertex_grad), 0, B, nver, ntri, H, W,
                                                 ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * nrec), h.stream_ptr(dev))
        h.check(rc, "fr_attr_interp_backward")
        return vertex_grad, attr_grad, None, None


def attr_interpolate(ver, attr, tri, tri_ind):
    """A three-channel per-vertex attribute interpolated at the pixel -> [B,H,W,3]: per pixel whose tri_ind ([B,H,W,1], e.g.
    render_depth's fourth output) names a triangle (p1, p2, p3) of `tri` [3,ntri], w1 attr[p1] + w2 attr[p2] + w3 attr[p3] with the
    barycentric weights of depth_interpolate (fr_attr_interp_forward: float64, one gather pass); (+0, +0, +0) where no triangle
    wins, the render's flat texture lookup (the mean of the three) for a triangle without area.  Which triangle wins is not
    re-decided, and nothing is normalised: a plane of interpolated normals is normalised by its consumer.  `ver` is [B,3,nver];
    `attr` is [B,3,nver], or a shared [3,nver] / [1,3,nver], which is expanded to the batch and made dense first -- its gradient is
    therefore torch's sum of the per-face gradients over the faces, in torch's order.  Gradients go to `attr` and to the x and y
    rows of `ver` (the z row is +0): moving a vertex sideways slides the attribute under the pixel (fr_attr_interp_backward:
    bit-reproducible; only the gradients autograd needs are formed); a tri_ind that requires grad is refused.  The node saves
    `ver`, `attr`, `tri` and `tri_ind`."""
    if isinstance(attr, torch.Tensor) and isinstance(ver, torch.Tensor) and ver.dim() == 3:
        if attr.dim() == 2:
            attr = attr.unsqueeze(0)
        if attr.dim() == 3 and attr.shape[0] == 1 and ver.shape[0] != 1:
            attr = attr.expand(ver.shape[0], -1, -1)
        attr = attr.contiguous()
    return _AttrInterpolate.apply(ver, attr, tri, tri_ind)


class _SoftCoverage(torch.autograd.Function):
    """fr_coverage_forward / _backward (include/fr_hotpath.h, "soft coverage") as one autograd node."""

    @staticmethod
    def forward(ctx, ver, tri, tri_ind):
        h = _host()
        if isinstance(tri_ind, torch.Tensor) and tri_ind.requires_grad:
            raise ValueError("soft_coverage: tri_ind requires grad, but the winning triangles are held fixed (detach it)")
        ver_c = h.require_gpu_f32(ver, "ver")
        tri_c = h.require_gpu_f32(tri, "tri")
        ti_c = h.require_gpu_f32(tri_ind, "tri_ind")
        _check_ver(ver_c)
        _check_tri(tri_c)
        if ti_c.dim() != 4 or ti_c.shape[0] != ver_c.shape[0] or ti_c.shape[3] != 1:
            raise ValueError("soft_coverage expects tri_ind [B,H,W,1] with the vertex's batch (got %s)" % (tuple(ti_c.shape),))
        if tri_c.device != ver_c.device or ti_c.device != ver_c.device:
            raise ValueError("soft_coverage: ver, tri and tri_ind must be on one device")
        B, H, W = int(ti_c.shape[0]), int(ti_c.shape[1]), int(ti_c.shape[2])
        nver, ntri = int(ver_c.shape[2]), int(tri_c.shape[1])
        dev = ver_c.device
        cov = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = h.lib().fr_coverage_forward(h.ptr(ver_c), nver, h.ptr(tri_c), h.ptr(ti_c), B, nver, ntri, H, W, h.ptr(cov),
                                             h.stream_ptr(dev))
        h.check(rc, "fr_coverage_forward")
        ctx.save_for_backward(ver_c, tri_c, ti_c, cov)
        ctx.dims = (B, nver, ntri, H, W)
        return cov

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        h = _host()
        ver_c, tri_c, ti_c, cov = ctx.saved_tensors
        B, nver, ntri, H, W = ctx.dims
        dev = ver_c.device
        if B * H * W == 0 or nver == 0:   # the entry point writes nothing for an empty image
            return torch.zeros((B, 3, nver), dtype=torch.float32, device=dev), None, None
        vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
        g_c = h.require_gpu_f32(g, "cov_grad")
        L = h.lib()
        nws = L.fr_coverage_backward_workspace_bytes(B, nver, H, W)
        # (the workspace is dead once the two launches are enqueued: one per stream, under the pool's hold)
        with torch.cuda.device(dev), _KINDS_POOL.hold("coverage_bwd", dev, nws) as ent:
            rc = L.fr_coverage_backward(h.ptr(g_c), h.ptr(cov), h.ptr(ver_c), nver, h.ptr(tri_c), h.ptr(ti_c), h.ptr(vertex_grad), B,
                                        nver, ntri, H, W, 0, h.ptr(ent.buf), ent.nbytes, h.stream_ptr(dev))
        h.check(rc, "fr_coverage_backward")
        return vertex_grad, None, None


def soft_coverage(ver, tri, tri_ind):
    """The soft silhouette [B,H,W,1] of a render's winners, in [0, 1]: 1 on a pixel whose tri_ind ([B,H,W,1], e.g. render_depth's
    fourth output) names a triangle of `tri` [3,ntri] and whose four neighbours do too, +0 on a background pixel among background
    pixels, and on the pixels either side of the face / background border the share of the pixel the face covers along the line
    to its neighbour (fr_coverage_forward: float64, one pass).  Which triangle wins is not re-decided.  The gradient goes to the x
    and y rows of `ver` [B,3,nver] (the z row is +0): moving the border's vertices moves the border (fr_coverage_backward:
    bit-reproducible); a tri_ind that requires grad is refused.  Only the face / background border is soft -- not an occlusion edge
    inside the face.  The node saves `ver`, `tri`, `tri_ind` and the plane itself."""
    return _SoftCoverage.apply(ver, tri, tri_ind)


# ---- fine mesh (include/fr_hotpath.h, "fine mesh"): forward only, outside autograd ------------------------------------------------------
def _mesh_plane(h, t, name, op, B, H, W, dev):
    """a [B,H,W,1] or [B,H,W] fp32 plane on `dev`, detached and contiguous"""
    t_c = h.require_gpu_f32(t.detach() if isinstance(t, torch.Tensor) else t, name)
    _check_plane(op, name, t_c, B, H, W, 1, dev, "vertex", flat=True)
    return t_c


def _mesh_tri_ind(h, tri_ind, op):
    ti_c = h.require_gpu_f32(tri_ind.detach() if isinstance(tri_ind, torch.Tensor) else tri_ind, "tri_ind")
    if not (ti_c.dim() == 3 or (ti_c.dim() == 4 and ti_c.shape[3] == 1)):
        raise ValueError("%s expects tri_ind [B,H,W,1] or [B,H,W] (got %s)" % (op, tuple(ti_c.shape)))
    return ti_c, int(ti_c.shape[0]), int(ti_c.shape[1]), int(ti_c.shape[2])


def mesh_visible(tri, tri_ind, nver):
    """The per-vertex visibility of a render: uint8 [B,nver], 1 where at least one pixel of the face's tri_ind ([B,H,W,1] or
    [B,H,W], e.g. render_depth's fourth output) names a triangle of `tri` [3,ntri] that has the vertex among its three ids, else 0
    (fr_mesh_visible: one pass over the pixels; a function of the inputs alone).  A pixel counts exactly as in the render
    backwards: -1, NaN, a value >= ntri or a triangle with an id outside [0, nver) marks nothing.  Outside autograd: the inputs are
    read as constants and the result does not require grad.  Runs on the current stream."""
    h = _host()
    tri_c = h.require_gpu_f32(tri.detach() if isinstance(tri, torch.Tensor) else tri, "tri")
    _check_tri(tri_c)
    ti_c, B, H, W = _mesh_tri_ind(h, tri_ind, "mesh_visible")
    if ti_c.device != tri_c.device:
        raise ValueError("mesh_visible: tri_ind is on %s, tri on %s" % (ti_c.device, tri_c.device))
    nver = int(nver)
    if nver < 0:
        raise ValueError("mesh_visible: nver must not be negative")
    dev = tri_c.device
    visible = torch.empty((B, nver), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = h.lib().fr_mesh_visible(h.ptr(tri_c), h.ptr(ti_c), B, nver, int(tri_c.shape[1]), H, W, h.ptr(visible),
                                     h.stream_ptr(dev))
    h.check(rc, "fr_mesh_visible")
    return visible


def mesh_lift(vertex, tri_ind, visible, fine_depth, coarse_depth, ntri=None):
    """The fine depth map lifted onto the vertices -> (vertex_fine [B,3,nver] fp32, state uint8 [B,nver]).  Rows x and y are
    `vertex`'s, bit for bit.  A visible vertex (`visible` uint8 [B,nver], mesh_visible) whose position (x = column, y = row) has
    at least one of its four surrounding pixels on the face gets z + the bilinear sample of fine_depth - coarse_depth over those
    of the four that are (state 1); a visible vertex without such a pixel, or at a non-finite position, keeps its z (state 2); a
    hidden one keeps it (state 0) (fr_mesh_lift: float64, one gather pass, bit-exact against numpy).  tri_ind, fine_depth and
    coarse_depth are [B,H,W,1] or [B,H,W]; a pixel is on the face when its tri_ind names a triangle in [0, ntri) (ntri=None: any
    non-negative id does).  Outside autograd: every input is read as a constant, neither output requires grad.  Runs on the
    current stream."""
    h = _host()
    ver_c = h.require_gpu_f32(vertex.detach() if isinstance(vertex, torch.Tensor) else vertex, "vertex")
    _check_ver(ver_c)
    dev = ver_c.device
    ti_c, B, H, W = _mesh_tri_ind(h, tri_ind, "mesh_lift")
    nver = int(ver_c.shape[2])
    if B != int(ver_c.shape[0]) or ti_c.device != dev:
        raise ValueError("mesh_lift: tri_ind must have the vertex's batch and device (got %s on %s)" % (tuple(ti_c.shape), ti_c.device))
    if not (isinstance(visible, torch.Tensor) and visible.dtype == torch.uint8 and tuple(visible.shape) == (B, nver)
            and visible.device == dev):
        raise ValueError("mesh_lift: visible must be a uint8 tensor [%d,%d] on %s (mesh_visible)" % (B, nver, dev))
    f_c = _mesh_plane(h, fine_depth, "fine_depth", "mesh_lift", B, H, W, dev)
    c_c = _mesh_plane(h, coarse_depth, "coarse_depth", "mesh_lift", B, H, W, dev)
    ntri = (1 << 24) - 1 if ntri is None else int(ntri)
    vis_c = visible.contiguous()
    out = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
    state = torch.empty((B, nver), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = h.lib().fr_mesh_lift(h.ptr(ver_c), nver, h.ptr(ti_c), h.ptr(vis_c), h.ptr(f_c), h.ptr(c_c), B, nver,
                                  ntri, H, W, h.ptr(out), nver, h.ptr(state), h.stream_ptr(dev))
    h.check(rc, "fr_mesh_lift")
    return out, state


class MeshAdjacency:
    """A vertex -> triangle CSR table (utils/mesh_io.vertex_adjacency) checked on the host and held on a device: adj_start int32
    [nver + 1] starts at 0, never decreases and ends at most at 3 ntri (at 3 ntri unless a triangle names a vertex twice or an id
    outside the mesh); adj_tri int32 [3 ntri] holds ids in [0, ntri).  ValueError otherwise -- the kernel trusts what passed."""

    def __init__(self, adj_start, adj_tri, nver, ntri, device):
        import numpy as np
        s = np.ascontiguousarray(np.asarray(adj_start.cpu() if isinstance(adj_start, torch.Tensor) else adj_start))
        t = np.ascontiguousarray(np.asarray(adj_tri.cpu() if isinstance(adj_tri, torch.Tensor) else adj_tri))
        nver, ntri = int(nver), int(ntri)
        if s.dtype.kind not in "iu" or t.dtype.kind not in "iu":
            raise ValueError("adjacency: adj_start and adj_tri must be integer arrays")
        if s.shape != (nver + 1,) or t.shape != (3 * ntri,):
            raise ValueError("adjacency: adj_start must be [%d] and adj_tri [%d] (got %s, %s)" % (nver + 1, 3 * ntri, s.shape, t.shape))
        s64, t64 = s.astype(np.int64), t.astype(np.int64)
        if s64[0] != 0 or (np.diff(s64) < 0).any() or s64[-1] > 3 * ntri:
            raise ValueError("adjacency: adj_start must start at 0, never decrease and end at most at 3 ntri = %d" % (3 * ntri))
        if t64.size and (t64.min() < 0 or t64.max() >= ntri):
            raise ValueError("adjacency: adj_tri names a triangle outside [0, %d)" % ntri)
        self.nver, self.ntri = nver, ntri
        self.adj_start = torch.as_tensor(s.astype(np.int32), device=device)
        self.adj_tri = torch.as_tensor(t.astype(np.int32), device=device)


class _VertexNormals(torch.autograd.Function):
    """fr_mesh_vertex_normals / _backward (include/fr_hotpath.h, "smooth planes") as one autograd node over a checked adjacency."""

    @staticmethod
    def forward(ctx, vertex, tri, adjacency):
        normal = vertex_normals(vertex, tri, adjacency)
        ctx.save_for_backward(_host().require_gpu_f32(vertex.detach(), "vertex"), _host().require_gpu_f32(tri.detach(), "tri"))
        ctx.adjacency = adjacency
        return normal

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        h = _host()
        ver_c, tri_c = ctx.saved_tensors
        adj = ctx.adjacency
        B, nver, ntri = int(ver_c.shape[0]), int(ver_c.shape[2]), int(tri_c.shape[1])
        dev = ver_c.device
        if B == 0 or nver == 0:   # the entry point writes nothing
            return torch.zeros((B, 3, nver), dtype=torch.float32, device=dev), None, None
        g_c = h.require_gpu_f32(g, "normal_grad")
        vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
        # (h is dead once the two launches are enqueued: one per stream, under the pool's hold)
        with torch.cuda.device(dev), _KINDS_POOL.hold("vertex_normals_bwd", dev, 8 * B * 3 * nver) as ent:
            rc = h.lib().fr_mesh_vertex_normals_backward(h.ptr(g_c), nver, h.ptr(ver_c), nver, h.ptr(tri_c), h.ptr(adj.adj_start),
                                                         h.ptr(adj.adj_tri), B, nver, ntri, h.ptr(ent.buf), h.ptr(vertex_grad), nver,
                                                         0, h.stream_ptr(dev))
        h.check(rc, "fr_mesh_vertex_normals_backward")
        return vertex_grad, None, None


def vertex_normals(vertex, tri, adjacency, grad=False):
    """Per-vertex unit normals [B,3,nver] fp32 of a vertex tensor [B,3,nver] over the triangles `tri` [3,ntri]: the area-weighted
    sum of (P2 - P1) x (P3 - P1) -- the render's orientation -- over the vertex's triangles in the order of `adjacency`, normalised;
    exactly (0, 0, 0) for a vertex without a triangle or whose sum vanishes (fr_mesh_vertex_normals: float64 chains in table
    order, one gather pass, bit-exact against numpy).  adjacency: a MeshAdjacency (checked once, e.g. FaceRecNet.adjacency()) or
    the (adj_start, adj_tri) pair of utils/mesh_io.vertex_adjacency (checked and uploaded by this call).  grad=False (default):
    outside autograd -- the inputs are read as constants, the result does not require grad.  grad=True: an autograd node with the
    same forward bits whose gradient goes to `vertex` (fr_mesh_vertex_normals_backward: two float64 gathers, bit-exact against
    numpy; the forward's rounding to fp32 is not differentiated, and a vertex whose normal is (0, 0, 0) passes nothing on); the
    node saves `vertex`, `tri` and the adjacency.  Runs on the current stream."""
    h = _host()
    if grad:
        if not hasattr(adjacency, "adj_start"):
            adj_start, adj_tri = adjacency
            adjacency = MeshAdjacency(adj_start, adj_tri, int(vertex.shape[2]), int(tri.shape[1]), vertex.device)
        return _VertexNormals.apply(vertex, tri, adjacency)
    ver_c = h.require_gpu_f32(vertex.detach() if isinstance(vertex, torch.Tensor) else vertex, "vertex")
    tri_c = h.require_gpu_f32(tri.detach() if isinstance(tri, torch.Tensor) else tri, "tri")
    _check_ver(ver_c)
    _check_tri(tri_c)
    dev = ver_c.device
    if tri_c.device != dev:
        raise ValueError("vertex_normals: tri is on %s, vertex on %s" % (tri_c.device, dev))
    B, nver, ntri = int(ver_c.shape[0]), int(ver_c.shape[2]), int(tri_c.shape[1])
    if not hasattr(adjacency, "adj_start"):   # (not isinstance: this file is loaded under two module names)
        adj_start, adj_tri = adjacency
        adjacency = MeshAdjacency(adj_start, adj_tri, nver, ntri, dev)
    if adjacency.nver != nver or adjacency.ntri != ntri or adjacency.adj_start.device != dev:
        raise ValueError("vertex_normals: the adjacency is of a mesh of %d vertices and %d triangles on %s, the call's has %d and %d on %s"
                         % (adjacency.nver, adjacency.ntri, adjacency.adj_start.device, nver, ntri, dev))
    normal = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = h.lib().fr_mesh_vertex_normals(h.ptr(ver_c), nver, h.ptr(tri_c), h.ptr(adjacency.adj_start), h.ptr(adjacency.adj_tri),
                                            B, nver, ntri, h.ptr(normal), nver, h.stream_ptr(dev))
    h.check(rc, "fr_mesh_vertex_normals")
    return normal


_LAPLACE_K = ((0.5, 1.0, 0.5), (1.0, -6.0, 1.0), (0.5, 1.0, 0.5))  # network.py:383-385


def _fine_losses_planes(h, pred, coarse):
    """-> (pred, coarse) contiguous fp32 on one GPU, and (B, H, W)"""
    p_c = h.require_gpu_f32(pred, "pred")
    c_c = h.require_gpu_f32(coarse, "coarse")
    if p_c.dim() == 4 and p_c.shape[3] == 1:
        B, H, W = int(p_c.shape[0]), int(p_c.shape[1]), int(p_c.shape[2])
    elif p_c.dim() == 3:
        B, H, W = (int(v) for v in p_c.shape)
    else:
        raise ValueError("fine_depth_losses expects pred [B,H,W,1] or [B,H,W] (got %s)" % (tuple(p_c.shape),))
    _check_plane("fine_depth_losses", "coarse", c_c, B, H, W, 1, p_c.device, "pred", flat=True)
    return p_c, c_c, (B, H, W)


class _FineDepthLosses(torch.autograd.Function):
    """fr_fine_losses_forward / _backward (include/fr_hotpath.h, "fine-depth losses") as one autograd node: (pred, coarse) ->
    (fidelity, smoothness), two 0-dim fp32 tensors.  It saves pred and coarse and nothing plane-sized of its own: the backward
    recomputes the signs from pred.  The forward's state (two float64 partials per tile) is dead once the forward has run, so it
    is the pooled per-stream buffer of kind "fine_losses", held across the forward's two launches.  A gradient that never arrives
    (an output nobody used) is passed as NULL and its term is not evaluated."""

    @staticmethod
    def forward(ctx, pred, coarse):
        h = _host()
        L = h.lib()
        p_c, c_c, (B, H, W) = _fine_losses_planes(h, pred, coarse)
        dev = p_c.device
        out = torch.empty((2,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nst = L.fr_fine_losses_state_bytes(B, H, W)
            with _KINDS_POOL.hold("fine_losses", dev, nst) as ent:
                rc = L.fr_fine_losses_forward(p_c.data_ptr(), c_c.data_ptr(), B, H, W, out.data_ptr(), out.data_ptr() + 4,
                                              ent.buf.data_ptr(), nst, ent.stream)   # (the hold has asked for the stream)
        if rc:
            h.check(rc, "fr_fine_losses_forward")
        ctx.save_for_backward(p_c, c_c)
        ctx.dims = (B, H, W)
        ctx.shapes = (tuple(pred.shape), tuple(coarse.shape))
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_fidelity, g_smoothness):
        h = _host()
        p_c, c_c = ctx.saved_tensors
        B, H, W = ctx.dims
        dev = p_c.device
        gf = h.require_gpu_f32(g_fidelity, "grad_fidelity") if g_fidelity is not None else None
        gs = h.require_gpu_f32(g_smoothness, "grad_smoothness") if g_smoothness is not None else None
        gp = torch.empty(ctx.shapes[0], dtype=torch.float32, device=dev)
        gc = torch.empty(ctx.shapes[1], dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            rc = h.lib().fr_fine_losses_backward(h.ptr(gf), h.ptr(gs), p_c.data_ptr(), c_c.data_ptr(), B, H, W, gp.data_ptr(),
                                                 h.ptr(gc), torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            h.check(rc, "fr_fine_losses_backward")
        return (gp if ctx.needs_input_grad[0] else None), gc


def fine_depth_losses(pred, coarse):
    """(fidelity, smoothness) of the fine depth map `pred` against the coarse one, both [B,H,W,1] (or [B,H,W]): 0-dim fp32 tensors
    equal to `F.mse_loss(pred, coarse)` and `laplace_transform(pred[..., 0]).abs().sum()` (nets/losses.py) up to rounding -- float64
    sums in a fixed association instead of fp32 reductions (fr_fine_losses_forward: one pass and a finish launch).  The gradient
    goes to `pred` and, where it requires grad, to `coarse`, each in its own shape (fr_fine_losses_backward: one gather pass,
    bit-reproducible, the incoming scalar gradients read from the device).  The node saves `pred` and `coarse`.  An empty batch
    or image takes the stock torch expressions."""
    if pred.numel() == 0:
        import torch.nn.functional as F
        x = pred.reshape(pred.shape[0], pred.shape[1], pred.shape[2])
        k = torch.tensor(_LAPLACE_K, dtype=x.dtype, device=x.device)[None, None]
        return F.mse_loss(pred, coarse), F.conv2d(x[:, None], k, padding=1)[:, 0].abs().sum()
    return _FineDepthLosses.apply(pred, coarse)


def albedo_basis(tri, pc_tex):
    """Phi [T,K] float64: the texture basis `pc_tex` [3N,K] seen through the rasteriser's lookup for the triangles `tri` [3,T]
    (float ids) -- Phi[t][k] = (1/9) sum over the three channels and the three vertices of pc_tex[c N + v_j(t), k]
    (fr_albedo_basis_build: nine widened terms in a fixed order, bit-exact against numpy).  Built once per mesh
    (FaceRecNet.albedo_basis caches it); 1 <= K <= 15.  Runs on the current stream."""
    h = _host()
    tri_c = h.require_gpu_f32(tri, "tri")
    pc_c = h.require_gpu_f32(pc_tex, "pc_tex")
    _check_tri(tri_c)
    if pc_c.dim() != 2 or pc_c.shape[0] % 3 != 0:
        raise ValueError("albedo_basis expects pc_tex [3N,K] (got %s)" % (tuple(pc_c.shape),))
    if pc_c.device != tri_c.device:
        raise ValueError("albedo_basis: pc_tex is on %s, tri on %s" % (pc_c.device, tri_c.device))
    T, K, nver = int(tri_c.shape[1]), int(pc_c.shape[1]), int(pc_c.shape[0]) // 3
    dev = tri_c.device
    L = h.lib()
    basis = torch.empty((T, K), dtype=torch.float64, device=dev)
    nbytes = L.fr_albedo_basis_bytes(T, K)
    with torch.cuda.device(dev):
        rc = L.fr_albedo_basis_build(h.ptr(tri_c), h.ptr(pc_c), nver, T, K, h.ptr(basis), nbytes, h.stream_ptr(dev))
    h.check(rc, "fr_albedo_basis_build")
    return basis


def sfs_lighting(abedo, normal, im_gray, rcond=1e-15):
    """The per-pixel lighting l [3,H,W] float64 of the fused SfS solve, without the shading: fr_sfs_moments then fr_sfs_lighting,
    planes 6-8 of the state -- the very bits sfs_intensity's forward holds for the same maps.  abedo, im_gray [B,H,W,1] and normal
    [B,H,W,3] are constants here (the result does not require grad).  Runs on the current stream; the moments live in the
    per-stream scratch, the state is the call's own (the result is a view of it)."""
    h = _host()
    a_c = h.require_gpu_f32(abedo.detach(), "abedo")
    n_c = h.require_gpu_f32(normal.detach(), "normal")
    i_c = h.require_gpu_f32(im_gray.detach(), "im_gray")
    if n_c.dim() != 4 or n_c.shape[3] != 3:
        raise ValueError("sfs_lighting expects normal [B,H,W,3]")
    B, H, W = int(n_c.shape[0]), int(n_c.shape[1]), int(n_c.shape[2])
    dev = n_c.device
    for t, name in ((a_c, "abedo"), (i_c, "im_gray")):
        _check_plane("sfs_lighting", name, t, B, H, W, 1, dev, "normal")
    L = h.lib()
    state = torch.empty((10, H, W), dtype=torch.float64, device=dev)
    if H * W == 0:
        return state[6:9]
    nst, nmo = L.fr_sfs_state_bytes(H, W), L.fr_sfs_moments_bytes(H, W)
    with torch.cuda.device(dev), _KINDS_POOL.hold("sfs_lighting", dev, nmo) as ent:
        rc = L.fr_sfs_moments(h.ptr(a_c), h.ptr(n_c), h.ptr(i_c), B, H, W, h.ptr(ent.buf), nmo, h.stream_ptr(dev))
        h.check(rc, "fr_sfs_moments")
        rc = L.fr_sfs_lighting(h.ptr(ent.buf), 1, H, W, float(rcond), h.ptr(state), nst, h.stream_ptr(dev))
    h.check(rc, "fr_sfs_lighting")
    return state[6:9]


def albedo_lse(basis, tri_ind, lighting, normal_new, abedo, im_gray, ridge=1e-6):
    """The per-face least-squares albedo coefficients (fr_albedo_lse_forward): per face b the alpha_b that minimises
    sum_p (I - (a + Phi[tri_ind] . alpha) (l . n'))^2 + lambda |alpha|^2 over the pixels the face covers, lambda = ridge x the mean
    diagonal of the face's Gram matrix.  basis [T,K] float64 (albedo_basis), tri_ind / abedo / im_gray [B,H,W,1], lighting [3,H,W]
    float64 (sfs_lighting), normal_new [B,H,W,3].  -> (alpha [B,K] fp32, stats [B,4] float64 = {counted pixels, E0 = the residual
    energy at alpha = 0, E1 = at the returned alpha, ok}); a face that cannot be fitted (no pixel, a pivot that vanishes, a
    non-finite input) gets alpha = 0 and ok = 0.  alpha is a fitted quantity: neither output requires grad, every input is read as
    a constant.  float64 sums in a fixed association (a function of H, W and K alone), bit-reproducible.  Runs on the current
    stream with the per-stream scratch as its workspace."""
    h = _host()
    ti_c = h.require_gpu_f32(tri_ind.detach(), "tri_ind")
    n_c = h.require_gpu_f32(normal_new.detach(), "normal_new")
    a_c = h.require_gpu_f32(abedo.detach(), "abedo")
    i_c = h.require_gpu_f32(im_gray.detach(), "im_gray")
    if n_c.dim() != 4 or n_c.shape[3] != 3:
        raise ValueError("albedo_lse expects normal_new [B,H,W,3]")
    B, H, W = int(n_c.shape[0]), int(n_c.shape[1]), int(n_c.shape[2])
    dev = n_c.device
    for t, name in ((ti_c, "tri_ind"), (a_c, "abedo"), (i_c, "im_gray")):
        _check_plane("albedo_lse", name, t, B, H, W, 1)   # (their devices are checked with the basis's and the lighting's, below)
    if not (isinstance(basis, torch.Tensor) and basis.dtype == torch.float64 and basis.dim() == 2):
        raise ValueError("albedo_lse: basis must be a float64 tensor [T,K] (albedo_basis)")
    if not (isinstance(lighting, torch.Tensor) and lighting.dtype == torch.float64 and tuple(lighting.shape) == (3, H, W)):
        raise ValueError("albedo_lse: lighting must be a float64 tensor [3,%d,%d] (sfs_lighting)" % (H, W))
    for t, name in ((ti_c, "tri_ind"), (a_c, "abedo"), (i_c, "im_gray"), (basis, "basis"), (lighting, "lighting")):
        if t.device != dev:
            raise ValueError("albedo_lse: %s is on %s, normal_new on %s" % (name, t.device, dev))
    b_c, l_c = basis.detach().contiguous(), lighting.detach().contiguous()
    T, K = int(b_c.shape[0]), int(b_c.shape[1])
    L = h.lib()
    make = torch.zeros if B * H * W == 0 else torch.empty   # (an empty shape launches nothing: alpha = 0, ok = 0)
    alpha = make((B, K), dtype=torch.float32, device=dev)
    moments = make((B, 16, 16), dtype=torch.float64, device=dev)   # (the C call's third output; not returned)
    stats = make((B, 4), dtype=torch.float64, device=dev)
    nws = L.fr_albedo_lse_workspace_bytes(B, H, W, K)
    with torch.cuda.device(dev), _KINDS_POOL.hold("albedo_lse", dev, nws) as ent:
        rc = L.fr_albedo_lse_forward(h.ptr(b_c), h.ptr(ti_c), h.ptr(l_c), h.ptr(n_c), h.ptr(a_c), h.ptr(i_c), B, T, H, W, K,
                                     float(ridge), h.ptr(alpha), h.ptr(moments), h.ptr(stats), h.ptr(ent.buf), ent.nbytes,
                                     h.stream_ptr(dev))
    h.check(rc, "fr_albedo_lse_forward")
    return alpha, stats


SYNTH_LIGHT_RANGES = ((0.3, 0.7), (-0.4, 0.4), (-0.4, 0.4), (0.2, 0.9))   # (l0, lx, ly, lz): ambient, then a frontal light


def _synth_ranges(ranges, n, name):
    """n (lo, hi) pairs -> a host float array the C call reads; a scalar s means (-s, s) for every component"""
    if n == 0:
        return None
    if isinstance(ranges, (int, float)):
        ranges = [(-abs(float(ranges)), abs(float(ranges)))] * n
    flat = [float(v) for pair in ranges for v in pair]
    if len(flat) != 2 * n:
        raise ValueError("%s must be %d (lo, hi) pairs" % (name, n))
    return (ctypes.c_float * (2 * n))(*flat)


def synth_params(seed, first_face, batch, n_shape, n_exp, n_tex, im_size, beta=0.7, light_ranges=SYNTH_LIGHT_RANGES,
                 alpha_ranges=1.0, focal=1e-3, device=None, out=None):
    """`batch` faces of random parameters drawn on the device (fr_synth_params): Philox4x32-10 keyed by `seed`, counted by the
    GLOBAL face index first_face + b, so a face's values do not depend on the batch, the call or the rank that drew it.
    -> (params [B, 7 + n_shape + n_exp] in the 235-d layout with the distributions of utils/synth.get_random_params, light [B,4],
    alpha [B,n_tex]), the last two uniform in light_ranges / alpha_ranges ((lo, hi) pairs per component; a scalar s means
    (-s, s)).  focal: the reference's 1e-3; a smaller image takes a smaller one.  out: three tensors to write instead of fresh
    ones.  A data source: nothing requires grad.  Runs on the current stream."""
    h = _host()
    B, ns, ne, K = int(batch), int(n_shape), int(n_exp), int(n_tex)
    if out is None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("synth_params draws on an MI355X only (no CPU fallback); got %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        f32 = dict(dtype=torch.float32, device=dev)
        out = (torch.empty((B, 7 + ns + ne), **f32), torch.empty((B, 4), **f32), torch.empty((B, K), **f32))
    params, light, alpha = out
    for t, name, shape in ((params, "params", (B, 7 + ns + ne)), (light, "light", (B, 4)), (alpha, "alpha", (B, K))):
        if h.require_gpu_f32(t, name) is not t or tuple(t.shape) != shape:
            raise ValueError("synth_params: out %s must be a contiguous float32 tensor %s" % (name, shape))
    dev = params.device
    lr = _synth_ranges(light_ranges, 4, "light_ranges")
    ar = _synth_ranges(alpha_ranges, K, "alpha_ranges")
    with torch.cuda.device(dev):
        rc = h.lib().fr_synth_params(int(seed) & (2 ** 64 - 1), int(first_face) & (2 ** 64 - 1), B, ns, ne, K, float(im_size),
                                     float(beta), float(focal), lr, ar, h.ptr(params), h.ptr(light),
                                     h.ptr(alpha) if K > 0 else None, h.stream_ptr(dev))
    h.check(rc, "fr_synth_params")
    return params, light, alpha


def _synth_texture_call(mu_tex, pc_tex, alpha, out=None):
    """fr_synth_texture on constants -> (tex [B,3,N], the contiguous pc_tex it read or None)"""
    h = _host()
    mu_c = h.require_gpu_f32(mu_tex.detach(), "mu_tex")
    al_c = h.require_gpu_f32(alpha.detach(), "alpha")
    if mu_c.dim() != 2 or mu_c.shape[0] != 3:
        raise ValueError("synth_texture expects mu_tex [3,N]")
    if al_c.dim() != 2:
        raise ValueError("synth_texture expects alpha [B,K]")
    N, B, K = int(mu_c.shape[1]), int(al_c.shape[0]), int(al_c.shape[1])
    dev = mu_c.device
    pc_c = None
    if K > 0:
        pc_c = h.require_gpu_f32(pc_tex.detach(), "pc_tex")
        if tuple(pc_c.shape) != (3 * N, K):
            raise ValueError("synth_texture: pc_tex must be [%d,%d] (got %s)" % (3 * N, K, tuple(pc_c.shape)))
    for t, name in ((al_c, "alpha"), (pc_c, "pc_tex")):
        if t is not None and t.device != dev:
            raise ValueError("synth_texture: %s is on %s, mu_tex on %s" % (name, t.device, dev))
    if out is None:
        out = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
    elif h.require_gpu_f32(out, "out") is not out or tuple(out.shape) != (B, 3, N) or out.device != dev:
        raise ValueError("synth_texture: out must be a contiguous float32 tensor [%d,3,%d] on %s" % (B, N, dev))
    with torch.cuda.device(dev):
        rc = h.lib().fr_synth_texture(h.ptr(mu_c), h.ptr(pc_c), h.ptr(al_c) if K > 0 else None, B, N, K, h.ptr(out),
                                      h.stream_ptr(dev))
    h.check(rc, "fr_synth_texture")
    return out, pc_c


def synth_texture_backward(pc_tex, grad_tex):
    """The adjoint of the albedo blend (fr_synth_texture_backward): grad_alpha [B,K] = grad_tex [B,3,N] read as [B,3N] times
    pc_tex [3N,K], as float64 sums of exact products in an association that is a function of (N, K) alone, rounded once to fp32;
    bit-reproducible.  Both inputs are constants.  Runs on the current stream with the per-stream scratch as its workspace."""
    h = _host()
    g_c = h.require_gpu_f32(grad_tex.detach(), "grad_tex")
    if g_c.dim() != 3 or g_c.shape[1] != 3:
        raise ValueError("synth_texture_backward expects grad_tex [B,3,N]")
    B, N = int(g_c.shape[0]), int(g_c.shape[2])
    dev = g_c.device
    K = 0 if pc_tex is None else int(pc_tex.shape[1])
    grad_alpha = torch.empty((B, K), dtype=torch.float32, device=dev)
    if K == 0:
        return grad_alpha
    pc_c = h.require_gpu_f32(pc_tex.detach(), "pc_tex")
    if tuple(pc_c.shape) != (3 * N, K) or pc_c.device != dev:
        raise ValueError("synth_texture_backward: pc_tex must be [%d,%d] on %s (got %s on %s)" % (3 * N, K, dev, tuple(pc_c.shape),
                                                                                                 pc_c.device))
    L = h.lib()
    nws = L.fr_synth_texture_backward_workspace_bytes(B, N, K)
    with torch.cuda.device(dev), _KINDS_POOL.hold("synth_texture_backward", dev, nws) as ent:
        rc = L.fr_synth_texture_backward(h.ptr(pc_c), h.ptr(g_c), B, N, K, h.ptr(grad_alpha), h.ptr(ent.buf), ent.nbytes,
                                         h.stream_ptr(dev))
    h.check(rc, "fr_synth_texture_backward")
    return grad_alpha


class _SynthTexture(torch.autograd.Function):
    """fr_synth_texture / fr_synth_texture_backward as one autograd node: (mu_tex, pc_tex, alpha) -> tex [B,3,N], the gradient going
    to alpha alone.  The node saves pc_tex (by reference) and nothing else: the blend is linear in alpha."""

    @staticmethod
    def forward(ctx, mu_tex, pc_tex, alpha):
        tex, pc_c = _synth_texture_call(mu_tex, pc_tex, alpha)
        ctx.has_pc = pc_c is not None
        ctx.alpha_shape = tuple(alpha.shape)
        if ctx.has_pc:
            ctx.save_for_backward(pc_c)
        ctx.set_materialize_grads(False)
        return tex

    @staticmethod
    def backward(ctx, grad_tex):
        if grad_tex is None or not ctx.needs_input_grad[2]:
            return None, None, None
        if not ctx.has_pc:   # K = 0: an empty gradient
            return None, None, torch.zeros(ctx.alpha_shape, dtype=torch.float32, device=grad_tex.device)
        return None, None, synth_texture_backward(ctx.saved_tensors[0], grad_tex)


def synth_texture(mu_tex, pc_tex, alpha, out=None):
    """The per-face albedo tex [B,3,N] = mu_tex + pc_tex . alpha_b (fr_synth_texture: the chain acc = acc + pc alpha in ascending
    k from mu_tex, bit-exact against numpy): mu_tex [3,N], pc_tex [3N,K], alpha [B,K].  What render_depth takes as a per-face
    texture.  K = 0 repeats mu_tex.  Where alpha requires grad the call is an autograd node (same forward bits) whose backward
    is the blend's adjoint, synth_texture_backward (fr_synth_texture_backward); the gradient goes to alpha alone, mu_tex and pc_tex
    are constants.  out: a tensor to write instead of a fresh one; ValueError with an alpha that requires grad (a caller's buffer
    cannot be the output of a node).  Runs on the current stream."""
    if isinstance(alpha, torch.Tensor) and alpha.requires_grad and torch.is_grad_enabled():
        if out is not None:
            raise ValueError("synth_texture: out= cannot be combined with an alpha that requires grad")
        return _SynthTexture.apply(mu_tex, pc_tex, alpha)
    return _synth_texture_call(mu_tex, pc_tex, alpha, out)[0]


# ---- the shading models (csrc/fr_shade.h) as this file sees them: the gray one and the colour one are the same calls over other sizes ----
# loss: the photometric op, "fr_" + loss its entry points' prefix; kind: the pool kind of its forward's state; shader: the shading op
# and "fr_" + shader its entry point; light: a face's lighting; channels: of the image, the target and the background; sums: float64
# sums per face, 2 + the lighting's size; planes: the shader's outputs (name, channels), in the entry point's order
_ShadeModel = collections.namedtuple("_ShadeModel", "loss kind shader light channels sums planes")
_GRAY = _ShadeModel("photo_loss", "photo_loss", "synth_shade", (4,), 1, 6, (("im_gray", 1), ("mask", 1)))
_RGB = _ShadeModel("photo_loss_rgb", "photo_loss_rgb", "synth_shade_rgb", (3, 9), 3, 29, (("im_rgb", 3), ("im_gray", 1), ("mask", 1)))


def _model_light(h, m, op, light, B, dev):
    l_c = h.require_gpu_f32(light.detach(), "light")
    if tuple(l_c.shape) != (B,) + m.light or l_c.device != dev:
        raise ValueError("%s: light must be %s on %s (got %s on %s)" % (op, list((B,) + m.light), dev, tuple(l_c.shape), l_c.device))
    return l_c


def _photo_plane(h, op, t, name, B, H, W, dev):
    t_c = h.require_gpu_f32(t.detach(), name)
    _check_plane(op, name, t_c, B, H, W, 1, dev, "normal", flat=True)
    return t_c


def _photo_forward(m, ctx, tex_img, normal, tri_ind, light, target, weight, gain, offset):
    """The forward of both photometric nodes, for the model m: it saves its inputs by reference and the forward's sums [B, m.sums]
    (the lighting gradient is linear in them); nothing plane-sized of its own.  The forward's state (m.sums float64 partials per
    tile) is dead once the forward has run: it is the pooled per-stream buffer of kind m.kind, held across the forward's two
    launches."""
    h = _host()
    L = h.lib()
    op = m.loss
    n_c = h.require_gpu_f32(normal.detach(), "normal")
    if n_c.dim() != 4 or n_c.shape[3] != 3:
        raise ValueError("%s expects normal [B,H,W,3]" % op)
    B, H, W = int(n_c.shape[0]), int(n_c.shape[1]), int(n_c.shape[2])
    dev = n_c.device
    t_c = h.require_gpu_f32(tex_img.detach(), "tex_img")
    tg_c = h.require_gpu_f32(target.detach(), "target")
    _check_plane(op, "tex_img", t_c, B, H, W, 3, dev, "normal")
    _check_plane(op, "target", tg_c, B, H, W, m.channels, dev, "normal", flat=m.channels == 1)
    l_c = _model_light(h, m, op, light, B, dev)
    ti_c = _photo_plane(h, op, tri_ind, "tri_ind", B, H, W, dev)
    w_c = _photo_plane(h, op, weight, "weight", B, H, W, dev) if weight is not None else None
    empty = B * H * W == 0
    sums = (torch.zeros if empty else torch.empty)((B, m.sums), dtype=torch.float64, device=dev)
    if not empty:
        nst = getattr(L, "fr_%s_state_bytes" % op)(B, H, W)
        with torch.cuda.device(dev), _KINDS_POOL.hold(m.kind, dev, nst) as ent:
            rc = getattr(L, "fr_%s_forward" % op)(h.ptr(t_c), h.ptr(n_c), h.ptr(ti_c), h.ptr(l_c), h.ptr(tg_c), h.ptr(w_c), B, H, W,
                                                  float(gain), float(offset), h.ptr(sums), h.ptr(ent.buf), ent.nbytes, h.stream_ptr(dev))
        h.check(rc, "fr_%s_forward" % op)
    ctx.save_for_backward(t_c, n_c, ti_c, l_c, tg_c, sums, *(() if w_c is None else (w_c,)))
    ctx.dims = (B, H, W)
    ctx.scale = (float(gain), float(offset))
    ctx.shapes = (tuple(tex_img.shape), tuple(normal.shape), tuple(light.shape))
    ctx.set_materialize_grads(False)
    sse, count = sums[:, 0].contiguous(), sums[:, 1].contiguous()
    ctx.mark_non_differentiable(count)
    return sse, count


def _photo_backward(m, ctx, g_sse):
    """The backward of both photometric nodes: it asks the kernel only for the outputs needs_input_grad names; target, weight and
    tri_ind are constants."""
    if g_sse is None:
        return (None,) * 8
    h = _host()
    t_c, n_c, ti_c, l_c, tg_c, sums = ctx.saved_tensors[:6]
    w_c = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
    B, H, W = ctx.dims
    dev = n_c.device
    want = ctx.needs_input_grad
    empty = B * H * W == 0
    make = torch.zeros if empty else torch.empty
    gt = make(ctx.shapes[0], dtype=torch.float32, device=dev) if want[0] else None
    gn = make(ctx.shapes[1], dtype=torch.float32, device=dev) if want[1] else None
    gl = make(ctx.shapes[2], dtype=torch.float32, device=dev) if want[3] else None
    if not empty and (want[0] or want[1] or want[3]):
        g = g_sse.detach().to(device=dev, dtype=torch.float64).contiguous()
        with torch.cuda.device(dev):
            rc = getattr(h.lib(), "fr_%s_backward" % m.loss)(h.ptr(g), h.ptr(sums), h.ptr(t_c), h.ptr(n_c), h.ptr(ti_c), h.ptr(l_c),
                                                             h.ptr(tg_c), h.ptr(w_c), B, H, W, ctx.scale[0], ctx.scale[1], h.ptr(gt),
                                                             h.ptr(gn), h.ptr(gl), h.stream_ptr(dev))
        h.check(rc, "fr_%s_backward" % m.loss)
    return gt, gn, None, gl, None, None, None, None


class _PhotoLoss(torch.autograd.Function):
    """fr_photo_loss_forward / _backward (include/fr_hotpath.h, "photometric loss") as one autograd node: (tex_img, normal, tri_ind,
    light [B,4], target, weight, gain, offset) -> (sse [B], count [B]) float64: _photo_forward / _photo_backward over the gray model
    (sums [B,6], pool kind "photo_loss")."""

    @staticmethod
    def forward(ctx, *args):
        return _photo_forward(_GRAY, ctx, *args)

    @staticmethod
    def backward(ctx, g_sse, g_count):
        return _photo_backward(_GRAY, ctx, g_sse)


class _PhotoLossRGB(torch.autograd.Function):
    """fr_photo_loss_rgb_forward / _backward (include/fr_hotpath.h, "colour shading") as one autograd node: (tex_img, normal,
    tri_ind, light [B,3,9], target [B,H,W,3], weight, gain, offset) -> (sse [B], count [B]) float64: _photo_forward /
    _photo_backward over the colour model (sums [B,29], pool kind "photo_loss_rgb")."""

    @staticmethod
    def forward(ctx, *args):
        return _photo_forward(_RGB, ctx, *args)

    @staticmethod
    def backward(ctx, g_sse, g_count):
        return _photo_backward(_RGB, ctx, g_sse)


def photo_loss(tex_img, normal, tri_ind, light, target, weight=None, gain=1.0, offset=0.0):
    """The photometric term of a render's planes against a picture (fr_photo_loss_forward / _backward): per face b,
    sse[b] = sum over the covered pixels (tri_ind >= 0) of weight (I^ - target)^2 with I^ the image synth_shade makes of the same
    planes, light, gain and offset -- the same bits -- and count[b] = the covered pixels.  tex_img, normal [B,H,W,3] (the op's raw
    planes), tri_ind, target, weight [B,H,W,1] or [B,H,W] (weight None = 1), light [B,4]; -> (sse, count), float64 [B], float64
    sums in an association that is a function of (H, W) alone (bit-reproducible; a face's numbers do not depend on its batch).
    One autograd node: the gradient of sse reaches tex_img, normal and light (one map pass, no reduction; count is not
    differentiable; tri_ind, target and weight are constants).  A mean squared error is sse.sum() / count.sum().clamp_min(1).
    Runs on the current stream."""
    return _PhotoLoss.apply(tex_img, normal, tri_ind, light, target, weight, gain, offset)


def synth_shade(tex_img, normal, tri_ind, light, background=None, gain=1.0, offset=0.0, out=None):
    """The gray image of a render's planes under a first-order lighting (fr_synth_shade, one lane per pixel): where tri_ind >= 0,
    im_gray = a max(l0 + l . n^, 0) gain + offset with a = the mean of clamp_min(tex_img, 1e-6) over the channels and n^ the
    normal map of FaceRecNet.compute_abedo_image (flipped to n_z >= 0, normalised); elsewhere the background pixel ([1,H,W,1]
    or [B,H,W,1]; 0 without one).  tex_img, normal [B,H,W,3] (the op's raw normal), tri_ind [B,H,W,1], light [B,4].
    -> (im_gray, mask) [B,H,W,1], mask = 1.0 where tri_ind >= 0 else 0.0.  fp32 in a stated order, bit-exact against numpy
    (include/fr_hotpath.h).  Nothing requires grad.  Runs on the current stream."""
    return _synth_shade_call(_GRAY, tex_img, normal, tri_ind, light, background, gain, offset, out)


def _synth_shade_call(m, tex_img, normal, tri_ind, light, background, gain, offset, out):
    """synth_shade / synth_shade_rgb for the model m: the checks, the output planes m.planes and the one launch"""
    h = _host()
    op = m.shader
    t_c = h.require_gpu_f32(tex_img.detach(), "tex_img")
    n_c = h.require_gpu_f32(normal.detach(), "normal")
    ti_c = h.require_gpu_f32(tri_ind.detach(), "tri_ind")
    if n_c.dim() != 4 or n_c.shape[3] != 3:
        raise ValueError("%s expects normal [B,H,W,3]" % op)
    B, H, W = int(n_c.shape[0]), int(n_c.shape[1]), int(n_c.shape[2])
    dev = n_c.device
    bg_c, bg_batch = None, 0
    if background is not None:
        bg_c = h.require_gpu_f32(background.detach(), "background")
        bg_batch = int(bg_c.shape[0]) if bg_c.dim() == 4 else -1
        if bg_batch not in (1, B) or tuple(bg_c.shape[1:]) != (H, W, m.channels) or bg_c.device != dev:
            raise ValueError("%s: background must be [1,%d,%d,%d] or [%d,%d,%d,%d] on %s (got %s on %s)"
                             % (op, H, W, m.channels, B, H, W, m.channels, dev, tuple(bg_c.shape), bg_c.device))
    _check_plane(op, "tex_img", t_c, B, H, W, 3, dev, "normal")
    _check_plane(op, "tri_ind", ti_c, B, H, W, 1, dev, "normal")
    l_c = _model_light(h, m, op, light, B, dev)
    if out is None:
        out = tuple(torch.empty((B, H, W, c), dtype=torch.float32, device=dev) for _name, c in m.planes)
    out = tuple(out)
    if len(out) != len(m.planes):
        raise ValueError("%s: out must be the %d tensors (%s)" % (op, len(m.planes), ", ".join(name for name, _c in m.planes)))
    for t, (name, c) in zip(out, m.planes):
        if h.require_gpu_f32(t, name) is not t or tuple(t.shape) != (B, H, W, c) or t.device != dev:
            raise ValueError("%s: out %s must be a contiguous float32 tensor [%d,%d,%d,%d] on %s" % (op, name, B, H, W, c, dev))
    with torch.cuda.device(dev):
        rc = getattr(h.lib(), "fr_" + op)(h.ptr(t_c), h.ptr(n_c), h.ptr(ti_c), h.ptr(l_c), h.ptr(bg_c), bg_batch, B, H, W, float(gain),
                                          float(offset), *[h.ptr(t) for t in out], h.stream_ptr(dev))
    h.check(rc, "fr_" + op)
    return out


# ---- colour shading (opt-in): per-channel albedo under a second-order lighting per channel ---------------------------------------------
# light[b][c][k]: the four first-order ranges above in every channel, then five second-order coefficients around 0
SYNTH_LIGHT_RANGES_RGB = tuple(SYNTH_LIGHT_RANGES[k] if k < 4 else (-0.15, 0.15) for _c in range(3) for k in range(9))


def synth_light_rgb(seed, first_face, batch, ranges=SYNTH_LIGHT_RANGES_RGB, device=None, out=None):
    """`batch` faces of colour lighting drawn on the device (fr_synth_light_rgb) -> light [B,3,9], channel-major, uniform in
    `ranges` (27 (lo, hi) pairs; a scalar s means (-s, s)).  The sampler and key of synth_params on a stream of its own (the
    counter's fourth word is 1): under one seed no draw of synth_params moves.  out: a tensor to write instead of a fresh one.
    Nothing requires grad.  Runs on the current stream."""
    h = _host()
    B = int(batch)
    if out is None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("synth_light_rgb draws on an MI355X only (no CPU fallback); got %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((B, 3, 9), dtype=torch.float32, device=dev)
    elif h.require_gpu_f32(out, "out") is not out or tuple(out.shape) != (B, 3, 9):
        raise ValueError("synth_light_rgb: out must be a contiguous float32 tensor [%d,3,9]" % B)
    dev = out.device
    rg = _synth_ranges(ranges, 27, "ranges")
    with torch.cuda.device(dev):
        rc = h.lib().fr_synth_light_rgb(int(seed) & (2 ** 64 - 1), int(first_face) & (2 ** 64 - 1), B, rg, h.ptr(out), h.stream_ptr(dev))
    h.check(rc, "fr_synth_light_rgb")
    return out


def synth_shade_rgb(tex_img, normal, tri_ind, light, background=None, gain=1.0, offset=0.0, out=None):
    """The colour image of a render's planes (fr_synth_shade_rgb, one lane per pixel): where tri_ind >= 0, per channel c,
    im_rgb_c = a_c max(s_c, 0) gain + offset with a_c = clamp_min(tex_img_c, 1e-6) -- no mean over the channels -- and
    s_c = sum over k of light[b][c][k] H_k(n^), H the nine second-order polynomials of include/fr_hotpath.h ("colour shading")
    in the normal map of synth_shade; elsewhere the background pixel ([1,H,W,3] or [B,H,W,3]; 0 without one).  im_gray is the
    gray of im_rgb, 0.3 R + 0.59 G + 0.11 B, background included: the plane the nets take.  tex_img, normal [B,H,W,3],
    tri_ind [B,H,W,1], light [B,3,9].  -> (im_rgb [B,H,W,3], im_gray [B,H,W,1], mask [B,H,W,1]); out: three tensors to write
    instead.  fp32 in a stated order, bit-exact against numpy.  Nothing requires grad.  Runs on the current stream."""
    return _synth_shade_call(_RGB, tex_img, normal, tri_ind, light, background, gain, offset, out)


def photo_loss_rgb(tex_img, normal, tri_ind, light, target, weight=None, gain=1.0, offset=0.0):
    """The photometric term in colour (fr_photo_loss_rgb_forward / _backward): per face b, sse[b] = sum over the covered pixels
    and the three channels of weight (I^_c - target_c)^2 with I^ the image synth_shade_rgb makes of the same planes, light, gain
    and offset -- the same bits -- and count[b] = the covered pixels.  tex_img, normal, target [B,H,W,3], tri_ind, weight
    [B,H,W,1] or [B,H,W] (weight None = 1), light [B,3,9]; -> (sse, count), float64 [B], in the association of photo_loss.  One
    autograd node: the gradient of sse reaches tex_img (per channel), normal and light; count is not differentiable; tri_ind,
    target and weight are constants.  A mean squared error is sse.sum() / (3 count.sum()).clamp_min(1).  Runs on the current
    stream."""
    return _PhotoLossRGB.apply(tex_img, normal, tri_ind, light, target, weight, gain, offset)


# ---- colour photometric solve (opt-in): per-face least squares for the lighting and for alpha (include/fr_hotpath.h) -----------------
def albedo_basis_rgb(tri, mu_tex, pc_tex):
    """basis [T,3,K+1] float64: the texture model seen through the rasteriser's lookup, per channel -- slot k < K the mean over a
    triangle's three vertices of pc_tex[c N + v, k], slot K the same mean of mu_tex (fr_albedo_basis_rgb_build, bit-exact against
    numpy).  tri [3,T] float ids, mu_tex [3,N] or [3N], pc_tex [3N,K], 1 <= K <= 15.  Built once per mesh
    (FaceRecNet.albedo_basis_rgb caches it).  Runs on the current stream."""
    h = _host()
    tri_c = h.require_gpu_f32(tri, "tri")
    mu_c = h.require_gpu_f32(mu_tex.detach().reshape(-1), "mu_tex")
    pc_c = h.require_gpu_f32(pc_tex.detach(), "pc_tex")
    _check_tri(tri_c)
    if pc_c.dim() != 2 or pc_c.shape[0] % 3 != 0 or mu_c.numel() != pc_c.shape[0]:
        raise ValueError("albedo_basis_rgb expects mu_tex [3N] and pc_tex [3N,K] (got %s, %s)" % (tuple(mu_tex.shape), tuple(pc_c.shape)))
    dev = tri_c.device
    if pc_c.device != dev or mu_c.device != dev:
        raise ValueError("albedo_basis_rgb: mu_tex is on %s, pc_tex on %s, tri on %s" % (mu_c.device, pc_c.device, dev))
    T, K, nver = int(tri_c.shape[1]), int(pc_c.shape[1]), int(pc_c.shape[0]) // 3
    L = h.lib()
    basis = torch.empty((T, 3, K + 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = L.fr_albedo_basis_rgb_build(h.ptr(tri_c), h.ptr(mu_c), h.ptr(pc_c), nver, T, K, h.ptr(basis),
                                         L.fr_albedo_basis_rgb_bytes(T, K), h.stream_ptr(dev))
    h.check(rc, "fr_albedo_basis_rgb_build")
    return basis


def _solve_basis(op, basis, dev):
    if not (isinstance(basis, torch.Tensor) and basis.dtype == torch.float64 and basis.dim() == 3 and basis.shape[1] == 3
            and basis.shape[2] >= 2):
        raise ValueError("%s: basis must be a float64 tensor [T,3,K+1] (albedo_basis_rgb)" % op)
    if basis.device != dev:
        raise ValueError("%s: basis is on %s, tri_ind on %s" % (op, basis.device, dev))
    return basis.detach().contiguous(), int(basis.shape[0]), int(basis.shape[2]) - 1


def albedo_image_rgb(basis, tri_ind, alpha):
    """The albedo plane of the texture model at the coefficients alpha, without blending a [B,3,N] texture or rasterising again
    (fr_albedo_image_rgb, one lane per pixel): tex_img[b,p,c] = m_c[t] + Phi_c[t] . alpha_b with t = tri_ind[b,p], a float64 chain
    rounded once; +0 where no triangle of the basis is hit.  basis [T,3,K+1] (albedo_basis_rgb), tri_ind [B,H,W,1] or [B,H,W],
    alpha [B,K]; -> tex_img [B,H,W,3] fp32, bit-exact against numpy.  Nothing requires grad.  Runs on the current stream."""
    h = _host()
    ti_c = h.require_gpu_f32(tri_ind.detach(), "tri_ind")
    if ti_c.dim() not in (3, 4) or (ti_c.dim() == 4 and ti_c.shape[3] != 1):
        raise ValueError("albedo_image_rgb expects tri_ind [B,H,W,1] or [B,H,W]")
    B, H, W = int(ti_c.shape[0]), int(ti_c.shape[1]), int(ti_c.shape[2])
    dev = ti_c.device
    b_c, T, K = _solve_basis("albedo_image_rgb", basis, dev)
    a_c = h.require_gpu_f32(alpha.detach(), "alpha")
    if tuple(a_c.shape) != (B, K) or a_c.device != dev:
        raise ValueError("albedo_image_rgb: alpha must be [%d,%d] on %s (got %s on %s)" % (B, K, dev, tuple(a_c.shape), a_c.device))
    tex_img = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = h.lib().fr_albedo_image_rgb(h.ptr(b_c), h.ptr(ti_c), h.ptr(a_c), B, T, H, W, K, h.ptr(tex_img), h.stream_ptr(dev))
    h.check(rc, "fr_albedo_image_rgb")
    return tex_img


def _solve_planes(h, op, normal, tri_ind, target, weight):
    n_c = h.require_gpu_f32(normal.detach(), "normal")
    if n_c.dim() != 4 or n_c.shape[3] != 3:
        raise ValueError("%s expects normal [B,H,W,3]" % op)
    B, H, W = int(n_c.shape[0]), int(n_c.shape[1]), int(n_c.shape[2])
    dev = n_c.device
    tg_c = h.require_gpu_f32(target.detach(), "target")
    _check_plane(op, "target", tg_c, B, H, W, 3, dev, "normal")
    ti_c = _photo_plane(h, op, tri_ind, "tri_ind", B, H, W, dev)
    w_c = _photo_plane(h, op, weight, "weight", B, H, W, dev) if weight is not None else None
    return n_c, ti_c, tg_c, w_c, B, H, W, dev


def photo_light_lse_rgb(tex_img, normal, tri_ind, target, weight=None, gate_light=None, gain=1.0, offset=0.0, ridge=0.0,
                        return_moments=False):
    """The per-face, per-channel least-squares lighting of the colour model with the texture held (fr_photo_light_lse_rgb_forward):
    light[b][c] minimises sum_p weight (target_c - offset - gain a_c sum_k light[b][c][k] H_k)^2 + lambda |light[b][c]|^2 over the
    pixels channel c counts -- covered (tri_ind >= 0), weight > 0 and, with gate_light [B,3,9], lit under it (s_c > 0: the clamp's
    active set) -- with a_c and H_k the bits of photo_loss_rgb, lambda = ridge x the mean diagonal of the Gram matrix.  tex_img,
    normal, target [B,H,W,3], tri_ind, weight [B,H,W,1] or [B,H,W].  -> (light [B,3,9] fp32, stats [B,3,4] float64 = {count, E0,
    E1, ok}[, moments [B,3,16,16]]); a (face, channel) that cannot be fitted gets gate_light's row (0 without one) and ok = 0.
    float64 MFMA moments in a fixed association, bit-reproducible.  Nothing requires grad.  Runs on the current stream with the
    per-stream scratch as its workspace."""
    h = _host()
    op = "photo_light_lse_rgb"
    n_c, ti_c, tg_c, w_c, B, H, W, dev = _solve_planes(h, op, normal, tri_ind, target, weight)
    t_c = h.require_gpu_f32(tex_img.detach(), "tex_img")
    _check_plane(op, "tex_img", t_c, B, H, W, 3, dev, "normal")
    g_c = _model_light(h, _RGB, op, gate_light, B, dev) if gate_light is not None else None
    L = h.lib()
    make = torch.zeros if B * H * W == 0 else torch.empty
    light = make((B, 3, 9), dtype=torch.float32, device=dev)
    moments = make((B, 3, 16, 16), dtype=torch.float64, device=dev)
    stats = make((B, 3, 4), dtype=torch.float64, device=dev)
    nws = L.fr_photo_solve_rgb_workspace_bytes(B, H, W)
    with torch.cuda.device(dev), _KINDS_POOL.hold("photo_solve_rgb", dev, nws) as ent:
        rc = L.fr_photo_light_lse_rgb_forward(h.ptr(t_c), h.ptr(n_c), h.ptr(ti_c), h.ptr(tg_c), h.ptr(w_c), h.ptr(g_c), B, H, W,
                                              float(gain), float(offset), float(ridge), h.ptr(light), h.ptr(moments), h.ptr(stats),
                                              h.ptr(ent.buf), ent.nbytes, h.stream_ptr(dev))
    h.check(rc, "fr_photo_light_lse_rgb_forward")
    return (light, stats, moments) if return_moments else (light, stats)


def albedo_lse_rgb(basis, tri_ind, normal, light, target, weight=None, gain=1.0, offset=0.0, ridge=0.0, return_moments=False):
    """The per-face least-squares albedo coefficients of the colour model with the lighting held (fr_albedo_lse_rgb_forward):
    alpha_b minimises sum_p sum_c weight (target_c - offset - gain max(s_c, 0) (m_c[t] + Phi_c[t] . alpha))^2 + lambda |alpha|^2
    over the pixels that hit a triangle of the basis (and have weight > 0), s_c the chain of photo_loss_rgb under light [B,3,9].
    The albedo's clamp at 1e-6 is not in this affine model.  -> (alpha [B,K] fp32, stats [B,4] float64 = {count, E0, E1, ok}[,
    moments [B,16,16]]); a face that cannot be fitted gets alpha = 0 and ok = 0.  Nothing requires grad.  Runs on the current stream
    with the per-stream scratch as its workspace."""
    h = _host()
    op = "albedo_lse_rgb"
    n_c, ti_c, tg_c, w_c, B, H, W, dev = _solve_planes(h, op, normal, tri_ind, target, weight)
    b_c, T, K = _solve_basis(op, basis, dev)
    l_c = _model_light(h, _RGB, op, light, B, dev)
    L = h.lib()
    make = torch.zeros if B * H * W == 0 else torch.empty
    alpha = make((B, K), dtype=torch.float32, device=dev)
    moments = make((B, 16, 16), dtype=torch.float64, device=dev)
    stats = make((B, 4), dtype=torch.float64, device=dev)
    nws = L.fr_photo_solve_rgb_workspace_bytes(B, H, W)
    with torch.cuda.device(dev), _KINDS_POOL.hold("photo_solve_rgb", dev, nws) as ent:
        rc = L.fr_albedo_lse_rgb_forward(h.ptr(b_c), h.ptr(ti_c), h.ptr(n_c), h.ptr(l_c), h.ptr(tg_c), h.ptr(w_c), B, T, H, W, K,
                                         float(gain), float(offset), float(ridge), h.ptr(alpha), h.ptr(moments), h.ptr(stats),
                                         h.ptr(ent.buf), ent.nbytes, h.stream_ptr(dev))
    h.check(rc, "fr_albedo_lse_rgb_forward")
    return (alpha, stats, moments) if return_moments else (alpha, stats)


def photo_solve_rgb(basis, tri_ind, normal, target, weight=None, alpha0=None, light0=None, iters=8, gate=True, ridge_light=0.0,
                    ridge_alpha=0.0, gain=1.0, offset=0.0):
    """Alternating least squares for a face's colour lighting and albedo coefficients against `target` [B,H,W,3], the geometry
    (tri_ind, normal) held: `iters` times albedo_image_rgb -> photo_light_lse_rgb -> albedo_lse_rgb.  Each half-step is the exact
    minimiser of the model's squared error in its own unknowns (ridge 0), so the error does not rise.  alpha0 [B,K] (default 0, the
    mean albedo) and light0 [B,3,9] (default none) start it; with gate=True the light step counts, per channel, only the pixels
    lit under the previous lighting -- from the second iteration on, or from the first with a light0.  A (face, channel) or face
    whose step fails (ok = 0) keeps its previous value.  -> (light [B,3,9], alpha [B,K], tex_img [B,H,W,3] at the returned alpha,
    info) with info["E"] float64 [iters,2,B] -- the residual after the light step (summed over the channels) and after the albedo
    step -- and info["ok"] bool [iters,2,B].  No host synchronisation: 5 launches per iteration and one for the last image.
    Nothing requires grad."""
    iters = int(iters)
    if iters < 1:
        raise ValueError("photo_solve_rgb: iters must be >= 1")
    B, dev = int(tri_ind.shape[0]), tri_ind.device
    K = int(basis.shape[2]) - 1
    alpha = torch.zeros((B, K), dtype=torch.float32, device=dev) if alpha0 is None else alpha0.detach().to(torch.float32)
    light = None if light0 is None else light0.detach().to(torch.float32)
    E = torch.empty((iters, 2, B), dtype=torch.float64, device=dev)
    ok = torch.empty((iters, 2, B), dtype=torch.bool, device=dev)
    for it in range(iters):
        tex_img = albedo_image_rgb(basis, tri_ind, alpha)
        new_light, st = photo_light_lse_rgb(tex_img, normal, tri_ind, target, weight, light if gate else None, gain, offset, ridge_light)
        good = st[:, :, 3] > 0
        light = new_light if light is None else torch.where(good[:, :, None], new_light, light)
        E[it, 0], ok[it, 0] = st[:, :, 2].sum(1), good.all(1)
        new_alpha, st = albedo_lse_rgb(basis, tri_ind, normal, light, target, weight, gain, offset, ridge_alpha)
        good = st[:, 3] > 0
        alpha = torch.where(good[:, None], new_alpha, alpha)
        E[it, 1], ok[it, 1] = st[:, 2], good
    return light, alpha, albedo_image_rgb(basis, tri_ind, alpha), {"E": E, "ok": ok}


class LandmarkBasis:
    """The compact image of K chosen vertices' basis rows (fr_landmark_basis_build; include/fr_hotpath.h, "landmarks"): `image`
    (uint8, on the device), K, n_shape, n_exp and `idx` (the ids as a tuple of ints).  Built once by landmark_basis().  An image of
    landmark_contour_basis() also says how its K ids are laid out: `n_fixed` fixed ids, then `C` lines of `M` candidates (K = n_fixed
    + C M); a plain image has n_fixed = K and no lines."""

    def __init__(self, image, K, n_shape, n_exp, idx, n_fixed=None, C=0, M=0):
        self.image, self.K, self.n_shape, self.n_exp, self.idx = image, int(K), int(n_shape), int(n_exp), tuple(idx)
        self.device = image.device
        self.n_fixed, self.C, self.M = int(K) if n_fixed is None else int(n_fixed), int(C), int(M)

    @property
    def nbytes(self):
        return int(self.image.numel())


def landmark_basis(mu, pc_shape, pc_exp, idx):
    """Gathers the mean and the basis rows of the vertices `idx` (ints in [0, N); duplicates are legal) out of mu [3N], pc_shape
    [3N,n_shape], pc_exp [3N,n_exp] (blocked rows) into a LandmarkBasis: one launch on the current stream, never repeated per step.
    ValueError for an id outside [0, N), K outside 1 .. 1024 or more than 256 coefficients."""
    h = _host()
    L = h.lib()
    mu_c = h.require_gpu_f32(mu.detach().reshape(-1), "mu")
    ps_c = h.require_gpu_f32(pc_shape.detach(), "pc_shape")
    pe_c = h.require_gpu_f32(pc_exp.detach(), "pc_exp")
    N = int(mu_c.numel() // 3)
    if mu_c.numel() != 3 * N or ps_c.dim() != 2 or pe_c.dim() != 2 or ps_c.shape[0] != 3 * N or pe_c.shape[0] != 3 * N:
        raise ValueError("landmark_basis: mu must be [3N], pc_shape [3N,n_shape], pc_exp [3N,n_exp]")
    ids = [int(i) for i in (idx.reshape(-1).tolist() if hasattr(idx, "reshape") else list(idx))]
    bad = [i for i in ids if not 0 <= i < N]
    if bad:
        raise ValueError("landmark_basis: vertex id %d is outside [0, %d)" % (bad[0], N))
    K, ns, ne = len(ids), int(ps_c.shape[1]), int(pe_c.shape[1])
    nbytes = L.fr_landmark_basis_bytes(K, ns, ne)
    if nbytes == 0:
        raise ValueError("landmark_basis: needs 1 <= K <= 1024 and n_shape + n_exp <= 256 (got K = %d, %d + %d)" % (K, ns, ne))
    dev = mu_c.device
    idx_t = torch.tensor(ids, dtype=torch.int32, device=dev)
    image = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.fr_landmark_basis_build(h.ptr(mu_c), h.ptr(ps_c), h.ptr(pe_c), h.ptr(idx_t), N, ns, ne, K, h.ptr(image), nbytes,
                                       h.stream_ptr(dev))
    h.check(rc, "fr_landmark_basis_build")
    return LandmarkBasis(image, K, ns, ne, ids)


class _Landmark(torch.autograd.Function):
    """fr_landmark_forward / _backward as one autograd node: (params, R, lbasis, target, weight, im_size, pose_grad) -> (points
    [B,3,K] fp32, sse [B] float64 -- zeros without a target).  One launch each way.  It saves its inputs by reference and nothing of
    its own: the backward recomputes the landmarks from params.  Gradient to params, and to R where R requires grad and pose_grad is
    set; target and weight are constants."""

    @staticmethod
    def forward(ctx, params, R, lbasis, target, weight, im_size, pose_grad):
        h = _host()
        p_c = h.require_gpu_f32(params.detach(), "params")
        K, nd = lbasis.K, 7 + lbasis.n_shape + lbasis.n_exp
        if p_c.dim() != 2 or p_c.shape[1] != nd:
            raise ValueError("landmarks: params must be [B,%d] (got %s)" % (nd, tuple(p_c.shape)))
        B, dev = int(p_c.shape[0]), p_c.device
        if lbasis.device != dev:
            raise ValueError("landmarks: the basis image is on %s, params on %s" % (lbasis.device, dev))
        R_c = None
        if R is not None:
            R_c = h.require_gpu_f32(R.detach(), "R")
            if tuple(R_c.shape) != (B, 3, 3) or R_c.device != dev:
                raise ValueError("landmarks: R must be [%d,3,3] on %s" % (B, dev))
        t_c = w_c = None
        wb = 0
        if target is not None:
            t_c = h.require_gpu_f32(target.detach(), "target")
            if tuple(t_c.shape) != (B, K, 2) or t_c.device != dev:
                raise ValueError("landmark_sse: target must be [%d,%d,2] on %s (got %s)" % (B, K, dev, tuple(t_c.shape)))
            if weight is not None:
                w_c = h.require_gpu_f32(weight.detach(), "weight")
                if tuple(w_c.shape) not in ((K,), (B, K)) or w_c.device != dev:
                    raise ValueError("landmark_sse: weight must be [%d] or [%d,%d] on %s" % (K, B, K, dev))
                wb = 1 if w_c.dim() == 2 else 0
        points = torch.empty((B, 3, K), dtype=torch.float32, device=dev)
        sse = (torch.empty if t_c is not None and B else torch.zeros)((B,), dtype=torch.float64, device=dev)
        if B:
            with torch.cuda.device(dev):
                rc = h.lib().fr_landmark_forward(h.ptr(p_c), h.ptr(lbasis.image), lbasis.nbytes, h.ptr(R_c), h.ptr(t_c), h.ptr(w_c), wb,
                                                 B, K, lbasis.n_shape, lbasis.n_exp, float(im_size), h.ptr(points), h.ptr(sse),
                                                 h.stream_ptr(dev))
            h.check(rc, "fr_landmark_forward")
        ctx.save_for_backward(p_c, *[t for t in (R_c, t_c, w_c) if t is not None])
        ctx.have = (R_c is not None, t_c is not None, w_c is not None)
        ctx.lbasis, ctx.wb, ctx.im_size, ctx.pose_grad = lbasis, wb, float(im_size), bool(pose_grad)
        ctx.set_materialize_grads(False)
        if t_c is None:
            ctx.mark_non_differentiable(sse)
        return points, sse

    @staticmethod
    def backward(ctx, g_points, g_sse):
        if (g_points is None and g_sse is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 7
        h = _host()
        saved = list(ctx.saved_tensors)
        p_c = saved.pop(0)
        R_c, t_c, w_c = [saved.pop(0) if have else None for have in ctx.have]
        lb = ctx.lbasis
        B, dev = int(p_c.shape[0]), p_c.device
        grad_params = (torch.empty if B else torch.zeros)(tuple(p_c.shape), dtype=torch.float32, device=dev)
        grad_R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev) if R_c is not None and ctx.pose_grad else None
        if B:
            gp = h.require_gpu_f32(g_points.detach(), "grad_points") if g_points is not None else None
            gs = g_sse.detach().to(device=dev, dtype=torch.float64).contiguous() if g_sse is not None and t_c is not None else None
            if gp is None and gs is None:
                return (None,) * 7
            with torch.cuda.device(dev):
                rc = h.lib().fr_landmark_backward(h.ptr(gp), h.ptr(gs), h.ptr(p_c), h.ptr(lb.image), lb.nbytes, h.ptr(R_c), h.ptr(t_c),
                                                  h.ptr(w_c), ctx.wb, B, lb.K, lb.n_shape, lb.n_exp, ctx.im_size, h.ptr(grad_params),
                                                  h.ptr(grad_R), int(ctx.pose_grad), h.stream_ptr(dev))
            h.check(rc, "fr_landmark_backward")
        return grad_params, (grad_R if ctx.needs_input_grad[1] else None), None, None, None, None, None


def _landmark_args(op, lbasis, target, weight):
    # (by its fields, not its class: this file is loaded under two module names -- the package's, and FaceRecNet's by path)
    if not all(hasattr(lbasis, k) for k in ("image", "K", "n_shape", "n_exp", "idx")):
        raise TypeError("%s: lbasis must be a LandmarkBasis (landmark_basis())" % op)
    for name, t in (("target", target), ("weight", weight)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError("%s: %s is a constant of the term and must not require grad" % (op, name))


def landmarks(params, lbasis, R=None, im_size=200, pose_grad=False):
    """The projected landmarks [B,3,K] (x, y, z in the picture's frame, as vertices_transform gives them) of params [B, 7 + n_shape
    + n_exp], decoded from the compact image alone (fr_landmark_forward): float64 arithmetic on the fp32 inputs, rounded to fp32
    once.  R: optional [B,3,3] rotation (else the rotation of the angles, evaluated in the kernel).  An autograd node: the gradient
    reaches params -- the angle columns only with pose_grad=True, the project's default being 0 there -- and, with pose_grad=True,
    R where it requires grad.  Runs on the current stream."""
    _landmark_args("landmarks", lbasis, None, None)
    return _Landmark.apply(params, R, lbasis, None, None, im_size, bool(pose_grad))[0]


def landmark_sse(params, lbasis, target, weight=None, R=None, im_size=200, pose_grad=False):
    """The landmark term: per face b, sse[b] = sum_k w_k ((x_k - tx_k)^2 + (y_k - ty_k)^2) with (x, y) the projections of
    landmarks() BEFORE their rounding to fp32 -> float64 [B].  target [B,K,2] (x, y in pixels), weight None (= 1), [K] or [B,K]; a
    landmark of weight 0 is skipped entirely, so a missing landmark may carry any target, NaN included.  One launch each way: the
    backward recomputes the landmarks.  Gradient to params (angles with pose_grad=True) and, with pose_grad=True, to R; a target or
    weight that requires grad is refused.  Runs on the current stream."""
    _landmark_args("landmark_sse", lbasis, target, weight)
    if target is None:
        raise ValueError("landmark_sse: target is required")
    return _Landmark.apply(params, R, lbasis, target, weight, im_size, bool(pose_grad))[1]


LANDMARK_CONTOUR_RULES = {"nearest": 0, "extreme": 1}


def landmark_contour_basis(mu, pc_shape, pc_exp, fixed_idx, lines):
    """landmark_basis() over the ids `fixed_idx` (Kf of them, may be empty) followed by the lines `lines` [C,M] (ints, rectangular;
    pad a short line by repeating its last id: a repeat can never beat its original): candidate (c, m) is landmark Kf + c M + m.
    -> a LandmarkBasis that also carries n_fixed, C and M, for landmark_contour_select / _sse and landmark_fit(line_target=).
    ValueError for lines that are not [C,M] with C, M >= 1, more than 256 lines, an id outside [0, N) or K = Kf + C M over 1024."""
    fixed = [] if fixed_idx is None else [int(i) for i in (fixed_idx.reshape(-1).tolist() if hasattr(fixed_idx, "reshape")
                                                            else list(fixed_idx))]
    rows = lines.tolist() if hasattr(lines, "tolist") else [list(r) if hasattr(r, "__iter__") else r for r in lines]
    if not rows or any(not isinstance(r, list) or not r or len(r) != len(rows[0]) or any(isinstance(i, list) for i in r) for r in rows):
        raise ValueError("landmark_contour_basis: lines must be [C,M] vertex ids with C >= 1 and M >= 1, every line of the same length")
    C, M = len(rows), len(rows[0])
    if C > 256 or len(fixed) + C * M > 1024:
        raise ValueError("landmark_contour_basis: needs C <= 256 and Kf + C M <= 1024 (got %d + %d x %d)" % (len(fixed), C, M))
    ids = fixed + [int(i) for r in rows for i in r]
    N = int(mu.numel() // 3)
    bad = [i for i in ids if not 0 <= i < N]
    if bad:
        raise ValueError("landmark_contour_basis: vertex id %d is outside [0, %d)" % (bad[0], N))
    lb = landmark_basis(mu, pc_shape, pc_exp, ids)
    return LandmarkBasis(lb.image, lb.K, lb.n_shape, lb.n_exp, lb.idx, n_fixed=len(fixed), C=C, M=M)


def _landmark_contour_args(op, params, cbasis, line_target, line_weight, fixed_target, fixed_weight, rule, line_dir, R):
    """the checked, contiguous arguments of one select call -> (p_c, R_c, ft_c, fw_c, fwb, lt_c, lw_c, lwb, ld_c, rule number)"""
    h = _host()
    _landmark_args(op, cbasis, None, None)
    if not all(hasattr(cbasis, k) for k in ("n_fixed", "C", "M")) or cbasis.C < 1:
        raise ValueError("%s: the basis carries no lines (landmark_contour_basis())" % op)
    if rule not in LANDMARK_CONTOUR_RULES:
        raise ValueError("%s: rule is one of %s (got %r)" % (op, " ".join(LANDMARK_CONTOUR_RULES), rule))
    for name, t in (("line_target", line_target), ("line_weight", line_weight), ("fixed_target", fixed_target),
                    ("fixed_weight", fixed_weight), ("line_dir", line_dir)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError("%s: %s is a constant of the term and must not require grad" % (op, name))
    p_c = h.require_gpu_f32(params.detach(), "params")
    Kf, C, nd = cbasis.n_fixed, cbasis.C, 7 + cbasis.n_shape + cbasis.n_exp
    if p_c.dim() != 2 or p_c.shape[1] != nd:
        raise ValueError("%s: params must be [B,%d] (got %s)" % (op, nd, tuple(p_c.shape)))
    B, dev = int(p_c.shape[0]), p_c.device
    if cbasis.device != dev:
        raise ValueError("%s: the basis image is on %s, params on %s" % (op, cbasis.device, dev))

    def take(t, name, shapes):
        if t is None:
            return None
        t = h.require_gpu_f32(t.detach(), name)
        if tuple(t.shape) not in shapes or t.device != dev:
            raise ValueError("%s: %s must be %s on %s (got %s)" % (op, name, " or ".join(str(list(s)) for s in shapes), dev,
                                                                     tuple(t.shape)))
        return t
    R_c = take(R, "R", ((B, 3, 3),))
    lt_c = take(line_target, "line_target", ((B, C, 2),))
    lw_c = take(line_weight, "line_weight", ((C,), (B, C)))
    ft_c = take(fixed_target, "fixed_target", ((B, Kf, 2),))
    fw_c = take(fixed_weight, "fixed_weight", ((Kf,), (B, Kf)))
    ld_c = take(line_dir, "line_dir", ((C, 2),))
    if rule == "nearest" and lt_c is None:
        raise ValueError("%s: the nearest rule needs line_target [%d,%d,2]" % (op, B, C))
    if rule == "extreme" and ld_c is None:
        raise ValueError("%s: the extreme rule needs line_dir [%d,2]" % (op, C))
    return (p_c, R_c, ft_c, fw_c, 1 if fw_c is not None and fw_c.dim() == 2 else 0, lt_c, lw_c,
            1 if lw_c is not None and lw_c.dim() == 2 else 0, ld_c, LANDMARK_CONTOUR_RULES[rule])


def _landmark_contour_call(args, cbasis, im_size):
    """-> (sel, line_points, target or None, weight): target only where the call can fill it (line_target, and fixed_target if
    the basis has fixed ids)"""
    h = _host()
    p_c, R_c, ft_c, fw_c, fwb, lt_c, lw_c, lwb, ld_c, rule = args
    B, dev = int(p_c.shape[0]), p_c.device
    Kf, C, M, K = cbasis.n_fixed, cbasis.C, cbasis.M, cbasis.K
    make = torch.empty if B else torch.zeros
    sel = make((B, C), dtype=torch.int32, device=dev)
    line_points = make((B, C, 2), dtype=torch.float32, device=dev)
    target = make((B, K, 2), dtype=torch.float32, device=dev) if lt_c is not None and (Kf == 0 or ft_c is not None) else None
    weight = make((B, K), dtype=torch.float32, device=dev)
    if B:
        with torch.cuda.device(dev):
            rc = h.lib().fr_landmark_contour_select(h.ptr(p_c), h.ptr(cbasis.image), cbasis.nbytes, h.ptr(R_c), h.ptr(ft_c), h.ptr(fw_c),
                                                    fwb, h.ptr(lt_c), h.ptr(lw_c), lwb, h.ptr(ld_c), rule, B, Kf, C, M, cbasis.n_shape,
                                                    cbasis.n_exp, float(im_size), h.ptr(sel), h.ptr(line_points), h.ptr(target),
                                                    h.ptr(weight), h.stream_ptr(dev))
        h.check(rc, "fr_landmark_contour_select")
    return sel, line_points, target, weight


def landmark_contour_select(params, cbasis, line_target=None, line_weight=None, fixed_target=None, fixed_weight=None, rule="nearest",
                            line_dir=None, R=None, im_size=200):
    """Picks one candidate per line and face (fr_landmark_contour_select; include/fr_hotpath.h, "contour landmarks") at params
    [B, 7 + Kt] over a landmark_contour_basis(): rule "nearest" -- the candidate whose projection lies nearest line_target [B,C,2]
    -- or "extreme" -- the one furthest along line_dir [C,2], the model's own occluding contour along the line.  Ties go to the
    lowest m; a line of weight 0 is not looked at and a line without a winner (a NaN face) has sel = -1.
    -> (sel [B,C] int32, line_points [B,C,2] fp32 the winners' (x, y), target [B,K,2] or None, weight [B,K]): target and weight are
    what landmark_sse / landmark_solve_step take over the K = Kf + C M landmarks -- fixed_target [B,Kf,2] and fixed_weight (None,
    [Kf] or [B,Kf]) copied, every candidate of a line carrying the line's target, line_weight (None = 1, [C] or [B,C]) on the winner
    and +0 on the losers.  target is None where it cannot be filled (no line_target, or fixed ids without fixed_target).  Outside
    autograd: the selection is a constant.  ValueError for shapes that do not fit, an input that requires grad or an unknown rule.
    Runs on the current stream."""
    args = _landmark_contour_args("landmark_contour_select", params, cbasis, line_target, line_weight, fixed_target, fixed_weight,
                                  rule, line_dir, R)
    with torch.no_grad():
        return _landmark_contour_call(args, cbasis, im_size)


def landmark_contour_sse(params, cbasis, line_target, line_weight=None, fixed_target=None, fixed_weight=None, rule="nearest",
                         line_dir=None, R=None, im_size=200, pose_grad=False):
    """The landmark term with sliding contour correspondences: landmark_contour_select at params, then landmark_sse over its target
    and weight -> sse [B] float64.  Gradients as in landmark_sse; the selection is a constant, as tri_ind is elsewhere.  line_target
    is required, and fixed_target where the basis has fixed ids."""
    op = "landmark_contour_sse"
    args = _landmark_contour_args(op, params, cbasis, line_target, line_weight, fixed_target, fixed_weight, rule, line_dir, R)
    if line_target is None or (cbasis.n_fixed > 0 and fixed_target is None):
        raise ValueError("%s: line_target is required, and fixed_target for a basis with fixed ids" % op)
    with torch.no_grad():
        _, _, target, weight = _landmark_contour_call(args, cbasis, im_size)
    return _Landmark.apply(params, R, cbasis, target, weight, im_size, bool(pose_grad))[1]


LANDMARK_POSE_BITS = {"phi": 0, "gamma": 1, "theta": 2, "tx": 3, "ty": 4, "f": 6}   # (tz, bit 5, has no column: its Jacobian is zero)


def _landmark_pose_mask(op, fit_pose):
    if fit_pose is True:
        return 0x5F
    if fit_pose is False or fit_pose is None:
        return 0
    if isinstance(fit_pose, str):
        fit_pose = (fit_pose,)
    mask = 0
    for name in fit_pose:
        if name not in LANDMARK_POSE_BITS:
            raise ValueError("%s: fit_pose names come out of %s (got %r)" % (op, " ".join(LANDMARK_POSE_BITS), name))
        mask |= 1 << LANDMARK_POSE_BITS[name]
    return mask


def _landmark_solve_args(op, params, lbasis, target, weight, ridge, center, damp, fit_pose, fit_coef):
    """the checked, contiguous arguments of one solver call -> (p_c, t_c, w_c, wb, r_c, c_c, d_c, mask, coef)"""
    h = _host()
    _landmark_args(op, lbasis, target, weight)
    if target is None:
        raise ValueError("%s: target is required" % op)
    p_c = h.require_gpu_f32(params.detach(), "params")
    K, Kt = lbasis.K, lbasis.n_shape + lbasis.n_exp
    if p_c.dim() != 2 or p_c.shape[1] != 7 + Kt:
        raise ValueError("%s: params must be [B,%d] (got %s)" % (op, 7 + Kt, tuple(p_c.shape)))
    B, dev = int(p_c.shape[0]), p_c.device
    if lbasis.device != dev:
        raise ValueError("%s: the basis image is on %s, params on %s" % (op, lbasis.device, dev))
    t_c = h.require_gpu_f32(target.detach(), "target")
    if tuple(t_c.shape) != (B, K, 2) or t_c.device != dev:
        raise ValueError("%s: target must be [%d,%d,2] on %s (got %s)" % (op, B, K, dev, tuple(t_c.shape)))
    w_c, wb = None, 0
    if weight is not None:
        w_c = h.require_gpu_f32(weight.detach(), "weight")
        if tuple(w_c.shape) not in ((K,), (B, K)) or w_c.device != dev:
            raise ValueError("%s: weight must be [%d] or [%d,%d] on %s" % (op, K, B, K, dev))
        wb = 1 if w_c.dim() == 2 else 0
    return (p_c, t_c, w_c, wb) + _landmark_solve_extras(op, Kt, B, dev, ridge, center, damp, fit_pose, fit_coef)


def _landmark_solve_extras(op, Kt, B, dev, ridge, center, damp, fit_pose, fit_coef):
    """the solver's arguments beside the term's own, checked -> (r_c, c_c, d_c, mask, coef)"""
    h = _host()
    vec = []
    for name, t in (("ridge", ridge), ("center", center)):
        if t is not None:
            t = h.require_gpu_f32(t.detach(), name)
            if tuple(t.shape) != (Kt,) or t.device != dev:
                raise ValueError("%s: %s must be [%d] on %s (got %s)" % (op, name, Kt, dev, tuple(t.shape)))
        vec.append(t)
    d_c = None
    if damp is not None:
        if not isinstance(damp, torch.Tensor) or damp.dtype != torch.float64 or tuple(damp.shape) != (B,) or damp.device != dev:
            raise ValueError("%s: damp must be a float64 tensor [%d] on %s" % (op, B, dev))
        d_c = damp.detach().contiguous()
    mask = _landmark_pose_mask(op, fit_pose)
    coef = bool(fit_coef) and Kt > 0
    if mask == 0 and not coef:
        raise ValueError("%s: nothing to fit (fit_pose is empty and fit_coef is off or the model has no coefficients)" % op)
    return vec[0], vec[1], d_c, mask, coef


def _landmark_solve_call(args, lbasis, im_size):
    h = _host()
    L = h.lib()
    p_c, t_c, w_c, wb, r_c, c_c, d_c, mask, coef = args
    B, dev = int(p_c.shape[0]), p_c.device
    make = torch.empty if B else torch.zeros
    delta = make(tuple(p_c.shape), dtype=torch.float64, device=dev)
    cost = make((B, 2), dtype=torch.float64, device=dev)
    ok = make((B,), dtype=torch.int32, device=dev)
    if B:
        nws = L.fr_landmark_solve_workspace_bytes(B, lbasis.n_shape, lbasis.n_exp) if coef else 0
        # (the workspace is dead once the one launch is enqueued: one per stream, under the pool's hold)
        with torch.cuda.device(dev), _KINDS_POOL.hold("landmark_solve", dev, nws) as ent:
            rc = L.fr_landmark_solve_step(h.ptr(p_c), h.ptr(lbasis.image), lbasis.nbytes, h.ptr(t_c), h.ptr(w_c), wb, h.ptr(r_c),
                                          h.ptr(c_c), h.ptr(d_c), mask, int(coef), B, lbasis.K, lbasis.n_shape, lbasis.n_exp,
                                          float(im_size), h.ptr(delta), h.ptr(cost), h.ptr(ok), h.ptr(ent.buf), ent.nbytes,
                                          h.stream_ptr(dev))
        h.check(rc, "fr_landmark_solve_step")
    return delta, cost, ok


def landmark_solve_step(params, lbasis, target, weight=None, ridge=None, center=None, damp=None, fit_pose=True, fit_coef=False,
                        im_size=200):
    """One damped Gauss-Newton step of the landmark term per face (fr_landmark_solve_step; include/fr_hotpath.h, "landmark
    solver"): with r the residuals of landmark_sse, J their Jacobian in the fitted columns, H = J^T W J + diag(ridge), g = J^T W r +
    ridge (a - center) and D = diag(J^T W J), it solves (H + damp_b D) delta = -g by Cholesky, in float64, in one launch.
    -> (delta [B, 7 + Kt] float64, +0 in the columns that are not fitted; cost [B,2] float64 = (F at params, the quadratic model's
    prediction at params + delta) with F = sse + [fit_coef] sum ridge (a - center)^2; ok [B] int32).  A face whose system is not
    positive definite or not finite (f = 0 with an angle fitted, no landmark of weight > 0, a non-finite input) reports ok = 0, a
    zero step and cost[b,1] = cost[b,0], and changes no other face.
    target [B,K,2], weight None / [K] / [B,K] as in landmark_sse; ridge, center None or fp32 [Kt] (the coefficients' prior);
    damp None or float64 [B]; fit_pose True (the six columns phi gamma theta tx ty f -- tz has no column), False, or an iterable
    of those names; fit_coef: fit the Kt coefficients as well.  ValueError for a shape, device or name that does not fit, and when
    nothing is fitted.  Runs outside autograd, on the current stream; the workspace of a fit_coef call comes from the stream's pool."""
    args = _landmark_solve_args("landmark_solve_step", params, lbasis, target, weight, ridge, center, damp, fit_pose, fit_coef)
    with torch.no_grad():
        return _landmark_solve_call(args, lbasis, im_size)


def landmark_fit(params, lbasis, target, weight=None, ridge=None, center=None, iters=10, damp0=1e-3, fit_pose=True, fit_coef=False,
                 im_size=200, line_target=None, line_weight=None, rule="nearest", line_dir=None):
    """Levenberg-Marquardt on the landmark term from `params`: `iters` times landmark_solve_step, the candidate
    fl32(params.double() + delta), its F from landmark_sse plus the prior in float64, and per face: where ok and F_new < F_old the
    candidate is taken and damp divided by 3 (floor 1e-9), else the face stays and damp is multiplied by 4 (cap 1e9).  Everything
    stays on the device (torch.where; no host synchronisation).  -> (params_fitted [B, 7 + Kt] fp32, info) with info["cost"]
    [iters + 1, B] float64 (F before the first step, then after each iteration: non-increasing), info["accepted"] [iters, B] bool
    and info["damp"] [B] float64 (the damping the next step would use).  Arguments as landmark_solve_step; damp0 > 0 is the
    initial damping of every face.  Runs outside autograd, on the current stream.
    line_target [B,C,2] (default None: the code path and every bit are today's) over a landmark_contour_basis(): contour landmarks
    that slide.  `target` and `weight` then belong to the basis's fixed ids ([B,Kf,2]; None, [Kf] or [B,Kf]; target may be None
    when there are none), line_weight is None, [C] or [B,C], rule and line_dir as in landmark_contour_select.  At the top of every
    iteration the candidates are re-selected at the current parameters; F before and after the step is taken under that one
    selection, then the step is accepted or rejected as above.  info["cost"][0] is F under the first selection and info gains "sel"
    [iters + 1, B, C] int32: the selection of every iteration, then the one at the fitted parameters.  Under the nearest rule a
    re-selection can only lower a term, so the cost stays non-increasing.  Still no host synchronisation."""
    iters = int(iters)
    if iters < 0 or not float(damp0) >= 0.0:
        raise ValueError("landmark_fit: iters and damp0 must not be negative")
    if line_target is not None or line_weight is not None or line_dir is not None or rule != "nearest":
        return _landmark_fit_contour(params, lbasis, target, weight, ridge, center, iters, damp0, fit_pose, fit_coef, im_size,
                                     line_target, line_weight, rule, line_dir)
    args = _landmark_solve_args("landmark_fit", params, lbasis, target, weight, ridge, center, None, fit_pose, fit_coef)
    p_c, t_c, w_c, wb, r_c, c_c, _, mask, coef = args
    B, dev = int(p_c.shape[0]), p_c.device
    with torch.no_grad():
        r64 = r_c.double() if coef and r_c is not None else None
        c64 = c_c.double() if r64 is not None and c_c is not None else None

        def F_of(p):
            F = landmark_sse(p, lbasis, t_c, w_c, im_size=im_size)
            if r64 is not None:
                d = p[:, 7:].double() if c64 is None else p[:, 7:].double() - c64
                F = F + (r64 * d * d).sum(dim=1)
            return F
        cur = p_c.clone()
        damp = torch.full((B,), float(damp0), dtype=torch.float64, device=dev)
        three = torch.full((B,), 3.0, dtype=torch.float64, device=dev)   # (a tensor: torch divides by a Python scalar through its reciprocal)
        F = F_of(cur)
        costs, accepted = [F], []
        for _ in range(iters):
            delta, _, ok = _landmark_solve_call((cur, t_c, w_c, wb, r_c, c_c, damp, mask, coef), lbasis, im_size)
            cand = (cur.double() + delta).float()
            F_new = F_of(cand)
            acc = (ok != 0) & (F_new < F)
            cur = torch.where(acc[:, None], cand, cur)
            F = torch.where(acc, F_new, F)
            damp = torch.where(acc, (damp / three).clamp_min(1e-9), (damp * 4.0).clamp_max(1e9))
            costs.append(F)
            accepted.append(acc)
        info = {"cost": torch.stack(costs), "damp": damp,
                "accepted": torch.stack(accepted) if accepted else torch.zeros((0, B), dtype=torch.bool, device=dev)}
    return cur, info


def _landmark_fit_contour(params, cbasis, target, weight, ridge, center, iters, damp0, fit_pose, fit_coef, im_size, line_target,
                          line_weight, rule, line_dir):
    """landmark_fit with sliding contour landmarks: the same loop, with one selection per iteration"""
    op = "landmark_fit"
    sargs = _landmark_contour_args(op, params, cbasis, line_target, line_weight, target, weight, rule, line_dir, None)
    if line_target is None or (cbasis.n_fixed > 0 and target is None):
        raise ValueError("%s: line_target is required, and target [B,Kf,2] for a basis with fixed ids" % op)
    p_c = sargs[0]
    B, dev = int(p_c.shape[0]), p_c.device
    r_c, c_c, _, mask, coef = _landmark_solve_extras(op, cbasis.n_shape + cbasis.n_exp, B, dev, ridge, center, None, fit_pose, fit_coef)
    with torch.no_grad():
        r64 = r_c.double() if coef and r_c is not None else None
        c64 = c_c.double() if r64 is not None and c_c is not None else None

        def F_of(p, t, w):
            F = landmark_sse(p, cbasis, t, w, im_size=im_size)
            if r64 is not None:
                d = p[:, 7:].double() if c64 is None else p[:, 7:].double() - c64
                F = F + (r64 * d * d).sum(dim=1)
            return F
        cur = p_c.clone()
        damp = torch.full((B,), float(damp0), dtype=torch.float64, device=dev)
        three = torch.full((B,), 3.0, dtype=torch.float64, device=dev)
        costs, accepted, sels = [], [], []
        for _ in range(iters):
            sel, _, t_k, w_k = _landmark_contour_call((cur,) + sargs[1:], cbasis, im_size)
            F = F_of(cur, t_k, w_k)
            if not costs:
                costs.append(F)
            delta, _, ok = _landmark_solve_call((cur, t_k, w_k, 1, r_c, c_c, damp, mask, coef), cbasis, im_size)
            cand = (cur.double() + delta).float()
            F_new = F_of(cand, t_k, w_k)
            acc = (ok != 0) & (F_new < F)
            cur = torch.where(acc[:, None], cand, cur)
            damp = torch.where(acc, (damp / three).clamp_min(1e-9), (damp * 4.0).clamp_max(1e9))
            costs.append(torch.where(acc, F_new, F))
            accepted.append(acc)
            sels.append(sel)
        sel, _, t_k, w_k = _landmark_contour_call((cur,) + sargs[1:], cbasis, im_size)
        sels.append(sel)
        if not costs:
            costs.append(F_of(cur, t_k, w_k))
        info = {"cost": torch.stack(costs), "damp": damp, "sel": torch.stack(sels),
                "accepted": torch.stack(accepted) if accepted else torch.zeros((0, B), dtype=torch.bool, device=dev)}
    return cur, info


def rendering_layer_fused(ver, tri, texture, im_gray, normal_grad=False):
    """One-pass rendering layer: returns (net_input [B,H,W,7] = [mask*im | pncc | normal],
    depth_img, raw depth, tri_ind).  Raises NotImplementedError for shapes only the fallback rasteriser covers.
    normal_grad=False (default): as the reference, the normal channels carry no gradient and the vertex gradient is z-only.
    normal_grad=True: the gradient of channels 4-6 reaches all three coordinates of the winning triangles' vertices
    (fr_render_normal_backward, post mode, behind the depth backward); same outputs, bit for bit.  The node then keeps the
    vertex tensor: [B,3,nver] fp32, 41 MB at 64 faces of the full mesh."""
    return _RenderingLayerFused.apply(ver, tri, texture, im_gray, bool(normal_grad))


def render_depth(ver, tri, texture, image, normal_grad=False, texture_grad=False, depth_interp=False, **kwargs):
    """Forward function of RenderDepth (reference ops.py:78-81).

    The first output is the rendered depth, the fourth the triangle index each depth pixel corresponds to.
    `image` only donates the batch / height / width (its values are never read, render_depth_op.cc:397-403).
    `**kwargs` is accepted for call compatibility (TF passed `name=`); unknown keys are ignored.
    normal_grad=False (default): as the reference, only `depth` has a backward (vertex z; the x and y rows are zeros).
    normal_grad=True: the third output, `normal`, has one too -- its gradient reaches all three coordinates of the winning
    triangles' vertices (fr_render_normal_backward, raw mode, behind the depth backward; tri_ind held fixed).  Same outputs, bit
    for bit.  The node then keeps the vertex tensor: [B,3,nver] fp32, 41 MB at 64 faces of the full mesh.
    texture_grad=False (default): as the reference, `texture` gets no gradient.  texture_grad=True: a gradient arriving at the
    second output, `tex_img`, reaches `texture` in the input's own shape ([3,N], [1,3,N] or [B,3,N]) -- the adjoint of the
    lookup (t[p1] + t[p2] + t[p3]) / 3 (fr_render_texture_backward; tri_ind held fixed).  Same outputs, bit for bit; the node
    saves no tensor beyond what it keeps anyway, and no backward is launched for an output nobody used.  Combines with normal_grad.
    depth_interp=False (default): `depth` is the reference's flat value, (z1 + z2 + z3) / 3 at every pixel a triangle wins.
    depth_interp=True: the first output is depth_interpolate(ver, tri, tri_ind) of this render -- the winner's plane at the pixel;
    the other three outputs are the default call's, bit for bit (the winner is still chosen on the flat value, so a pixel's z may
    exceed a neighbour's winner by less than its triangle's z range).  A gradient of `depth` then fills x, y and z
    (fr_depth_interp_backward; the flat backward is not launched) and the node keeps the vertex tensor, as with normal_grad.
    Combines with normal_grad (the normal backward follows with accumulate) and texture_grad.
    """
    return _RenderDepth.apply(ver, tri, texture, image, bool(normal_grad), bool(texture_grad), bool(depth_interp))


def render_depth_grad(depth_grad, ver, tri, depth, tri_ind, image):
    """The RenderDepthGrad op called directly with the reference's argument order
    (depth_grad, vertex, tri, depth, tri_ind, image; render_depth_op.cc:473-478) -> vertex_grad [B,3,nver]."""
    h = _host()
    g = h.require_gpu_f32(depth_grad, "depth_grad")
    tri_c = h.require_gpu_f32(tri, "tri")
    ti = h.require_gpu_f32(tri_ind, "tri_ind")
    _check_ver(ver)
    if ver.shape[0] != image.shape[0]:
        raise ValueError("The vertex's batch is not the same as image batch")
    _check_tri(tri_c)
    B, H, W = int(image.shape[0]), int(image.shape[1]), int(image.shape[2])
    nver, ntri = int(ver.shape[2]), int(tri_c.shape[1])
    dev = g.device
    vertex_grad = torch.empty((B, 3, nver), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _backward_call(h, g, tri_c, ti, vertex_grad, B, nver, ntri, H, W, dev)
    return vertex_grad
