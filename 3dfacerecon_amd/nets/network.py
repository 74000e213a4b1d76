"""Hot-path half of the reference's nets/network.py `FaceRecNet`, on PyTorch-ROCm + the gfx950 C ABI.

Only the 3DMM decoder and the rendering-layer wrapper are here -- the methods on the CoarseNet -> render loop
that BASELINE.json's north_star names:

    vertices_transform(pred_params)            reference nets/network.py:140-171   (HIP: fr_decode_3dmm)
    rendering_layer(vertex_proj, tri, colors)  reference nets/network.py:174-201   (HIP: fr_render_depth_forward)
    set_constraints / parse_pose_params / rotation_matrix / rotation_matrix_batch  (:204-218, :253-297)

CoarseNet / FineNet / losses / summaries / checkpoints (network.py:103-136, 311-603) are out of scope.
The 235-d layout is unchanged: [phi, gamma, theta, tx, ty, tz, f | shape x199 | exp x29].
"""
import importlib.util
import os
import sys
import threading
from math import cos, sin

import numpy as np
import torch

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, relpath):
    mod = sys.modules.get(name)
    if mod is None:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_PKG_DIR, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod


def _host():
    return _load("_fr_hotpath_host", "_lib.py")


def _ops():
    return _load("_fr_hotpath_ops", os.path.join("rendering_layer", "ops.py"))


def _publish(device):
    """A lazily built constant image is packed on whichever stream first needs it (possibly autograd's backward stream) and
    then cached with no event: wait for the pack kernel ONCE, here, so that a later consumer on any other stream finds the
    image complete.  (Not under graph capture, where a synchronize is illegal: the capture's own stream order covers it.)"""
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).synchronize()


class PackedBasis:
    """The constant basis (a tf.constant of the reference model, network.py:41-43) in the layouts the decode kernels
    stream: the f32 MFMA-fragment image, built at once (fr_decode_pack_basis), and -- only if the opt-in Q30 arithmetic
    is ever selected (_lib.set_decode_arith / FR_DECODE_ARITH=q30) -- its digit image, built on first use.  A default user
    holds 153 MB per basis and never launches a q_* kernel."""

    def __init__(self, mu, pc_shape, pc_exp, nvert, ndim_shape, ndim_exp, device):
        h = _host()
        L = h.lib()
        self.mu, self.pc_shape, self.pc_exp = mu, pc_shape, pc_exp
        self.nvert, self.ndim_shape, self.ndim_exp, self.device = nvert, ndim_shape, ndim_exp, device
        nbytes = L.fr_decode_packed_basis_bytes(nvert, ndim_shape, ndim_exp)
        self.image = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            rc = L.fr_decode_pack_basis(h.ptr(mu), h.ptr(pc_shape), h.ptr(pc_exp), nvert, ndim_shape, ndim_exp,
                                        h.ptr(self.image), nbytes, h.stream_ptr(device))
        h.check(rc, "fr_decode_pack_basis")
        _publish(device)
        self._qimage = None
        self._image_t = None   # K-major image for the backward's reduction over the vertices, built at the first backward
        self._t_owner = None   # another PackedBasis of the SAME pc_shape / pc_exp whose image_t this one shares (the K-major
                               # image does not contain mu, so a mu = 0 twin needs no second 153 MB copy)
        self.q30_ws_bytes = L.fr_decode_q30_workspace_bytes(ndim_shape, ndim_exp)
        self._packed_ok = None
        self.backward_from_mu = False   # True: the autograd node's backward does not keep the forward's output (see _Decode3DMM)
        self._bwd_ws = _host().StreamBuffers(4, 16)   # decode-backward workspaces, the byte count as the kind: backward_workspace()

    def image_t(self):
        """The basis packed for the decode backward (fr_decode_backward_pack_basis), built on first use: callers that never
        take a gradient never hold it."""
        if self._t_owner is not None:
            return self._t_owner.image_t()
        if self._image_t is None:
            h = _host()
            L = h.lib()
            nbytes = L.fr_decode_backward_basis_bytes(self.nvert, self.ndim_shape, self.ndim_exp)
            if nbytes == 0:   # not served by the packed kernel (more than 256 coefficients, or fewer than 16 vertices): reference-layout entry point
                return None
            buf = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                rc = L.fr_decode_backward_pack_basis(h.ptr(self.pc_shape), h.ptr(self.pc_exp), self.nvert, self.ndim_shape,
                                                     self.ndim_exp, h.ptr(buf), nbytes, h.stream_ptr(self.device))
            h.check(rc, "fr_decode_backward_pack_basis")
            _publish(self.device)
            self._image_t = buf
        return self._image_t

    def backward_packed_ok(self):
        """True when the fused backward (packed image, d f from mu) serves this basis / mesh."""
        if self._t_owner is not None:
            return self._t_owner.backward_packed_ok()
        if self._packed_ok is None:
            self._packed_ok = _host().lib().fr_decode_backward_basis_bytes(self.nvert, self.ndim_shape, self.ndim_exp) > 0
        return self._packed_ok

    def backward_workspace(self, B, dev):
        """`with basis.backward_workspace(B, dev) as (bytes, buffer):` -- a hold (_lib.StreamBuffers) on the decode backward's
        workspace for B faces on torch's current stream of `dev`, in this basis's own pool of four: kept per (stream, size), so
        alternating batch sizes keep a buffer each.  The size query and the allocation used to be paid per call: with the
        kernels at ~70 us the autograd route was host-bound below 64 faces (profiles/round4_bwd_probe.log)."""
        nws = _host().lib().fr_decode_backward_workspace_bytes(B, self.nvert, self.ndim_shape, self.ndim_exp)
        return self._bwd_ws.hold(nws, dev, nws, sized=True)

    def use_q30(self):
        """True when the Q30 entry point serves this call: selected AND the shape is covered (else the f32 chain)."""
        h = _host()
        return h.decode_arith() == h.DECODE_ARITH_Q30 and self.q30_ws_bytes > 0

    def qimage(self):
        if self._qimage is None:
            h = _host()
            L = h.lib()
            nbytes = L.fr_decode_q30_image_bytes(self.nvert, self.ndim_shape, self.ndim_exp)
            buf = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                rc = L.fr_decode_q30_pack(h.ptr(self.mu), h.ptr(self.pc_shape), h.ptr(self.pc_exp), self.nvert,
                                          self.ndim_shape, self.ndim_exp, h.ptr(buf), nbytes, h.stream_ptr(self.device))
            h.check(rc, "fr_decode_q30_pack")
            _publish(self.device)
            self._qimage = buf
        return self._qimage

    def decode(self, params, R, B, im_size, out, workspace=None):
        """One decode launch on torch's current stream.  `workspace` (Q30 only): a caller-owned staging buffer of
        q30_ws_bytes; by default one is taken from torch's caching allocator for this call (stream-safe)."""
        h = _host()
        L = h.lib()
        dev = params.device
        with torch.cuda.device(dev):
            if self.use_q30():
                ws = workspace if workspace is not None else torch.empty((self.q30_ws_bytes,), dtype=torch.uint8, device=dev)
                rc = L.fr_decode_3dmm_q30_lv(h.ptr(params), h.ptr(self.qimage()), h.ptr(R), B, self.nvert, self.ndim_shape,
                                             self.ndim_exp, float(im_size), h.q30_levels(), h.ptr(out), h.ptr(ws),
                                             self.q30_ws_bytes, h.stream_ptr(dev))
                h.check(rc, "fr_decode_3dmm_q30_lv")
            else:
                rc = L.fr_decode_3dmm(h.ptr(params), h.ptr(self.image), h.ptr(R), B, self.nvert, self.ndim_shape,
                                      self.ndim_exp, float(im_size), h.ptr(out), h.stream_ptr(dev))
                h.check(rc, "fr_decode_3dmm")


class _Decode3DMM(torch.autograd.Function):
    """vertices_transform as one autograd node: fr_decode_3dmm forward, fr_decode_3dmm_backward for the gradient TF
    autodiff derives from network.py:140-171 (d alpha, d beta, d t3d, d f; the three angles get zero because the
    reference's rotation goes through tf.py_func, network.py:150, which has no gradient).  That is the default and stays so;
    pose_grad=True adds what the reference drops (fr_decode_pose_backward, enqueued behind the decode backward): the angle
    columns of the gradient when the rotation is evaluated in-kernel, dL/dR for a caller-computed R (the angle columns then
    stay 0: the angles did not enter the forward).  It needs the forward's output, so it keeps it (no mu form)."""

    @staticmethod
    def forward(ctx, params, net, R, basis=None, im_size=None, pose_grad=False):
        B = int(params.shape[0])
        out = torch.empty((B, 3, net.nvert), dtype=torch.float32, device=params.device)
        basis = net._basis if basis is None else basis
        im_size = float(net.im_size if im_size is None else im_size)
        basis.decode(params, R, B, im_size, out)
        ctx.net = net
        ctx.basis = basis
        ctx.im_size = im_size
        # The fused backward has two forms of d f.  Default: from the forward's output (fr_decode_3dmm_backward_packed; `out` stays
        # alive for the backward -- 41 MB per 64-face decode).  `basis.backward_from_mu = True` selects the form that needs no
        # forward output (fr_decode_3dmm_backward_packed_mu: d f from mu and the coefficient gradients) -- a MEMORY saving, not a
        # faster kernel (same time at 64 faces, 3 us more at 32: profiles/round5_probes/r5d).  Bases / meshes the fused kernel
        # does not serve take the reference-layout entry point, which needs `out`.
        ctx.packed = basis.backward_packed_ok()
        ctx.pose_grad = bool(pose_grad)
        ctx.from_mu = ctx.packed and bool(getattr(basis, "backward_from_mu", False)) and not ctx.pose_grad
        if ctx.from_mu:
            ctx.save_for_backward(params, R if R is not None else params.new_empty(0))
        else:
            ctx.save_for_backward(params, R if R is not None else params.new_empty(0), out)
        ctx.has_R = R is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h = _host()
        net = ctx.net
        basis = ctx.basis
        params, R = ctx.saved_tensors[0], ctx.saved_tensors[1]
        B = int(params.shape[0])
        g = h.require_gpu_f32(grad_out, "grad_vertex_proj")
        gp = torch.empty_like(params)
        L = h.lib()
        dev = params.device
        with torch.cuda.device(dev):
            Rp = h.ptr(R) if ctx.has_R else None
            # (the fused kernels stream the packed image: built once per basis, at the first backward -- before the hold)
            image_t = basis.image_t() if ctx.packed else None
            with basis.backward_workspace(B, dev) as (nws, ws):
                if ctx.from_mu:
                    rc = L.fr_decode_3dmm_backward_packed_mu(h.ptr(g), h.ptr(params), h.ptr(basis.mu), h.ptr(image_t), Rp, B,
                                                             net.nvert, net.ndim_shape, net.ndim_exp, ctx.im_size, h.ptr(gp),
                                                             h.ptr(ws), nws, h.stream_ptr(dev))
                elif ctx.packed:
                    rc = L.fr_decode_3dmm_backward_packed(h.ptr(g), h.ptr(params), h.ptr(ctx.saved_tensors[2]), h.ptr(image_t),
                                                          Rp, B, net.nvert, net.ndim_shape, net.ndim_exp, ctx.im_size, h.ptr(gp),
                                                          h.ptr(ws), nws, h.stream_ptr(dev))
                else:   # more than 256 coefficients or fewer than 16 vertices (not the model's): reference-layout entry point
                    out = ctx.saved_tensors[2]
                    rc = L.fr_decode_3dmm_backward(h.ptr(g), h.ptr(params), h.ptr(out), h.ptr(basis.pc_shape),
                                                   h.ptr(basis.pc_exp), Rp, B, net.nvert, net.ndim_shape, net.ndim_exp,
                                                   ctx.im_size, h.ptr(gp), h.ptr(ws), nws, h.stream_ptr(dev))
            h.check(rc, "fr_decode_3dmm_backward")
            gR = None
            if ctx.pose_grad:
                # completes gp: the angle columns (R evaluated in-kernel) or dL/dR (only when somebody asked for R's gradient)
                if ctx.has_R and ctx.needs_input_grad[2]:
                    gR = torch.empty_like(R)
                if gR is not None or not ctx.has_R:
                    pws_bytes = L.fr_decode_pose_backward_workspace_bytes(B, net.nvert)
                    pws = h.byte_buffer(pws_bytes, dev)
                    rc = L.fr_decode_pose_backward(h.ptr(g), h.ptr(ctx.saved_tensors[2]), h.ptr(params), Rp, B, net.nvert,
                                                   net.ndim_shape, net.ndim_exp, ctx.im_size, h.ptr(gp), h.ptr(gR), h.ptr(pws),
                                                   pws_bytes, h.stream_ptr(dev))
                    h.check(rc, "fr_decode_pose_backward")
        return gp, None, gR, None, None, None


class _GeometryGramLoss(torch.autograd.Function):
    """The geometry loss in its Gram form as one autograd node: diff [B,K] fp32 -> mean(([pc_shape | pc_exp] diff^T)^2), a 0-dim
    fp32 tensor, from G = U^T U (FaceRecNet.gram()) -- fr_geometry_loss_forward, fr_geometry_loss_backward; no pass of the basis,
    no [B,3,N] tensor.  The forward leaves y = G d in its state buffer and the backward scales it, so a buffer belongs to ONE call
    from its forward to its backward: the node takes it from FaceRecNet.gram_state() and hands it back when its backward has
    been enqueued (the same stream: launches are ordered).  A second backward through one node (retain_graph) finds the buffer
    gone and raises.  The kernels take 18 us at 64 faces, so the node is host-bound: it makes one stream query per direction and
    passes addresses as plain integers (the binding's argtypes convert them)."""

    @staticmethod
    def forward(ctx, diff, net, gram):
        L = _host().lib()
        dev = diff.device
        B = int(diff.shape[0])
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            key, nst, state = net.gram_state(B, dev, stream)
            rc = L.fr_geometry_loss_forward(diff.data_ptr(), gram.data_ptr(), B, net.nvert, net.ndim_shape, net.ndim_exp,
                                            loss.data_ptr(), state.data_ptr(), nst, stream)
        if rc:
            _host().check(rc, "fr_geometry_loss_forward")
        ctx.net, ctx.key, ctx.nst, ctx.state, ctx.shape = net, key, nst, state, (B, int(diff.shape[1]))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        h = _host()
        if ctx.state is None:
            raise RuntimeError("geometry_loss(gram=True): the node's state went back to the pool with its first backward; "
                               "call the loss again for a second backward")
        net = ctx.net
        g = h.require_gpu_f32(grad_loss, "grad_loss")
        B, K = ctx.shape
        dev = g.device
        gd = torch.empty((B, K), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = h.lib().fr_geometry_loss_backward(g.data_ptr(), ctx.state.data_ptr(), ctx.nst, B, net.nvert, net.ndim_shape,
                                                   net.ndim_exp, gd.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            h.check(rc, "fr_geometry_loss_backward")
        net.gram_state_done(ctx.key, ctx.state)
        ctx.state = None
        return gd, None, None


class FaceRecNet:
    def __init__(self, im_gray=None, params_label=None, mesh_data=None, nIter=4, batch_size=64, im_size=200,
                 weight_decay=1e-4, device="cuda"):
        self.im_gray = im_gray
        self.params_label = params_label
        self.nIter = nIter
        self.batch_size = batch_size
        self.im_size = im_size
        self.weight_decay = weight_decay
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FaceRecNet hot path needs an MI355X device (got %s); there is no CPU fallback"
                               % self.device)

        # mesh data (same dict keys as utils/parser_3dmm.py:50-60)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.vertex_code = torch.as_tensor(np.asarray(mesh_data['vertex'], np.float32), **f32)    # (3, N)
        self.tri = torch.as_tensor(np.asarray(mesh_data['tri'], np.float32), **f32)               # (3, T) float ids
        self.mu = torch.as_tensor(np.asarray(mesh_data['mu'], np.float32).reshape(-1), **f32)      # (3*N,)
        self.pc_shape = torch.as_tensor(np.asarray(mesh_data['pc_shape'], np.float32), **f32)     # (3*N, ndim_shape)
        self.pc_exp = torch.as_tensor(np.asarray(mesh_data['pc_exp'], np.float32), **f32)         # (3*N, ndim_exp)

        # albedo model of the shape-from-shading loss (network.py:26, 45-47): mean texture (3,N), the first ndim_tex
        # texture components (3N, ndim_tex) and their coefficients (ndim_tex, 1); optional in the asset dict
        self.ndim_tex = 10
        self.mu_tex = self.pc_tex = self.param_tex = None
        if mesh_data.get('mu_tex') is not None:
            self.mu_tex = torch.as_tensor(np.asarray(mesh_data['mu_tex'], np.float32), **f32)
        if mesh_data.get('pc_tex') is not None and mesh_data.get('param_tex') is not None:
            self.pc_tex = torch.as_tensor(np.asarray(mesh_data['pc_tex'], np.float32)[:, 0:self.ndim_tex], **f32)
            self.param_tex = torch.as_tensor(np.asarray(mesh_data['param_tex'], np.float32)[0:self.ndim_tex, :], **f32)

        # mesh info
        self.ndim_shape = int(mesh_data['ndim_shape'])
        self.ndim_exp = int(mesh_data['ndim_exp'])
        self.ndim_pose = int(mesh_data['ndim_pose'])
        self.ndim = self.ndim_pose + self.ndim_shape + self.ndim_exp
        self.nvert = int(self.mu.numel() // 3)
        if self.ndim_pose != 7:
            raise ValueError("ndim_pose must be 7")
        if tuple(self.pc_shape.shape) != (3 * self.nvert, self.ndim_shape) or \
                tuple(self.pc_exp.shape) != (3 * self.nvert, self.ndim_exp):
            raise ValueError("pc_shape / pc_exp must be (3*Nvert, ndim)")

        # one-time re-layout of the constant basis into MFMA-fragment order (include/fr_hotpath.h)
        self._basis = PackedBasis(self.mu, self.pc_shape, self.pc_exp, self.nvert, self.ndim_shape, self.ndim_exp,
                                  self.device)
        self._basis_nomu = None  # second image with mu = 0, built on first use by geometry_product()
        self._gram = None        # U^T U in float64 (fr_geometry_gram_build), built on first use by gram()
        self._gram_state = {}    # free state buffers of the Gram-form loss by (device, stream, bytes): gram_state()
        self._gram_nst = {}      # fr_geometry_loss_state_bytes by batch
        self._gram_lock = threading.Lock()
        self._albedo_basis = None   # the texture basis per triangle in float64 (fr_albedo_basis_build), built on first use
        self._albedo_basis_rgb = None   # the texture model per triangle and channel (fr_albedo_basis_rgb_build), built on first use
        self._adjacency = None      # the vertex -> triangle CSR table on the device (utils/mesh_io.vertex_adjacency), on first use
        self._landmark_bases = {}   # compact basis images of chosen vertices by id tuple (fr_landmark_basis_build): landmark_basis()

        # initial parameters (network.py:57-62)
        geo = torch.zeros((batch_size, self.ndim_shape + self.ndim_exp), **f32)
        init_pose = torch.tensor([0, 0, 0, im_size / 2.0, im_size / 2.0, 0, 0.001], **f32)
        self.pred_params = torch.cat([init_pose[None].repeat(batch_size, 1), geo], 1)[:, None, None, :]  # (B,1,1,d)
        self.init_pred_params = self.pred_params.clone()  # eager callers restart every forward from this constant

    # ---- 3DMM decode ----------------------------------------------------------------------------------
    def vertices_transform(self, pred_params, R=None, pose_grad=False):
        """(B,1,1,d) or (B,d) parameters -> projected vertices (B,3,N)  (network.py:140-171).

        R: optional host-computed (B,3,3) rotation (what the reference gets from tf.py_func at :150); by default
        the rotation is evaluated inside the kernel in float64.
        pose_grad: False (default) -- the three angles get gradient 0 and R none, as in the reference.  True -- the backward
        also runs fr_decode_pose_backward: with R=None the angle columns of the gradient are filled; with R given its gradient
        dL/dR is returned (it flows on if R is a tensor that requires grad) and the angle columns stay 0.  The node then keeps
        the forward's output for the backward (`backward_from_mu` does not apply to such a call)."""
        h = _host()
        p = pred_params
        if p.dim() == 4:
            p = p.reshape(p.shape[0], p.shape[-1])
        if p.dim() != 2 or p.shape[1] != self.ndim:
            raise ValueError("pred_params must be (B,1,1,%d) or (B,%d)" % (self.ndim, self.ndim))
        p = h.require_gpu_f32(p, "pred_params")
        B = int(p.shape[0])
        Rc = None
        if R is not None:
            Rc = h.require_gpu_f32(torch.as_tensor(R, dtype=torch.float32, device=p.device), "R")
            if tuple(Rc.shape) != (B, 3, 3):
                raise ValueError("R must be (B,3,3)")
        if pose_grad:
            return _Decode3DMM.apply(p, self, Rc, None, None, True)
        return _Decode3DMM.apply(p, self, Rc)

    def geometry_product(self, geometry_params):
        """(B, ndim_shape + ndim_exp) coefficients -> basis product [pc_shape | pc_exp] . coeff as (B,3,N) (blocked rows),
        the `tf.matmul(geometry_basis, geometry, transpose_b=True)` of the geometry loss (network.py:347-353), on the
        MFMA decode kernel: a second packed image with mu = 0 is decoded with the identity pose (R = I, f = 1, t = 0,
        im_size = 1).  The y row comes out as (1 - y) - 1, i.e. -y to within half an ulp of max(1, |y|) -- the loss
        squares it.  Differentiable (fr_decode_3dmm_backward)."""
        h = _host()
        g = h.require_gpu_f32(geometry_params, "geometry_params")
        B = int(g.shape[0])
        if g.dim() != 2 or g.shape[1] != self.ndim_shape + self.ndim_exp:
            raise ValueError("geometry_params must be (B,%d)" % (self.ndim_shape + self.ndim_exp))
        if self._basis_nomu is None:
            self._basis_nomu = PackedBasis(torch.zeros_like(self.mu), self.pc_shape, self.pc_exp, self.nvert,
                                           self.ndim_shape, self.ndim_exp, self.device)
            self._basis_nomu._t_owner = self._basis   # same pc_shape / pc_exp: one K-major backward image for both
        pose = torch.zeros((B, self.ndim_pose), dtype=torch.float32, device=g.device)
        pose[:, 6] = 1.0
        eye = torch.eye(3, dtype=torch.float32, device=g.device)[None].repeat(B, 1, 1).contiguous()
        return _Decode3DMM.apply(torch.cat([pose, g], 1), self, eye, self._basis_nomu, 1.0)

    def gram(self):
        """G = U^T U of U = [pc_shape | pc_exp] as a [Kp,Kp] float64 tensor (Kp = ndim_shape + ndim_exp rounded up to 16), built
        on first use by fr_geometry_gram_build -- one pass over the basis in its reference layout, float64 MFMA -- and cached: a
        caller that never asks for the Gram-form loss never holds it.  None where the kernels do not serve the basis (more than
        256 coefficients)."""
        with self._gram_lock:
            if self._gram is None:
                h = _host()
                L = h.lib()
                nbytes = L.fr_geometry_gram_bytes(self.ndim_shape, self.ndim_exp)
                if nbytes == 0:
                    return None
                kp = (self.ndim_shape + self.ndim_exp + 15) // 16 * 16
                G = torch.empty((kp, kp), dtype=torch.float64, device=self.device)
                nws = L.fr_geometry_gram_workspace_bytes(self.nvert, self.ndim_shape, self.ndim_exp)
                ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=self.device)
                with torch.cuda.device(self.device):
                    rc = L.fr_geometry_gram_build(h.ptr(self.pc_shape), h.ptr(self.pc_exp), self.nvert, self.ndim_shape,
                                                  self.ndim_exp, h.ptr(G), nbytes, h.ptr(ws), nws, h.stream_ptr(self.device))
                h.check(rc, "fr_geometry_gram_build")
                _publish(self.device)
                self._gram = G
            return self._gram

    def albedo_basis(self):
        """Phi [T,ndim_tex] float64: pc_tex seen through the rasteriser's lookup, per triangle (rendering_layer/ops.py::
        albedo_basis), built on first use and cached under the lock gram() uses: a caller that never asks for the per-face albedo
        fit never holds it (8.5 MB at the full mesh).  ValueError without a texture model."""
        with self._gram_lock:
            if self._albedo_basis is None:
                if self.pc_tex is None:
                    raise ValueError("the asset dict has no texture model (mu_tex / pc_tex / param_tex)")
                with torch.cuda.device(self.device):
                    self._albedo_basis = _ops().albedo_basis(self.tri, self.pc_tex)
                _publish(self.device)
            return self._albedo_basis

    def albedo_basis_rgb(self):
        """basis [T,3,ndim_tex+1] float64: pc_tex and mu_tex seen through the rasteriser's lookup, per triangle and channel
        (rendering_layer/ops.py::albedo_basis_rgb), built on first use and cached under the lock albedo_basis() uses (28 MB at the
        full mesh with ten coefficients).  ValueError without a texture model."""
        with self._gram_lock:
            if self._albedo_basis_rgb is None:
                if self.pc_tex is None:
                    raise ValueError("the asset dict has no texture model (mu_tex / pc_tex / param_tex)")
                with torch.cuda.device(self.device):
                    self._albedo_basis_rgb = _ops().albedo_basis_rgb(self.tri, self.mu_tex, self.pc_tex)
                _publish(self.device)
            return self._albedo_basis_rgb

    def photo_solve_rgb(self, tri_ind, normal, target, weight=None, alpha0=None, light0=None, **kwargs):
        """The closed-form colour fit of this mesh's texture model against `target` [B,H,W,3] on a render's planes
        (rendering_layer/ops.py::photo_solve_rgb with albedo_basis_rgb()): -> (light [B,3,9], alpha [B,ndim_tex], tex_img, info)."""
        return _ops().photo_solve_rgb(self.albedo_basis_rgb(), tri_ind, normal, target, weight, alpha0, light0, **kwargs)

    def adjacency(self):
        """The vertex -> triangle CSR table of the mesh (utils/mesh_io.vertex_adjacency) as a rendering_layer/ops.py::MeshAdjacency
        on the device, built on the host on first use and cached under the lock gram() uses: a caller that never asks for vertex
        normals never holds it (1.5 MB at the full mesh)."""
        with self._gram_lock:
            if self._adjacency is None:
                mesh_io = _load("_fr_hotpath_mesh_io", os.path.join("utils", "mesh_io.py"))
                adj_start, adj_tri = mesh_io.vertex_adjacency(self.tri.cpu().numpy(), self.nvert)
                self._adjacency = _ops().MeshAdjacency(adj_start, adj_tri, self.nvert, int(self.tri.shape[1]), self.device)
            return self._adjacency

    def smooth_planes(self, ver, texture, tri_ind, normals=True, tex=True):
        """The smooth counterparts (tex_img, normal) [B,H,W,3] of a render's flat planes, over that render's tri_ind [B,H,W,1]
        (held fixed), in the layouts photo_loss, photo_loss_rgb, synth_shade* and the SfS route take:
        tex_img  rendering_layer/ops.py::attr_interpolate of `texture` ([B,3,N], or a shared [3,N] / [1,3,N]) at the pixel, where
                 the render has the mean of the triangle's three vertices;
        normal   attr_interpolate of vertex_normals(ver, grad=True) over the cached adjacency(), where the render has the winner's
                 facet normal.  It is not normalised (the consumers normalise, csrc/fr_shade.h) and (+0, +0, +0) off the face.
        Gradients reach `texture`, and `ver` [B,3,N] through x and y (both planes) and through the vertex normals (all three
        rows).  normals=False / tex=False: that plane is None and costs nothing."""
        ops = _ops()
        ver = ver.float()
        tri_ind = tri_ind.detach()
        tex_img = ops.attr_interpolate(ver, texture, self.tri, tri_ind) if tex else None
        normal = None
        if normals:
            normal = ops.attr_interpolate(ver, ops.vertex_normals(ver, self.tri, self.adjacency(), grad=True), self.tri, tri_ind)
        return tex_img, normal

    def landmark_basis(self, idx):
        """The compact image of the basis rows of the vertices `idx` (a sequence or tensor of ids in [0, N); duplicates are legal)
        as a rendering_layer/ops.py::LandmarkBasis, built on first use per id tuple and cached under the lock gram() uses: 187 KB
        twice over at 68 landmarks of the full model.  ValueError for an id outside [0, N)."""
        ids = tuple(int(i) for i in (idx.reshape(-1).tolist() if hasattr(idx, "reshape") else idx))
        with self._gram_lock:
            lb = self._landmark_bases.get(ids)
            if lb is None:
                bad = [i for i in ids if not 0 <= i < self.nvert]
                if bad:
                    raise ValueError("landmark id %d is outside [0, %d)" % (bad[0], self.nvert))
                with torch.cuda.device(self.device):
                    lb = _ops().landmark_basis(self.mu, self.pc_shape, self.pc_exp, ids)
                _publish(self.device)
                self._landmark_bases[ids] = lb
            return lb

    def landmark_contour_basis(self, fixed_idx, lines):
        """The compact image over the fixed ids `fixed_idx` (may be empty or None) followed by the candidate lines `lines` [C,M]
        (rendering_layer/ops.py::landmark_contour_basis: a LandmarkBasis that also carries n_fixed, C, M), built on first use per
        (ids, lines) and cached beside landmark_basis()'s.  ValueError as there."""
        fixed = () if fixed_idx is None else tuple(int(i) for i in (fixed_idx.reshape(-1).tolist() if hasattr(fixed_idx, "reshape")
                                                                    else fixed_idx))
        rows = lines.tolist() if hasattr(lines, "tolist") else [list(r) if hasattr(r, "__iter__") else r for r in lines]
        key = ("contour", fixed, tuple(tuple(r) if isinstance(r, list) else r for r in rows))
        with self._gram_lock:
            lb = self._landmark_bases.get(key)
            if lb is None:
                with torch.cuda.device(self.device):
                    lb = _ops().landmark_contour_basis(self.mu, self.pc_shape, self.pc_exp, list(fixed), rows)
                _publish(self.device)
                self._landmark_bases[key] = lb
            return lb

    def landmarks(self, pred_params, idx, R=None, pose_grad=False):
        """(B,1,1,d) or (B,d) parameters -> the projections [B,3,K] of the vertices `idx`: what vertices_transform(pred_params)
        [:, :, idx] holds, to the rounding of an fp32 chain, from the compact image of landmark_basis(idx) alone -- float64
        arithmetic rounded once, no pass over the dense basis and no [B,3,N] tensor (rendering_layer/ops.py::landmarks).  R and
        pose_grad as in vertices_transform."""
        p = pred_params
        if p.dim() == 4:
            p = p.reshape(p.shape[0], p.shape[-1])
        if p.dim() != 2 or p.shape[1] != self.ndim:
            raise ValueError("pred_params must be (B,1,1,%d) or (B,%d)" % (self.ndim, self.ndim))
        if R is not None and not isinstance(R, torch.Tensor):
            R = torch.as_tensor(R, dtype=torch.float32, device=p.device)
        return _ops().landmarks(p, self.landmark_basis(idx), R=R, im_size=self.im_size, pose_grad=pose_grad)

    def landmark_fit(self, pred_params, idx_or_lbasis, target, weight=None, ridge=None, center=None, iters=10, damp0=1e-3,
                     fit_pose=True, fit_coef=False, line_target=None, line_weight=None, rule="nearest", line_dir=None):
        """(B,1,1,d) or (B,d) parameters -> (the parameters [B,d] after `iters` Levenberg-Marquardt iterations on the landmark
        term, info): rendering_layer/ops.py::landmark_fit at this model's im_size, over the cached landmark_basis(idx) -- or over a
        LandmarkBasis handed in as it is.  target [B,K,2], weight, ridge, center, fit_pose and fit_coef as there.  line_target,
        line_weight, rule and line_dir (default: absent, today's path) go with a landmark_contour_basis(): contour landmarks that
        are re-selected at every iteration, as there."""
        p = pred_params
        if p.dim() == 4:
            p = p.reshape(p.shape[0], p.shape[-1])
        if p.dim() != 2 or p.shape[1] != self.ndim:
            raise ValueError("pred_params must be (B,1,1,%d) or (B,%d)" % (self.ndim, self.ndim))
        lb = idx_or_lbasis if hasattr(idx_or_lbasis, "image") else self.landmark_basis(idx_or_lbasis)
        return _ops().landmark_fit(p, lb, target, weight=weight, ridge=ridge, center=center, iters=iters, damp0=damp0,
                                   fit_pose=fit_pose, fit_coef=fit_coef, im_size=self.im_size, line_target=line_target,
                                   line_weight=line_weight, rule=rule, line_dir=line_dir)

    def fine_mesh(self, vertices_proj, pred_depth_map, coarse_depth_map, with_normals=True):
        """The fine depth map taken back to the mesh: {"vertices": [B,3,N] fp32, "state": uint8 [B,N], "normals": [B,3,N] fp32 or
        None}.  `vertices_proj` is rendered once for its tri_ind -- the same winners, bit for bit, that produced
        `coarse_depth_map` (rendering_layer / coarse_net_input of the same vertices) -- then rendering_layer/ops.py::mesh_visible,
        mesh_lift and (with_normals) vertex_normals of the lifted vertices over adjacency().  x and y do not move; a vertex with
        state 1 has z + the bilinear sample of pred_depth_map - coarse_depth_map at its position, the others (0: hidden, 2: visible
        without a pixel of the face around it) keep the coarse z.  Forward only: the inputs are read as constants and nothing
        returned requires grad."""
        ops = _ops()
        with torch.no_grad():
            ver = vertices_proj.detach().float()
            B = int(ver.shape[0])
            image = torch.zeros((B, self.im_size, self.im_size, 3), dtype=torch.float32, device=ver.device)
            tri_ind = ops.render_depth(ver=ver, tri=self.tri, texture=self.vertex_code, image=image)[3]
            visible = ops.mesh_visible(self.tri, tri_ind, self.nvert)
            vertices, state = ops.mesh_lift(ver, tri_ind, visible, pred_depth_map, coarse_depth_map, ntri=int(self.tri.shape[1]))
            normals = ops.vertex_normals(vertices, self.tri, self.adjacency()) if with_normals else None
        return {"vertices": vertices, "state": state, "normals": normals}

    def soft_mask(self, vertices_proj):
        """The soft silhouette [B,H,W,1] in [0, 1] of the face of vertices_proj [B,3,N]: one render for its tri_ind (the winners are
        held fixed), then rendering_layer/ops.py::soft_coverage -- 1 inside, +0 outside, the covered share on the pixels either
        side of the face / background border.  Its gradient reaches the x and y rows of vertices_proj, which is what tells a fit
        where the face is in the picture; through vertices_transform(pose_grad=True) it reaches t3d, f and the angles."""
        ops = _ops()
        ver = vertices_proj.float()
        B = int(ver.shape[0])
        with torch.no_grad():
            image = torch.zeros((B, self.im_size, self.im_size, 3), dtype=torch.float32, device=ver.device)
            tri_ind = ops.render_depth(ver=ver.detach(), tri=self.tri, texture=self.vertex_code, image=image)[3]
        return ops.soft_coverage(ver, self.tri, tri_ind)

    def gram_state(self, B, dev, stream):
        """(key, bytes, buffer): a state buffer of the Gram-form loss for B faces on `stream` (torch's current stream of `dev`, as
        its address), the caller's until it hands it back through gram_state_done(key, buffer).  Free buffers are kept per
        (stream, size) -- launches on one stream are ordered, so the next call may reuse what the last one's backward has read --
        at most four in all; a buffer that never comes back (a forward without a backward) is the allocator's again when its
        node dies.  Under graph capture a fresh one is taken and never pooled.  (Not a _lib.StreamBuffers hold: the buffer is one
        node's from its forward to its backward, not one call's -- a free list, where that pool shares entries under a lock.)"""
        nst = self._gram_nst.get(B)
        if nst is None:
            nst = self._gram_nst[B] = _host().lib().fr_geometry_loss_state_bytes(B, self.ndim_shape, self.ndim_exp)
        if torch.cuda.is_current_stream_capturing():
            return None, nst, torch.empty((nst,), dtype=torch.uint8, device=dev)
        key = (dev.index, stream, nst)
        with self._gram_lock:
            free = self._gram_state.get(key)
            buf = free.pop() if free else None
        if buf is None:
            buf = torch.empty((nst,), dtype=torch.uint8, device=dev)
        return key, nst, buf

    def gram_state_done(self, key, buf):
        if key is None:
            return
        with self._gram_lock:
            if sum(len(v) for v in self._gram_state.values()) < 4:
                self._gram_state.setdefault(key, []).append(buf)

    def geometry_loss(self, geometry_diff, gram=False):
        """(B, ndim_shape + ndim_exp) coefficient differences -> the geometry loss mean(([pc_shape | pc_exp] diff^T)^2), 0-dim.
        gram=False (default): the product route, `g = geometry_product(diff); (g * g).mean()` -- two passes over the basis per
        step, a [B,3,N] tensor kept for the backward.
        gram=True: the same quantity from G = U^T U (gram(), built at the first call), in float64 chains of a fixed order
        (include/fr_hotpath.h, "Gram-form geometry loss"): no basis traffic per step, and the second packed image of the basis is
        never built.  An empty batch, or a basis gram() does not serve, takes the product route."""
        G = None
        if gram and int(geometry_diff.shape[0]) > 0:
            G = self._gram if self._gram is not None else self.gram()
        if G is not None:
            d = _host().require_gpu_f32(geometry_diff, "geometry_diff")
            if d.dim() != 2 or d.shape[1] != self.ndim_shape + self.ndim_exp:
                raise ValueError("geometry_diff must be (B,%d)" % (self.ndim_shape + self.ndim_exp))
            return _GeometryGramLoss.apply(d, self, G)
        g = self.geometry_product(geometry_diff)
        return (g * g).mean()

    # ---- rendering layer wrapper --------------------------------------------------------------------------
    def rendering_layer(self, vertex_proj, triangles, colors, im_gray=None, normal_grad=False, depth_interp=False):
        """(network.py:174-201) -> pncc_batch, normalimg_batch, maskimg_batch, depthimg_batch.
        normal_grad=True: the op's `normal` output has a backward (rendering_layer/ops.py::render_depth), so normalimg_batch
        carries its gradient to x, y and z of the vertices; the default leaves it a constant to autograd, as the reference.
        depth_interp=True: depthimg_batch is clamp_min of the interpolated plane (rendering_layer/ops.py::depth_interpolate over
        this render's tri_ind: the winner's plane at the pixel, with an x, y, z backward); the coverage mask -- maskimg_batch --
        keeps coming from the flat plane, bit for bit, as do the other two outputs.  Default: the reference's flat depth."""
        im_gray = self.im_gray if im_gray is None else im_gray
        ver = vertex_proj.float()
        tri = torch.as_tensor(triangles, dtype=torch.float32, device=ver.device)
        tex = torch.as_tensor(colors, dtype=torch.float32, device=ver.device)  # (3,N) shared across the batch
        B = ver.shape[0]
        if im_gray is None:
            im_gray = torch.ones((B, self.im_size, self.im_size, 1), dtype=torch.float32, device=ver.device)
        image = im_gray.expand(-1, -1, -1, 3)
        kw = {"normal_grad": True} if normal_grad else {}
        depth, tex_img, normal, tri_ind = _ops().render_depth(ver=ver, tri=tri, texture=tex, image=image, **kw)
        # 1. pncc result
        pncc_batch = torch.clamp(tex_img, 1e-6, 1.0)
        # 2. normal map: flip normals with negative z, normalise by magnitude
        flip = normal[..., 2:3] < 0
        normal = torch.where(flip, -1.0 * normal, normal)
        mag = (normal * normal).sum(-1)
        mag = torch.where(mag > 1e-6, mag, torch.ones_like(mag))
        normalimg_batch = normal / (torch.sqrt(mag) + 1e-6)[..., None]
        # 3. masked image
        mask = torch.clamp(depth, 1e-6, 1.0)
        maskimg_batch = mask * im_gray
        # 4. depth image
        # (tri_ind is an output of the render node, hence part of the graph: the winners are held fixed)
        depthimg_batch = torch.clamp_min(_ops().depth_interpolate(ver, tri, tri_ind.detach()) if depth_interp else depth, 1e-6)
        return pncc_batch, normalimg_batch, maskimg_batch, depthimg_batch

    def coarse_net_input(self, vertex_proj, triangles=None, colors=None, im_gray=None, normal_grad=False, depth_interp=False):
        """The 7-channel CoarseNet input [maskimg | pncc | normal] (network.py:122) and the depth image, produced by
        the fused kernel pass (falls back to rendering_layer + concat for shapes it does not cover).
        normal_grad=True: channels 4-6 carry their gradient to x, y and z of the vertices (fr_render_normal_backward behind the
        depth backward; the render node keeps the vertex tensor, 41 MB at 64 faces of the full mesh).  Default: none, as the
        reference -- the vertex gradient is z-only.
        depth_interp=True: net_input is the default call's, bit for bit (the fused kernel's; its mask channel is the flat
        plane's); depth_img is clamp_min(depth_interpolate(ver, tri, tri_ind), 1e-6) of the same render's winners, and its
        gradient reaches x, y and z.  Default: the flat depth image."""
        im_gray = self.im_gray if im_gray is None else im_gray
        ver = vertex_proj.float()
        tri = self.tri if triangles is None else torch.as_tensor(triangles, dtype=torch.float32, device=ver.device)
        tex = self.vertex_code if colors is None else torch.as_tensor(colors, dtype=torch.float32, device=ver.device)
        if im_gray is None:
            im_gray = torch.ones((ver.shape[0], self.im_size, self.im_size, 1), dtype=torch.float32, device=ver.device)
        try:
            kw = {"normal_grad": True} if normal_grad else {}
            net_in, depth_img, _, tri_ind = _ops().rendering_layer_fused(ver, tri, tex, im_gray, **kw)
            if depth_interp:
                depth_img = torch.clamp_min(_ops().depth_interpolate(ver, tri, tri_ind), 1e-6)
        except NotImplementedError:
            if depth_interp:
                kw["depth_interp"] = True
            pncc, normal, mask, depth_img = self.rendering_layer(ver, tri, tex, im_gray=im_gray, **kw)
            net_in = torch.cat([mask, pncc, normal], dim=3)
        return net_in, depth_img

    def decode_rendering_layer(self, pred_params, im_gray=None, R=None, pose_grad=False, normal_grad=False, depth_interp=False):
        """vertices_transform -> coarse_net_input in one call and ONE autograd node: (B,1,1,d) or (B,d) parameters ->
        (net_input [B,H,W,7], depth_img [B,H,W,1]), the same bits as the two-step route.  Forward
        fr_decode_rendering_layer_forward, backward fr_decode_render_backward (rendering_layer/ops.py::_DecodeRenderingLayer):
        no dense [B,3,N] vertex tensor exists in either direction and none is kept for the backward.  Where the fused entry
        points do not serve the call (a shape only the fallback rasteriser covers, a basis of more than 256 coefficients, a
        mesh of fewer than 16 vertices, the opt-in Q30 decode arithmetic) it IS the two-step route.
        pose_grad=True (default False: the angles get 0, R no gradient): the backward is fr_decode_render_backward_pose -- the
        angle columns are filled (R=None) or dL/dR is returned for R.  The node then KEEPS the forward's pitched vertex hand-off,
        a [B,3,pitch] buffer of its own (41 MB at 64 faces of the full mesh), instead of the shared per-stream scratch.  The
        two-step route takes the flag through vertices_transform.
        normal_grad=True: the call IS the two-step route -- vertices_transform, then coarse_net_input(normal_grad=True).  The
        one-call backward does not apply: it is z-only by construction (only the z plane of the vertex gradient ever exists in
        it), and the normal gradient fills x, y and z.
        depth_interp=True: likewise the two-step route -- vertices_transform, then coarse_net_input(depth_interp=True) -- and for
        the same reason: the interpolated depth's gradient fills x, y and z.  With pose_grad=True that is what turns the head
        from a depth loss."""
        h = _host()
        p = pred_params
        if p.dim() == 4:
            p = p.reshape(p.shape[0], p.shape[-1])
        if p.dim() != 2 or p.shape[1] != self.ndim:
            raise ValueError("pred_params must be (B,1,1,%d) or (B,%d)" % (self.ndim, self.ndim))
        p = h.require_gpu_f32(p, "pred_params")
        B = int(p.shape[0])
        im_gray = self.im_gray if im_gray is None else im_gray
        if im_gray is None:
            im_gray = torch.ones((B, self.im_size, self.im_size, 1), dtype=torch.float32, device=p.device)
        Rc = None
        if R is not None:
            Rc = h.require_gpu_f32(torch.as_tensor(R, dtype=torch.float32, device=p.device), "R")
            if tuple(Rc.shape) != (B, 3, 3):
                raise ValueError("R must be (B,3,3)")
        if normal_grad or depth_interp:
            kw = {"normal_grad": True} if normal_grad else {}
            if depth_interp:
                kw["depth_interp"] = True
            return self.coarse_net_input(self.vertices_transform(p, R=Rc, pose_grad=pose_grad), im_gray=im_gray, **kw)
        if self._basis.backward_packed_ok() and not self._basis.use_q30():
            try:
                return _ops().decode_rendering_layer(p, Rc, im_gray, self.tri, self.vertex_code, self._basis, self.im_size,
                                                     pose_grad=pose_grad)
            except NotImplementedError:
                pass
        return self.coarse_net_input(self.vertices_transform(p, R=Rc, pose_grad=pose_grad), im_gray=im_gray)

    def compute_abedo_image(self, vertices, triangles, abedos, im_gray=None, normal_grad=False, texture_grad=False,
                            with_tri_ind=False):
        """Albedo (3,N) -> albedo image + normalised normal map through a second render (network.py:394-417).
        normal_grad=True: the normal map carries its gradient to the vertices (render_depth, normal_grad); default: a constant
        to autograd, as the reference.
        texture_grad=True: the albedo image carries its gradient to `abedos` (render_depth, texture_grad); default: none.
        with_tri_ind=True: also returns the render's tri_ind [B,H,W,1] (-1 = background) as a third value; default: two values."""
        ver = vertices.float()
        tri = torch.as_tensor(triangles, dtype=torch.float32, device=ver.device)
        tex = torch.as_tensor(abedos, dtype=torch.float32, device=ver.device)
        B = ver.shape[0]
        image = torch.zeros((B, self.im_size, self.im_size, 3), dtype=torch.float32, device=ver.device)
        kw = {"normal_grad": True} if normal_grad else {}
        if texture_grad:
            kw["texture_grad"] = True
        _, tf_abedo, normal, tri_ind = _ops().render_depth(ver=ver, tri=tri, texture=tex, image=image, **kw)
        abedos_image = torch.clamp_min(tf_abedo, 1e-6).mean(dim=-1, keepdim=True)  # (B, H, W, 1)
        flip = normal[..., 2:3] < 0
        normal = torch.where(flip, -1.0 * normal, normal)
        mag = (normal * normal).sum(-1)
        mag = torch.where(mag > 1e-6, mag, torch.ones_like(mag))
        normal_map = normal / (torch.sqrt(mag) + 1e-6)[..., None]
        if with_tri_ind:
            return abedos_image, normal_map, tri_ind
        return abedos_image, normal_map

    def depth_rendering_layer(self):
        """(network.py:300-309)"""
        self.vertices_proj = self.vertices_transform(self.pred_params)
        self.pncc_batch, self.normal_batch, self.maskimg_batch, self.coarse_depth_map = \
            self.rendering_layer(self.vertices_proj, self.tri, self.vertex_code)
        return self.coarse_depth_map

    # ---- parameter helpers ----------------------------------------------------------------------------------
    def set_constraints(self, pred_params):
        """sigmoid -> value ranges of the 235-d vector (network.py:204-218)."""
        s = torch.sigmoid(pred_params)
        nps, ns = self.ndim_pose, self.ndim_shape
        self.pred_params = torch.cat([s[..., 0:3] * 3.0 - 1.5,
                                      s[..., 3:5] * self.im_size,
                                      s[..., 5:6] * 0.0,
                                      s[..., 6:7] * 1e-3,
                                      s[..., nps:nps + ns] * 1e4,
                                      s[..., nps + ns:self.ndim] * 3.0 - 1.5], dim=-1)
        return self.pred_params

    def parse_pose_params(self, pose_params):
        """(B,7) -> phi, gamma, theta (B,1), t3d (B,3), f (B,1)  (network.py:253-263)."""
        return (pose_params[:, 0:1], pose_params[:, 1:2], pose_params[:, 2:3], pose_params[:, 3:6],
                pose_params[:, 6:7])

    def rotation_matrix(self, angles):
        """Host numpy rotation, float64 trig and products, one rounding to fp32 (network.py:266-291)."""
        phi, gamma, theta = angles
        R_pitch = np.array([[1, 0, 0], [0, cos(phi), sin(phi)], [0, -sin(phi), cos(phi)]])
        R_yaw = np.array([[cos(gamma), 0, -sin(gamma)], [0, 1, 0], [sin(gamma), 0, cos(gamma)]])
        R_roll = np.array([[cos(theta), sin(theta), 0], [-sin(theta), cos(theta), 0], [0, 0, 1]])
        return np.dot(np.dot(R_pitch, R_yaw), R_roll).astype(np.float32)

    def rotation_matrix_batch(self, angles_batch):
        """(network.py:292-297)"""
        angles_batch = np.asarray(angles_batch)
        R_batch = np.zeros([angles_batch.shape[0], 3, 3], dtype=np.float32)
        for i in range(angles_batch.shape[0]):
            R_batch[i] = self.rotation_matrix(angles_batch[i])
        return R_batch
