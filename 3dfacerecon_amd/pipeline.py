"""Launch plan for the CoarseNet -> render loop's hot path: 235-d parameters -> decode -> render_depth.

`FaceRecNet.vertices_transform` + `rendering_layer.ops.render_depth` allocate their outputs per call, like the
reference op does (render_depth_op.cc:442-445).  A serving / training loop that runs the same shapes every
iteration should not pay that: a `DecodeRenderPlan` owns the vertex hand-off buffer and the four output planes once
(HBM is 288 GB; one 64-face plan is 123 MB), keeps the ctypes argument list prebuilt, and runs the fused
decode -> render entry point (fr_decode_render_forward: ONE C call, three kernel launches on torch's current HIP
stream); it can be captured into a hipGraph (`capture()` / `replay()`).  The projected vertices are handed from the
decode to the rasteriser in the library's pitched row layout (rows padded to 128-byte multiples, so every decode
store is an aligned half line); `plan.vertex_proj` is the strided [B,3,N] VIEW of that buffer -- same values, same
indexing, not contiguous.  Outputs are views of the plan's buffers: they are overwritten by the next `step()`.
Forward only (no autograd); use rendering_layer.ops.render_depth when gradients are needed.
"""
import ctypes
import importlib.util
import os
import sys

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))


def _host():
    name = "_fr_hotpath_host"
    mod = sys.modules.get(name)
    if mod is None:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_PKG_DIR, "_lib.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return mod


class DecodeRenderPlan:
    def __init__(self, net, batch, height=None, width=None, texture=None, stream=None, strip_rows=0):
        """net: nets.network.FaceRecNet (holds the packed basis, tri, vertex_code); texture: (3,N) or (B,3,N)
        tensor, default net.vertex_code (the PNCC colour code, reference network.py:116).  stream: a torch.cuda.Stream
        every launch of this plan goes to (default: whatever torch's current stream is at the call).  strip_rows: rows per
        screen strip of the resolver (FR_PHASES_STRIP_ROWS in include/fr_hotpath.h; 0 = the library's choice), 0 .. 255, fixed
        for the plan's life (a read-only property)."""
        h = _host()
        self.stream = stream
        rows = int(strip_rows)
        if not 0 <= rows <= 255:
            raise ValueError("strip_rows must be 0 (the library's choice) .. 255, got %d" % rows)
        self._strip_rows = rows
        self._hint = rows << 8
        # the strip geometry the buckets in the workspace were emitted under: the strip hint is the plan's for life, so the launcher
        # option epoch (_lib.option_epoch) of the last successful call that ran the emit phase names it; None before any -- a
        # resolve-only call must find the same (_run)
        self._opts = h._STATE
        self._emit_epoch = None
        self._h = h
        self._L = L = h.lib()
        self.net = net
        self.device = net.device
        self.B = int(batch)
        self.H = int(net.im_size if height is None else height)
        self.W = int(net.im_size if width is None else width)
        self.N = net.nvert
        self.T = int(net.tri.shape[1])
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros((self.B, net.ndim), **f32)
        self.depth = torch.empty((self.B, self.H, self.W, 1), **f32)
        self.texture_image = torch.empty((self.B, self.H, self.W, 3), **f32)
        self.normal = torch.empty((self.B, self.H, self.W, 3), **f32)
        self.tri_ind = torch.empty((self.B, self.H, self.W, 1), **f32)
        tex = net.vertex_code if texture is None else h.require_gpu_f32(texture, "texture")
        self.texture = tex.contiguous()
        self.tex_batch = 1 if self.texture.dim() == 2 else int(self.texture.shape[0])
        if self.tex_batch not in (1, self.B) or self.texture.shape[-2] != 3 or self.texture.shape[-1] != self.N:
            raise ValueError("texture must be (3,N), (1,3,N) or (B,3,N)")
        ws_bytes = L.fr_render_depth_workspace_bytes(self.B, self.N, self.T, self.H, self.W)
        self._ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=self.device)
        self._ws_bytes = ws_bytes
        p = h.ptr
        # The decode arithmetic is fixed when the plan is built: the f32 chain (fr_decode_render_forward), or -- when the Q30
        # arithmetic is selected at that moment -- fr_decode_render_forward_q30 with the level count of that moment and a
        # staging workspace the PLAN owns.  Same phases, same pitched hand-off.  Nothing is allocated at launch time either
        # way, so the plan can be captured on any stream.  `plan.q30` = 0 (f32 chain) or the Q30 level count (7 / 5 / 4).
        basis = net._basis
        self.q30 = int(h.q30_levels()) if basis.use_q30() else 0
        self.pitch = int(L.fr_decode_render_vertex_pitch(self.N))
        self._vertex = torch.empty((self.B, 3, self.pitch), **f32)     # (torch allocations are >= 256-byte aligned)
        self._vertex_bytes = self._vertex.numel() * 4
        self.vertex_proj = self._vertex[:, :, :self.N]                   # [B,3,N]; a strided view when pitch > N
        if self.q30:
            self._q_ws = torch.empty((basis.q30_ws_bytes,), dtype=torch.uint8, device=self.device)
            self._fused_args = (p(self.params), p(basis.qimage()), None, p(net.tri), p(self.texture), self.B, self.N,
                                net.ndim_shape, net.ndim_exp, self.T, self.H, self.W, self.tex_batch,
                                ctypes.c_float(float(net.im_size)), self.q30, p(self._vertex), self._vertex_bytes, p(self.depth),
                                p(self.texture_image), p(self.normal), p(self.tri_ind), p(self._ws), ws_bytes,
                                p(self._q_ws), basis.q30_ws_bytes)
            self._fused_fn, self._fused_name = L.fr_decode_render_forward_q30, "fr_decode_render_forward_q30"
        else:
            self._fused_args = (p(self.params), p(basis.image), None, p(net.tri), p(self.texture), self.B, self.N,
                                net.ndim_shape, net.ndim_exp, self.T, self.H, self.W, self.tex_batch,
                                ctypes.c_float(float(net.im_size)), p(self._vertex), self._vertex_bytes, p(self.depth),
                                p(self.texture_image), p(self.normal), p(self.tri_ind), p(self._ws), ws_bytes)
            self._fused_fn, self._fused_name = L.fr_decode_render_forward, "fr_decode_render_forward"
        self._graph = None
        # the triangle list is a constant of the model (reference network.py:178): convert + range-check it ONCE into the
        # workspace's table; every step then runs the decode, emit and resolve phases only
        self._tri_packed = False
        self.pack_tri()

    @property
    def strip_rows(self):
        return self._strip_rows

    def _stream(self):
        st = self.stream if self.stream is not None else torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(st.cuda_stream)

    def _run(self, phases):
        """Phase bits of fr_decode_render_forward: 8 = decode, 4 = pack the triangle list, 1 = emit, 2 = resolve.
        The resolver reads the buckets the emit phase wrote for ONE strip layout, which the strip hint and the process-wide
        FR_RENDER_ROWS / FR_RENDER_IMPL decide: a resolve without its emit (render_phase(2)) is refused, before anything is
        launched, unless the last emit of this plan ran under the launcher options in force now (the same option epoch; the
        strip hint is the plan's for life)."""
        epoch = self._opts.option_epoch
        if (phases & 3) == 2 and self._emit_epoch != epoch:
            raise RuntimeError("DecodeRenderPlan: a resolve without an emit under the same strip geometry (%s): run render_phase(1) "
                               "or step() first" % ("no emit yet" if self._emit_epoch is None else
                                                    "the launcher options changed since the last emit"))
        rc = self._fused_fn(*self._fused_args, self._stream(), phases | self._hint)
        if phases & 1:
            self._emit_epoch = epoch if rc == 0 else None
        if rc:
            self._h.check(rc, self._fused_name)

    def pack_tri(self):
        """(Re)builds the pre-validated triangle table in the workspace; call again after changing net.tri in place."""
        with torch.cuda.device(self.device):
            self._run(4)
        self._tri_packed = True

    # -- eager launches on the current stream ---------------------------------------------------------------
    def decode(self):
        self._run(8)

    def render(self):
        self._run(3)

    def render_phase(self, phases):
        """phases = 1 launches only raster_emit_kernel, 2 only resolve_write_kernel, 4 only pack_tri_kernel."""
        self._run(int(phases) & 7)

    def outputs(self):
        return self.depth, self.texture_image, self.normal, self.tri_ind

    def _take_params(self, params):
        """Copies `params` (B,d) into the plan's buffer in the order the launches need.  An unbound plan copies on torch's
        current stream, where its launches go too.  A plan BOUND to a stream launches there, so the copy must run there as
        well, behind whatever produced `params` on the current stream: the bound stream waits for the current one, the copy is
        enqueued on the bound stream, and `params` is marked as used by it (the caller may drop it at once)."""
        if params is None:
            return
        src = params.reshape(self.B, -1)
        if self.stream is None:
            self.params.copy_(src, non_blocking=True)
            return
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self.params.copy_(src, non_blocking=True)
        if src.is_cuda:
            src.record_stream(self.stream)

    def step(self, params=None):
        """decode + render of one batch (one C call).  `params` (B,d) is copied into the plan's buffer when given (on the
        plan's own stream when it is bound to one: see _take_params).  A bound plan's outputs are complete when ITS stream
        has run them (`plan.stream.synchronize()`, or `torch.cuda.current_stream().wait_stream(plan.stream)`)."""
        self._take_params(params)
        self._run(11)
        return self.outputs()

    # -- hipGraph ------------------------------------------------------------------------------------------------
    def capture(self):
        """Captures decode + render (reading self.params, writing the plan's outputs) into a hipGraph."""
        if self.stream is not None:
            raise RuntimeError("a plan bound to a stream launches eagerly on it; build an unbound plan to capture a hipGraph")
        with torch.cuda.device(self.device):
            self.step()  # warm-up launch outside the capture (function attributes, lazy module load)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run(11)
        self._graph = g
        return g

    def replay(self, params=None):
        if self._graph is None:
            self.capture()
        self._take_params(params)   # (capture() refuses bound plans, so this is the current-stream copy)
        self._graph.replay()
        return self.outputs()

    def __del__(self):   # a bound plan's buffers go back to torch's allocator: not while its stream still runs on them
        try:
            if self.stream is not None:
                self.stream.synchronize()
        except Exception:
            pass


class GraphedSteps:
    """R consecutive batches captured into ONE hipGraph: R DecodeRenderPlans (each its own parameters, vertex buffer, workspace
    and output planes) whose 3 R launches are replayed with a single hipGraphLaunch.  Why: a replay is followed by a ~9 us
    bubble before the next replay's first kernel starts (hipGraphLaunch is not pipelined with the previous graph's tail on this
    runtime: profiles/round4_probes/r4h), which makes a one-step graph slower than three eager launches; with R steps per graph
    the bubble is paid once per R batches.  `replay(params_list)` copies up to R parameter sets and replays; `plans[i].outputs()`
    are batch i's planes."""

    def __init__(self, net, batch, steps, height=None, width=None, texture=None):
        if int(steps) < 1:
            raise ValueError("steps must be >= 1")
        self.device = net.device
        self.plans = [DecodeRenderPlan(net, batch, height, width, texture) for _ in range(int(steps))]
        self._graph = None

    def capture(self):
        with torch.cuda.device(self.device):
            for p in self.plans:
                p.step()     # warm-up launches outside the capture
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for p in self.plans:
                    p._run(11)
        self._graph = g
        return g

    def replay(self, params_list=None):
        if self._graph is None:
            self.capture()
        if params_list is not None:
            for p, prm in zip(self.plans, params_list):
                p._take_params(prm)
        self._graph.replay()
        return [p.outputs() for p in self.plans]


class BatchesInFlight:
    """S (default two) independent batches in flight: S DecodeRenderPlans -- each with its own parameters, vertex buffer,
    workspace and output planes -- each bound to its own HIP stream, with NO edge between the streams.  `submit()` sends the
    next batch down the next slot's stream (round robin) and returns that slot.  Consecutive batches of a serving loop are
    independent (render_depth_op.cc:180 loops over them one after the other only because it is a serial program), so the
    hardware may run the decode of one beside the render of the other: one batch's kernels fill the tails, launch gaps and
    idle units of the other's.  Measured on an MI355X at 64 faces: 100-103 us per batch against 110 us for one plan stepping
    on one stream (tools/multistream_probe.py; three in flight: slower again -- the batches' working sets evict each other
    from the 256 MiB Infinity Cache).  The first slot's stream has high priority and the others normal priority: at equal priority the
    streams sometimes lock into step (both decodes, then both emits ... -- 100 to 107 us from one process to the next); with
    one batch entitled to run ahead and the other filling in, 100.5-101.6 us (profiles/round4_probes/r4p).

    Rules of use: a slot's outputs are complete when ITS stream has run dry (`slot.wait()`, or
    `slot.make_current_stream_wait()` to order a consumer on torch's current stream behind it) and are overwritten when the
    slot comes round again (S submits later).  `submit(params)` copies `params` into the slot's buffer on the slot's stream
    after making that stream wait for torch's current stream (the producer of `params`)."""

    def __init__(self, net, batch, height=None, width=None, texture=None, slots=2, strip_rows=None):
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        self.device = net.device
        if strip_rows is None or int(strip_rows) < 0:   # (negative: "auto", as bench.py --strip-rows -1)
            strip_rows = self.strip_rows_in_flight(net, batch, height, width) if int(slots) > 1 else 0
        self._strip_rows = int(strip_rows)
        with torch.cuda.device(self.device):
            self.slots = []
            for i in range(int(slots)):
                # torch stream priorities on ROCm: negative = high, and anything >= 0 is clamped to 0 = normal (there is no "low"
                # through this API): slot 0 runs at HIGH priority, the others at NORMAL -- one batch entitled to run ahead, the
                # other filling in (profiles/round4_probes/r4p: equal priorities sometimes lock the streams into step)
                st = torch.cuda.Stream(device=self.device, priority=(-1 if i == 0 else 0))
                self.slots.append(_Slot(net, batch, height, width, texture, stream=st, strip_rows=self._strip_rows))
            torch.cuda.synchronize(self.device)   # every slot's triangle table is packed before anything else touches the slots
        self._next = 0
        self.B = self.slots[0].B

    @property
    def strip_rows(self):
        """The strip hint every slot was built with (read-only: the slots' plans keep theirs for life)."""
        return self._strip_rows

    @staticmethod
    def strip_rows_in_flight(net, batch, height=None, width=None):
        """The resolver's strip height for plans that run BESIDE another batch: four fifths of the library's own choice in the regime
        it was measured in -- strips of ten rows or more and at least four resolver workgroups per CU (200 x 200 at 64 faces: 8
        rows instead of 10, 1,600 workgroups instead of 1,280, which fill the other batch's gaps better: -0.8 us per batch with two in
        flight, +1.3 us one batch at a time; profiles/round4_probes/r4q, round6_probes/r6f) -- otherwise 0 = no hint.  A scheduling
        hint: no result bit depends on it."""
        h = _host()
        H = int(net.im_size if height is None else height)
        W = int(net.im_size if width is None else width)
        rows = int(h.lib().fr_render_depth_strip_rows(int(batch), int(net.tri.shape[1]), H, W))
        if rows < 10 or int(batch) * ((H + rows - 1) // rows) < 1024:
            return 0
        return (4 * rows) // 5

    def submit(self, params=None, marks=None):
        """Launches decode + render of one batch on the next slot's stream; returns the slot (a DecodeRenderPlan).
        marks: four torch.cuda.Events to record on the slot's stream before the decode, between the three launches and
        after the resolve (bench.py's per-kernel timing; the step then goes out as three C calls instead of one)."""
        sl = self.slots[self._next]
        self._next = (self._next + 1) % len(self.slots)
        sl._take_params(params)   # (on the slot's stream, behind torch's current stream: DecodeRenderPlan._take_params)
        if marks is None:
            sl._run(11)
        else:
            marks[0].record(sl.stream)
            sl._run(8)
            marks[1].record(sl.stream)
            sl._run(1)
            marks[2].record(sl.stream)
            sl._run(2)
            marks[3].record(sl.stream)
        return sl

    def synchronize(self):
        for sl in self.slots:
            sl.stream.synchronize()

    def __del__(self):   # the slots' buffers go back to torch's allocator: not while their streams still run
        try:
            self.synchronize()
        except Exception:
            pass


class _Slot(DecodeRenderPlan):
    def wait(self):
        self.stream.synchronize()
        return self.outputs()

    def make_current_stream_wait(self):
        torch.cuda.current_stream(self.device).wait_stream(self.stream)


def synth_face_range(step, rank, world, batch):
    """(first_face, end) of the batch rank `rank` of `world` draws at step `step`: first_face = (step world + rank) batch.  The
    ranks' ranges of one step lie side by side and the steps follow one another, so the union over ranks is exactly the face
    sequence one process draws with batch `world batch` -- a face's values depend on (seed, global face index) alone."""
    step, rank, world, batch = int(step), int(rank), int(world), int(batch)
    if step < 0 or world < 1 or not 0 <= rank < world or batch < 1:
        raise ValueError("synth_face_range: step >= 0, 0 <= rank < world, batch >= 1")
    first = (step * world + rank) * batch
    return first, first + batch


class _SynthSlot:
    """One buffer set of SynthBatches and the stream its five launches go down."""

    def __init__(self, owner, stream):
        net, B, H, W = owner.net, owner.B, owner.H, owner.W
        f32 = dict(dtype=torch.float32, device=owner.device)
        self.stream = stream
        self.event = torch.cuda.Event()
        self.tex = torch.empty((B, 3, net.nvert), **f32)
        # decode -> render of the slot's own parameters with the slot's per-face texture, bound to the slot's stream
        self.plan = DecodeRenderPlan(net, B, H, W, texture=self.tex, stream=stream)
        self.params = self.plan.params
        self.light = torch.empty((B, 4), **f32)
        # colour: the batch's lighting is [B,3,9] and the image has three channels; the first-order draw above is still made (the
        # sampler's other outputs do not move) and goes unused
        self.light_rgb = torch.empty((B, 3, 9), **f32) if owner.colour else None
        self.im_rgb = torch.empty((B, H, W, 3), **f32) if owner.colour else None
        self.alpha = torch.empty((B, owner.K), **f32)
        self.im_gray = torch.empty((B, H, W, 1), **f32)
        self.mask = torch.empty((B, H, W, 1), **f32)
        self.depth = torch.empty((B, H, W, 1), **f32)
        self.landmarks = self.landmark_visible = None
        if owner.landmark_basis is not None:
            self.landmarks = torch.empty((B, owner.landmark_basis.K, 2), **f32)
            self.landmark_visible = torch.empty((B, owner.landmark_basis.K), **f32)
        self.contour_landmarks = self.contour_sel = None
        if owner.contour_basis is not None:
            self.contour_landmarks = torch.empty((B, owner.contour_basis.C, 2), **f32)
            self.contour_sel = torch.empty((B, owner.contour_basis.C), dtype=torch.int32, device=owner.device)
        self.first_face = None

    def batch(self):
        out = {"im_gray": self.im_gray, "params": self.params, "depth": self.depth, "mask": self.mask,
               "tri_ind": self.plan.tri_ind, "light": self.light, "alpha": self.alpha}
        if self.im_rgb is not None:
            out.update(im_rgb=self.im_rgb, light=self.light_rgb)
        if self.landmarks is not None:
            out.update(landmarks=self.landmarks, landmark_visible=self.landmark_visible)
        if self.contour_landmarks is not None:
            out.update(contour_landmarks=self.contour_landmarks, contour_sel=self.contour_sel)
        return out


class SynthBatches:
    """Training batches made on the device: every `next()` returns a batch whose image DEPICTS its label -- random parameters, the
    face they decode to rendered with a random per-face albedo under a random first-order lighting, and that face's ground-truth
    depth and mask.  Per batch, on a side stream, with no host work, no copy and no dataset:
        synth_params -> fr_decode_3dmm -> synth_texture -> render (per-face [B,3,N] texture) -> synth_shade
    (rendering_layer/ops.py; decode and render are one DecodeRenderPlan step).  Modelled on BatchesInFlight: every slot owns its
    buffers and a stream.  `next()` makes torch's current stream wait for the slot that holds the batch, starts the FOLLOWING
    batch on the following slot's stream, and returns
        {"im_gray" [B,H,W,1], "params" [B,d], "depth" [B,H,W,1], "mask" [B,H,W,1], "tri_ind" [B,H,W,1], "light" [B,4], "alpha" [B,K]}
    -- views of the slot's buffers, nothing requires grad.  `depth` is the clamped flat depth image FaceRecNet.rendering_layer
    returns for those parameters; `mask` is 1.0 where a triangle covers the pixel.  A returned batch stays as it is until `slots`
    calls later: `slots` batches are the caller's, and one more buffer set holds the batch in the making, so slots + 1 sets exist.
    Before a set is written again its stream waits for torch's current stream of that moment (the consumer's reads enqueued so far).
    Faces are numbered globally: call n draws faces first_face + n stride .. + batch (stride: default `batch`).  A rank of a
    sharded loop passes first_face = synth_face_range(0, rank, world, batch)[0] and stride = world batch; the ranks' streams
    together are then the single-process stream, face for face.  Two streams with different seeds are independent.
    The launches go out eagerly: first_face travels in the sampler's launch arguments, which a captured graph would freeze.
    colour=True (default False: every bit is the gray stream's): the face is shaded in colour -- per-channel albedo under a
    second-order lighting per channel (synth_light_rgb -> synth_shade_rgb).  A batch then also carries "im_rgb" [B,H,W,3], its
    "light" is [B,3,9] (light_ranges: 27 pairs, default ops.SYNTH_LIGHT_RANGES_RGB), "im_gray" is the gray of that image
    (0.3 R + 0.59 G + 0.11 B: what the nets take) and a background is [1,H,W,3] or [B,H,W,3].  params, alpha, depth, mask and
    tri_ind are those of the gray stream with the same seed: the colour lighting is drawn on a sampler stream of its own.
    landmarks=idx (default None: every bit is today's stream): K vertex ids.  A batch then also carries, made on the slot's stream,
    "landmarks" [B,K,2] -- x and y of the sparse forward of its own parameters (FaceRecNet.landmarks: the compact image, not the
    dense decode) -- and "landmark_visible" [B,K] fp32, 1.0 where rendering_layer/ops.py::mesh_visible of the batch's render marks
    the vertex, else 0.0: ready to be the weight of nets/losses.py::landmark_loss.
    contour_lines=(lines [C,M], line_dir [C,2]) (default None: every existing key keeps its bits), e.g. utils/synth.py::contour_lines:
    a batch then also carries, made on the slot's stream, "contour_landmarks" [B,C,2] -- per line, x and y of the candidate that is
    extreme along the line's direction at the batch's own parameters: the face's occluding contour on that line -- and "contour_sel"
    [B,C] int32, that candidate's position in its line (rendering_layer/ops.py::landmark_contour_select, rule "extreme")."""

    def __init__(self, net, batch, seed, slots=2, first_face=0, stride=None, light_ranges=None, alpha_ranges=1.0, background=None,
                 gain=1.0, offset=0.0, beta=0.7, focal=1e-3, height=None, width=None, landmarks=None,
                 contour_lines=None, colour=False):
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        if net.mu_tex is None:
            raise ValueError("the asset dict has no texture model (mu_tex)")
        # the operator module the net itself renders through: the loader of the module that defines FaceRecNet (nets/network.py)
        self._ops = ops = next(m._ops for m in (sys.modules.get(c.__module__) for c in type(net).__mro__) if hasattr(m, "_ops"))()
        self.net = net
        self.device = net.device
        self.B = int(batch)
        self.H = int(net.im_size if height is None else height)
        self.W = int(net.im_size if width is None else width)
        self.K = 0 if net.pc_tex is None else int(net.pc_tex.shape[1])
        self.seed = int(seed)
        self.first_face = int(first_face)
        self.stride = self.B if stride is None else int(stride)
        self.colour = bool(colour)
        self.light_ranges = ops.SYNTH_LIGHT_RANGES if light_ranges is None or self.colour else light_ranges
        self.light_ranges_rgb = (ops.SYNTH_LIGHT_RANGES_RGB if light_ranges is None else light_ranges) if self.colour else None
        self.alpha_ranges = alpha_ranges
        self.gain, self.offset, self.beta, self.focal = float(gain), float(offset), float(beta), float(focal)
        self.background = None
        if background is not None:
            self.background = _host().require_gpu_f32(background, "background")
        self.lifetime = int(slots)
        self.landmark_basis = self._landmark_idx = None
        if landmarks is not None:
            self.landmark_basis = net.landmark_basis(landmarks)
            self._landmark_idx = torch.tensor(self.landmark_basis.idx, dtype=torch.int64, device=self.device)
        self.contour_basis = self._contour_dir = None
        if contour_lines is not None:
            lines, line_dir = contour_lines
            self.contour_basis = net.landmark_contour_basis(None, lines)
            self._contour_dir = torch.as_tensor(line_dir, dtype=torch.float32).to(self.device).contiguous()
        with torch.cuda.device(self.device):
            self.slots = [_SynthSlot(self, torch.cuda.Stream(device=self.device)) for _ in range(int(slots) + 1)]
            torch.cuda.synchronize(self.device)   # every slot's triangle table is packed before anything else touches the slots
            self._made = 0     # batches started
            self._taken = 0    # batches returned
            self._generate()

    def _generate(self):
        """Starts batch number self._made on its slot's stream, behind whatever torch's current stream holds now."""
        n = self._made
        sl = self.slots[n % len(self.slots)]
        ops, net = self._ops, self.net
        sl.first_face = self.first_face + n * self.stride
        sl.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(sl.stream):
            ops.synth_params(self.seed, sl.first_face, self.B, net.ndim_shape, net.ndim_exp, self.K, net.im_size, beta=self.beta,
                             light_ranges=self.light_ranges, alpha_ranges=self.alpha_ranges, focal=self.focal,
                             out=(sl.params, sl.light, sl.alpha))
            ops.synth_texture(net.mu_tex, net.pc_tex, sl.alpha, out=sl.tex)
            sl.plan.step()
            if self.colour:
                ops.synth_light_rgb(self.seed, sl.first_face, self.B, ranges=self.light_ranges_rgb, out=sl.light_rgb)
                ops.synth_shade_rgb(sl.plan.texture_image, sl.plan.normal, sl.plan.tri_ind, sl.light_rgb, background=self.background,
                                    gain=self.gain, offset=self.offset, out=(sl.im_rgb, sl.im_gray, sl.mask))
            else:
                ops.synth_shade(sl.plan.texture_image, sl.plan.normal, sl.plan.tri_ind, sl.light, background=self.background,
                                gain=self.gain, offset=self.offset, out=(sl.im_gray, sl.mask))
            torch.clamp_min(sl.plan.depth, 1e-6, out=sl.depth)
            if self.landmark_basis is not None:
                with torch.no_grad():
                    points = ops.landmarks(sl.params, self.landmark_basis, im_size=net.im_size)
                    sl.landmarks.copy_(points[:, 0:2].transpose(1, 2))
                    visible = ops.mesh_visible(net.tri, sl.plan.tri_ind, net.nvert)
                    sl.landmark_visible.copy_(visible.index_select(1, self._landmark_idx))
            if self.contour_basis is not None:
                sel, points, _, _ = ops.landmark_contour_select(sl.params, self.contour_basis, rule="extreme", line_dir=self._contour_dir,
                                                                im_size=net.im_size)
                sl.contour_sel.copy_(sel)
                sl.contour_landmarks.copy_(points)
            sl.event.record(sl.stream)
        self._made = n + 1

    def next(self):
        sl = self.slots[self._taken % len(self.slots)]
        self._taken += 1
        torch.cuda.current_stream(self.device).wait_event(sl.event)
        self._generate()
        return sl.batch()

    def synchronize(self):
        for sl in self.slots:
            sl.stream.synchronize()

    def __del__(self):   # the slots' buffers go back to torch's allocator: not while their streams still run
        try:
            self.synchronize()
        except Exception:
            pass
