/*
 * fr_hotpath.h -- C ABI of the MI355X (gfx950) render_depth + 3DMM-decode hot path.
 *
 * This is the drop-in boundary.  The reference has no C ABI of its own for this path: its only native
 * boundary is the TensorFlow OpKernel C++ ABI (rendering_layer/ops_src/render_depth_op.cc:371-604, loaded by
 * rendering_layer/ops.py:68 through tf.load_op_library).  Each entry point below cites the reference
 * interface it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds to rendering_layer/ops.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (outputs and workspaces included); the library
 *     allocates nothing and never synchronises with the host;
 *   - `hip_stream` is a hipStream_t (NULL = the default stream); all work is enqueued on it, in order;
 *   - return value: FR_OK (0) or a negative FR_ERR_* code (never swallowed, unlike the reference's
 *     printf-and-return at render_depth_op.cu.cc:290-295); fr_strerror() names it;
 *   - reentrant: no static scratch (unlike render_depth_op.cc:125-131); the only process-wide state is the option table
 *     (atomics, filled from the environment once under std::call_once) and per-device caches of launch attributes (atomics),
 *     so any number of host threads may make their first calls at the same moment.  What is supported, exactly
 *     (tests/test_threads_gpu.py holds each to the single-threaded results, bit for bit):
 *       * threads calling on DIFFERENT streams with disjoint output / workspace / vertex buffers (the model constants --
 *         packed basis, triangle list, texture -- are only read);
 *       * threads sharing ONE stream: each call enqueues its launches in order, but a call of several phases is several
 *         launches, so calls that share a workspace must be serialised by the caller from the first launch to the last
 *         (rendering_layer/ops.py holds a lock per cached workspace for this);
 *       * options (fr_set_option) are process-wide: a change made by any thread applies to the next call of every thread;
 *       * every phase of ONE workspace's forward -- emit and resolve, and the pack the emit relies on -- must be called under
 *         one geometry: the same strip hint (FR_PHASES_STRIP_ROWS) and the same FR_RENDER_ROWS / FR_RENDER_IMPL.  A resolve
 *         under another strip layout than its emit writes wrong planes with no error (pipeline.DecodeRenderPlan refuses such
 *         a call on the host side);
 *   - calls on different streams run beside each other: two independent batches in flight on two streams
 *     measure ~100 us per 64-face batch against ~111 us one batch at a time on an MI355X (pipeline.BatchesInFlight,
 *     DESIGN.md 4.7);
 *   - tensors are dense, row-major, fp32; triangle indices and tri_ind stay float-typed at the surface as in
 *     the reference op schema (render_depth_op.cc:535-589).
 */
#ifndef FR_HOTPATH_H_
#define FR_HOTPATH_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_OK 0
#define FR_ERR_INVALID_ARG (-1) /* OP_REQUIRES failures, render_depth_op.cc:408-418, 498-503 */
#define FR_ERR_WORKSPACE (-2)   /* workspace / packed-basis buffer too small */
#define FR_ERR_LAUNCH (-3)      /* HIP launch or runtime error */
#define FR_ERR_UNSUPPORTED (-4) /* size outside what the kernels cover (e.g. image row does not fit in LDS) */

#define FR_N_POSE 7 /* [phi,gamma,theta,tx,ty,tz,f], reference README.md:43-46, utils/parser_3dmm.py:49 */

/* Library identification / error text. */
const char* fr_version(void);
const char* fr_strerror(int code);

/* Tuning / A-B knobs of the launchers (no reference counterpart).  Each knob is named like the environment variable
 * that gives it its initial value -- read ONCE per process, at the first use of any knob; the launch path never calls
 * getenv -- and can be changed afterwards only through fr_set_option:
 *   FR_DECODE_IMPL (0 | 1 = "loop": generic decode kernel)   FR_DECODE_WIDE (1 | 0)   FR_DECODE_NBW (0 = auto | 1 | 4)
 *   FR_DECODE_WAVES (16 | 8)   FR_DECODE_NT (-1 = by batch: non-temporal basis stream for passes of 64 faces, default cache
 *   policy below -- default | 1 = always non-temporal | 0 = always the default cache policy)
 *   FR_RESOLVE_OPT (2 = default: wave-local front for 256-thread bins | 1 = block-wide list, single-trip bins keep their
 *   records in registers | 0 = two-pass resolver)   FR_EMIT_FILTER (bits 0-1, default 3)   FR_RENDER_IMPL (0 | 1 = "scan": strip-scan fallback)
 *   FR_RESOLVE_BLOCK (0 = auto | 256 | 512 | 1024)   FR_RENDER_ROWS (0 = auto | rows per screen strip)
 *   FR_DECODE_STORE (0 | 1 = transposed accumulators, one dword per lane per store: measured +1.1 us, A/B only)
 *   FR_DECODE_CUS (test knob: 0 = default, the decode forward launchers fr_decode_3dmm / fr_decode_3dmm_q30* plan for the device's
 *   compute units | n > 0 = for min(n, device): fewer workgroups, so a small mesh walks several rounds of tiles per wave; it
 *   changes no result bit and, at its default, no launch)
 *   FR_BWD_CHUNKS (row chunks of the packed decode-backward GEMM: 256 = default | 1 .. 512; changes the association of the
 *   partial sums, i.e. the gradient's last bits)
 *   FR_BWD_CB (16-coefficient blocks per wave of the fused decode backward: 0 = by batch | 2 | 4; changes no result bit except
 *   d f of fr_decode_3dmm_backward_packed_mu, whose per-workgroup partial it re-associates)
 *   FR_EMIT_ORDER (lane order of a segment's triangles in the emit kernel, fixed by the pack phase: -1 = scored per segment
 *   (default) | 0 = list order | 1 = even triangles, then odd ones; read when the triangle list is packed)
 * Apart from FR_BWD_CHUNKS and FR_BWD_CB, none of them changes a result bit (tests/test_render_gpu.py, tests/test_decode_gpu.py
 * hold every setting to the oracle; tests/test_decode_backward_bounds_gpu.py the two backward knobs).
 * Returns FR_OK or FR_ERR_INVALID_ARG (unknown name). */
int fr_set_option(const char* name, int value);
int fr_get_option(const char* name, int* value);

/* ---- render_depth forward ------------------------------------------------------------------------------
 * Replaces RenderDepthOp<Device>::Compute + functor RenderDepth (render_depth_op.cc:378-458, 132-322;
 * CUDA launchers render_depth_op.cu.cc:239-341) reached from rendering_layer/ops.py:78-81.
 *   vertex  [B,3,nver]  projected vertices (x = column, y = row, z = depth)
 *   tri     [3,ntri]    float-stored 0-based vertex ids (truncated with (int), render_depth_op.cc:204-206)
 *   texture [tex_batch,3,nver], tex_batch == B, or 1 to share one texture across the batch
 *   depth [B,H,W,1], tex_img [B,H,W,3], normal [B,H,W,3], tri_ind [B,H,W,1]   (render_depth_op.cc:437-440)
 * C must be 3 (render_depth_op.cc:418).  Semantics are those of the CPU functor: per pixel the triangle with
 * the largest fp32 centroid depth wins, ties go to the lowest triangle index; background depth is
 * (float)(-99999999999999), tri_ind -1, texture/normal 0.  Triangles with a vertex id outside [0,nver) are
 * skipped.  `workspace` must hold fr_render_depth_workspace_bytes() bytes (may be NULL when that is 0). */
size_t fr_render_depth_workspace_bytes(int B, int nver, int ntri, int H, int W);

int fr_render_depth_forward(const float* vertex, const float* tri, const float* texture, int B, int nver,
                            int ntri, int H, int W, int C, int tex_batch, float* depth, float* tex_img,
                            float* normal, float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream);

/* The forward op phase by phase.  It is three launches: pack_tri_kernel (phase bit 4) converts and range-checks the
 * float-stored triangle list once into a table in the workspace (twice: by triangle id, and per 504-triangle segment in the
 * lane order that makes the emit kernel's gathers cheapest for this list); raster_emit_kernel (bit 1) writes per-strip hit
 * records into the workspace; resolve_write_kernel (bit 2) turns them into the four planes.  phases = 7 is
 * fr_render_depth_forward.  A caller whose triangle list is a constant of the model (the reference makes it a
 * tf.constant, nets/network.py:178) and whose workspace persists may pack once (phases = 4) and then run phases = 3
 * per batch.  The table carries a header naming the (nver, ntri) it was packed for: an emit phase handed a table that
 * was not packed for its arguments (no pack phase yet, or the workspace reused for another shape) treats every triangle
 * as invalid and the planes come out as pure background -- defined, never an out-of-bounds gather.  The table does NOT
 * record the ids themselves: repack after changing `tri` in place.  bench.py also uses single phases to bracket each
 * kernel with HIP events inside the timed region. */
int fr_render_depth_forward_phases(const float* vertex, const float* tri, const float* texture, int B, int nver,
                                   int ntri, int H, int W, int C, int tex_batch, float* depth, float* tex_img,
                                   float* normal, float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream,
                                   int phases);

/* ---- fused rendering layer ------------------------------------------------------------
 * render_depth + the caller-side post-processing of FaceRecNet.rendering_layer (nets/network.py:185-199) in one
 * pass, emitting CoarseNet's 7-channel input directly (network.py:122):
 *   net_input [B,H,W,7] = [ clip(depth,1e-6,1) * im_gray | clip(texture_image,1e-6,1) x3 | n / (sqrt(|n|^2)+1e-6) x3 ]
 *                         with n flipped to n_z >= 0 and |n|^2 <= 1e-6 replaced by 1
 *   depth_img [B,H,W,1] = max(depth, 1e-6);  depth [B,H,W,1] and tri_ind [B,H,W,1] as in fr_render_depth_forward
 *   im_gray   [B,H,W,1].  Same workspace as fr_render_depth_forward.
 * Returns FR_ERR_UNSUPPORTED for shapes only the fallback rasteriser covers (use the plain op + elementwise ops). */
int fr_rendering_layer_forward(const float* vertex, const float* tri, const float* texture, const float* im_gray,
                               int B, int nver, int ntri, int H, int W, int tex_batch, float* net_input,
                               float* depth_img, float* depth, float* tri_ind, void* workspace, size_t ws_bytes,
                               void* hip_stream);

/* The same phase by phase (bits as in fr_render_depth_forward_phases: 4 = pack the triangle list, 1 = emit, 2 = the fused
 * resolve): a caller whose triangle list is a model constant (nets/network.py:178) packs once and runs phases = 3 per call
 * (rendering_layer/ops.py does, under the same tensor-identity rule as render_depth). */
int fr_rendering_layer_forward_phases(const float* vertex, const float* tri, const float* texture, const float* im_gray,
                                      int B, int nver, int ntri, int H, int W, int tex_batch, float* net_input,
                                      float* depth_img, float* depth, float* tri_ind, void* workspace, size_t ws_bytes,
                                      void* hip_stream, int phases);

/* ---- render_depth backward -----------------------------------------------------------------------------
 * Replaces RenderDepthOpGrad::Compute + functor RenderDepthGrad (render_depth_op.cc:470-528, 325-368;
 * render_depth_op.cu.cc:345-423) reached from the gradient registration at rendering_layer/ops.py:86-95.
 *   depth_grad [B,H,W,1], tri [3,ntri], tri_ind [B,H,W,1] (forward output) -> vertex_grad [B,3,nver]
 * Every pixel with tri_ind >= 0 adds (depth_grad * 1.0f) / 3.0f to the z row of its triangle's three vertices; the x and
 * y rows are 0 (render_depth_op.cc:359-363); all of vertex_grad is written.  The per-vertex sums are formed as exact
 * 64-bit fixed-point integers and rounded to fp32 once (a subnormal result is rounded a second time by the final power-of-
 * two scaling): the result is the correctly rounded real sum up to n * 2^-39 * max|term| per face and is bit-identical
 * from run to run (the reference's serial loop has one fixed fp32 order; its CUDA twin uses order-dependent float
 * atomics).  max|term| is taken over the pixels with 0 <= tri_ind < ntri.  Images above 2^20 pixels give up one bit of
 * that resolution per doubling of the pixel count (2^-38 at 2^21 pixels, ...). */
int fr_render_depth_backward(const float* depth_grad, const float* tri, const float* tri_ind,
                             float* vertex_grad, int B, int nver, int ntri, int H, int W, void* hip_stream);

/* The same with a caller-owned workspace (fr_render_depth_backward_workspace_bytes(B, H, W): 16 bytes per pixel of the
 * batch plus 8 per 1,024 pixels, 16-byte aligned): one pre-kernel resolves every pixel to its triangle's three vertex ids ONCE and writes a
 * record per pixel; the accumulating workgroups (several per face) then stream the records instead of each repeating the
 * scattered id gathers.  Results are bit-identical to fr_render_depth_backward (which is this function with
 * workspace = NULL).  A workspace smaller than that, or not 16-byte aligned, is not an error here: it is left untouched
 * and the call runs as fr_render_depth_backward (tests/test_render_backward_exact_gpu.py calls it both ways). */
size_t fr_render_depth_backward_workspace_bytes(int B, int H, int W);

int fr_render_depth_backward_ws(const float* depth_grad, const float* tri, const float* tri_ind, float* vertex_grad,
                                int B, int nver, int ntri, int H, int W, void* workspace, size_t ws_bytes,
                                void* hip_stream);

/* ---- 3DMM decode ---------------------------------------------------------------------------------------
 * Replaces FaceRecNet.vertices_transform + parse_pose_params + rotation_matrix_batch
 * (nets/network.py:140-171, 253-263, 266-297): 235-d parameters -> projected, y-flipped vertices [B,3,N].
 *
 * The basis is a constant of the model (tf.constant at network.py:41-43), so it is re-laid-out ONCE into an
 * MFMA-fragment-ordered image in HBM by fr_decode_pack_basis and then streamed by every decode call:
 *   mu [3N] (blocked: element r = coordinate r/N of vertex r%N, network.py:157),
 *   pc_shape [3N,n_shape], pc_exp [3N,n_exp] row-major (network.py:42-43)
 *   -> packed, fr_decode_packed_basis_bytes(N,n_shape,n_exp) bytes, 16-byte aligned. */
size_t fr_decode_packed_basis_bytes(int N, int n_shape, int n_exp);

int fr_decode_pack_basis(const float* mu, const float* pc_shape, const float* pc_exp, int N, int n_shape,
                         int n_exp, void* packed, size_t packed_bytes, void* hip_stream);

/*   params [B, 7+n_shape+n_exp] = [phi,gamma,theta,tx,ty,tz,f | alpha | beta]   (network.py:142-147)
 *   R_override: NULL, or a caller-computed [B,3,3] rotation (what network.py:150 obtains through tf.py_func);
 *               with NULL the rotation is evaluated in-kernel in float64 exactly as network.py:276-290 does.
 *   vertex_proj [B,3,N]; y row is (im_size - y) - 1 (network.py:167-169).
 * Numerical definition: the reference evaluates S = pc_shape.alpha and E = pc_exp.beta with two fp32
 * tf.matmuls whose summation order is unspecified (network.py:153-156).  fr_decode_3dmm's written definition:
 *   S, E = k-ordered fmaf chains from +0, v = (mu + S) + E  (the f32-input MFMA; the reference's own arithmetic type),
 * restated on the CPU in oracle/fr_oracle.c; the kernel is held to it bit for bit, at every schedule the launcher can choose
 * (FR_DECODE_*, every batch boundary, every grid size) and over all of fp32: subnormal parameters, products and sums are kept
 * (never flushed), a chain may overflow to Inf, a non-finite parameter or pose scalar gives what IEEE arithmetic gives (NaN
 * compares equal to NaN of any sign / payload), and the SIGN of a zero is part of the result -- a chain whose products all
 * underflow ends at -0 when its last product is negative, which is why the packed image pads the basis with -0.0
 * (tests/test_decode_forward_edges_gpu.py).  With n_shape = n_exp = 0 the result is the pose applied to mu. */
int fr_decode_3dmm(const float* params, const void* packed_basis, const float* R_override, int B, int N,
                   int n_shape, int n_exp, float im_size, float* vertex_proj, void* hip_stream);

/* ---- fused decode -> render step (reference hand-off nets/network.py:140-171 -> :174-182) ---------
 * One call launches fr_decode_3dmm and then fr_render_depth_forward_phases on its result.  The projected vertices never
 * take the op surface's dense [B,3,N] form: they are handed from the decode to the rasteriser in a buffer the CALLER owns
 * but whose layout is the library's -- [B,3,pitch] rows with pitch = fr_decode_render_vertex_pitch(N) (N rounded up to a
 * multiple of 32 floats), fr_decode_render_vertex_bytes(B, N) bytes, 128-byte aligned: every 16-vertex piece a decode wave
 * stores is then an aligned half of a 128-byte line (N = 53,215 is odd: in the dense tensor every row starts at another
 * 4-byte phase and every 64-byte piece straddles two lines; measured -2.7 us per 64-face decode).  Element (b, c, p) sits at
 * (b * 3 + c) * pitch + p, so a strided view of the buffer IS the [B,3,N] tensor (the pad floats are never written or read).
 *   phases: bit 8 = decode, bit 4 = pack the triangle list, bit 1 = emit, bit 2 = resolve (15 = everything; a caller whose
 *   triangle list is a model constant runs 4 once and 11 per batch).  Results are bit-identical to the two separate calls.
 *   FR_PHASES_STRIP_ROWS(n) (bits 8-15 of `phases`, 0 = the library's choice): rows per screen strip of the resolver, i.e. how many
 *   resolver workgroups the screen is cut into -- a scheduling hint with no effect on any result bit or workspace size, to be
 *   passed unchanged with every phase of the same workspace.  The library's own choice (10 rows at 64 faces of 200 x 200) is the
 *   fastest one batch at a time; a caller that keeps two batches in flight on two streams does better with 8 (-0.9 us per
 *   batch: smaller resolver workgroups fill the other batch's gaps; +1.3 us one at a time).  A hint the binned rasteriser does not
 *   serve is ignored. */
#define FR_PHASES_STRIP_ROWS(n) (((n) & 0xFF) << 8)
/* The strip height the library itself picks for a shape (what FR_PHASES_STRIP_ROWS(0) means; no GPU needed), 0 when the binned
 * rasteriser does not serve the shape: what a caller scales its hint from. */
int fr_render_depth_strip_rows(int B, int ntri, int H, int W);
int fr_decode_render_vertex_pitch(int N);
size_t fr_decode_render_vertex_bytes(int B, int N);
int fr_decode_render_forward(const float* params, const void* packed_basis, const float* R_override, const float* tri,
                             const float* texture, int B, int N, int n_shape, int n_exp, int ntri, int H, int W,
                             int tex_batch, float im_size, float* vertex_handoff, size_t vertex_bytes, float* depth,
                             float* tex_img, float* normal, float* tri_ind, void* workspace, size_t ws_bytes,
                             void* hip_stream, int phases);

/* (Rounds 4-5 also exported fr_decode_render_pipelined: the emit of batch k and the resolve of batch k-1 as two roles of ONE
 * launch.  Bit-identical, measured 5-8 % slower than this entry point in both rounds and removed in round 6; a caller
 * that wants batches to overlap calls fr_decode_render_forward on two streams with two sets of buffers -- pipeline.BatchesInFlight.) */

/* Second definition of the same decode (nothing of it is built, allocated or launched unless these entry
 * points are called):
 *   Q30: v = fl32(mu + S + E) with S + E a fixed-point dot product of the operands quantised to 31 bits against power-of-two
 *   row / column scales, evaluated on the int8 matrix cores as products of base-256 digits.  `levels` = how many of the seven
 *   digit-product levels are kept: 7 = all sixteen products (the EXACT product of the quantised operands: the correctly
 *   rounded fp32 value of the real-number blend in > 99 % of the cases, half the f32 chain's mean error), 5 = the thirteen
 *   products of weight >= 2^-32 of full scale (what is dropped is below 2^-38 of a term's scale: the same fp32 result in
 *   > 99.98 % of the cases), 4 = the ten products of weight >= 2^-24 (dropped: below 2^-30; mean error 0.29 ulp against 0.26
 *   for the exact product and 0.34 - 0.5 for the f32 chain).  Integer arithmetic: order-independent, restated bit for bit in
 *   oracle/fr_oracle.c ("Q30 decode", the same `levels`).  A non-finite parameter makes the face's vertices NaN, a non-finite
 *   basis entry its own vertex's.  The blend is rounded ONCE, from mu + I 2^e with I an integer: a zero blend is the exact +0, so
 *   a mu of -0.0 under all-zero coefficients gives +0.0 (the f32 chain's rule for the sign of a zero does not apply), and a sum
 *   below half the smallest subnormal gives a zero of the sum's sign (tests/test_decode_q30_edges_gpu.py).
 * It has its own basis image (fr_decode_q30_image_bytes, 256-byte aligned; 0 = shape not covered: n_shape + n_exp > 512,
 * for which fr_decode_q30_pack / fr_decode_3dmm_q30 return FR_ERR_UNSUPPORTED; the image does not depend on `levels`) and
 * needs a caller-owned staging workspace (fr_decode_q30_workspace_bytes: 68 KiB for the model's shape, 16-byte aligned) that
 * must not be shared by launches in flight on different streams.  fr_decode_3dmm_q30 is levels = 7 on dense [B,3,N] rows.
 * FR_Q30_SCHED (fr_set_option): 0 = 8 waves per CU, a wave owns a tile's four column blocks, 16-deep ring (default) | 1 = 16
 * waves per CU, a tile's two 32-column halves on neighbouring waves; no result bit depends on it (profiles/round5_probes/r5b:
 * what each measured, and the launch-free staging forms that were built and not kept). */
size_t fr_decode_q30_image_bytes(int N, int n_shape, int n_exp);
int fr_decode_q30_pack(const float* mu, const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp,
                       void* qimage, size_t qimage_bytes, void* hip_stream);
size_t fr_decode_q30_workspace_bytes(int n_shape, int n_exp);
int fr_decode_3dmm_q30(const float* params, const void* qimage, const float* R_override, int B, int N, int n_shape,
                       int n_exp, float im_size, float* vertex_proj, void* workspace, size_t ws_bytes, void* hip_stream);
int fr_decode_3dmm_q30_lv(const float* params, const void* qimage, const float* R_override, int B, int N, int n_shape,
                          int n_exp, float im_size, int levels, float* vertex_proj, void* workspace, size_t ws_bytes,
                          void* hip_stream);
/* fr_decode_render_forward with the Q30 decode (same phases, same pitched vertex hand-off, same render workspace; q_workspace =
 * the decode's staging buffer, one per stream in flight). */
int fr_decode_render_forward_q30(const float* params, const void* qimage, const float* R_override, const float* tri,
                                 const float* texture, int B, int N, int n_shape, int n_exp, int ntri, int H, int W,
                                 int tex_batch, float im_size, int levels, float* vertex_handoff, size_t vertex_bytes,
                                 float* depth, float* tex_img, float* normal, float* tri_ind, void* workspace, size_t ws_bytes,
                                 void* q_workspace, size_t q_ws_bytes, void* hip_stream, int phases);

/* ---- 3DMM decode backward (the gradient TF autodiff derives from nets/network.py:140-171) ------------
 *   grad_vertex_proj [B,3,N] = dL/d vertex_proj;  vertex_proj [B,3,N] = the forward output (used for d f);
 *   mu / pc_shape / pc_exp in the reference layouts (not the packed image);  grad_params [B, 7+n_shape+n_exp].
 * d alpha = pc_shape^T dv, d beta = pc_exp^T dv with dv = (f R)^T dq, dq = (g_x, -g_y, g_z); d t3d = sum_p dq;
 * d f = sum_p (R v_p) . dq evaluated as sum_p (q - t3d) . dq / f, which needs no second pass over the basis; the three
 * angles get 0: in the reference R passes through tf.py_func (network.py:150), which has no gradient.  (That is the default and
 * stays so; fr_decode_pose_backward below adds the angle gradients and dL/dR for a caller that asks for them.)
 * f == 0 (only reachable when set_constraints' sigmoid underflows, raw input < -103): every vertex projects onto t3d, the
 * quotient form is 0/0 and d f is DEFINED as 0 here (the true value sum_p (R v_p) . dq would need the un-projected
 * vertices, i.e. another basis pass); d alpha = d beta = 0 and d t3d are exact in that case.  Stated, tested
 * (tests/test_decode_backward_gpu.py::test_zero_focal_column), not silent.
 * Deterministic (fixed-order partial sums, no float atomics). */
size_t fr_decode_backward_workspace_bytes(int B, int N, int n_shape, int n_exp);

int fr_decode_3dmm_backward(const float* grad_vertex_proj, const float* params, const float* vertex_proj,
                            const float* pc_shape, const float* pc_exp, const float* R_override, int B, int N,
                            int n_shape, int n_exp, float im_size, float* grad_params, void* workspace, size_t ws_bytes,
                            void* hip_stream);

/* The same gradient from a packed basis image, in ONE fused kernel + the fixed-order reduction (round 4).
 * fr_decode_3dmm_backward above reads pc_shape / pc_exp in their reference layouts (no extra memory) and runs three
 * launches: a prepass that writes the 41 MB of dv rows, the reduction over the vertices, the slab sum (70 us of GEMM at 64
 * faces against a 33 us matrix-pipe floor).  A caller that takes gradients every step packs the basis ONCE --
 * fr_decode_backward_basis_bytes(N, n_shape, n_exp) bytes (the size of the forward image), 16-byte aligned: MFMA A-fragment
 * order, [vertex group of 16][x / y / z rows][16-coefficient block][lane] float4 -- and calls the packed entry point: one
 * workgroup per CU turns a 16-vertex tile of the incoming gradient into the three dv row blocks in LDS (and the d t3d / d f
 * partial sums in registers) and multiplies them against the group's basis fragments (counted-wait register ring); dv never
 * reaches global memory.  rocprofv3 at 64 faces: 27.6 + 59.4 + 16.7 us (round 3) -> 70.1 + 6.9 us.  Same workspace
 * (fr_decode_backward_workspace_bytes), same definition of every output, deterministic (bit-reproducible for a given
 * FR_BWD_CHUNKS); the two entry points sum their partial results in different (each fixed) orders, so they agree to rounding,
 * not bit for bit.
 * fr_decode_backward_basis_bytes answers 0 -- and the pack / packed entry points FR_ERR_UNSUPPORTED -- for what the fused kernel
 * does not serve: more than 256 coefficients, or a mesh of fewer than 16 vertices (its tile loads are sixteen floats wide); use
 * fr_decode_3dmm_backward there. */
size_t fr_decode_backward_basis_bytes(int N, int n_shape, int n_exp);
int fr_decode_backward_pack_basis(const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp, void* packed_t,
                                  size_t packed_bytes, void* hip_stream);
int fr_decode_3dmm_backward_packed(const float* grad_vertex_proj, const float* params, const float* vertex_proj,
                                   const void* packed_t, const float* R_override, int B, int N, int n_shape, int n_exp,
                                   float im_size, float* grad_params, void* workspace, size_t ws_bytes, void* hip_stream);

/* The same fused backward WITHOUT the forward output (round 5).  d f = sum_p (R v_p) . dq needs the un-projected vertices; the
 * entry points above recover R v_p from vertex_proj ((q - t3d) / f: 41 MB more to read per 64 faces, and the caller must keep
 * the forward's output alive for the backward).  With v = mu + S alpha + E beta and dv = (f R)^T dq,
 *     sum_p (R v_p) . dq  =  sum_p v_p . dv_p / f  =  ( sum_p mu_p . dv_p  +  alpha . d alpha  +  beta . d beta ) / f,
 * whose first term the fused kernel forms from the 0.64 MB of mu beside the dv rows it builds anyway and whose other two are dot
 * products of the parameters with the coefficient gradients: linear, so every workgroup adds the product with ITS partial
 * gradients to its partial of d f and the fixed-order reduction sums them like every other output -- two launches, as before.
 * What it buys is MEMORY, not time: measured in one process (tools/bwd_ab_probe.py) 71.3 against 71.1 us per backward at 64 faces
 * and 56.3 against 53.2 at 32 -- the 41 MB of vertex_proj stream in for free beside the 153 MB of basis.
 * mu [3N] in the reference layout (16-byte aligned); every other output as fr_decode_3dmm_backward_packed; d f := 0 at f == 0 as
 * there; deterministic.  The three entry points agree to rounding.  FR_ERR_UNSUPPORTED where fr_decode_backward_basis_bytes is 0. */
int fr_decode_3dmm_backward_packed_mu(const float* grad_vertex_proj, const float* params, const float* mu, const void* packed_t,
                                      const float* R_override, int B, int N, int n_shape, int n_exp, float im_size,
                                      float* grad_params, void* workspace, size_t ws_bytes, void* hip_stream);

/* ---- differentiable decode -> rendering-layer step (the CoarseNet loop: nets/network.py:140-171 -> :174-201, five times per
 * training step, nets/coarse_net.py) ---------------------------------------------------------------------------------------
 * FORWARD.  fr_decode_render_forward with the fused resolver of fr_rendering_layer_forward: same decode and pose arguments, same
 * pitched vertex hand-off, same render workspace, same `phases` word (8 = decode, 4 = pack the triangle list, 1 = emit, 2 = the
 * fused resolve, plus FR_PHASES_STRIP_ROWS); it takes im_gray [B,H,W,1] and writes net_input [B,H,W,7], depth_img, depth and
 * tri_ind exactly as fr_rendering_layer_forward defines them -- bit-identical to fr_decode_3dmm followed by
 * fr_rendering_layer_forward, without the dense [B,3,N] tensor between them.  The f32 chain only (no Q30 variant).
 * FR_ERR_UNSUPPORTED wherever fr_rendering_layer_forward answers it (shapes only the fallback rasteriser covers,
 * FR_RENDER_IMPL = scan, no triangles / vertices), decided before anything is launched. */
int fr_decode_rendering_layer_forward(const float* params, const void* packed_basis, const float* R_override, const float* tri,
                                      const float* texture, const float* im_gray, int B, int N, int n_shape, int n_exp, int ntri,
                                      int H, int W, int tex_batch, float im_size, float* vertex_handoff, size_t vertex_bytes,
                                      float* net_input, float* depth_img, float* depth, float* tri_ind, void* workspace,
                                      size_t ws_bytes, void* hip_stream, int phases);

/* BACKWARD.  Pixel gradients -> grad_params [B, 7+n_shape+n_exp] in one call: four launches, no [B,3,N]-sized tensor.
 * Every vertex gradient of this model comes through the depth plane, so only the z row of d L / d vertex_proj is non-zero
 * (render_depth_op.cc:359-363): the composed chain writes 2/3 of that tensor as zeros and reads them back.  Here
 *   1. the records pass of the render backward FORMS the pixel gradient, per pixel, in fp32 without contraction, absent
 *      planes skipped (not added as zero):
 *          g = +0
 *          g_net_input given:  g = g + (g_net_input[..,0] * im_gray) * m1,   m1 = (1e-6f <= depth && depth <= 1.0f) ? 1.0f : 0.0f
 *          g_depth_img given:  g = g + g_depth_img * m2,                       m2 = (depth >= 1e-6f) ? 1.0f : 0.0f
 *          g_depth given:      g = g + g_depth
 *      -- the torch expression of _RenderingLayerFused.backward.  The thresholds are fp32 compares against (float)1e-6 and 1.0f:
 *      that is what torch does with a Python scalar beside a float32 tensor (the scalar is cast to the tensor's type; checked on
 *      the values 1e-6f, 1.0f and their 1-ulp neighbours, tests/test_decode_layer_gpu.py).  The masks are multiplied in, so an
 *      infinite gradient on a masked pixel gives NaN, as there;
 *   2. the owner kernel of fr_render_depth_backward_ws writes ONLY a pitched z plane [B, pitch], pitch =
 *      fr_decode_render_vertex_pitch(N): same fixed-point sums, same max|g| predicate over covered pixels, same Inf/NaN path;
 *   3. a z-only fused decode backward (bwd_fused_z_kernel: one 16-byte load of g_z plus the three mu rows per staging thread
 *      instead of six loads) and the fixed-order reduction give grad_params = fr_decode_3dmm_backward_packed_mu for
 *      grad_vertex_proj = (0, 0, z) -- the same expressions with +0 / -0 for the absent rows.
 * For finite inputs the result is BIT-IDENTICAL to: that torch expression -> fr_render_depth_backward_ws ->
 * fr_decode_3dmm_backward_packed_mu (same FR_BWD_CHUNKS / FR_BWD_CB dependence, deterministic).
 *   g_depth / g_depth_img [B,H,W,1], g_net_input [B,H,W,7] (channel 0 read): each may be NULL, all three NULL is
 *   FR_ERR_INVALID_ARG;  im_gray, depth [B,H,W,1]: required when g_depth_img or g_net_input is given;  tri [3,ntri], tri_ind: as
 *   fr_render_depth_backward;  params, mu (16-byte aligned), packed_t (fr_decode_backward_pack_basis), R_override (NULL or
 *   [B,3,3]), im_size: as fr_decode_3dmm_backward_packed_mu.
 * `workspace`: fr_decode_render_backward_workspace_bytes(B, N, n_shape, n_exp, H, W) bytes, 256-byte aligned, caller-owned: the
 * per-pixel records and chunk partials, the z plane, the decode backward's slabs.  Too small or misaligned is FR_ERR_WORKSPACE
 * (no fallback).  The size is 0 -- and the call FR_ERR_UNSUPPORTED -- where fr_decode_backward_basis_bytes is 0.  grad_params is
 * fully written on every FR_OK; nothing is synchronised or allocated; reentrant under the rules at the top of this file (the
 * workspace is per call in flight). */
size_t fr_decode_render_backward_workspace_bytes(int B, int N, int n_shape, int n_exp, int H, int W);
int fr_decode_render_backward(const float* g_depth, const float* g_depth_img, const float* g_net_input, const float* im_gray,
                              const float* depth, const float* tri, const float* tri_ind, const float* params, const float* mu,
                              const void* packed_t, const float* R_override, int B, int N, int n_shape, int n_exp, int ntri,
                              int H, int W, float im_size, float* grad_params, void* workspace, size_t ws_bytes,
                              void* hip_stream);

/* ---- pose gradients: dL/dR and the three angles (opt-in; SURVEY.md 8f rank 2, "d pose incl. dR/d angles") ------------------
 * Every entry point above gives the three angles 0 (the reference's rotation passes through tf.py_func, network.py:150) and
 * nothing for R_override: that stays their definition.  These two calls ADD the missing gradient, from the forward's vertices.
 * In the notation above -- dq = (g_x, -g_y, g_z); q - t formed as the decode backward forms it, q0 = out_x - tx,
 * q1 = ((im_size - 1) - out_y) - ty, q2 = out_z - tz; R the fp32 rotation the forward used (evaluated in-kernel, or R_override);
 * q - t = f R v:
 *   pose moment  A[i][k] = sum_p dq_i,p (q_k,p - t_k)                     (nine sums per face; trace(A) / f is d f)
 *   grad_R       G = dL/dR = f sum_p dq_p v_p^T = A R^-T = A cof(R) / det(R)   [B,3,3]
 *                (cof(R) = R for a rotation; the cofactor form is right for ANY invertible R_override, where A R is not)
 *   angles       d phi = <G, R_pitch' R_yaw R_roll>, d gamma = <G, R_pitch R_yaw' R_roll>, d theta = <G, R_pitch R_yaw R_roll'>
 *                (the matrices of network.py:276-290 and their elementwise derivatives), ONLY with R_override == NULL; with
 *                R_override the angles do not enter the forward and columns 0-2 are written as exactly 0: the caller chains grad_R.
 * f == 0 gives A = 0 and G = 0, the true value.  det(R) == 0 (a singular R_override) is DEFINED as G = 0 and angle gradients 0
 * (tests/test_pose_backward_gpu.py).  The moment is a streaming reduction with a fixed association (chunks of 2,048 vertices, a
 * constant: the bits depend on N alone, not on B or the part), chunk records summed in float64, G and the angle derivatives
 * formed in float64 and rounded ONCE to fp32; no float atomics: bit-reproducible.  It needs the forward's vertices (there is no
 * mu form: the cross terms pc_j^T dv_i are never formed).
 *
 * fr_decode_pose_backward: enqueue AFTER any of fr_decode_3dmm_backward{,_packed,_packed_mu} on the same stream: it completes
 * their grad_params.  grad_vertex_proj, vertex_proj [B,3,N] (any N >= 1, rows at any 4-byte phase; no basis is read, so it
 * also completes the reference-layout entry point for bases above 256 coefficients); grad_params [B, 7+n_shape+n_exp] or NULL:
 * ONLY columns 0-2 of each row are written; grad_R [B,3,3] or NULL; both NULL is FR_ERR_INVALID_ARG.  `workspace`:
 * fr_decode_pose_backward_workspace_bytes(B, N) bytes (0 for B <= 0 or N <= 0), 16-byte aligned; too small or misaligned is
 * FR_ERR_WORKSPACE.  Every check runs before any HIP call; B == 0 is FR_OK; nothing is allocated or synchronised; reentrant
 * under the rules at the top of this file with a workspace per call in flight.
 * Measured on an MI355X (tools/pose_grad_probe.py, profiles/decode_pose_backward.json; same process, device events, medians): behind
 * fr_decode_3dmm_backward_packed this call adds 21.5 us at 64 faces (71.5 -> 92.9) and 16.5 us at 32 (53.7 -> 70.2);
 * fr_decode_render_backward_pose costs 20.0 us more than fr_decode_render_backward at 64 faces (120.1 -> 140.1) and 16.5 us at 32
 * (82.2 -> 98.7).  The moment kernel must move 2 x 40.9 MB dense, 13.7 + 41.2 MB z-only at 64 faces (13.0 / 8.7 us at the 6.29 TB/s
 * measured-copy rate) and takes 14.6 / 10.6 us (rocprofv3 --kernel-trace); the finish kernel, one thread per face, takes 8.7 us:
 * that and the two launches are the rest of the difference. */
size_t fr_decode_pose_backward_workspace_bytes(int B, int N);
int fr_decode_pose_backward(const float* grad_vertex_proj, const float* vertex_proj, const float* params,
                            const float* R_override, int B, int N, int n_shape, int n_exp, float im_size, float* grad_params,
                            float* grad_R, void* workspace, size_t ws_bytes, void* hip_stream);

/* fr_decode_render_backward + the z-only pose moment over its own z plane and the forward's hand-off, in ONE call: every
 * argument of fr_decode_render_backward, then the pitched vertex hand-off the forward wrote (fr_decode_rendering_layer_forward /
 * fr_decode_render_forward: [B,3,pitch], fr_decode_render_vertex_bytes(B, N) bytes, 128-byte aligned; missing, too small or
 * misaligned is FR_ERR_WORKSPACE) and grad_R [B,3,3] or NULL.  Columns 3.. of grad_params are bit-identical to
 * fr_decode_render_backward; columns 0-2 hold the angle gradients (zeros under R_override).  dq0 = +0, dq1 = -0 as in the z-only
 * decode backward: for finite inputs grad_R and the angle columns are bit-identical to fr_decode_pose_backward fed (0, 0, z).
 * `workspace`: fr_decode_render_backward_pose_workspace_bytes bytes, 256-byte aligned.  FR_ERR_UNSUPPORTED (and size 0) exactly
 * where fr_decode_render_backward answers it. */
size_t fr_decode_render_backward_pose_workspace_bytes(int B, int N, int n_shape, int n_exp, int H, int W);
int fr_decode_render_backward_pose(const float* g_depth, const float* g_depth_img, const float* g_net_input,
                                   const float* im_gray, const float* depth, const float* tri, const float* tri_ind,
                                   const float* params, const float* mu, const void* packed_t, const float* R_override, int B,
                                   int N, int n_shape, int n_exp, int ntri, int H, int W, float im_size, float* grad_params,
                                   void* workspace, size_t ws_bytes, void* hip_stream, const float* vertex_handoff,
                                   size_t vertex_bytes, float* grad_R);

/* ---- normal-map gradients: the render backward fills x, y and z (opt-in) ------------------------------------------------------
 * fr_render_depth_backward gives the x and y rows zeros and never reads a gradient of `normal` (render_depth_op.cc:359-363): that
 * stays its definition.  This call ADDS the gradient of the op's `normal` plane (mode 0, raw) or of the normalised map that
 * post_normal / FaceRecNet.rendering_layer makes of it (mode 1, post) with respect to the three vertices of each pixel's winning
 * triangle.  tri_ind is held fixed (no coverage gradient) and the fp32 roundings of the forward are treated as the identity.
 * Per pixel whose tri_ind names t = (p1, p2, p3) -- 0 <= tri_ind < ntri and all three ids inside [0, nver), else nothing:
 *   a = fl32(P1 - P2), b = fl32(P1 - P3) (fp32 differences, as the forward); G = normal_grad widened to double; in double, each
 *   operation rounded on its own:
 *     da = b x G = (by Gz - bz Gy, bz Gx - bx Gz, bx Gy - by Gx)      db = G x a = (Gy az - Gz ay, Gz ax - Gx az, Gx ay - Gy ax)
 *     term(p1) = fl32(da + db)   term(p2) = fl32(-da)   term(p3) = fl32(-db)          (nine fp32 terms per pixel)
 *   mode 1: n = the forward's fp32 normal fl32(a x b); s = (n.z < 0) ? -1 : 1; m = s n; mag32 = (mx mx + my my) + mz mz in fp32
 *     (post_normal's value: the backward takes the forward's branch); r = sqrt(m.m), d = r + (double)1e-6f;
 *     mag32 > 1e-6f:  Gm = g'/d - m (g'.m) / (d d r);   else  Gm = g' / (1.0 + (double)1e-6f);   G = s Gm, then as mode 0.
 *     (the double sqrt / divide sequences are not pinned: a post-mode term may differ from this text by one fp32 ulp)
 * Each (face, row, vertex) sum of terms is formed as fr_render_depth_backward forms its own: the terms as 64-bit fixed-point
 * integers on a grid of 2^(e - 39 + shift), e = floor(log2 M), M the face's largest finite |term| over all three rows, shift as
 * above 2^20 pixels; integer addition in LDS by per-face owner workgroups; one rounding to fp32.  No float atomics, bit-
 * reproducible, independent of the launch geometry; |result - exact sum| <= 2^-24 |sum| + n 2^(shift - 39) M for n terms.  A face
 * with a non-finite term takes fp32 LDS atomics: the vertices that receive such a term come out non-finite, the others finite.
 *   normal_grad: three floats per pixel, grad_stride (>= 3) floats between pixels: 3 for a dense [B,H,W,3] plane, 7 with the
 *                pointer advanced by 4 for the normal channels of a [B,H,W,7] net_input gradient.
 *   vertex:      [B,3,vertex_pitch] rows (vertex_pitch >= nver: nver for the dense tensor, fr_decode_render_vertex_pitch(N) for
 *                the hand-off);  tri [3,ntri], tri_ind [B,H,W,1]: as fr_render_depth_backward.
 *   vertex_grad: dense [B,3,nver].  accumulate 0: all three rows of every vertex are written.  accumulate 1: each element becomes
 *                fl32(old + new), one add -- enqueued after fr_render_depth_backward(_ws) on the same stream it completes that
 *                tensor, and the depth part's bits survive wherever the normal part is zero.
 *   workspace:   fr_render_normal_backward_workspace_bytes(B, nver, H, W) bytes (48 per pixel + 8 per 1,024-pixel chunk; 0 for
 *                an empty shape), 16-byte aligned, caller-owned, per call in flight.
 * Every check runs before any HIP call: a negative size, mode outside {0, 1}, accumulate outside {0, 1}, grad_stride < 3 or
 * vertex_pitch < nver is FR_ERR_INVALID_ARG; then B == 0 (or nver == 0) is FR_OK; a NULL vertex_grad -- or, where pixels and
 * triangles exist, a NULL normal_grad / vertex / tri / tri_ind -- is FR_ERR_INVALID_ARG; a workspace that is missing, too small or
 * misaligned is FR_ERR_WORKSPACE (there is no variant without one).  Nothing is allocated or synchronised; reentrant under the
 * rules at the top of this file.
 * Time: tools/normal_grad_probe.py (profiles/render_normal_backward.json) measures this call beside fr_render_depth_backward_ws at 64
 * and 32 faces of the full mesh at 200 x 200 and the bytes it must move.  MI355X, medians of 6 rounds of 40 calls: raw mode 76.0 /
 * 44.0 us, post mode at stride 7 with accumulate 92.8 / 51.8 us, fr_render_depth_backward_ws on the same inputs 34.5 / 26.4 us, the
 * two in a row 140.7 / 75.9 us.  Must move 120 / 60 MB = 19.1 / 9.5 us at the 6.29 TB/s copy rate (0.25 / 0.22 of it in raw mode); the
 * rest goes to the call's own records and to the id plane that each of a face's 8 owners streams. */
size_t fr_render_normal_backward_workspace_bytes(int B, int nver, int H, int W);
int fr_render_normal_backward(const float* normal_grad, int grad_stride, const float* vertex, int vertex_pitch,
                              const float* tri, const float* tri_ind, float* vertex_grad, int B, int nver, int ntri,
                              int H, int W, int mode, int accumulate, void* workspace, size_t ws_bytes, void* hip_stream);

/* The normal-backward launch geometry (no GPU needed; the launcher reads the same function): out[6] = {owner workgroups per
 * face, vertices per owner (three 64-bit accumulators each), shift, 1,024-pixel record chunks, dynamic LDS bytes of an owner
 * workgroup, 1 if the block -> (face, owner) map keeps a face's owners on one XCD (batch a multiple of 8) else 0}; all zero for a
 * shape that launches no kernel.  Used by tests/test_normal_backward_cpu.py and tests/test_normal_backward_gpu.py. */
void fr_debug_render_normal_bwd_geom(int B, int nver, int H, int W, int* out);

/* ---- texture gradients: tex_img backward down to the texture (opt-in) ----------------------------------------------------------
 * fr_render_depth_backward never reads a gradient of `tex_img`: the reference's op has none, and its "LSE for alpha" block
 * (nets/network.py:436-445) gives up on "inversely transforming the diff into (3N, 1, B) space".  That inverse transform is the
 * adjoint of the rasteriser's texture lookup, and this call is it.  tri_ind is held fixed; every default stays the reference's.
 * The forward gives a pixel tritex_c = (t_c[p1] + t_c[p2] + t_c[p3]) / 3.0f in fp32.
 * Which pixels contribute.  A pixel is COUNTED when 0 <= (int)tri_ind < ntri (the x86 conversion of the other backwards: NaN and
 * out-of-range floats become INT_MIN).  A counted pixel CONTRIBUTES when all three ids (int)tri[k,t] lie in [0, nver).  A
 * contributing pixel has three terms term_c = fl32(g_c / 3.0f), c = 0..2, by the forward's own division sequence; every one of the
 * triangle's three vertices receives term_c in row c (a triangle that names one vertex three times gives it three terms).
 * Scale and sum, per scope.  A SCOPE is one face when tex_batch == B, the whole batch when tex_batch == 1 (B == 1: the same thing).
 *   m     = the largest finite |term| among the scope's contributing pixels, all three channels, as fp32 bits;  e = (m >> 23) - 127
 *   shift = the smallest s >= 0 with 2^(20+s) >= the scope's pixel count (H*W, or B*H*W for the shared texture)
 *   q     = rint(term * 2^(39 - shift - e)) as int64 (the product is exact in double; ties to even)
 *   S     = sum of q per (scope, row, vertex): integer addition, any order;   r = fp32(S), one rounding
 *   out   = fp32(double(r) * 2^(e - 39 + shift))
 * |q| < 2^(40 - shift) and an element receives at most 3 * 2^(20+shift) terms, so |S| < 2^62.  An element that receives no term is
 * +0.  accumulate 1 makes each element fl32(old + out), one add.  |out - exact sum| <= 2^-24 |sum| + n 2^(shift - 39) M for n terms,
 * M = the scope's largest |term| (plus one rounding to the subnormal grid where out is subnormal).
 * No float atomics on the finite path; bit-reproducible; independent of the launch geometry; with tex_batch == 1 independent of how
 * the faces are grouped (and of their order in the batch).
 * Non-finite terms.  A scope with a non-finite term does not have predictable bits.  An element that receives such a term comes out
 * non-finite: NaN if a NaN arrives or Infs of both signs arrive, otherwise the Inf.  Every other element of the scope is finite and
 * within 2^-23 A of the float64 sum of its terms, A = sum |term| over that element (float64 LDS atomics, one rounding to fp32).
 *   tex_grad:     three floats per pixel, grad_stride (>= 3) floats between pixels: 3 for a dense [B,H,W,3] plane, 7 with the
 *                 pointer advanced by 1 for channels 1-3 of a [B,H,W,7] net_input gradient.
 *   tri [3,ntri], tri_ind [B,H,W,1]: as fr_render_depth_backward.
 *   texture_grad: dense [tex_batch,3,nver]; tex_batch is 1 (the texture shared by the batch) or B.
 *   workspace:    fr_render_texture_backward_workspace_bytes(B, nver, H, W, tex_batch) bytes: 24 per pixel + 8 per 1,024-pixel
 *                 chunk (rounded up to 16), and for a shared texture of more than one face 24 nver per face slice; 0 for an empty
 *                 shape or a tex_batch that is neither 1 nor B.  16-byte aligned, caller-owned, per call in flight.
 * Every check runs before any HIP call: a negative size, tex_batch outside {1, B} (for B > 0), accumulate outside {0, 1} or
 * grad_stride < 3 is FR_ERR_INVALID_ARG; then B == 0 or nver == 0 is FR_OK; then a NULL texture_grad -- or, where pixels and
 * triangles exist, a NULL tex_grad / tri / tri_ind -- is FR_ERR_INVALID_ARG; more than 2^31 - 1 pixels per face (or 2^24 triangles
 * and more) is FR_ERR_UNSUPPORTED; where pixels and triangles exist a workspace that is missing, too small or not 16-byte aligned
 * is FR_ERR_WORKSPACE.  H*W == 0 or ntri == 0 writes zeros (accumulate: leaves the tensor as it is).  Nothing is allocated or
 * synchronised; the call can be captured in a graph; reentrant under the rules at the top of this file, one workspace per call in
 * flight.
 * Kernels (csrc/fr_render_tbwd.hip on the shared scheme of csrc/fr_owner_scatter.h): a records pass (triangle -> ids once, a 16-byte
 * {p1,p2,p3,term0} plane and an 8-byte {term1,term2} plane, {max, non-finite} per chunk), then owner workgroups with three 64-bit
 * LDS accumulators per owned vertex that stream the id plane.  tex_batch == B: one owner per (face, vertex range) rounds and writes.
 * tex_batch == 1: owners are (face slice, vertex range), each stores its raw int64 slab [3][range] in the workspace with plain
 * stores and a finish kernel adds a vertex's slabs and rounds once.  Sized before it was built: at 64 faces of the
 * full mesh 32 slices of 2 faces x 8 ranges keep one workgroup per CU; their slabs are 32 x 1.28 MB written and read once, against
 * 61 MB of records -- the alternative, 64-bit integer global atomics into one [3][nver] array, has no published rate on this chip
 * and was not built.
 * Time: tools/texture_grad_probe.py (profiles/render_texture_backward.json) measures this call in both modes beside
 * fr_render_depth_backward_ws at 64 and 32 faces of the full mesh at 200 x 200 and the bytes it must move.  MI355X, medians of 6 rounds of 40 calls: tex_batch == B 59.6 / 33.9 us,
 * tex_batch == 1 62.6 / 45.1 us (32 / 32 face slices x 8 ranges), fr_render_depth_backward_ws on the same inputs 34.5 / 26.0 us.  Must move 91 / 46 MB
 * (per face) and 51 / 26 MB (shared) = 14.5 / 7.3 and 8.1 / 4.1 us at the 6.29 TB/s copy rate (0.24 / 0.21 and 0.13 / 0.09 of it); the rest goes to
 * the call's own records, the id plane every owner streams and, for the shared texture, 82 / 82 MB of slabs.  The SfS
 * backward writing grad_normal_new takes 10.8 / 6.2 us without and 17.1 / 9.6 us with the albedo output. */
size_t fr_render_texture_backward_workspace_bytes(int B, int nver, int H, int W, int tex_batch);
int fr_render_texture_backward(const float* tex_grad, int grad_stride, const float* tri, const float* tri_ind,
                               float* texture_grad, int B, int nver, int ntri, int H, int W, int tex_batch, int accumulate,
                               void* workspace, size_t ws_bytes, void* hip_stream);

/* The texture-backward launch geometry (no GPU needed; the launcher reads the same function): out[7] = {owner workgroups per face
 * (tex_batch == B) or per face slice (shared texture), vertices per owner (three 64-bit accumulators each), shift, 1,024-pixel
 * record chunks per face, dynamic LDS bytes of an owner workgroup, 1 if the block -> (face or slice, owner) map keeps a group's
 * owners on one XCD (a group count that is a multiple of 8) else 0, face slices of the shared texture (0 where each face is its own
 * scope, B == 1 included: no cross-face reduction, no finish kernel)}; all zero for a shape that launches no kernel or is refused.
 * Used by tests/test_texture_backward_cpu.py and tests/test_texture_backward_gpu.py. */
void fr_debug_render_texture_bwd_geom(int B, int nver, int H, int W, int tex_batch, int* out);

/* ---- shape-from-shading term: fused lighting solve with a normal backward (opt-in) ---------------------------------------------
 * Replaces the linear algebra of get_spherical_harmonics_model (nets/network.py:424-460) on already rendered maps: four transposes,
 * a batched matmul, np.linalg.pinv through tf.py_func on H*W 3x3 matrices (:431), two more matmuls and a transpose back.  One
 * streaming pass per direction; the backward hands fr_render_normal_backward the gradient of the normalised normal map.
 *   abedo, im_gray, abedo_new, intensity, grad_intensity  [B,H,W,1];   normal, normal_new, grad_normal, grad_normal_new  [B,H,W,3]
 *   dense fp32; normal_new may be the same pointer as normal.  Written a_b, I_b, a'_b, n_b, n'_b below (face b, one pixel).
 * FORWARD, per pixel.  All arithmetic in float64 on the widened fp32 inputs, every operation rounded on its own (no contraction):
 *   u_b = I_b / (a_b + 1.0)
 *   M = sum_b n_b n_b^T   (six sums: xx, xy, xz, yy, yz, zz)        r = sum_b n_b u_b   (three sums; the term is n times u)
 *   P = pinv(M) through the symmetric eigendecomposition M = V diag(lambda) V^T: eigenvalue i is KEPT iff
 *       lambda_i > rcond * lambda_max  and  lambda_i > 0;   P = sum over the kept i of (v_i v_i^T) * (1 / lambda_i);
 *       M = 0 gives P = 0 and rank 0.  The eigensolver is cyclic Jacobi with a FIXED count of six sweeps (csrc/fr_sfs_pinv.h, one
 *       __host__ __device__ function; four reach the float64 floor): no data-dependent loop anywhere.
 *   l = P r, row by row as (P_i0 r_0 + P_i1 r_1) + P_i2 r_2
 *   intensity_b = fl32( a'_b * ((l_x n'_bx + l_y n'_by) + l_z n'_bz) )
 * -- (M^+ Y) rhs^T of network.py:433, associated as M^+ (Y rhs^T).
 * Association of the sums over b: a function of B ALONE -- not of H, W, the pixel's position or any option.  S = min(4, max(1,
 * B / 4)) slices (integer division); slice s owns the faces [s C, min(B, (s + 1) C)), C = ceil(B / S), and adds their terms in
 * ascending b onto +0.0; the slices are then added in ascending s onto slice 0's sum: ((s0 + s1) + s2) + s3.  No float atomics;
 * bit-reproducible.
 * Non-finite inputs.  If any of the six sums of M is NaN or Inf, P is six NaNs and the rank is 0; if any of the three sums of r is,
 * l is three NaNs: every intensity of that pixel is then NaN, and no other pixel changes by a bit.  A NaN or Inf in a'_b or n'_b
 * alone reaches face b's own intensity through the ordinary IEEE operations above.  Nothing lengthens a loop.
 * STATE.  state[k H W + p] (doubles, p = the pixel's row-major index): k = 0..5 P as xx, xy, xz, yy, yz, zz; k = 6..8 l; k = 9 the
 * number of kept eigenvalues.  fr_sfs_state_bytes(H, W) = 10 planes of H * W doubles (0 for an empty image), 16-byte aligned,
 * caller-owned, one per call in flight; the forward writes all of it, the backward reads it.  The layout is public.
 * BACKWARD.  P is held constant (the autograd semantics of a detached pinv, and of the reference's tf.py_func).  With g_b = dL / d
 * intensity_b and w_b = g_b a'_b:
 *   q = sum_b w_b n'_b   (three sums, the forward's association)         s = P q   (rows as for l)
 *   grad_normal_b = fl32(u_b * s)   (three components)                   grad_normal_new_b = fl32(w_b * l)
 * Either output may be NULL (the other is bit-identical to the joint call); both NULL is FR_ERR_INVALID_ARG.  No gradient is formed
 * for abedo or im_gray: they are constants of this model.  A caller that passed one tensor as normal and normal_new adds the
 * two outputs.
 * fr_sfs_intensity_backward_tex (opt-in: the albedo coefficients as a fitted quantity) is the same call with one more output,
 *   grad_abedo_new_b = fl32( (double)g_b * d_b ),   d_b = (l_x n'_bx + l_y n'_by) + l_z n'_bz   -- the forward's own d,
 * float64 with l from state planes 6-8, each operation rounded on its own; [B,H,W,1].  Any of the three outputs may be NULL (the
 * others are bit-identical to fr_sfs_intensity_backward's); all three NULL is FR_ERR_INVALID_ARG.  fr_sfs_intensity_backward IS
 * this call with a NULL grad_abedo_new.  abedo (the render of the mean texture) and im_gray stay constants.
 * Checks, all before any HIP call: a negative size, or an rcond that is negative or not finite, is FR_ERR_INVALID_ARG; then B == 0
 * or an empty image is FR_OK; then a NULL input or output pointer (the backward: both outputs NULL) is FR_ERR_INVALID_ARG; a state
 * that is missing, too small or not 16-byte aligned is FR_ERR_WORKSPACE; more than 2^31 - 65 pixels is FR_ERR_UNSUPPORTED.  Nothing
 * is allocated or synchronised; reentrant under the rules at the top of this file with a state buffer per call in flight.
 * Kernels (csrc/fr_sfs.hip): a workgroup owns 64 consecutive pixels, one per lane, and S waves; wave s streams its slice's maps (per
 * face 768 contiguous bytes of a normal plane), the nine partial sums meet in LDS in the order above, wave 0 solves the 3 x 3 once
 * per pixel and broadcasts l through LDS for the shading pass.  200 x 200 gives 625 workgroups of 4 waves for the chip's 1,024 SIMDs.
 * Time: tools/sfs_probe.py (profiles/sfs_intensity.json) measures both directions beside the stock-torch route at 64 and 32 faces of
 * 200 x 200 and the bytes each must move. */
size_t fr_sfs_state_bytes(int H, int W);
int fr_sfs_intensity_forward(const float* abedo, const float* normal, const float* im_gray, const float* abedo_new,
                             const float* normal_new, int B, int H, int W, double rcond, float* intensity, void* state,
                             size_t state_bytes, void* hip_stream);
int fr_sfs_intensity_backward(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                              const float* normal_new, const void* state, size_t state_bytes, int B, int H, int W,
                              float* grad_normal, float* grad_normal_new, void* hip_stream);
int fr_sfs_intensity_backward_tex(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                                  const float* normal_new, const void* state, size_t state_bytes, int B, int H, int W,
                                  float* grad_normal, float* grad_normal_new, float* grad_abedo_new, void* hip_stream);

/* The SfS launch geometry (no GPU needed; the launchers read the same function): out[4] = {pixels per workgroup, batch slices per
 * pixel (S above), workgroups, dynamic LDS bytes of a forward workgroup}; all zero for an empty shape.  Used by
 * tests/test_sfs_cpu.py. */
void fr_debug_sfs_geom(int B, int H, int W, int* out);

/* HOST instantiation of the kernel's pseudo-inverse (no GPU): m6 -> p6, both xx, xy, xz, yy, yz, zz, *rank = kept eigenvalues.
 * FR_ERR_INVALID_ARG for a NULL pointer or an rcond that is negative or not finite.  Used by tests/test_sfs_cpu.py. */
int fr_debug_sfs_pinv(const double* m6, double rcond, double* p6, int* rank);

/* ---- shape-from-shading term across ranks: the same solve with the batch spread over several callers (opt-in) -------------------
 * The lighting solve couples the faces of a batch only through sums that are additive over faces: M and r in the forward (nine
 * sums), q in the backward (three).  These entry points cut the two passes above at that point, so that each of several callers
 * (data-parallel ranks, each with its own B faces of one H x W image grid) streams its own maps once, exchanges 9 + 3 float64 planes
 * per direction instead of its maps, and finishes with the totals.  The exchange itself is the caller's (an all-gather into one
 * tensor: utils/dist.py, all_gather_stack); nothing here communicates.  Inputs, outputs, u_b, w_b and the state are those of the
 * section above; the one-call entry points do not change.
 * PART.  A part is one caller's nine (or three) sums over its own B faces, formed exactly as the one-call kernel forms them for a
 * batch of that size: S = sfs_slices(B) slices, each adding its faces' terms in ascending b onto +0.0, then the slices added in
 * ascending s onto slice 0's sum.  fr_sfs_moments writes the part [9][H*W] doubles: Mxx, Mxy, Mxz, Myy, Myz, Mzz, rx, ry, rz;
 * fr_sfs_backward_q writes [3][H*W]: qx, qy, qz.  fr_sfs_moments_bytes(H, W) = 9 planes, fr_sfs_q_bytes(H, W) = 3 planes of H * W
 * doubles (0 for an empty image); the buffers are caller-owned and 16-byte aligned.
 * PART LAYOUT.  moment_parts is [nparts][9][H*W] doubles and q_parts is [nparts][3][H*W] doubles, both contiguous: what an
 * all-gather of the parts into one tensor produces.  Every caller passes the same stacked buffer, in the same order.
 * TOTALS.  total = ((part0 + part1) + part2) + ...  in ascending part index, per plane and pixel, float64, starting FROM part0 (not
 * from zero).  The bits are a function of the parts and their order, and of nothing else -- not of B, H, W or the caller.
 * Everything after the totals is the text of the section above: fr_sfs_pinv3 on the total M, the rows of l, the poison rule for
 * non-finite sums (applied to the totals), the ten state planes, intensity_b = fl32(a'_b (l . n'_b)) for the caller's own faces,
 * s = P q with the total q, and the three gradient outputs of fr_sfs_intensity_backward_tex for the caller's own faces.  Every
 * caller therefore holds the same state, bit for bit.
 * nparts == 1 is bit-identical to the one-call entry points: fr_sfs_moments then fr_sfs_solve_shade gives the state and intensity
 * of fr_sfs_intensity_forward; fr_sfs_backward_q then fr_sfs_backward_apply gives the outputs of fr_sfs_intensity_backward_tex.
 * GRADIENT ACROSS CALLERS.  grad_normal_b = fl32(u_b * (P sum_r q_r)) for the caller's own faces: the part of EVERY caller's loss
 * that passes through the shared lighting into this caller's normals.  With each caller's loss the mean over its own faces and the
 * callers' gradients averaged (data-parallel training), that is the single-process gradient of the mean loss over all faces.
 * grad_normal_new and grad_abedo_new are local.  P is held constant, as above.
 * EMPTY SHARDS.  A caller may own no faces.  With B == 0 and a non-empty image fr_sfs_moments and fr_sfs_backward_q write planes of
 * +0.0 (the caller still takes part in the exchange; the face pointers may then be NULL); fr_sfs_solve_shade and
 * fr_sfs_backward_apply with B == 0 are FR_OK and write nothing, the state included.  An empty image is FR_OK everywhere.
 * q_parts may be NULL exactly when grad_normal is NULL (it is not read then); all three outputs NULL is FR_ERR_INVALID_ARG.
 * Checks, all before any HIP call, in this order: a negative size is FR_ERR_INVALID_ARG; an rcond that is negative or not finite
 * is FR_ERR_INVALID_ARG; nparts < 1 or nparts > 4096 is FR_ERR_INVALID_ARG; then the empty cases above are FR_OK; then a NULL
 * input, parts or output pointer is FR_ERR_INVALID_ARG; a moments, q or state buffer that is missing, too small or not 16-byte
 * aligned is FR_ERR_WORKSPACE; more than 2^31 - 65 pixels is FR_ERR_UNSUPPORTED.  The stacked parts carry no size: the caller
 * vouches for nparts * 9 (or 3) planes.  Nothing is allocated or synchronised; reentrant with buffers per call in flight.
 * Kernels (csrc/fr_sfs.hip), built from the device functions of the one-call kernels: sfs_moments_kernel and sfs_backward_q_kernel
 * are their streaming halves (a workgroup owns 64 consecutive pixels, S waves stream contiguous shares of the faces, the partial
 * sums meet in LDS, wave 0 stores the planes); sfs_solve_shade_kernel: wave 0 adds the parts, solves once per pixel and broadcasts
 * l through LDS, every wave shades its faces; sfs_backward_apply_kernel: every wave adds the q parts for itself (24 doubles per
 * pixel at 8 parts, from the workgroup's own L1 lines; no LDS, no barrier).  No atomics.
 * Bytes and time: per direction the split route moves the one-call route's maps plus 72 B per pixel and part written and read
 * (forward) or 24 B (backward), plus one launch; tools/sfs_probe.py --sharded measures it beside the one-call kernels
 * (profiles/sfs_sharded.json; the figures and their reading: DESIGN.md 4.4f). */
size_t fr_sfs_moments_bytes(int H, int W);
int fr_sfs_moments(const float* abedo, const float* normal, const float* im_gray, int B, int H, int W, void* moments,
                   size_t moments_bytes, void* hip_stream);
int fr_sfs_solve_shade(const void* moment_parts, int nparts, const float* abedo_new, const float* normal_new, int B, int H, int W,
                       double rcond, float* intensity, void* state, size_t state_bytes, void* hip_stream);
size_t fr_sfs_q_bytes(int H, int W);
int fr_sfs_backward_q(const float* grad_intensity, const float* abedo_new, const float* normal_new, int B, int H, int W, void* q,
                      size_t q_bytes, void* hip_stream);
int fr_sfs_backward_apply(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                          const float* normal_new, const void* state, size_t state_bytes, const void* q_parts, int nparts, int B,
                          int H, int W, float* grad_normal, float* grad_normal_new, float* grad_abedo_new, void* hip_stream);

/* The split route's launch geometry (no GPU needed; the four launchers read the same function): out[6] = {pixels per workgroup,
 * batch slices per pixel (S = sfs_slices(B); 1 for B == 0, which still launches the two part kernels), workgroups, dynamic LDS
 * bytes of the moments kernel (9 S 64 doubles), of the solve-and-shade kernel (3 x 64 doubles), of the q kernel (3 S 64 doubles)};
 * the apply kernel uses no LDS.  All zero for a negative B, an empty image or one the launchers refuse.  Used by
 * tests/test_sfs_sharded_cpu.py. */
void fr_debug_sfs_split_geom(int B, int H, int W, int* out);

/* ---- depth-map normals: the normal map of a depth map on the pixel grid, with a backward (opt-in) --------------------------------
 * The reference's shape-from-shading term shades the COARSE mesh's normals twice and says so (nets/network.py:451-453: "how to
 * inversely convert predicted fine depth into new vertices, in order to get new normals ??").  No conversion is needed: the fine
 * depth map lives on the pixel grid and so do its normals.  These entry points turn a depth map into a normal map in the renderer's
 * conventions, masked to the face and exact at the mask's edges, and carry a normal-map gradient back to the depth map; the
 * backward's input is what fr_sfs_intensity_backward hands out as grad_normal_new.
 *   depth, mask, grad_depth  [B,H,W,1];   normal, grad_normal  [B,H,W,3];   dense fp32.  Pixel (r, c) is row-major with x = column,
 *   y = row: the rasteriser's q = y * W + x.
 * MASK.  mask may be NULL: every pixel of the image is then valid.  Otherwise pixel p is valid iff mask[p] >= 0.0f -- the tri_ind
 * convention (background is -1; a NaN is invalid).  Positions outside the image are invalid.
 * FORWARD, per pixel.  All arithmetic in float64 on the widened fp32 inputs, every operation rounded on its own (no contraction).
 * An invalid p gives normal = (+0, +0, +0).  For a valid p = (r, c), with L = valid(r, c - 1), R = valid(r, c + 1) and z_L, z_R, z_p
 * the depths there:
 *   dx = (z_R - z_L) * 0.5   L and R (central)          dx = z_R - z_p   R only          dx = z_p - z_L   L only          dx = 0.0   neither
 *   dy likewise from the rows r - 1 (lo) and r + 1 (hi)
 *   s = sqrt((dx * dx + dy * dy) + 1.0)
 *   normal = ( fl32(-dx / s), fl32(-dy / s), fl32(1.0 / s) )
 * The sign is the renderer's: the larger depth wins the z-test, so the surface faces +z and its normal is (-dz/dx, -dz/dy, 1)
 * normalised, n_z > 0 -- compute_abedo_image's normalised map is the triangle normal flipped to z >= 0 (on a tessellated plane the
 * two agree to the render's own +1e-6 and fp32 roundings: tests/test_depth_normals_cpu.py).  An invalid pixel's depth is never
 * read, and a valid pixel's own depth enters a one-sided difference only.  A non-finite depth reaches only the pixels whose stencil
 * reads it, through the ordinary IEEE operations above; no other pixel changes by a bit.
 * BACKWARD.  g = grad_normal[p] widened; dx, dy, s recomputed as in the forward; n = (-dx / s, -dy / s, 1.0 / s) in float64, NOT
 * rounded to fp32.  Per valid pixel
 *   d = (g_x n_x + g_y n_y) + g_z n_z          e_x(p) = -((g_x - n_x d) / s)          e_y(p) = -((g_y - n_y d) / s)
 * (dL / d dx and dL / d dy).  The coefficients of dx on the depths it reads are the forward's: +-0.5 for a central difference, +-1
 * for a one-sided one, and on the pixel's own depth -1 ("R only"), +1 ("L only"), 0 otherwise.  For a valid p
 *   grad_depth[p] = fl32( ((((own_x + own_y) + from_left) + from_right) + from_up) + from_down )
 *   own_x      = -e_x(p) "R only", e_x(p) "L only", else +0.0;   own_y alike with e_y and the rows
 *   from_left  = c * e_x(left neighbour),  c = 0.5 if that neighbour's difference is central, 1 if one-sided (p is its R)
 *   from_right = -(c * e_x(right neighbour)),  c likewise (p is its L);   from_up, from_down: the same with e_y of (r - 1, c), (r + 1, c)
 * A term whose neighbour is invalid, and an own term whose coefficient is 0, is +0.0 -- never 0 times a value.  An invalid p gets
 * exactly +0.  A gather: no atomics, no workspace; each output is a function of its pixel's 13-point neighbourhood (mask, depth,
 * grad_normal) and of nothing else -- not of B, H, W, the pixel's position or the launch geometry.  Bit-reproducible.  No gradient
 * is formed for the mask.
 * Checks, all before any HIP call, in this order: a negative size is FR_ERR_INVALID_ARG; then B == 0 or an empty image is FR_OK;
 * then a NULL depth, output or grad_normal is FR_ERR_INVALID_ARG; more than 2^31 - 65 pixels per face is FR_ERR_UNSUPPORTED (as is
 * a grid the runtime does not take: more than 65,535 faces or 65,535 tile rows).  Nothing is allocated or synchronised; reentrant
 * under the rules at the top of this file.
 * Kernels (csrc/fr_depth_normals.hip): a workgroup owns a 32 x 16 pixel tile of one face, one lane per pixel; a wave covers two
 * 32-pixel row segments (2 x 384 contiguous bytes of a normal plane).  The forward reads its five-point stencil from global memory
 * (the workgroup's own L1 lines) and uses no LDS.  The backward STAGES e_x, e_y in LDS instead of recomputing them in their readers:
 * every lane evaluates its own pixel once, 96 lanes the halo (two columns for e_x, two rows for e_y), one barrier, then the gather
 * -- 1.19 evaluations per output instead of 5, 8,960 bytes of LDS.  200 x 200 x 64 faces is 5,824 workgroups of 8 waves.
 * Bytes and time: at 64 faces of 200 x 200 the forward must move 51 MB (depth 10 + mask 10 read, normal 31 written), the backward
 * 61 MB (31 + 10 + 10 read, 10 written); tools/depth_normals_probe.py (profiles/depth_normals.json) measures both beside the same
 * operator composed from stock torch ops. */
int fr_depth_normals_forward(const float* depth, const float* mask, int B, int H, int W, float* normal, void* hip_stream);
int fr_depth_normals_backward(const float* grad_normal, const float* depth, const float* mask, int B, int H, int W,
                              float* grad_depth, void* hip_stream);

/* The depth-normals launch geometry (no GPU needed; the launchers read the same function): out[6] = {tile width, tile height,
 * threads per workgroup, tiles across, tiles down, static LDS bytes of a backward workgroup}; the grid is tiles across x tiles
 * down x B.  All zero for an empty shape or one the launchers refuse.  Used by tests/ref_depth_normals.py to place its shapes on
 * the tile's edges and by tests/test_depth_normals_cpu.py. */
void fr_debug_depth_normals_geom(int B, int H, int W, int* out);

/* ---- Gram-form geometry loss: one pass of the basis at load time, none per step (opt-in) ------------------------------------------
 * The geometry loss (nets/network.py:347-355) is a quadratic form in K = n_shape + n_exp numbers per face,
 *   mean((U d)^2) = (1 / (3N B)) sum_b d_b^T (U^T U) d_b,      d / d d_b = (2 / (3N B)) (U^T U) d_b,      U = [pc_shape | pc_exp],
 * and U is a constant of the model, so G = U^T U is one too.  fr_geometry_gram_build forms it once, in float64; after that the
 * loss and its gradient are a Kp x Kp matrix against B short vectors: no basis traffic per step, no second packed image of the
 * basis, no [B,3,N] tensor kept for the backward.  Notation: Kp = K rounded up to a multiple of 16, rows = 3N.
 *   pc_shape [3N, n_shape], pc_exp [3N, n_exp]   the reference layouts (row strides of 199 and 29 floats: no alignment assumed);
 *                                                either may have 0 columns, its pointer is then not read
 *   gram   [Kp][Kp] float64, row-major, full storage;   diff, grad_diff  [B, K] fp32;   loss, grad_loss  one fp32 on the DEVICE
 * NAMES.  The stream parameter of these entry points is called `stream`, not `hip_stream` as everywhere above: tests/
 * test_capi_codes_cpu.py replays a fixture recorded from exactly the prototypes that have a parameter named hip_stream, and that
 * fixture is not re-recorded for an opt-in addition; tests/test_geometry_gram_cpu.py holds these entry points' return codes.
 * GRAM.  G[i][j] = sum_r U[r][i] U[r][j] in float64 on the widened fp32 entries (every product is exact).  The row axis is cut into
 * chunks of 1,024 rows -- a compile-time constant: no function of the device, of B or of a knob -- each chunk's partial comes from
 * v_mfma_f64_16x16x4_f64 accumulations over its rows in row order, and the chunk partials are added in chunk order from +0.0.  Only
 * i <= j is computed; the one value is written to G[i][j] and G[j][i], so G equals its transpose bit for bit.  Every element with
 * i >= K or j >= K is exactly +0, whatever the basis holds.  G's bits are a function of (N, n_shape, n_exp, the basis) alone: the
 * same run to run and device to device.  For a finite basis, |G[i][j] - exact| <= 3N 2^-53 sum_r |U[r][i] U[r][j]| (a sum of 3N
 * exact terms, at most 3N - 1 roundings of relative size 2^-53 in any association).  The workspace holds the chunk
 * partials and is free again when the build has run; neither buffer needs to be cleared.
 * LOSS.  Float64, every multiplication and every addition rounded on its own (no fma):
 *   d_j       = (double) diff[b][j]
 *   y[b][k]   = chain over j = 0 .. K-1 from +0.0:   y = y + G[j][k] * d_j
 *   q[b]      = chain over k = 0 .. K-1 from +0.0:   q = q + d_k * y[b][k]
 *   S         = chain over b = 0 .. B-1 from +0.0:   S = S + q[b]
 *   loss      = (float)( S / ((double)(3N) * (double)B) )
 *   grad_diff[b][k] = (float)( ((double)grad_loss[0] * (2.0 / ((double)(3N) * (double)B))) * y[b][k] )
 * (tests/ref_geometry_gram.py is this in numpy).  A non-finite diff entry makes that face's y row and the loss non-finite by the
 * IEEE rules and leaves every other face's gradient row untouched.  Under data parallelism each rank takes the mean over its own
 * faces, as it does with the product form: no collective.
 * STATE.  `state` is caller-owned, 16-byte aligned, fr_geometry_loss_state_bytes(B, ..) bytes: y [B][Kp], q [B], S, float64.  It
 * carries y from the forward to the backward, so there is one per call in flight; the backward reads grad_loss from the device.
 * Nothing is allocated or synchronised; reentrant under the rules at the top of this file.
 * Checks, all before any HIP call, in this order: (1) a negative size or N < 1 is FR_ERR_INVALID_ARG; (2) K < 1 or K > 256 is
 * FR_ERR_UNSUPPORTED (the size functions answer 0 for both); (3) B == 0 is FR_OK with nothing written; (4) a NULL diff, loss,
 * grad_loss, grad_diff, or basis matrix that has columns, is FR_ERR_INVALID_ARG; (5) a missing, small or misaligned gram,
 * workspace or state is FR_ERR_WORKSPACE.
 * Kernels (csrc/fr_geometry.hip): the build is a workgroup of 8 waves per chunk that stages 32-row slabs in LDS and deals the 16 x 16
 * tile pairs of the upper triangle to its waves (K = 228: 120 pairs, 15 per wave), then one thread per element for the chunk sum;
 * the forward is one workgroup per face (d in LDS, one thread per k) and a one-wave launch for S and the loss; the backward one
 * elementwise launch.  tools/geometry_gram_probe.py (profiles/geometry_gram.json) measures both routes and the build. */
size_t fr_geometry_gram_bytes(int n_shape, int n_exp);
size_t fr_geometry_gram_workspace_bytes(int N, int n_shape, int n_exp);
int fr_geometry_gram_build(const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp, void* gram, size_t gram_bytes,
                           void* workspace, size_t ws_bytes, void* stream);
size_t fr_geometry_loss_state_bytes(int B, int n_shape, int n_exp);
int fr_geometry_loss_forward(const float* diff, const void* gram, int B, int N, int n_shape, int n_exp, float* loss, void* state,
                             size_t state_bytes, void* stream);
int fr_geometry_loss_backward(const float* grad_loss, const void* state, size_t state_bytes, int B, int N, int n_shape, int n_exp,
                              float* grad_diff, void* stream);

/* The Gram build's geometry (no GPU needed; the launcher reads the same function): out[6] = {rows per chunk (the same for every
 * shape), chunks, Kp, 16 x 16 tile pairs with ti <= tj, workgroups of the chunk kernel, its static LDS bytes}.  All zero for a shape
 * the build refuses.  Used by tests/test_geometry_gram_gpu.py to place its shapes on the chunk's edges and by
 * tests/test_geometry_gram_cpu.py. */
void fr_debug_geometry_gram_geom(int N, int n_shape, int n_exp, int* out);

/* ---- fine-depth losses: the fidelity and the smoothness term in one pass, with a backward (opt-in) ---------------------------------
 * The two terms that train the fine depth map (nets/network.py:364-367, 381-392),
 *   fidelity = mse(pred_depth_map, coarse_depth_map)          smoothness = sum |laplace(pred_depth_map)|,
 * are one streaming pass over two planes per direction.  z = pred and c = coarse are [B,H,W] fp32, dense (a trailing channel of 1 is
 * the caller's); pixel (r, c) is row-major.  All arithmetic is float64 on the widened fp32 inputs, every product and every sum
 * rounded on its own (no contraction).
 * NAMES.  The stream parameter is called `stream`, as in the Gram-form geometry loss above and for its reason;
 * tests/test_fine_losses_cpu.py holds these entry points' return codes.
 * LAPLACIAN.  k = ((0.5, 1, 0.5), (1, -6, 1), (0.5, 1, 0.5)).  L(p) = chain over the nine taps t in row-major tap order from +0.0:
 * L = L + k_t * (double)z(p + t), for the taps inside the image; a tap outside contributes nothing (the reference's zero 'SAME'
 * padding).  A face never reads another face.
 * SUMS.  S_f = sum (z - c)^2 and S_s = sum |L| over all B H W pixels, each term formed as above ((double)z - (double)c, squared).
 * Their association is a function of (B, H, W) alone -- not of the stream, an option, the device or a launch geometry chosen at
 * run time -- and both sums use the same one:
 *   tile     the image is cut into tiles of TW x TH = 32 x 16 pixels (fr_debug_fine_losses_geom), tiles across = ceil(W / TW), tiles
 *            down = ceil(H / TH).  A tile has TW TH = 512 slots, slot i = (row in tile) TW + (column in tile); a slot outside the
 *            image holds +0.0.  The slots are taken in groups of 64 consecutive ones (w = 0 .. 7); inside a group, for k = 32, 16, 8,
 *            4, 2, 1 in turn: v[i] = v[i] + v[i + k] for every i < k; the group's sum is v[0].  The eight group sums the same way with
 *            k = 4, 2, 1.  That is the tile's partial.
 *   all      partial p = (face * tiles down + tile row) * tiles across + tile column, p < P.  With F = 1,024: a[i] = chain over
 *            j = 0, 1, .. from +0.0 of partial[i + F j] (while i + F j < P), i < F; then the a[i] in 16 groups of 64 as above, and the
 *            16 group sums with k = 8, 4, 2, 1.
 * (tests/ref_fine_losses.py is this in numpy.)  Every term is >= +0 or NaN, so for finite input each sum lies within
 * n 2^-53 sum |term| of the exact one, n = B H W, in this or any association.
 * OUTPUTS.  fidelity = fl32(S_f / ((double)B (double)H (double)W)), smoothness = fl32(S_s): one fp32 each, on the device.
 * STATE.  `state` is caller-owned, 16-byte aligned, fr_fine_losses_state_bytes(B, H, W) bytes of float64: S_f, S_s, the P fidelity
 * partials, the P smoothness partials.  The forward writes all of it and needs none of it cleared; the backward does not read it
 * (it recomputes what it needs from z and c), so the state is free again when the forward has run.
 * BACKWARD.  s(x) = (x > 0) - (x < 0), so s(+-0) = 0 and s(NaN) = 0 (torch.sign's definition).  The kernel is symmetric, so the
 * adjoint of the stencil is the stencil:
 *   T(p)          = chain over the nine taps in row-major order from +0.0:  T = T + k_t * s(L(p + t)),  taps inside the image
 *                   (a sum of multiples of 0.5: exact)
 *   a             = (double)grad_fidelity[0] * c_f,      c_f = 2.0 / ((double)B (double)H (double)W) formed on the host
 *   grad_pred[p]  = fl32( a * ((double)z - (double)c)  +  (double)grad_smoothness[0] * T(p) )
 *   grad_coarse[p] = fl32( -(a * ((double)z - (double)c)) )
 * grad_fidelity and grad_smoothness are one fp32 each, read from the DEVICE (no host synchronisation).  Either may be NULL: that
 * term is absent -- not evaluated, not added -- so grad_pred is fl32 of the other term alone, exactly +0 with both NULL, and
 * grad_coarse is exactly +0 without grad_fidelity.  grad_coarse may be NULL: not wanted.  Every output bit is fixed by the above,
 * whatever the kernels' design; a gather, no atomics, bit-reproducible.
 * NON-FINITE INPUT.  A non-finite z or c makes the losses non-finite by the IEEE rules.  In the backward the fidelity part is
 * non-finite at that pixel only; a NaN z makes L NaN on its 3 x 3 ring, whose signs are then 0, so T stays finite and changes on the
 * 5 x 5 ring of that face.  No other face's gradient changes by a bit.
 * Checks, all before any HIP call, in this order: a negative size is FR_ERR_INVALID_ARG; then B == 0 or an empty image is FR_OK with
 * nothing launched or written; then a NULL pred, coarse, fidelity, smoothness or grad_pred is FR_ERR_INVALID_ARG; a state that is
 * missing, too small or not 16-byte aligned is FR_ERR_WORKSPACE; more than 2^31 - 65 pixels per face, more than 65,535 faces or
 * more than 65,535 tile rows is FR_ERR_UNSUPPORTED, and fr_fine_losses_state_bytes answers 0 for it (as for an empty or negative
 * shape).  Nothing is allocated or synchronised; reentrant under the rules at the top of this file with a state per call in flight.
 * Kernels (csrc/fr_fine_losses.hip): a workgroup owns a tile, one lane per pixel.  The forward reads its nine-point stencil from
 * global memory (the workgroup's own L1 lines), reduces by lane shuffles and 128 bytes of LDS and writes two partials; a second
 * launch of one 1,024-thread workgroup finishes.  The backward stages z with a 2-pixel halo and s(L) with a 1-pixel halo in LDS
 * (5,328 bytes; 1.2 Laplacians per output) and gathers; the halo runs the device function the forward runs.  At 64 faces of
 * 200 x 200 the forward must move 20 MB and the backward 31 MB (41 with grad_coarse); tools/fine_losses_probe.py
 * (profiles/fine_losses.json) measures both beside the stock-torch route. */
size_t fr_fine_losses_state_bytes(int B, int H, int W);
int fr_fine_losses_forward(const float* pred, const float* coarse, int B, int H, int W, float* fidelity, float* smoothness,
                           void* state, size_t state_bytes, void* stream);
int fr_fine_losses_backward(const float* grad_fidelity, const float* grad_smoothness, const float* pred, const float* coarse, int B,
                            int H, int W, float* grad_pred, float* grad_coarse, void* stream);

/* The fine-losses launch geometry (no GPU needed; the launchers read the same function): out[7] = {tile width, tile height, threads
 * per workgroup, tiles across, tiles down, threads of the finish workgroup (F above), static LDS bytes of a backward workgroup}; the
 * grid is tiles across x tiles down x B.  All zero for an empty shape or one the launchers refuse.  Used by tests/ref_fine_losses.py
 * for the sums' association and by the tests to place their shapes on the tile's edges. */
void fr_debug_fine_losses_geom(int B, int H, int W, int* out);

/* ---- interpolated depth: barycentric z with an x, y, z backward (opt-in) --------------------------------------------------------------
 * Every `depth` plane of the render forward is flat per triangle, h = fl32((z1 + z2) + z3) / 3.0f: the reference's definition, which
 * has no x or y derivative.  The reference also carries get_point_weight (render_depth_op.cc:29-74: the barycentric weights
 * (1 - u - v, v, u) of a point), which nothing calls.  These entry points are a post-pass over a forward's tri_ind that evaluates the
 * winning triangle's PLANE at the pixel, and its gradient with respect to all three coordinates of the triangle's vertices.  Which
 * triangle wins a pixel is not theirs to say: it stays the forward's rule on the flat h, so a pixel's interpolated z may exceed a
 * neighbouring pixel's winner by less than its triangle's z range.  tri_ind, tex_img and normal are not touched.
 *   vertex [B,3,vertex_pitch] (vertex_pitch >= nver: nver for the dense tensor, fr_decode_render_vertex_pitch(N) for the hand-off);
 *   tri [3,ntri], float-stored ids;  tri_ind, depth, depth_grad dense [B,H,W,1];  vertex_grad dense [B,3,nver].
 * NAMES.  The stream parameter is called `stream`, as in the Gram-form geometry loss above and for its reason;
 * tests/test_depth_interp_cpu.py holds these entry points' return codes.
 * WHICH PIXEL.  Pixel (row j, column i) of face b is OK exactly as in the render backwards: tri_ind names t in [0, ntri) and all three
 * ids (p1, p2, p3) of t lie in [0, nver).  NaN, -1, a value >= ntri or a bad id is not OK.  P_k = vertex[b][.][p_k].
 * FORWARD.  Float64 on the widened fp32 inputs, every product and every sum rounded on its own, in get_point_weight's source order
 * (no contraction); x and y only in the first three lines:
 *   v0 = P3 - P1,  v1 = P2 - P1,  v2 = (i, j) - P1
 *   dot00 = v0x v0x + v0y v0y   dot01 = v0x v1x + v0y v1y   dot02 = v0x v2x + v0y v2y
 *   dot11 = v1x v1x + v1y v1y   dot12 = v1x v2x + v1y v2y
 *   den = dot00 dot11 - dot01 dot01
 *   den != 0:  inv = 1 / den
 *              u = (dot11 dot02 - dot01 dot12) inv      v = (dot00 dot12 - dot01 dot02) inv
 *              w1 = (1 - u) - v,  w2 = v,  w3 = u
 *              depth = fl32((w1 z1 + w2 z2) + w3 z3)
 *   den == 0:  depth = the op's own h, formed in fp32 as the forward forms it: fl32(fl32(fl32(z1 + z2) + z3) / 3.0f)
 *   not OK:    depth = the op's background, fl32(-99999999999999.0)
 * (tests/ref_depth_interp.py is this in numpy.)  A pixel outside its triangle (a hand-made tri_ind) is extrapolated by the same lines.
 * BACKWARD.  tri_ind is held fixed and the forward's fp32 rounding is treated as the identity.  G = (double)depth_grad.  For an OK
 * pixel with den != 0, with the forward's values:
 *   gu = ((dot11 v0x - dot01 v1x) inv, (dot11 v0y - dot01 v1y) inv)
 *   gv = ((dot00 v1x - dot01 v0x) inv, (dot00 v1y - dot01 v0y) inv)
 *   A  = ((z2 - z1) gvx + (z3 - z1) gux,  (z2 - z1) gvy + (z3 - z1) guy)          the plane's screen-space slope
 *   for k = 1, 2, 3:   c = G w_k      term_z(p_k) = fl32(c)      term_x(p_k) = fl32(-(c Ax))      term_y(p_k) = fl32(-(c Ay))
 * (d depth / d P_k = -w_k A in x and y: moving a vertex sideways slides the plane under the pixel.)  For an OK pixel with den == 0
 * the z terms are the flat backward's fl32(fl32(g * 1.0f) / 3.0f) for each of the three vertices and the x, y terms are +0.
 * Each (face, row, vertex) sum of terms is formed exactly as fr_render_normal_backward forms its own -- the same record planes, the
 * same owner workgroups (csrc/fr_owner_scatter.h): the terms as 64-bit fixed-point integers on a grid of 2^(e - 39 + shift),
 * e = floor(log2 M), M the face's largest finite |term| over all three rows, shift as above 2^20 pixels; integer addition in LDS by
 * per-face owner workgroups; one rounding to fp32.  No float atomics, bit-reproducible, independent of the launch geometry;
 * |result - exact sum| <= 2^-24 |sum| + n 2^(shift - 39) M for n terms.  A face with a non-finite term takes fp32 LDS atomics: the
 * vertices that receive such a term come out non-finite, the others finite.
 *   accumulate 0: all three rows of every vertex are written (exactly +0 where no OK pixel names the vertex).  accumulate 1: each
 *                 element becomes fl32(old + new), one add; fr_render_normal_backward(.., accumulate = 1) may follow on the same stream.
 *   workspace:    fr_depth_interp_backward_workspace_bytes(B, nver, H, W) = B H W 48 + B ceil(H W / 1024) 8 bytes (0 for an empty
 *                 shape), 16-byte aligned, caller-owned, per call in flight.  The forward needs none.
 * Checks, all before any HIP call, in this order: (1) a negative size, accumulate outside {0, 1} or vertex_pitch < nver is
 * FR_ERR_INVALID_ARG; (2) B == 0 or an empty image is FR_OK with nothing launched and nothing written (so is the backward with
 * nver == 0); (3) a NULL tri_ind, depth or vertex_grad -- or, where triangles exist, a NULL tri, vertex or depth_grad -- is
 * FR_ERR_INVALID_ARG; ntri >= 2^24 or more than 2^31 - 1 pixels per face is FR_ERR_UNSUPPORTED; (4) a workspace that is missing, too
 * small or misaligned is FR_ERR_WORKSPACE.  With ntri == 0 the forward writes the background and the backward zeros (or, accumulate 1,
 * nothing).  Nothing is allocated or synchronised; reentrant under the rules at the top of this file.
 * Kernels (csrc/fr_depth_interp.hip): the forward is one gather pass, one lane per pixel: three id gathers and nine vertex gathers out
 * of L2 (neighbouring lanes hold neighbouring triangles), about 40 fp64 operations, one store; no LDS, no atomics.  The backward is the
 * normal backward's pair: a records pass that makes the same gathers once and writes nine terms per pixel, then the shared owner.
 * Time: tools/depth_interp_probe.py (profiles/depth_interp.json) measures both at 64 and 32 faces of the full mesh at 200 x 200, beside
 * fr_render_depth_backward_ws and fr_render_normal_backward (raw mode, dense stride) on the same inputs and a 512 MiB copy.  MI355X,
 * medians of 6 rounds of 40 calls: forward 25.9 / 14.5 us, where it must move 59 / 29 MB = 11.8 / 5.9 us at the 4.98 TB/s that run's
 * copy reached (0.46 / 0.40 of it); backward 75.4 / 42.6 us beside the normal backward's 76.7 / 43.3 us and the flat backward's
 * 34.2 / 25.9 us, where it must move 100 / 50 MB = 20.0 / 10.0 us (0.27 / 0.23); the rest is the scheme's own records and the id plane
 * that each of a face's 8 owners streams, as in the normal backward. */
int fr_depth_interp_forward(const float* vertex, int vertex_pitch, const float* tri, const float* tri_ind, int B, int nver, int ntri,
                            int H, int W, float* depth, void* stream);
size_t fr_depth_interp_backward_workspace_bytes(int B, int nver, int H, int W);
int fr_depth_interp_backward(const float* depth_grad, const float* vertex, int vertex_pitch, const float* tri, const float* tri_ind,
                             float* vertex_grad, int B, int nver, int ntri, int H, int W, int accumulate, void* workspace,
                             size_t ws_bytes, void* stream);

/* The interpolated-depth backward's launch geometry (no GPU needed; the launcher reads the same function): out[6] as
 * fr_debug_render_normal_bwd_geom -- {owner workgroups per face, vertices per owner (three 64-bit accumulators each), shift,
 * 1,024-pixel record chunks, dynamic LDS bytes of an owner workgroup, 1 if a face's owners are kept on one XCD (batch a multiple of 8)
 * else 0}; all zero for a shape that launches no kernel.  Used by tests/test_depth_interp_cpu.py and tests/test_depth_interp_gpu.py. */
void fr_debug_depth_interp_bwd_geom(int B, int nver, int H, int W, int* out);

/* ---- per-face albedo fit: the least-squares alpha of the shape-from-shading term, on the pixel grid (opt-in) -----------------------
 * The reference's SfS block wanted a least-squares estimate of the albedo coefficients alpha per face given the lighting, and gave it
 * up (nets/network.py:436-455, "The following step cannot be fulfilled!!") for want of a map between the pixel grid and the (3N, 10)
 * texture basis; it uses one param_tex for every face instead.  That map is the rasteriser's tri_ind.  Per face b, all else fixed,
 *   alpha_b = argmin over alpha of  sum_p ( I_b(p) - (a_b(p) + phi_b(p) . alpha) d_b(p) )^2  +  lambda_b |alpha|^2
 * over the pixels the face covers: I = im_gray, a = the albedo image of the MEAN texture (abedo), d = l . n' the shading of the
 * normals the term shades, l = state planes 6-8 of the fused solve, phi(p) = Phi[tri_ind(p)].  Linear in alpha: one Gram matrix of a
 * K-column design per face.  alpha is a fitted quantity, held constant in the backward like the lighting's pseudo-inverse: there is
 * no backward entry point.
 * NAMES.  The stream parameter is called `stream`, as in the Gram-form geometry loss above and for its reason;
 * tests/test_albedo_lse_cpu.py holds these entry points' return codes.
 * BASIS.  Phi is [ntri][K] float64, fr_albedo_basis_bytes(ntri, K) = ntri K 8 bytes (0 for ntri <= 0 or an unserved K), built once:
 *   Phi[t][k] = (1/9) sum_c sum_j pc_tex[c nver + v_j(t)][k],   tri [3,ntri] float-stored ids, pc_tex [3 nver, K] fp32 row-major
 * -- the rasteriser's lookup (t[p1] + t[p2] + t[p3]) / 3 averaged over the three channels.  The nine widened fp32 terms are added in
 * float64 channel-major, then vertex 1, 2, 3, onto the first term (c = 0, j = 1), and the sum is divided by 9.0.  A triangle with a
 * vertex id outside [0, nver) (NaN included; x86 conversion) gets a row of +0.0.  Every bit is fixed by this.  Checks, in this order:
 * a negative size is FR_ERR_INVALID_ARG; K outside 1 .. 15 is FR_ERR_UNSUPPORTED; ntri == 0 is FR_OK; a NULL tri (or pc_tex with
 * nver > 0) is FR_ERR_INVALID_ARG; a basis that is missing, too small or not 16-byte aligned is FR_ERR_WORKSPACE; ntri > 2^24 is
 * FR_ERR_UNSUPPORTED.
 * LIGHTING.  fr_sfs_lighting is the solve half of fr_sfs_solve_shade without the shade: it adds the nparts parts ([nparts][9][H*W],
 * "across ranks" above) in ascending part index starting from part 0, runs fr_sfs_pinv3 and writes the ten state planes -- built from
 * the same device functions, so its state is bit-identical to what fr_sfs_solve_shade and fr_sfs_intensity_forward write for the same
 * maps.  It exists because the fit needs l before abedo_new exists.  Checks as fr_sfs_solve_shade's without the faces: a negative
 * size, a bad rcond, nparts outside 1 .. 4096 is FR_ERR_INVALID_ARG; an empty image is FR_OK; a NULL moment_parts is
 * FR_ERR_INVALID_ARG; a bad state is FR_ERR_WORKSPACE; more than 2^31 - 65 pixels is FR_ERR_UNSUPPORTED.
 * FIT, per pixel p of face b.  Float64 on the widened fp32 inputs, every operation rounded on its own (no contraction).  The pixel is
 * COUNTED iff 0 <= (int)tri_ind < ntri (the x86 conversion of the render backwards: NaN and -1 are not).  With t = (int)tri_ind,
 *   d = (l_x n'_x + l_y n'_y) + l_z n'_z          rho = I - a d
 *   x_k = d Phi[t][k] for k < K,   x_K = rho,   x_k = +0.0 for K < k < 16;   an uncounted pixel gives x = 0 whatever its maps hold.
 *   lighting [3][H*W] float64 (state planes 6-8, shared by the faces);  tri_ind, abedo, im_gray [B,H,W,1], normal_new [B,H,W,3] fp32.
 * MOMENTS.  M_b = sum_p x x^T, 16 x 16, written to moments [B][16][16] float64 (row-major; symmetric bit for bit; rows and columns
 * above K are +0.0).  G = M[:K,:K], r = M[:K,K], E0 = M[K][K]: the residual energy at alpha = 0.
 * ASSOCIATION.  A face's pixels in row-major order are cut into tiles of T = 256 (fr_debug_albedo_lse_geom), tiles = ceil(H W / T).
 * Within a tile, consecutive groups of four pixels are added in ascending order onto +0.0 accumulators by v_mfma_f64_16x16x4_f64
 * (the four products of a group are summed by the instruction, then added to the accumulator).  The tile partials are added in
 * ascending tile order from +0.0; element (i <= j) is written to (i, j) and (j, i).  The bits are a function of the inputs and of
 * (H, W, K) alone -- not of B, the device, a knob or the launch geometry.  No atomics.  Every M_ij lies within n 2^-53 / (1 - n 2^-53)
 * sum_p |x_i x_j| of the exact sum of the rounded products, n = H W.
 * SOLVE.  Per face, float64; every element's chain of products and sums is that of this sequential source order (the kernel forms the
 * elements of a column side by side on the lanes of one wave; tests/ref_albedo_lse.py):
 *   tr = chain over k < K from +0.0 of M_kk;   lambda = (ridge tr) / (double)K;   G' = G + lambda I
 *   Cholesky G' = L L^T by columns c = 0 .. K-1:  piv = G'_cc - (chain over m < c from +0.0 of L_cm L_cm);  L_cc = sqrt(piv);
 *       L_rc = (G_rc - (chain over m < c from +0.0 of L_rm L_cm)) / L_cc  for r > c
 *   L y = r forward (y_r = (r_r - chain over m < r of L_rm y_m) / L_rr),  L^T alpha = y backward (chain over m = r+1 .. K-1 ascending)
 * A face FAILS when it has no counted pixel, when any M_ij (i, j <= K) is not finite, when a pivot is not finite or not
 * > 2^-40 G'_cc, or when an alpha_k is not finite.  A failed face gets alpha_b = +0 (the mean albedo), ok = 0 and E1 = E0, and
 * leaves every other face's bits untouched.
 * OUTPUTS.  alpha [B][K] fp32, rounded once.  stats [B][4] float64 = {counted pixels, E0, E1, ok}, with alpha^ = the rounded alpha
 * widened and the UNRIDGED G:  S1 = chain over k from +0.0 of alpha^_k r_k;  (G alpha^)_k = chain over j from +0.0 of G_kj alpha^_j;
 * S2 = chain over k from +0.0 of alpha^_k (G alpha^)_k;  E1 = (E0 - 2.0 S1) + S2.
 * WORKSPACE.  fr_albedo_lse_workspace_bytes(B, H, W, K) = B tiles 257 doubles (the tile partials as they lie in the registers, then
 * the tiles' counts; 0 for an empty or refused shape), 16-byte aligned, caller-owned, one per call in flight; written before it is read.
 * Checks, all before any HIP call, in this order: a negative size, or a ridge that is negative or not finite, is FR_ERR_INVALID_ARG;
 * K outside 1 .. 15 is FR_ERR_UNSUPPORTED; then B == 0 or an empty image is FR_OK with nothing launched or written; then a NULL
 * pointer is FR_ERR_INVALID_ARG; a workspace that is missing, too small or misaligned is FR_ERR_WORKSPACE; more than 2^31 - 65
 * pixels per face, or more than 2^31 - 1 tile workgroups, is FR_ERR_UNSUPPORTED.  ntri == 0 counts no pixel: every face fails.
 * Nothing is allocated or synchronised; the call makes two launches, can be captured in a graph and is reentrant under the rules at
 * the top of this file with buffers per call in flight.
 * Kernels (csrc/fr_albedo_lse.hip).  The reduction over pixels IS the matrix instruction: X X^T with X = [x(p0) x(p1) x(p2) x(p3)]
 * takes the same register as both operands, lane l holding x_(l mod 16) of pixel 4 g + l / 16, so a wave keeps the whole 16 x 16 sum
 * in four float64 per lane with no cross-lane reduction.  One wave owns a tile (four tiles per workgroup, nothing shared): it reads
 * 64 pixels' maps once, coalesced, and hands d, rho and t to the 16 lanes of each pixel by lane shuffles; lanes k < K gather
 * Phi[t][k], 8 K contiguous bytes per pixel out of a table of 8.5 MB at the full mesh.  The second launch is one workgroup per face:
 * 136 threads chain the tile partials, then one wave solves: lane r holds row r of G' and of L in registers, the rows meet by lane
 * shuffles.
 * Time: tools/albedo_lse_probe.py (profiles/albedo_lse.json) measures the basis build, fr_sfs_lighting and this call at 32 and 64
 * faces of the full mesh at 200 x 200 beside the bytes each must move and the same fit from stock torch ops.
 * MI355X, medians of 6 rounds of 40 calls: the fit 52.8 / 73.8 us, where it must move 84 / 167 MB = 17.7 / 35.3 us at the 4.75 TB/s
 * that run's copy reached (0.33 / 0.48 of it; 52.6 us of the 64-face figure is the tile kernel, 22.9 us finish and solve), beside
 * 2.95 / 3.48 ms for the stock-torch fit; fr_sfs_lighting 7.9 / 8.0 us; the basis build 8.8 / 8.6 us.  Not tuned further. */
size_t fr_albedo_basis_bytes(int ntri, int K);
int fr_albedo_basis_build(const float* tri, const float* pc_tex, int nver, int ntri, int K, void* basis, size_t basis_bytes,
                          void* stream);
int fr_sfs_lighting(const void* moment_parts, int nparts, int H, int W, double rcond, void* state, size_t state_bytes, void* stream);
size_t fr_albedo_lse_workspace_bytes(int B, int H, int W, int K);
int fr_albedo_lse_forward(const void* basis, const float* tri_ind, const void* lighting, const float* normal_new, const float* abedo,
                          const float* im_gray, int B, int ntri, int H, int W, int K, double ridge, float* alpha, void* moments,
                          void* stats, void* workspace, size_t ws_bytes, void* stream);

/* The albedo fit's launch geometry (no GPU needed; the launcher reads the same function): out[5] = {pixels per tile (T above), tiles
 * per face, workgroups of the tile kernel (B ceil(tiles / 4)), workgroups of the finish kernel (B), static LDS bytes of a finish
 * workgroup}; all zero for an empty shape, an unserved K or a shape the launcher refuses.  Used by tests/test_albedo_lse_cpu.py and
 * by tests/test_albedo_lse_gpu.py to place their shapes on the tile's edges. */
void fr_debug_albedo_lse_geom(int B, int H, int W, int K, int* out);

/* ---- synthetic batches: sample, blend the albedo, shade (opt-in; a data source; the blend has an adjoint) ---------------------------
 * The method trains CoarseNet on RENDERED faces of random parameters; the reference pairs a photograph with an unrelated random
 * vector instead (prepare_data/script_generate_dataset.m:105-106).  The decode, the rasteriser with a per-face [B,3,N] texture and
 * the normal map are here already; these three entry points are the rest: parameters drawn where they are consumed, the albedo per
 * face, and the gray image of (tex_img, normal, tri_ind) under a first-order lighting.  pipeline.SynthBatches strings them together.
 * ARITHMETIC.  fp32 in the written order, every operation rounded on its own (no contraction), IEEE division and square root: a
 * float32 model reproduces every output bit (tests/ref_synth_batch.py).  No entry point but the blend's adjoint needs a workspace;
 * nothing is allocated or synchronised; each of the three forward ones makes one launch, can be captured in a graph and is reentrant under the rules at the top of this file.
 * NAMES.  The stream parameter is called `stream`, as in the sections above.
 * SAMPLER.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed lo, seed hi),
 * counter = (j >> 2, g lo, g hi, 0) with g = first_face + b the GLOBAL face index (mod 2^64) and j the draw's index within the
 * face; draw j takes output word j & 3, and u = (float)(word >> 8) * 2^-24 in [0, 1).  A face's values depend on (seed, g) and the
 * sizes alone -- not on B, on the launch geometry, or on which call or rank drew them.  Draw order:
 *   phi, gamma, theta, f, tx, ty, shape[0 .. n_shape), exp[0 .. n_exp), light[0 .. 4), alpha[0 .. K)
 * with the distributions of the reference's get_random_params.m (utils/synth.get_random_params), c = fl32(pi / 180):
 *   phi = (-75 + 120 u) c    gamma = (-90 + 180 u) c    theta = (-30 + 60 u) c    f = u focal    tx, ty = 60 u    tz = 0
 *   pose = beta base + (1 - beta) rand,  base = (0, 0, 0, im_size / 2, im_size / 2, 0, focal);  (1 - beta) is formed once
 *   shape = u 1e4    exp = -1.5 + 3 u    light_k = lo_k + (hi_k - lo_k) u    alpha_k = lo_k + (hi_k - lo_k) u
 * focal is the reference's 1e-3 (a smaller image takes a smaller one).  The kernel holds no transcendental function.
 *   params [B, 7 + n_shape + n_exp] in the 235-d layout [phi, gamma, theta, tx, ty, tz, f | shape | exp], light [B,4], alpha [B,K]:
 *   device fp32.  light_ranges [4][2], alpha_ranges [K][2]: HOST arrays of (lo, hi) pairs, read before the call returns.
 * Checks, in this order: B < 1, a negative n_shape, n_exp or K, a beta outside [0, 1], an im_size or focal that is not finite is
 * FR_ERR_INVALID_ARG; K > FR_SYNTH_MAX_TEX, B > 65,535 or 2^31 - 64 draws per face is FR_ERR_UNSUPPORTED; a NULL params, light or light_ranges -- or, with
 * K > 0, alpha or alpha_ranges -- is FR_ERR_INVALID_ARG; a range pair that is not finite or has lo > hi is FR_ERR_INVALID_ARG.
 * K == 0 draws no albedo and touches neither alpha pointer.  One lane per draw: the four lanes of a block each run the ten rounds.
 * TEXTURE.  tex[b][c][p] = mu_tex[c][p] + sum_k pc_tex[c N + p][k] alpha[b][k] as the chain acc = acc + pc alpha, k ascending from
 * acc = mu_tex: mu_tex [3,N], pc_tex [3N,K] row-major, alpha [B,K], tex [B,3,N] -- what fr_render_depth_forward takes as a
 * per-face texture (tex_batch = B).  Checks: B < 1, N < 1 or K < 0 is FR_ERR_INVALID_ARG; B > 65,535 is FR_ERR_UNSUPPORTED; a NULL
 * mu_tex or tex -- or, with K > 0, pc_tex or alpha -- is FR_ERR_INVALID_ARG.  K == 0 gives tex = mu_tex for every face.  One lane
 * per (c, p) row and face of a group of eight: a workgroup fetches its 256 rows of pc_tex (256 K contiguous floats) once per group,
 * coalesced, through LDS, and writes 64 contiguous floats per wave and face; every output keeps its own chain.
 * TEXTURE BACKWARD.  The blend's adjoint, what carries a gradient of tex to alpha (the photometric loss below is its user):
 *   grad_alpha[b][k] = sum over r < 3N of pc_tex[r][k] grad_tex[b][r],     grad_tex [B,3,N] read as [B,3N], grad_alpha [B,K] fp32.
 * Each product of two widened fp32 values is exact in float64; the sum is float64 in an association that is a function of (N, K)
 * alone -- not of B, the stream or the device: the rows are cut into tiles of 256 consecutive r (the last one ragged; a slot past 3N
 * holds +0.0); inside a tile the 256 products are taken in groups of 64 consecutive ones, v[i] = v[i] + v[i + k] for every i < k with
 * k = 32, 16, .. 1, and the four group sums as (w0 + w2) + (w1 + w3); then a[i] = chain over j = 0, 1, .. from +0.0 of the partial of
 * tile i + 64 j (while there is one), i < 64, the 64 a[i] by the same k = 32 .. 1 steps, and one rounding to fp32
 * (tests/ref_photo_loss.py is this in numpy).  For finite input it lies within
 * 3N 2^-53 sum |pc g| of the exact sum, plus that rounding.  The workspace is caller-owned, 16-byte aligned,
 * fr_synth_texture_backward_workspace_bytes(B, N, K) bytes = ceil(3N / 256) B K float64 partials [b][k][row tile]; the call writes
 * all of it that it reads.  Checks, in this order: B < 1, N < 1 or K < 0 is FR_ERR_INVALID_ARG; B > 65,535, 3N > 2^31 - 257 or
 * B K > 2^31 - 1 is FR_ERR_UNSUPPORTED (the size query answers 0 for all of these); K == 0 is FR_OK with nothing launched, read or
 * written; a NULL pc_tex, grad_tex or grad_alpha is FR_ERR_INVALID_ARG; a missing, short or misaligned workspace is
 * FR_ERR_WORKSPACE.  Two launches: a workgroup owns a row tile and a group of eight faces, stages its run of pc_tex in LDS once,
 * reduces by lane shuffles; a finish kernel adds the tiles, one wave per (b, k).  No atomics, bit-reproducible.
 * SHADE, per pixel, over the planes of a render: tex_img, normal (the op's RAW normal) [B,H,W,3], tri_ind [B,H,W,1], light [B,4],
 * background NULL (bg_batch 0), [1,H,W,1] (bg_batch 1) or [B,H,W,1] (bg_batch B).  A pixel is COVERED iff tri_ind >= 0.  An
 * uncovered pixel gets im_gray = its background pixel (0 without one) and mask = 0.  A covered one gets mask = 1 and
 *   a = ((m(t0) + m(t1)) + m(t2)) / 3.0f,  m(t) = t < 1e-6 ? 1e-6 : t                  (a NaN stays a NaN)
 *   n = -n where n_z < 0;  mag = (nx nx + ny ny) + nz nz, replaced by 1 unless mag > 1e-6;  n^ = n / (sqrt(mag) + 1e-6)
 *   s = ((l0 + l1 n^x) + l2 n^y) + l3 n^z;   I = a (s < 0 ? 0 : s);   im_gray = I gain + offset
 * -- the conventions of FaceRecNet.compute_abedo_image, then a relu(l . n^).  A pixel's outputs depend on that pixel's inputs and
 * its face's light alone: a NaN in a covered pixel's tex_img or normal makes that pixel's im_gray a NaN and no other's.  Two
 * exceptions follow from the rules above: a NaN tri_ind is not >= 0, so the pixel is UNCOVERED and gets its (finite) background;
 * and a NaN in light[b] reaches every covered pixel of face b.  The rasteriser writes neither.  Checks: B, H or W < 1, or a bg_batch that is not 0, 1
 * or B (0 with a background, or not 0 without one), is FR_ERR_INVALID_ARG; a NULL tex_img, normal, tri_ind, light, im_gray or mask
 * is FR_ERR_INVALID_ARG; more than 2^31 - 1 pixels per face or B > 65,535 is FR_ERR_UNSUPPORTED.  One lane per pixel: 28 bytes
 * read and 8 written per covered pixel, 4 (+ 4 of background) and 8 per uncovered one.
 * Time: tools/synth_batch_probe.py (profiles/synth_batch.json). */
enum { FR_SYNTH_MAX_TEX = 64 }; /* albedo coefficients per face the sampler serves (their ranges travel in the launch's arguments) */
int fr_synth_params(unsigned long long seed, unsigned long long first_face, int B, int n_shape, int n_exp, int K, float im_size,
                    float beta, float focal, const float* light_ranges, const float* alpha_ranges, float* params, float* light,
                    float* alpha, void* stream);
int fr_synth_texture(const float* mu_tex, const float* pc_tex, const float* alpha, int B, int N, int K, float* tex, void* stream);
int fr_synth_shade(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* background,
                   int bg_batch, int B, int H, int W, float gain, float offset, float* im_gray, float* mask, void* stream);
size_t fr_synth_texture_backward_workspace_bytes(int B, int N, int K);
int fr_synth_texture_backward(const float* pc_tex, const float* grad_tex, int B, int N, int K, float* grad_alpha, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- photometric loss: fused shade-and-compare with a backward (opt-in) ----------------------------------------------------------------
 * The analysis-by-synthesis term: the image the shader above makes of a render's planes, compared with a picture, per face, in one
 * streaming pass per direction.  tex_img, normal [B,H,W,3] are the render's RAW planes, tri_ind [B,H,W] (a trailing channel of 1 is
 * the caller's), light [B,4], target [B,H,W], weight [B,H,W] or NULL (= 1 everywhere); all fp32, dense.  gain, offset: the shader's.
 * MODEL.  A pixel is COVERED iff tri_ind >= 0 (a NaN tri_ind is uncovered, as in the shader).  At a covered pixel a, n (flipped), mag,
 * d, n^, s and I^ = (a (s < 0 ? 0 : s)) gain + offset are the SHADE chain above in fp32 -- the same device function
 * (csrc/fr_shade.h), the same bits as fr_synth_shade's im_gray.  Then, in float64 on the widened values, every product and sum rounded
 * on its own (no contraction):
 *   r = (double)I^ - (double)target        t = ((2.0 w) r) (double)gain        u = t (double)a where s > 0, else +0.0
 * FORWARD.  sums [B][6] float64 per face:
 *   sse = sum (w r) r      cnt = sum 1.0 (the covered pixels: exact)      L0 = sum u      Lk = sum u (double)n^_k,  k = 1, 2, 3
 * An uncovered pixel contributes +0.0 to all six and nothing of it is read beyond tri_ind.  Only subtraction, multiplication and
 * addition of float64 are involved, so numpy reproduces the sums bit for bit (tests/ref_photo_loss.py).
 * CHOICE.  The four lighting sums are taken in the forward: they are linear in the upstream gradient, so the backward needs no
 * reduction and no second launch, and the forward is memory-bound either way.
 * ASSOCIATION.  A function of (H, W) alone, per face -- not of B (a face's six numbers are the same in any batch), the stream, the
 * device or an option; all six sums use the same one:
 *   tile     the face's H W pixels, row-major, are cut into tiles of T = 256 consecutive ones (fr_debug_photo_loss_geom), tiles =
 *            ceil(H W / T); a slot past the image or off the face holds +0.0.  The slots are taken in groups of 64 consecutive ones;
 *            inside a group, for k = 32, 16, 8, 4, 2, 1 in turn: v[i] = v[i] + v[i + k] for every i < k; the group's sum is v[0].
 *            The four group sums as (w0 + w2) + (w1 + w3).  That is the tile's partial.
 *   face     with F = 256: a[i] = chain over j = 0, 1, .. from +0.0 of partial[i + F j] (while i + F j < tiles), i < F; then the
 *            a[i] in four groups of 64 as above, and the four group sums as (w0 + w2) + (w1 + w3).
 * STATE.  Caller-owned, 16-byte aligned, fr_photo_loss_state_bytes(B, H, W) bytes: the partials [B][tiles][6], float64.  The forward
 * writes all of it and needs none of it cleared; the backward does not read it.
 * BACKWARD.  One pass, one launch; tri_ind is held fixed, target and weight are constants.  Inputs: the forward's, sums, and
 * grad_sse [B] float64, read from the DEVICE (no host synchronisation).  Each output pointer may be NULL: not wanted, not written.
 * Every element of a non-NULL plane is written, +0 at an uncovered pixel: no memset is needed.  With dI = grad_sse[b] t:
 *   grad_tex_img[c] = fl32((dI (double)s) (1.0 / 3.0))   where s > 0 and not tex_c < 1e-6f (the clamp passes a NaN, as the forward
 *                     does); +0 elsewhere
 *   grad_light[b][k] = fl32(grad_sse[b] L_k),  k = 0 .. 3           (needs sums; written by the launch, not reduced again)
 *   grad_normal: q = dI (double)a where s > 0, else +0.0;  g~ = (q (double)l1, q (double)l2, q (double)l3);  with n the flipped
 *                normal, d and mag widened and rho = sqrt((double)mag):
 *                  where the forward kept mag (mag > 1e-6f):  (g~ - n c) / d,  c = ((nx g~x + ny g~y) + nz g~z) / (d rho)
 *                  where it replaced mag by 1:                g~ / d
 *                negated where the forward flipped; rounded once to fp32 at the store.
 * grad_tex_img and grad_light are fixed to the bit by the above; grad_normal up to the device's float64 division and square root
 * (within 2^-24 |value| + 2^-40 (|g~|_1 + |n|_1 |n . g~| / (d rho)) / d of the numpy evaluation).
 * SPECIAL VALUES.  A NaN in a covered pixel's tex_img or normal makes that pixel's r, hence its face's sse, NaN (and, through t, the
 * lighting sums where the pixel is lit, and its own gradients); cnt stays the exact count.  No other face changes by a bit.  A NaN
 * in light[b] or grad_sse[b] reaches face b alone.
 * Checks, all before any HIP call, in this order: a negative size is FR_ERR_INVALID_ARG; then B == 0 or an empty image is FR_OK with
 * nothing launched or written; then a NULL tex_img, normal, tri_ind, light, target or sums (forward), or a NULL grad_sse, tex_img,
 * normal, tri_ind, light or target, or a NULL sums beside a non-NULL grad_light (backward), is FR_ERR_INVALID_ARG; a state that is
 * missing, too small or not 16-byte aligned is FR_ERR_WORKSPACE (forward); more than 2^31 - 1 pixels per face or more than 65,535
 * faces is FR_ERR_UNSUPPORTED, and fr_photo_loss_state_bytes answers 0 for it (as for an empty or negative shape).  A backward with
 * all three outputs NULL launches nothing.  Nothing is allocated or synchronised; reentrant under the rules at the top of this file
 * with a state per call in flight.
 * Kernels (csrc/fr_photo.hip): one lane per pixel, 256 per workgroup, as the shader.  The forward must move about 32 bytes per covered
 * pixel (tex_img, normal, tri_ind, target; 4 more with a weight) and 4 per uncovered one, the backward the same plus the 12 or 24 it
 * writes per pixel; tools/photo_loss_probe.py (profiles/photo_loss.json) measures both beside the stock-torch route
 * (DESIGN.md 4.4m). */
size_t fr_photo_loss_state_bytes(int B, int H, int W);
int fr_photo_loss_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* target,
                          const float* weight, int B, int H, int W, float gain, float offset, double* sums, void* state,
                          size_t state_bytes, void* stream);
int fr_photo_loss_backward(const double* grad_sse, const double* sums, const float* tex_img, const float* normal, const float* tri_ind,
                           const float* light, const float* target, const float* weight, int B, int H, int W, float gain,
                           float offset, float* grad_tex_img, float* grad_normal, float* grad_light, void* stream);

/* The photometric loss's launch geometry (no GPU needed; the launchers read the same functions): out[4] = {pixels per tile (T above),
 * tiles per face, threads of the finish workgroup (F above), sums per face}; the forward's grid is tiles x B, the finish step's B.
 * All zero for an empty shape or one the launchers refuse.  Used by tests/ref_photo_loss.py for the sums' association. */
void fr_debug_photo_loss_geom(int B, int H, int W, int* out);

/* ---- colour shading: RGB second-order lighting, its sampler, the loss and its backward (opt-in) ------------------------------------
 * The gray route above collapses tex_img's three channels into one mean and lights it to first order.  This is the same chain in
 * colour: per-channel albedo under a nine-term lighting per channel.  The gray entry points, their arithmetic and their bits are
 * unchanged; nothing here is reached unless it is called.  tex_img, normal [B,H,W,3] are the render's RAW planes, tri_ind [B,H,W] (a
 * trailing channel of 1 is the caller's), light [B,3,9] channel-major (light[b][c][k]); all fp32, dense.
 * MODEL (csrc/fr_shade.h, stated once; the shader and the loss run the same device function).  A pixel is COVERED iff tri_ind >= 0 (a
 * NaN is uncovered).  At a covered pixel, in fp32, every operation rounded on its own (no contraction):
 *   a_c = t_c < 1e-6f ? 1e-6f : t_c   per channel, no mean                                      (a NaN stays a NaN)
 *   n, mag, d, n^ = (hx, hy, hz): exactly the SHADE chain above (the same helper)
 *   H0 = 1 (never multiplied)   H1 = hx   H2 = hy   H3 = hz   H4 = hx hy   H5 = hx hz   H6 = hy hz
 *   H7 = hx hx - hy hy          H8 = 3.0f (hz hz) - 1.0f
 *   s_c = l_c0 + l_c1 H1, then + l_c2 H2, .. , + l_c8 H8, left to right;   I_c = a_c (s_c < 0 ? 0 : s_c);   im_rgb_c = I_c gain + offset
 * The basis is the real spherical harmonics up to order two WITHOUT their normalisation: those constants, and the cosine lobe's, are
 * folded into the coefficients.  im_gray = (0.3f R + 0.59f G) + 0.11f B of im_rgb (the weights of utils/data_process.py), at an
 * uncovered pixel too, where im_rgb is the background's pixel.
 * SAMPLER.  fr_synth_light_rgb: Philox4x32-10 with the key of fr_synth_params, counter = (j >> 2, g lo, g hi, 1), j = 9 c + k, word
 * j & 3 -- the fourth counter word is 1 where fr_synth_params uses 0: the two streams are disjoint and no existing draw moves.
 * u = (float)(word >> 8) * 2^-24 and light[b][c][k] = lo_j + (hi_j - lo_j) u, as there.  ranges: a HOST array [27][2] of (lo, hi)
 * pairs, read before the call returns.  Checks, in this order: B < 1 is FR_ERR_INVALID_ARG; B > 65,535 is FR_ERR_UNSUPPORTED; a NULL
 * ranges or light is FR_ERR_INVALID_ARG; a pair that is not finite or has lo > hi is FR_ERR_INVALID_ARG.  One launch, capturable.
 * SHADE.  fr_synth_shade_rgb: background NULL (bg_batch 0), [1,H,W,3] (bg_batch 1) or [B,H,W,3] (bg_batch B).  An uncovered pixel
 * gets im_rgb = its background pixel (0 without one) and mask = 0, a covered one the model's im_rgb and mask = 1; im_gray [B,H,W]
 * may be NULL (not wanted, not written).  Checks: those of fr_synth_shade in its order, with im_rgb in im_gray's place.  One lane per
 * pixel, one launch, capturable: 28 bytes read and 16 or 20 written per covered pixel.
 * LOSS.  target [B,H,W,3], weight [B,H,W] or NULL (= 1).  Per covered pixel, in float64 on the widened fp32 values, every operation
 * rounded on its own, with I^_c = im_rgb_c above (the shader's bits):
 *   r_c = (double)I^_c - (double)target_c      t_c = ((2.0 w) r_c) (double)gain      u_c = t_c (double)a_c where s_c > 0, else +0.0
 * FORWARD.  sums [B][29] float64 per face:
 *   sse = sum (((w r_0) r_0 + (w r_1) r_1) + (w r_2) r_2)       cnt = sum 1.0 (exact)
 *   L[c][k] = sum u_c (double)H_k at index 2 + 9 c + k; for k = 0 the term is u_c itself
 * An uncovered pixel contributes +0.0 to every sum and nothing of it beyond tri_ind is read.
 * ASSOCIATION.  The gray loss's, for every one of the 29 sums: the same 256-pixel tile, the same lane tree, the same finish chain with
 * F = 256; a function of (H, W) alone.  The kernels share the tree and the finish step with the gray loss (templates in the number of
 * sums).  STATE: caller-owned, 16-byte aligned, fr_photo_loss_rgb_state_bytes(B, H, W) bytes: the partials [B][tiles][29], float64, all
 * written by the forward; the backward does not read it.
 * BACKWARD.  One map pass, one launch; grad_sse [B] float64 is read from the DEVICE.  Each output may be NULL; every element of a
 * non-NULL plane is written (+0 at an uncovered pixel).  With dI_c = grad_sse[b] t_c:
 *   grad_tex_img[c] = fl32(dI_c (double)s_c) where s_c > 0 and not tex_c < 1e-6f; +0 elsewhere
 *   grad_light[b][c][k] = fl32(grad_sse[b] L[c][k])                                       (needs sums)
 *   grad_normal: q_c = dI_c (double)a_c where s_c > 0, else +0.0;  g~ = sum over c of q_c ds_c/dn^, the channels ascending from +0.0,
 *                in float64 on the widened l and n^, each bracket left to right:
 *                  ds/dhx = ((l1 + l4 hy) + l5 hz) + (2.0 l7) hx
 *                  ds/dhy = ((l2 + l4 hx) + l6 hz) - (2.0 l7) hy
 *                  ds/dhz = ((l3 + l5 hx) + l6 hy) + (6.0 l8) hz
 *                then the normalisation's backward of the gray loss above, on this g~: (g~ - n c) / d where mag was kept, g~ / d where
 *                it was replaced; negated where the forward flipped; rounded once to fp32 at the store.
 * grad_tex_img and grad_light are fixed to the bit; grad_normal within the gray loss's bound evaluated with this g~.
 * SPECIAL VALUES.  A NaN in a covered pixel makes its face's sse NaN, and reaches a channel's lighting sums where that channel is
 * lit; cnt stays exact.  A NaN in a pixel, in light[b] or in grad_sse[b] changes no other face.
 * Checks, limits and their order: the gray loss's, entry point by entry point (fr_photo_loss_rgb_state_bytes answers 0 where
 * fr_photo_loss_state_bytes does).  Kernels (csrc/fr_photo.hip): one lane per pixel, 256 per workgroup.  The forward must move 40
 * bytes per covered pixel (tex_img, normal, tri_ind, target; 4 more with a weight) and 4 per uncovered one, the backward the same
 * plus the 24 it writes; tools/photo_rgb_probe.py (profiles/photo_rgb.json). */
int fr_synth_light_rgb(unsigned long long seed, unsigned long long first_face, int B, const float* ranges, float* light, void* stream);
int fr_synth_shade_rgb(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* background,
                       int bg_batch, int B, int H, int W, float gain, float offset, float* im_rgb, float* im_gray, float* mask,
                       void* stream);
size_t fr_photo_loss_rgb_state_bytes(int B, int H, int W);
int fr_photo_loss_rgb_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* target,
                              const float* weight, int B, int H, int W, float gain, float offset, double* sums, void* state,
                              size_t state_bytes, void* stream);
int fr_photo_loss_rgb_backward(const double* grad_sse, const double* sums, const float* tex_img, const float* normal,
                               const float* tri_ind, const float* light, const float* target, const float* weight, int B, int H, int W,
                               float gain, float offset, float* grad_tex_img, float* grad_normal, float* grad_light, void* stream);
/* out[4] = {pixels per tile, tiles per face, threads of the finish workgroup, sums per face (29)}; all zero as above. */
void fr_debug_photo_loss_rgb_geom(int B, int H, int W, int* out);

/* ---- colour photometric solve: per-face least squares for the lighting and for the albedo coefficients (opt-in) ---------------------
 * The colour model above is bilinear, I_c(p) = a_c(p) s_c(p): s_c = sum_k light[c][k] H_k(n^) is linear in the lighting, and with
 * t = tri_ind(p) the albedo a_c(p) = m_c[t] + Phi_c[t] . alpha is affine in alpha.  With the texture held each channel's lighting is a
 * 9-unknown linear least squares per face; with the lighting held alpha is a K-unknown one per face over the three channels.  These
 * entry points are the two solves and the two maps that let a caller alternate them without blending [B,3,N] textures or rasterising
 * again.  Nothing existing changes; nothing here has a backward (the results are fitted quantities).  All planes dense, fp32: tex_img,
 * normal, target [B,H,W,3]; tri_ind, weight [B,H,W] (a trailing channel of 1 is the caller's); light, gate_light [B,3,9]; alpha [B,K].
 * NAMES.  The stream parameter is called `stream`, as in the sections above; tests/test_photo_solve_rgb_cpu.py holds the return codes.
 * BASIS.  fr_albedo_basis_rgb_build, once per mesh: basis [ntri][3][K+1] float64, fr_albedo_basis_rgb_bytes(ntri, K) =
 * ntri 3 (K + 1) 8 bytes (0 for ntri <= 0 or an unserved K).  tri [3,ntri] float-stored ids, mu_tex [3 nver], pc_tex [3 nver, K]
 * row-major, both channel-major (row c nver + v).  On the widened fp32 values, in float64:
 *   Phi_c[t][k] = ((pc[c,v1,k] + pc[c,v2,k]) + pc[c,v3,k]) / 3.0   at slot k < K;     m_c[t] = the same expression of mu_tex at slot K
 * A triangle with a vertex id outside [0, nver) (NaN included; x86 conversion) gets a row of +0.0.  1 <= K <= 15.  Every bit is fixed.
 * IMAGE.  fr_albedo_image_rgb, one lane per pixel, one launch: at a pixel with 0 <= (int)tri_ind < ntri (x86 conversion)
 *   tex_img_c = fl32( chain from m_c[t] of + Phi_c[t][k] (double)alpha_k, k ascending ),  float64, rounded once;   +0 elsewhere.
 * Every element is written; every bit is fixed.  Against render_depth's tex_img of the texture fr_synth_texture blends from the same
 * mu_tex, pc_tex and alpha -- an fp32 chain of K products and K sums per vertex, two sums over the vertices and a division, K + 4
 * roundings on the largest path -- this plane differs at a pixel both cover by at most
 *   gamma A,   gamma = n u / (1 - n u),  u = 2^-24,  n = K + 6,   A = (1/3) sum_j ( |mu_c[v_j]| + sum_k |pc_c[v_j][k]| |alpha_k| )
 * (K + 4 roundings there, one here, one more unit for the float64 chain and the second-order terms).
 * LIGHT FIT.  fr_photo_light_lse_rgb_forward.  A pixel is COVERED iff tri_ind >= 0, the loss's rule; nothing is gathered.  At a covered
 * pixel a_c (clamped) and H_0 .. H_8 are the MODEL's, from the shader's own device function: the loss's bits.  Channel c COUNTS the
 * pixel iff it is covered, weight is NULL or w > 0, and gate_light is NULL or the fp32 chain s_c of gate_light[b] is > 0 there (the
 * active set of the clamp: an unlit pixel's model value does not depend on the lighting).  In float64 on the widened values, every
 * operation rounded on its own:
 *   x^c_k = ((double)a_c (double)H_k) (double)gain  for k = 1 .. 8;   x^c_0 = (double)a_c (double)gain;   x^c_9 = (double)T_c - (double)offset
 *   x^c_k = +0.0 for 9 < k < 16, and x^c = 0 where channel c does not count the pixel, whatever the planes hold.
 * MOMENTS.  M_bc = sum_p (w x_i) x_j with i <= j mirrored: moments [B][3][16][16] float64, symmetric bit for bit, rows and columns
 * above 9 +0.0.  G = M[:9,:9], r = M[:9,9], E0 = M[9][9].  Without a weight the product is x_i x_j (the same register twice).
 * ALBEDO FIT.  fr_albedo_lse_rgb_forward.  A pixel is COUNTED iff 0 <= (int)tri_ind < ntri (x86 conversion) and weight is NULL or
 * w > 0.  With s_c the fp32 chain of light[b] at the pixel's normal (the model's function) and s+_c = s_c < 0 ? 0 : s_c, per channel:
 *   x_k = ((double)s+_c Phi_c[t][k]) (double)gain  for k < K;   x_K = ((double)T_c - (double)offset) - ((double)s+_c m_c[t]) (double)gain
 *   x_k = +0.0 for K < k < 16.  M_b = sum_p sum_c (w x_i) x_j, the channels ascending within a pixel group: moments [B][16][16].
 * The albedo's clamp at 1e-6 is NOT in this affine model: E1 below is the affine model's residual, photo_loss_rgb the clamped one's;
 * they agree where every fitted albedo is >= 1e-6.
 * ASSOCIATION.  That of the per-face albedo fit above: tiles of T = 256 pixels (fr_debug_photo_solve_rgb_geom), within a tile
 * consecutive groups of four pixels added in ascending order onto +0.0 accumulators by v_mfma_f64_16x16x4_f64 -- one accumulator per
 * channel in the light fit, ONE in the albedo fit, which takes a group's channels 0, 1, 2 in turn -- the tile partials
 * [face][tile][channel][register][lane] added in ascending tile order from +0.0.  A function of the inputs and (H, W) alone.  No
 * atomics.  Every M_ij lies within gamma_n sum |w x_i x_j| of the exact sum of the rounded products, gamma_n = n 2^-53 / (1 - n 2^-53),
 * n = H W for the light fit and 3 H W for the albedo fit.
 * SOLVE.  One wave per (face, channel) of the light fit (9 unknowns, lambda = (ridge tr) / 9.0) and per face of the albedo fit (K
 * unknowns, lambda = (ridge tr) / (double)K): the SOLVE of the per-face albedo fit above, word for word -- the trace chain, the
 * Cholesky by columns, the two substitutions, the pivot test piv > 2^-40 G'_cc (a Gram matrix of condition 1e8 has every pivot
 * >= 1e-8 G'_cc: admitted), the failure rules, and E1 = (E0 - 2.0 S1) + S2 on the rounded coefficients and the unridged G.
 * OUTPUTS.  light [B,3,9] / alpha [B,K] fp32, rounded once; stats [B][3][4] / [B][4] float64 = {count, E0, E1, ok}.  A unit that
 * FAILS (no counted pixel, a non-finite moment, a vanishing pivot, a non-finite coefficient) has ok = 0 and E1 = E0; the light fit
 * writes gate_light's row there (+0 without a gate), the albedo fit +0.  A failure touches its (face, channel) or face alone.
 * WORKSPACE.  fr_photo_solve_rgb_workspace_bytes(B, H, W) = B tiles 3 257 doubles serves either solve (0 for an empty or refused
 * shape); 16-byte aligned, caller-owned, one per call in flight; written before it is read.
 * Checks, all before any HIP call, in this order: a negative size, or a ridge that is negative or not finite, or a gain or offset that
 * is not finite, is FR_ERR_INVALID_ARG; an empty shape (B, H or W of 0; ntri == 0 for the basis) is FR_OK with nothing launched or
 * written; a NULL pointer (weight and gate_light may be NULL; basis only with ntri == 0; mu_tex and pc_tex only with nver == 0) is
 * FR_ERR_INVALID_ARG; a workspace or basis that is missing, too small or misaligned is FR_ERR_WORKSPACE; K outside 1 .. 15, more than
 * 65,535 faces, more than 2^31 - 1 pixels per face, more than 2^31 - 1 tile workgroups or ntri > 2^24 in the build is
 * FR_ERR_UNSUPPORTED.  Nothing is allocated or synchronised; each solve makes two launches, can be captured in a graph and is reentrant
 * with buffers per call in flight.  Kernels: csrc/fr_photo_solve.hip; time: tools/photo_solve_rgb_probe.py. */
size_t fr_albedo_basis_rgb_bytes(int ntri, int K);
int fr_albedo_basis_rgb_build(const float* tri, const float* mu_tex, const float* pc_tex, int nver, int ntri, int K, void* basis,
                              size_t basis_bytes, void* stream);
int fr_albedo_image_rgb(const void* basis, const float* tri_ind, const float* alpha, int B, int ntri, int H, int W, int K,
                        float* tex_img, void* stream);
size_t fr_photo_solve_rgb_workspace_bytes(int B, int H, int W);
int fr_photo_light_lse_rgb_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* target,
                                   const float* weight, const float* gate_light, int B, int H, int W, float gain, float offset,
                                   double ridge, float* light, void* moments, void* stats, void* workspace, size_t ws_bytes,
                                   void* stream);
int fr_albedo_lse_rgb_forward(const void* basis, const float* tri_ind, const float* normal, const float* light, const float* target,
                              const float* weight, int B, int ntri, int H, int W, int K, float gain, float offset, double ridge,
                              float* alpha, void* moments, void* stats, void* workspace, size_t ws_bytes, void* stream);
/* out[6] = {pixels per tile, tiles per face, workgroups of a tile kernel (B ceil(tiles / 4)), workgroups of the light fit's finish
 * kernel (3 B), of the albedo fit's (B), static LDS bytes of a finish workgroup}; all zero for an empty or refused shape. */
void fr_debug_photo_solve_rgb_geom(int B, int H, int W, int* out);

/* ---- fine mesh: the fine depth map lifted onto the vertices, visibility, vertex normals (opt-in, forward only) ----------------------
 * FineNet's output is a [B,H,W,1] plane and the coarse decode a [B,3,N] vertex tensor; the reference leaves them unjoined
 * (nets/network.py:451-453, "how to inversely convert predicted fine depth into new vertices?") and keeps the coarse vertices.  The
 * map between the two is the rasteriser's tri_ind.  Three entry points, none with a backward (the vertex normals' is stated with the
 * smooth planes below, its one consumer):
 *   vertex [B,3,vertex_pitch] (vertex_pitch >= nver, as in the interpolated depth);  tri [3,ntri], float-stored ids;  tri_ind,
 *   fine_depth, coarse_depth dense [B,H,W] (a trailing channel of 1 is the caller's);  visible, state uint8 [B,nver];  vertex_out,
 *   normal [B,3,out_pitch] (out_pitch >= nver; the columns from nver on are not written).  x is the column, y the row.
 * NAMES.  The stream parameter is called `stream`, as in the sections above; tests/test_fine_mesh_cpu.py holds the return codes.
 * ARITHMETIC.  Float64 on the widened fp32 inputs, every operation rounded on its own (no contraction), IEEE division and square root:
 * numpy reproduces every output bit (tests/ref_mesh.py).  Every output element is written on every call.  No float atomics.
 * VISIBLE.  visible[b][v] = 1 iff at least one OK pixel of face b -- OK exactly as in the interpolated depth above: tri_ind names
 * t in [0, ntri) and all three ids of t lie in [0, nver); NaN, -1, a value >= ntri or a bad id is not OK -- names v among the three
 * ids of its triangle; else 0.  The call zeroes the plane itself (a memset on `stream`), then one pass over the pixels stores the
 * byte 1: the only race is several lanes storing the same value, so the result is a function of the inputs alone.  ntri == 0 or an
 * empty image gives all zeros.
 * LIFT.  Rows x and y of vertex_out are copies of vertex's, bit for bit.  Per (face, vertex), with (x, y, z) its position:
 *   visible == 0:                      state = 0, z copied
 *   x or y not finite, or ntri == 0:   state = 2, z copied
 *   else  c0 = floor(x), r0 = floor(y), fx = x - c0, fy = y - r0; the corners (r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1)
 *         in this order, with the weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy  ((1 - fx) and (1 - fy) formed once).
 *         A corner COUNTS when it lies inside the image, its tri_ind converts (the x86 conversion of the render backwards) to a
 *         t in [0, ntri), and its weight is not 0; a corner that does not count is neither read in the depth maps nor multiplied.
 *         For a counting corner d_k = (double)fine - (double)coarse; num and den are the chains, from +0.0 in corner order, of
 *         w_k d_k and of w_k.
 *   no counting corner:                state = 2, z copied
 *   else                               state = 1, z' = fl32((double)z + num / den)
 * The DIFFERENCE is sampled, not fine_depth: the flat coarse depth is a staircase per triangle, and the difference leaves it out of
 * the mesh.  A non-finite depth reaches only the vertices whose stencil reads it.  x and y do not move.
 * VERTEX NORMALS.  A gather over a vertex -> triangle adjacency in CSR form, built once per mesh on the host: adj_start int32
 * [nver + 1], adj_tri int32 [3 ntri] (utils/mesh_io.vertex_adjacency; device arrays, shared by the faces).  Per (face, vertex) the
 * triangles adj_tri[adj_start[v] .. adj_start[v + 1]) are walked in table order; each contributes (P2 - P1) x (P3 - P1), the render's
 * orientation, area-weighted: with a = P2 - P1, b = P3 - P1 in float64, (ay bz - az by, az bx - ax bz, ax by - ay bx).  The three sums
 * are float64 chains from +0.0 in table order; s = sqrt((nx nx + ny ny) + nz nz); normal = fl32(n / s) per component, or (+0, +0, +0)
 * where s is 0 or not finite.  A triangle with an id outside [0, nver) contributes nothing.  The TABLE is checked on the host side of
 * the binding (rendering_layer/ops.py::MeshAdjacency: adj_start starts at 0, never decreases and ends at most at 3 ntri -- at 3 ntri unless a
 * triangle names a vertex twice, which lists it once, or names an id outside the mesh -- and ids in range); the kernel skips an entry
 * outside [0, ntri) and clamps a row to the table, so a bad table gives wrong normals, not a fault.
 * Checks, all before any HIP call, in this order: (1) a negative size, or a pitch below nver, is FR_ERR_INVALID_ARG; (2) B == 0 or
 * nver == 0 is FR_OK with nothing launched and nothing written; (3) a NULL vertex, visible, vertex_out, state, normal -- or, where
 * triangles (and, for the first two, pixels) exist, a NULL tri, tri_ind, fine_depth, coarse_depth, adj_start, adj_tri -- is
 * FR_ERR_INVALID_ARG; (4) ntri >= 2^24, more than 2^31 - 1 pixels per face, or more than 2^31 - 1 workgroups of 256 lanes (pixels for
 * the first, vertices for the other two; the grid is one-dimensional, so the 65,535 limit of the other grid axes does not arise) is
 * FR_ERR_UNSUPPORTED.  Nothing is allocated or synchronised; each call is one launch (fr_mesh_visible: a memset and a launch), can be
 * captured in a graph and is reentrant under the rules at the top of this file.
 * Kernels (csrc/fr_mesh.hip): fr_mesh_visible one lane per pixel in 256-pixel blocks, as the interpolated depth's forward; the other
 * two one lane per (face, vertex), consecutive lanes on consecutive vertices.  No LDS, no workspace.
 * Time: tools/fine_mesh_probe.py (profiles/fine_mesh.json) measures the three at 32 and 64 faces of the full mesh at 200 x 200 beside
 * the bytes each must move, a 512 MiB copy and the same operators from stock torch ops. */
int fr_mesh_visible(const float* tri, const float* tri_ind, int B, int nver, int ntri, int H, int W, unsigned char* visible,
                    void* stream);
int fr_mesh_lift(const float* vertex, int vertex_pitch, const float* tri_ind, const unsigned char* visible, const float* fine_depth,
                 const float* coarse_depth, int B, int nver, int ntri, int H, int W, float* vertex_out, int out_pitch,
                 unsigned char* state, void* stream);
int fr_mesh_vertex_normals(const float* vertex, int vertex_pitch, const float* tri, const int* adj_start, const int* adj_tri, int B,
                           int nver, int ntri, float* normal, int out_pitch, void* stream);

/* ---- smooth planes: interpolated vertex attributes with a backward, and the backward of the vertex normals (opt-in) -------------------
 * Every plane the render forward hands to the shading chain is flat per triangle: tex_img is (t[p1] + t[p2] + t[p3]) / 3, normal the
 * winner's facet normal; only depth has a barycentric variant (the interpolated depth above).  These entry points are the third
 * primitive beside "rasterise" and "shade": INTERPOLATE a three-channel per-vertex attribute at the pixel, by the interpolated depth's
 * weights, with gradients to the attribute and to the vertex positions -- and the adjoint of fr_mesh_vertex_normals, so that a plane
 * of interpolated vertex normals is differentiable down to the vertices.  Post-passes over a forward's tri_ind: which triangle wins a
 * pixel is not theirs to say.  No existing plane, flag or bit changes.
 *   vertex [B,3,vertex_pitch], attr [B,3,attr_pitch] (pitches >= nver, as in the interpolated depth);  tri [3,ntri], float-stored ids;
 *   tri_ind dense [B,H,W,1];  out, grad dense [B,H,W,3];  attr_grad, vertex_grad dense [B,3,nver];
 *   records int32 [2,B,3,H W,4], 16-byte aligned;  partial uint32 [2,B,ceil(H W / 1024),2], 8-byte aligned;
 *   normal_grad [B,3,grad_pitch], vertex_grad of the normals' backward [B,3,out_pitch] (pitches >= nver);  h float64 [B,3,nver].
 * NAMES.  The stream parameter is called `stream`, as in the sections above; tests/test_attr_interp_cpu.py holds the return codes.
 * WHICH PIXEL.  A pixel is OK exactly as in the interpolated depth (tri_ind names t in [0, ntri) and all three ids (p1, p2, p3) of t
 * lie in [0, nver)); NaN, -1, a value >= ntri or a bad id is not OK.  a_kc = attr[b][c][p_k].
 * FORWARD.  w and den are the interpolated depth's, by the same lines in the same order (csrc/fr_point_weight.h), in float64 on the
 * widened fp32 inputs, every product and sum rounded on its own.  Per channel c = 0, 1, 2:
 *   den != 0:  out_c = fl32((w1 a_1c + w2 a_2c) + w3 a_3c)
 *   den == 0:  out_c = the render's own texture lookup, in fp32: fl32(fl32(fl32(a_1c + a_2c) + a_3c) / 3.0f)
 *   not OK:    out_c = +0
 * Every element of out is written.  With attr = vertex, channel 2 is fr_depth_interp_forward's depth bit for bit on OK pixels.
 * (tests/ref_attr_interp.py is this in numpy.)  Nothing is normalised: a consumer of a normal plane normalises (csrc/fr_shade.h does).
 * BACKWARD.  tri_ind is held fixed and the forward's fp32 rounding is treated as the identity.  G_c = (double)grad_c.  For an OK pixel
 * with den != 0, with gu, gv of the interpolated depth's backward:
 *   attribute terms   term_c(p_k) = fl32(G_c w_k)
 *   vertex terms      A_c = ((a_2c - a_1c) gvx + (a_3c - a_1c) gux,  (a_2c - a_1c) gvy + (a_3c - a_1c) guy)     channel c's slope
 *                     S = ((G_0 A_0x + G_1 A_1x) + G_2 A_2x,  (G_0 A_0y + G_1 A_1y) + G_2 A_2y)
 *                     term_x(p_k) = fl32(-(w_k Sx))      term_y(p_k) = fl32(-(w_k Sy))      term_z(p_k) = +0
 * For an OK pixel with den == 0 the attribute terms are fl32(fl32(g_c * 1.0f) / 3.0f) for each of the three vertices and all nine
 * vertex terms are +0.  Each (face, row, vertex) sum of terms is formed exactly as the interpolated depth's backward forms its own
 * (the same record planes, the same owner workgroups, csrc/fr_owner_scatter.h), ONE SET OF RECORDS AND MAXIMA PER OUTPUT: 64-bit
 * fixed point on a grid of 2^(e - 39 + shift), e = floor(log2 M), M the face's largest finite |term| of THAT output; integer
 * addition in LDS; one rounding to fp32.  No float atomics, bit-reproducible, independent of the launch geometry and of the batch a
 * face is in, and an output requested alone has the bits it has when both are requested;
 * |result - exact sum| <= 2^-24 |sum| + n 2^(shift - 39) M for n terms.  A face with a non-finite term in an output takes fp32 LDS
 * atomics for that output, as there.  The z row of vertex_grad is exactly +0 (accumulate 0).
 *   attr_grad, vertex_grad: either may be NULL (not requested: its terms are not formed), not both.  attr_accumulate,
 *                 vertex_accumulate 0: every element is written (exactly +0 where no OK pixel names the vertex); 1: each element
 *                 becomes fl32(old + new), one add.
 *   records, partial: caller-owned, per call in flight; set 0 is the attribute's, set 1 the vertex's.  The call needs neither
 *                 cleared, writes nothing outside the stated shapes, and their contents after the call are unspecified.  The forward
 *                 needs none.
 * Checks of fr_attr_interp_*, all before any HIP call, in the order and with the codes of fr_depth_interp_*: (1) a negative size, an
 * accumulate flag outside {0, 1} or a pitch below nver is FR_ERR_INVALID_ARG; (2) B == 0 or an empty image is FR_OK with nothing
 * launched and nothing written (so is the backward with nver == 0); (3) a NULL tri_ind or out, both gradients NULL -- or, where
 * triangles exist, a NULL tri, vertex, attr or grad -- is FR_ERR_INVALID_ARG; ntri >= 2^24 or more than 2^31 - 1 pixels per face is
 * FR_ERR_UNSUPPORTED; (4) where triangles exist, a records or partial that is NULL or misaligned is FR_ERR_WORKSPACE; (5) more than
 * 2^31 - 1 workgroups in a launch is FR_ERR_UNSUPPORTED.  With ntri == 0 the forward writes +0 everywhere and the backward zeros
 * (or, under accumulate, nothing).  Nothing is allocated or synchronised; reentrant under the rules at the top of this file.
 * VERTEX NORMALS, BACKWARD.  The adjoint of fr_mesh_vertex_normals as two gathers (no atomics, one fixed chain per element), in
 * float64 with every operation rounded on its own.  The forward's single rounding of N / s to fp32 is not differentiated.
 *   launch 1, per (face, vertex u): N and s are the forward's three chains and their length, recomputed.  Where the forward wrote
 *             (+0, +0, +0) (s is 0 or not finite), h_u = (0, 0, 0).  Else n^ = N / s per component, g = (double)normal_grad[b][.][u],
 *             d = (n^x gx + n^y gy) + n^z gz, and h_u = (g - n^ d) / s per component.
 *   launch 2, per (face, vertex v): the triangles adj_tri[adj_start[v] .. adj_start[v + 1]) in table order, those with an id outside
 *             [0, nver) skipped as in the forward.  Hs = h[p1], + h[p2] if p2 != p1, + h[p3] if p3 is neither (every distinct vertex
 *             of a triangle counted it once).  For each position k = 1, 2, 3 in this order with p_k == v, the three chains (from
 *             +0.0) add  (P2 - P3) x Hs (k = 1),  (P3 - P1) x Hs (k = 2),  Hs x (P2 - P1) (k = 3), each cross product p x q as
 *             (py qz - pz qy, pz qx - px qz, px qy - py qx) -- the forward's order.  vertex_grad = the chains rounded to fp32 once;
 *             accumulate 1: fl32(old + that).
 * h is caller-owned typed scratch, 8-byte aligned, per call in flight; the call needs it not cleared and leaves its contents
 * unspecified.  The table conventions and the host-side table check are the forward's.  Checks, in this order: (1) a negative size,
 * a pitch below nver or accumulate outside {0, 1} is FR_ERR_INVALID_ARG; (2) B == 0 or nver == 0 is FR_OK with nothing launched;
 * (3) a NULL normal_grad, vertex, vertex_grad -- or, where triangles exist, a NULL tri, adj_start, adj_tri -- is FR_ERR_INVALID_ARG;
 * (4) ntri >= 2^24 or more than 2^31 - 1 workgroups of 256 vertices is FR_ERR_UNSUPPORTED; (5) an h that is NULL or misaligned is
 * FR_ERR_WORKSPACE.
 * Kernels (csrc/fr_attr_interp.hip, csrc/fr_mesh.hip): the interpolation's forward is one gather pass, one lane per pixel (three id
 * gathers, six coordinate and nine attribute gathers out of L2, three stores; no LDS, no atomics); its backward one records pass
 * (256 threads x 4 pixels, every gather issued before the first use) that writes the terms of the requested outputs, then the shared
 * owner once per requested output.
 * Time: tools/attr_interp_probe.py (profiles/attr_interp.json) measures every call at 32 and 64 faces of the full mesh at 200 x 200
 * beside the bytes each must move, a 512 MiB copy, fr_depth_interp_* on the same inputs and the same operators from stock torch ops
 * (DESIGN.md 4.4u). */
int fr_attr_interp_forward(const float* vertex, int vertex_pitch, const float* attr, int attr_pitch, const float* tri,
                           const float* tri_ind, int B, int nver, int ntri, int H, int W, float* out, void* stream);
int fr_attr_interp_backward(const float* grad, const float* vertex, int vertex_pitch, const float* attr, int attr_pitch,
                            const float* tri, const float* tri_ind, float* attr_grad, int attr_accumulate, float* vertex_grad,
                            int vertex_accumulate, int B, int nver, int ntri, int H, int W, int* records, unsigned int* partial,
                            void* stream);
int fr_mesh_vertex_normals_backward(const float* normal_grad, int grad_pitch, const float* vertex, int vertex_pitch, const float* tri,
                                    const int* adj_start, const int* adj_tri, int B, int nver, int ntri, double* h,
                                    float* vertex_grad, int out_pitch, int accumulate, void* stream);

/* The attribute interpolation backward's launch geometry (no GPU needed; the launcher reads the same function): out[6] as
 * fr_debug_depth_interp_bwd_geom; both outputs share it.  Used by tests/test_attr_interp_gpu.py. */
void fr_debug_attr_interp_bwd_geom(int B, int nver, int H, int W, int* out);

/* ---- soft coverage: an antialiased silhouette with an x, y backward (opt-in) ---------------------------------------------------------
 * Every gradient above holds tri_ind fixed and every plane is flat per triangle in the screen plane: when a face moves sideways or is
 * scaled in the image, no plane changes through x and y except by the slope of the interpolated depth.  These entry points are a
 * post-pass over a forward's tri_ind that gives the SILHOUETTE of the rendered face as a plane cov in [0, 1] -- 1 inside, +0 outside,
 * in between on the pixels either side of the face / background border -- with an exact gradient to the x and y rows of the vertices.
 * It is the pair construction differentiable rasterisers use for antialiasing, restricted to face-against-background.
 *   vertex [B,3,vertex_pitch] (vertex_pitch >= nver, as in the interpolated depth);  tri [3,ntri], float-stored ids;
 *   tri_ind, cov, cov_grad dense [B,H,W,1];  vertex_grad dense [B,3,nver].  Pixel (row j, column i) is the point X = (i, j).
 * NAMES.  The stream parameter is called `stream`, as in the Gram-form geometry loss above and for its reason;
 * tests/test_coverage_cpu.py holds these entry points' return codes.
 * WHICH PIXEL.  A pixel is OK exactly as in the interpolated depth (tri_ind names t in [0, ntri) and all three ids of t lie in
 * [0, nver)); NaN, -1, a value >= ntri or a bad id is not OK.  P_k = (x, y) of vertex[b][.][p_k].
 * ARITHMETIC.  Float64 on the widened fp32 inputs; every difference, product, sum and quotient is rounded on its own (no
 * contraction).  The neighbours of a pixel are visited in the order left, right, up, down; a neighbour outside the image does not
 * exist.
 * PAIR (c, n): c an OK pixel with triangle (P1, P2, P3), n a not-OK neighbour of c.
 *   e(A, B, X) = (Bx - Ax)(Xy - Ay) - (By - Ay)(Xx - Ax)
 *   area = e(P1, P2, P3); area == 0 or not finite: the pair is INERT.  Otherwise sigma = +-1 is its sign.
 *   for edge k = 1, 2, 3 = (P1,P2), (P2,P3), (P3,P1):   Fc = sigma e(A, B, c),   Fn = sigma e(A, B, n)
 *   edge k is a candidate iff Fn < 0 and Fc > Fn and s_k = Fc / (Fc - Fn) is finite
 *   s = the smallest s_k, the lowest k on a tie; no candidate: the pair is inert.   s^ = min(max(s, 0), 1)
 * s is the position along c -> n at which the segment leaves c's triangle.  The border sits at s^: the face covers s^ - 0.5 of n
 * beyond the pixel boundary, or leaves 0.5 - s^ of c uncovered.
 * FORWARD, from a = +0:
 *   OK pixel c:      for each not-OK neighbour with a non-inert pair:       a = a + max(0.5 - s^, 0);   cov = fl32(max(0, 1 - a))
 *   not-OK pixel u:  for each OK neighbour n with a non-inert pair (n, u):  a = a + max(s^ - 0.5, 0);   cov = fl32(min(1, a))
 * A pixel whose four neighbours share its state is exactly 1.0 or +0.  (tests/ref_coverage.py is this in numpy.)
 * BACKWARD.  tri_ind is held fixed; the fp32 roundings and the clamps count as the identity where they are inactive.  The call takes
 * G = (double)cov_grad and the forward's cov plane.  For an OK pixel c and each not-OK neighbour n, in order, whose pair is non-inert
 * with 0 < s < 1:
 *   q = 0;   s < 0.5 and cov(c) > 0:  q = q + G(c);   s > 0.5 and cov(n) < 1:  q = q + G(n)
 *   with the winning edge (A, B), D = Fc - Fn, and v one of (Ax, Ay, Bx, By):
 *     d e(X) / d v = (By - Xy,  Xx - Bx,  Xy - Ay,  Ax - Xx)
 *     d s / d v    = (sigma ((-Fn) d e(c)/d v + Fc d e(n)/d v)) / (D D)
 *   slot(vertex of v, row of v) = slot + q (d s / d v)          six float64 slots per pixel, each from +0, pair after pair
 * Each of the pixel's six x, y slots is rounded to fp32 once: these are its terms; its z terms are +0.  A pixel whose six terms are
 * all zero contributes nothing (no record).  Each (face, row, vertex) sum of terms is formed exactly as the interpolated depth's
 * backward forms its own (the same record planes, the same owner workgroups, csrc/fr_owner_scatter.h): 64-bit fixed point on a grid
 * of 2^(e - 39 + shift), integer addition in LDS, one rounding to fp32; no float atomics, bit-reproducible, independent of the launch
 * geometry; |result - exact sum| <= 2^-24 |sum| + n 2^(shift - 39) M for n terms, M the face's largest finite |term|.  A face with
 * a non-finite term takes fp32 LDS atomics, as there.  The z row is exactly +0 (accumulate 0).
 *   accumulate 0 / 1 and the workspace -- fr_coverage_backward_workspace_bytes(B, nver, H, W) = B H W 48 + B ceil(H W / 1024) 8
 *   bytes, 16-byte aligned, caller-owned, per call in flight -- are those of fr_depth_interp_backward.  The forward needs none.
 * LIMITS.  Only the face / background border is softened: an occlusion edge between two triangles of the face is not (both pixels
 * are OK, no pair exists).  A neighbouring triangle that covers part of the segment c -> n without winning a pixel centre is
 * ignored: the border is put where c's own triangle ends.
 * Checks, all before any HIP call, in the order and with the codes of fr_depth_interp_*: (1) a negative size, accumulate outside
 * {0, 1} or vertex_pitch < nver is FR_ERR_INVALID_ARG; (2) B == 0 or an empty image is FR_OK with nothing launched and nothing
 * written (so is the backward with nver == 0); (3) a NULL tri_ind, cov or vertex_grad -- or, where triangles exist, a NULL tri,
 * vertex, cov_grad or (backward) cov -- is FR_ERR_INVALID_ARG; ntri >= 2^24 or more than 2^31 - 1 pixels per face is
 * FR_ERR_UNSUPPORTED; (4) a workspace that is missing, too small or misaligned is FR_ERR_WORKSPACE.  With ntri == 0 the forward
 * writes +0 everywhere and the backward zeros (or, accumulate 1, nothing).  Nothing is allocated or synchronised; reentrant under the
 * rules at the top of this file.
 * Kernels (csrc/fr_coverage.hip): the forward is one lane per pixel in tiles of 32 x 8; the workgroup stages its tile of tri_ind with
 * a one-pixel halo in LDS as "triangle if OK, else -1" (OK depends on the triangle's ids, so a covered pixel costs three id gathers
 * there; an uncovered one none), and only a lane with a neighbour of the other state gathers vertices.  The backward is a records
 * pass over 1,024-pixel chunks in which only border pixels evaluate pairs and write term planes, then the shared owner.
 * Time: tools/coverage_probe.py (profiles/coverage.json) measures both at 64 and 32 faces of the full mesh at 200 x 200 beside
 * fr_depth_interp_forward / _backward on the same inputs and a 512 MiB copy.  MI355X, medians of 6 rounds of 40 calls: forward
 * 27.7 / 17.3 us beside the interpolated depth's 26.0 / 14.7 us, where it must move 31 / 16 MB = 5.8 / 2.9 us at the 5.3 TB/s that
 * run's copy reached (0.21 / 0.17 of it): the staged tile binds, not memory -- on a tri_ind of -1 everywhere it takes 13.6 / 7.9 us
 * where the interpolated depth's plain map takes 6.7 / 4.9 us; backward 92.2 / 53.6 us beside the interpolated depth's 75.1 / 42.5 us
 * (the same owners; a records pass that decides OK for four neighbours by id gathers of its own). */
int fr_coverage_forward(const float* vertex, int vertex_pitch, const float* tri, const float* tri_ind, int B, int nver, int ntri,
                        int H, int W, float* cov, void* stream);
size_t fr_coverage_backward_workspace_bytes(int B, int nver, int H, int W);
int fr_coverage_backward(const float* cov_grad, const float* cov, const float* vertex, int vertex_pitch, const float* tri,
                         const float* tri_ind, float* vertex_grad, int B, int nver, int ntri, int H, int W, int accumulate,
                         void* workspace, size_t ws_bytes, void* stream);

/* The soft-coverage backward's launch geometry (no GPU needed; the launcher reads the same function): out[6] as
 * fr_debug_depth_interp_bwd_geom.  Used by tests/test_coverage_cpu.py and tests/test_coverage_gpu.py. */
void fr_debug_coverage_bwd_geom(int B, int nver, int H, int W, int* out);

/* ---- landmarks ----------------------------------------------------------------------------------------------
 * The projections of K chosen vertices, their squared distance to 2D points of the picture, and the gradient of both with respect to
 * the parameters -- without the dense decode: the landmarks' basis rows are gathered once into a compact image, then one launch each
 * way per step (csrc/fr_landmark.hip).  Opt-in; no reference counterpart.
 *
 * Image (fr_landmark_basis_build; fr_landmark_basis_bytes bytes, 16-byte aligned; 0 for sizes that are not served).  fp32, with
 * Kt = n_shape + n_exp, R3 = 3 K and row r = 3 k + c = coordinate c of landmark k:
 *     part A  [Kt + 1][R3]  plane 0 = mu[c N + idx[k]], plane 1 + j = coefficient j of that row (shape first, then expression)
 *     part B  [R3][Kt]      the same coefficients row-major, directly behind part A
 * (the data twice: the forward's lane r walks the planes of A, the backward's lane j the rows of B, both coalesced).  mu [3N],
 * pc_shape [3N,n_shape], pc_exp [3N,n_exp] and idx [K] (int) are device pointers, the basis in the reference's blocked row order
 * (row c N + p = coordinate c of vertex p).  An id outside [0, N) gives a landmark whose mean and rows are all +0; duplicate ids
 * are legal.  A pure gather: bit-exact.
 *
 * Forward.  params [B, 7 + Kt] fp32; R_override NULL or [B,3,3] fp32; target NULL or [B,K,2] fp32; weight NULL (all 1), [K]
 * (weight_batch 0) or [B,K] (weight_batch 1); points [B,3,K] fp32; sse [B] float64, required when target is given, else ignored.
 * All arithmetic is float64 on the widened fp32 inputs, every product and every sum rounded on its own (no contraction):
 *     v_c  = mu_c, then + a_j U[c][j] for j ascending over the shape coefficients, then over the expression coefficients;
 *     R    = the fp32 matrix the dense decode uses (rotation_from_sincos of csrc/fr_decode_shared.h on the float64 sincos of the
 *            widened angles, rounded to fp32) or the override; widened;
 *     q_i  = f ((R_i0 v_0 + R_i1 v_1) + R_i2 v_2) + t_i;      x = q_0,  y = (im_size - q_1) - 1,  z = q_2;
 *     points = (x, y, z), each rounded to fp32 once;
 *     sse_b = sum over k ascending, from +0, of  w_k ((x - tx)(x - tx) + (y - ty)(y - ty))   with x, y BEFORE the fp32 rounding.
 * A landmark with w_k == 0 is skipped entirely (its target is not read: a NaN target under weight 0 changes nothing).
 *
 * Backward.  grad_points NULL or [B,3,K] fp32; grad_sse NULL or [B] float64 (read from the device; it needs target); at least one
 * of the two.  It saves nothing: v is recomputed from params in the forward's chain, with the same bits.
 *     g    = grad_points (or 0);  where w_k != 0:  s = grad_sse_b (2 w_k),  g_x = g_x + s (x - tx),  g_y = g_y + s (y - ty);
 *     dq   = (g_x, -g_y, g_z);    Rv_i = (R_i0 v_0 + R_i1 v_1) + R_i2 v_2;    (R^T dq)_c = (R_0c dq_0 + R_1c dq_1) + R_2c dq_2;
 *     grad t3d_i = sum_k dq_i;    grad f = sum_k ((dq_0 Rv_0 + dq_1 Rv_1) + dq_2 Rv_2);    G_ij = f sum_k dq_i v_j;
 *     grad a_j   = f sum over (k, c) ascending of (R^T dq)_c[k] U[k][c][j];
 *     angle a (pose_grad 1, no override):  sum over (i, j) row-major of G_ij dR_a[i][j], where dR_phi = (dR_pitch R_yaw) R_roll,
 *     dR_gamma = (R_pitch dR_yaw) R_roll, dR_theta = (R_pitch R_yaw) dR_roll in float64 with the 3-term dots of mat3_mul and the
 *     matrices of tests/ref_pose_backward.py::rotation_f64 (the sincos are the forward's float64 ones, not rounded to fp32).
 * Every sum is sequential from +0 in ascending order, in float64; each output is rounded to fp32 once.  grad_params [B, 7 + Kt]:
 * every element is written; with pose_grad 0 (the project's default) the angle columns are +0 and grad_R is untouched; under an
 * override with pose_grad 1, grad_R [B,3,3] = G (required then) and the angle columns are +0.  No workspace, no atomics:
 * bit-reproducible.
 *
 * Limits: n_shape + n_exp <= 256 and 1 <= K <= 1024.  Checks, all before any HIP call, in the order and with the codes of
 * fr_coverage_*: (1) a negative size, or weight_batch / pose_grad outside {0, 1}, is FR_ERR_INVALID_ARG; (2) B == 0 or K == 0 is
 * FR_OK with nothing launched; (3) a NULL params, points, grad_params or idx, a NULL basis matrix that has elements, a target without
 * sse, both gradients NULL, grad_sse without target, or pose_grad 1 under an override without grad_R is FR_ERR_INVALID_ARG; (4) a
 * size outside the limits is FR_ERR_UNSUPPORTED; (5) an image that is missing, too small or not 16-byte aligned is
 * FR_ERR_WORKSPACE.  Nothing is allocated or synchronised; reentrant under the rules at the top of this file.
 * Kernels: one workgroup per face; the landmarks go through LDS in chunks of 256 in ascending order.  The forward gives a lane to
 * each (k, c) for the Kt-long chain, then one to each landmark for the projection and its sse term, and lane 0 adds the terms.  The
 * backward recomputes v the same way, forms dq, dq . Rv and R^T dq per landmark, and then gives one lane to each coefficient
 * (walking part B) and one to each of the 13 pose sums; a lane carries its sum from chunk to chunk.
 * Time: tools/landmark_probe.py (profiles/landmark.json) measures both at 64 and 32 faces of the full model (199 + 29 coefficients,
 * K = 68; a 373 KB image) beside the dense route to the same 68 points in the same run.  MI355X, medians of 6 rounds of 40 calls:
 * forward 10.1 / 10.1 us, backward 17.0 / 17.0 us -- the same at either batch: one workgroup per face, latency of the 228-long
 * float64 chain and of the launch, not bytes.  The autograd operator forward + backward (nets/losses.py::landmark_loss) takes 208 /
 * 136 us of mostly host time (133 us in the quiet rounds at 64 faces) where vertices_transform(pose_grad=True) -> index_select ->
 * the same loss -> backward takes 338 / 294 us, and holds 62 / 32 KB at its peak where the dense route holds 109 / 55 MB beside the
 * 154 MB basis image. */
size_t fr_landmark_basis_bytes(int K, int n_shape, int n_exp);
int fr_landmark_basis_build(const float* mu, const float* pc_shape, const float* pc_exp, const int* idx, int N, int n_shape,
                            int n_exp, int K, void* lbasis, size_t bytes, void* stream);
int fr_landmark_forward(const float* params, const void* lbasis, size_t lbasis_bytes, const float* R_override, const float* target,
                        const float* weight, int weight_batch, int B, int K, int n_shape, int n_exp, float im_size, float* points,
                        double* sse, void* stream);
int fr_landmark_backward(const float* grad_points, const double* grad_sse, const float* params, const void* lbasis,
                         size_t lbasis_bytes, const float* R_override, const float* target, const float* weight, int weight_batch,
                         int B, int K, int n_shape, int n_exp, float im_size, float* grad_params, float* grad_R, int pose_grad,
                         void* stream);

/* ---- landmark solver ----------------------------------------------------------------------------------------
 * One damped Gauss-Newton (Levenberg-Marquardt) step of the landmark term per face, in one launch (csrc/fr_landmark_solve.hip): the
 * term is a small nonlinear least-squares problem -- 2 K residuals, at most 6 + Kt unknowns -- whose parameters live on scales from
 * 1e-3 (f) to 1e4 (shape), which a scale-free second-order step covers in a handful of iterations.  Opt-in; no reference counterpart.
 *
 * Inputs per face b.  params [B, 7 + Kt] fp32 in the layout [phi, gamma, theta, tx, ty, tz, f | shape | exp]; the image of
 * fr_landmark_basis_build; target [B,K,2] fp32; weight NULL, [K] or [B,K] as in fr_landmark_forward (a landmark of weight 0 is
 * skipped entirely and its target is never read: it may be NaN); ridge [Kt] fp32 >= 0 or NULL (= 0); center [Kt] fp32 or NULL (= 0);
 * damp [B] float64 >= 0 or NULL (= 0), read from the device; pose_mask: bit i set = pose column i is fitted (bit 5, tz, is refused:
 * its column is identically zero; tz is not read); fit_coef 0 or 1: the Kt coefficients are fitted.  At least one column is fitted.
 * The unknowns, P of them, are the fitted pose columns in parameter order, then the coefficients.
 *
 * The mathematics, in float64 on the widened fp32 inputs, every product and every sum rounded on its own (no contraction):
 *     v, R, Rv_i, x, y  exactly the forward's (above): x = f Rv_0 + tx, y = (im_size - (f Rv_1 + ty)) - 1, before any fp32 rounding;
 *     residual rows     row 2 k:  r = x - target_x;   row 2 k + 1:  r = y - target_y;
 *     F                 = sse + [fit_coef] prior;  sse the forward's sum, bit for bit;  prior = sum over j ascending, from +0, of
 *                         ridge_j ((a_j - center_j) (a_j - center_j));
 *     J                 coefficient j: (f (R_0 . U_kj), -(f (R_1 . U_kj))), R_i . U = (R_i0 U_0 + R_i1 U_1) + R_i2 U_2;
 *                       tx: (1, 0);  ty: (0, -1);  f: (Rv_0, -Rv_1);
 *                       angle a: (f (dR_a v)_0, -(f (dR_a v)_1)) with the dR_a of the backward (above) and the same 3-term dots;
 *                       a landmark of weight 0 has rows and residuals of exact +0;
 *     H = J^T W J + diag(ridge) (the ridge on the coefficient block only);   g = J^T W r + ridge (a - center);   D = diag(J^T W J);
 *     (H + damp_b D) delta = -g  by Cholesky.
 * Summation orders.  Every sum that touches a pose column, g and D are sequential float64 sums from +0 over the rows ascending: the
 * term of (J^T W J)_ij, i >= j in the order of the unknowns, is (w J[row][i]) J[row][j]; that of (J^T W r)_i is (w J[row][i]) r[row];
 * g_j = that sum + ridge_j (a_j - center_j).  The coefficient-coefficient block is formed on v_mfma_f64_16x16x4_f64, lower triangle
 * only, operand A = J[row][i], operand B = w J[row][j]: 16 rows (8 landmarks) at a time ascending, four rows per instruction ascending,
 * accumulated in registers from +0 -- its bits are a function of (K, Kt) and the inputs, not of B or the device; how the instruction
 * rounds inside its four products is the hardware's.  H_jj = (J^T W J)_jj + ridge_j;  A_ii = H_ii + damp D_ii.
 * Cholesky, on the packed lower triangle with -g as an extra row P: for c ascending, the pivot d = A_cc must be positive and finite;
 * l = sqrt(d); A_ic = A_ic / l for i = c + 1 .. P; A_ij = A_ij - A_ic A_jc for c < j <= i <= P (no (P, P)).  Row P ends as
 * y = L^-1 (-g).  Then for c descending: delta_c = y_c / l_c;  y_j = y_j - L_cj delta_c for j < c.
 * Prediction: q_i = sum over j ascending of H_ij delta_j;  e_i = delta_i (2 g_i + q_i);  cost_1 = F + (sum over i ascending of e_i).
 *
 * Outputs, every element written on every call that launches: delta [B, 7 + Kt] float64 (columns that are not fitted are +0);
 * cost [B,2] float64 = (F at params, the quadratic model's prediction F + 2 g.delta + delta.H delta); ok [B] int32.  A face whose
 * factorisation meets a pivot that is not positive and finite, or whose F, prediction or delta is not finite, reports ok = 0,
 * delta = +0 and cost[b][1] = cost[b][0]; no other face changes by a bit.  That covers f = 0 with an angle fitted, all weights 0 with
 * a pose column fitted, and any non-finite input that is read.  A face's outputs are a function of that face's inputs and of
 * (K, n_shape, n_exp, pose_mask, fit_coef) alone: not of B, of its place in the batch or of the device.  No atomics.
 *
 * Workspace: fit_coef calls only (with Kt > 0; fr_landmark_solve_workspace_bytes, 16-byte aligned; 0 for sizes not served: B < 1, a
 * negative count, Kt > 256).  Per face, with Pm = 6 + Kt, (2 (Pm (Pm + 1) / 2) + Pm) float64 rounded up to even: the augmented
 * triangle, element (i, j) at i (i + 1) / 2 + j, rows 0 .. P, then at offset Pm (Pm + 1) / 2 + Pm the packed copy of H that the
 * prediction reads (220 KB + 220 KB at P = 234: more than the 160 KB of LDS, so the factorisation runs in the caller's memory, from the
 * face's one workgroup, with block barriers between dependent column steps).  A pose-only call forms and solves its system of at most
 * 6 x 6 in LDS and takes no workspace (NULL is fine).
 *
 * Checks, all before any HIP call, in the order of fr_landmark_forward: (1) a negative size, weight_batch or fit_coef outside {0, 1},
 * a pose_mask with bit 5 or a bit above 6, or nothing to fit (an empty mask without fit_coef, or with Kt == 0) is
 * FR_ERR_INVALID_ARG; (2) B == 0 or K == 0 is FR_OK with nothing launched and nothing written; (3) a NULL params, target, delta, cost
 * or ok is FR_ERR_INVALID_ARG; (4) K or Kt outside the landmark limits is FR_ERR_UNSUPPORTED; (5) a missing, short or misaligned
 * image, then -- for a fit_coef call -- workspace, is FR_ERR_WORKSPACE.  Nothing is allocated or synchronised.
 * Time: tools/landmark_solve_probe.py (profiles/landmark_solve.json) measures a step at 64 and 32 faces of the full model (199 + 29
 * coefficients, K = 68) beside the same step in stock torch float64 (einsum Jacobian and normal matrix, linalg.cholesky,
 * cholesky_solve) in the same run.  MI355X, medians of 6 rounds of 20 calls: the pose-only step about 23 us at either batch against
 * about 810 us; the step with the coefficients (P = 234) about 1.5 ms against 1.6 - 1.7 ms -- only a tenth faster: it is the latency
 * of 234 dependent column steps through memory, two block barriers each, not arithmetic (the matrix-core block is a few percent of
 * it); a panel-blocked factorisation is the next step. */
size_t fr_landmark_solve_workspace_bytes(int B, int n_shape, int n_exp);
int fr_landmark_solve_step(const float* params, const void* lbasis, size_t lbasis_bytes, const float* target, const float* weight,
                           int weight_batch, const float* ridge, const float* center, const double* damp, int pose_mask, int fit_coef,
                           int B, int K, int n_shape, int n_exp, float im_size, double* delta, double* cost, int* ok, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- contour landmarks --------------------------------------------------------------------------------------
 * Sliding correspondences for the landmarks that mark the face's visible outline: which vertex lies under such a 2D point depends on
 * the pose, so the point is given a LINE of M candidate vertices and, per face, one candidate is picked (csrc/fr_landmark_contour.hip).
 * Opt-in; no reference counterpart.  No other kernel changes: the compact image is fr_landmark_basis_build's, over Kf fixed ids
 * followed by C lines of M candidate ids, K = Kf + C M; candidate (c, m) is landmark k = Kf + c M + m.  This call writes a per-face
 * weight [B,K] and target [B,K,2] -- the line's weight on its winner, +0 on the losers -- and fr_landmark_forward / _backward /
 * fr_landmark_solve_step then run over K with weight_batch = 1: they skip a landmark of weight 0 entirely.  The selection is held
 * fixed in every derivative, as tri_ind is elsewhere.
 *
 * Inputs.  params [B, 7 + Kt], the image and R_override as in fr_landmark_forward.  fixed_target NULL or [B,Kf,2]; fixed_weight NULL
 * (all 1), [Kf] (fixed_weight_batch 0) or [B,Kf] (1); line_target NULL or [B,C,2]; line_weight NULL (all 1), [C] (line_weight_batch 0)
 * or [B,C] (1); line_dir NULL or [C,2]; all fp32.  rule 0 (nearest) needs line_target, rule 1 (extreme) line_dir.
 *
 * Decode.  x and y of every candidate are the forward's float64 values BEFORE the fp32 rounding: the same prologue, chain and
 * expressions (csrc/fr_landmark_shared.h), so v and R carry the forward's bits by construction.  Float64 on the widened fp32 inputs,
 * every product and every sum rounded on its own.
 *     rule 0 (nearest):  d = (x - tx)(x - tx) + (y - ty)(y - ty) against the line's target; for m ascending a candidate wins if
 *                        d < best, best starting at +inf: ties go to the lowest m, and a NaN or +inf d never wins;
 *     rule 1 (extreme):  s = dir_x x + dir_y y (two products, one sum); a candidate wins if s > best, best starting at -inf.  This is
 *                        the model's own occluding contour along the line: it makes synthetic ground truth, and serves as a
 *                        "landmark marching" rule.
 * A line whose weight is 0 is not looked at (its target may be NaN) and has no winner.  A line with no winner gives sel = -1,
 * line_points = +0 and weight +0 on all its candidates.
 *
 * Outputs, every element written on every call that launches: sel [B,C] int32 the winning m; line_points [B,C,2] fp32 the winner's
 * (x, y), each rounded to fp32 once; target [B,K,2] or NULL: its fixed part a bit copy of fixed_target, every candidate of a line
 * carrying that line's target (bit copies); weight [B,K] or NULL: the fixed part fixed_weight broadcast (1 when NULL), the line's
 * weight on its winner (1 when NULL), +0 elsewhere.  A face's outputs are a function of that face's inputs and of (Kf, C, M, n_shape,
 * n_exp, rule) alone.  No atomics, no workspace: bit-reproducible.
 *
 * Kernel: one workgroup per face; the landmarks go through LDS in the forward's chunks of 256 (boundaries at multiples of 256 of k;
 * what lies below Kf is not decoded).  A lane per (k, c) runs the chain, a lane per candidate projects and scores, and lane c walks
 * line c's candidates of the chunk in ascending m, carrying (best, m, x, y) from chunk to chunk -- a line may straddle a boundary.
 *
 * Limits: the landmark limits (n_shape + n_exp <= 256, 1 <= K <= 1024), M >= 1 and C <= 256.  Checks, all before any HIP call, in the
 * order and with the codes of fr_landmark_forward: (1) a negative size, rule outside {0, 1} or a *_batch flag outside {0, 1} is
 * FR_ERR_INVALID_ARG; (2) B == 0 or C == 0 is FR_OK with nothing launched; (3) a NULL params, sel or line_points, rule 0 without
 * line_target, rule 1 without line_dir, a target output without line_target, or a target output with Kf > 0 and no fixed_target is
 * FR_ERR_INVALID_ARG; (4) a size outside the limits is FR_ERR_UNSUPPORTED; (5) an image that is missing, too small or not 16-byte
 * aligned is FR_ERR_WORKSPACE.  Nothing is allocated or synchronised.
 * Time: tools/landmark_contour_probe.py (profiles/landmark_contour.json) measures the call at 64 and 32 faces of the full model
 * with Kf = 52 and 16 lines of 24 candidates (K = 436).  MI355X, medians of 6 rounds of 20 calls: 27.0 / 27.0 us, beside
 * fr_landmark_forward at 25.8 / 25.5 us over the same K and 10.2 / 10.1 us over K = 68 -- one workgroup per face and the latency of
 * two chunks of the 228-long chain, flat in the batch.  The solver over the masked K: 68 us (pose only) and 2.2 ms (with the
 * coefficients) against 22 us and 1.5 ms over K = 68. */
int fr_landmark_contour_select(const float* params, const void* lbasis, size_t lbasis_bytes, const float* R_override,
                               const float* fixed_target, const float* fixed_weight, int fixed_weight_batch, const float* line_target,
                               const float* line_weight, int line_weight_batch, const float* line_dir, int rule, int B, int Kf, int C,
                               int M, int n_shape, int n_exp, float im_size, int* sel, float* line_points, float* target, float* weight,
                               void* stream);

/* ---- test hook ---------------------------------------------------------------------------------------------
 * The screen-bin geometry the forward launcher chooses for a shape (no GPU needed): out = {rows per strip, strips,
 * triangle segments, 1 if the binned path covers the shape else 0 (the strip-scan fallback runs)}.  rows_override > 0
 * plays the FR_RENDER_ROWS tuning knob.  Used by tests/test_capi_cpu.py. */
void fr_debug_render_geom(int B, int ntri, int H, int W, int rows_override, int* out);

/* The decode-backward launch geometry under the current FR_BWD_CHUNKS / FR_BWD_CB (no GPU needed): out[7] = {vertex groups of
 * 16 per fused workgroup, fused workgroups, CB of a 64-face pass of min(nbatch, 64) faces, waves per fused workgroup, rows per
 * reference-layout GEMM workgroup, GEMM workgroups, prepass workgroups}.  Used by tests/test_decode_backward_bounds_gpu.py to
 * derive its rounding-error bounds and by tests/test_capi_cpu.py. */
void fr_debug_decode_bwd_geom(int nbatch, int N, int n_shape, int n_exp, int* out);

/* The decode-forward launch decision under the current FR_DECODE_* knobs on a part of `cus` compute units (no GPU needed; the
 * launcher of fr_decode_3dmm calls the same function, with the device's CU count, and takes its kernel template arguments from
 * the table this reports from): out[0] = passes, then 12 ints per pass = {first column, live columns, kernel (0 = generic
 * decode_kernel, 1 = ring schedule of the 13 + 2 group shape), NBW (16-column blocks per work item), waves per workgroup, MB
 * (columns the pass's LDS image holds: 64 or 128), halves (items per tile), NT (non-temporal basis stream), PRIO (ranked waves),
 * TR (transposed accumulators), dynamic LDS bytes, workgroups}.  `out` must hold 1 + 12 * ceil(B / 64) ints.  Returns FR_OK
 * (out[0] = 0 for B = 0 or N = 0), FR_ERR_INVALID_ARG (a negative size, cus < 1, NULL), or FR_ERR_UNSUPPORTED exactly where
 * fr_decode_3dmm does (a basis whose 64-column LDS image exceeds 160 KiB).  Used by tests/test_decode_geom_cpu.py and by
 * tests/test_decode_forward_edges_gpu.py to pick shapes that reach a geometry. */
int fr_debug_decode_geom(int B, int N, int n_shape, int n_exp, int cus, int* out);

/* The same for the Q30 decode (fr_decode_3dmm_q30_lv and the decode phase of fr_decode_render_forward_q30) under the current
 * FR_DECODE_IMPL / FR_Q30_SCHED: its launcher calls the same function, with the device's CU count (under FR_DECODE_CUS), and
 * takes its kernel template arguments from the table this reports from.  out[0] = passes (one per 64 columns), then 10 ints per
 * pass = {first column, live columns, kernel (0 = generic decode_q_kernel, 1 = ring schedule of the 15-group shape), NBW
 * (16-column blocks per wave), waves per workgroup, H2 (waves that share a tile: 2 = its two 32-column halves on neighbouring
 * waves), ring depth in fragments (0: generic), decode launches of the pass (2 for a generic pass of 3-4 column blocks; the
 * staging launch is not counted), dynamic LDS bytes, workgroups}; a wave owns whole tiles, waves / H2 of them in work per
 * workgroup.  `out` must hold 1 + 10 * ceil(B / 64) ints.  Returns FR_OK (out[0] = 0 for B = 0 or N = 0), FR_ERR_INVALID_ARG
 * (a negative size, cus < 1, levels not 7 / 5 / 4, NULL) or FR_ERR_UNSUPPORTED (n_shape + n_exp > 512).  Used by
 * tests/test_decode_geom_cpu.py and by tests/test_decode_q30_edges_gpu.py to pick shapes that reach a geometry. */
int fr_debug_decode_q_geom(int B, int N, int n_shape, int n_exp, int levels, int cus, int* out);

/* The decode kernels' work distribution, evaluated on the host through the function the kernels call (wave_work / tile_walk of
 * csrc/fr_decode_shared.h): visits[tile * halves + half] = how many waves of a launch of `grid` workgroups of `waves` waves take
 * the item (tile, half), for tile < tiles.  Every entry is 1 for every geometry fr_debug_decode_geom can return: waves / halves
 * tiles are in work per workgroup, and when halves does not divide waves (FR_DECODE_NBW=1 with 33-48 columns: 3 halves on 16
 * waves) the surplus waves take no work.  FR_ERR_INVALID_ARG for tiles < 0, halves < 1, halves > waves or grid < 1. */
int fr_debug_decode_walk(int tiles, int waves, int halves, int grid, int* visits);

/* The pose-moment launch geometry (no GPU needed; a function of N alone -- B is accepted and ignored): out[4] = {chunk length in
 * vertices, chunks per face, threads per workgroup, longest chain of rounded fp32 additions behind one element of a chunk
 * record}; all zero for N <= 0.  Used by tests/test_pose_backward_gpu.py to derive its bounds. */
void fr_debug_pose_bwd_geom(int B, int N, int* out);

/* The render-backward launch geometry (no GPU needed; the launcher reads the same function): out[6] = {owner workgroups
 * per face, vertices per owner, shift (resolution bits given up above 2^20 pixels), 1,024-pixel record chunks of the
 * workspace variant, dynamic LDS bytes of an owner workgroup, 1 if the block -> (face, owner) map is the one that keeps a
 * face's owners on one XCD (batch a multiple of 8) else 0}; all zero for a shape that launches no kernel.  Used by
 * tests/test_render_backward_exact_gpu.py to assert that a case reaches the geometry it was written for, and by
 * tests/test_capi_cpu.py. */
void fr_debug_render_bwd_geom(int B, int nver, int H, int W, int* out);

/* The kernels divide by 3.0f (render_depth_op.cc:217, 223, 361) through a 3-instruction exact sequence: this hook
 * compares it with x / 3.0f on the fp32 bit patterns [first, first + count) and writes the number of differing results
 * to the device word `mismatches`.  Used by tests/test_render_gpu.py (all 2^32 patterns). */
int fr_debug_div3_sweep(unsigned long long first, unsigned long long count, unsigned long long* mismatches,
                        void* hip_stream);

/* Measurement hook (bench.py `clock_GHz_held`; no reference counterpart): `blocks` 1,024-thread workgroups each issue
 * `iters` x 6 v_mfma_f32_16x16x4_f32 per wave (the decode's matrix instruction at the decode's occupancy) and write
 * ticks[2 b] = shader-clock ticks and ticks[2 b + 1] = 100 MHz ticks their loop took (device buffer of 2 * blocks 64-bit
 * words): clock held = 0.1 GHz * ticks[2 b] / ticks[2 b + 1]. */
int fr_debug_clock_probe(unsigned long long* ticks, int blocks, int iters, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FR_HOTPATH_H_ */
