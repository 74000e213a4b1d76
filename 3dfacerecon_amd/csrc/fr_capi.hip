// extern "C" entry points declared in include/fr_hotpath.h: argument validation (the OP_REQUIRES checks of
// render_depth_op.cc:408-418, 498-503 re-stated) and dispatch to the gfx950 launchers.
#include <atomic>
#include <mutex>

#include "fr_common.h"
#include "fr_landmark_shared.h"

// ---- option table: environment read once, fr_set_option afterwards ------------------------------------------------------
namespace {
struct OptDesc {
    const char* name;
    int dflt;
    const char* word;  // a non-numeric spelling of value 1 ("loop", "scan"), or null
};
const OptDesc kOpts[fr::OPT_COUNT] = {
    {"FR_DECODE_IMPL", 0, "loop"}, {"FR_DECODE_WIDE", 1, nullptr}, {"FR_DECODE_NBW", 0, nullptr},
    {"FR_DECODE_WAVES", 16, nullptr}, {"FR_DECODE_NT", -1, nullptr}, {"FR_RESOLVE_OPT", 2, nullptr},
    {"FR_EMIT_FILTER", 3, nullptr}, {"FR_RENDER_IMPL", 0, "scan"}, {"FR_RESOLVE_BLOCK", 0, nullptr},
    {"FR_RENDER_ROWS", 0, nullptr}, {"FR_DECODE_STORE", 0, nullptr},
    {"FR_BWD_CHUNKS", 256, nullptr}, {"FR_BWD_CB", 0, nullptr}, {"FR_EMIT_ORDER", -1, nullptr},
    {"FR_Q30_SCHED", 0, nullptr}, {"FR_DECODE_CUS", 0, nullptr},
};
std::atomic<int> g_opt[fr::OPT_COUNT];
std::once_flag g_opt_once;
void opts_init() {
    for (int i = 0; i < fr::OPT_COUNT; i++) {
        int v = kOpts[i].dflt;
        const char* e = getenv(kOpts[i].name);
        if (e && *e) v = (kOpts[i].word && !strcmp(e, kOpts[i].word)) ? 1 : atoi(e);
        g_opt[i].store(v, std::memory_order_relaxed);
    }
}
int opt_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < fr::OPT_COUNT; i++)
        if (!strcmp(name, kOpts[i].name)) return i;
    return -1;
}
}  // namespace

int fr::opt(fr::Opt o) {
    std::call_once(g_opt_once, opts_init);
    return g_opt[o].load(std::memory_order_relaxed);
}

extern "C" {

int fr_set_option(const char* name, int value) {
    const int i = opt_index(name);
    if (i < 0) return FR_ERR_INVALID_ARG;
    std::call_once(g_opt_once, opts_init);
    g_opt[i].store(value, std::memory_order_relaxed);
    return FR_OK;
}

int fr_get_option(const char* name, int* value) {
    const int i = opt_index(name);
    if (i < 0 || !value) return FR_ERR_INVALID_ARG;
    *value = fr::opt((fr::Opt)i);
    return FR_OK;
}

#ifndef FR_SRC_HASH
#define FR_SRC_HASH "unhashed"
#endif
// the build identity: _lib.py refuses a library whose source hash differs from the tree's
const char* fr_version(void) { return "fr_hotpath 0.4 (gfx950) src=" FR_SRC_HASH; }

const char* fr_strerror(int code) {
    switch (code) {
        case FR_OK: return "ok";
        case FR_ERR_INVALID_ARG: return "invalid argument";
        case FR_ERR_WORKSPACE: return "workspace / packed buffer too small";
        case FR_ERR_LAUNCH: return "HIP launch or runtime error";
        case FR_ERR_UNSUPPORTED: return "size not supported by the gfx950 kernels";
        default: return "unknown error";
    }
}

size_t fr_render_depth_workspace_bytes(int B, int nver, int ntri, int H, int W) {
    (void)nver;
    if (B < 0 || ntri < 0 || H < 0 || W < 0) return 0;
    return fr_render_workspace_bytes_impl(B, ntri, H, W);  // per-segment hit records + bucket offsets
}

// ---- the render forward's argument checks, stated once ------------------------------------------------------------------------
// Every entry point that ends in a render forward makes them in this order: render_shape_check, its own "nothing to render"
// return, render_call_check.
static int render_shape_check(int B, int nver, int ntri, int H, int W, int C, int tex_batch) {
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (C != 3) return FR_ERR_INVALID_ARG;                         // render_depth_op.cc:418
    if (tex_batch != 1 && tex_batch != B) return FR_ERR_INVALID_ARG;
    return FR_OK;
}

enum RenderKind {
    RENDER_PLAIN,        // render_depth
    RENDER_LAYER,        // the fused rendering layer: it also refuses an empty mesh (nothing to fuse: use the plain op)
    RENDER_LAYER_SERVED  // the fused layer behind a decode: whatever fr_rendering_layer_supported does not serve is refused
};
// outs: the entry point's own outputs (and the layer's im_gray) are all there.  vertex: the caller's, or the decode's hand-off.
static int render_call_check(bool outs, const float* vertex, const float* tri, const float* texture, int B, int nver, int ntri,
                             int H, int W, size_t ws_bytes, RenderKind kind) {
    if (!outs) return FR_ERR_INVALID_ARG;
    if (ntri > 0 && (!tri || (nver > 0 && (!vertex || !texture)))) return FR_ERR_INVALID_ARG;
    if (kind == RENDER_LAYER_SERVED) {
        if (!fr_rendering_layer_supported(B, nver, ntri, H, W)) return FR_ERR_UNSUPPORTED;
    } else {
        if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;              // float-stored ids stop being exact
        if (kind == RENDER_LAYER && (ntri == 0 || nver == 0)) return FR_ERR_UNSUPPORTED;
    }
    if (ws_bytes < fr_render_depth_workspace_bytes(B, nver, ntri, H, W)) return FR_ERR_WORKSPACE;
    return FR_OK;
}

int fr_render_depth_forward(const float* vertex, const float* tri, const float* texture, int B, int nver, int ntri,
                            int H, int W, int C, int tex_batch, float* depth, float* tex_img, float* normal,
                            float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream) {
    int rc = render_shape_check(B, nver, ntri, H, W, C, tex_batch);
    if (rc != FR_OK || (size_t)B * H * W == 0) return rc;          // empty batch / image: nothing to write
    rc = render_call_check(depth && tex_img && normal && tri_ind, vertex, tri, texture, B, nver, ntri, H, W, ws_bytes, RENDER_PLAIN);
    if (rc != FR_OK) return rc;
    return fr_launch_render_forward(vertex, tri, texture, B, nver, ntri, H, W, tex_batch, depth, tex_img, normal,
                                    tri_ind, workspace, ws_bytes, (hipStream_t)hip_stream);
}

int fr_render_depth_forward_phases(const float* vertex, const float* tri, const float* texture, int B, int nver, int ntri,
                                   int H, int W, int C, int tex_batch, float* depth, float* tex_img, float* normal,
                                   float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream, int phases) {
    if (phases < 1 || phases > 7) return FR_ERR_INVALID_ARG;
    int rc = render_shape_check(B, nver, ntri, H, W, C, tex_batch);
    if (rc != FR_OK || (size_t)B * H * W == 0) return rc;
    rc = render_call_check(depth && tex_img && normal && tri_ind, vertex, tri, texture, B, nver, ntri, H, W, ws_bytes, RENDER_PLAIN);
    if (rc != FR_OK) return rc;
    return fr_launch_render_forward_phases(vertex, tri, texture, B, nver, ntri, H, W, tex_batch, depth, tex_img, normal,
                                           tri_ind, workspace, ws_bytes, (hipStream_t)hip_stream, phases);
}

static int rendering_layer_checked(const float* vertex, const float* tri, const float* texture, const float* im_gray, int B,
                                   int nver, int ntri, int H, int W, int tex_batch, float* net_input, float* depth_img,
                                   float* depth, float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream, int phases) {
    if (phases < 1 || phases > 7) return FR_ERR_INVALID_ARG;
    int rc = render_shape_check(B, nver, ntri, H, W, 3, tex_batch);
    if (rc != FR_OK || (size_t)B * H * W == 0) return rc;
    rc = render_call_check(net_input && depth_img && depth && tri_ind && im_gray, vertex, tri, texture, B, nver, ntri, H, W,
                           ws_bytes, RENDER_LAYER);
    if (rc != FR_OK) return rc;
    return fr_launch_rendering_layer(vertex, tri, texture, im_gray, B, nver, ntri, H, W, tex_batch, net_input, depth_img,
                                     depth, tri_ind, workspace, ws_bytes, (hipStream_t)hip_stream, phases);
}

int fr_rendering_layer_forward(const float* vertex, const float* tri, const float* texture, const float* im_gray, int B,
                               int nver, int ntri, int H, int W, int tex_batch, float* net_input, float* depth_img,
                               float* depth, float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream) {
    return rendering_layer_checked(vertex, tri, texture, im_gray, B, nver, ntri, H, W, tex_batch, net_input, depth_img, depth,
                                   tri_ind, workspace, ws_bytes, hip_stream, 7);
}

int fr_rendering_layer_forward_phases(const float* vertex, const float* tri, const float* texture, const float* im_gray, int B,
                                      int nver, int ntri, int H, int W, int tex_batch, float* net_input, float* depth_img,
                                      float* depth, float* tri_ind, void* workspace, size_t ws_bytes, void* hip_stream,
                                      int phases) {
    return rendering_layer_checked(vertex, tri, texture, im_gray, B, nver, ntri, H, W, tex_batch, net_input, depth_img, depth,
                                   tri_ind, workspace, ws_bytes, hip_stream, phases);
}

static int render_backward_checked(const float* depth_grad, const float* tri, const float* tri_ind, float* vertex_grad,
                                   int B, int nver, int ntri, int H, int W, void* workspace, size_t ws_bytes,
                                   void* hip_stream) {
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if ((size_t)B * nver == 0) return FR_OK;
    if (!vertex_grad) return FR_ERR_INVALID_ARG;
    if ((size_t)B * H * W > 0 && ntri > 0 && (!depth_grad || !tri || !tri_ind)) return FR_ERR_INVALID_ARG;
    return fr_launch_render_backward(depth_grad, tri, tri_ind, vertex_grad, B, nver, ntri, H, W, workspace, ws_bytes,
                                     (hipStream_t)hip_stream);
}

int fr_render_depth_backward(const float* depth_grad, const float* tri, const float* tri_ind, float* vertex_grad,
                             int B, int nver, int ntri, int H, int W, void* hip_stream) {
    return render_backward_checked(depth_grad, tri, tri_ind, vertex_grad, B, nver, ntri, H, W, nullptr, 0, hip_stream);
}

size_t fr_render_depth_backward_workspace_bytes(int B, int H, int W) {
    return (B > 0 && H > 0 && W > 0) ? fr_render_backward_workspace_bytes_impl(B, H, W) : 0;
}

int fr_render_depth_backward_ws(const float* depth_grad, const float* tri, const float* tri_ind, float* vertex_grad,
                                int B, int nver, int ntri, int H, int W, void* workspace, size_t ws_bytes,
                                void* hip_stream) {
    // a workspace that is too small or not 16-byte aligned is never touched: the launcher takes the plain variant (same bits)
    return render_backward_checked(depth_grad, tri, tri_ind, vertex_grad, B, nver, ntri, H, W, workspace, ws_bytes,
                                   hip_stream);
}

size_t fr_decode_packed_basis_bytes(int N, int n_shape, int n_exp) {
    if (N < 0 || n_shape < 0 || n_exp < 0) return 0;
    return fr_packed_basis_bytes(N, n_shape, n_exp);
}

int fr_decode_pack_basis(const float* mu, const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp,
                         void* packed, size_t packed_bytes, void* hip_stream) {
    if (N < 0 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if (packed_bytes < fr_packed_basis_bytes(N, n_shape, n_exp)) return FR_ERR_WORKSPACE;
    if (N == 0) return FR_OK;
    if (!mu || !packed || (n_shape > 0 && !pc_shape) || (n_exp > 0 && !pc_exp)) return FR_ERR_INVALID_ARG;
    if (((uintptr_t)packed & 15) != 0) return FR_ERR_INVALID_ARG;
    return fr_launch_pack_basis(mu, pc_shape, pc_exp, N, n_shape, n_exp, packed, (hipStream_t)hip_stream);
}

// what fr_launch_decode reads: the parameters and a 16-byte aligned image
static int decode_inputs_check(const float* params, const void* packed_basis) {
    if (!params || !packed_basis) return FR_ERR_INVALID_ARG;
    if (((uintptr_t)packed_basis & 15) != 0) return FR_ERR_INVALID_ARG;
    return FR_OK;
}

int fr_decode_3dmm(const float* params, const void* packed_basis, const float* R_override, int B, int N, int n_shape,
                   int n_exp, float im_size, float* vertex_proj, void* hip_stream) {
    if (B < 0 || N < 0 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if ((size_t)B * N == 0) return FR_OK;
    if (!vertex_proj || decode_inputs_check(params, packed_basis) != FR_OK) return FR_ERR_INVALID_ARG;
    return fr_launch_decode(params, packed_basis, R_override, B, N, n_shape, n_exp, im_size, vertex_proj, N,
                            (hipStream_t)hip_stream);
}

// ---- fused decode -> render step ---------------------------------------------------------------------------------------
int fr_decode_render_vertex_pitch(int N) { return N <= 0 ? 0 : (N + 31) & ~31; }

size_t fr_decode_render_vertex_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * 3 * (size_t)fr_decode_render_vertex_pitch(N) * sizeof(float);
}

// The prologue of the three decode -> render entry points: phase bits, sizes, the empty batch, the hand-off buffer.  Returns
// true when the entry point goes on; otherwise *rc is its answer (FR_OK for an empty batch).
// What follows it differs, and is kept as it is: fr_decode_rendering_layer_forward makes ALL its remaining checks (decode
// inputs, then the layer's) before it enqueues anything; fr_decode_render_forward and fr_decode_render_forward_q30 check the
// decode's inputs, ENQUEUE THE DECODE, and only then look at the render's arguments -- a bad render argument there is
// answered with the decode already on the stream.
static bool decode_render_prologue(int phases, int B, int N, int n_shape, int n_exp, int ntri, int H, int W, int tex_batch,
                                   const float* vertex_handoff, size_t vertex_bytes, int* rc) {
    *rc = FR_ERR_INVALID_ARG;
    if ((phases & 15) < 1 || (phases & ~0xFF0F)) return false;   // bits 0-3: phases; bits 8-15: strip-height hint
    if (n_shape < 0 || n_exp < 0 || render_shape_check(B, N, ntri, H, W, 3, tex_batch) != FR_OK) return false;
    *rc = FR_OK;
    if (B == 0) return false;
    if (N > 0 && !ws_ok(vertex_handoff, vertex_bytes, fr_decode_render_vertex_bytes(B, N), 128)) *rc = FR_ERR_WORKSPACE;
    return *rc == FR_OK;
}

int fr_decode_render_forward(const float* params, const void* packed_basis, const float* R_override, const float* tri,
                             const float* texture, int B, int N, int n_shape, int n_exp, int ntri, int H, int W,
                             int tex_batch, float im_size, float* vertex_handoff, size_t vertex_bytes, float* depth,
                             float* tex_img, float* normal, float* tri_ind, void* workspace, size_t ws_bytes,
                             void* hip_stream, int phases) {
    int rc;
    if (!decode_render_prologue(phases, B, N, n_shape, n_exp, ntri, H, W, tex_batch, vertex_handoff, vertex_bytes, &rc)) return rc;
    const int pitch = fr_decode_render_vertex_pitch(N);
    if ((phases & 8) && N > 0) {
        rc = decode_inputs_check(params, packed_basis);
        if (rc == FR_OK)
            rc = fr_launch_decode(params, packed_basis, R_override, B, N, n_shape, n_exp, im_size, vertex_handoff, pitch,
                                  (hipStream_t)hip_stream);
        if (rc != FR_OK) return rc;
    }
    if (!(phases & 7) || (size_t)H * W == 0) return FR_OK;
    rc = render_call_check(depth && tex_img && normal && tri_ind, vertex_handoff, tri, texture, B, N, ntri, H, W, ws_bytes,
                           RENDER_PLAIN);
    if (rc != FR_OK) return rc;
    return fr_launch_render_forward_phases(vertex_handoff, tri, texture, B, N, ntri, H, W, tex_batch, depth, tex_img, normal,
                                           tri_ind, workspace, ws_bytes, (hipStream_t)hip_stream, phases & 7, pitch, (phases >> 8) & 0xFF);
}

// ---- opt-in Q30 arithmetic: its own image, its own entry point, caller-owned staging workspace ----------------------------
size_t fr_decode_q30_image_bytes(int N, int n_shape, int n_exp) {
    if (N < 0 || n_shape < 0 || n_exp < 0 || !fr_decode_q_supported(n_shape, n_exp)) return 0;
    return fr_packed_q_bytes(N, n_shape, n_exp);
}

int fr_decode_q30_pack(const float* mu, const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp,
                       void* qimage, size_t qimage_bytes, void* hip_stream) {
    if (N < 0 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if (!fr_decode_q_supported(n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    if (qimage_bytes < fr_packed_q_bytes(N, n_shape, n_exp)) return FR_ERR_WORKSPACE;
    if (N == 0) return FR_OK;
    if (!mu || !qimage || (n_shape > 0 && !pc_shape) || (n_exp > 0 && !pc_exp)) return FR_ERR_INVALID_ARG;
    if (((uintptr_t)qimage & 255) != 0) return FR_ERR_INVALID_ARG;
    return fr_launch_pack_q(mu, pc_shape, pc_exp, N, n_shape, n_exp, qimage, (hipStream_t)hip_stream);
}

size_t fr_decode_q30_workspace_bytes(int n_shape, int n_exp) {
    if (n_shape < 0 || n_exp < 0) return 0;
    return fr_decode_q_workspace_bytes_impl(n_shape, n_exp);
}

static int decode_q30_checked(const float* params, const void* qimage, const float* R_override, int B, int N, int n_shape,
                              int n_exp, float im_size, float* vertex_proj, int pitch, int levels, void* workspace,
                              size_t ws_bytes, void* hip_stream) {
    if (B < 0 || N < 0 || n_shape < 0 || n_exp < 0 || !fr_decode_q_levels_ok(levels)) return FR_ERR_INVALID_ARG;
    if (!fr_decode_q_supported(n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    if ((size_t)B * N == 0) return FR_OK;
    if (!params || !qimage || !vertex_proj || pitch < N) return FR_ERR_INVALID_ARG;
    if (((uintptr_t)qimage & 255) != 0) return FR_ERR_INVALID_ARG;
    if (!ws_ok(workspace, ws_bytes, fr_decode_q_workspace_bytes_impl(n_shape, n_exp), 16)) return FR_ERR_WORKSPACE;
    return fr_launch_decode_q(params, qimage, R_override, B, N, n_shape, n_exp, im_size, vertex_proj, pitch, levels, workspace,
                              ws_bytes, (hipStream_t)hip_stream);
}

int fr_decode_3dmm_q30(const float* params, const void* qimage, const float* R_override, int B, int N, int n_shape,
                       int n_exp, float im_size, float* vertex_proj, void* workspace, size_t ws_bytes, void* hip_stream) {
    return decode_q30_checked(params, qimage, R_override, B, N, n_shape, n_exp, im_size, vertex_proj, N, 7, workspace, ws_bytes,
                              hip_stream);
}

int fr_decode_3dmm_q30_lv(const float* params, const void* qimage, const float* R_override, int B, int N, int n_shape,
                          int n_exp, float im_size, int levels, float* vertex_proj, void* workspace, size_t ws_bytes,
                          void* hip_stream) {
    return decode_q30_checked(params, qimage, R_override, B, N, n_shape, n_exp, im_size, vertex_proj, N, levels, workspace,
                              ws_bytes, hip_stream);
}

int fr_decode_render_forward_q30(const float* params, const void* qimage, const float* R_override, const float* tri,
                                 const float* texture, int B, int N, int n_shape, int n_exp, int ntri, int H, int W,
                                 int tex_batch, float im_size, int levels, float* vertex_handoff, size_t vertex_bytes,
                                 float* depth, float* tex_img, float* normal, float* tri_ind, void* workspace, size_t ws_bytes,
                                 void* q_workspace, size_t q_ws_bytes, void* hip_stream, int phases) {
    int rc;
    if (!fr_decode_q_levels_ok(levels)) return FR_ERR_INVALID_ARG;   // (ahead of the empty batch, like every argument error)
    if (!decode_render_prologue(phases, B, N, n_shape, n_exp, ntri, H, W, tex_batch, vertex_handoff, vertex_bytes, &rc)) return rc;
    const int pitch = fr_decode_render_vertex_pitch(N);
    if ((phases & 8) && N > 0) {
        rc = decode_q30_checked(params, qimage, R_override, B, N, n_shape, n_exp, im_size, vertex_handoff, pitch, levels,
                                q_workspace, q_ws_bytes, hip_stream);
        if (rc != FR_OK) return rc;
    }
    if (!(phases & 7) || (size_t)H * W == 0) return FR_OK;
    rc = render_call_check(depth && tex_img && normal && tri_ind, vertex_handoff, tri, texture, B, N, ntri, H, W, ws_bytes,
                           RENDER_PLAIN);
    if (rc != FR_OK) return rc;
    return fr_launch_render_forward_phases(vertex_handoff, tri, texture, B, N, ntri, H, W, tex_batch, depth, tex_img, normal,
                                           tri_ind, workspace, ws_bytes, (hipStream_t)hip_stream, phases & 7, pitch, (phases >> 8) & 0xFF);
}

int fr_debug_clock_probe(unsigned long long* ticks, int blocks, int iters, void* hip_stream) {
    if (!ticks || blocks < 1 || blocks > 65535 || iters < 1) return FR_ERR_INVALID_ARG;
    return fr_launch_clock_probe(ticks, blocks, iters, (hipStream_t)hip_stream);
}

size_t fr_decode_backward_workspace_bytes(int B, int N, int n_shape, int n_exp) {
    if (B <= 0 || N <= 0 || n_shape < 0 || n_exp < 0) return 0;
    return fr_decode_backward_workspace_impl(N, n_shape, n_exp);
}

// The argument list of the three decode backwards.  They take the basis in three forms, so the caller states what is its own:
// point = vertex_proj, or mu; basis = the basis pointers this shape reads are there; aligned = those that must be are 16-byte
// aligned; fused_only = the entry point serves only what the fused kernel does.  Returns true when the entry point launches;
// otherwise *rc is its answer (FR_OK for an empty batch).
static bool decode_backward_check(int B, int N, int n_shape, int n_exp, bool fused_only, const float* grad_vertex_proj,
                                  const float* params, const float* point, bool basis, bool aligned, const float* grad_params,
                                  const void* workspace, size_t ws_bytes, int* rc) {
    *rc = FR_OK;
    if (B < 0 || N < 0 || n_shape < 0 || n_exp < 0) *rc = FR_ERR_INVALID_ARG;
    else if (fused_only && fr_decode_backward_basis_bytes(N, n_shape, n_exp) == 0) *rc = FR_ERR_UNSUPPORTED;
    else if (B == 0) return false;
    else if (!grad_params || !params) *rc = FR_ERR_INVALID_ARG;
    else if (N > 0 && (!grad_vertex_proj || !point || !basis)) *rc = FR_ERR_INVALID_ARG;
    else if (!aligned) *rc = FR_ERR_INVALID_ARG;
    else if (N > 0 && !ws_ok(workspace, ws_bytes, fr_decode_backward_workspace_bytes(B, N, n_shape, n_exp), 16))
        *rc = FR_ERR_WORKSPACE;
    return *rc == FR_OK;
}

int fr_decode_3dmm_backward(const float* grad_vertex_proj, const float* params, const float* vertex_proj,
                            const float* pc_shape, const float* pc_exp, const float* R_override, int B, int N, int n_shape,
                            int n_exp, float im_size, float* grad_params, void* workspace, size_t ws_bytes,
                            void* hip_stream) {
    int rc;
    if (!decode_backward_check(B, N, n_shape, n_exp, false, grad_vertex_proj, params, vertex_proj,
                               (n_shape <= 0 || pc_shape) && (n_exp <= 0 || pc_exp), true, grad_params, workspace, ws_bytes, &rc))
        return rc;
    return fr_launch_decode_backward(grad_vertex_proj, params, vertex_proj, pc_shape, pc_exp, R_override, B, N, n_shape,
                                     n_exp, im_size, grad_params, workspace, (hipStream_t)hip_stream);
}

size_t fr_decode_backward_basis_bytes(int N, int n_shape, int n_exp) {
    if (N <= 0 || n_shape < 0 || n_exp < 0) return 0;
    return fr_decode_backward_basis_bytes_impl(N, n_shape, n_exp);
}

int fr_decode_backward_pack_basis(const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp, void* packed_t,
                                  size_t packed_bytes, void* hip_stream) {
    if (N < 0 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if (packed_bytes < fr_decode_backward_basis_bytes(N, n_shape, n_exp)) return FR_ERR_WORKSPACE;
    if (N == 0 || n_shape + n_exp == 0) return FR_OK;
    if (!packed_t || (n_shape > 0 && !pc_shape) || (n_exp > 0 && !pc_exp)) return FR_ERR_INVALID_ARG;
    if (((uintptr_t)packed_t & 15) != 0) return FR_ERR_INVALID_ARG;
    return fr_launch_decode_backward_pack(pc_shape, pc_exp, N, n_shape, n_exp, packed_t, (hipStream_t)hip_stream);
}

int fr_decode_3dmm_backward_packed(const float* grad_vertex_proj, const float* params, const float* vertex_proj,
                                   const void* packed_t, const float* R_override, int B, int N, int n_shape, int n_exp,
                                   float im_size, float* grad_params, void* workspace, size_t ws_bytes, void* hip_stream) {
    int rc;
    if (!decode_backward_check(B, N, n_shape, n_exp, false, grad_vertex_proj, params, vertex_proj, n_shape + n_exp <= 0 || packed_t,
                               ((uintptr_t)packed_t & 15) == 0, grad_params, workspace, ws_bytes, &rc))
        return rc;
    return fr_launch_decode_backward(grad_vertex_proj, params, vertex_proj, nullptr, nullptr, R_override, B, N, n_shape, n_exp,
                                     im_size, grad_params, workspace, (hipStream_t)hip_stream, n_shape + n_exp > 0 ? packed_t : nullptr);
}

int fr_decode_3dmm_backward_packed_mu(const float* grad_vertex_proj, const float* params, const float* mu, const void* packed_t,
                                      const float* R_override, int B, int N, int n_shape, int n_exp, float im_size,
                                      float* grad_params, void* workspace, size_t ws_bytes, void* hip_stream) {
    int rc;   // (fused_only: N > 0 wherever the list below is reached)
    if (!decode_backward_check(B, N, n_shape, n_exp, true, grad_vertex_proj, params, mu, packed_t != nullptr,
                               ((uintptr_t)packed_t & 15) == 0 && ((uintptr_t)mu & 15) == 0, grad_params, workspace, ws_bytes, &rc))
        return rc;
    return fr_launch_decode_backward(grad_vertex_proj, params, nullptr, nullptr, nullptr, R_override, B, N, n_shape, n_exp,
                                     im_size, grad_params, workspace, (hipStream_t)hip_stream, packed_t, mu);
}

// ---- differentiable decode -> rendering-layer step -----------------------------------------------------------------------
int fr_decode_rendering_layer_forward(const float* params, const void* packed_basis, const float* R_override, const float* tri,
                                      const float* texture, const float* im_gray, int B, int N, int n_shape, int n_exp, int ntri,
                                      int H, int W, int tex_batch, float im_size, float* vertex_handoff, size_t vertex_bytes,
                                      float* net_input, float* depth_img, float* depth, float* tri_ind, void* workspace,
                                      size_t ws_bytes, void* hip_stream, int phases) {
    int rc;
    if (!decode_render_prologue(phases, B, N, n_shape, n_exp, ntri, H, W, tex_batch, vertex_handoff, vertex_bytes, &rc)) return rc;
    const int pitch = fr_decode_render_vertex_pitch(N);
    const bool decode = (phases & 8) && N > 0, layer = (phases & 7) && (size_t)H * W > 0;
    if (decode && (rc = decode_inputs_check(params, packed_basis)) != FR_OK) return rc;
    if (layer) {   // the checks of fr_rendering_layer_forward, all of them BEFORE the decode is launched
        rc = render_call_check(net_input && depth_img && depth && tri_ind && im_gray, vertex_handoff, tri, texture, B, N, ntri, H, W,
                               ws_bytes, RENDER_LAYER_SERVED);
        if (rc != FR_OK) return rc;
    }
    if (decode) {
        rc = fr_launch_decode(params, packed_basis, R_override, B, N, n_shape, n_exp, im_size, vertex_handoff, pitch,
                              (hipStream_t)hip_stream);
        if (rc != FR_OK) return rc;
    }
    if (!layer) return FR_OK;
    return fr_launch_rendering_layer(vertex_handoff, tri, texture, im_gray, B, N, ntri, H, W, tex_batch, net_input, depth_img,
                                     depth, tri_ind, workspace, ws_bytes, (hipStream_t)hip_stream, phases & 7, pitch,
                                     (phases >> 8) & 0xFF);
}

// workspace of fr_decode_render_backward: [records + chunk partials of the render backward | z plane [B, pitch] | decode-backward
// slabs], each part rounded up to 256 bytes
namespace {
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
struct DrbLayout { size_t rec, z, dec; };
DrbLayout drb_layout(int B, int N, int n_shape, int n_exp, int H, int W) {
    DrbLayout l;
    l.rec = up256(fr_render_depth_backward_workspace_bytes(B, H, W));
    l.z = up256((size_t)B * (size_t)fr_decode_render_vertex_pitch(N) * sizeof(float));
    l.dec = up256(fr_decode_backward_workspace_impl(N, n_shape, n_exp));
    return l;
}
}  // namespace

size_t fr_decode_render_backward_workspace_bytes(int B, int N, int n_shape, int n_exp, int H, int W) {
    if (B <= 0 || N <= 0 || n_shape < 0 || n_exp < 0 || H < 0 || W < 0) return 0;
    if (fr_decode_backward_basis_bytes_impl(N, n_shape, n_exp) == 0) return 0;
    const DrbLayout l = drb_layout(B, N, n_shape, n_exp, H, W);
    return l.rec + l.z + l.dec;
}

int fr_decode_render_backward(const float* g_depth, const float* g_depth_img, const float* g_net_input, const float* im_gray,
                              const float* depth, const float* tri, const float* tri_ind, const float* params, const float* mu,
                              const void* packed_t, const float* R_override, int B, int N, int n_shape, int n_exp, int ntri,
                              int H, int W, float im_size, float* grad_params, void* workspace, size_t ws_bytes,
                              void* hip_stream) {
    if (B < 0 || N < 0 || n_shape < 0 || n_exp < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (fr_decode_backward_basis_bytes(N, n_shape, n_exp) == 0) return FR_ERR_UNSUPPORTED;   // what the fused kernel does not serve
    if (B == 0) return FR_OK;
    if (!g_depth && !g_depth_img && !g_net_input) return FR_ERR_INVALID_ARG;
    if ((g_depth_img || g_net_input) && (!im_gray || !depth)) return FR_ERR_INVALID_ARG;
    if (!grad_params || !params || !mu || !packed_t || !tri_ind || (ntri > 0 && !tri)) return FR_ERR_INVALID_ARG;
    if (((uintptr_t)packed_t & 15) != 0 || ((uintptr_t)mu & 15) != 0) return FR_ERR_INVALID_ARG;
    if ((long long)H * W > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (!ws_ok(workspace, ws_bytes, fr_decode_render_backward_workspace_bytes(B, N, n_shape, n_exp, H, W), 256)) return FR_ERR_WORKSPACE;
    const DrbLayout l = drb_layout(B, N, n_shape, n_exp, H, W);
    char* ws = reinterpret_cast<char*>(workspace);
    float* zplane = reinterpret_cast<float*>(ws + l.rec);
    const int pitch = fr_decode_render_vertex_pitch(N);
    const FrPixelGrad pg = {g_depth, g_depth_img, g_net_input, im_gray, depth};
    int rc = fr_launch_render_backward_z(pg, tri, tri_ind, zplane, pitch, B, N, ntri, H, W, ws, l.rec, (hipStream_t)hip_stream);
    if (rc != FR_OK) return rc;
    return fr_launch_decode_backward(zplane, params, nullptr, nullptr, nullptr, R_override, B, N, n_shape, n_exp, im_size,
                                     grad_params, ws + l.rec + l.z, (hipStream_t)hip_stream, packed_t, mu, pitch);
}

// ---- pose gradients --------------------------------------------------------------------------------------------------------
size_t fr_decode_pose_backward_workspace_bytes(int B, int N) { return fr_decode_pose_backward_workspace_impl(B, N); }

int fr_decode_pose_backward(const float* grad_vertex_proj, const float* vertex_proj, const float* params,
                            const float* R_override, int B, int N, int n_shape, int n_exp, float im_size, float* grad_params,
                            float* grad_R, void* workspace, size_t ws_bytes, void* hip_stream) {
    if (B < 0 || N < 0 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if (B == 0) return FR_OK;
    if (!grad_params && !grad_R) return FR_ERR_INVALID_ARG;
    if (!params || (N > 0 && (!grad_vertex_proj || !vertex_proj))) return FR_ERR_INVALID_ARG;
    const size_t need = fr_decode_pose_backward_workspace_impl(B, N);
    if (need > 0 && !ws_ok(workspace, ws_bytes, need, 16)) return FR_ERR_WORKSPACE;
    if (need / (9 * sizeof(float)) > 0x7FFFFFFFull) return FR_ERR_UNSUPPORTED;   // (face, chunk) workgroups beyond one grid
    return fr_launch_decode_pose_backward(grad_vertex_proj, vertex_proj, params, R_override, B, N, n_shape, n_exp, im_size,
                                          grad_params, grad_R, workspace, (hipStream_t)hip_stream);
}

// workspace of fr_decode_render_backward_pose: that of fr_decode_render_backward, then the chunk records of the pose moment
size_t fr_decode_render_backward_pose_workspace_bytes(int B, int N, int n_shape, int n_exp, int H, int W) {
    const size_t base = fr_decode_render_backward_workspace_bytes(B, N, n_shape, n_exp, H, W);
    return base == 0 ? 0 : base + up256(fr_decode_pose_backward_workspace_impl(B, N));
}

int fr_decode_render_backward_pose(const float* g_depth, const float* g_depth_img, const float* g_net_input,
                                   const float* im_gray, const float* depth, const float* tri, const float* tri_ind,
                                   const float* params, const float* mu, const void* packed_t, const float* R_override, int B,
                                   int N, int n_shape, int n_exp, int ntri, int H, int W, float im_size, float* grad_params,
                                   void* workspace, size_t ws_bytes, void* hip_stream, const float* vertex_handoff,
                                   size_t vertex_bytes, float* grad_R) {
    if (B < 0 || N < 0 || n_shape < 0 || n_exp < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (fr_decode_backward_basis_bytes(N, n_shape, n_exp) == 0) return FR_ERR_UNSUPPORTED;   // as fr_decode_render_backward
    if (B == 0) return FR_OK;
    if ((long long)H * W > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (!ws_ok(vertex_handoff, vertex_bytes, fr_decode_render_vertex_bytes(B, N), 128)) return FR_ERR_WORKSPACE;
    const size_t base = fr_decode_render_backward_workspace_bytes(B, N, n_shape, n_exp, H, W);
    if (!ws_ok(workspace, ws_bytes, fr_decode_render_backward_pose_workspace_bytes(B, N, n_shape, n_exp, H, W), 256)) return FR_ERR_WORKSPACE;
    // (every remaining check is fr_decode_render_backward's own, made before its first launch)
    const int rc = fr_decode_render_backward(g_depth, g_depth_img, g_net_input, im_gray, depth, tri, tri_ind, params, mu, packed_t,
                                             R_override, B, N, n_shape, n_exp, ntri, H, W, im_size, grad_params, workspace, base,
                                             hip_stream);
    if (rc != FR_OK) return rc;
    const DrbLayout l = drb_layout(B, N, n_shape, n_exp, H, W);
    char* ws = reinterpret_cast<char*>(workspace);
    return fr_launch_decode_pose_backward(reinterpret_cast<const float*>(ws + l.rec), vertex_handoff, params, R_override, B, N,
                                          n_shape, n_exp, im_size, grad_params, grad_R, ws + base, (hipStream_t)hip_stream,
                                          fr_decode_render_vertex_pitch(N));
}

// ---- normal-map gradients -----------------------------------------------------------------------------------------------------
size_t fr_render_normal_backward_workspace_bytes(int B, int nver, int H, int W) {
    (void)nver;
    return fr_render_normal_backward_workspace_impl(B, H, W);
}

int fr_render_normal_backward(const float* normal_grad, int grad_stride, const float* vertex, int vertex_pitch,
                              const float* tri, const float* tri_ind, float* vertex_grad, int B, int nver, int ntri,
                              int H, int W, int mode, int accumulate, void* workspace, size_t ws_bytes, void* hip_stream) {
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if ((mode != 0 && mode != 1) || (accumulate != 0 && accumulate != 1)) return FR_ERR_INVALID_ARG;
    if (grad_stride < 3 || vertex_pitch < nver) return FR_ERR_INVALID_ARG;
    if (B == 0) return FR_OK;
    if (nver == 0) return FR_OK;   // an empty vertex_grad: nothing to write
    if (!vertex_grad) return FR_ERR_INVALID_ARG;
    const bool work = (size_t)H * W > 0 && ntri > 0;
    if (work && (!normal_grad || !vertex || !tri || !tri_ind)) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;   // float-stored ids stop being exact
    if (work && !ws_ok(workspace, ws_bytes, fr_render_normal_backward_workspace_impl(B, H, W), 16)) return FR_ERR_WORKSPACE;
    return fr_launch_render_normal_backward(normal_grad, grad_stride, vertex, vertex_pitch, tri, tri_ind, vertex_grad, B, nver,
                                            ntri, H, W, mode, accumulate, workspace, (hipStream_t)hip_stream);
}

// ---- texture gradients ----------------------------------------------------------------------------------------------------------
size_t fr_render_texture_backward_workspace_bytes(int B, int nver, int H, int W, int tex_batch) {
    if (B > 0 && tex_batch != 1 && tex_batch != B) return 0;
    return fr_render_texture_backward_workspace_impl(B, nver, H, W, tex_batch);
}

int fr_render_texture_backward(const float* tex_grad, int grad_stride, const float* tri, const float* tri_ind,
                               float* texture_grad, int B, int nver, int ntri, int H, int W, int tex_batch, int accumulate,
                               void* workspace, size_t ws_bytes, void* hip_stream) {
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (B > 0 && tex_batch != 1 && tex_batch != B) return FR_ERR_INVALID_ARG;
    if ((accumulate != 0 && accumulate != 1) || grad_stride < 3) return FR_ERR_INVALID_ARG;
    if (B == 0 || nver == 0) return FR_OK;   // an empty batch or an empty texture_grad: nothing to write
    if (!texture_grad) return FR_ERR_INVALID_ARG;
    const bool work = (size_t)H * W > 0 && ntri > 0;
    if (work && (!tex_grad || !tri || !tri_ind)) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;   // float-stored ids stop being exact
    if ((long long)H * W > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;   // (a shape no workspace serves: answered before the workspace)
    if (work && !ws_ok(workspace, ws_bytes, fr_render_texture_backward_workspace_impl(B, nver, H, W, tex_batch), 16))
        return FR_ERR_WORKSPACE;
    return fr_launch_render_texture_backward(tex_grad, grad_stride, tri, tri_ind, texture_grad, B, nver, ntri, H, W, tex_batch,
                                             accumulate, workspace, (hipStream_t)hip_stream);
}

// ---- synthetic batches ------------------------------------------------------------------------------------------------------------
// n (lo, hi) pairs on the host: finite, lo <= hi
static bool synth_ranges_ok(const float* r, int n) {
    for (int k = 0; k < n; k++)
        if (!(r[2 * k] <= r[2 * k + 1]) || !(r[2 * k] - r[2 * k] == 0.0f) || !(r[2 * k + 1] - r[2 * k + 1] == 0.0f)) return false;
    return true;
}

int fr_synth_params(unsigned long long seed, unsigned long long first_face, int B, int n_shape, int n_exp, int K, float im_size,
                    float beta, float focal, const float* light_ranges, const float* alpha_ranges, float* params, float* light,
                    float* alpha, void* stream) {
    if (B < 1 || n_shape < 0 || n_exp < 0 || K < 0) return FR_ERR_INVALID_ARG;
    if (!(beta >= 0.0f && beta <= 1.0f) || !(im_size - im_size == 0.0f) || !(focal - focal == 0.0f)) return FR_ERR_INVALID_ARG;
    if (K > FR_SYNTH_MAX_TEX || B > 65535) return FR_ERR_UNSUPPORTED;
    if ((long long)n_shape + n_exp + K > 0x7FFFFFFFll - 64) return FR_ERR_UNSUPPORTED;   // (the draw index stays an int)
    if (!params || !light || !light_ranges || (K > 0 && (!alpha || !alpha_ranges))) return FR_ERR_INVALID_ARG;
    if (!synth_ranges_ok(light_ranges, 4) || !synth_ranges_ok(alpha_ranges, K)) return FR_ERR_INVALID_ARG;
    return fr_launch_synth_params(seed, first_face, B, n_shape, n_exp, K, im_size, beta, focal, light_ranges, alpha_ranges, params,
                                  light, alpha, (hipStream_t)stream);
}

int fr_synth_texture(const float* mu_tex, const float* pc_tex, const float* alpha, int B, int N, int K, float* tex, void* stream) {
    if (B < 1 || N < 1 || K < 0) return FR_ERR_INVALID_ARG;
    if (B > 65535) return FR_ERR_UNSUPPORTED;
    if (!mu_tex || !tex || (K > 0 && (!pc_tex || !alpha))) return FR_ERR_INVALID_ARG;
    return fr_launch_synth_texture(mu_tex, pc_tex, alpha, B, N, K, tex, (hipStream_t)stream);
}

size_t fr_synth_texture_backward_workspace_bytes(int B, int N, int K) { return fr_synth_texture_backward_workspace_impl(B, N, K); }

int fr_synth_texture_backward(const float* pc_tex, const float* grad_tex, int B, int N, int K, float* grad_alpha, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (B < 1 || N < 1 || K < 0) return FR_ERR_INVALID_ARG;
    if (B > 65535 || (long long)N * 3 > 0x7FFFFFFFll - 256 || (long long)B * K > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (K == 0) return FR_OK;   // an empty gradient: nothing launched, nothing read
    if (!pc_tex || !grad_tex || !grad_alpha) return FR_ERR_INVALID_ARG;
    if (!ws_ok(workspace, workspace_bytes, fr_synth_texture_backward_workspace_impl(B, N, K), 16)) return FR_ERR_WORKSPACE;
    return fr_launch_synth_texture_backward(pc_tex, grad_tex, B, N, K, grad_alpha, workspace, (hipStream_t)stream);
}

// both shaders' checks, in their order; image: the model's own plane (im_gray of the gray shader, im_rgb of the colour one)
static int synth_shade_check(const float* tex_img, const float* normal, const float* tri_ind, const float* light,
                             const float* background, int bg_batch, int B, int H, int W, const float* image, const float* mask) {
    if (B < 1 || H < 1 || W < 1) return FR_ERR_INVALID_ARG;
    if (background ? (bg_batch != 1 && bg_batch != B) : bg_batch != 0) return FR_ERR_INVALID_ARG;
    if (!tex_img || !normal || !tri_ind || !light || !image || !mask) return FR_ERR_INVALID_ARG;
    if ((long long)H * W > 0x7FFFFFFFll || B > 65535) return FR_ERR_UNSUPPORTED;
    return FR_OK;
}

int fr_synth_shade(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* background,
                   int bg_batch, int B, int H, int W, float gain, float offset, float* im_gray, float* mask, void* stream) {
    const int rc = synth_shade_check(tex_img, normal, tri_ind, light, background, bg_batch, B, H, W, im_gray, mask);
    if (rc != FR_OK) return rc;
    return fr_launch_synth_shade(tex_img, normal, tri_ind, light, background, bg_batch, B, H, W, gain, offset, im_gray, mask,
                                 (hipStream_t)stream);
}

// ---- colour shading: the checks of fr_synth_params and fr_synth_shade ----------------------------------------------------------------
int fr_synth_light_rgb(unsigned long long seed, unsigned long long first_face, int B, const float* ranges, float* light, void* stream) {
    if (B < 1) return FR_ERR_INVALID_ARG;
    if (B > 65535) return FR_ERR_UNSUPPORTED;
    if (!ranges || !light) return FR_ERR_INVALID_ARG;
    if (!synth_ranges_ok(ranges, 27)) return FR_ERR_INVALID_ARG;
    return fr_launch_synth_light_rgb(seed, first_face, B, ranges, light, (hipStream_t)stream);
}

int fr_synth_shade_rgb(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* background,
                       int bg_batch, int B, int H, int W, float gain, float offset, float* im_rgb, float* im_gray, float* mask,
                       void* stream) {
    const int rc = synth_shade_check(tex_img, normal, tri_ind, light, background, bg_batch, B, H, W, im_rgb, mask);   // (im_gray may be NULL)
    if (rc != FR_OK) return rc;
    return fr_launch_synth_shade_rgb(tex_img, normal, tri_ind, light, background, bg_batch, B, H, W, gain, offset, im_rgb, im_gray,
                                     mask, (hipStream_t)stream);
}

// ---- landmark solver: the checks of fr_landmark_forward, then its own -----------------------------------------------------------------
size_t fr_landmark_solve_workspace_bytes(int B, int n_shape, int n_exp) { return fr_landmark_solve_workspace_impl(B, n_shape, n_exp); }

int fr_landmark_solve_step(const float* params, const void* lbasis, size_t lbasis_bytes, const float* target, const float* weight,
                           int weight_batch, const float* ridge, const float* center, const double* damp, int pose_mask, int fit_coef,
                           int B, int K, int n_shape, int n_exp, float im_size, double* delta, double* cost, int* ok, void* workspace,
                           size_t workspace_bytes, void* stream) {
    using namespace fr;
    if (B < 0 || K < 0 || n_shape < 0 || n_exp < 0 || (weight_batch != 0 && weight_batch != 1)) return FR_ERR_INVALID_ARG;
    if ((fit_coef != 0 && fit_coef != 1) || (pose_mask & ~0x5F)) return FR_ERR_INVALID_ARG;   // bit 5, tz: its column is zero
    const bool coef = fit_coef && (long long)n_shape + n_exp > 0;
    if (pose_mask == 0 && !coef) return FR_ERR_INVALID_ARG;                                   // nothing to fit
    if (B == 0 || K == 0) return FR_OK;
    if (!params || !target || !delta || !cost || !ok) return FR_ERR_INVALID_ARG;
    if (!lm_sizes_ok(K, n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    if (!ws_ok(lbasis, lbasis_bytes, lm_basis_floats(K, n_shape + n_exp) * sizeof(float), 16)) return FR_ERR_WORKSPACE;
    if (coef && !ws_ok(workspace, workspace_bytes, fr_landmark_solve_workspace_impl(B, n_shape, n_exp), 16)) return FR_ERR_WORKSPACE;
    return fr_launch_landmark_solve(params, reinterpret_cast<const float*>(lbasis), target, weight, weight_batch, ridge, center, damp,
                                    pose_mask, coef ? 1 : 0, B, K, n_shape, n_exp, im_size, delta, cost, ok, workspace,
                                    (hipStream_t)stream);
}

}  // extern "C"
