// Photometric loss (opt-in; include/fr_hotpath.h, "photometric loss"): the shader's image compared with a target picture, per face, in
// ONE streaming pass, and its gradients with respect to the render's planes and the lighting in one more.
//
//   photo_loss[_rgb]_forward_kernel   a workgroup owns PH_TILE = 256 consecutive pixels of one face, one lane per pixel, as the shader
//                               does.  A covered lane runs the shader's own device function (fr_shade.h) and forms, in float64, the NS
//                               terms of the header; the 256 x NS values meet in a fixed tree: inside a wave by lane exchanges (strides
//                               32 .. 1, all the sums packed into one pass: ph_pack_level), then the four wave sums as
//                               (w0 + w2) + (w1 + w3).  NS float64 partials per tile.
//   photo_loss_finish_kernel<NS>  one workgroup of PH_FIN = 256 threads per face: thread i chains that face's partials i, i + 256, ..
//                               from +0.0 (one addition at 200 x 200: 157 tiles), then the same tree.  Writes sums[b][0 .. NS).
//                               CHOICE: the lighting sums are taken HERE, in the forward: they are linear in the upstream
//                               gradient, so the backward is a pure map -- no reduction, no second launch -- and the forward is
//                               memory-bound with or without them.
//   photo_loss[_rgb]_backward_kernel  the same lane-per-pixel map: recomputes the shading (the same device function, the same bits),
//                               writes every element of the planes that were asked for (zeros off the face), and the lighting
//                               gradients from sums.  grad_sse is read from the device.
// ONE programme for both losses: every body below is a template in the model M of fr_shade.h (GrayModel: NC = 1 channel, NK = 4
// lighting terms; ColourModel, include/fr_hotpath.h "colour shading": NC = 3, NK = 9) or in its number of sums NS = 2 + NC NK per face
// (sse, cnt and NK lighting sums per channel: 6 or 29), in the SAME association.  The four pass kernels keep their names as wrappers
// over the templated bodies (profiles, DESIGN.md and the resource test name them).  Where the two models' arithmetic is not the same
// expression, the model owns the piece (fr_shade.h: tex_gradient, chain_gradient); nothing here branches on the model.
// Float64 products and sums each rounded on their own (-ffp-contract=off).  No atomics.
#include "fr_common.h"
#include "fr_shade.h"

namespace fr {

constexpr int PH_TILE = 256, PH_WAVES = PH_TILE / 64, PH_FIN = 256;
template <class M>
constexpr int PH_SUMS = 2 + M::NC * M::NK;

struct PhArgs {             // NC, NK, NS: the model's
    const float* tex_img;   // [B,H,W,3]
    const float* normal;    // [B,H,W,3]
    const float* tri_ind;   // [B,H,W]
    const float* light;     // [B,NC,NK]
    const float* target;    // [B,H,W,NC]
    const float* weight;    // [B,H,W] or null
    const double* sums;     // [B,NS]                     (backward, for grad_light)
    const double* grad_sse; // [B]                        (backward)
    double* part;           // [B][tiles][NS]             (forward)
    float* g_tex;           // [B,H,W,3] or null          (backward)
    float* g_normal;        // [B,H,W,3] or null          (backward)
    float* g_light;         // [B,NC,NK] or null          (backward)
    int HW, tiles;
    float gain, offset;
};

// what both directions need of a covered pixel: the shading, and per channel t = ((2 w) r) gain in float64
template <class M>
struct PhPixel {
    typename M::State sh;
    double w, r[M::NC], t[M::NC];
};
template <class M>
__device__ __forceinline__ void ph_pixel(const PhArgs& a, int b, size_t i, PhPixel<M>& p) {
    float I[M::NC];
    M::shade(a.tex_img + 3 * i, a.normal + 3 * i, a.light + (size_t)b * (M::NC * M::NK), p.sh, I);
    p.w = a.weight ? (double)a.weight[i] : 1.0;
#pragma unroll
    for (int c = 0; c < M::NC; c++) {
        const float im = I[c] * a.gain + a.offset;
        p.r[c] = (double)im - (double)a.target[M::NC * i + c];
        p.t[c] = ((2.0 * p.w) * p.r[c]) * (double)a.gain;
    }
}

// the tree over a workgroup's 256 slots, for NS values at once; thread 0 ends with the NS sums in v
//
// The lane tree of the header -- v[i] = v[i] + v[i + k] for i < k, k = 32 .. 1 -- leaves 64 - k lanes idle at every step, once per sum.
// ph_pack_level runs the SAME additions for all the sums together and fills the idle lanes: at distance K two registers a, b share one
// exchange and one addition -- the lanes with bit K clear form a[i] + a[i ^ K], the others b[i] + b[i ^ K] (the operands of the
// header's addition; IEEE addition commutes) -- so N registers become ceil(N / 2), and after the six steps ONE register holds every
// sum: sum j in the lane whose bits 5 .. 1 are j's bits 0 .. 4 (bit 0 clear).  31 exchanges and additions for 29 sums where one tree
// per sum takes 174; the bits are the one-tree-per-sum bits (fr::wave_tree_f64).
// At K = 32 and 16 the exchange is gfx950's v_permlane32_swap / v_permlane16_swap (the upper half -- the odd rows of 16 -- of a trade
// places with the lower half -- the even rows -- of b, in registers: no trip through the LDS crossbar, no select); below, a lane
// shuffle of the register the lane does not keep.
template <int K>
__device__ __forceinline__ void ph_swap_words(unsigned& a, unsigned& b) {
    const auto r = K == 32 ? __builtin_amdgcn_permlane32_swap(a, b, false, false) : __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0]; b = r[1];
}
template <int N, int K>
__device__ __forceinline__ double ph_pack_level(const double (&v)[N], int lane) {
    constexpr int M = (N + 1) / 2;
    static_assert(K > 1 || N == 1, "at most 32 sums");
    double w[M];
    const bool up = (lane & K) != 0;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const double a = v[2 * m];
        const double b = 2 * m + 1 < N ? v[2 * m + 1] : 0.0;
        if constexpr (K >= 16) {
            unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
            unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
            ph_swap_words<K>(alo, blo);
            ph_swap_words<K>(ahi, bhi);
            // now a = (a's lower part | b's lower part) and b = (a's upper part | b's upper part): v[i] + v[i + K] for both
            w[m] = __hiloint2double((int)ahi, (int)alo) + __hiloint2double((int)bhi, (int)blo);
        } else {
            const double got = __shfl_xor(up ? a : b, K, 64);
            w[m] = (up ? b : a) + got;
        }
    }
    if constexpr (K == 1) return w[0];
    else return ph_pack_level<M, K / 2>(w, lane);
}

template <int NS>
__device__ __forceinline__ void ph_block_tree(double (&v)[NS], double (*ws)[PH_WAVES]) {
    const int t = (int)threadIdx.x;
    const int lane = t & 63;
    const double r = ph_pack_level<NS, 32>(v, lane);
    const int mine = ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2) | (((lane >> 2) & 1) << 3) |
                     (((lane >> 1) & 1) << 4);   // the sum this lane holds
    if (!(lane & 1) && mine < NS) ws[mine][t >> 6] = r;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < NS; j++) v[j] = (ws[j][0] + ws[j][2]) + (ws[j][1] + ws[j][3]);
    }
}

// the normalisation's backward, shared by both losses: g~ (the gradient with respect to n^) -> the gradient with respect to the raw
// normal, rounded once to fp32
__device__ __forceinline__ void ph_normal_backward(const ShadeNormal& sh, double gx, double gy, double gz, float (&gn)[3]) {
    const double d = (double)sh.d;
    double ox, oy, oz;
    if (sh.unit) {   // the forward replaced mag by 1: d is a constant
        ox = gx / d; oy = gy / d; oz = gz / d;
    } else {
        const double nx = (double)sh.nx, ny = (double)sh.ny, nz = (double)sh.nz;
        const double rho = sqrt((double)sh.mag);
        const double c = ((nx * gx + ny * gy) + nz * gz) / (d * rho);
        ox = (gx - nx * c) / d; oy = (gy - ny * c) / d; oz = (gz - nz * c) / d;
    }
    if (sh.flipped) { ox = -ox; oy = -oy; oz = -oz; }
    gn[0] = (float)ox; gn[1] = (float)oy; gn[2] = (float)oz;
}

template <class M>
__device__ __forceinline__ void photo_loss_forward_body(const PhArgs& a) {
    constexpr int NC = M::NC, NK = M::NK, NS = PH_SUMS<M>;
    __shared__ double ws[NS][PH_WAVES];
    const unsigned int pix = blockIdx.x * (unsigned)PH_TILE + threadIdx.x;
    const int b = (int)blockIdx.y;
    double v[NS];   // a slot outside the image or off the face: +0.0
#pragma unroll
    for (int j = 0; j < NS; j++) v[j] = 0.0;
    if (pix < (unsigned int)a.HW) {
        const size_t i = (size_t)b * (size_t)a.HW + pix;
        if (a.tri_ind[i] >= 0.0f) {
            PhPixel<M> p;
            ph_pixel(a, b, i, p);
            double e = (p.w * p.r[0]) * p.r[0];   // the first channel, then the others in ascending order
#pragma unroll
            for (int c = 1; c < NC; c++) e = e + (p.w * p.r[c]) * p.r[c];
            v[0] = e;
            v[1] = 1.0;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const double u = M::chain(p.sh, c) > 0.0f ? p.t[c] * (double)M::albedo(p.sh, c) : 0.0;
                v[2 + NK * c] = u;   // (H0 = 1 is not multiplied)
#pragma unroll
                for (int k = 1; k < NK; k++) v[2 + NK * c + k] = u * (double)M::basis(p.sh, k);
            }
        }
    }
    ph_block_tree(v, ws);
    if (threadIdx.x == 0) {
        double* out = a.part + ((size_t)b * a.tiles + blockIdx.x) * NS;
#pragma unroll
        for (int j = 0; j < NS; j++) out[j] = v[j];
    }
}

template <int NS>
__global__ __launch_bounds__(PH_FIN) void photo_loss_finish_kernel(const double* __restrict__ part, int tiles, double* __restrict__ sums) {
    __shared__ double ws[NS][PH_WAVES];
    const int b = (int)blockIdx.x;
    const double* mine = part + (size_t)b * tiles * NS;
    double v[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) v[j] = 0.0;
    for (int p = (int)threadIdx.x; p < tiles; p += PH_FIN) {
#pragma unroll
        for (int j = 0; j < NS; j++) v[j] = v[j] + mine[(size_t)p * NS + j];
    }
    ph_block_tree(v, ws);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NS; j++) sums[(size_t)b * NS + j] = v[j];
    }
}

template <class M>
__device__ __forceinline__ void photo_loss_backward_body(const PhArgs& a) {
    constexpr int NC = M::NC, NK = M::NK;
    const unsigned int pix = blockIdx.x * (unsigned)PH_TILE + threadIdx.x;
    const int b = (int)blockIdx.y;
    const double g = a.grad_sse[b];
    if (a.g_light && blockIdx.x == 0 && threadIdx.x < NC * NK)
        a.g_light[(size_t)b * (NC * NK) + threadIdx.x] = (float)(g * a.sums[(size_t)b * PH_SUMS<M> + 2 + threadIdx.x]);
    if (pix >= (unsigned int)a.HW) return;
    const size_t i = (size_t)b * (size_t)a.HW + pix;
    float gt[3] = {0.0f, 0.0f, 0.0f}, gn[3] = {0.0f, 0.0f, 0.0f};
    if (a.tri_ind[i] >= 0.0f) {
        PhPixel<M> p;
        ph_pixel(a, b, i, p);
        double gx = 0.0, gy = 0.0, gz = 0.0;   // g~; what a channel does to it is the model's (fr_shade.h, chain_gradient)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const double dI = g * p.t[c];
            const bool lit = M::chain(p.sh, c) > 0.0f;
            if (a.g_tex) M::tex_gradient(p.sh, c, dI, lit, a.tex_img + 3 * i, gt);
            if (a.g_normal) {
                const double q = lit ? dI * (double)M::albedo(p.sh, c) : 0.0;
                M::chain_gradient(p.sh, a.light + (size_t)b * (NC * NK) + NK * c, q, gx, gy, gz);
            }
        }
        if (a.g_normal) ph_normal_backward(p.sh, gx, gy, gz, gn);
    }
    if (a.g_tex) { a.g_tex[3 * i] = gt[0]; a.g_tex[3 * i + 1] = gt[1]; a.g_tex[3 * i + 2] = gt[2]; }
    if (a.g_normal) { a.g_normal[3 * i] = gn[0]; a.g_normal[3 * i + 1] = gn[1]; a.g_normal[3 * i + 2] = gn[2]; }
}

// the four pass kernels under their own names (not instantiations of one __global__ template: the names are what profiles, DESIGN.md
// and tests/test_photo_rgb_cpu.py know them by)
__global__ __launch_bounds__(PH_TILE) void photo_loss_forward_kernel(const PhArgs a) { photo_loss_forward_body<GrayModel>(a); }
__global__ __launch_bounds__(PH_TILE) void photo_loss_backward_kernel(const PhArgs a) { photo_loss_backward_body<GrayModel>(a); }
__global__ __launch_bounds__(PH_TILE) void photo_loss_rgb_forward_kernel(const PhArgs a) { photo_loss_forward_body<ColourModel>(a); }
__global__ __launch_bounds__(PH_TILE) void photo_loss_rgb_backward_kernel(const PhArgs a) { photo_loss_backward_body<ColourModel>(a); }

}  // namespace fr

// The launch geometry and the state's layout, chosen in ONE place: the size query, the launchers and the test hook read them from here.
namespace {
// more than 2^31 - 1 pixels per face (the pixel index is a 32-bit word), or more faces than the grid's y takes
bool ph_size_ok(int B, int H, int W) { return (long long)H * W <= 0x7FFFFFFFll && B <= 65535; }
int ph_tiles(int H, int W) { return (int)(((long long)H * W + fr::PH_TILE - 1) / fr::PH_TILE); }
// state: the tile partials [B][tiles][sums], float64.  0 for an empty shape or one the launchers refuse.
size_t ph_state_bytes(int B, int H, int W, int sums) {
    if (B <= 0 || H <= 0 || W <= 0 || !ph_size_ok(B, H, W)) return 0;
    return (size_t)B * (size_t)ph_tiles(H, W) * (size_t)sums * sizeof(double);
}
// test hook: out = {pixels per tile, tiles per face, threads of the finish workgroup, sums per face}
void ph_geom(int B, int H, int W, int sums, int* out) {
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (B <= 0 || H <= 0 || W <= 0 || !ph_size_ok(B, H, W)) return;
    out[0] = fr::PH_TILE; out[1] = ph_tiles(H, W); out[2] = fr::PH_FIN; out[3] = sums;
}
// the order both entry points answer in: a negative size, an empty shape (FR_OK, nothing launched), the entry point's own pointers,
// its state, a shape beyond one grid.  FR_OK with *go = true: launch.
int ph_check(int B, int H, int W, bool pointers_ok, bool state_ok, bool* go) {
    *go = false;
    if (B < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!pointers_ok) return FR_ERR_INVALID_ARG;
    if (!state_ok) return FR_ERR_WORKSPACE;
    if (!ph_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    *go = true;
    return FR_OK;
}

// the two launchers, handed a model's pass kernel (the kernels are named, not instantiated: see there); the forward's state and finish
// step need the model's number of sums as well
using PhKernel = void (*)(const fr::PhArgs);
template <class M>
int ph_forward(PhKernel pass, const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* target,
               const float* weight, int B, int H, int W, float gain, float offset, double* sums, void* state, size_t state_bytes,
               void* stream) {
    constexpr int NS = fr::PH_SUMS<M>;
    bool go;
    const int rc = ph_check(B, H, W, tex_img && normal && tri_ind && light && target && sums,
                            ws_ok(state, state_bytes, ph_state_bytes(B, H, W, NS), 16), &go);
    if (!go) return rc;
    fr::PhArgs a{};
    a.tex_img = tex_img; a.normal = normal; a.tri_ind = tri_ind; a.light = light; a.target = target; a.weight = weight;
    a.part = (double*)state; a.HW = H * W; a.tiles = ph_tiles(H, W); a.gain = gain; a.offset = offset;
    hipLaunchKernelGGL(pass, dim3((unsigned)a.tiles, (unsigned)B, 1), dim3(fr::PH_TILE, 1, 1), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::photo_loss_finish_kernel<NS>, dim3((unsigned)B, 1, 1), dim3(fr::PH_FIN, 1, 1), 0, (hipStream_t)stream,
                       (const double*)a.part, a.tiles, sums);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int ph_backward(PhKernel pass, const double* grad_sse, const double* sums, const float* tex_img, const float* normal,
                const float* tri_ind, const float* light, const float* target, const float* weight, int B, int H, int W, float gain,
                float offset, float* grad_tex_img, float* grad_normal, float* grad_light, void* stream) {
    bool go;
    const int rc = ph_check(B, H, W, grad_sse && tex_img && normal && tri_ind && light && target && (sums || !grad_light), true, &go);
    if (!go) return rc;
    if (!grad_tex_img && !grad_normal && !grad_light) return FR_OK;   // nothing is wanted
    fr::PhArgs a{};
    a.tex_img = tex_img; a.normal = normal; a.tri_ind = tri_ind; a.light = light; a.target = target; a.weight = weight;
    a.sums = sums; a.grad_sse = grad_sse; a.g_tex = grad_tex_img; a.g_normal = grad_normal; a.g_light = grad_light;
    a.HW = H * W; a.tiles = ph_tiles(H, W); a.gain = gain; a.offset = offset;
    hipLaunchKernelGGL(pass, dim3((unsigned)a.tiles, (unsigned)B, 1), dim3(fr::PH_TILE, 1, 1), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
}  // namespace

extern "C" {

size_t fr_photo_loss_state_bytes(int B, int H, int W) { return ph_state_bytes(B, H, W, fr::PH_SUMS<fr::GrayModel>); }
size_t fr_photo_loss_rgb_state_bytes(int B, int H, int W) { return ph_state_bytes(B, H, W, fr::PH_SUMS<fr::ColourModel>); }

void fr_debug_photo_loss_geom(int B, int H, int W, int* out) { ph_geom(B, H, W, fr::PH_SUMS<fr::GrayModel>, out); }
void fr_debug_photo_loss_rgb_geom(int B, int H, int W, int* out) { ph_geom(B, H, W, fr::PH_SUMS<fr::ColourModel>, out); }

int fr_photo_loss_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* target,
                          const float* weight, int B, int H, int W, float gain, float offset, double* sums, void* state,
                          size_t state_bytes, void* stream) {
    return ph_forward<fr::GrayModel>(fr::photo_loss_forward_kernel, tex_img, normal, tri_ind, light, target, weight, B, H, W, gain,
                                     offset, sums, state, state_bytes, stream);
}

int fr_photo_loss_rgb_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* target,
                              const float* weight, int B, int H, int W, float gain, float offset, double* sums, void* state,
                              size_t state_bytes, void* stream) {
    return ph_forward<fr::ColourModel>(fr::photo_loss_rgb_forward_kernel, tex_img, normal, tri_ind, light, target, weight, B, H, W,
                                       gain, offset, sums, state, state_bytes, stream);
}

int fr_photo_loss_backward(const double* grad_sse, const double* sums, const float* tex_img, const float* normal, const float* tri_ind,
                           const float* light, const float* target, const float* weight, int B, int H, int W, float gain,
                           float offset, float* grad_tex_img, float* grad_normal, float* grad_light, void* stream) {
    return ph_backward(fr::photo_loss_backward_kernel, grad_sse, sums, tex_img, normal, tri_ind, light, target, weight, B, H, W, gain,
                       offset, grad_tex_img, grad_normal, grad_light, stream);
}

int fr_photo_loss_rgb_backward(const double* grad_sse, const double* sums, const float* tex_img, const float* normal,
                               const float* tri_ind, const float* light, const float* target, const float* weight, int B, int H, int W,
                               float gain, float offset, float* grad_tex_img, float* grad_normal, float* grad_light, void* stream) {
    return ph_backward(fr::photo_loss_rgb_backward_kernel, grad_sse, sums, tex_img, normal, tri_ind, light, target, weight, B, H, W,
                       gain, offset, grad_tex_img, grad_normal, grad_light, stream);
}

}  // extern "C"
