// Photometric loss (opt-in; include/fr_hotpath.h, "photometric loss"): the shader's image compared with a target picture, per face, in
// ONE streaming pass, and its gradients with respect to the render's planes and the lighting in one more.
//
//   photo_loss_forward_kernel   a workgroup owns PH_TILE = 256 consecutive pixels of one face, one lane per pixel, as the shader does.
//                               A covered lane runs the shader's own device function (fr_shade.h) and forms, in float64, the six terms
//                               of the header; the 256 x 6 values meet in a fixed tree: inside a wave by lane shuffles (strides
//                               32 .. 1; fr::wave_tree_f64), then the four wave sums as (w0 + w2) + (w1 + w3).  Six float64 partials per tile.
//   photo_loss_finish_kernel    one workgroup of PH_FIN = 256 threads per face: thread i chains that face's partials i, i + 256, ..
//                               from +0.0 (one addition at 200 x 200: 157 tiles), then the same tree.  Writes sums[b][0 .. 6).
//                               CHOICE: the four lighting sums are taken HERE, in the forward: they are linear in the upstream
//                               gradient, so the backward is a pure map -- no reduction, no second launch -- and the forward is
//                               memory-bound with or without them.
//   photo_loss_backward_kernel  the same lane-per-pixel map: recomputes the shading (the same device function, the same bits), writes
//                               every element of the planes that were asked for (zeros off the face), and the four lighting
//                               gradients from sums.  grad_sse is read from the device.
// Float64 products and sums each rounded on their own (-ffp-contract=off).  No atomics.
#include "fr_common.h"
#include "fr_shade.h"

namespace fr {

constexpr int PH_TILE = 256, PH_WAVES = PH_TILE / 64, PH_FIN = 256, PH_SUMS = 6;

struct PhArgs {
    const float* tex_img;   // [B,H,W,3]
    const float* normal;    // [B,H,W,3]
    const float* tri_ind;   // [B,H,W]
    const float* light;     // [B,4]
    const float* target;    // [B,H,W]
    const float* weight;    // [B,H,W] or null
    const double* sums;     // [B,6]                      (backward, for grad_light)
    const double* grad_sse; // [B]                        (backward)
    double* part;           // [B][tiles][6]              (forward)
    float* g_tex;           // [B,H,W,3] or null          (backward)
    float* g_normal;        // [B,H,W,3] or null          (backward)
    float* g_light;         // [B,4] or null              (backward)
    int HW, tiles;
    float gain, offset;
};

// what both directions need of a covered pixel: the shading, and t = ((2 w) r) gain in float64
struct PhPixel {
    Shade sh;
    double r, w, t;
};
__device__ __forceinline__ void ph_pixel(const PhArgs& a, int b, size_t i, PhPixel& p) {
    const float I = shade_pixel(a.tex_img[3 * i], a.tex_img[3 * i + 1], a.tex_img[3 * i + 2], a.normal[3 * i], a.normal[3 * i + 1],
                                a.normal[3 * i + 2], a.light + (size_t)b * 4, p.sh);
    const float im = I * a.gain + a.offset;
    p.w = a.weight ? (double)a.weight[i] : 1.0;
    p.r = (double)im - (double)a.target[i];
    p.t = ((2.0 * p.w) * p.r) * (double)a.gain;
}

// the tree over a workgroup's 256 slots, for six values at once; thread 0 ends with the six sums in v
__device__ __forceinline__ void ph_block_tree(double (&v)[PH_SUMS], double (*ws)[PH_WAVES]) {
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < PH_SUMS; j++) v[j] = wave_tree_f64(v[j]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int j = 0; j < PH_SUMS; j++) ws[j][t >> 6] = v[j];
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < PH_SUMS; j++) v[j] = (ws[j][0] + ws[j][2]) + (ws[j][1] + ws[j][3]);
    }
}

__global__ __launch_bounds__(PH_TILE) void photo_loss_forward_kernel(const PhArgs a) {
    __shared__ double ws[PH_SUMS][PH_WAVES];
    const unsigned int pix = blockIdx.x * (unsigned)PH_TILE + threadIdx.x;
    const int b = (int)blockIdx.y;
    double v[PH_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // a slot outside the image or off the face: +0.0
    if (pix < (unsigned int)a.HW) {
        const size_t i = (size_t)b * (size_t)a.HW + pix;
        if (a.tri_ind[i] >= 0.0f) {
            PhPixel p;
            ph_pixel(a, b, i, p);
            const double u = p.sh.s > 0.0f ? p.t * (double)p.sh.a : 0.0;
            v[0] = (p.w * p.r) * p.r;
            v[1] = 1.0;
            v[2] = u;
            v[3] = u * (double)p.sh.hx;
            v[4] = u * (double)p.sh.hy;
            v[5] = u * (double)p.sh.hz;
        }
    }
    ph_block_tree(v, ws);
    if (threadIdx.x == 0) {
        double* out = a.part + ((size_t)b * a.tiles + blockIdx.x) * PH_SUMS;
#pragma unroll
        for (int j = 0; j < PH_SUMS; j++) out[j] = v[j];
    }
}

__global__ __launch_bounds__(PH_FIN) void photo_loss_finish_kernel(const double* __restrict__ part, int tiles, double* __restrict__ sums) {
    __shared__ double ws[PH_SUMS][PH_WAVES];
    const int b = (int)blockIdx.x;
    const double* mine = part + (size_t)b * tiles * PH_SUMS;
    double v[PH_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = (int)threadIdx.x; p < tiles; p += PH_FIN) {
#pragma unroll
        for (int j = 0; j < PH_SUMS; j++) v[j] = v[j] + mine[(size_t)p * PH_SUMS + j];
    }
    ph_block_tree(v, ws);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < PH_SUMS; j++) sums[(size_t)b * PH_SUMS + j] = v[j];
    }
}

__global__ __launch_bounds__(PH_TILE) void photo_loss_backward_kernel(const PhArgs a) {
    const unsigned int pix = blockIdx.x * (unsigned)PH_TILE + threadIdx.x;
    const int b = (int)blockIdx.y;
    const double g = a.grad_sse[b];
    if (a.g_light && blockIdx.x == 0 && threadIdx.x < 4)
        a.g_light[(size_t)b * 4 + threadIdx.x] = (float)(g * a.sums[(size_t)b * PH_SUMS + 2 + threadIdx.x]);
    if (pix >= (unsigned int)a.HW) return;
    const size_t i = (size_t)b * (size_t)a.HW + pix;
    float gt[3] = {0.0f, 0.0f, 0.0f}, gn[3] = {0.0f, 0.0f, 0.0f};
    if (a.tri_ind[i] >= 0.0f) {
        PhPixel p;
        ph_pixel(a, b, i, p);
        const Shade& sh = p.sh;
        const double dI = g * p.t;
        const bool lit = sh.s > 0.0f;
        if (a.g_tex) {
            const float gc = (float)((dI * (double)sh.s) * (1.0 / 3.0));
#pragma unroll
            for (int c = 0; c < 3; c++) gt[c] = (lit && !(a.tex_img[3 * i + c] < 1e-6f)) ? gc : 0.0f;
        }
        if (a.g_normal) {
            const float* l = a.light + (size_t)b * 4;
            const double q = lit ? dI * (double)sh.a : 0.0;
            const double gx = q * (double)l[1], gy = q * (double)l[2], gz = q * (double)l[3];
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
    }
    if (a.g_tex) { a.g_tex[3 * i] = gt[0]; a.g_tex[3 * i + 1] = gt[1]; a.g_tex[3 * i + 2] = gt[2]; }
    if (a.g_normal) { a.g_normal[3 * i] = gn[0]; a.g_normal[3 * i + 1] = gn[1]; a.g_normal[3 * i + 2] = gn[2]; }
}

}  // namespace fr

// The launch geometry and the state's layout, chosen in ONE place: the size query, the launchers and the test hook read them from here.
namespace {
// more than 2^31 - 1 pixels per face (the pixel index is a 32-bit word), or more faces than the grid's y takes
bool ph_size_ok(int B, int H, int W) { return (long long)H * W <= 0x7FFFFFFFll && B <= 65535; }
int ph_tiles(int H, int W) { return (int)(((long long)H * W + fr::PH_TILE - 1) / fr::PH_TILE); }
// state: the tile partials [B][tiles][6], float64.  0 for an empty shape or one the launchers refuse.
size_t ph_state_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !ph_size_ok(B, H, W)) return 0;
    return (size_t)B * (size_t)ph_tiles(H, W) * fr::PH_SUMS * sizeof(double);
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
}  // namespace

extern "C" {

size_t fr_photo_loss_state_bytes(int B, int H, int W) { return ph_state_bytes(B, H, W); }

// test hook: out = {pixels per tile, tiles per face, threads of the finish workgroup, sums per face}
void fr_debug_photo_loss_geom(int B, int H, int W, int* out) {
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (B <= 0 || H <= 0 || W <= 0 || !ph_size_ok(B, H, W)) return;
    out[0] = fr::PH_TILE; out[1] = ph_tiles(H, W); out[2] = fr::PH_FIN; out[3] = fr::PH_SUMS;
}

int fr_photo_loss_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* light, const float* target,
                          const float* weight, int B, int H, int W, float gain, float offset, double* sums, void* state,
                          size_t state_bytes, void* stream) {
    bool go;
    const int rc = ph_check(B, H, W, tex_img && normal && tri_ind && light && target && sums,
                            ws_ok(state, state_bytes, ph_state_bytes(B, H, W), 16), &go);
    if (!go) return rc;
    fr::PhArgs a{};
    a.tex_img = tex_img; a.normal = normal; a.tri_ind = tri_ind; a.light = light; a.target = target; a.weight = weight;
    a.part = (double*)state; a.HW = H * W; a.tiles = ph_tiles(H, W); a.gain = gain; a.offset = offset;
    hipLaunchKernelGGL(fr::photo_loss_forward_kernel, dim3((unsigned)a.tiles, (unsigned)B, 1), dim3(fr::PH_TILE, 1, 1), 0,
                       (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::photo_loss_finish_kernel, dim3((unsigned)B, 1, 1), dim3(fr::PH_FIN, 1, 1), 0, (hipStream_t)stream,
                       (const double*)a.part, a.tiles, sums);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_photo_loss_backward(const double* grad_sse, const double* sums, const float* tex_img, const float* normal, const float* tri_ind,
                           const float* light, const float* target, const float* weight, int B, int H, int W, float gain,
                           float offset, float* grad_tex_img, float* grad_normal, float* grad_light, void* stream) {
    bool go;
    const int rc = ph_check(B, H, W, grad_sse && tex_img && normal && tri_ind && light && target && (sums || !grad_light), true, &go);
    if (!go) return rc;
    if (!grad_tex_img && !grad_normal && !grad_light) return FR_OK;   // nothing is wanted
    fr::PhArgs a{};
    a.tex_img = tex_img; a.normal = normal; a.tri_ind = tri_ind; a.light = light; a.target = target; a.weight = weight;
    a.sums = sums; a.grad_sse = grad_sse; a.g_tex = grad_tex_img; a.g_normal = grad_normal; a.g_light = grad_light;
    a.HW = H * W; a.tiles = ph_tiles(H, W); a.gain = gain; a.offset = offset;
    hipLaunchKernelGGL(fr::photo_loss_backward_kernel, dim3((unsigned)a.tiles, (unsigned)B, 1), dim3(fr::PH_TILE, 1, 1), 0,
                       (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
