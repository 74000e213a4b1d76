// Fine-depth losses (opt-in; include/fr_hotpath.h, "fine-depth losses"): the fidelity term mean((z - c)^2) and the smoothness term
// sum |Laplacian(z)| of the fine depth map in ONE streaming pass, and their gradients in one more.  Float64 arithmetic, every product
// and sum rounded on its own; both sums in an association that is a function of (B, H, W) alone.
//
//   fine_losses_forward_kernel    a workgroup owns an FL_TW x FL_TH = 32 x 16 pixel tile of one face, one lane per pixel.  Every lane
//                                 reads its own nine-point stencil straight from global memory (the neighbours' lines are the
//                                 workgroup's own L1 lines; clamped offsets, so the nine loads go out together) and its coarse depth,
//                                 forms (z - c)^2 and |L|, and the 512 pairs meet in a fixed tree: inside a wave by lane shuffles
//                                 (strides 32 .. 1), then the eight wave sums in LDS (strides 4, 2, 1).  Two float64 partials per tile.
//   fine_losses_finish_kernel     one workgroup of FL_FIN = 1,024 threads: thread i chains the partials i, i + 1024, ... from +0.0 (six
//                                 dependent additions at 64 faces of 200 x 200, not 5,824), then the same wave tree and the sixteen
//                                 wave sums (strides 8, 4, 2, 1); writes S_f, S_s and the two fp32 scalars.
//                                 CHOICE: a SECOND SMALL LAUNCH, not a last-workgroup-done counter: the counter would need a cleared
//                                 word in the state (a memset node or a third launch) and a device-scope fence and atomic per tile;
//                                 the launch costs a few microseconds of an idle stream and keeps the state write-only.
//   fine_losses_backward_kernel   the same tile, a gather.  CHOICE: the signs s(L) are RECOMPUTED FROM A STAGED z TILE, not read from a
//                                 sign plane the forward would write.  The workgroup stages z with a 2-pixel halo in LDS (20 x 36
//                                 floats), then s(L) with a 1-pixel halo (18 x 34: 612 evaluations for 512 outputs, 1.2 per output,
//                                 each nine LDS reads), then every lane adds its nine taps.  A sign plane would add 1 byte per pixel
//                                 written by the forward and 1 read by the backward -- an eighth more bytes in each direction -- tie a
//                                 state of B H W bytes to every call in flight, and still need the 1-pixel halo.
// The forward's lane and the backward's halo lanes run the SAME device function (fl_laplacian) on the same nine values, so a pixel's
// sign is the same bits wherever it is evaluated.  No atomics.
#include "fr_common.h"

namespace fr {

constexpr int FL_TW = 32, FL_TH = 16;               // tile: one lane per pixel
constexpr int FL_THREADS = FL_TW * FL_TH;           // 8 waves
constexpr int FL_WAVES = FL_THREADS / 64;
constexpr int FL_FIN = 1024, FL_FIN_WAVES = FL_FIN / 64;   // the finish step's one workgroup
constexpr int FL_ZW = FL_TW + 4, FL_ZH = FL_TH + 4;        // staged z tile: 2-pixel halo
constexpr int FL_SW = FL_TW + 2, FL_SH = FL_TH + 2;        // staged sign tile: 1-pixel halo

struct FlArgs {
    const float* pred;     // [B,H,W]
    const float* coarse;   // [B,H,W]
    const float* gf;       // one fp32 on the device, or null   (backward)
    const float* gs;       // one fp32 on the device, or null   (backward)
    double* part;          // [2][P] tile partials               (forward)
    float* gp;             // [B,H,W]                            (backward)
    float* gc;             // [B,H,W] or null                    (backward)
    double cf;             // 2 / (B H W)                        (backward)
    long long P;           // tiles across x tiles down x B
    int H, W;
};

// a face's depth plane in global memory / the staged tile in LDS: z(r, c) for an IN-IMAGE (r, c)
struct FlGlobalZ {
    const float* z;
    int W;
    __device__ __forceinline__ float operator()(int r, int c) const { return z[(size_t)r * W + c]; }
};
struct FlTileZ {
    const float (*z)[FL_ZW];
    int r0, c0;   // image position of tile element [2][2]
    __device__ __forceinline__ float operator()(int r, int c) const { return z[r - r0 + 2][c - c0 + 2]; }
};

// L at an in-image pixel: the nine taps in row-major order from +0.0, k = ((0.5, 1, 0.5), (1, -6, 1), (0.5, 1, 0.5)); a tap outside
// the image is not added.  The nine values are read together at clamped positions -- a tap outside the image reads a pixel inside it
// and is selected away, never multiplied.
template <typename Z>
__device__ __forceinline__ double fl_laplacian(const Z& z, int r, int c, int H, int W) {
    const bool u = r > 0, d = r + 1 < H, l = c > 0, rt = c + 1 < W;
    const int ru = u ? r - 1 : r, rd = d ? r + 1 : r, cl = l ? c - 1 : c, cr = rt ? c + 1 : c;
    const float z00 = z(ru, cl), z01 = z(ru, c), z02 = z(ru, cr);
    const float z10 = z(r, cl), z11 = z(r, c), z12 = z(r, cr);
    const float z20 = z(rd, cl), z21 = z(rd, c), z22 = z(rd, cr);
    double L = 0.0;
    L = (u && l) ? L + 0.5 * (double)z00 : L;
    L = u ? L + 1.0 * (double)z01 : L;
    L = (u && rt) ? L + 0.5 * (double)z02 : L;
    L = l ? L + 1.0 * (double)z10 : L;
    L = L + -6.0 * (double)z11;
    L = rt ? L + 1.0 * (double)z12 : L;
    L = (d && l) ? L + 0.5 * (double)z20 : L;
    L = d ? L + 1.0 * (double)z21 : L;
    L = (d && rt) ? L + 0.5 * (double)z22 : L;
    return L;
}

// s(x) = (x > 0) - (x < 0): s(+-0) = 0, s(NaN) = 0
__device__ __forceinline__ float fl_sign(double x) { return (float)((int)(x > 0.0) - (int)(x < 0.0)); }

// the tree inside a wave: lane l adds lane l + k for k = 32, 16, .. 1; lane 0 ends with the wave's sum (every lane takes part)
__device__ __forceinline__ double fl_wave_tree(double v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_down(v, (unsigned)k, 64);
    return v;
}

__global__ __launch_bounds__(FL_THREADS) void fine_losses_forward_kernel(FlArgs a) {
    __shared__ double wf[FL_WAVES], wl[FL_WAVES];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * FL_TW + tx;
    const int c = blockIdx.x * FL_TW + tx, r = blockIdx.y * FL_TH + ty;
    const size_t face = (size_t)blockIdx.z * ((size_t)a.H * a.W);
    double f = 0.0, s = 0.0;   // a lane outside the image: +0.0
    if (r < a.H && c < a.W) {
        const size_t at = (size_t)r * a.W + c;
        const float cp = a.coarse[face + at], zp = a.pred[face + at];
        const double L = fl_laplacian(FlGlobalZ{a.pred + face, a.W}, r, c, a.H, a.W);
        const double d = (double)zp - (double)cp;
        f = d * d;
        s = __builtin_fabs(L);
    }
    f = fl_wave_tree(f);
    s = fl_wave_tree(s);
    if ((t & 63) == 0) {
        wf[t >> 6] = f;
        wl[t >> 6] = s;
    }
    __syncthreads();
    if (t == 0) {
        const long long p = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.part[p] = ((wf[0] + wf[4]) + (wf[2] + wf[6])) + ((wf[1] + wf[5]) + (wf[3] + wf[7]));
        a.part[a.P + p] = ((wl[0] + wl[4]) + (wl[2] + wl[6])) + ((wl[1] + wl[5]) + (wl[3] + wl[7]));
    }
}

__global__ __launch_bounds__(FL_FIN) void fine_losses_finish_kernel(const double* part, long long P, double n, double* sums,
                                                                     float* fidelity, float* smoothness) {
    __shared__ double wf[FL_FIN_WAVES], wl[FL_FIN_WAVES];
    const int t = threadIdx.x;
    double f = 0.0, s = 0.0;
    for (long long p = t; p < P; p += FL_FIN) {
        f = f + part[p];
        s = s + part[P + p];
    }
    f = fl_wave_tree(f);
    s = fl_wave_tree(s);
    if ((t & 63) == 0) {
        wf[t >> 6] = f;
        wl[t >> 6] = s;
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int k = FL_FIN_WAVES / 2; k >= 1; k >>= 1) {
#pragma unroll
            for (int i = 0; i < k; i++) {
                wf[i] = wf[i] + wf[i + k];
                wl[i] = wl[i] + wl[i + k];
            }
        }
        sums[0] = wf[0];
        sums[1] = wl[0];
        *fidelity = (float)(wf[0] / n);
        *smoothness = (float)wl[0];
    }
}

__global__ __launch_bounds__(FL_THREADS) void fine_losses_backward_kernel(FlArgs a) {
    __shared__ float zt[FL_ZH][FL_ZW];
    __shared__ float st[FL_SH][FL_SW];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * FL_TW + tx;
    const int c0 = blockIdx.x * FL_TW, r0 = blockIdx.y * FL_TH;
    const int r = r0 + ty, c = c0 + tx;
    const size_t face = (size_t)blockIdx.z * ((size_t)a.H * a.W);
    const float* z = a.pred + face;
    const bool in = r < a.H && c < a.W;
    double T = 0.0;
    if (a.gs) {   // (the same for every workgroup of the launch)
        for (int i = t; i < FL_ZH * FL_ZW; i += FL_THREADS) {
            const int j = i / FL_ZW, k = i - j * FL_ZW;
            const int rr = r0 - 2 + j, cc = c0 - 2 + k;
            const bool ok = rr >= 0 && rr < a.H && cc >= 0 && cc < a.W;
            zt[j][k] = ok ? z[(size_t)rr * a.W + cc] : 0.0f;   // (a position outside the image is never read back)
        }
        __syncthreads();
        for (int i = t; i < FL_SH * FL_SW; i += FL_THREADS) {
            const int j = i / FL_SW, k = i - j * FL_SW;
            const int rr = r0 - 1 + j, cc = c0 - 1 + k;
            const bool ok = rr >= 0 && rr < a.H && cc >= 0 && cc < a.W;
            // a position outside the image has no L: its tap contributes nothing, which a sign of 0 says exactly
            st[j][k] = ok ? fl_sign(fl_laplacian(FlTileZ{zt, r0, c0}, rr, cc, a.H, a.W)) : 0.0f;
        }
        __syncthreads();
        T = T + 0.5 * (double)st[ty][tx];
        T = T + 1.0 * (double)st[ty][tx + 1];
        T = T + 0.5 * (double)st[ty][tx + 2];
        T = T + 1.0 * (double)st[ty + 1][tx];
        T = T + -6.0 * (double)st[ty + 1][tx + 1];
        T = T + 1.0 * (double)st[ty + 1][tx + 2];
        T = T + 0.5 * (double)st[ty + 2][tx];
        T = T + 1.0 * (double)st[ty + 2][tx + 1];
        T = T + 0.5 * (double)st[ty + 2][tx + 2];
    }
    if (!in) return;
    const size_t at = face + (size_t)r * a.W + c;
    double fid = 0.0;
    if (a.gf) fid = ((double)a.gf[0] * a.cf) * ((double)a.pred[at] - (double)a.coarse[at]);
    float out = 0.0f;
    if (a.gf && a.gs) out = (float)(fid + (double)a.gs[0] * T);
    else if (a.gf) out = (float)fid;
    else if (a.gs) out = (float)((double)a.gs[0] * T);
    a.gp[at] = out;
    if (a.gc) a.gc[at] = a.gf ? (float)(-fid) : 0.0f;
}

}  // namespace fr

// The launch geometry and the state's layout, chosen in ONE place: the size query, the launchers and the test hook read them from here.
namespace {
struct FlGeom {
    int tiles_x, tiles_y;
    long long P;   // tile partials per sum
};
FlGeom fl_geom(int B, int H, int W) {
    FlGeom g;
    g.tiles_x = (W + fr::FL_TW - 1) / fr::FL_TW;
    g.tiles_y = (H + fr::FL_TH - 1) / fr::FL_TH;
    g.P = (long long)g.tiles_x * g.tiles_y * B;
    return g;
}
// more than 2^31 - 65 pixels per face, or a grid the runtime does not take (faces in z, tile rows in y: 65,535 each)
bool fl_size_ok(int B, int H, int W) {
    return (long long)H * W <= 0x7FFFFFFFll - 64 && B <= 65535 && (H + fr::FL_TH - 1) / fr::FL_TH <= 65535;
}
// state: S_f, S_s, then the tile partials of the fidelity sum, then those of the smoothness sum; float64.  0 for an empty shape or
// one the launchers refuse.
size_t fl_state_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !fl_size_ok(B, H, W)) return 0;
    return (size_t)(2 + 2 * fl_geom(B, H, W).P) * sizeof(double);
}
constexpr size_t FL_LDS_BWD = (size_t)(fr::FL_ZH * fr::FL_ZW + fr::FL_SH * fr::FL_SW) * sizeof(float);

// What the two launching entry points share, in the order both answer: a negative size (FR_ERR_INVALID_ARG), an empty shape (FR_OK,
// nothing launched), the entry point's own pointers (FR_ERR_INVALID_ARG), its state (FR_ERR_WORKSPACE), a shape beyond one grid
// (FR_ERR_UNSUPPORTED).  FR_OK with *go = true: launch.
int fl_check(int B, int H, int W, bool pointers_ok, bool state_ok, bool* go) {
    *go = false;
    if (B < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!pointers_ok) return FR_ERR_INVALID_ARG;
    if (!state_ok) return FR_ERR_WORKSPACE;
    if (!fl_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    *go = true;
    return FR_OK;
}
}  // namespace

extern "C" {

size_t fr_fine_losses_state_bytes(int B, int H, int W) { return fl_state_bytes(B, H, W); }

// test hook: out = {tile width, tile height, threads per workgroup, tiles across, tiles down, threads of the finish workgroup, static
// LDS bytes of a backward workgroup}; zeros for an empty shape or one the launchers refuse
void fr_debug_fine_losses_geom(int B, int H, int W, int* out) {
    for (int i = 0; i < 7; i++) out[i] = 0;
    if (B <= 0 || H <= 0 || W <= 0 || !fl_size_ok(B, H, W)) return;
    const FlGeom g = fl_geom(B, H, W);
    out[0] = fr::FL_TW; out[1] = fr::FL_TH; out[2] = fr::FL_THREADS; out[3] = g.tiles_x; out[4] = g.tiles_y;
    out[5] = fr::FL_FIN; out[6] = (int)FL_LDS_BWD;
}

int fr_fine_losses_forward(const float* pred, const float* coarse, int B, int H, int W, float* fidelity, float* smoothness,
                           void* state, size_t state_bytes, void* stream) {
    bool go;
    const int rc = fl_check(B, H, W, pred && coarse && fidelity && smoothness,
                            ws_ok(state, state_bytes, fl_state_bytes(B, H, W), 16), &go);
    if (!go) return rc;
    const FlGeom g = fl_geom(B, H, W);
    double* sums = (double*)state;
    fr::FlArgs a{};
    a.pred = pred; a.coarse = coarse; a.part = sums + 2; a.P = g.P; a.H = H; a.W = W;
    hipLaunchKernelGGL(fr::fine_losses_forward_kernel, dim3((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)B),
                       dim3(fr::FL_TW, fr::FL_TH, 1), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::fine_losses_finish_kernel, dim3(1), dim3(fr::FL_FIN), 0, (hipStream_t)stream, (const double*)(sums + 2),
                       g.P, (double)B * (double)H * (double)W, sums, fidelity, smoothness);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_fine_losses_backward(const float* grad_fidelity, const float* grad_smoothness, const float* pred, const float* coarse, int B,
                            int H, int W, float* grad_pred, float* grad_coarse, void* stream) {
    bool go;
    const int rc = fl_check(B, H, W, pred && coarse && grad_pred, true, &go);
    if (!go) return rc;
    const FlGeom g = fl_geom(B, H, W);
    fr::FlArgs a{};
    a.pred = pred; a.coarse = coarse; a.gf = grad_fidelity; a.gs = grad_smoothness; a.gp = grad_pred; a.gc = grad_coarse;
    a.cf = 2.0 / ((double)B * (double)H * (double)W);
    a.H = H; a.W = W;
    hipLaunchKernelGGL(fr::fine_losses_backward_kernel, dim3((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)B),
                       dim3(fr::FL_TW, fr::FL_TH, 1), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
