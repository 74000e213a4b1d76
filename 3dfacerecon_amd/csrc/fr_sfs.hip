// Shape-from-shading term (opt-in; include/fr_hotpath.h, "shape-from-shading term"): the per-pixel lighting solve of
// get_spherical_harmonics_model (nets/network.py:424-460) and the shading it feeds, one streaming pass per direction.
//
//   sfs_forward_kernel    a workgroup owns SFS_PX = 64 consecutive pixels and S = sfs_slices(B) waves; wave s streams the maps of
//                         its contiguous share of the faces (per face a wave's 64 pixels are 768 contiguous bytes of a normal
//                         plane) into nine float64 sums per lane; the partial sums meet in LDS and wave 0 adds them in slice
//                         order, solves the pixel's 3 x 3 (fr_sfs_pinv.h: fixed sweep count), writes the ten state planes and
//                         leaves l in LDS; every wave then shades its own faces.
//   sfs_backward_kernel   the same split: three sums q per lane, combined in the same order; s = P q from the state; every wave
//                         writes the gradients of its own faces.
// The split entry points (opt-in; "shape-from-shading term across ranks") cut both passes where the batch couples, so that the sums
// of several ranks' faces can meet between the halves; they are built from the SAME device functions as the two kernels above:
//   sfs_moments_kernel          the forward's streaming half: the nine sums of this call's faces -> nine float64 planes (a "part").
//   sfs_solve_shade_kernel      wave 0 adds the parts in ascending part index, solves, writes the state, leaves l in LDS; every wave
//                               shades its own faces.
//   sfs_backward_q_kernel       the backward's streaming half: the three sums q of this call's faces -> three planes.
//   sfs_backward_apply_kernel   every wave adds the q parts in ascending part index (no LDS, no barrier), s = P q, and writes the
//                               gradients of its own faces.
// No atomics; the association of every sum is a function of B alone (sfs_slices / sfs_chunk below) and, for the split route, of the
// parts and their order.
#include "fr_common.h"
#include "fr_sfs_pinv.h"

#include <cmath>

#ifndef FR_SFS_SLICES_MAX
#define FR_SFS_SLICES_MAX 4   // (a build with another cap: tools/sfs_probe.py --alt-lib times it beside this one)
#endif

namespace fr {

constexpr int SFS_PX = 64;   // pixels per workgroup: one per lane

// batch slices per pixel and faces per slice: functions of B ALONE (they fix the association of the sums over b)
__host__ __device__ inline int sfs_slices(int B) {
    const int s = B / 4;   // a slice is worth a wave from four faces up
    return s < 1 ? 1 : (s > FR_SFS_SLICES_MAX ? FR_SFS_SLICES_MAX : s);
}
__host__ __device__ inline int sfs_chunk(int B, int S) { return (B + S - 1) / S; }

struct SfsArgs {
    const float* abedo;       // [B,npix]
    const float* normal;      // [B,npix,3]
    const float* im_gray;     // [B,npix]
    const float* abedo_new;   // [B,npix]
    const float* normal_new;  // [B,npix,3]
    const float* g;           // [B,npix]     (backward)
    float* intensity;         // [B,npix]     (forward)
    float* gn;                // [B,npix,3]   (backward, may be null)
    float* gnn;               // [B,npix,3]   (backward, may be null)
    float* gan;               // [B,npix]     (backward, may be null): the gradient of abedo_new
    double* state;            // [10,npix]
    double* parts_out;        // [9,npix] or [3,npix]            (split route: this call's sums)
    const double* parts_in;   // [nparts,9,npix] or [nparts,3,npix]   (split route: every part's sums)
    double rcond;
    int B, npix, S, chunk, nparts;
};

// ---- the pieces both routes are made of (one text: the one-call kernels and the split kernels run the same operations) ----------

// the nine sums of the faces [b0, b1) at pixel p, ascending b onto +0.0: m[0..5] = M as xx, xy, xz, yy, yz, zz; m[6..8] = r
__device__ __forceinline__ void sfs_sum_moments(const SfsArgs& a, int b0, int b1, size_t p, double (&m)[9]) {
    const size_t npix = (size_t)a.npix;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll 4
    for (int b = b0; b < b1; b++) {
        const size_t i = (size_t)b * npix + p;
        const float* n = a.normal + i * 3;
        const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
        const double u = (double)a.im_gray[i] / ((double)a.abedo[i] + 1.0);
        m0 = m0 + nx * nx; m1 = m1 + nx * ny; m2 = m2 + nx * nz;
        m3 = m3 + ny * ny; m4 = m4 + ny * nz; m5 = m5 + nz * nz;
        r0 = r0 + nx * u; r1 = r1 + ny * u; r2 = r2 + nz * u;
    }
    m[0] = m0; m[1] = m1; m[2] = m2; m[3] = m3; m[4] = m4; m[5] = m5; m[6] = r0; m[7] = r1; m[8] = r2;
}

// the slices' sums meet in LDS ([K][S][64]): slices above 0 store theirs, and after the barrier slice 0 adds them onto its own in
// slice order, ((s0 + s1) + s2) + ...   Every thread of the workgroup calls this (it holds a barrier).
template <int K>
__device__ __forceinline__ void sfs_meet_in_slice0(double* part, int S, int slice, int lane, double (&m)[K]) {
    const int st = S * SFS_PX;
    if (slice > 0) {
        double* q = part + slice * SFS_PX + lane;
#pragma unroll
        for (int k = 0; k < K; k++) q[k * st] = m[k];
    }
    __syncthreads();
    if (slice == 0) {
        for (int s = 1; s < S; s++) {
            const double* q = part + s * SFS_PX + lane;
#pragma unroll
            for (int k = 0; k < K; k++) m[k] = m[k] + q[k * st];
        }
    }
}

// rows of a symmetric 3 x 3 (xx, xy, xz, yy, yz, zz) times a vector: (P_i0 v_0 + P_i1 v_1) + P_i2 v_2
__device__ __forceinline__ void sfs_rows(const double (&P)[6], double v0, double v1, double v2, double& x, double& y, double& z) {
    x = (P[0] * v0 + P[1] * v1) + P[2] * v2;
    y = (P[1] * v0 + P[3] * v1) + P[4] * v2;
    z = (P[2] * v0 + P[4] * v1) + P[5] * v2;
}

// the nine total sums of one pixel -> P, l, rank; the state planes where the pixel exists; l into LDS for the shading pass
__device__ __forceinline__ void sfs_solve_pixel(const SfsArgs& a, const double (&m)[9], size_t p, bool active, double* lsh, int lane) {
    const size_t npix = (size_t)a.npix;
    const double m6[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
    const double r0 = m[6], r1 = m[7], r2 = m[8];
    double P[6];
    int rank;
    fr_sfs_pinv3(m6, a.rcond, P, &rank);
    double lx, ly, lz;
    sfs_rows(P, r0, r1, r2, lx, ly, lz);
    // a non-finite right-hand side (an Inf or NaN in im_gray / abedo) must not pass for a finite l through a zero of P
    const double poison = ((r0 + r1) + r2) * 0.0;
    if (!(poison == 0.0)) { lx = poison; ly = poison; lz = poison; }
    lsh[lane] = lx; lsh[SFS_PX + lane] = ly; lsh[2 * SFS_PX + lane] = lz;
    if (active) {
        double* st8 = a.state + p;
#pragma unroll
        for (int k = 0; k < 6; k++) st8[(size_t)k * npix] = P[k];
        st8[6 * npix] = lx; st8[7 * npix] = ly; st8[8 * npix] = lz;
        st8[9 * npix] = (double)rank;
    }
}

// intensity_b = fl32(a'_b (l . n'_b)) for the faces [b0, b1) at pixel p
__device__ __forceinline__ void sfs_shade(const SfsArgs& a, int b0, int b1, size_t p, double lx, double ly, double lz) {
    const size_t npix = (size_t)a.npix;
#pragma unroll 4
    for (int b = b0; b < b1; b++) {
        const size_t i = (size_t)b * npix + p;
        const float* n = a.normal_new + i * 3;
        const double d = (lx * (double)n[0] + ly * (double)n[1]) + lz * (double)n[2];
        a.intensity[i] = (float)((double)a.abedo_new[i] * d);
    }
}

// q = sum over the faces [b0, b1) of (g_b a'_b) n'_b at pixel p, ascending b onto +0.0
__device__ __forceinline__ void sfs_sum_q(const SfsArgs& a, int b0, int b1, size_t p, double (&q)[3]) {
    const size_t npix = (size_t)a.npix;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
#pragma unroll 4
    for (int b = b0; b < b1; b++) {
        const size_t i = (size_t)b * npix + p;
        const float* n = a.normal_new + i * 3;
        const double ga = (double)a.g[i] * (double)a.abedo_new[i];
        q0 = q0 + ga * (double)n[0]; q1 = q1 + ga * (double)n[1]; q2 = q2 + ga * (double)n[2];
    }
    q[0] = q0; q[1] = q1; q[2] = q2;
}

// s = P q with P from the state planes 0-5 of pixel p
__device__ __forceinline__ void sfs_state_rows(const SfsArgs& a, size_t p, double q0, double q1, double q2, double& sx, double& sy,
                                               double& sz) {
    const size_t npix = (size_t)a.npix;
    const double* Pp = a.state + p;
    const double P[6] = {Pp[0], Pp[npix], Pp[2 * npix], Pp[3 * npix], Pp[4 * npix], Pp[5 * npix]};
    sfs_rows(P, q0, q1, q2, sx, sy, sz);
}

// the gradients of the faces [b0, b1) at pixel p: s = P q (read when a.gn), l from the state planes 6-8 (when a.gnn or a.gan)
__device__ __forceinline__ void sfs_write_grads(const SfsArgs& a, int b0, int b1, size_t p, double sx, double sy, double sz) {
    const size_t npix = (size_t)a.npix;
    double lx = 0.0, ly = 0.0, lz = 0.0;
    if (a.gnn || a.gan) {
        const double* l = a.state + 6 * npix + p;
        lx = l[0]; ly = l[npix]; lz = l[2 * npix];
    }
#pragma unroll 4
    for (int b = b0; b < b1; b++) {
        const size_t i = (size_t)b * npix + p;
        if (a.gn) {
            const double u = (double)a.im_gray[i] / ((double)a.abedo[i] + 1.0);
            float* o = a.gn + i * 3;
            o[0] = (float)(u * sx); o[1] = (float)(u * sy); o[2] = (float)(u * sz);
        }
        if (a.gnn) {
            const double ga = (double)a.g[i] * (double)a.abedo_new[i];
            float* o = a.gnn + i * 3;
            o[0] = (float)(ga * lx); o[1] = (float)(ga * ly); o[2] = (float)(ga * lz);
        }
        if (a.gan) {   // d intensity / d abedo_new: the forward's own d = l . n'
            const float* n = a.normal_new + i * 3;
            const double d = (lx * (double)n[0] + ly * (double)n[1]) + lz * (double)n[2];
            a.gan[i] = (float)((double)a.g[i] * d);
        }
    }
}

// ---- the one-call kernels ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_forward_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [9][S][64] partial sums, then [3][64] l
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int S = a.S, B = a.B;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < (size_t)a.npix;
    const int b0 = slice * a.chunk, b1 = min(B, b0 + a.chunk);
    double m[9];
    sfs_sum_moments(a, b0, active ? b1 : b0, p, m);
    double* lsh = sfs_lds + 9 * S * SFS_PX;
    sfs_meet_in_slice0<9>(sfs_lds, S, slice, lane, m);
    if (slice == 0) sfs_solve_pixel(a, m, p, active, lsh, lane);
    __syncthreads();
    if (active) sfs_shade(a, b0, b1, p, lsh[lane], lsh[SFS_PX + lane], lsh[2 * SFS_PX + lane]);
}

__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_backward_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [3][S][64] partial sums
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int S = a.S, B = a.B;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < (size_t)a.npix;
    const int b0 = slice * a.chunk, b1 = min(B, b0 + a.chunk);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (a.gn) {   // (uniform over the launch)
        double q3[3];
        sfs_sum_q(a, b0, active ? b1 : b0, p, q3);
        const int st = S * SFS_PX;
        double* mine = sfs_lds + slice * SFS_PX + lane;
        mine[0] = q3[0]; mine[st] = q3[1]; mine[2 * st] = q3[2];
        __syncthreads();
        // every wave forms the total in the same slice order: ((s0 + s1) + s2) + ...
        const double* q = sfs_lds + lane;
        double q0 = q[0], q1 = q[st], q2 = q[2 * st];
        for (int s = 1; s < S; s++) {
            q0 = q0 + q[s * SFS_PX]; q1 = q1 + q[st + s * SFS_PX]; q2 = q2 + q[2 * st + s * SFS_PX];
        }
        if (active) sfs_state_rows(a, p, q0, q1, q2, sx, sy, sz);
    }
    if (!active) return;
    sfs_write_grads(a, b0, b1, p, sx, sy, sz);
}

// ---- the split kernels ------------------------------------------------------------------------------------------------------------
// a.parts_out: [K][npix] planes of this call's sums (K = 9: the moments, K = 3: q); B == 0 writes +0.0 planes
__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_moments_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [9][S][64] partial sums
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t npix = (size_t)a.npix;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < npix;
    const int b0 = slice * a.chunk, b1 = min(a.B, b0 + a.chunk);
    double m[9];
    sfs_sum_moments(a, b0, active ? b1 : b0, p, m);
    sfs_meet_in_slice0<9>(sfs_lds, a.S, slice, lane, m);
    if (slice == 0 && active) {
#pragma unroll
        for (int k = 0; k < 9; k++) a.parts_out[(size_t)k * npix + p] = m[k];
    }
}

__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_backward_q_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [3][S][64] partial sums
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t npix = (size_t)a.npix;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < npix;
    const int b0 = slice * a.chunk, b1 = min(a.B, b0 + a.chunk);
    double q[3];
    sfs_sum_q(a, b0, active ? b1 : b0, p, q);
    sfs_meet_in_slice0<3>(sfs_lds, a.S, slice, lane, q);
    if (slice == 0 && active) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.parts_out[(size_t)k * npix + p] = q[k];
    }
}

// the totals of K planes over a.nparts parts ([nparts][K][npix]) at pixel p: ((part0 + part1) + part2) + ...
template <int K>
__device__ __forceinline__ void sfs_sum_parts(const SfsArgs& a, size_t p, double (&m)[K]) {
    const size_t npix = (size_t)a.npix;
    const double* q = a.parts_in + p;
#pragma unroll
    for (int k = 0; k < K; k++) m[k] = q[(size_t)k * npix];
    for (int r = 1; r < a.nparts; r++) {
        q += (size_t)K * npix;
#pragma unroll
        for (int k = 0; k < K; k++) m[k] = m[k] + q[(size_t)k * npix];
    }
}

__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_solve_shade_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [3][64] l
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < (size_t)a.npix;
    const int b0 = slice * a.chunk, b1 = min(a.B, b0 + a.chunk);
    if (slice == 0) {
        double m[9];
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = 0.0;   // (a lane past the image solves M = 0 and stores nothing)
        if (active) sfs_sum_parts<9>(a, p, m);
        sfs_solve_pixel(a, m, p, active, sfs_lds, lane);
    }
    __syncthreads();
    if (active) sfs_shade(a, b0, b1, p, sfs_lds[lane], sfs_lds[SFS_PX + lane], sfs_lds[2 * SFS_PX + lane]);
}

__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_backward_apply_kernel(SfsArgs a) {
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    if (!(p < (size_t)a.npix)) return;   // (no barrier in this kernel)
    const int b0 = slice * a.chunk, b1 = min(a.B, b0 + a.chunk);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (a.gn) {   // (uniform over the launch) every wave forms the total for itself, in part order
        double q[3];
        sfs_sum_parts<3>(a, p, q);
        sfs_state_rows(a, p, q[0], q[1], q[2], sx, sy, sz);
    }
    sfs_write_grads(a, b0, b1, p, sx, sy, sz);
}

// the solve half of sfs_solve_shade_kernel without the shade (opt-in; "per-face albedo fit": the fit needs l before abedo_new exists):
// one wave per 64 pixels adds the parts, solves and writes the state -- the same device functions, hence the same bits
__global__ __launch_bounds__(SFS_PX) void sfs_lighting_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [3][64] l (written by sfs_solve_pixel, not read here)
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < (size_t)a.npix;
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = 0.0;
    if (active) sfs_sum_parts<9>(a, p, m);
    sfs_solve_pixel(a, m, p, active, sfs_lds, lane);
}

}  // namespace fr

// The launch geometry, chosen in ONE place: the launchers and the test hook both read it from here.
namespace {
struct SfsGeom {
    int px, slices, chunk, blocks;
    size_t lds_fwd, lds_bwd;
    size_t lds_moments, lds_solve, lds_q;   // the split kernels (the apply kernel uses no LDS)
};
SfsGeom sfs_geom(int B, long long npix) {
    using namespace fr;
    SfsGeom g{};
    g.px = SFS_PX;
    g.slices = sfs_slices(B);
    g.chunk = sfs_chunk(B, g.slices);
    g.blocks = (int)((npix + SFS_PX - 1) / SFS_PX);
    g.lds_fwd = (size_t)(9 * g.slices + 3) * SFS_PX * sizeof(double);
    g.lds_bwd = (size_t)(3 * g.slices) * SFS_PX * sizeof(double);
    g.lds_moments = (size_t)(9 * g.slices) * SFS_PX * sizeof(double);
    g.lds_solve = (size_t)3 * SFS_PX * sizeof(double);
    g.lds_q = g.lds_bwd;
    return g;
}
bool sfs_shape_empty(int B, int H, int W) { return B == 0 || H == 0 || W == 0; }
constexpr int SFS_PARTS_MAX = 4096;
bool sfs_rcond_ok(double rcond) { return rcond >= 0.0 && std::isfinite(rcond); }

// What the launching entry points share, in the order all of them answer: a negative size or a bad scalar (FR_ERR_INVALID_ARG),
// an empty shape (FR_OK, nothing launched), the entry point's OWN verdict on its pointers and buffers, an image beyond one
// grid (FR_ERR_UNSUPPORTED); then the geometry, the geometry fields of `a`, and the launch.  `a` arrives with the entry point's
// own fields set; lds = the kernel's dynamic LDS size in SfsGeom (null: none).
template <typename Kernel>
int sfs_launch(Kernel kernel, size_t SfsGeom::*lds, fr::SfsArgs& a, int B, int H, int W, bool scalars_ok, bool empty, int own,
               void* hip_stream) {
    if (B < 0 || H < 0 || W < 0 || !scalars_ok) return FR_ERR_INVALID_ARG;
    if (empty) return FR_OK;
    if (own != FR_OK) return own;
    const long long npix = (long long)H * W;
    if (npix > 0x7FFFFFFFll - fr::SFS_PX) return FR_ERR_UNSUPPORTED;
    const SfsGeom geo = sfs_geom(B, npix);
    a.B = B; a.npix = (int)npix; a.S = geo.slices; a.chunk = geo.chunk;
    hipLaunchKernelGGL(kernel, dim3((unsigned)geo.blocks), dim3(fr::SFS_PX * geo.slices), lds ? geo.*lds : 0,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
// an entry point's own verdict: its pointers, then its buffer
int sfs_own(bool pointers_ok, bool buffer_ok) {
    return !pointers_ok ? FR_ERR_INVALID_ARG : !buffer_ok ? FR_ERR_WORKSPACE : FR_OK;
}
}  // namespace

extern "C" {

size_t fr_sfs_state_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)10 * (size_t)H * (size_t)W * sizeof(double);
}

// test hook: out = {pixels per workgroup, batch slices per pixel, workgroups, dynamic LDS bytes of the forward}; zeros for an
// empty shape or one the launchers refuse
void fr_debug_sfs_geom(int B, int H, int W, int* out) {
    for (int i = 0; i < 4; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll) return;
    const SfsGeom g = sfs_geom(B, npix);
    out[0] = g.px; out[1] = g.slices; out[2] = g.blocks; out[3] = (int)g.lds_fwd;
}

// HOST instantiation of the kernel's solver (no GPU): m6, p6 = xx, xy, xz, yy, yz, zz
int fr_debug_sfs_pinv(const double* m6, double rcond, double* p6, int* rank) {
    if (!m6 || !p6 || !rank || !sfs_rcond_ok(rcond)) return FR_ERR_INVALID_ARG;
    fr_sfs_pinv3(m6, rcond, p6, rank);
    return FR_OK;
}

int fr_sfs_intensity_forward(const float* abedo, const float* normal, const float* im_gray, const float* abedo_new,
                             const float* normal_new, int B, int H, int W, double rcond, float* intensity, void* state,
                             size_t state_bytes, void* hip_stream) {
    fr::SfsArgs a{};
    a.abedo = abedo; a.normal = normal; a.im_gray = im_gray; a.abedo_new = abedo_new; a.normal_new = normal_new;
    a.intensity = intensity; a.state = reinterpret_cast<double*>(state); a.rcond = rcond;
    const int own = sfs_own(abedo && normal && im_gray && abedo_new && normal_new && intensity,
                            ws_ok(state, state_bytes, fr_sfs_state_bytes(H, W), 16));
    return sfs_launch(fr::sfs_forward_kernel, &SfsGeom::lds_fwd, a, B, H, W, sfs_rcond_ok(rcond), sfs_shape_empty(B, H, W), own,
                      hip_stream);
}

int fr_sfs_intensity_backward_tex(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                                  const float* normal_new, const void* state, size_t state_bytes, int B, int H, int W,
                                  float* grad_normal, float* grad_normal_new, float* grad_abedo_new, void* hip_stream) {
    fr::SfsArgs a{};
    a.g = grad_intensity; a.abedo = abedo; a.im_gray = im_gray; a.abedo_new = abedo_new; a.normal_new = normal_new;
    a.gn = grad_normal; a.gnn = grad_normal_new; a.gan = grad_abedo_new;
    a.state = const_cast<double*>(reinterpret_cast<const double*>(state));
    const int own = sfs_own((grad_normal || grad_normal_new || grad_abedo_new) && grad_intensity && abedo && im_gray && abedo_new &&
                                normal_new,
                            ws_ok(state, state_bytes, fr_sfs_state_bytes(H, W), 16));
    return sfs_launch(fr::sfs_backward_kernel, &SfsGeom::lds_bwd, a, B, H, W, true, sfs_shape_empty(B, H, W), own, hip_stream);
}

int fr_sfs_intensity_backward(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                              const float* normal_new, const void* state, size_t state_bytes, int B, int H, int W,
                              float* grad_normal, float* grad_normal_new, void* hip_stream) {
    return fr_sfs_intensity_backward_tex(grad_intensity, abedo, im_gray, abedo_new, normal_new, state, state_bytes, B, H, W,
                                         grad_normal, grad_normal_new, nullptr, hip_stream);
}

// ---- the split route: the same two passes cut where the batch couples (include/fr_hotpath.h, "... across ranks") ----------------

size_t fr_sfs_moments_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)9 * (size_t)H * (size_t)W * sizeof(double);
}

size_t fr_sfs_q_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)3 * (size_t)H * (size_t)W * sizeof(double);
}

// test hook: out = {pixels per workgroup, batch slices per pixel, workgroups, dynamic LDS bytes of the moments kernel, of the
// solve-and-shade kernel, of the q kernel}; zeros for an empty image or a shape the launchers refuse.  B == 0 is a launch here.
void fr_debug_sfs_split_geom(int B, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B < 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll - fr::SFS_PX) return;
    const SfsGeom g = sfs_geom(B, npix);
    out[0] = g.px; out[1] = g.slices; out[2] = g.blocks; out[3] = (int)g.lds_moments; out[4] = (int)g.lds_solve;
    out[5] = (int)g.lds_q;
}

int fr_sfs_moments(const float* abedo, const float* normal, const float* im_gray, int B, int H, int W, void* moments,
                   size_t moments_bytes, void* hip_stream) {
    fr::SfsArgs a{};
    a.abedo = abedo; a.normal = normal; a.im_gray = im_gray; a.parts_out = reinterpret_cast<double*>(moments);
    const int own = sfs_own(B <= 0 || (abedo && normal && im_gray), ws_ok(moments, moments_bytes, fr_sfs_moments_bytes(H, W), 16));
    return sfs_launch(fr::sfs_moments_kernel, &SfsGeom::lds_moments, a, B, H, W, true, H == 0 || W == 0, own, hip_stream);
}

int fr_sfs_solve_shade(const void* moment_parts, int nparts, const float* abedo_new, const float* normal_new, int B, int H, int W,
                       double rcond, float* intensity, void* state, size_t state_bytes, void* hip_stream) {
    fr::SfsArgs a{};
    a.parts_in = reinterpret_cast<const double*>(moment_parts); a.nparts = nparts;
    a.abedo_new = abedo_new; a.normal_new = normal_new;
    a.intensity = intensity; a.state = reinterpret_cast<double*>(state); a.rcond = rcond;
    const int own = sfs_own(moment_parts && abedo_new && normal_new && intensity,
                            ws_ok(state, state_bytes, fr_sfs_state_bytes(H, W), 16));
    return sfs_launch(fr::sfs_solve_shade_kernel, &SfsGeom::lds_solve, a, B, H, W,
                      sfs_rcond_ok(rcond) && nparts >= 1 && nparts <= SFS_PARTS_MAX, sfs_shape_empty(B, H, W), own, hip_stream);
}

int fr_sfs_backward_q(const float* grad_intensity, const float* abedo_new, const float* normal_new, int B, int H, int W, void* q,
                      size_t q_bytes, void* hip_stream) {
    fr::SfsArgs a{};
    a.g = grad_intensity; a.abedo_new = abedo_new; a.normal_new = normal_new; a.parts_out = reinterpret_cast<double*>(q);
    const int own = sfs_own(B <= 0 || (grad_intensity && abedo_new && normal_new), ws_ok(q, q_bytes, fr_sfs_q_bytes(H, W), 16));
    return sfs_launch(fr::sfs_backward_q_kernel, &SfsGeom::lds_q, a, B, H, W, true, H == 0 || W == 0, own, hip_stream);
}

int fr_sfs_backward_apply(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                          const float* normal_new, const void* state, size_t state_bytes, const void* q_parts, int nparts, int B,
                          int H, int W, float* grad_normal, float* grad_normal_new, float* grad_abedo_new, void* hip_stream) {
    fr::SfsArgs a{};
    a.g = grad_intensity; a.abedo = abedo; a.im_gray = im_gray; a.abedo_new = abedo_new; a.normal_new = normal_new;
    a.gn = grad_normal; a.gnn = grad_normal_new; a.gan = grad_abedo_new;
    a.state = const_cast<double*>(reinterpret_cast<const double*>(state));
    a.parts_in = reinterpret_cast<const double*>(q_parts); a.nparts = nparts;
    const int own = sfs_own((grad_normal || grad_normal_new || grad_abedo_new) && grad_intensity && abedo && im_gray && abedo_new &&
                                normal_new && (!grad_normal || q_parts),
                            ws_ok(state, state_bytes, fr_sfs_state_bytes(H, W), 16));
    return sfs_launch(fr::sfs_backward_apply_kernel, nullptr, a, B, H, W, nparts >= 1 && nparts <= SFS_PARTS_MAX,
                      sfs_shape_empty(B, H, W), own, hip_stream);
}

// the lighting alone: B = 1 stands for "one wave per workgroup" in the shared launcher (the kernel reads no face)
int fr_sfs_lighting(const void* moment_parts, int nparts, int H, int W, double rcond, void* state, size_t state_bytes, void* stream) {
    fr::SfsArgs a{};
    a.parts_in = reinterpret_cast<const double*>(moment_parts); a.nparts = nparts;
    a.state = reinterpret_cast<double*>(state); a.rcond = rcond;
    const int own = sfs_own(moment_parts != nullptr, ws_ok(state, state_bytes, fr_sfs_state_bytes(H, W), 16));
    return sfs_launch(fr::sfs_lighting_kernel, &SfsGeom::lds_solve, a, 1, H, W,
                      sfs_rcond_ok(rcond) && nparts >= 1 && nparts <= SFS_PARTS_MAX, H == 0 || W == 0, own, stream);
}

}  // extern "C"
