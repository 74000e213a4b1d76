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
// No atomics; the association of every sum is a function of B alone (sfs_slices / sfs_chunk below).
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
    double rcond;
    int B, npix, S, chunk;
};

__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_forward_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [9][S][64] partial sums, then [3][64] l
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int S = a.S, B = a.B;
    const size_t npix = (size_t)a.npix;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < npix;
    const int b0 = slice * a.chunk, b1 = min(B, b0 + a.chunk);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    if (active) {
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
    }
    double* part = sfs_lds;
    double* lsh = sfs_lds + 9 * S * SFS_PX;
    if (slice > 0) {
        double* q = part + slice * SFS_PX + lane;
        const int st = S * SFS_PX;
        q[0] = m0; q[st] = m1; q[2 * st] = m2; q[3 * st] = m3; q[4 * st] = m4; q[5 * st] = m5;
        q[6 * st] = r0; q[7 * st] = r1; q[8 * st] = r2;
    }
    __syncthreads();
    if (slice == 0) {
        const int st = S * SFS_PX;
        for (int s = 1; s < S; s++) {   // slice order: ((s0 + s1) + s2) + ...
            const double* q = part + s * SFS_PX + lane;
            m0 = m0 + q[0]; m1 = m1 + q[st]; m2 = m2 + q[2 * st]; m3 = m3 + q[3 * st]; m4 = m4 + q[4 * st]; m5 = m5 + q[5 * st];
            r0 = r0 + q[6 * st]; r1 = r1 + q[7 * st]; r2 = r2 + q[8 * st];
        }
        const double m6[6] = {m0, m1, m2, m3, m4, m5};
        double P[6];
        int rank;
        fr_sfs_pinv3(m6, a.rcond, P, &rank);
        double lx = (P[0] * r0 + P[1] * r1) + P[2] * r2;
        double ly = (P[1] * r0 + P[3] * r1) + P[4] * r2;
        double lz = (P[2] * r0 + P[4] * r1) + P[5] * r2;
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
    __syncthreads();
    if (active) {
        const double lx = lsh[lane], ly = lsh[SFS_PX + lane], lz = lsh[2 * SFS_PX + lane];
#pragma unroll 4
        for (int b = b0; b < b1; b++) {
            const size_t i = (size_t)b * npix + p;
            const float* n = a.normal_new + i * 3;
            const double d = (lx * (double)n[0] + ly * (double)n[1]) + lz * (double)n[2];
            a.intensity[i] = (float)((double)a.abedo_new[i] * d);
        }
    }
}

__global__ __launch_bounds__(SFS_PX* FR_SFS_SLICES_MAX) void sfs_backward_kernel(SfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfs_lds[];   // [3][S][64] partial sums
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int S = a.S, B = a.B;
    const size_t npix = (size_t)a.npix;
    const size_t p = (size_t)blockIdx.x * SFS_PX + lane;
    const bool active = p < npix;
    const int b0 = slice * a.chunk, b1 = min(B, b0 + a.chunk);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (a.gn) {   // (uniform over the launch)
        double q0 = 0.0, q1 = 0.0, q2 = 0.0;
        if (active) {
#pragma unroll 4
            for (int b = b0; b < b1; b++) {
                const size_t i = (size_t)b * npix + p;
                const float* n = a.normal_new + i * 3;
                const double ga = (double)a.g[i] * (double)a.abedo_new[i];
                q0 = q0 + ga * (double)n[0]; q1 = q1 + ga * (double)n[1]; q2 = q2 + ga * (double)n[2];
            }
        }
        const int st = S * SFS_PX;
        double* mine = sfs_lds + slice * SFS_PX + lane;
        mine[0] = q0; mine[st] = q1; mine[2 * st] = q2;
        __syncthreads();
        // every wave forms the total in the same slice order: ((s0 + s1) + s2) + ...
        const double* q = sfs_lds + lane;
        q0 = q[0]; q1 = q[st]; q2 = q[2 * st];
        for (int s = 1; s < S; s++) {
            q0 = q0 + q[s * SFS_PX]; q1 = q1 + q[st + s * SFS_PX]; q2 = q2 + q[2 * st + s * SFS_PX];
        }
        if (active) {
            const double* P = a.state + p;
            const double Pxx = P[0], Pxy = P[npix], Pxz = P[2 * npix], Pyy = P[3 * npix], Pyz = P[4 * npix], Pzz = P[5 * npix];
            sx = (Pxx * q0 + Pxy * q1) + Pxz * q2;
            sy = (Pxy * q0 + Pyy * q1) + Pyz * q2;
            sz = (Pxz * q0 + Pyz * q1) + Pzz * q2;
        }
    }
    if (!active) return;
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

}  // namespace fr

// The launch geometry, chosen in ONE place: the launchers and the test hook both read it from here.
namespace {
struct SfsGeom {
    int px, slices, chunk, blocks;
    size_t lds_fwd, lds_bwd;
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
    return g;
}
bool sfs_shape_empty(int B, int H, int W) { return B == 0 || H == 0 || W == 0; }
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
    if (!m6 || !p6 || !rank || !(rcond >= 0.0) || !std::isfinite(rcond)) return FR_ERR_INVALID_ARG;
    fr_sfs_pinv3(m6, rcond, p6, rank);
    return FR_OK;
}

int fr_sfs_intensity_forward(const float* abedo, const float* normal, const float* im_gray, const float* abedo_new,
                             const float* normal_new, int B, int H, int W, double rcond, float* intensity, void* state,
                             size_t state_bytes, void* hip_stream) {
    using namespace fr;
    if (B < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (!(rcond >= 0.0) || !std::isfinite(rcond)) return FR_ERR_INVALID_ARG;
    if (sfs_shape_empty(B, H, W)) return FR_OK;
    if (!abedo || !normal || !im_gray || !abedo_new || !normal_new || !intensity) return FR_ERR_INVALID_ARG;
    if (!state || ((uintptr_t)state & 15) || state_bytes < fr_sfs_state_bytes(H, W)) return FR_ERR_WORKSPACE;
    const long long npix = (long long)H * W;
    if (npix > 0x7FFFFFFFll - SFS_PX) return FR_ERR_UNSUPPORTED;
    const SfsGeom geo = sfs_geom(B, npix);
    SfsArgs a{};
    a.abedo = abedo; a.normal = normal; a.im_gray = im_gray; a.abedo_new = abedo_new; a.normal_new = normal_new;
    a.intensity = intensity; a.state = reinterpret_cast<double*>(state); a.rcond = rcond;
    a.B = B; a.npix = (int)npix; a.S = geo.slices; a.chunk = geo.chunk;
    hipLaunchKernelGGL(sfs_forward_kernel, dim3((unsigned)geo.blocks), dim3(SFS_PX * geo.slices), geo.lds_fwd,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_sfs_intensity_backward_tex(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                                  const float* normal_new, const void* state, size_t state_bytes, int B, int H, int W,
                                  float* grad_normal, float* grad_normal_new, float* grad_abedo_new, void* hip_stream) {
    using namespace fr;
    if (B < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (sfs_shape_empty(B, H, W)) return FR_OK;
    if (!grad_normal && !grad_normal_new && !grad_abedo_new) return FR_ERR_INVALID_ARG;
    if (!grad_intensity || !abedo || !im_gray || !abedo_new || !normal_new) return FR_ERR_INVALID_ARG;
    if (!state || ((uintptr_t)state & 15) || state_bytes < fr_sfs_state_bytes(H, W)) return FR_ERR_WORKSPACE;
    const long long npix = (long long)H * W;
    if (npix > 0x7FFFFFFFll - SFS_PX) return FR_ERR_UNSUPPORTED;
    const SfsGeom geo = sfs_geom(B, npix);
    SfsArgs a{};
    a.g = grad_intensity; a.abedo = abedo; a.im_gray = im_gray; a.abedo_new = abedo_new; a.normal_new = normal_new;
    a.gn = grad_normal; a.gnn = grad_normal_new; a.gan = grad_abedo_new;
    a.state = const_cast<double*>(reinterpret_cast<const double*>(state));
    a.B = B; a.npix = (int)npix; a.S = geo.slices; a.chunk = geo.chunk;
    hipLaunchKernelGGL(sfs_backward_kernel, dim3((unsigned)geo.blocks), dim3(SFS_PX * geo.slices), geo.lds_bwd,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_sfs_intensity_backward(const float* grad_intensity, const float* abedo, const float* im_gray, const float* abedo_new,
                              const float* normal_new, const void* state, size_t state_bytes, int B, int H, int W,
                              float* grad_normal, float* grad_normal_new, void* hip_stream) {
    return fr_sfs_intensity_backward_tex(grad_intensity, abedo, im_gray, abedo_new, normal_new, state, state_bytes, B, H, W,
                                         grad_normal, grad_normal_new, nullptr, hip_stream);
}

}  // extern "C"
