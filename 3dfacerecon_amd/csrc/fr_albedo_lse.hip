// Per-face albedo fit (opt-in; include/fr_hotpath.h, "per-face albedo fit"): the least-squares estimate of the albedo coefficients
// the reference's shape-from-shading block wanted and gave up (nets/network.py:436-455), on the pixel grid: the rasteriser's tri_ind
// is the map from a pixel to its row of the texture basis.
//
//   albedo_basis_kernel          load time.  One thread per (triangle, coefficient): Phi[t][k], the texture basis seen through the
//                                rasteriser's lookup -- nine widened fp32 terms in a fixed order, divided by 9.0.
//   albedo_lse_tile_kernel       per step.  A face's pixels in row-major order are cut into tiles of AL_TILE = 256 -- a compile-time
//                                constant -- and ONE WAVE OWNS A TILE (a workgroup holds AL_WAVES = 4 consecutive tiles; its waves share
//                                nothing: no LDS, no barrier).  The wave takes 64 pixels at a time: lane l reads pixel l's tri_ind,
//                                a, I, n' and l once (coalesced) and forms d and rho; then for each of the 16 groups of four pixels the
//                                lanes fetch d, rho and t of pixel 4 g + (lane >> 4) by lane shuffles, lane k = lane & 15 forms
//                                x_k (k < K: one gather of Phi[t][k], 8 K contiguous bytes per pixel; k = K: rho; else +0) and ONE
//                                v_mfma_f64_16x16x4_f64 with the SAME register as both operands adds x x^T of the four pixels onto the
//                                wave's 16 x 16 sum: four float64 per lane, no cross-lane reduction.  The accumulators go to the
//                                workspace as they lie in the registers, partial[face][tile][register][lane]; the tile's counted
//                                pixels (a wave ballot) beside them.
//   albedo_lse_finish_kernel     one workgroup of 256 threads per face: thread (i, j), i <= j, adds the tile partials in ascending tile
//                                order from +0.0 and writes the value to (i, j) and (j, i) of `moments`; then ONE WAVE solves the face
//                                in float64 (Cholesky by columns: lane r holds row r in registers, the rows meet by lane shuffles; every
//                                element's chain is the header's sequential source order) and writes alpha and stats.
// Plain float64 VALU under -ffp-contract=off outside the matrix instruction; ordinary vector stores; no atomics.
#include "fr_common.h"

#include <cmath>

namespace fr {

constexpr int AL_TILE = 256;                      // pixels per tile: one wave's chain of 64 matrix instructions
constexpr int AL_WAVES = 4, AL_THREADS = 64 * AL_WAVES;   // tiles per workgroup of the tile kernel
constexpr int AL_KMAX = 15;                       // coefficients served: x has 16 slots, slot K holds rho
constexpr int AL_FIN = 256;                       // threads of the finish workgroup: one per element of M

typedef double al_f64x4 __attribute__((ext_vector_type(4)));

struct AlArgs {
    const double* basis;       // [ntri][K]
    const float* tri_ind;      // [B,npix]
    const double* lighting;    // [3][npix]
    const float* normal_new;   // [B,npix,3]
    const float* abedo;        // [B,npix]
    const float* im_gray;      // [B,npix]
    double* partial;           // [B][tiles][4][64]
    double* counts;            // [B][tiles]
    float* alpha;              // [B][K]
    double* moments;           // [B][16][16]
    double* stats;             // [B][4]
    double ridge;
    int ntri, K, npix, tiles, wgpf;
};

__global__ __launch_bounds__(256) void albedo_basis_kernel(const float* tri, const float* pc_tex, int nver, int ntri, int K,
                                                           double* basis) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)ntri * K) return;
    const int t = (int)(idx / K), k = (int)(idx - (long long)t * K);
    const int v[3] = {f2i_x86(tri[t]), f2i_x86(tri[(size_t)ntri + t]), f2i_x86(tri[2 * (size_t)ntri + t])};
    double s = 0.0;   // a triangle with a vertex id outside [0, nver): a row of +0.0
    if (v[0] >= 0 && v[0] < nver && v[1] >= 0 && v[1] < nver && v[2] >= 0 && v[2] < nver) {
        // channel-major, then vertex 1, 2, 3, onto the first term
        s = (double)pc_tex[(size_t)v[0] * K + k];
#pragma unroll
        for (int c = 0; c < 3; c++) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (c == 0 && j == 0) continue;
                s = s + (double)pc_tex[((size_t)c * nver + v[j]) * K + k];
            }
        }
        s = s / 9.0;
    }
    basis[idx] = s;
}

__global__ __launch_bounds__(AL_THREADS) void albedo_lse_tile_kernel(AlArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int face = blockIdx.x / a.wgpf;
    const int tile = (blockIdx.x - face * a.wgpf) * AL_WAVES + wave;
    if (tile >= a.tiles) return;   // (a whole wave: the waves of a workgroup share nothing)
    const size_t npix = (size_t)a.npix;
    const size_t fo = (size_t)face * npix;
    const int k = lane & 15, sub = lane >> 4;
    al_f64x4 acc = al_f64x4{0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < AL_TILE / 64; s++) {   // (unrolled, and every map read unconditionally at a clamped pixel: the loads of the
                                               // four batches carry no dependence on each other or on tri_ind and go out together)
        const size_t base = (size_t)tile * AL_TILE + (size_t)s * 64;
        if (base >= npix) continue;   // (sixteen groups of +0.0 would leave every accumulator's bits as they are)
        const bool in = base + lane < npix;
        const size_t p = in ? base + lane : npix - 1;
        const int ti = f2i_x86(a.tri_ind[fo + p]);
        const float* n = a.normal_new + (fo + p) * 3;
        const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
        const double lx = a.lighting[p], ly = a.lighting[npix + p], lz = a.lighting[2 * npix + p];
        const double I = (double)a.im_gray[fo + p], al = (double)a.abedo[fo + p];
        const bool counted = in && ti >= 0 && ti < a.ntri;
        const int t = counted ? ti : -1;
        const double d = (lx * nx + ly * ny) + lz * nz;
        const double rho = I - al * d;   // (an uncounted pixel's d and rho are never used: x is selected, not multiplied, to +0.0)
        cnt += __builtin_popcountll(__ballot(counted));
#pragma unroll
        for (int g = 0; g < 16; g++) {   // (unrolled: the sixteen gathers of a batch are in flight together)
            const int src = 4 * g + sub;
            const double dd = __shfl(d, src, 64), rr = __shfl(rho, src, 64);
            const int tt = __shfl(t, src, 64);
            double x = 0.0;
            if (tt >= 0) {
                if (k < a.K) x = dd * a.basis[(size_t)tt * a.K + k];
                else if (k == a.K) x = rr;
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
        }
    }
    const size_t rec = (size_t)face * a.tiles + tile;
    double* o = a.partial + rec * 256 + lane;
    o[0] = acc[0]; o[64] = acc[1]; o[128] = acc[2]; o[192] = acc[3];
    if (lane == 0) a.counts[rec] = (double)cnt;
}

// The f64 16x16x4 result layout (csrc/fr_geometry.hip): register g of lane l holds element (row = (l >> 4) + 4 g, column = l & 15), so a
// tile's record [register][lane] IS the 16 x 16 matrix in row-major order.
__global__ __launch_bounds__(AL_FIN) void albedo_lse_finish_kernel(AlArgs a) {
    __shared__ double M[16][16];
    const int e = threadIdx.x, i = e >> 4, j = e & 15;
    const int face = blockIdx.x, K = a.K;
    __shared__ double count_sh;
    if (i <= j) {
        // sixteen loads in flight per thread: the additions stay one chain in ascending tile order
        const double* src = a.partial + (size_t)face * a.tiles * 256 + i * 16 + j;
        double sum = 0.0;
        int t = 0;
        for (; t + 16 <= a.tiles; t += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = src[(size_t)(t + u) * 256];
#pragma unroll
            for (int u = 0; u < 16; u++) sum = sum + v[u];
        }
        for (; t < a.tiles; t++) sum = sum + src[(size_t)t * 256];
        M[i][j] = sum; M[j][i] = sum;
        double* mo = a.moments + (size_t)face * 256;
        mo[i * 16 + j] = sum; mo[j * 16 + i] = sum;
    } else if (e == 16) {   // an idle thread of the lower triangle counts meanwhile (integers: exact in any order; kept a chain)
        const double* src = a.counts + (size_t)face * a.tiles;
        double count = 0.0;
        int t = 0;
        for (; t + 16 <= a.tiles; t += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = src[t + u];
#pragma unroll
            for (int u = 0; u < 16; u++) count = count + v[u];
        }
        for (; t < a.tiles; t++) count = count + src[t];
        count_sh = count;
    }
    __syncthreads();
    if (e >= 64) return;

    // ---- the solve: one wave, float64.  Lane r (= lane & 15; the four quarters of the wave run the same thing) holds row r of G' and
    // of L in registers and meets the other rows through lane shuffles, so the elements of a column are formed side by side -- but
    // every element's own chain of products and sums is the one of the sequential source order in the header, so are its bits.
    const int r = j;
    const double count = count_sh;
    const double E0 = M[K][K];
    bool bad = false;   // a non-finite moment in rows and columns 0 .. K: lane e looks at elements e, e + 64, e + 128, e + 192
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int idx = e + 64 * u;
        bad = bad || ((idx >> 4) <= K && (idx & 15) <= K && !__builtin_isfinite(M[idx >> 4][idx & 15]));
    }
    bool ok = count > 0.0 && __ballot(bad) == 0;
    double tr = 0.0;
    for (int c = 0; c < K; c++) tr = tr + M[c][c];
    const double lam = (a.ridge * tr) / (double)K;
    const double tiny = 9.094947017729282379150390625e-13;   // 2^-40
    double grow[AL_KMAX], Lrow[AL_KMAX], al[AL_KMAX];
#pragma unroll
    for (int m = 0; m < AL_KMAX; m++) {
        grow[m] = M[r][m];
        Lrow[m] = 0.0;
        al[m] = 0.0;
    }
    const double rhs = M[r][K];
    // Cholesky of G' = G + lam I by columns, inner sums ascending from +0.0; Lrow[c] is meaningful on the lanes r >= c alone
#pragma unroll
    for (int c = 0; c < AL_KMAX; c++) {
        if (c < K && ok) {   // (the same on every lane)
            double q = 0.0;
#pragma unroll
            for (int m = 0; m < c; m++) q = q + Lrow[m] * __shfl(Lrow[m], c, 64);
            const double gcc = M[c][c] + lam;
            const double piv = gcc - __shfl(q, c, 64);
            if (!(__builtin_isfinite(piv) && piv > tiny * gcc)) {
                ok = false;
            } else {
                const double root = __builtin_sqrt(piv);
                Lrow[c] = r == c ? root : (grow[c] - q) / root;
            }
        }
    }
    if (ok) {
        double qy = 0.0, y = 0.0;   // L y = r: lane m closes y_m, the lanes below it take it into their chains
#pragma unroll
        for (int m = 0; m < AL_KMAX; m++) {
            if (m < K) {
                const double ym = __shfl((rhs - qy) / Lrow[m], m, 64);
                if (r == m) y = ym;
                if (r > m) qy = qy + Lrow[m] * ym;
            }
        }
#pragma unroll
        for (int p = AL_KMAX - 1; p >= 0; p--) {   // L^T alpha = y: every lane forms alpha_p, inner sum ascending in m
            if (p < K) {
                double q = 0.0;
#pragma unroll
                for (int m = p + 1; m < AL_KMAX; m++) {
                    const double lmp = __shfl(Lrow[p], m, 64);   // L[m][p] lives on lane m
                    if (m < K) q = q + lmp * al[m];
                }
                al[p] = (__shfl(y, p, 64) - q) / __shfl(Lrow[p], p, 64);
            }
        }
#pragma unroll
        for (int p = 0; p < AL_KMAX; p++)
            if (p < K) ok = ok && __builtin_isfinite(al[p]);
    }
    double E1 = E0;   // a failed face: alpha = 0, the mean albedo
    if (ok) {
#pragma unroll
        for (int p = 0; p < AL_KMAX; p++) al[p] = (double)(float)al[p];   // E1 is taken at the alpha the caller receives
        double ga = 0.0;   // (G alpha)_r on lane r
#pragma unroll
        for (int c = 0; c < AL_KMAX; c++)
            if (c < K) ga = ga + grow[c] * al[c];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int p = 0; p < AL_KMAX; p++)
            if (p < K) s1 = s1 + al[p] * M[p][K];
#pragma unroll
        for (int p = 0; p < AL_KMAX; p++) {
            const double gap = __shfl(ga, p, 64);
            if (p < K) s2 = s2 + al[p] * gap;
        }
        E1 = (E0 - 2.0 * s1) + s2;
    }
    if (e != 0) return;
    float* ao = a.alpha + (size_t)face * K;
#pragma unroll
    for (int p = 0; p < AL_KMAX; p++)
        if (p < K) ao[p] = ok ? (float)al[p] : 0.0f;
    double* so = a.stats + (size_t)face * 4;
    so[0] = count; so[1] = E0; so[2] = E1; so[3] = ok ? 1.0 : 0.0;
}

}  // namespace fr

// The sizes and the launch geometry, stated in ONE place: the size functions, the launchers and the test hook read them from here.
namespace {
struct AlGeom {
    int tiles;              // per face
    int wgpf;               // tile-kernel workgroups per face
    long long blocks;       // of the tile kernel
};
AlGeom al_geom(int B, long long npix) {
    AlGeom g;
    g.tiles = (int)((npix + fr::AL_TILE - 1) / fr::AL_TILE);
    g.wgpf = (g.tiles + fr::AL_WAVES - 1) / fr::AL_WAVES;
    g.blocks = (long long)g.wgpf * B;
    return g;
}
constexpr size_t AL_LDS_FIN = (size_t)257 * sizeof(double);
bool al_k_served(int K) { return K >= 1 && K <= fr::AL_KMAX; }
// more than 2^31 - 65 pixels per face, or more workgroups than one grid takes
bool al_size_ok(int B, int H, int W) {
    const long long npix = (long long)H * W;
    return npix <= 0x7FFFFFFFll - 64 && al_geom(B, npix).blocks <= 0x7FFFFFFFll;
}
// workspace: the tile partials [B][tiles][4][64], then the tile counts [B][tiles]; float64
size_t al_workspace_bytes(int B, int H, int W) {
    const AlGeom g = al_geom(B, (long long)H * W);
    return (size_t)B * g.tiles * 257 * sizeof(double);
}
}  // namespace

extern "C" {

size_t fr_albedo_basis_bytes(int ntri, int K) {
    if (ntri <= 0 || !al_k_served(K)) return 0;
    return (size_t)ntri * K * sizeof(double);
}

int fr_albedo_basis_build(const float* tri, const float* pc_tex, int nver, int ntri, int K, void* basis, size_t basis_bytes,
                          void* stream) {
    if (nver < 0 || ntri < 0) return FR_ERR_INVALID_ARG;
    if (!al_k_served(K)) return FR_ERR_UNSUPPORTED;
    if (ntri == 0) return FR_OK;
    if (!tri || (nver > 0 && !pc_tex)) return FR_ERR_INVALID_ARG;
    if (!ws_ok(basis, basis_bytes, fr_albedo_basis_bytes(ntri, K), 16)) return FR_ERR_WORKSPACE;
    if (ntri > (1 << 24)) return FR_ERR_UNSUPPORTED;   // float-stored ids
    const long long n = (long long)ntri * K;
    hipLaunchKernelGGL(fr::albedo_basis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tri, pc_tex,
                       nver, ntri, K, (double*)basis);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

size_t fr_albedo_lse_workspace_bytes(int B, int H, int W, int K) {
    if (B <= 0 || H <= 0 || W <= 0 || !al_k_served(K) || !al_size_ok(B, H, W)) return 0;
    return al_workspace_bytes(B, H, W);
}

// test hook: out = {pixels per tile, tiles per face, workgroups of the tile kernel, workgroups of the finish kernel, static LDS bytes of
// a finish workgroup}; zeros for an empty shape or one the launcher refuses
void fr_debug_albedo_lse_geom(int B, int H, int W, int K, int* out) {
    for (int i = 0; i < 5; i++) out[i] = 0;
    if (B <= 0 || H <= 0 || W <= 0 || !al_k_served(K) || !al_size_ok(B, H, W)) return;
    const AlGeom g = al_geom(B, (long long)H * W);
    out[0] = fr::AL_TILE; out[1] = g.tiles; out[2] = (int)g.blocks; out[3] = B; out[4] = (int)AL_LDS_FIN;
}

int fr_albedo_lse_forward(const void* basis, const float* tri_ind, const void* lighting, const float* normal_new, const float* abedo,
                          const float* im_gray, int B, int ntri, int H, int W, int K, double ridge, float* alpha, void* moments,
                          void* stats, void* workspace, size_t ws_bytes, void* stream) {
    if (B < 0 || ntri < 0 || H < 0 || W < 0 || !(ridge >= 0.0 && std::isfinite(ridge))) return FR_ERR_INVALID_ARG;
    if (!al_k_served(K)) return FR_ERR_UNSUPPORTED;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!basis || !tri_ind || !lighting || !normal_new || !abedo || !im_gray || !alpha || !moments || !stats)
        return FR_ERR_INVALID_ARG;
    if (!ws_ok(workspace, ws_bytes, fr_albedo_lse_workspace_bytes(B, H, W, K), 16)) return FR_ERR_WORKSPACE;
    if (!al_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    const long long npix = (long long)H * W;
    const AlGeom g = al_geom(B, npix);
    fr::AlArgs a{};
    a.basis = (const double*)basis; a.tri_ind = tri_ind; a.lighting = (const double*)lighting; a.normal_new = normal_new;
    a.abedo = abedo; a.im_gray = im_gray;
    a.partial = (double*)workspace; a.counts = a.partial + (size_t)B * g.tiles * 256;
    a.alpha = alpha; a.moments = (double*)moments; a.stats = (double*)stats; a.ridge = ridge;
    a.ntri = ntri; a.K = K; a.npix = (int)npix; a.tiles = g.tiles; a.wgpf = g.wgpf;
    hipLaunchKernelGGL(fr::albedo_lse_tile_kernel, dim3((unsigned)g.blocks), dim3(fr::AL_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::albedo_lse_finish_kernel, dim3((unsigned)B), dim3(fr::AL_FIN), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
