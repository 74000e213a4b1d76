// Colour photometric solve (opt-in; include/fr_hotpath.h, "colour photometric solve"): the colour model I_c = a_c s_c is linear in the
// lighting with the texture held and affine in alpha with the lighting held, so each half is a small linear least squares per face.
//
//   ps_basis_kernel        load time.  One thread per (triangle, channel, slot): the rasteriser's lookup of the texture basis (slots
//                          k < K) and of the mean texture (slot K), three widened fp32 terms in a fixed order, divided by 3.0.
//   ps_image_kernel        map pass, one lane per pixel: tex_img = m[t] + Phi[t] . alpha, a float64 chain rounded once.
//   ps_light_tile_kernel   per step.  The tile structure of csrc/fr_albedo_lse.hip: a face's pixels in row-major order are cut into tiles
//                          of PS_TILE = 256 and ONE WAVE OWNS A TILE (four tiles per workgroup; nothing shared, no LDS, no barrier).
//                          Lane l reads pixel l's planes once (coalesced) and runs the shader's own device function on them; for each
//                          group of four pixels the lanes fetch a_c, H_k, T_c, w and the channels' count bits of pixel 4 g + (lane >> 4)
//                          by lane shuffles, lane k = lane & 15 forms x^c_k, and one v_mfma_f64_16x16x4_f64 per channel adds the four
//                          pixels' (w x) x^T onto that channel's 16 x 16 sum.  Without a weight both operands are the same register.
//   ps_albedo_tile_kernel  per step.  The same structure; the three channels' rank-one updates go into ONE accumulator, channels
//                          ascending: lane k gathers Phi_c[t][k] (k < K) or m_c[t] (k = K), 8 (K + 1) contiguous bytes per channel.
//   ps_finish_kernel       one workgroup of 256 threads per unit -- a (face, channel) of the light fit, a face of the albedo fit:
//                          thread (i, j), i <= j, adds the tile partials in ascending tile order from +0.0 and mirrors; then ONE WAVE
//                          solves the unit in float64 (Cholesky by columns, lane r holds row r; every element's chain is the header's
//                          sequential source order, which is fr_albedo_lse_forward's) and writes the coefficients and stats.
// Plain float64 VALU under -ffp-contract=off outside the matrix instruction; ordinary vector stores; no atomics.
#include "fr_common.h"
#include "fr_shade.h"

#include <cmath>

namespace fr {

constexpr int PS_TILE = 256;                      // pixels per tile
constexpr int PS_WAVES = 4, PS_THREADS = 64 * PS_WAVES;   // tiles per workgroup of a tile kernel
constexpr int PS_KMAX = 15;                       // unknowns served: x has 16 slots, slot K holds the right-hand side
constexpr int PS_NL = 9;                          // lighting terms per channel
constexpr int PS_FIN = 256;                       // threads of the finish workgroup: one per element of M

typedef double ps_f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void ps_basis_kernel(const float* tri, const float* mu_tex, const float* pc_tex, int nver, int ntri,
                                                       int K, double* basis) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int S = K + 1;
    if (idx >= (long long)ntri * 3 * S) return;
    const int t = (int)(idx / (3 * S));
    const int rem = (int)(idx - (long long)t * 3 * S);
    const int c = rem / S, k = rem - c * S;
    const int v[3] = {f2i_x86(tri[t]), f2i_x86(tri[(size_t)ntri + t]), f2i_x86(tri[2 * (size_t)ntri + t])};
    double s = 0.0;   // a triangle with a vertex id outside [0, nver): a row of +0.0
    if (v[0] >= 0 && v[0] < nver && v[1] >= 0 && v[1] < nver && v[2] >= 0 && v[2] < nver) {
        double q[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const size_t row = (size_t)c * nver + v[j];
            q[j] = (double)(k < K ? pc_tex[row * K + k] : mu_tex[row]);
        }
        s = ((q[0] + q[1]) + q[2]) / 3.0;
    }
    basis[idx] = s;
}

__global__ __launch_bounds__(256) void ps_image_kernel(const double* basis, const float* tri_ind, const float* alpha, int ntri, int K,
                                                       size_t npix, float* tex_img) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const size_t face = blockIdx.y;
    const int t = f2i_x86(tri_ind[face * npix + p]);
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (t >= 0 && t < ntri) {
        const int S = K + 1;
        const double* row = basis + (size_t)t * 3 * S;
        const float* al = alpha + face * K;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double acc = row[c * S + K];
            for (int k = 0; k < K; k++) acc = acc + row[c * S + k] * (double)al[k];
            o[c] = (float)acc;
        }
    }
    float* dst = tex_img + (face * npix + p) * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

struct PsLightArgs {
    const float* tex_img;      // [B,npix,3]
    const float* normal;       // [B,npix,3]
    const float* tri_ind;      // [B,npix]
    const float* target;       // [B,npix,3]
    const float* weight;       // [B,npix] or null
    const float* gate;         // [B,3,9] or null
    double* partial;           // [B][tiles][3][4][64]
    double* counts;            // [B][tiles][3]
    size_t npix;
    float gain, offset;
    int tiles, wgpf;
};

__global__ __launch_bounds__(PS_THREADS) void ps_light_tile_kernel(PsLightArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int face = blockIdx.x / a.wgpf;
    const int tile = (blockIdx.x - face * a.wgpf) * PS_WAVES + wave;
    if (tile >= a.tiles) return;   // (a whole wave: the waves of a workgroup share nothing)
    const size_t npix = a.npix;
    const size_t fo = (size_t)face * npix;
    const int k = lane & 15, sub = lane >> 4;
    const bool weighted = a.weight != nullptr, gated = a.gate != nullptr;
    const double gain = (double)a.gain, off = (double)a.offset;
    float l[3 * PS_NL];   // the gate's lighting (uniform: scalar loads); without a gate the chain s_c is not looked at
#pragma unroll
    for (int i = 0; i < 3 * PS_NL; i++) l[i] = gated ? a.gate[(size_t)face * 3 * PS_NL + i] : 0.0f;
    ps_f64x4 acc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) acc[c] = ps_f64x4{0.0, 0.0, 0.0, 0.0};
    int cnt[3] = {0, 0, 0};
#pragma unroll 1
    for (int s = 0; s < PS_TILE / 64; s++) {
        const size_t base = (size_t)tile * PS_TILE + (size_t)s * 64;
        if (base >= npix) break;   // (sixteen groups of +0.0 would leave every accumulator's bits as they are)
        const bool in = base + lane < npix;
        const size_t p = in ? base + lane : npix - 1;   // (every plane read unconditionally at a clamped pixel)
        const float ti = a.tri_ind[fo + p];
        const float* tx = a.tex_img + (fo + p) * 3;
        const float* n = a.normal + (fo + p) * 3;
        const float* tg = a.target + (fo + p) * 3;
        const float T0 = tg[0], T1 = tg[1], T2 = tg[2];
        const float w = weighted ? a.weight[fo + p] : 1.0f;
        ShadeRGB o;
        float I[3];
        shade_pixel_rgb(tx[0], tx[1], tx[2], n[0], n[1], n[2], l, o, I);
        const bool live = in && ti >= 0.0f && (!weighted || w > 0.0f);   // (a NaN tri_ind or weight: not counted)
        int mask = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const bool counted = live && (!gated || o.s[c] > 0.0f);
            mask |= (counted ? 1 : 0) << c;
            cnt[c] += __builtin_popcountll(__ballot(counted));
        }
#pragma unroll 4
        for (int g = 0; g < 16; g++) {
            const int src = 4 * g + sub;
            const int m = __shfl(mask, src, 64);
            const float h1 = __shfl(o.h[1], src, 64), h2 = __shfl(o.h[2], src, 64), h3 = __shfl(o.h[3], src, 64),
                        h4 = __shfl(o.h[4], src, 64), h5 = __shfl(o.h[5], src, 64), h6 = __shfl(o.h[6], src, 64),
                        h7 = __shfl(o.h[7], src, 64), h8 = __shfl(o.h[8], src, 64);
            const float hk = k == 1 ? h1 : k == 2 ? h2 : k == 3 ? h3 : k == 4 ? h4 : k == 5 ? h5 : k == 6 ? h6 : k == 7 ? h7 : h8;
            const float ac[3] = {__shfl(o.a[0], src, 64), __shfl(o.a[1], src, 64), __shfl(o.a[2], src, 64)};
            const float Tc[3] = {__shfl(T0, src, 64), __shfl(T1, src, 64), __shfl(T2, src, 64)};
            const double wd = weighted ? (double)__shfl(w, src, 64) : 1.0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const bool used = ((m >> c) & 1) && k <= PS_NL;   // x is selected, not multiplied, to +0.0
                double x = 0.0;
                if (used) {
                    if (k == 0) x = (double)ac[c] * gain;
                    else if (k < PS_NL) x = ((double)ac[c] * (double)hk) * gain;
                    else x = (double)Tc[c] - off;
                }
                const double wx = weighted ? (used ? wd * x : 0.0) : x;
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(wx, x, acc[c], 0, 0, 0);
            }
        }
    }
    const size_t rec = (size_t)face * a.tiles + tile;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double* o = a.partial + (rec * 3 + c) * 256 + lane;
        o[0] = acc[c][0]; o[64] = acc[c][1]; o[128] = acc[c][2]; o[192] = acc[c][3];
        if (lane == 0) a.counts[rec * 3 + c] = (double)cnt[c];
    }
}

struct PsAlbedoArgs {
    const double* basis;       // [ntri][3][K+1]
    const float* tri_ind;      // [B,npix]
    const float* normal;       // [B,npix,3]
    const float* light;        // [B,3,9]
    const float* target;       // [B,npix,3]
    const float* weight;       // [B,npix] or null
    double* partial;           // [B][tiles][4][64]
    double* counts;            // [B][tiles]
    size_t npix;
    float gain, offset;
    int ntri, K, tiles, wgpf;
};

__global__ __launch_bounds__(PS_THREADS) void ps_albedo_tile_kernel(PsAlbedoArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int face = blockIdx.x / a.wgpf;
    const int tile = (blockIdx.x - face * a.wgpf) * PS_WAVES + wave;
    if (tile >= a.tiles) return;
    const size_t npix = a.npix;
    const size_t fo = (size_t)face * npix;
    const int k = lane & 15, sub = lane >> 4;
    const int K = a.K, S = a.K + 1;
    const bool weighted = a.weight != nullptr;
    const double gain = (double)a.gain, off = (double)a.offset;
    float l[3 * PS_NL];
#pragma unroll
    for (int i = 0; i < 3 * PS_NL; i++) l[i] = a.light[(size_t)face * 3 * PS_NL + i];
    ps_f64x4 acc = ps_f64x4{0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
#pragma unroll 1
    for (int s = 0; s < PS_TILE / 64; s++) {
        const size_t base = (size_t)tile * PS_TILE + (size_t)s * 64;
        if (base >= npix) break;
        const bool in = base + lane < npix;
        const size_t p = in ? base + lane : npix - 1;
        const int ti = f2i_x86(a.tri_ind[fo + p]);
        const float* n = a.normal + (fo + p) * 3;
        const float* tg = a.target + (fo + p) * 3;
        const float T0 = tg[0], T1 = tg[1], T2 = tg[2];
        const float w = weighted ? a.weight[fo + p] : 1.0f;
        ShadeRGB o;
        float I[3];
        shade_pixel_rgb(0.0f, 0.0f, 0.0f, n[0], n[1], n[2], l, o, I);   // (the chain s_c alone is taken: the albedo is the model's)
        const float sp0 = o.s[0] < 0.0f ? 0.0f : o.s[0], sp1 = o.s[1] < 0.0f ? 0.0f : o.s[1], sp2 = o.s[2] < 0.0f ? 0.0f : o.s[2];
        const bool counted = in && ti >= 0 && ti < a.ntri && (!weighted || w > 0.0f);
        const int t = counted ? ti : -1;
        cnt += __builtin_popcountll(__ballot(counted));
#pragma unroll 4
        for (int g = 0; g < 16; g++) {
            const int src = 4 * g + sub;
            const int tt = __shfl(t, src, 64);
            const float sp[3] = {__shfl(sp0, src, 64), __shfl(sp1, src, 64), __shfl(sp2, src, 64)};
            const float Tc[3] = {__shfl(T0, src, 64), __shfl(T1, src, 64), __shfl(T2, src, 64)};
            const double wd = weighted ? (double)__shfl(w, src, 64) : 1.0;
            const bool used = tt >= 0 && k <= K;
            const double* row = a.basis + (size_t)(used ? tt : 0) * 3 * S + (used ? k : 0);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                double x = 0.0;
                if (used) {
                    const double q = ((double)sp[c] * row[c * S]) * gain;
                    x = k < K ? q : ((double)Tc[c] - off) - q;
                }
                const double wx = weighted ? (used ? wd * x : 0.0) : x;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wx, x, acc, 0, 0, 0);
            }
        }
    }
    const size_t rec = (size_t)face * a.tiles + tile;
    double* o = a.partial + rec * 256 + lane;
    o[0] = acc[0]; o[64] = acc[1]; o[128] = acc[2]; o[192] = acc[3];
    if (lane == 0) a.counts[rec] = (double)cnt;
}

struct PsFinishArgs {
    const double* partial;     // [faces][tiles][NC][4][64]
    const double* counts;      // [faces][tiles][NC]
    const float* fallback;     // [units][K] or null: what a failed unit receives (null: +0)
    float* out;                // [units][K]
    double* moments;           // [units][16][16]
    double* stats;             // [units][4]
    double ridge;
    int NC, K, tiles;
};

// The f64 16x16x4 result layout (csrc/fr_geometry.hip): register g of lane l holds element (row = (l >> 4) + 4 g, column = l & 15), so a
// tile's record [register][lane] IS the 16 x 16 matrix in row-major order.  unit = blockIdx.x = face NC + channel.
__global__ __launch_bounds__(PS_FIN) void ps_finish_kernel(PsFinishArgs a) {
    __shared__ double M[16][16];
    __shared__ double count_sh;
    const int e = threadIdx.x, i = e >> 4, j = e & 15;
    const int unit = blockIdx.x, K = a.K, NC = a.NC;
    const int face = unit / NC, ch = unit - face * NC;
    if (i <= j) {
        // sixteen loads in flight per thread: the additions stay one chain in ascending tile order
        const double* src = a.partial + ((size_t)face * a.tiles * NC + ch) * 256 + i * 16 + j;
        const size_t stride = (size_t)NC * 256;
        double sum = 0.0;
        int t = 0;
        for (; t + 16 <= a.tiles; t += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = src[(size_t)(t + u) * stride];
#pragma unroll
            for (int u = 0; u < 16; u++) sum = sum + v[u];
        }
        for (; t < a.tiles; t++) sum = sum + src[(size_t)t * stride];
        M[i][j] = sum; M[j][i] = sum;
        double* mo = a.moments + (size_t)unit * 256;
        mo[i * 16 + j] = sum; mo[j * 16 + i] = sum;
    } else if (e == 16) {   // an idle thread of the lower triangle counts meanwhile (integers: exact in any order; kept a chain)
        const double* src = a.counts + (size_t)face * a.tiles * NC + ch;
        double count = 0.0;
        for (int t = 0; t < a.tiles; t++) count = count + src[(size_t)t * NC];
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
    const double tiny = 9.094947017729282379150390625e-13;   // 2^-40: a pivot of a Gram matrix of condition 1e8 is >= 1e-8 G'_cc
    double grow[PS_KMAX], Lrow[PS_KMAX], al[PS_KMAX];
#pragma unroll
    for (int m = 0; m < PS_KMAX; m++) {
        grow[m] = M[r][m];
        Lrow[m] = 0.0;
        al[m] = 0.0;
    }
    const double rhs = M[r][K];
    // Cholesky of G' = G + lam I by columns, inner sums ascending from +0.0; Lrow[c] is meaningful on the lanes r >= c alone
#pragma unroll
    for (int c = 0; c < PS_KMAX; c++) {
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
        for (int m = 0; m < PS_KMAX; m++) {
            if (m < K) {
                const double ym = __shfl((rhs - qy) / Lrow[m], m, 64);
                if (r == m) y = ym;
                if (r > m) qy = qy + Lrow[m] * ym;
            }
        }
#pragma unroll
        for (int p = PS_KMAX - 1; p >= 0; p--) {   // L^T x = y: every lane forms x_p, inner sum ascending in m
            if (p < K) {
                double q = 0.0;
#pragma unroll
                for (int m = p + 1; m < PS_KMAX; m++) {
                    const double lmp = __shfl(Lrow[p], m, 64);   // L[m][p] lives on lane m
                    if (m < K) q = q + lmp * al[m];
                }
                al[p] = (__shfl(y, p, 64) - q) / __shfl(Lrow[p], p, 64);
            }
        }
#pragma unroll
        for (int p = 0; p < PS_KMAX; p++)
            if (p < K) ok = ok && __builtin_isfinite(al[p]);
    }
    double E1 = E0;   // a failed unit: the residual energy at zero coefficients
    if (ok) {
#pragma unroll
        for (int p = 0; p < PS_KMAX; p++) al[p] = (double)(float)al[p];   // E1 is taken at the coefficients the caller receives
        double ga = 0.0;   // (G x)_r on lane r
#pragma unroll
        for (int c = 0; c < PS_KMAX; c++)
            if (c < K) ga = ga + grow[c] * al[c];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int p = 0; p < PS_KMAX; p++)
            if (p < K) s1 = s1 + al[p] * M[p][K];
#pragma unroll
        for (int p = 0; p < PS_KMAX; p++) {
            const double gap = __shfl(ga, p, 64);
            if (p < K) s2 = s2 + al[p] * gap;
        }
        E1 = (E0 - 2.0 * s1) + s2;
    }
    if (e != 0) return;
    float* xo = a.out + (size_t)unit * K;
    const float* fb = a.fallback ? a.fallback + (size_t)unit * K : nullptr;
#pragma unroll
    for (int p = 0; p < PS_KMAX; p++)
        if (p < K) xo[p] = ok ? (float)al[p] : (fb ? fb[p] : 0.0f);
    double* so = a.stats + (size_t)unit * 4;
    so[0] = count; so[1] = E0; so[2] = E1; so[3] = ok ? 1.0 : 0.0;
}

}  // namespace fr

// The sizes and the launch geometry, stated in ONE place: the size functions, the launchers and the test hook read them from here.
namespace {
struct PsGeom {
    int tiles;              // per face
    int wgpf;               // tile-kernel workgroups per face
    long long blocks;       // of a tile kernel
};
PsGeom ps_geom(int B, long long npix) {
    PsGeom g;
    g.tiles = (int)((npix + fr::PS_TILE - 1) / fr::PS_TILE);
    g.wgpf = (g.tiles + fr::PS_WAVES - 1) / fr::PS_WAVES;
    g.blocks = (long long)g.wgpf * B;
    return g;
}
constexpr size_t PS_LDS_FIN = (size_t)257 * sizeof(double);
constexpr int PS_MAX_FACES = 65535;
bool ps_k_served(int K) { return K >= 1 && K <= fr::PS_KMAX; }
// more than 65,535 faces, more than 2^31 - 1 pixels per face, or more workgroups than one grid takes
bool ps_size_ok(int B, int H, int W) {
    const long long npix = (long long)H * W;
    return B <= PS_MAX_FACES && npix <= 0x7FFFFFFFll && ps_geom(B, npix).blocks <= 0x7FFFFFFFll;
}
bool ps_finite(double x) { return std::isfinite(x); }
}  // namespace

extern "C" {

size_t fr_albedo_basis_rgb_bytes(int ntri, int K) {
    if (ntri <= 0 || !ps_k_served(K)) return 0;
    return (size_t)ntri * 3 * (K + 1) * sizeof(double);
}

int fr_albedo_basis_rgb_build(const float* tri, const float* mu_tex, const float* pc_tex, int nver, int ntri, int K, void* basis,
                              size_t basis_bytes, void* stream) {
    if (nver < 0 || ntri < 0) return FR_ERR_INVALID_ARG;
    if (ntri == 0) return FR_OK;
    if (!tri || (nver > 0 && (!mu_tex || !pc_tex))) return FR_ERR_INVALID_ARG;
    if (!ws_ok(basis, basis_bytes, fr_albedo_basis_rgb_bytes(ntri, K), 16)) return FR_ERR_WORKSPACE;
    if (!ps_k_served(K) || ntri > (1 << 24)) return FR_ERR_UNSUPPORTED;   // (float-stored ids)
    const long long n = (long long)ntri * 3 * (K + 1);
    hipLaunchKernelGGL(fr::ps_basis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tri, mu_tex, pc_tex,
                       nver, ntri, K, (double*)basis);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_albedo_image_rgb(const void* basis, const float* tri_ind, const float* alpha, int B, int ntri, int H, int W, int K,
                        float* tex_img, void* stream) {
    if (B < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!tri_ind || !alpha || !tex_img || (ntri > 0 && !basis)) return FR_ERR_INVALID_ARG;
    if (!ps_k_served(K) || !ps_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(fr::ps_image_kernel, dim3((unsigned)((npix + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const double*)basis, tri_ind, alpha, ntri, K, npix, tex_img);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

// workspace of either solve: the light fit's tile partials [B][tiles][3][4][64], then its tile counts [B][tiles][3]; float64.  The
// albedo fit lays its own [B][tiles][4][64] and [B][tiles] into the same buffer.
size_t fr_photo_solve_rgb_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !ps_size_ok(B, H, W)) return 0;
    return (size_t)B * ps_geom(B, (long long)H * W).tiles * (3 * 257) * sizeof(double);
}

// test hook: out = {pixels per tile, tiles per face, workgroups of a tile kernel, workgroups of the light fit's finish kernel,
// workgroups of the albedo fit's, static LDS bytes of a finish workgroup}; zeros for an empty shape or one the launchers refuse
void fr_debug_photo_solve_rgb_geom(int B, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    if (B <= 0 || H <= 0 || W <= 0 || !ps_size_ok(B, H, W)) return;
    const PsGeom g = ps_geom(B, (long long)H * W);
    out[0] = fr::PS_TILE; out[1] = g.tiles; out[2] = (int)g.blocks; out[3] = 3 * B; out[4] = B; out[5] = (int)PS_LDS_FIN;
}

int fr_photo_light_lse_rgb_forward(const float* tex_img, const float* normal, const float* tri_ind, const float* target,
                                   const float* weight, const float* gate_light, int B, int H, int W, float gain, float offset,
                                   double ridge, float* light, void* moments, void* stats, void* workspace, size_t ws_bytes,
                                   void* stream) {
    if (B < 0 || H < 0 || W < 0 || !(ridge >= 0.0 && ps_finite(ridge)) || !ps_finite(gain) || !ps_finite(offset))
        return FR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!tex_img || !normal || !tri_ind || !target || !light || !moments || !stats) return FR_ERR_INVALID_ARG;
    if (!ws_ok(workspace, ws_bytes, fr_photo_solve_rgb_workspace_bytes(B, H, W), 16)) return FR_ERR_WORKSPACE;
    if (!ps_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    const long long npix = (long long)H * W;
    const PsGeom g = ps_geom(B, npix);
    fr::PsLightArgs a{};
    a.tex_img = tex_img; a.normal = normal; a.tri_ind = tri_ind; a.target = target; a.weight = weight; a.gate = gate_light;
    a.partial = (double*)workspace; a.counts = a.partial + (size_t)B * g.tiles * 3 * 256;
    a.npix = (size_t)npix; a.gain = gain; a.offset = offset; a.tiles = g.tiles; a.wgpf = g.wgpf;
    fr::PsFinishArgs f{};
    f.partial = a.partial; f.counts = a.counts; f.fallback = gate_light; f.out = light; f.moments = (double*)moments;
    f.stats = (double*)stats; f.ridge = ridge; f.NC = 3; f.K = fr::PS_NL; f.tiles = g.tiles;
    hipLaunchKernelGGL(fr::ps_light_tile_kernel, dim3((unsigned)g.blocks), dim3(fr::PS_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::ps_finish_kernel, dim3((unsigned)(3 * B)), dim3(fr::PS_FIN), 0, (hipStream_t)stream, f);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_albedo_lse_rgb_forward(const void* basis, const float* tri_ind, const float* normal, const float* light, const float* target,
                              const float* weight, int B, int ntri, int H, int W, int K, float gain, float offset, double ridge,
                              float* alpha, void* moments, void* stats, void* workspace, size_t ws_bytes, void* stream) {
    if (B < 0 || ntri < 0 || H < 0 || W < 0 || !(ridge >= 0.0 && ps_finite(ridge)) || !ps_finite(gain) || !ps_finite(offset))
        return FR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!tri_ind || !normal || !light || !target || !alpha || !moments || !stats || (ntri > 0 && !basis)) return FR_ERR_INVALID_ARG;
    if (!ws_ok(workspace, ws_bytes, fr_photo_solve_rgb_workspace_bytes(B, H, W), 16)) return FR_ERR_WORKSPACE;
    if (!ps_k_served(K) || !ps_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    const long long npix = (long long)H * W;
    const PsGeom g = ps_geom(B, npix);
    fr::PsAlbedoArgs a{};
    a.basis = (const double*)basis; a.tri_ind = tri_ind; a.normal = normal; a.light = light; a.target = target; a.weight = weight;
    a.partial = (double*)workspace; a.counts = a.partial + (size_t)B * g.tiles * 256;
    a.npix = (size_t)npix; a.gain = gain; a.offset = offset; a.ntri = ntri; a.K = K; a.tiles = g.tiles; a.wgpf = g.wgpf;
    fr::PsFinishArgs f{};
    f.partial = a.partial; f.counts = a.counts; f.fallback = nullptr; f.out = alpha; f.moments = (double*)moments;
    f.stats = (double*)stats; f.ridge = ridge; f.NC = 1; f.K = K; f.tiles = g.tiles;
    hipLaunchKernelGGL(fr::ps_albedo_tile_kernel, dim3((unsigned)g.blocks), dim3(fr::PS_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::ps_finish_kernel, dim3((unsigned)B), dim3(fr::PS_FIN), 0, (hipStream_t)stream, f);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
