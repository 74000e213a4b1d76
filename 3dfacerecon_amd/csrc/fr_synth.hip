// On-device synthetic training batches (include/fr_hotpath.h, "synthetic batches"): the counter-based parameter sampler, the per-face
// albedo blend and the shading / compositing post-pass over a render's planes.  All three are streaming or tiny: one lane per
// element, coalesced, no atomics; LDS only to turn the texture basis' row-major reads into coalesced ones.  fp32 in the header's
// stated order, one rounding per operation (-ffp-contract=off).  The blend has an adjoint (synth_texture_bwd_kernel and its finish
// step): float64 sums of exact products in an association that is a function of (N, K) alone.  The shader is written once, over the
// shading model of fr_shade.h (synth_shade_body<M>): synth_shade_kernel is the gray model's, synth_shade_rgb_kernel the colour one's.
#include "fr_common.h"
#include "fr_shade.h"

namespace fr {

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2]
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* out) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct SynthParamsArgs {
    unsigned long long seed, first_face;
    int B, ns, ne, K, draws;
    float half_im, beta, focal;
    float* params;
    float* light;
    float* alpha;
    float light_lo[4], light_hi[4];
    float alpha_lo[FR_SYNTH_MAX_TEX], alpha_hi[FR_SYNTH_MAX_TEX];
};

// one lane per draw j of face b: draw j is word j & 3 of the block with counter (j >> 2, g_lo, g_hi, 0), g = first_face + b
__global__ __launch_bounds__(256) void synth_params_kernel(const SynthParamsArgs a) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    const int b = (int)blockIdx.y;
    if (j >= a.draws) return;
    const unsigned long long g = a.first_face + (unsigned long long)b;
    uint32_t w[4];
    philox4x32_10((uint32_t)j >> 2, (uint32_t)g, (uint32_t)(g >> 32), 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
    const uint32_t word = (j & 3) == 0 ? w[0] : (j & 3) == 1 ? w[1] : (j & 3) == 2 ? w[2] : w[3];
    const float u = (float)(word >> 8) * 5.9604644775390625e-8f;   // 2^-24: exact, in [0,1)
    const int d = 7 + a.ns + a.ne;
    float* prm = a.params + (size_t)b * d;
    if (j < 6) {   // pose = beta base + (1 - beta) rand, base = (0, 0, 0, im/2, im/2, 0, focal)
        const float c = 0.01745329238474369049072265625f;   // fl32(pi / 180)
        const float omb = 1.0f - a.beta;
        float rnd, base;
        int col;
        if (j == 0) { rnd = (-75.0f + 120.0f * u) * c; base = 0.0f; col = 0; }
        else if (j == 1) { rnd = (-90.0f + 180.0f * u) * c; base = 0.0f; col = 1; }
        else if (j == 2) { rnd = (-30.0f + 60.0f * u) * c; base = 0.0f; col = 2; }
        else if (j == 3) { rnd = u * a.focal; base = a.focal; col = 6; }
        else { rnd = 60.0f * u; base = a.half_im; col = j - 1; }   // tx -> 3, ty -> 4
        prm[col] = a.beta * base + omb * rnd;
        if (j == 5) prm[5] = 0.0f;   // tz = beta 0 + (1 - beta) 0 with beta in [0, 1]: no draw
        return;
    }
    int k = j - 6;
    if (k < a.ns) { prm[7 + k] = u * 1.0e4f; return; }
    k -= a.ns;
    if (k < a.ne) { prm[7 + a.ns + k] = -1.5f + 3.0f * u; return; }
    k -= a.ne;
    if (k < 4) { a.light[(size_t)b * 4 + k] = a.light_lo[k] + (a.light_hi[k] - a.light_lo[k]) * u; return; }
    k -= 4;
    a.alpha[(size_t)b * a.K + k] = a.alpha_lo[k] + (a.alpha_hi[k] - a.alpha_lo[k]) * u;
}

// One lane per (c, p) row and per face of its workgroup's group of TX_FACES: acc = mu_tex[c][p]; acc = acc + pc_tex[c N + p][k] *
// alpha[b][k], k ascending -- each output's own chain, whatever the tiling.  A workgroup's 256 rows of pc_tex are one contiguous
// run of 256 K floats: it is fetched ONCE per group of faces, coalesced, TX_KC columns at a time into LDS (row pitch TX_KC + 1: a
// lane's walk along its row is conflict-free), instead of each lane striding K floats through the cache once per face.  alpha is
// wave-uniform (scalar loads).  The stores are 64 contiguous floats per wave and face.
constexpr int TX_ROWS = 256, TX_KC = 16, TX_FACES = 8;
__global__ __launch_bounds__(TX_ROWS) void synth_texture_kernel(const float* __restrict__ mu_tex, const float* __restrict__ pc_tex,
                                                                const float* __restrict__ alpha, int B, int N, int K,
                                                                float* __restrict__ tex) {
    __shared__ float tile[TX_ROWS * (TX_KC + 1)];
    const int tid = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * TX_ROWS;
    const int c = (int)blockIdx.y, b0 = (int)blockIdx.z * TX_FACES;
    const int nb = min(TX_FACES, B - b0), nrows = min(TX_ROWS, N - row0);
    const bool live = tid < nrows;
    const size_t row = (size_t)c * N + row0 + (live ? tid : 0);
    float acc[TX_FACES];
    const float mu = mu_tex[row];
#pragma unroll
    for (int f = 0; f < TX_FACES; f++) acc[f] = mu;
    const float* src = pc_tex + ((size_t)c * N + row0) * (size_t)K;   // rows row0 .. row0 + nrows of channel c
    for (int k0 = 0; k0 < K; k0 += TX_KC) {
        const int kc = min(TX_KC, K - k0);
        if (k0) __syncthreads();
        for (int e = tid; e < nrows * kc; e += TX_ROWS) {
            const int r = e / kc, kk = e - r * kc;
            tile[r * (TX_KC + 1) + kk] = src[(size_t)r * K + k0 + kk];
        }
        __syncthreads();
        if (live) {
            for (int kk = 0; kk < kc; kk++) {
                const float pc = tile[tid * (TX_KC + 1) + kk];
#pragma unroll
                for (int f = 0; f < TX_FACES; f++)
                    if (f < nb) acc[f] = acc[f] + pc * alpha[(size_t)(b0 + f) * K + k0 + kk];
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int f = 0; f < TX_FACES; f++)
        if (f < nb) tex[(size_t)(b0 + f) * 3 * N + row] = acc[f];
}

// The blend's adjoint, grad_alpha[b][k] = sum over the 3N rows r of pc_tex[r][k] * grad_tex[b][r], mirrors the forward's tiling over the
// FLAT row index r: a workgroup owns TX_ROWS consecutive rows and a group of TX_FACES faces, one lane per row; it stages its run of
// pc_tex TX_KC columns at a time in LDS (fetched once per group of faces, coalesced) and keeps its rows of grad_tex in registers.
// Every product of two widened fp32 values is exact in float64; the 256 products of a (face, column) meet in the fixed lane tree
// (groups of 64 with k = 32 .. 1, then (w0 + w2) + (w1 + w3); a row past 3N holds +0.0) and go out as one partial
// [b][k][row tile].  synth_texture_bwd_finish_kernel: one wave per (b, k); lane i chains the partials of the row tiles i, i + 64, ..
// in ascending order from +0.0 (contiguous reads), the 64 chains meet in the same lane tree, one rounding to fp32.  No atomics.
__global__ __launch_bounds__(TX_ROWS) void synth_texture_bwd_kernel(const float* __restrict__ pc_tex, const float* __restrict__ grad_tex,
                                                                    int B, int R, int K, double* __restrict__ part) {
    __shared__ float tile[TX_ROWS * (TX_KC + 1)];
    __shared__ double wsum[TX_FACES][TX_KC][TX_ROWS / 64];
    const int tid = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * TX_ROWS;
    const int b0 = (int)blockIdx.y * TX_FACES;
    const int nb = min(TX_FACES, B - b0), nrows = min(TX_ROWS, R - row0);
    const bool live = tid < nrows;
    double g[TX_FACES];
#pragma unroll
    for (int f = 0; f < TX_FACES; f++) g[f] = (live && f < nb) ? (double)grad_tex[(size_t)(b0 + f) * R + row0 + tid] : 0.0;
    const float* src = pc_tex + (size_t)row0 * (size_t)K;
    for (int k0 = 0; k0 < K; k0 += TX_KC) {
        const int kc = min(TX_KC, K - k0);
        if (k0) __syncthreads();   // (the last chunk's tile and wave sums have been read)
        for (int e = tid; e < nrows * kc; e += TX_ROWS) {
            const int r = e / kc, kk = e - r * kc;
            tile[r * (TX_KC + 1) + kk] = src[(size_t)r * K + k0 + kk];
        }
        __syncthreads();
        for (int kk = 0; kk < kc; kk++) {
            const double pc = live ? (double)tile[tid * (TX_KC + 1) + kk] : 0.0;
#pragma unroll
            for (int f = 0; f < TX_FACES; f++) {
                if (f < nb) {   // (workgroup-uniform)
                    const double v = wave_tree_f64(live ? pc * g[f] : 0.0);
                    if ((tid & 63) == 0) wsum[f][kk][tid >> 6] = v;
                }
            }
        }
        __syncthreads();
        if (tid < nb * kc) {
            const int f = tid / kc, kk = tid - f * kc;
            part[((size_t)(b0 + f) * K + k0 + kk) * gridDim.x + blockIdx.x] =
                (wsum[f][kk][0] + wsum[f][kk][2]) + (wsum[f][kk][1] + wsum[f][kk][3]);
        }
    }
}
__global__ __launch_bounds__(64) void synth_texture_bwd_finish_kernel(const double* __restrict__ part, int tiles,
                                                                      float* __restrict__ grad_alpha) {
    const double* mine = part + (size_t)blockIdx.x * tiles;   // blockIdx.x = b K + k
    double acc = 0.0;
    for (int t = (int)threadIdx.x; t < tiles; t += 64) acc = acc + mine[t];
    acc = wave_tree_f64(acc);
    if (threadIdx.x == 0) grad_alpha[blockIdx.x] = (float)acc;
}

// The shader, one lane per pixel, for the model M of fr_shade.h (the photometric loss runs the same M::shade): im [B,H,W,NC] is the
// model's image where the face covers the pixel and the background's NC channels elsewhere (0 without one).  The colour model also
// writes the gray of the result, background included, where im_gray is wanted.
template <class M>
__device__ __forceinline__ void synth_shade_body(const float* __restrict__ tex_img, const float* __restrict__ normal,
                                                 const float* __restrict__ tri_ind, const float* __restrict__ light,
                                                 const float* __restrict__ background, int bg_batch, int HW, float gain, float offset,
                                                 float* __restrict__ im, float* __restrict__ im_gray, float* __restrict__ mask) {
    constexpr int NC = M::NC;
    const unsigned int pix = blockIdx.x * 256u + threadIdx.x;
    const int b = (int)blockIdx.y;
    if (pix >= (unsigned int)HW) return;
    const size_t i = (size_t)b * (size_t)HW + pix;
    float v[NC];
    const bool covered = tri_ind[i] >= 0.0f;
    if (!covered) {
        const size_t k = (bg_batch == 1 ? (size_t)0 : (size_t)b * (size_t)HW) + pix;
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] = background ? background[NC * k + c] : 0.0f;
    } else {
        typename M::State sh;
        float I[NC];
        M::shade(tex_img + 3 * i, normal + 3 * i, light + (size_t)b * (NC * M::NK), sh, I);
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] = I[c] * gain + offset;
    }
#pragma unroll
    for (int c = 0; c < NC; c++) im[NC * i + c] = v[c];
    if constexpr (NC == 3) {
        if (im_gray) im_gray[i] = fr::gray_of(v[0], v[1], v[2]);
    }
    mask[i] = covered ? 1.0f : 0.0f;
}
// (two named kernels, not instantiations of one: profiles and tests/test_photo_rgb_cpu.py know them by these names)
__global__ __launch_bounds__(256) void synth_shade_kernel(const float* __restrict__ tex_img, const float* __restrict__ normal,
                                                          const float* __restrict__ tri_ind, const float* __restrict__ light,
                                                          const float* __restrict__ background, int bg_batch, int HW, float gain,
                                                          float offset, float* __restrict__ im_gray, float* __restrict__ mask) {
    synth_shade_body<GrayModel>(tex_img, normal, tri_ind, light, background, bg_batch, HW, gain, offset, im_gray, nullptr, mask);
}
__global__ __launch_bounds__(256) void synth_shade_rgb_kernel(const float* __restrict__ tex_img, const float* __restrict__ normal,
                                                              const float* __restrict__ tri_ind, const float* __restrict__ light,
                                                              const float* __restrict__ background, int bg_batch, int HW, float gain,
                                                              float offset, float* __restrict__ im_rgb, float* __restrict__ im_gray,
                                                              float* __restrict__ mask) {
    synth_shade_body<ColourModel>(tex_img, normal, tri_ind, light, background, bg_batch, HW, gain, offset, im_rgb, im_gray, mask);
}

// The colour lighting's sampler: one lane per draw j = 9 c + k of face b, word j & 3 of the block with counter (j >> 2, g_lo, g_hi, 1)
// -- the fourth word is 1 where synth_params_kernel's is 0, so the two streams are disjoint under one seed.
struct SynthLightRgbArgs {
    unsigned long long seed, first_face;
    float* light;   // [B,3,9]
    float lo[27], hi[27];
};
__global__ __launch_bounds__(64) void synth_light_rgb_kernel(const SynthLightRgbArgs a) {
    const int j = (int)threadIdx.x;
    const int b = (int)blockIdx.x;
    if (j >= 27) return;
    const unsigned long long g = a.first_face + (unsigned long long)b;
    uint32_t w[4];
    philox4x32_10((uint32_t)j >> 2, (uint32_t)g, (uint32_t)(g >> 32), 1u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
    const uint32_t word = (j & 3) == 0 ? w[0] : (j & 3) == 1 ? w[1] : (j & 3) == 2 ? w[2] : w[3];
    const float u = (float)(word >> 8) * 5.9604644775390625e-8f;   // 2^-24: exact, in [0,1)
    a.light[(size_t)b * 27 + j] = a.lo[j] + (a.hi[j] - a.lo[j]) * u;
}

}  // namespace fr

int fr_launch_synth_light_rgb(unsigned long long seed, unsigned long long first_face, int B, const float* ranges, float* light,
                              hipStream_t stream) {
    fr::SynthLightRgbArgs a{};
    a.seed = seed; a.first_face = first_face; a.light = light;
    for (int j = 0; j < 27; j++) { a.lo[j] = ranges[2 * j]; a.hi[j] = ranges[2 * j + 1]; }
    hipLaunchKernelGGL(fr::synth_light_rgb_kernel, dim3((unsigned)B, 1, 1), dim3(64, 1, 1), 0, stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_launch_synth_params(unsigned long long seed, unsigned long long first_face, int B, int ns, int ne, int K, float im_size,
                           float beta, float focal, const float* light_ranges, const float* alpha_ranges, float* params,
                           float* light, float* alpha, hipStream_t stream) {
    fr::SynthParamsArgs a{};
    a.seed = seed; a.first_face = first_face;
    a.B = B; a.ns = ns; a.ne = ne; a.K = K; a.draws = 6 + ns + ne + 4 + K;
    a.half_im = im_size * 0.5f; a.beta = beta; a.focal = focal;
    a.params = params; a.light = light; a.alpha = alpha;
    for (int k = 0; k < 4; k++) { a.light_lo[k] = light_ranges[2 * k]; a.light_hi[k] = light_ranges[2 * k + 1]; }
    for (int k = 0; k < K; k++) { a.alpha_lo[k] = alpha_ranges[2 * k]; a.alpha_hi[k] = alpha_ranges[2 * k + 1]; }
    hipLaunchKernelGGL(fr::synth_params_kernel, dim3((unsigned)((a.draws + 255) / 256), (unsigned)B, 1), dim3(256, 1, 1), 0, stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_launch_synth_texture(const float* mu_tex, const float* pc_tex, const float* alpha, int B, int N, int K, float* tex,
                            hipStream_t stream) {
    const dim3 grid((unsigned)((N + fr::TX_ROWS - 1) / fr::TX_ROWS), 3, (unsigned)((B + fr::TX_FACES - 1) / fr::TX_FACES));
    hipLaunchKernelGGL(fr::synth_texture_kernel, grid, dim3(fr::TX_ROWS, 1, 1), 0, stream, mu_tex, pc_tex, alpha, B, N, K, tex);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

// the shaders' launch: out = the kernel's output planes, in its order
template <class Kernel, class... Out>
static int synth_shade_launch(Kernel kernel, const float* tex_img, const float* normal, const float* tri_ind, const float* light,
                              const float* background, int bg_batch, int B, int H, int W, float gain, float offset, hipStream_t stream,
                              Out*... out) {
    const int HW = H * W;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((long long)HW + 255) / 256), (unsigned)B, 1), dim3(256, 1, 1), 0, stream, tex_img, normal,
                       tri_ind, light, background, bg_batch, HW, gain, offset, out...);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_launch_synth_shade(const float* tex_img, const float* normal, const float* tri_ind, const float* light,
                          const float* background, int bg_batch, int B, int H, int W, float gain, float offset, float* im_gray,
                          float* mask, hipStream_t stream) {
    return synth_shade_launch(fr::synth_shade_kernel, tex_img, normal, tri_ind, light, background, bg_batch, B, H, W, gain, offset,
                              stream, im_gray, mask);
}

int fr_launch_synth_shade_rgb(const float* tex_img, const float* normal, const float* tri_ind, const float* light,
                              const float* background, int bg_batch, int B, int H, int W, float gain, float offset, float* im_rgb,
                              float* im_gray, float* mask, hipStream_t stream) {
    return synth_shade_launch(fr::synth_shade_rgb_kernel, tex_img, normal, tri_ind, light, background, bg_batch, B, H, W, gain, offset,
                              stream, im_rgb, im_gray, mask);
}

size_t fr_synth_texture_backward_workspace_impl(int B, int N, int K) {
    if (B < 1 || N < 1 || K < 1 || B > 65535 || (long long)N * 3 > 0x7FFFFFFFll - fr::TX_ROWS || (long long)B * K > 0x7FFFFFFFll) return 0;
    const size_t tiles = (size_t)((3ll * N + fr::TX_ROWS - 1) / fr::TX_ROWS);
    return tiles * (size_t)B * (size_t)K * sizeof(double);
}

int fr_launch_synth_texture_backward(const float* pc_tex, const float* grad_tex, int B, int N, int K, float* grad_alpha,
                                     void* workspace, hipStream_t stream) {
    const int R = 3 * N, tiles = (R + fr::TX_ROWS - 1) / fr::TX_ROWS, BK = B * K;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(fr::synth_texture_bwd_kernel, dim3((unsigned)tiles, (unsigned)((B + fr::TX_FACES - 1) / fr::TX_FACES), 1),
                       dim3(fr::TX_ROWS, 1, 1), 0, stream, pc_tex, grad_tex, B, R, K, part);
    hipLaunchKernelGGL(fr::synth_texture_bwd_finish_kernel, dim3((unsigned)BK, 1, 1), dim3(64, 1, 1), 0, stream, (const double*)part, tiles,
                       grad_alpha);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
