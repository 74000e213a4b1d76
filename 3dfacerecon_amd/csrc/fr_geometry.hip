// Gram-form geometry loss (opt-in; include/fr_hotpath.h, "Gram-form geometry loss"): mean((U d)^2) = d^T (U^T U) d / (3N B) with
// U = [pc_shape | pc_exp] a constant of the model, so G = U^T U is built ONCE, in float64, and a training step touches the basis no
// more: the loss and its gradient are G against B short vectors.
//
//   geometry_gram_chunk_kernel    load time.  The row axis of U is cut into chunks of GG_CHUNK = 1,024 rows -- a compile-time constant, no
//                                 function of the device, of B or of a knob, so G's bits are a function of (N, n_shape, n_exp, the basis)
//                                 alone.  A workgroup of 8 waves owns a chunk: it stages slabs of GG_SLAB = 32 rows x Kp columns in LDS
//                                 (fp32, read straight from the reference layouts with 4-byte loads: the row strides, 199 and 29 floats,
//                                 promise no alignment; rows past 3N and columns past K are +0), the next slab's loads in flight in
//                                 registers while this one is multiplied.  The 16 x 16 tile pairs (ti <= tj) of the upper triangle are
//                                 dealt to the waves round robin (K = 228: 120 pairs, 15 per wave, 120 accumulator VGPRs); per four rows a
//                                 wave reads its two fragments from LDS, widens them (every product of two widened fp32 is exact in
//                                 float64) and issues one v_mfma_f64_16x16x4_f64 per pair.  The accumulators go to the workspace as they
//                                 lie in the registers: partial[chunk][pair][register][lane].
//   geometry_gram_finish_kernel   one thread per element i <= j of G: adds the chunk partials IN CHUNK ORDER from +0.0 and writes the one
//                                 value to G[i][j] and G[j][i]; an element with i >= K or j >= K is written as +0.0 without reading
//                                 anything (a non-finite basis entry times a pad's zero would be a NaN).
//   geometry_loss_face_kernel     per step.  One workgroup per face, d widened into LDS, thread k runs the chain y_k = y_k + G[j][k] * d_j
//                                 over j (column access: coalesced; G is symmetric bit for bit), then the products d_k * y_k are formed in
//                                 parallel and thread 0 adds them in k order: q[b].
//   geometry_loss_sum_kernel      one wave: S = chain over b of q[b], loss = fl32(S / (3N B)).
//   geometry_loss_backward_kernel elementwise: grad_diff[b][k] = fl32((grad_loss * 2 / (3N B)) * y[b][k]).
// Plain float64 VALU under -ffp-contract=off in the three per-step kernels: every product and every sum rounds on its own, which is what
// tests/ref_geometry_gram.py restates in numpy.
#include "fr_common.h"

namespace fr {

constexpr int GG_CHUNK = 1024;                       // rows of U per workgroup
constexpr int GG_SLAB = 32;                          // rows staged in LDS at a time
constexpr int GG_WAVES = 8, GG_THREADS = 64 * GG_WAVES;
constexpr int GG_KMAX = 256;                         // coefficients served
constexpr int GG_TILES_MAX = GG_KMAX / 16;
constexpr int GG_PAIRS_MAX = GG_TILES_MAX * (GG_TILES_MAX + 1) / 2;              // 136
constexpr int GG_PAIRS_PER_WAVE = (GG_PAIRS_MAX + GG_WAVES - 1) / GG_WAVES;      // 17
// LDS row pitch in floats: 272 = 4 x 64 + 16, so the four rows a fragment read touches (16 consecutive floats each) lie in four
// different groups of 16 banks for every Kp
constexpr int GG_PITCH = GG_KMAX + 16;
constexpr int GG_LOADS = GG_SLAB * GG_KMAX / GG_THREADS;                         // 16 staged elements per thread and slab
constexpr int GL_THREADS = 256;                      // per-step kernels: one thread per coefficient

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct GgArgs {
    const float* pc_shape;   // [rows, ns]
    const float* pc_exp;     // [rows, ne]
    double* partial;         // [chunks][pairs][4][64]
    long long rows;          // 3N
    int ns, ne, Kp, tiles, pairs;
};

// element (row, c) of [pc_shape | pc_exp], +0 past the matrix
__device__ __forceinline__ float gg_elem(const GgArgs& a, long long row, int c) {
    if (row >= a.rows) return 0.0f;
    if (c < a.ns) return a.pc_shape[(size_t)row * a.ns + c];
    if (c < a.ns + a.ne) return a.pc_exp[(size_t)row * a.ne + (c - a.ns)];
    return 0.0f;
}

__global__ __launch_bounds__(GG_THREADS) void geometry_gram_chunk_kernel(GgArgs a) {
    __shared__ float slab[GG_SLAB * GG_PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long row0 = (long long)blockIdx.x * GG_CHUNK;
    const long long left = a.rows - row0;
    const int nrow = left < GG_CHUNK ? (int)left : GG_CHUNK;

    // this wave's pairs: p = wave + GG_WAVES s -> (ti, tj), ti <= tj, row-major over the upper triangle; kept as LDS column offsets
    int aoff[GG_PAIRS_PER_WAVE], boff[GG_PAIRS_PER_WAVE];
    int mine = 0;
#pragma unroll
    for (int s = 0; s < GG_PAIRS_PER_WAVE; s++) {
        const int p = wave + GG_WAVES * s;
        int ti = 0, rem = p;
        while (ti < a.tiles && rem >= a.tiles - ti) {
            rem -= a.tiles - ti;
            ti++;
        }
        const bool live = p < a.pairs;
        aoff[s] = live ? ti * 16 : 0;
        boff[s] = live ? (ti + rem) * 16 : 0;
        if (live) mine = s + 1;
    }

    f64x4 acc[GG_PAIRS_PER_WAVE];
#pragma unroll
    for (int s = 0; s < GG_PAIRS_PER_WAVE; s++) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};

    // staged element e of a thread: slab row (e * GG_THREADS + tid) / 256, column (e * GG_THREADS + tid) % 256 -- a wave reads 64
    // consecutive floats of one row
    const int lc = tid & (GG_KMAX - 1), lr = tid >> 8;
    float pre[GG_LOADS];
#pragma unroll
    for (int e = 0; e < GG_LOADS; e++) pre[e] = lc < a.Kp ? gg_elem(a, row0 + (e * 2 + lr), lc) : 0.0f;

    const int frow = lane >> 4, fcol = lane & 15;
    for (int s0 = 0; s0 < nrow; s0 += GG_SLAB) {
        __syncthreads();   // the slab's readers of the last round are done
        if (lc < a.Kp) {
#pragma unroll
            for (int e = 0; e < GG_LOADS; e++) slab[(e * 2 + lr) * GG_PITCH + lc] = pre[e];
        }
        __syncthreads();
        if (s0 + GG_SLAB < nrow) {
#pragma unroll
            for (int e = 0; e < GG_LOADS; e++) pre[e] = lc < a.Kp ? gg_elem(a, row0 + s0 + GG_SLAB + (e * 2 + lr), lc) : 0.0f;
        }
        for (int k4 = 0; k4 < GG_SLAB / 4; k4++) {
            const float* r = slab + (k4 * 4 + frow) * GG_PITCH + fcol;
#pragma unroll
            for (int s = 0; s < GG_PAIRS_PER_WAVE; s++) {
                if (s < mine) {
                    const double ua = (double)r[aoff[s]];
                    const double ub = (double)r[boff[s]];
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, ub, acc[s], 0, 0, 0);
                }
            }
        }
    }

#pragma unroll
    for (int s = 0; s < GG_PAIRS_PER_WAVE; s++) {
        if (s < mine) {
            double* o = a.partial + ((size_t)blockIdx.x * a.pairs + (wave + GG_WAVES * s)) * 256 + lane;
            o[0] = acc[s][0]; o[64] = acc[s][1]; o[128] = acc[s][2]; o[192] = acc[s][3];
        }
    }
}

// The f64 16x16x4 result layout: register g of lane l holds tile element (row = (l >> 4) + 4 g, column = l & 15) -- not the map of the
// other MFMA shapes.  Row = the A operand's index (tile ti of G's rows), column = the B operand's (tile tj).
__global__ __launch_bounds__(GL_THREADS) void geometry_gram_finish_kernel(const double* partial, double* G, int chunks, int K, int Kp,
                                                                           int tiles, int pairs) {
    const int idx = blockIdx.x * GL_THREADS + threadIdx.x;
    if (idx >= Kp * Kp) return;
    const int i = idx / Kp, j = idx - i * Kp;
    if (i > j) return;   // written by the thread of (j, i)
    double sum = 0.0;
    if (j < K) {
        const int ti = i >> 4, tj = j >> 4, row = i & 15, col = j & 15;
        const int p = ti * tiles - ti * (ti - 1) / 2 + (tj - ti);
        const double* src = partial + (size_t)p * 256 + (row >> 2) * 64 + (row & 3) * 16 + col;
        for (int c = 0; c < chunks; c++) sum = sum + src[(size_t)c * pairs * 256];
    }
    G[(size_t)i * Kp + j] = sum;
    G[(size_t)j * Kp + i] = sum;
}

__global__ __launch_bounds__(GL_THREADS) void geometry_loss_face_kernel(const float* diff, const double* G, double* y, double* q, int K,
                                                                         int Kp) {
    __shared__ double d[GL_THREADS];
    __shared__ double t[GL_THREADS];
    const int b = blockIdx.x, k = threadIdx.x;
    d[k] = k < K ? (double)diff[(size_t)b * K + k] : 0.0;
    __syncthreads();
    double yk = 0.0;
    if (k < K) {
        const double* col = G + k;
        for (int j = 0; j < K; j++) yk = yk + col[(size_t)j * Kp] * d[j];
    }
    if (k < Kp) y[(size_t)b * Kp + k] = yk;
    t[k] = d[k] * yk;
    __syncthreads();
    if (k == 0) {
        double s = 0.0;
        for (int kk = 0; kk < K; kk++) s = s + t[kk];
        q[b] = s;
    }
}

__global__ __launch_bounds__(64) void geometry_loss_sum_kernel(const double* q, double* S, float* loss, int B, double denom) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; b++) s = s + q[b];
    *S = s;
    *loss = (float)(s / denom);
}

__global__ __launch_bounds__(GL_THREADS) void geometry_loss_backward_kernel(const float* grad_loss, const double* y, float* grad_diff,
                                                                             long long n, int K, int Kp, double two_over_denom) {
    const long long idx = (long long)blockIdx.x * GL_THREADS + threadIdx.x;
    if (idx >= n) return;
    const long long b = idx / K;
    const int k = (int)(idx - b * K);
    const double c = (double)grad_loss[0] * two_over_denom;
    grad_diff[idx] = (float)(c * y[(size_t)b * Kp + k]);
}

}  // namespace fr

// The sizes and the build's geometry, stated in ONE place: the size functions, the launchers and the test hook read them from here.
namespace {
struct GgGeom {
    int K, Kp, tiles, pairs, chunks;
    long long rows;
};
// K outside 1 .. 256 is not served
bool gg_served(int n_shape, int n_exp) {
    const long long K = (long long)n_shape + n_exp;
    return K >= 1 && K <= fr::GG_KMAX;
}
GgGeom gg_geom(int N, int n_shape, int n_exp) {
    GgGeom g;
    g.K = n_shape + n_exp;
    g.Kp = (g.K + 15) / 16 * 16;
    g.tiles = g.Kp / 16;
    g.pairs = g.tiles * (g.tiles + 1) / 2;
    g.rows = 3ll * N;
    g.chunks = (int)((g.rows + fr::GG_CHUNK - 1) / fr::GG_CHUNK);
    return g;
}
size_t gg_gram_bytes(const GgGeom& g) { return (size_t)g.Kp * g.Kp * sizeof(double); }
size_t gg_workspace_bytes(const GgGeom& g) { return (size_t)g.chunks * g.pairs * 256 * sizeof(double); }
size_t gg_state_bytes(const GgGeom& g, int B) { return ((size_t)B * g.Kp + (size_t)B + 1) * sizeof(double); }
double gg_denom(const GgGeom& g, int B) { return (double)g.rows * (double)B; }

// What the three launching entry points share, in the order all answer (steps 1 and 2 of the header's list): a negative size or
// N < 1 is FR_ERR_INVALID_ARG, then K outside 1 .. 256 is FR_ERR_UNSUPPORTED.  FR_OK = go on.
int gg_check_sizes(int B, int N, int n_shape, int n_exp) {
    if (B < 0 || N < 1 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if (!gg_served(n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    return FR_OK;
}
}  // namespace

extern "C" {

size_t fr_geometry_gram_bytes(int n_shape, int n_exp) {
    if (n_shape < 0 || n_exp < 0 || !gg_served(n_shape, n_exp)) return 0;
    return gg_gram_bytes(gg_geom(1, n_shape, n_exp));
}

size_t fr_geometry_gram_workspace_bytes(int N, int n_shape, int n_exp) {
    if (gg_check_sizes(0, N, n_shape, n_exp) != FR_OK) return 0;
    return gg_workspace_bytes(gg_geom(N, n_shape, n_exp));
}

size_t fr_geometry_loss_state_bytes(int B, int n_shape, int n_exp) {
    if (gg_check_sizes(B, 1, n_shape, n_exp) != FR_OK) return 0;
    return gg_state_bytes(gg_geom(1, n_shape, n_exp), B);
}

// test hook: out = {rows per chunk, chunks, Kp, tile pairs, workgroups of the chunk kernel, its static LDS bytes}; zeros for a shape
// the build refuses
void fr_debug_geometry_gram_geom(int N, int n_shape, int n_exp, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    if (gg_check_sizes(0, N, n_shape, n_exp) != FR_OK) return;
    const GgGeom g = gg_geom(N, n_shape, n_exp);
    out[0] = fr::GG_CHUNK; out[1] = g.chunks; out[2] = g.Kp; out[3] = g.pairs; out[4] = g.chunks;
    out[5] = (int)(fr::GG_SLAB * fr::GG_PITCH * sizeof(float));
}

int fr_geometry_gram_build(const float* pc_shape, const float* pc_exp, int N, int n_shape, int n_exp, void* gram, size_t gram_bytes,
                           void* workspace, size_t ws_bytes, void* stream) {
    const int rc = gg_check_sizes(0, N, n_shape, n_exp);
    if (rc != FR_OK) return rc;
    if ((n_shape > 0 && !pc_shape) || (n_exp > 0 && !pc_exp)) return FR_ERR_INVALID_ARG;
    const GgGeom g = gg_geom(N, n_shape, n_exp);
    if (!ws_ok(gram, gram_bytes, gg_gram_bytes(g), 16) || !ws_ok(workspace, ws_bytes, gg_workspace_bytes(g), 16))
        return FR_ERR_WORKSPACE;
    fr::GgArgs a{pc_shape, pc_exp, (double*)workspace, g.rows, n_shape, n_exp, g.Kp, g.tiles, g.pairs};
    hipLaunchKernelGGL(fr::geometry_gram_chunk_kernel, dim3((unsigned)g.chunks), dim3(fr::GG_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fr::geometry_gram_finish_kernel, dim3((unsigned)((g.Kp * g.Kp + fr::GL_THREADS - 1) / fr::GL_THREADS)),
                       dim3(fr::GL_THREADS), 0, (hipStream_t)stream, (const double*)workspace, (double*)gram, g.chunks, g.K, g.Kp,
                       g.tiles, g.pairs);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_geometry_loss_forward(const float* diff, const void* gram, int B, int N, int n_shape, int n_exp, float* loss, void* state,
                             size_t state_bytes, void* stream) {
    const int rc = gg_check_sizes(B, N, n_shape, n_exp);
    if (rc != FR_OK) return rc;
    if (B == 0) return FR_OK;
    if (!diff || !loss) return FR_ERR_INVALID_ARG;
    const GgGeom g = gg_geom(N, n_shape, n_exp);
    if (!ws_ok(gram, 1, 1, 16) || !ws_ok(state, state_bytes, gg_state_bytes(g, B), 16)) return FR_ERR_WORKSPACE;
    double* y = (double*)state;
    double* q = y + (size_t)B * g.Kp;
    hipLaunchKernelGGL(fr::geometry_loss_face_kernel, dim3((unsigned)B), dim3(fr::GL_THREADS), 0, (hipStream_t)stream, diff,
                       (const double*)gram, y, q, g.K, g.Kp);
    hipLaunchKernelGGL(fr::geometry_loss_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)q, q + B, loss, B,
                       gg_denom(g, B));
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_geometry_loss_backward(const float* grad_loss, const void* state, size_t state_bytes, int B, int N, int n_shape, int n_exp,
                              float* grad_diff, void* stream) {
    const int rc = gg_check_sizes(B, N, n_shape, n_exp);
    if (rc != FR_OK) return rc;
    if (B == 0) return FR_OK;
    if (!grad_loss || !grad_diff) return FR_ERR_INVALID_ARG;
    const GgGeom g = gg_geom(N, n_shape, n_exp);
    if (!ws_ok(state, state_bytes, gg_state_bytes(g, B), 16)) return FR_ERR_WORKSPACE;
    const long long n = (long long)B * g.K;
    hipLaunchKernelGGL(fr::geometry_loss_backward_kernel, dim3((unsigned)((n + fr::GL_THREADS - 1) / fr::GL_THREADS)),
                       dim3(fr::GL_THREADS), 0, (hipStream_t)stream, grad_loss, (const double*)state, grad_diff, n, g.K, g.Kp,
                       2.0 / gg_denom(g, B));
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
