// Contour landmarks (include/fr_hotpath.h, "contour landmarks"): per face and per line of M candidate vertices, the one candidate
// the line's 2D point is held to -- the nearest to the point, or the extreme along a direction -- written as the per-face weight
// and target that fr_landmark_forward / _backward / fr_landmark_solve_step then run over with weight_batch = 1.
//
// The compact image is fr_landmark_basis_build's, over Kf fixed ids followed by C lines of M ids: candidate (c, m) is landmark
// k = Kf + c M + m.  One workgroup per face; the landmarks go through LDS in the forward's chunks of LM_KC = 256 (chunk boundaries at
// multiples of 256 of k; what lies below Kf is not decoded).  v, R, x and y are the forward's, by the shared prologue and chain
// (fr_landmark_shared.h) and the same expressions, in float64 before any fp32 rounding.  Lane c owns line c: it walks the line's
// candidates of the chunk in ascending m with a strict comparison and carries (best, m, x, y) from chunk to chunk.  No atomics, no
// workspace.  Built with -ffp-contract=off: every product and sum is rounded on its own.
#include "fr_landmark_shared.h"

namespace fr {

constexpr int LMC_MAX_LINES = 256;

struct LmContourArgs {
    const float* fixed_target;   // [B,Kf,2] or null
    const float* fixed_weight;   // null, [Kf] or [B,Kf]
    const float* line_target;    // [B,C,2] or null
    const float* line_weight;    // null, [C] or [B,C]
    const float* line_dir;       // [C,2] or null
    int* sel;                    // [B,C]
    float* line_points;          // [B,C,2]
    float* target;               // [B,K,2] or null
    float* weight;               // [B,K] or null
    int Kf, C, M, rule, fixed_weight_batch, line_weight_batch;
};

__device__ __forceinline__ float lmc_line_weight(const LmContourArgs& c, int b, int line) {
    if (!c.line_weight) return 1.0f;
    return c.line_weight[c.line_weight_batch ? (size_t)b * c.C + line : (size_t)line];
}

__global__ __launch_bounds__(768) void lm_contour_select_kernel(LmArgs a, LmContourArgs c) {
    __shared__ float a_s[LM_MAX_COEF];
    __shared__ LmPose P;
    __shared__ double v_s[3 * LM_KC];
    __shared__ double x_s[LM_KC];
    __shared__ double y_s[LM_KC];
    __shared__ double score_s[LM_KC];
    __shared__ int sel_s[LMC_MAX_LINES];
    __shared__ int looked_s[LMC_MAX_LINES];      // line c is looked at: its weight is not 0
    __shared__ float lt_s[2 * LMC_MAX_LINES];    // rule 0: the target of a line that is looked at
    const int b = blockIdx.x, tid = threadIdx.x;
    lm_prologue(a, b, a_s, P);
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)P.R[i];
    const double f = (double)P.f;
    // lane `tid` owns line `tid` (the launcher gives the block at least C lanes)
    const bool owner = tid < c.C;
    const float lw = owner ? lmc_line_weight(c, b, tid) : 0.0f;
    const bool looked = owner && lw != 0.0f;   // a line of weight 0 is not looked at: its target is not read
    if (owner) {   // published once per face; the candidate lanes read it behind the first chunk's barrier
        looked_s[tid] = looked;
        if (looked && c.rule == 0) {
            const float* tg = c.line_target + ((size_t)b * c.C + tid) * 2;
            lt_s[2 * tid] = tg[0];
            lt_s[2 * tid + 1] = tg[1];
        }
    }
    double best = c.rule == 0 ? (double)INFINITY : -(double)INFINITY;
    double bx = 0.0, by = 0.0;
    int bm = -1;
    for (int k0 = c.Kf / LM_KC * LM_KC; k0 < a.K; k0 += LM_KC) {
        const int kc = min(LM_KC, a.K - k0);
        const int skip = max(c.Kf - k0, 0);   // landmarks of the chunk that belong to the fixed part
        lm_chunk_v(a, k0 + skip, 3 * (kc - skip), a_s, v_s + 3 * skip);
        __syncthreads();
        for (int kl = skip + tid; kl < kc; kl += blockDim.x) {
            const int line = (k0 + kl - c.Kf) / c.M;
            if (!looked_s[line]) continue;   // nobody reads this candidate's score
            const double v0 = v_s[3 * kl], v1 = v_s[3 * kl + 1], v2 = v_s[3 * kl + 2];
            const double x = f * ((R[0] * v0 + R[1] * v1) + R[2] * v2) + (double)P.t[0];
            const double q1 = f * ((R[3] * v0 + R[4] * v1) + R[5] * v2) + (double)P.t[1];
            const double y = (a.im - q1) - 1.0;
            double s;
            if (c.rule == 0) {
                const double dx = x - (double)lt_s[2 * line], dy = y - (double)lt_s[2 * line + 1];
                s = dx * dx + dy * dy;
            } else {
                s = (double)c.line_dir[2 * line] * x + (double)c.line_dir[2 * line + 1] * y;
            }
            x_s[kl] = x;
            y_s[kl] = y;
            score_s[kl] = s;
        }
        __syncthreads();
        if (looked) {
            const int first = c.Kf + tid * c.M;                      // the line's landmarks are [first, first + M)
            const int lo = max(first, k0 + skip), hi = min(first + c.M, k0 + kc);
            for (int k = lo; k < hi; k++) {
                const double s = score_s[k - k0];
                if (c.rule == 0 ? s < best : s > best) {
                    best = s;
                    bm = k - first;
                    bx = x_s[k - k0];
                    by = y_s[k - k0];
                }
            }
        }
        __syncthreads();
    }
    if (owner) {
        sel_s[tid] = bm;
        c.sel[(size_t)b * c.C + tid] = bm;
        float* lp = c.line_points + ((size_t)b * c.C + tid) * 2;
        lp[0] = bm >= 0 ? (float)bx : 0.0f;
        lp[1] = bm >= 0 ? (float)by : 0.0f;
    }
    __syncthreads();
    if (c.weight) {
        float* w = c.weight + (size_t)b * a.K;
        for (int k = tid; k < a.K; k += blockDim.x) {
            float o;
            if (k < c.Kf) {
                o = c.fixed_weight ? c.fixed_weight[c.fixed_weight_batch ? (size_t)b * c.Kf + k : (size_t)k] : 1.0f;
            } else {
                const int line = (k - c.Kf) / c.M, m = (k - c.Kf) - line * c.M;
                o = m == sel_s[line] ? lmc_line_weight(c, b, line) : 0.0f;
            }
            w[k] = o;
        }
    }
    if (c.target) {
        // bit copies: the words are moved as integers, so that a NaN keeps its payload
        unsigned* t = reinterpret_cast<unsigned*>(c.target) + (size_t)b * a.K * 2;
        const unsigned* ft = reinterpret_cast<const unsigned*>(c.fixed_target) + (size_t)b * c.Kf * 2;
        const unsigned* lt = reinterpret_cast<const unsigned*>(c.line_target) + (size_t)b * c.C * 2;
        for (int e = tid; e < 2 * a.K; e += blockDim.x) {
            const int k = e >> 1, xy = e & 1;
            t[e] = k < c.Kf ? ft[e] : lt[2 * ((k - c.Kf) / c.M) + xy];
        }
    }
}

}  // namespace fr

// ---- C ABI (include/fr_hotpath.h) ---------------------------------------------------------------------------------------------
extern "C" {

int fr_landmark_contour_select(const float* params, const void* lbasis, size_t lbasis_bytes, const float* R_override,
                               const float* fixed_target, const float* fixed_weight, int fixed_weight_batch, const float* line_target,
                               const float* line_weight, int line_weight_batch, const float* line_dir, int rule, int B, int Kf, int C,
                               int M, int n_shape, int n_exp, float im_size, int* sel, float* line_points, float* target, float* weight,
                               void* stream) {
    using namespace fr;
    if (B < 0 || Kf < 0 || C < 0 || M < 0 || n_shape < 0 || n_exp < 0 || (rule != 0 && rule != 1)) return FR_ERR_INVALID_ARG;
    if ((fixed_weight_batch != 0 && fixed_weight_batch != 1) || (line_weight_batch != 0 && line_weight_batch != 1))
        return FR_ERR_INVALID_ARG;
    if (B == 0 || C == 0) return FR_OK;
    if (!params || !sel || !line_points) return FR_ERR_INVALID_ARG;
    if ((rule == 0 && !line_target) || (rule == 1 && !line_dir)) return FR_ERR_INVALID_ARG;
    if (target && (!line_target || (Kf > 0 && !fixed_target))) return FR_ERR_INVALID_ARG;
    const long long K64 = (long long)Kf + (long long)C * M;
    if (M < 1 || C > LMC_MAX_LINES || K64 > LM_MAX_K || !lm_sizes_ok((int)K64, n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    const int K = (int)K64;
    if (!ws_ok(lbasis, lbasis_bytes, lm_basis_floats(K, n_shape + n_exp) * sizeof(float), 16)) return FR_ERR_WORKSPACE;
    LmArgs a = {};
    a.params = params; a.lbasis = reinterpret_cast<const float*>(lbasis); a.R_override = R_override;
    a.K = K; a.Kt = n_shape + n_exp; a.im = (double)im_size;
    LmContourArgs c = {};
    c.fixed_target = fixed_target; c.fixed_weight = fixed_weight; c.line_target = line_target; c.line_weight = line_weight;
    c.line_dir = line_dir; c.sel = sel; c.line_points = line_points; c.target = target; c.weight = weight;
    c.Kf = Kf; c.C = C; c.M = M; c.rule = rule; c.fixed_weight_batch = fixed_weight_batch; c.line_weight_batch = line_weight_batch;
    const int rows = 3 * (K < LM_KC ? K : LM_KC);
    int block = (rows > C ? rows : C) + 63;
    block = block / 64 * 64;
    if (block > 768) block = 768;
    hipLaunchKernelGGL(lm_contour_select_kernel, dim3((unsigned)B), dim3(block), 0, (hipStream_t)stream, a, c);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
