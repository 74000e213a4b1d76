// What the landmark kernels share (fr_landmark.hip, fr_landmark_solve.hip): the limits, the image size, the face prologue, the
// decode chain of a chunk of landmarks and the weight lookup.  One definition, so that both files form v, R and w with the same bits.
#pragma once
#include "fr_common.h"
#include "fr_decode_shared.h"

namespace fr {

constexpr int LM_KC = 256;          // landmarks per chunk
constexpr int LM_MAX_COEF = 256;    // n_shape + n_exp
constexpr int LM_MAX_K = 1024;
constexpr int LM_POSE_SUMS = 13;    // t3d (3), f (1), G (9)

__host__ __device__ inline size_t lm_basis_floats(int K, int Kt) { return (size_t)3 * K * (2 * (size_t)Kt + 1); }
inline bool lm_sizes_ok(int K, int n_shape, int n_exp) {
    return K >= 1 && K <= LM_MAX_K && (long long)n_shape + n_exp <= LM_MAX_COEF;
}

struct LmArgs {
    const float* params;      // [B, 7 + Kt]
    const float* lbasis;
    const float* R_override;  // [B,9] or null
    const float* target;      // [B,K,2] or null
    const float* weight;      // null, [K] or [B,K]
    const float* grad_points; // [B,3,K] or null          (backward)
    const double* grad_sse;   // [B] or null              (backward)
    float* points;            // [B,3,K]                  (forward)
    double* sse;              // [B]                      (forward)
    float* grad_params;       // [B, 7 + Kt]              (backward)
    float* grad_R;            // [B,9]                    (backward)
    int K, Kt, weight_batch, pose_grad;
    double im;
};

struct LmPose {
    double sc[6];   // sin, cos of phi, gamma, theta
    float R[9];
    float f, t[3];
};

// coefficients and pose of face b into LDS; ends with a barrier
__device__ __forceinline__ void lm_prologue(const LmArgs& a, int b, float* a_s, LmPose& P) {
    const int tid = threadIdx.x, nd = 7 + a.Kt;
    const float* pr = a.params + (size_t)b * nd;
    for (int j = tid; j < a.Kt; j += blockDim.x) a_s[j] = pr[7 + j];
    if (tid < 3 && !a.R_override) {
        double sn, cs;
        sincos((double)pr[tid], &sn, &cs);
        P.sc[2 * tid] = sn;
        P.sc[2 * tid + 1] = cs;
    }
    __syncthreads();
    if (tid == 0) {
        if (a.R_override) {
#pragma unroll
            for (int i = 0; i < 9; i++) P.R[i] = a.R_override[(size_t)b * 9 + i];
        } else {
            rotation_from_sincos(P.sc[0], P.sc[1], P.sc[2], P.sc[3], P.sc[4], P.sc[5], P.R);
        }
        P.f = pr[6];
        P.t[0] = pr[3];
        P.t[1] = pr[4];
        P.t[2] = pr[5];
    }
    __syncthreads();
}

// v of the chunk's rows: v = mu, then + a_j U_j for j ascending.  No barrier.
__device__ __forceinline__ void lm_chunk_v(const LmArgs& a, int k0, int rows, const float* a_s, double* v_s) {
    const size_t R3 = (size_t)3 * a.K;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float* A = a.lbasis + (size_t)3 * k0 + r;
        double v = (double)A[0];
#pragma unroll 8
        for (int j = 0; j < a.Kt; j++) v = v + (double)a_s[j] * (double)A[(size_t)(1 + j) * R3];
        v_s[r] = v;
    }
}

__device__ __forceinline__ double lm_weight(const LmArgs& a, int b, int k) {
    if (!a.weight) return 1.0;
    return (double)a.weight[a.weight_batch ? (size_t)b * a.K + k : (size_t)k];
}

}  // namespace fr
