// Landmark term (include/fr_hotpath.h, "landmarks"): the 3DMM decode, projection, comparison and gradient of K chosen vertices, from
// a compact image of their basis rows -- the dense basis is read once, by fr_landmark_basis_build, and never per step.
//
// Image (fp32, R3 = 3 K rows, row r = 3 k + c = coordinate c of landmark k, Kt = n_shape + n_exp):
//   part A  [Kt + 1][R3]   plane 0 the mean, plane 1 + j coefficient j: the forward's lane r walks the planes, coalesced over r
//   part B  [R3][Kt]       the same coefficients row-major: the backward's lane j walks the rows, coalesced over j
//
// One workgroup per face.  The landmarks are taken in chunks of LM_KC = 256 in ascending order; every sum over k is a sequential
// float64 sum from +0 that one lane carries from chunk to chunk, so the order is k ascending whatever K is.  All arithmetic is float64
// on the widened fp32 inputs, each product and sum rounded on its own (the file is built with -ffp-contract=off).
#include "fr_landmark_shared.h"

namespace fr {

struct LmBuildArgs {
    const float* mu;
    const float* pcs;
    const float* pce;
    const int* idx;
    float* out;
    int N, ns, ne, K;
};

__device__ __forceinline__ float lm_gather(const LmBuildArgs& a, int gr, int p) {
    const int k = gr / 3, c = gr - 3 * k;
    const int id = a.idx[k];
    if (id < 0 || id >= a.N) return 0.0f;
    const size_t row = (size_t)c * a.N + id;
    if (p == 0) return a.mu[row];
    const int j = p - 1;
    return j < a.ns ? a.pcs[row * a.ns + j] : a.pce[row * a.ne + (j - a.ns)];
}

__global__ __launch_bounds__(256) void lm_build_kernel(LmBuildArgs a) {
    const int Kt = a.ns + a.ne, R3 = 3 * a.K;
    const size_t nA = (size_t)(Kt + 1) * R3, total = nA + (size_t)R3 * Kt;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    if (e < nA) {
        const int p = (int)(e / R3), gr = (int)(e - (size_t)p * R3);
        a.out[e] = lm_gather(a, gr, p);
    } else {
        const size_t e2 = e - nA;
        const int gr = (int)(e2 / Kt), j = (int)(e2 - (size_t)gr * Kt);
        a.out[e] = lm_gather(a, gr, 1 + j);
    }
}

__global__ __launch_bounds__(768) void lm_forward_kernel(LmArgs a) {
    __shared__ float a_s[LM_MAX_COEF];
    __shared__ LmPose P;
    __shared__ double v_s[3 * LM_KC];
    __shared__ double term_s[LM_KC];
    const int b = blockIdx.x, tid = threadIdx.x;
    lm_prologue(a, b, a_s, P);
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)P.R[i];
    const double f = (double)P.f;
    double sse = 0.0;
    for (int k0 = 0; k0 < a.K; k0 += LM_KC) {
        const int kc = min(LM_KC, a.K - k0);
        lm_chunk_v(a, k0, 3 * kc, a_s, v_s);
        __syncthreads();
        for (int kl = tid; kl < kc; kl += blockDim.x) {
            const int k = k0 + kl;
            const double v0 = v_s[3 * kl], v1 = v_s[3 * kl + 1], v2 = v_s[3 * kl + 2];
            const double x = f * ((R[0] * v0 + R[1] * v1) + R[2] * v2) + (double)P.t[0];
            const double q1 = f * ((R[3] * v0 + R[4] * v1) + R[5] * v2) + (double)P.t[1];
            const double z = f * ((R[6] * v0 + R[7] * v1) + R[8] * v2) + (double)P.t[2];
            const double y = (a.im - q1) - 1.0;
            float* o = a.points + (size_t)b * 3 * a.K + k;
            o[0] = (float)x;
            o[a.K] = (float)y;
            o[2 * (size_t)a.K] = (float)z;
            if (a.target) {
                const double w = lm_weight(a, b, k);
                double term = 0.0;
                if (w != 0.0) {   // a landmark of weight 0 is skipped: its target is not read
                    const float* tg = a.target + ((size_t)b * a.K + k) * 2;
                    const double dx = x - (double)tg[0], dy = y - (double)tg[1];
                    term = w * (dx * dx + dy * dy);
                }
                term_s[kl] = term;
            }
        }
        __syncthreads();
        if (a.target && tid == 0)
            for (int kl = 0; kl < kc; kl++) sse = sse + term_s[kl];
        __syncthreads();
    }
    if (a.target && tid == 0) a.sse[b] = sse;
}

__global__ __launch_bounds__(768) void lm_backward_kernel(LmArgs a) {
    __shared__ float a_s[LM_MAX_COEF];
    __shared__ LmPose P;
    __shared__ double v_s[3 * LM_KC];
    __shared__ double dq_s[3 * LM_KC];
    __shared__ double rt_s[3 * LM_KC];   // R^T dq
    __shared__ double ft_s[LM_KC];       // dq . (R v)
    __shared__ double G_s[9];
    const int b = blockIdx.x, tid = threadIdx.x, nd = 7 + a.Kt;
    lm_prologue(a, b, a_s, P);
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)P.R[i];
    const double f = (double)P.f;
    const bool with_sse = a.grad_sse && a.target;
    const double gs = with_sse ? a.grad_sse[b] : 0.0;
    const int Kt = a.Kt, R3 = 3 * a.K;
    const float* Bm = a.lbasis + (size_t)(Kt + 1) * R3;
    double acc = 0.0;   // this lane's sum: coefficient tid, or pose sum tid - Kt (the launcher gives the block >= Kt + 13 lanes)
    for (int k0 = 0; k0 < a.K; k0 += LM_KC) {
        const int kc = min(LM_KC, a.K - k0);
        lm_chunk_v(a, k0, 3 * kc, a_s, v_s);
        __syncthreads();
        for (int kl = tid; kl < kc; kl += blockDim.x) {
            const int k = k0 + kl;
            const double v0 = v_s[3 * kl], v1 = v_s[3 * kl + 1], v2 = v_s[3 * kl + 2];
            const double rv0 = (R[0] * v0 + R[1] * v1) + R[2] * v2;
            const double rv1 = (R[3] * v0 + R[4] * v1) + R[5] * v2;
            const double rv2 = (R[6] * v0 + R[7] * v1) + R[8] * v2;
            double gx = 0.0, gy = 0.0, gz = 0.0;
            if (a.grad_points) {
                const float* g = a.grad_points + (size_t)b * 3 * a.K + k;
                gx = (double)g[0];
                gy = (double)g[a.K];
                gz = (double)g[2 * (size_t)a.K];
            }
            if (with_sse) {
                const double w = lm_weight(a, b, k);
                if (w != 0.0) {
                    const float* tg = a.target + ((size_t)b * a.K + k) * 2;
                    const double x = f * rv0 + (double)P.t[0];
                    const double y = (a.im - (f * rv1 + (double)P.t[1])) - 1.0;
                    const double s = gs * (2.0 * w);
                    gx = gx + s * (x - (double)tg[0]);
                    gy = gy + s * (y - (double)tg[1]);
                }
            }
            const double d0 = gx, d1 = -gy, d2 = gz;
            dq_s[3 * kl] = d0;
            dq_s[3 * kl + 1] = d1;
            dq_s[3 * kl + 2] = d2;
            ft_s[kl] = (d0 * rv0 + d1 * rv1) + d2 * rv2;
            rt_s[3 * kl] = (R[0] * d0 + R[3] * d1) + R[6] * d2;
            rt_s[3 * kl + 1] = (R[1] * d0 + R[4] * d1) + R[7] * d2;
            rt_s[3 * kl + 2] = (R[2] * d0 + R[5] * d1) + R[8] * d2;
        }
        __syncthreads();
        if (tid < Kt) {
            const float* col = Bm + (size_t)3 * k0 * Kt + tid;
            const int rows = 3 * kc;
#pragma unroll 8
            for (int r = 0; r < rows; r++) acc = acc + rt_s[r] * (double)col[(size_t)r * Kt];
        } else if (tid < Kt + 3) {
            const int i = tid - Kt;
            for (int kl = 0; kl < kc; kl++) acc = acc + dq_s[3 * kl + i];
        } else if (tid == Kt + 3) {
            for (int kl = 0; kl < kc; kl++) acc = acc + ft_s[kl];
        } else if (tid < Kt + LM_POSE_SUMS) {
            const int ij = tid - Kt - 4, i = ij / 3, j = ij - 3 * i;
            for (int kl = 0; kl < kc; kl++) acc = acc + dq_s[3 * kl + i] * v_s[3 * kl + j];
        }
        __syncthreads();
    }
    float* gp = a.grad_params + (size_t)b * nd;
    if (tid < Kt) gp[7 + tid] = (float)(f * acc);
    else if (tid < Kt + 3) gp[3 + (tid - Kt)] = (float)acc;
    else if (tid == Kt + 3) gp[6] = (float)acc;
    else if (tid < Kt + LM_POSE_SUMS) G_s[tid - Kt - 4] = f * acc;
    __syncthreads();
    if (tid < 3) {
        float g = 0.0f;
        if (a.pose_grad && !a.R_override) {
            const double sp = P.sc[0], cp = P.sc[1], sy = P.sc[2], cy = P.sc[3], st = P.sc[4], ct = P.sc[5];
            double Rp[9] = {1, 0, 0, 0, cp, sp, 0, -sp, cp};
            double Ry[9] = {cy, 0, -sy, 0, 1, 0, sy, 0, cy};
            double Rr[9] = {ct, st, 0, -st, ct, 0, 0, 0, 1};
            const double dRp[9] = {0, 0, 0, 0, -sp, cp, 0, -cp, -sp};
            const double dRy[9] = {-sy, 0, -cy, 0, 0, 0, cy, 0, -sy};
            const double dRr[9] = {-st, ct, 0, -ct, -st, 0, 0, 0, 0};
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) Rp[i] = dRp[i];
            } else if (tid == 1) {
#pragma unroll
                for (int i = 0; i < 9; i++) Ry[i] = dRy[i];
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) Rr[i] = dRr[i];
            }
            double PY[9], D[9];
            mat3_mul(Rp, Ry, PY);
            mat3_mul(PY, Rr, D);
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 9; i++) s = s + G_s[i] * D[i];
            g = (float)s;
        }
        gp[tid] = g;
    } else if (tid < 12 && a.pose_grad && a.R_override) {
        a.grad_R[(size_t)b * 9 + (tid - 3)] = (float)G_s[tid - 3];
    }
}

inline int lm_block(int lanes) {
    int n = (lanes + 63) / 64 * 64;
    return n < 64 ? 64 : (n > 768 ? 768 : n);
}

}  // namespace fr

// ---- C ABI (include/fr_hotpath.h) ---------------------------------------------------------------------------------------------
extern "C" {

size_t fr_landmark_basis_bytes(int K, int n_shape, int n_exp) {
    if (n_shape < 0 || n_exp < 0 || !fr::lm_sizes_ok(K, n_shape, n_exp)) return 0;
    return fr::lm_basis_floats(K, n_shape + n_exp) * sizeof(float);
}

int fr_landmark_basis_build(const float* mu, const float* pc_shape, const float* pc_exp, const int* idx, int N, int n_shape, int n_exp,
                            int K, void* lbasis, size_t bytes, void* stream) {
    using namespace fr;
    if (N < 0 || n_shape < 0 || n_exp < 0 || K < 0) return FR_ERR_INVALID_ARG;
    if (K == 0) return FR_OK;
    if (!idx || (N > 0 && (!mu || (n_shape > 0 && !pc_shape) || (n_exp > 0 && !pc_exp)))) return FR_ERR_INVALID_ARG;
    if (!lm_sizes_ok(K, n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    const size_t nfl = lm_basis_floats(K, n_shape + n_exp);
    if (!ws_ok(lbasis, bytes, nfl * sizeof(float), 16)) return FR_ERR_WORKSPACE;
    LmBuildArgs a;
    a.mu = mu; a.pcs = pc_shape; a.pce = pc_exp; a.idx = idx; a.out = reinterpret_cast<float*>(lbasis);
    a.N = N; a.ns = n_shape; a.ne = n_exp; a.K = K;
    hipLaunchKernelGGL(lm_build_kernel, dim3((unsigned)((nfl + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_landmark_forward(const float* params, const void* lbasis, size_t lbasis_bytes, const float* R_override, const float* target,
                        const float* weight, int weight_batch, int B, int K, int n_shape, int n_exp, float im_size, float* points,
                        double* sse, void* stream) {
    using namespace fr;
    if (B < 0 || K < 0 || n_shape < 0 || n_exp < 0 || (weight_batch != 0 && weight_batch != 1)) return FR_ERR_INVALID_ARG;
    if (B == 0 || K == 0) return FR_OK;
    if (!params || !points || (target && !sse)) return FR_ERR_INVALID_ARG;
    if (!lm_sizes_ok(K, n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    if (!ws_ok(lbasis, lbasis_bytes, lm_basis_floats(K, n_shape + n_exp) * sizeof(float), 16)) return FR_ERR_WORKSPACE;
    LmArgs a = {};
    a.params = params; a.lbasis = reinterpret_cast<const float*>(lbasis); a.R_override = R_override; a.target = target;
    a.weight = weight; a.points = points; a.sse = sse;
    a.K = K; a.Kt = n_shape + n_exp; a.weight_batch = weight_batch; a.im = (double)im_size;
    hipLaunchKernelGGL(lm_forward_kernel, dim3((unsigned)B), dim3(lm_block(3 * (K < LM_KC ? K : LM_KC))), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_landmark_backward(const float* grad_points, const double* grad_sse, const float* params, const void* lbasis,
                         size_t lbasis_bytes, const float* R_override, const float* target, const float* weight, int weight_batch,
                         int B, int K, int n_shape, int n_exp, float im_size, float* grad_params, float* grad_R, int pose_grad,
                         void* stream) {
    using namespace fr;
    if (B < 0 || K < 0 || n_shape < 0 || n_exp < 0) return FR_ERR_INVALID_ARG;
    if ((weight_batch != 0 && weight_batch != 1) || (pose_grad != 0 && pose_grad != 1)) return FR_ERR_INVALID_ARG;
    if (B == 0 || K == 0) return FR_OK;
    if (!params || !grad_params || (!grad_points && !grad_sse) || (grad_sse && !target)) return FR_ERR_INVALID_ARG;
    if (pose_grad && R_override && !grad_R) return FR_ERR_INVALID_ARG;
    if (!lm_sizes_ok(K, n_shape, n_exp)) return FR_ERR_UNSUPPORTED;
    if (!ws_ok(lbasis, lbasis_bytes, lm_basis_floats(K, n_shape + n_exp) * sizeof(float), 16)) return FR_ERR_WORKSPACE;
    LmArgs a = {};
    a.params = params; a.lbasis = reinterpret_cast<const float*>(lbasis); a.R_override = R_override; a.target = target;
    a.weight = weight; a.grad_points = grad_points; a.grad_sse = grad_sse; a.grad_params = grad_params; a.grad_R = grad_R;
    a.K = K; a.Kt = n_shape + n_exp; a.weight_batch = weight_batch; a.pose_grad = pose_grad; a.im = (double)im_size;
    const int rows = 3 * (K < LM_KC ? K : LM_KC), sums = a.Kt + LM_POSE_SUMS;
    hipLaunchKernelGGL(lm_backward_kernel, dim3((unsigned)B), dim3(lm_block(rows > sums ? rows : sums)), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
