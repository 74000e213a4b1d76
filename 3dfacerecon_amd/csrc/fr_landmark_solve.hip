// Landmark solver (include/fr_hotpath.h, "landmark solver"): one damped Gauss-Newton step of the landmark term per face -- the
// residuals and their Jacobian in the fitted columns, H = J^T W J + diag(ridge), g = J^T W r + ridge (a - center), the Marquardt
// scaling D = diag(J^T W J), and (H + damp D) delta = -g by Cholesky, in one launch.
//
// One workgroup per face, v, R and w formed by the forward's own code (fr_landmark_shared.h).  The unknowns are the fitted pose
// columns in parameter order, then -- with fit_coef -- the Kt coefficients.
//   landmarks      v of 256 landmarks at a time (the forward's chunk), then sub-chunks: a lane per landmark forms the residual pair,
//                  the F term and the six pose columns of its two Jacobian rows (row 2 k the x row, 2 k + 1 the y row); a landmark
//                  of weight 0 leaves exact zeros and reads no target.
//   chains         every sum that touches a pose column, g and D: one lane each, a sequential float64 sum from +0 over the rows
//                  ascending that the lane carries from sub-chunk to sub-chunk; the term of (row, i, j), i >= j, is
//                  (w J[row][i]) J[row][j], that of g_i is (w J[row][i]) r[row].
//   coefficients   fit_coef only: sub-chunks of 8 landmarks = 16 rows = four k-steps of v_mfma_f64_16x16x4_f64.  The rows' coefficient
//                  columns f (R_0 . U_kj), -(f (R_1 . U_kj)) are staged in LDS (pitch 272 float64, pad columns and pad rows +0); the
//                  tile pairs ti >= tj of the lower triangle are dealt to the 8 waves round robin (pair p to wave p % 8) and stay
//                  in registers over the whole face: operand A the staged value, operand B the staged value times the row's weight.
//                  Sub-chunks ascending, k-steps ascending: the bits are a function of (K, Kt) and the inputs alone.
//   system         the packed lower triangle (row-major, element (i, j) at i (i + 1) / 2 + j) with the right-hand side -g as row P,
//                  and a second packed copy of H for the prediction: in the workspace with fit_coef (220 KB a face at P = 234 is
//                  more than the LDS), in LDS without.
//   factorisation  right-looking, column c ascending: the pivot d = A_cc must be positive and finite; l = sqrt(d); rows c + 1 .. P
//                  of the column are divided by l; then A_ij = A_ij - L_ic L_jc over the trailing triangle, row P included, with
//                  block barriers between (a wave takes rows c + 1 + wave, + waves, ...; its lanes the columns j).
//                  Measured and not adopted (tools/landmark_solve_probe.py, 64 faces, P = 234, 1,515 us as it stands): 16 rows' loads
//                  in flight per lane before the first is used, with the next column handed on in LDS: 2,095 us; the row-serial
//                  update with that LDS column, an LDS-only first barrier and a prefetched substitution: 1,654 us.  Element (i, j) therefore sees its subtractions in c ascending order, and row P ends as
//                  y = L^-1 (-g): the forward substitution costs nothing.
//   substitution   c descending: delta_c = y_c / L_cc, then y_j = y_j - L_cj delta_c for j < c.
//   prediction     q_i = sum_j H_ij delta_j (j ascending), e_i = delta_i (2 g_i + q_i), cost_1 = F + sum_i e_i (i ascending).
// All float64, each product and sum rounded on its own (-ffp-contract=off); the MFMA is the one fused operation.  No atomics.
#include "fr_landmark_shared.h"
#include <float.h>

namespace fr {

constexpr int LS_POSE = 6;                        // pose slots: phi, gamma, theta, tx, ty, f (tz has no column)
constexpr int LS_MAX_P = LS_POSE + LM_MAX_COEF;
constexpr int LS_SUB = 8;                         // landmarks per MFMA sub-chunk
constexpr int LS_PITCH = 272;                     // float64 per staged row
constexpr int LS_BLOCK = 512;                      // 2 waves per SIMD: 256 registers a lane, the 17 accumulator tiles fit
constexpr int LS_WAVES = LS_BLOCK / 64;
constexpr int LS_PAIRS = 17;                      // tile pairs per wave: 136 pairs of 16 tiles over 8 waves
constexpr int LS_POSE_LANES = 27;                 // 21 pose-pose sums (c >= c'), then 6 gradient sums
typedef double ls_f64x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int ls_tri(int n) { return n * (n + 1) / 2; }          // (n <= 263: 32 bits are plenty)
__host__ __device__ inline int ls_at(int i, int j) { return i * (i + 1) / 2 + j; }
// float64 per face: the augmented triangle (rows 0 .. Pmax, row Pmax the right-hand side), then the copy of H; Pmax = 6 + Kt
__host__ __device__ inline size_t ls_face_doubles(int Kt) {
    const int Pm = LS_POSE + Kt;
    return ((size_t)2 * ls_tri(Pm) + Pm + 1) & ~(size_t)1;
}

struct LsArgs {
    LmArgs lm;
    const float* ridge;
    const float* center;
    const double* damp;
    double* delta;   // [B, 7 + Kt]
    double* cost;    // [B, 2]
    int* ok;         // [B]
    double* ws;
    int pose_mask;
};

template <bool COEF>
__global__ __launch_bounds__(LS_BLOCK) void lm_solve_kernel(LsArgs s) {
    constexpr int SUB = COEF ? LS_SUB : LM_KC;
    constexpr int MAXP = COEF ? LS_MAX_P : LS_POSE;
    __shared__ float a_s[LM_MAX_COEF];
    __shared__ LmPose P;
    __shared__ double dR_s[3][6];                 // rows 0 and 1 of dR_phi, dR_gamma, dR_theta
    __shared__ double v_s[3 * LM_KC];
    __shared__ double jp_s[2 * SUB][LS_POSE];
    __shared__ double r_s[2 * SUB];
    __shared__ double w_s[SUB];
    __shared__ double term_s[SUB];
    __shared__ double jc_s[COEF ? 2 * LS_SUB * LS_PITCH : 1];
    __shared__ double D_s[MAXP], g_s[MAXP], y_s[MAXP], d_s[MAXP], diag_s[MAXP], e_s[MAXP], col_s[MAXP + 1];
    __shared__ double small_s[2 * (LS_POSE * (LS_POSE + 1) / 2) + LS_POSE];
    __shared__ double F_s[2];
    __shared__ int bad_s;
    __shared__ int pair_s[COEF ? LS_WAVES * LS_PAIRS : 1];   // tile pair p: 16 ti | 16 tj << 16
    const LmArgs& a = s.lm;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: the tile offsets below stay in scalar registers
    const int Kt = a.Kt, nd = 7 + Kt;
    lm_prologue(a, b, a_s, P);
    if (tid < 3) {
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
        double PY[9], Dm[9];
        mat3_mul(Rp, Ry, PY);
        mat3_mul(PY, Rr, Dm);
#pragma unroll
        for (int i = 0; i < 6; i++) dR_s[tid][i] = Dm[i];
    }
    if (tid == 0) bad_s = 0;
    __syncthreads();
    double R[6];
#pragma unroll
    for (int i = 0; i < 6; i++) R[i] = (double)P.R[i];
    const double f = (double)P.f, t0 = (double)P.t[0], t1 = (double)P.t[1];

    // the unknowns: pidx[slot] = the index of a fitted pose column, or -1
    int pidx[LS_POSE], np = 0;
#pragma unroll
    for (int c = 0; c < LS_POSE; c++) {
        const int bit = c < 5 ? c : 6;
        pidx[c] = ((s.pose_mask >> bit) & 1) ? np++ : -1;
    }
    const int Pn = np + (COEF ? Kt : 0);

    // which sum this lane carries
    const int pl = tid - (COEF ? Kt : 0);          // pose lane 0 .. 26, or outside
    int pc = 0, pc2 = 0;
    if (pl >= 0 && pl < 21) {
        while (ls_tri(pc + 1) <= pl) pc++;
        pc2 = pl - ls_tri(pc);
    } else if (pl >= 21 && pl < LS_POSE_LANES) {
        pc = pl - 21;
    }
    double pacc = 0.0, sse = 0.0;
    double accP[LS_POSE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, accg = 0.0, accD = 0.0;
    // this wave's tile pairs (COEF)
    const int T = (Kt + 15) / 16, npairs = T * (T + 1) / 2;
    int mine = 0;
    ls_f64x4 macc[LS_PAIRS];
    if (COEF) {
        if (tid < LS_WAVES * LS_PAIRS) {
            int ti = 0;
            while ((ti + 1) * (ti + 2) / 2 <= tid) ti++;
            pair_s[tid] = (16 * ti) | ((16 * (tid - ti * (ti + 1) / 2)) << 16);
        }
#pragma unroll
        for (int q = 0; q < LS_PAIRS; q++) {
            if (wave + LS_WAVES * q < npairs) mine = q + 1;
            macc[q] = ls_f64x4{0.0, 0.0, 0.0, 0.0};
        }
    }
    const float* partB = a.lbasis + (size_t)(Kt + 1) * 3 * a.K;

    for (int k0 = 0; k0 < a.K; k0 += LM_KC) {
        const int kc = min(LM_KC, a.K - k0);
        lm_chunk_v(a, k0, 3 * kc, a_s, v_s);
        __syncthreads();
        for (int s0 = 0; s0 < kc; s0 += SUB) {
            const int sc = min(SUB, kc - s0);
            for (int kl = tid; kl < SUB; kl += nt) {
                const int k = k0 + s0 + kl;
                const double w = kl < sc ? lm_weight(a, b, k) : 0.0;
                double jx[LS_POSE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, jy[LS_POSE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                double rx = 0.0, ry = 0.0, term = 0.0;
                if (w != 0.0) {   // a landmark of weight 0 is skipped: its target is not read, its rows are +0
                    const double v0 = v_s[3 * (s0 + kl)], v1 = v_s[3 * (s0 + kl) + 1], v2 = v_s[3 * (s0 + kl) + 2];
                    const double rv0 = (R[0] * v0 + R[1] * v1) + R[2] * v2;
                    const double rv1 = (R[3] * v0 + R[4] * v1) + R[5] * v2;
                    const double x = f * rv0 + t0;
                    const double q1 = f * rv1 + t1;
                    const double y = (a.im - q1) - 1.0;
                    const float* tg = a.target + ((size_t)b * a.K + k) * 2;
                    rx = x - (double)tg[0];
                    ry = y - (double)tg[1];
                    term = w * (rx * rx + ry * ry);
#pragma unroll
                    for (int an = 0; an < 3; an++) {
                        const double e0 = (dR_s[an][0] * v0 + dR_s[an][1] * v1) + dR_s[an][2] * v2;
                        const double e1 = (dR_s[an][3] * v0 + dR_s[an][4] * v1) + dR_s[an][5] * v2;
                        jx[an] = f * e0;
                        jy[an] = -(f * e1);
                    }
                    jx[3] = 1.0;
                    jy[4] = -1.0;
                    jx[5] = rv0;
                    jy[5] = -rv1;
                }
#pragma unroll
                for (int c = 0; c < LS_POSE; c++) {
                    jp_s[2 * kl][c] = jx[c];
                    jp_s[2 * kl + 1][c] = jy[c];
                }
                r_s[2 * kl] = rx;
                r_s[2 * kl + 1] = ry;
                w_s[kl] = w;
                term_s[kl] = term;
            }
            if (COEF) {
                const int j = tid & 255;
                if (j < 16 * T) {
                    for (int kl = tid >> 8; kl < LS_SUB; kl += LS_BLOCK / 256) {
                        const int k = k0 + s0 + kl;
                        double ux = 0.0, uy = 0.0;
                        if (kl < sc && j < Kt && lm_weight(a, b, k) != 0.0) {
                            const float* Bm = partB + (size_t)3 * k * Kt + j;
                            const double U0 = (double)Bm[0], U1 = (double)Bm[Kt], U2 = (double)Bm[2 * (size_t)Kt];
                            const double u0 = (R[0] * U0 + R[1] * U1) + R[2] * U2;
                            const double u1 = (R[3] * U0 + R[4] * U1) + R[5] * U2;
                            ux = f * u0;
                            uy = -(f * u1);
                        }
                        jc_s[(2 * kl) * LS_PITCH + j] = ux;
                        jc_s[(2 * kl + 1) * LS_PITCH + j] = uy;
                    }
                }
            }
            __syncthreads();
            if (tid == 0)
                for (int kl = 0; kl < sc; kl++) sse = sse + term_s[kl];
            if (pl >= 0 && pl < 21) {
                for (int row = 0; row < 2 * sc; row++) pacc = pacc + (w_s[row >> 1] * jp_s[row][pc]) * jp_s[row][pc2];
            } else if (pl >= 21 && pl < LS_POSE_LANES) {
                for (int row = 0; row < 2 * sc; row++) pacc = pacc + (w_s[row >> 1] * jp_s[row][pc]) * r_s[row];
            }
            if (COEF) {
                if (tid < Kt) {
                    for (int row = 0; row < 2 * sc; row++) {
                        const double u = jc_s[row * LS_PITCH + tid];
                        const double wj = w_s[row >> 1] * u;
                        accD = accD + wj * u;
                        accg = accg + wj * r_s[row];
#pragma unroll
                        for (int c = 0; c < LS_POSE; c++) accP[c] = accP[c] + wj * jp_s[row][c];
                    }
                }
                const int fr_ = lane >> 4, fc = lane & 15;
                for (int ks = 0; ks < 2 * LS_SUB / 4; ks++) {
                    const int row = 4 * ks + fr_;
                    const double wr = w_s[row >> 1];
                    const double* rp = jc_s + row * LS_PITCH + fc;
#pragma unroll
                    for (int q = 0; q < LS_PAIRS; q++) {
                        if (q < mine) {
                            const int pr = pair_s[wave + LS_WAVES * q];
                            const double ua = rp[pr & 0xFFFF];
                            const double ub = wr * rp[pr >> 16];
                            macc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, ub, macc[q], 0, 0, 0);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- the system ----
    double* A = COEF ? s.ws + (size_t)b * ls_face_doubles(Kt) : small_s;
    double* Hc = COEF ? A + ls_tri(LS_POSE + Kt) + (LS_POSE + Kt) : small_s + ls_tri(LS_POSE) + LS_POSE;
    if (pl >= 0 && pl < 21) {
        if (pidx[pc] >= 0 && pidx[pc2] >= 0) {
            if (pc == pc2) {
                D_s[pidx[pc]] = pacc;
            } else {
                A[ls_at(pidx[pc], pidx[pc2])] = pacc;
                Hc[ls_at(pidx[pc], pidx[pc2])] = pacc;
            }
        }
    } else if (pl >= 21 && pl < LS_POSE_LANES) {
        if (pidx[pc] >= 0) g_s[pidx[pc]] = pacc;
    }
    if (COEF) {
        if (tid < Kt) {
            const int i = np + tid;
            const double rg = s.ridge ? (double)s.ridge[tid] : 0.0;
            const double dj = (double)a_s[tid] - (s.center ? (double)s.center[tid] : 0.0);
            D_s[i] = accD;
            g_s[i] = accg + rg * dj;
            e_s[i] = rg * (dj * dj);
#pragma unroll
            for (int c = 0; c < LS_POSE; c++) {
                if (pidx[c] >= 0) {
                    A[ls_at(i, pidx[c])] = accP[c];
                    Hc[ls_at(i, pidx[c])] = accP[c];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < LS_PAIRS; q++) {
            if (q < mine) {
                const int pr = pair_s[wave + LS_WAVES * q];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ii = (pr & 0xFFFF) + (lane >> 4) + 4 * r, jj = (pr >> 16) + (lane & 15);
                    if (ii < Kt && jj < ii) {
                        A[ls_at(np + ii, np + jj)] = macc[q][r];
                        Hc[ls_at(np + ii, np + jj)] = macc[q][r];
                    } else if (ii < Kt && jj == ii) {
                        diag_s[np + ii] = macc[q][r];
                    }
                }
            }
        }
    }
    __syncthreads();
    {
        const double damp = s.damp ? s.damp[b] : 0.0;
        for (int i = tid; i < Pn; i += nt) {
            double h = D_s[i];
            if (COEF && i >= np) h = diag_s[i] + (s.ridge ? (double)s.ridge[i - np] : 0.0);
            Hc[ls_at(i, i)] = h;
            A[ls_at(i, i)] = h + damp * D_s[i];
            A[ls_at(Pn, i)] = -g_s[i];
        }
        if (tid == 0) {
            double F = sse;
            if (COEF) {
                double pr = 0.0;
                for (int j = 0; j < Kt; j++) pr = pr + e_s[np + j];
                F = sse + pr;
            }
            F_s[0] = F;
        }
    }
    __syncthreads();

    // ---- factorisation ----
    bool okf = true;
    for (int c = 0; c < Pn; c++) {
        const double d = A[ls_at(c, c)];
        if (!(d > 0.0) || !(d <= DBL_MAX)) {   // the same value in every lane: a uniform exit
            okf = false;
            break;
        }
        const double l = sqrt(d);
        for (int i = c + 1 + tid; i <= Pn; i += nt) {
            const double q = A[ls_at(i, c)] / l;
            col_s[i] = q;
            A[ls_at(i, c)] = q;
        }
        if (tid == 0) diag_s[c] = l;
        __syncthreads();
        for (int i = c + 1 + wave; i <= Pn; i += nt >> 6) {
            const double li = col_s[i];
            const int jmax = i < Pn ? i : Pn - 1;
            double* row = A + ls_at(i, 0);
            for (int j = c + 1 + lane; j <= jmax; j += 64) row[j] = row[j] - li * col_s[j];
        }
        __syncthreads();
    }

    // ---- substitution and prediction ----
    if (okf) {
        for (int i = tid; i < Pn; i += nt) y_s[i] = A[ls_at(Pn, i)];
        __syncthreads();
        for (int c = Pn - 1; c >= 0; c--) {
            const double dc = y_s[c] / diag_s[c];
            if (tid < c) y_s[tid] = y_s[tid] - A[ls_at(c, tid)] * dc;
            else if (tid == c) d_s[c] = dc;
            __syncthreads();
        }
        for (int i = tid; i < Pn; i += nt) {
            double q = 0.0;
            for (int j = 0; j < Pn; j++) q = q + (j <= i ? Hc[ls_at(i, j)] : Hc[ls_at(j, i)]) * d_s[j];
            e_s[i] = d_s[i] * (2.0 * g_s[i] + q);
            if (!(fabs(d_s[i]) <= DBL_MAX)) bad_s = 1;
        }
        __syncthreads();
        if (tid == 0) {
            double m = 0.0;
            for (int i = 0; i < Pn; i++) m = m + e_s[i];
            const double pred = F_s[0] + m;
            F_s[1] = pred;
            if (!(fabs(F_s[0]) <= DBL_MAX) || !(fabs(pred) <= DBL_MAX)) bad_s = 1;
        }
        __syncthreads();
    }
    const bool fail = !okf || bad_s != 0;
    for (int t = tid; t < nd; t += nt) {
        double out = 0.0;
        if (!fail) {
            if (t < 7) {
                const int slot = t < 5 ? t : (t == 6 ? 5 : -1);
                int pi = -1;
#pragma unroll
                for (int c = 0; c < LS_POSE; c++)
                    if (c == slot) pi = pidx[c];
                if (pi >= 0) out = d_s[pi];
            } else if (COEF) {
                out = d_s[np + (t - 7)];
            }
        }
        s.delta[(size_t)b * nd + t] = out;
    }
    if (tid == 0) {
        s.cost[2 * (size_t)b] = F_s[0];
        s.cost[2 * (size_t)b + 1] = fail ? F_s[0] : F_s[1];
        s.ok[b] = fail ? 0 : 1;
    }
}

}  // namespace fr

size_t fr_landmark_solve_workspace_impl(int B, int n_shape, int n_exp) {
    if (B < 1 || n_shape < 0 || n_exp < 0 || (long long)n_shape + n_exp > fr::LM_MAX_COEF) return 0;
    return (size_t)B * fr::ls_face_doubles(n_shape + n_exp) * sizeof(double);
}

int fr_launch_landmark_solve(const float* params, const float* lbasis, const float* target, const float* weight, int weight_batch,
                             const float* ridge, const float* center, const double* damp, int pose_mask, int fit_coef, int B, int K,
                             int n_shape, int n_exp, float im_size, double* delta, double* cost, int* ok, void* workspace,
                             hipStream_t stream) {
    using namespace fr;
    LsArgs s = {};
    s.lm.params = params; s.lm.lbasis = lbasis; s.lm.target = target; s.lm.weight = weight;
    s.lm.K = K; s.lm.Kt = n_shape + n_exp; s.lm.weight_batch = weight_batch; s.lm.im = (double)im_size;
    s.ridge = ridge; s.center = center; s.damp = damp; s.delta = delta; s.cost = cost; s.ok = ok;
    s.ws = reinterpret_cast<double*>(workspace); s.pose_mask = pose_mask;
    if (fit_coef) {
        hipLaunchKernelGGL(lm_solve_kernel<true>, dim3((unsigned)B), dim3(LS_BLOCK), 0, stream, s);
    } else {
        const int rows = 3 * (K < LM_KC ? K : LM_KC);
        int block = (rows + 63) / 64 * 64;
        block = block > LS_BLOCK ? LS_BLOCK : block;
        hipLaunchKernelGGL(lm_solve_kernel<false>, dim3((unsigned)B), dim3(block), 0, stream, s);
    }
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
