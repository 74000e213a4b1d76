// 3DMM decode backward for gfx950 (MI355X): dL/d vertex_proj [B,3,N] -> dL/d params [B,235].
//
// What it computes: the gradient TF autodiff derives from FaceRecNet.vertices_transform (nets/network.py:140-171):
//   dq      = (g_x, -g_y, g_z)                                  y row is (im_size - q_1) - 1 (:168)
//   d t3d_i = sum_p dq_i                                        (:164-165)
//   d f     = sum_p (R v) . dq  = sum_p (q - t3d) . dq / f      (f_expand * R, :163-165)
//   dv      = (f R)^T dq ;  d alpha = pc_shape^T dv ;  d beta = pc_exp^T dv          (:153-159)
//   d angles = 0: R comes out of tf.py_func (:150), which has no gradient in the reference.  (The default, and it stays so: the
//              opt-in pose kernels at the end of this file add d angles and dL/dR for a caller that asks -- fr_decode_pose_backward.)
//
// How (reference-layout entry point; the packed entry point runs bwd_fused_kernel + bwd_reduce_kernel: see there): three
// launches, no float atomics (bit-reproducible):
//   bwd_prepass_kernel  elementwise: dq -> dv, written transposed into MFMA B-fragment order dvT4[row][16][4]
//                       (LDS tile transpose so both the read of g and the write of dvT4 are coalesced), plus
//                       per-workgroup partial sums for d t3d and d f;
//   bwd_gemm_kernel     the [228 x 3N].[3N x 64] reduction on the matrix cores (exact-f32 v_mfma_f32_16x16x4_f32):
//                       split over row chunks, one workgroup per chunk, wave w owns 64 coefficient slots (lane l of a
//                       k-step loads FOUR consecutive coefficients of row l>>4 with one 16-byte request -- 256
//                       contiguous bytes of the reference-layout row per 16 lanes -- and feeds them to four MFMAs,
//                       element i to MFMA i, so MFMA i's 16 output rows are coefficients 4 m + i), dv fragments are
//                       one dwordx4 per k-step shared through L1 by the waves; partial [slots x 64] slabs go to the
//                       workspace;
//   bwd_reduce_kernel   sums the slabs / partials in a fixed order and writes grad_params.
#include "fr_common.h"

namespace fr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BW_PV = 64;        // vertices per prepass workgroup
constexpr int BW_MAXWAVES = 8;   // gemm waves per workgroup: one per 64 coefficient slots (<= 512 slots)
// coefficient slots: shape columns padded to a multiple of 4, then expression columns padded to a multiple of 4
__host__ __device__ inline int bw_ns4(int ns) { return (ns + 3) & ~3; }
__host__ __device__ inline int bw_waves(int ns, int ne) { return (bw_ns4(ns) + ((ne + 3) & ~3) + 63) / 64; }

struct BwdArgs {
    const float* g;          // [B,3,N]
    const float* params;     // [B,nd]
    const float* vproj;      // [B,3,N] forward output
    const float* pc_shape;   // [3N,ns]
    const float* pc_exp;     // [3N,ne]
    const float* R_override; // [B,9] or null
    float* grad_params;      // [B,nd]
    float4* dvT4;            // [3N][16] float4: dv[row][batch = 16*mb + j] at [row][j].mb
    float* pose_part;        // [prepass blocks][64][4]  (dt_x, dt_y, dt_z, sum (q-t).dq)
    float* slab;             // [gemm blocks][64 * waves slots][64]
    int B, N, ns, ne, b0, nbatch;
    int pre_blocks, gemm_blocks, rows_per_block;
    float im_size;
    // K-major packed image (fr_decode_backward_pack_basis) and its geometry; null: the reference-layout kernel runs
    const float4* At;        // packed image [vertex groups of 16][3 coordinates][slot blocks][64 lanes] float4 (bwd_pack_kernel)
    int sbt, sbs;            // slot blocks of 16 coefficients in all / of the shape basis (expression blocks follow)
    int rbt, rb_per_block;   // reference-layout path: 16-row blocks in all / per gemm workgroup.  Packed path (bwd_fused_kernel):
                             // vertex groups of 16 in all / per workgroup
    int exp_slot0;           // first coefficient slot of the expression basis in the slabs
    int nslots;              // coefficient slots per partial slab (64 per wave of the GEMM workgroup)
    int zpitch;              // > 0 (bwd_fused_z_kernel): g is NOT [B,3,N] but the z row alone, face b at g + b * zpitch -- the x and y rows
                             // are zero by construction (every vertex gradient of this model comes through the depth plane)
    const float* mu;         // [3N] mean shape, or null.  Non-null (fr_decode_3dmm_backward_packed_mu): d f is formed WITHOUT the
                             // forward output -- sum_p (R v_p) . dq = sum_p v_p . dv_p / f with v = mu + S alpha + E beta, i.e.
                             // d f = (sum_p mu_p . dv_p + alpha . d alpha + beta . d beta) / f: the fused kernel reads 0.64 MB of mu
                             // (L2-resident) instead of 41 MB of vertex_proj -- which buys MEMORY (the forward output need not be
                             // kept for the backward), not time: 71.3 vs 71.1 us at 64 faces, 56.3 vs 53.2 at 32; each workgroup adds the parameters' dot product with
                             // ITS partial coefficient gradients to its pose partial (linear: the partials add up to the whole)
};

__device__ __forceinline__ void bwd_rotation(const BwdArgs& a, int b, float* R9) {
    const int nd = FR_N_POSE + a.ns + a.ne;
    const float* pr = a.params + (size_t)(a.b0 + b) * nd;
    if (a.R_override) {
#pragma unroll
        for (int i = 0; i < 9; i++) R9[i] = a.R_override[(size_t)(a.b0 + b) * 9 + i];
        return;
    }
    double sp, cp, sy, cy, st, ct;
    sincos((double)pr[0], &sp, &cp);
    sincos((double)pr[1], &sy, &cy);
    sincos((double)pr[2], &st, &ct);
    // (R_pitch . R_yaw) . R_roll in float64, 3-term dots without FMA, one rounding (network.py:276-290)
    const double Rp[9] = {1, 0, 0, 0, cp, sp, 0, -sp, cp};
    const double Ry[9] = {cy, 0, -sy, 0, 1, 0, sy, 0, cy};
    const double Rr[9] = {ct, st, 0, -st, ct, 0, 0, 0, 1};
    double PY[9], Rm[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) PY[3 * i + j] = (Rp[3 * i] * Ry[j] + Rp[3 * i + 1] * Ry[3 + j]) + Rp[3 * i + 2] * Ry[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rm[3 * i + j] = (PY[3 * i] * Rr[j] + PY[3 * i + 1] * Rr[3 + j]) + PY[3 * i + 2] * Rr[6 + j];
#pragma unroll
    for (int i = 0; i < 9; i++) R9[i] = (float)Rm[i];
}

// Sum over the 64 lanes of a wave in a FIXED order (pairs, quads, half rows, rows, then the row totals passed on with
// row_bcast:15 / row_bcast:31): six v_add_f32_dpp, result valid in lane 63.  All 64 lanes must be active.
#define FR_DPP_ADD(x, ctrl, rmask, bc) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, rmask, 0xf, bc))
__device__ __forceinline__ float wave_sum_to_lane63(float x) {
    FR_DPP_ADD(x, 0x111, 0xf, true);    // row_shr:1
    FR_DPP_ADD(x, 0x112, 0xf, true);    // row_shr:2
    FR_DPP_ADD(x, 0x114, 0xf, true);    // row_shr:4
    FR_DPP_ADD(x, 0x118, 0xf, true);    // row_shr:8  -> lane 15 of every row holds the row's sum
    FR_DPP_ADD(x, 0x142, 0xa, false);   // row_bcast:15 into rows 1 and 3
    FR_DPP_ADD(x, 0x143, 0xc, false);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's sum
    return x;
}
#undef FR_DPP_ADD

// ---- prepass: 64 vertices x 64 batch columns per workgroup -------------------------------------------------------------
__global__ __launch_bounds__(256) void bwd_prepass_kernel(BwdArgs a) {
    __shared__ float Mt[64][13];                 // f*R (9), t (3), 1/f or 0
    __shared__ float tile[3][BW_PV][64 + 1];      // dv[c][p][bslot]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nd = FR_N_POSE + a.ns + a.ne;
    const int N = a.N;
    if (tid < 64) {
        float m[13];
#pragma unroll
        for (int i = 0; i < 13; i++) m[i] = 0.f;
        if (tid < a.nbatch) {
            const float* pr = a.params + (size_t)(a.b0 + tid) * nd;
            float R[9];
            bwd_rotation(a, tid, R);
            const float f = pr[6];
#pragma unroll
            for (int i = 0; i < 9; i++) m[i] = f * R[i];
            m[9] = pr[3]; m[10] = pr[4]; m[11] = pr[5];
            m[12] = (f != 0.0f) ? 1.0f / f : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 13; i++) Mt[tid][i] = m[i];
    }
    __syncthreads();
    const int p = blockIdx.x * BW_PV + lane;
    const bool pok = p < N;
    // wave wv handles batch columns 16*wv .. 16*wv+15, lane = vertex: reads of g / vproj are 256-byte coalesced.  Four
    // columns per trip: their 24 loads are requested (unconditionally, clamped) before anything is computed
    const int pc = pok ? p : 0;
    for (int bq0 = 0; bq0 < 16; bq0 += 4) {
        float gq[4][3], vq[4][3];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int c = 0; c < 3; c++) gq[u][c] = vq[u][c] = 0.f;
        if (16 * wv + bq0 < a.nbatch)   // (wave-uniform: a trip whose four columns are all dead requests nothing)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int b = min(16 * wv + bq0 + u, a.nbatch - 1);
            const float* gb = a.g + (size_t)(a.b0 + b) * 3 * N;
            const float* vb = a.vproj + (size_t)(a.b0 + b) * 3 * N;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                gq[u][c] = gb[(size_t)c * N + pc];
                vq[u][c] = vb[(size_t)c * N + pc];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int b = 16 * wv + bq0 + u;
            float dq0 = 0.f, dq1 = 0.f, dq2 = 0.f, fs = 0.f;
            if (pok && b < a.nbatch) {
                dq0 = gq[u][0];
                dq1 = -gq[u][1];
                dq2 = gq[u][2];
                // (q - t): q_0 = out_x, q_1 = (im - 1) - out_y, q_2 = out_z
                const float q0 = vq[u][0] - Mt[b][9];
                const float q1 = ((a.im_size - 1.0f) - vq[u][1]) - Mt[b][10];
                const float q2 = vq[u][2] - Mt[b][11];
                fs = __builtin_fmaf(q2, dq2, __builtin_fmaf(q1, dq1, q0 * dq0));
            }
            const float* m = Mt[b];
            const int bslot = (b & 15) * 4 + (b >> 4);
#pragma unroll
            for (int c = 0; c < 3; c++)
                tile[c][lane][bslot] = __builtin_fmaf(m[6 + c], dq2, __builtin_fmaf(m[3 + c], dq1, m[c] * dq0));
            // fixed-order wave reduction over the 64 vertices (six DPP adds per value, the total lands in lane 63; the
            // __shfl_xor butterfly was 24 dependent ds_bpermute trips per column)
            const float r0 = wave_sum_to_lane63(dq0), r1 = wave_sum_to_lane63(dq1), r2 = wave_sum_to_lane63(dq2),
                        r3 = wave_sum_to_lane63(fs);
            if (lane == 63) {
                float* pp = a.pose_part + ((size_t)blockIdx.x * 64 + b) * 4;
                pp[0] = r0; pp[1] = r1; pp[2] = r2; pp[3] = r3 * m[12];
            }
        }
    }
    __syncthreads();
    // flush: rows r = c*N + p, 64 floats (= 16 float4) per row, coalesced
    for (int i = tid; i < 3 * BW_PV * 16; i += 256) {
        const int j4 = i & 15, pl = (i >> 4) & (BW_PV - 1), c = i >> 10;
        const int pp = blockIdx.x * BW_PV + pl;
        if (pp < N) {
            const float* t = &tile[c][pl][j4 * 4];
            a.dvT4[((size_t)c * N + pp) * 16 + j4] = make_float4(t[0], t[1], t[2], t[3]);
        }
    }
    // the pad rows [3N, 16 * row blocks) of the last 16-row block (read as part of a 1 KiB fragment by the packed kernel): zeros
    if (blockIdx.x == 0) {
        const long long pad0 = 3ll * N * 16, pad1 = (long long)a.rbt * 256;
        for (long long i = pad0 + tid; i < pad1; i += 256) a.dvT4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- the reduction over vertices on the matrix cores -------------------------------------------------------------------
// D^T[coeff][batch] += sum_k basis[row k][coeff] * dv[row k][batch]:  A operand = basis^T (lane l: row r0+(l>>4),
// coefficient slot 4*(l&15)+i for MFMA i), B operand = dv (lane l: row r0+(l>>4), batch 16*mb+(l&15)).
// NB: live 16-column blocks of this pass (1..4): dead blocks cost neither MFMAs nor slab stores -- at the 32 faces per
// GPU of the reference's train loop that is half of the matrix work.  The row loop takes four k-steps per trip with all
// their operands requested before the first MFMA issues; every accumulation chain stays in row order.
typedef float f32x4u4 __attribute__((ext_vector_type(4), aligned(4)));
template <int NB>
__global__ __launch_bounds__(BW_MAXWAVES * 64) void bwd_gemm_kernel(BwdArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rows = 3ll * a.N;
    const long long r_begin = (long long)blockIdx.x * a.rows_per_block;
    const long long r_end = min(rows, r_begin + a.rows_per_block);
    const int kq = lane >> 4, jn = lane & 15;
    // this lane's four coefficient slots: source array, row stride, first column, live columns (0..4)
    const int ns4 = bw_ns4(a.ns);
    const int slot0 = 64 * wave + 4 * jn;
    const bool in_shape = slot0 < ns4;
    const float* src = in_shape ? a.pc_shape : a.pc_exp;
    const int stride = in_shape ? a.ns : a.ne;
    const int col0 = in_shape ? slot0 : slot0 - ns4;
    const int live = max(0, min(4, stride - col0));
    f32x4 acc[4][NB];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int mb = 0; mb < NB; mb++) acc[i][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto bsel = [](const float4& v, int mb) { return mb == 0 ? v.x : mb == 1 ? v.y : mb == 2 ? v.z : v.w; };
    constexpr int UN = 4;   // k-steps (of 4 rows) per trip
    auto request = [&](long long r, float4 (&dv)[UN], f32x4 (&av)[UN]) {
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const long long rr = r + 4 * u + kq;
            const bool rok = rr < r_end;
            dv[u] = rok ? a.dvT4[(size_t)rr * 16 + jn] : make_float4(0.f, 0.f, 0.f, 0.f);
            av[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (rok) {
                const float* ptr = src + (size_t)rr * stride + col0;
                if (live == 4) {
                    av[u] = *reinterpret_cast<const f32x4u4*>(ptr);   // (rows are only 4-byte aligned: 199 columns)
                } else {   // the array's last, partial quadruple: never read past the row
                    if (live > 0) av[u][0] = ptr[0];
                    if (live > 1) av[u][1] = ptr[1];
                    if (live > 2) av[u][2] = ptr[2];
                }
            }
        }
    };
    auto consume = [&](const float4 (&dv)[UN], const f32x4 (&av)[UN]) {
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int mb = 0; mb < NB; mb++)
                    acc[i][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], bsel(dv[u], mb), acc[i][mb], 0, 0, 0);
    };
    // (a second operand set, requested one trip ahead, measured no faster: 44.3 / 71.4 us against 45.1 / 68.0 us at
    // 32 / 64 faces, at 176 instead of 110 VGPRs)
    for (long long r = r_begin; r < r_end; r += 4 * UN) {
        float4 dv[UN];
        f32x4 av[UN];
        request(r, dv, av);
        consume(dv, av);
    }
    // D^T tile of MFMA i: row m = 4*(lane>>4) + reg is coefficient slot 64*wave + 4*m + i, column (batch within block) = lane & 15
    float* slab = a.slab + (size_t)blockIdx.x * a.nslots * 64;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int mb = 0; mb < NB; mb++)
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
                const int slot = 64 * wave + 4 * (4 * kq + rg) + i;
                slab[(size_t)slot * 64 + 16 * mb + jn] = acc[i][mb][rg];
            }
}


// ---- the same reduction from a K-major packed image (round 3) ---------------------------------------------------------
// The kernel above reads the basis in its reference layout: 16-byte pieces at a 796-byte row stride, requested a trip at a
// time and waited for with the compiler's vmcnt(0) -- the two waves that share a SIMD run in lock-step, so every trip
// exposes a full memory round trip (47 / 70 us at 32 / 64 faces against a 33 us MFMA floor).  With the basis packed ONCE
// into MFMA A-fragment order (fr_decode_backward_pack_basis: [16-row block][16-coefficient block][lane] float4, element
// j = basis[16 rb + 4 j + (lane >> 4)][16 sb + (lane & 15)], zero padded) every operand fetch is a coalesced, aligned 1 KiB
// fragment -- the dv rows of a 16-row block are four such fragments as well -- and the fragments run through a ring of
// BR row blocks of registers filled by inline-asm loads that the compiler can neither reorder nor drain; the only waits are
// counted.  Accumulation order per output: rows ascending within the workgroup's row range (as above); the partial
// slabs are summed by bwd_reduce_kernel in its fixed order.
__global__ __launch_bounds__(256) void bwd_pack_kernel(const float* __restrict__ pc_shape, const float* __restrict__ pc_exp,
                                                       int N, int ns, int ne, int sbs, int sbt, long long ngroups,
                                                       float4* __restrict__ At) {
    // image [vertex group of 16][coordinate][16-coefficient block][lane] float4, element j = basis[c N + 16 grp + 4 j + (lane >> 4)]
    // [16 sb + (lane & 15)], zero padded: a vertex group's three 16-row blocks (x, y, z rows of the SAME sixteen vertices) sit
    // side by side, so that the workgroup that multiplies them can form their dv rows from ONE tile of the incoming gradient
    const long long total = ngroups * 3 * sbt * 64;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        long long q = i >> 6;
        const int sb = (int)(q % sbt);
        q /= sbt;
        const int c = (int)(q % 3);
        const long long grp = q / 3;
        const int slot = 16 * sb + (lane & 15);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long pv = 16 * grp + 4 * j + (lane >> 4);
            float x = 0.f;
            if (pv < N) {
                const size_t row = (size_t)c * N + pv;
                if (sb < sbs) { if (slot < ns) x = pc_shape[row * ns + slot]; }
                else { const int cc = slot - 16 * sbs; if (cc < ne) x = pc_exp[row * ne + cc]; }
            }
            v[j] = x;
        }
        At[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

#define FRB_LD(dst, ptr) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(ptr))
// ---- the fused backward: gradient tile -> dv rows (LDS) -> MFMA reduction, one launch ------------------------------------------
// Round 3 ran a prepass (g, vertex_proj -> dv rows in B-fragment order + the pose partial sums: 123 MB moved, 27.6 us) and then
// the reduction (153 MB of basis + the 41 MB of dv rows again).  Here ONE workgroup per CU walks its vertex groups of 16; per
// group its 256 staging threads -- thread = (batch column b, vertex quad q) -- load the 16 x 64 tile of g and of vertex_proj
// (six 16-byte loads per thread, inline asm, in the same counted-wait stream as the basis fragments), form the group's
// three dv row blocks  dv = (f R)^T dq  and the d t3d / d f partial sums in registers, and park the dv rows in LDS in MFMA
// B-fragment order (double buffered; ONE LDS-only barrier per group); the waves then multiply the group's three basis row
// blocks (twelve 1 KiB fragments per wave, two groups in flight) against them.  dv never exists in global memory: g and
// vertex_proj are read once, the 41 MB write + re-read and the prepass launch are gone.
// Summation order: per output, groups ascending, x / y / z row block, k-step -- fixed by the chunking (FR_BWD_CHUNKS) alone: CB,
// NB, the batch size, a face's column and its 64-face pass (b0) change no bit -- with one exception, the mu form's d f, whose
// per-workgroup share alpha . d alpha + beta . d beta is summed over a wave's CB slot blocks first and then wave by wave, so its
// association follows CB as well (tests/test_decode_backward_bounds_gpu.py holds both).
// CB: 16-coefficient blocks per wave.  CB = 2 (eight waves for the model's 15 blocks: two per SIMD, one multiplying while the
// other waits for its fragments) or 4 (four waves, one per SIMD; also what bases of more than 16 blocks take).
// Either way the packed path covers bases of at most 16 blocks (256 coefficients: the model has 228); larger ones take the
// reference-layout entry point (fr_decode_backward_basis_bytes answers 0 for them).
// ZONLY (bwd_fused_z_kernel, fr_decode_render_backward): the incoming gradient is the pitched z plane of the render backward;
// the tile is ONE 16-byte load of g_z plus the three mu rows (mu form of d f only) -- four loads per staging thread instead of
// six, and every counted wait behind a tile counts four.  dv is evaluated with the SAME expression, dq0 = +0.0f and dq1 = -0.0f
// as constants (what the dense chain reads back from the zeroed x / y rows and negates): bit-identical for every f R,
// non-finite ones included, at a few VALU operations per vertex.
template <int NB, int CB, bool ZONLY>
__device__ __forceinline__ void bwd_fused_body(const BwdArgs& a) {
    constexpr int TL = ZONLY ? 4 : 6;   // tile loads per staging thread
    __shared__ float Mt[64][13];                                            // f*R (9), t (3), 1/f or 0
    __shared__ __attribute__((aligned(16))) float4 dvL[2][3][4][64];        // [buffer][coordinate][k-step][lane] (mb in .xyzw)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nd = FR_N_POSE + a.ns + a.ne;
    const int N = a.N;
    const bool muf = ZONLY || a.mu != nullptr;   // (uniform) d f from mu . dv: the tile's second operand is mu, not vertex_proj
    if (tid < 64) {
        float m[13];
#pragma unroll
        for (int i = 0; i < 13; i++) m[i] = 0.f;
        if (tid < a.nbatch) {
            const float* pr = a.params + (size_t)(a.b0 + tid) * nd;
            float R[9];
            bwd_rotation(a, tid, R);
            const float f = pr[6];
#pragma unroll
            for (int i = 0; i < 9; i++) m[i] = f * R[i];
            m[9] = pr[3]; m[10] = pr[4]; m[11] = pr[5];
            m[12] = (f != 0.0f) ? 1.0f / f : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 13; i++) Mt[tid][i] = m[i];
    }
    __syncthreads();
    // staging role (threads 0..255): batch column sb_ = tid >> 2 (its 16-column block is the wave index), vertex quad q
    const bool stager = tid < 256;
    const int sb_ = (tid >> 2) & 63, q = tid & 3;
    const bool blive = stager && sb_ < a.nbatch;
    float m[13];
#pragma unroll
    for (int i = 0; i < 13; i++) m[i] = Mt[sb_][i];
    const int bc = min(sb_, a.nbatch - 1);   // (dead columns load a live column's tile and discard it)
    const float* gx = ZONLY ? a.g + (size_t)(a.b0 + bc) * a.zpitch + 4 * q : a.g + (size_t)(a.b0 + bc) * 3 * N + 4 * q;
    const float* vx = muf ? a.mu + 4 * q : a.vproj + (size_t)(a.b0 + bc) * 3 * N + 4 * q;
    // MFMA role: this wave's CB 16-coefficient blocks
    const int kq = lane >> 4, jn = lane & 15;
    const int sbt = a.sbt;
    const int sb0 = CB * wave;
    const int nsb = max(0, min(CB, sbt - sb0));          // live ones (wave-uniform; 0: a staging-only wave)
    const bool stage_wave = wave < 4;                    // (wave-uniform: the 256 staging threads are waves 0..3)
    const long long g_begin = (long long)blockIdx.x * a.rb_per_block;              // (rb_per_block = vertex groups per workgroup)
    const long long g_end = min((long long)a.rbt, g_begin + a.rb_per_block);       // (rbt = vertex groups in all)
    const int n = (int)(g_end - g_begin);
    f32x4 acc[CB][NB];
#pragma unroll
    for (int i = 0; i < CB; i++)
#pragma unroll
        for (int mb = 0; mb < NB; mb++) acc[i][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 ra[2][3][CB];    // basis fragments of two groups in flight: [slot][coordinate][coefficient block]
    f32x4 tg[3], tv[3];    // the tile: g and vertex_proj, x / y / z rows, this thread's four vertices
    float ps0 = 0.f, ps1 = 0.f, ps2 = 0.f, ps3 = 0.f;   // pose partial sums of this thread's column: d t3d (3), sum (q - t) . dq
    // requests (a group past the end re-requests the last one and is never consumed; a dead coefficient block re-requests the
    // image's last block: every wave issues the same number of loads in the same order, which is what the counted waits count)
    auto req_tile = [&](long long grp) {
        if (!stage_wave) return;   // (a wave without staging threads requests no tile: its counted waits count accordingly)
        const long long gc = min(grp, (long long)a.rbt - 1);
        // (the LAST group's vertices may end before its sixteen: its loads are clamped to stay inside the rows; the values
        // of the missing vertices are zeroed by the mask below)
        const long long p0 = min(16 * gc, (long long)max(N - 16, 0));
        if constexpr (ZONLY) {
            const float* pg = gx + p0;
            FRB_LD(tg[2], pg);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* pv = vx + (size_t)c * N + p0;
                FRB_LD(tv[c], pv);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* pg = gx + (size_t)c * N + p0;
                const float* pv = vx + (size_t)c * N + p0;
                FRB_LD(tg[c], pg);
                FRB_LD(tv[c], pv);
            }
        }
    };
    auto req_basis = [&](int d, int c, long long grp) {
        const long long gc = min(grp, (long long)a.rbt - 1);
        const float4* ab = a.At + ((size_t)(gc * 3 + c) * sbt) * 64 + lane;
#pragma unroll
        for (int i = 0; i < CB; i++) {
            const float4* p = ab + (size_t)min(sb0 + i, sbt - 1) * 64;
            FRB_LD(ra[d][c][i], p);
        }
    };
    // counted waits: the tile is followed by the 3 CB fragments of its group; a coordinate's CB fragments by 5 CB fragments
    // (+ in a staging wave the tiles of the next TWO groups, requested in between: 2 TL loads -- 12, or 8 for the z-only tile)
    auto wait_tile = [&]() {
        if constexpr (ZONLY) {
            if (stage_wave) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(tg[2]), "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]) : "n"(3 * CB));
        } else {
            if (stage_wave) asm volatile("s_waitcnt vmcnt(%6)" : "+v"(tg[0]), "+v"(tg[1]), "+v"(tg[2]), "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]) : "n"(3 * CB));
        }
    };
    // tile -> dv rows of group grp into LDS buffer `buf` + the pose partial sums (tile registers must have arrived)
    auto stage = [&](long long grp, int buf) {
        const long long p0 = min(16 * grp, (long long)max(N - 16, 0));   // first vertex the tile was loaded from
        const int shift = (int)(16 * grp - p0);                              // > 0 only in a clamped last group
        float dvr[3][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // vertex of this slot: 16 grp + 4 q + r; it sits at tile position 4 q + r + shift (past 16: it does not exist)
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f;
            bool ok = blive && (16 * grp + 4 * q + r) < N;
            if (shift == 0) {
                if constexpr (!ZONLY) { g0 = tg[0][r]; g1 = tg[1][r]; }   // (z-only: g_x = g_y = +0, so dq0 = +0 and dq1 = -0)
                g2 = tg[2][r]; v0 = tv[0][r]; v1 = tv[1][r]; v2 = tv[2][r];
            } else {
                ok = false;   // (clamped group: taken by the slow path below)
            }
            const float dq0 = ok ? g0 : 0.f, dq1 = ok ? -g1 : 0.f, dq2 = ok ? g2 : 0.f;
            // (a slot without a vertex or a column without a face is exactly zero -- not 0 * m, which an infinite f would turn
            // into a NaN that the zero-padded basis rows then spread over the whole sum)
#pragma unroll
            for (int c = 0; c < 3; c++)
                dvr[c][r] = ok ? __builtin_fmaf(m[6 + c], dq2, __builtin_fmaf(m[3 + c], dq1, m[c] * dq0)) : 0.f;
            float fs;
            if (muf) {   // mu_p . dv_p (v0..v2 hold mu's x / y / z of this vertex)
                fs = ok ? __builtin_fmaf(v2, dvr[2][r], __builtin_fmaf(v1, dvr[1][r], v0 * dvr[0][r])) : 0.f;
            } else {
                const float q0 = v0 - m[9], q1 = ((a.im_size - 1.0f) - v1) - m[10], q2 = v2 - m[11];
                fs = ok ? __builtin_fmaf(q2, dq2, __builtin_fmaf(q1, dq1, q0 * dq0)) : 0.f;
            }
            ps0 += dq0; ps1 += dq1; ps2 += dq2; ps3 += fs;
        }
        if (shift != 0 && stager) {   // the one clamped group of the launch: guarded scalar loads (drains the wave's loads once)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const long long pvx = 16 * grp + 4 * q + r;
                float dq0 = 0.f, dq1 = 0.f, dq2 = 0.f, fs = 0.f;
                const bool okx = blive && pvx < N;
                float vv[3] = {0.f, 0.f, 0.f};
                if (okx) {
                    const float* vb = muf ? a.mu + pvx : a.vproj + (size_t)(a.b0 + bc) * 3 * N + pvx;
                    if constexpr (ZONLY) {
                        dq0 = 0.f; dq1 = -0.f; dq2 = a.g[(size_t)(a.b0 + bc) * a.zpitch + pvx];
                    } else {
                        const float* gb = a.g + (size_t)(a.b0 + bc) * 3 * N + pvx;
                        dq0 = gb[0]; dq1 = -gb[N]; dq2 = gb[2 * (size_t)N];
                    }
                    vv[0] = vb[0]; vv[1] = vb[N]; vv[2] = vb[2 * (size_t)N];
                }
#pragma unroll
                for (int c = 0; c < 3; c++)
                    dvr[c][r] = okx ? __builtin_fmaf(m[6 + c], dq2, __builtin_fmaf(m[3 + c], dq1, m[c] * dq0)) : 0.f;
                if (okx) {
                    if (muf) {
                        fs = __builtin_fmaf(vv[2], dvr[2][r], __builtin_fmaf(vv[1], dvr[1][r], vv[0] * dvr[0][r]));
                    } else {
                        const float q0 = vv[0] - m[9], q1 = ((a.im_size - 1.0f) - vv[1]) - m[10], q2 = vv[2] - m[11];
                        fs = __builtin_fmaf(q2, dq2, __builtin_fmaf(q1, dq1, q0 * dq0));
                    }
                }
                ps0 += dq0; ps1 += dq1; ps2 += dq2; ps3 += fs;
            }
        }
        if (stager) {
            // B fragment of k-step j = q: lane 16 r + (column & 15) holds dv[row 4 q + r][column], component = column >> 4
            float* base = reinterpret_cast<float*>(&dvL[buf][0][q][0]) + (size_t)(sb_ & 15) * 4 + (sb_ >> 4);
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) base[(size_t)c * (4 * 64 * 4) + (size_t)(16 * r) * 4] = dvr[c][r];
        }
    };
    if (n > 0) {
        // prologue: group 0's tile and basis fragments, its dv rows into buffer 0; then group 1's tile and fragments
        req_tile(g_begin);
#pragma unroll
        for (int c = 0; c < 3; c++) req_basis(0, c, g_begin);
        wait_tile();
        stage(g_begin, 0);
        req_tile(g_begin + 1);
#pragma unroll
        for (int c = 0; c < 3; c++) req_basis(1, c, g_begin + 1);
        // (two trips per loop pass, fully unrolled: the ring slot / LDS buffer index d is a compile-time constant -- indexed at
        // run time the fragment ring lands in scratch memory; a trip past the last group still waits, requests and meets the
        // barrier like the others -- every wave runs the same count -- and only skips the staging and the MFMAs)
        for (int i0 = 0; i0 < n; i0 += 2) {
#pragma unroll
            for (int d = 0; d < 2; d++) {
                const int i = i0 + d;
                const long long grp = g_begin + i;
                // tile of group i + 1 (behind it: the twelve fragments of group i + 1)
                wait_tile();
                // every wave has finished reading buffer d ^ 1 (group i - 1); buffer d (group i, written last trip) is published
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (i + 1 < n) stage(grp + 1, d ^ 1);
                req_tile(grp + 2);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    // the CB fragments of (group i, coordinate c), the oldest loads in flight
                    // (behind them: 5 CB fragments, and in a staging wave the 2 TL loads of two tiles)
                    if constexpr (CB == 4) {
                        if (stage_wave) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(ra[d][c][0]), "+v"(ra[d][c][1]), "+v"(ra[d][c][2]), "+v"(ra[d][c][3]) : "n"(20 + 2 * TL));
                        else asm volatile("s_waitcnt vmcnt(20)" : "+v"(ra[d][c][0]), "+v"(ra[d][c][1]), "+v"(ra[d][c][2]), "+v"(ra[d][c][3]));
                    } else {
                        static_assert(CB == 2 || CB == 4, "coefficient blocks per wave");
                        if (stage_wave) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(ra[d][c][0]), "+v"(ra[d][c][1]) : "n"(10 + 2 * TL));
                        else asm volatile("s_waitcnt vmcnt(10)" : "+v"(ra[d][c][0]), "+v"(ra[d][c][1]));
                    }
                    if (nsb > 0 && i < n) {
#pragma unroll
                        for (int j = 0; j < 4; j++) {          // k-step: rows 4 j .. 4 j + 3 of the row block, ascending
                            const float4 bv = dvL[d][c][j][lane];
                            const float bq[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                            for (int ii = 0; ii < CB; ii++)
                                if (ii < nsb) {
#pragma unroll
                                    for (int mb = 0; mb < NB; mb++)
                                        acc[ii][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[d][c][ii][j], bq[mb], acc[ii][mb], 0, 0, 0);
                                }
                        }
                    }
                    req_basis(d, c, grp + 2);
                }
            }
        }
#pragma unroll
        for (int dd = 0; dd < 2; dd++)
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int ii = 0; ii < CB; ii++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra[dd][c][ii]));
        if constexpr (ZONLY) asm volatile("s_waitcnt vmcnt(0)" : "+v"(tg[2]), "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]));
        else asm volatile("s_waitcnt vmcnt(0)" : "+v"(tg[0]), "+v"(tg[1]), "+v"(tg[2]), "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]));
    }
    // mu form of d f: this workgroup's share of alpha . d alpha + beta . d beta -- the parameters against the PARTIAL coefficient
    // gradients it has just accumulated (the dot product is linear, so the shares of all workgroups add up to the whole; no
    // third launch, nothing read back).  Lane (kq, jn) of wave w holds slots 16 (CB w + i) + 4 kq + rg of columns 16 mb + jn:
    // its products go to xp[w][kq][column], and the column's 4 x waves partials are added in a fixed order below.
    float* xp = reinterpret_cast<float*>(&dvL[0][0][0][0]);   // (the dv buffers are dead: every wave is past its last MFMA)
    const int nwaves = (int)(blockDim.x >> 6);
    if (muf) {
        __syncthreads();
        float xd[NB];
#pragma unroll
        for (int mb = 0; mb < NB; mb++) xd[mb] = 0.f;
#pragma unroll
        for (int i = 0; i < CB; i++)
            if (i < nsb) {
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int slot = 16 * (CB * wave + i) + 4 * kq + rg;
                    // slot -> parameter: shape slots [0, ns), expression slots from 16 sbs; padding slots carry no parameter.
                    // (Gathered here, once per workgroup.  Staging the parameters by slot in LDS at kernel start instead --
                    // 62 KB, conflict-free reads -- measured 1 / 4 / 7 us SLOWER at 64 / 32 / 16 faces: tools/bwd_ab_probe.py.)
                    int k = -1;
                    if (slot < 16 * a.sbs) { if (slot < a.ns) k = slot; }
                    else if (slot - 16 * a.sbs < a.ne) k = a.ns + slot - 16 * a.sbs;
#pragma unroll
                    for (int mb = 0; mb < NB; mb++) {
                        const int col = 16 * mb + jn;
                        const float x = (k >= 0 && col < a.nbatch) ? a.params[(size_t)(a.b0 + col) * nd + FR_N_POSE + k] : 0.f;
                        xd[mb] = __builtin_fmaf(x, acc[i][mb][rg], xd[mb]);
                    }
                }
            }
#pragma unroll
        for (int mb = 0; mb < 4; mb++) xp[(wave * 4 + kq) * 64 + 16 * mb + jn] = mb < NB ? xd[mb < NB ? mb : 0] : 0.f;
        __syncthreads();
    }
    // pose partial sums: the four vertex quads of a column are the four lanes of a DPP quad -- (q0 + q1) + (q2 + q3), fixed
    if (stager) {
#define FR_QUAD_SUM(x)                                                                                                         \
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true)); /* quad_perm [1,0,3,2] */       \
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true)); /* quad_perm [2,3,0,1] */
        FR_QUAD_SUM(ps0) FR_QUAD_SUM(ps1) FR_QUAD_SUM(ps2) FR_QUAD_SUM(ps3)
#undef FR_QUAD_SUM
        if (q == 0) {
            if (muf) {   // + this workgroup's share of alpha . d alpha + beta . d beta, waves ascending, kq ascending
                float t = 0.f;
                for (int w = 0; w < nwaves; w++)
#pragma unroll
                    for (int kk = 0; kk < 4; kk++) t += xp[(w * 4 + kk) * 64 + sb_];
                ps3 += t;
            }
            float* pp = a.pose_part + ((size_t)blockIdx.x * 64 + sb_) * 4;
            pp[0] = ps0; pp[1] = ps1; pp[2] = ps2; pp[3] = ps3 * m[12];
        }
    }
    // D tile of coefficient block i: row m = 4 * (lane >> 4) + reg is slot 16 (CB wave + i) + m, column (batch in block) = lane & 15
    float* slab = a.slab + (size_t)blockIdx.x * a.nslots * 64;
#pragma unroll
    for (int i = 0; i < CB; i++)
        if (i < nsb) {
#pragma unroll
            for (int mb = 0; mb < NB; mb++)
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int slot = 16 * (CB * wave + i) + 4 * kq + rg;
                    slab[(size_t)slot * 64 + 16 * mb + jn] = acc[i][mb][rg];
                }
        }
}
#undef FRB_LD
template <int NB, int CB>
__global__ __launch_bounds__(CB == 2 ? 512 : 256) void bwd_fused_kernel(BwdArgs a) {
    bwd_fused_body<NB, CB, false>(a);
}
// (its own __global__ name, not a third template argument of bwd_fused_kernel: tests/test_capi_cpu.py counts that kernel's
// instantiations by mangled prefix)
template <int NB, int CB>
__global__ __launch_bounds__(CB == 2 ? 512 : 256) void bwd_fused_z_kernel(BwdArgs a) {
    bwd_fused_body<NB, CB, true>(a);
}

// ---- fixed-order reduction of the partials ---------------------------------------------------------------------------------
// One 1024-thread workgroup per 64 consecutive outputs (output i = what*64 + batch: what 0..3 = d t3d / d f, 4.. = the
// padded coefficients).  Wave w sums its contiguous 1/16 of the partials with eight independent loads in flight per
// lane (the slabs are contiguous in i, so every load is a 256-byte row); the 16 wave sums meet in LDS and are added in
// wave order.  The association is fixed by (gemm_blocks, pre_blocks) alone, so the result is bit-reproducible.
constexpr int RED_WAVES = 16;
__global__ __launch_bounds__(RED_WAVES * 64) void bwd_reduce_kernel(BwdArgs a) {
    __shared__ float part[RED_WAVES][64];
    const int nd = FR_N_POSE + a.ns + a.ne;
    const int nslots = a.nslots;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int what = blockIdx.x, b = lane;  // i = what * 64 + b
    const float* src;
    size_t kstride;
    int nk;
    if (what < 4) {
        src = a.pose_part + (size_t)b * 4 + what;
        kstride = 64 * 4;
        nk = a.pre_blocks;
    } else {
        src = a.slab + (size_t)(what - 4) * 64 + b;
        kstride = (size_t)nslots * 64;
        nk = a.gemm_blocks;
    }
    const int per = (nk + RED_WAVES - 1) / RED_WAVES;
    const int k0 = wave * per, k1 = min(nk, k0 + per);
    float s[8];
#pragma unroll
    for (int u = 0; u < 8; u++) s[u] = 0.f;
    int k = k0;
    for (; k + 16 <= k1; k += 16) {   // sixteen loads in flight; s[u] still receives k0+u, k0+u+8, ... in that order
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = src[(size_t)(k + u) * kstride];
#pragma unroll
        for (int u = 0; u < 8; u++) s[u] += v[u];
#pragma unroll
        for (int u = 0; u < 8; u++) s[u] += v[8 + u];
    }
    for (; k + 8 <= k1; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = src[(size_t)(k + u) * kstride];
#pragma unroll
        for (int u = 0; u < 8; u++) s[u] += v[u];
    }
    for (; k < k1; k++) s[0] += src[(size_t)k * kstride];
    part[wave][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (wave != 0 || b >= a.nbatch) return;
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < RED_WAVES; w++) tot += part[w][lane];
    float* gp = a.grad_params + (size_t)(a.b0 + b) * nd;
    if (what < 3) {
        gp[3 + what] = tot;
        gp[what] = 0.0f;  // angles: no gradient through tf.py_func (network.py:150) -- the default; bwd_pose_finish_kernel overwrites it on request
    } else if (what == 3) {
        gp[6] = tot;
    } else {
        const int slot = what - 4, e0 = a.exp_slot0;   // shape slots [0, e0), expression slots from e0
        if (slot < e0) {
            if (slot < a.ns) gp[FR_N_POSE + slot] = tot;
        } else if (slot - e0 < a.ne) {
            gp[FR_N_POSE + a.ns + slot - e0] = tot;
        }
    }
}

struct BwdGeom {
    int pre_blocks, gemm_blocks, rows_per_block;
    size_t dv_bytes, pose_bytes, slab_bytes;
    // packed-image variant
    int sbs, sbt, rbt, rb_per_block, gemm_blocks_p, waves_p;
    int ngroups, groups_per_block, block_waves_p;   // packed path: vertex groups of 16, per workgroup; waves per workgroup
    int cb_p;                                       // packed path: 16-coefficient blocks per wave (2 or 4)
    size_t slab_bytes_p, at_bytes;
};
// (tests/test_decode_backward_bounds_gpu.py derives its error bounds from this geometry: it reads it through
// fr_debug_decode_bwd_geom, never from a copy of these rules)
static BwdGeom bwd_geom(int N, int ns = 199, int ne = 29) {
    BwdGeom g;
    g.pre_blocks = (N + BW_PV - 1) / BW_PV;
    const long long rows = 3ll * N;
    long long want = 512;
    long long rpb = (rows + want - 1) / want;
    rpb = ((rpb + 3) / 4) * 4;
    if (rpb < 4) rpb = 4;
    g.rows_per_block = (int)rpb;
    g.gemm_blocks = (int)((rows + rpb - 1) / rpb);
    // (dv rows padded to whole 16-row blocks: the packed variant reads them as 1 KiB fragments)
    g.rbt = (int)((rows + 15) / 16);
    g.dv_bytes = (size_t)g.rbt * 16 * 16 * sizeof(float4);
    g.sbs = (ns + 15) / 16;
    g.sbt = g.sbs + (ne + 15) / 16;
    g.waves_p = (g.sbt + 3) / 4;
    // Packed path: row chunks = workgroups = partial slabs: FR_BWD_CHUNKS, at most 512.  Default 256 = one four-wave workgroup per
    // CU of an MI355X (a constant, not the device's CU count: the chunking fixes the association of the sums, so the gradient's
    // bits must not depend on the part).  Round 4, same-process A/B through the autograd surface (round 3's prepass + ring GEMM):
    // 512 chunks 108.2 us, 256 chunks 96.0 us at 64 faces; 80.2 -> 76.4 us at 32; 384 and 128 are slower than both.  The slab /
    // partial space is sized for 512 chunks whatever the knob says, so that a workspace sized before it changed still fits.
    int chunks = opt(OPT_BWD_CHUNKS);
    if (chunks < 1 || chunks > 512) chunks = 256;
    g.ngroups = (N + 15) / 16;
    g.groups_per_block = (g.ngroups + chunks - 1) / chunks;
    if (g.groups_per_block < 1) g.groups_per_block = 1;
    g.gemm_blocks_p = g.ngroups > 0 ? (g.ngroups + g.groups_per_block - 1) / g.groups_per_block : 0;
    // FR_BWD_CB: 16-coefficient blocks per wave -- 2 (eight waves, two per SIMD), 4 (four waves), 0 = by batch (below).
    // Same-box runs through the autograd surface: 64 faces 77 us (2) vs 80 (4); 32 faces 73 (2) vs 67 (4).
    g.cb_p = opt(OPT_BWD_CB) == 4 ? 4 : 2;
    g.block_waves_p = (g.sbt + g.cb_p - 1) / g.cb_p;
    if (g.block_waves_p < 4) g.block_waves_p = 4;      // (the 256 staging threads of bwd_fused_kernel)
    {
        const int max_blocks = g.ngroups < 512 ? g.ngroups : 512;
        g.slab_bytes_p = (size_t)max_blocks * 64 * g.block_waves_p * 64 * sizeof(float);
        const size_t pose_p = (size_t)max_blocks * 64 * 4 * sizeof(float);
        const size_t pose_r = (size_t)g.pre_blocks * 64 * 4 * sizeof(float);
        g.pose_bytes = (((pose_p > pose_r ? pose_p : pose_r)) + 15) & ~(size_t)15;
    }
    g.at_bytes = (size_t)g.ngroups * 3 * g.sbt * 64 * sizeof(float4);
    g.slab_bytes = (size_t)g.gemm_blocks * 64 * bw_waves(ns, ne) * 64 * sizeof(float);
    return g;
}

// CB of one pass of nbatch (<= 64) faces: FR_BWD_CB 2 or 4, or 0 = by batch -- four blocks per wave up to 32 live columns,
// two beyond
static int bwd_pass_cb(int nbatch) {
    const int o = opt(OPT_BWD_CB);
    if (o == 0) return (nbatch + 15) / 16 <= 2 ? 4 : 2;
    return o == 4 ? 4 : 2;
}

}  // namespace fr

// test hook (include/fr_hotpath.h): the geometry the decode-backward launcher would choose under the current knobs, without a GPU.
// out = {vertex groups per fused workgroup, fused workgroups, CB of a pass of min(nbatch, 64) faces, waves per fused workgroup
// at that CB, rows per reference-layout GEMM workgroup, GEMM workgroups, prepass workgroups}
extern "C" void fr_debug_decode_bwd_geom(int nbatch, int N, int n_shape, int n_exp, int* out) {
    for (int i = 0; i < 7; i++) out[i] = 0;
    if (N <= 0 || n_shape < 0 || n_exp < 0) return;
    const fr::BwdGeom g = fr::bwd_geom(N, n_shape, n_exp);
    const int cb = fr::bwd_pass_cb(nbatch < 64 ? nbatch : 64);
    const int waves = (g.sbt + cb - 1) / cb;
    out[0] = g.groups_per_block; out[1] = g.gemm_blocks_p; out[2] = cb; out[3] = waves < 4 ? 4 : waves;
    out[4] = g.rows_per_block; out[5] = g.gemm_blocks; out[6] = g.pre_blocks;
}

size_t fr_decode_backward_workspace_impl(int N, int ns, int ne) {
    if (N <= 0) return 0;
    fr::BwdGeom g = fr::bwd_geom(N, ns, ne);
    return g.dv_bytes + g.pose_bytes + (g.slab_bytes > g.slab_bytes_p ? g.slab_bytes : g.slab_bytes_p);
}

// the packed path serves bases of at most 16 coefficient blocks (see bwd_fused_kernel)
static bool bwd_packed_supported(int ns, int ne) { return ns + ne > 0 && (ns + 15) / 16 + (ne + 15) / 16 <= 16; }
// ... and meshes of at least one whole 16-vertex tile: the fused kernel clamps a tile's origin to max(N - 16, 0) and always loads
// sixteen floats per row, which for N < 16 would run past the row (and, for the last batch's z row, past the tensor).  Smaller
// meshes take the reference-layout entry point (fr_decode_backward_basis_bytes answers 0 for them).
static bool bwd_packed_mesh_ok(int N) { return N >= 16; }

size_t fr_decode_backward_basis_bytes_impl(int N, int ns, int ne) {
    if (N <= 0 || !bwd_packed_supported(ns, ne) || !bwd_packed_mesh_ok(N)) return 0;
    return fr::bwd_geom(N, ns, ne).at_bytes;
}

int fr_launch_decode_backward_pack(const float* pc_shape, const float* pc_exp, int N, int ns, int ne, void* packed_t,
                                   hipStream_t stream) {
    using namespace fr;
    if (N <= 0 || ns + ne <= 0) return FR_OK;
    if (!bwd_packed_supported(ns, ne) || !bwd_packed_mesh_ok(N)) return FR_ERR_UNSUPPORTED;
    BwdGeom g = bwd_geom(N, ns, ne);
    hipLaunchKernelGGL(bwd_pack_kernel, dim3(2048), dim3(256), 0, stream, pc_shape, pc_exp, N, ns, ne, g.sbs, g.sbt,
                       (long long)g.ngroups, reinterpret_cast<float4*>(packed_t));
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_launch_decode_backward(const float* grad_vertex_proj, const float* params, const float* vertex_proj,
                              const float* pc_shape, const float* pc_exp, const float* R_override, int B, int N, int ns,
                              int ne, float im_size, float* grad_params, void* workspace, hipStream_t stream,
                              const void* packed_t, const float* mu, int zpitch) {
    using namespace fr;
    if (B == 0) return FR_OK;
    const int nd = FR_N_POSE + ns + ne;
    if (N == 0) return hipMemsetAsync(grad_params, 0, (size_t)B * nd * sizeof(float), stream) == hipSuccess ? FR_OK
                                                                                                             : FR_ERR_LAUNCH;
    BwdGeom g = bwd_geom(N, ns, ne);
    const bool packed = packed_t != nullptr;
    if (packed && (!bwd_packed_supported(ns, ne) || !bwd_packed_mesh_ok(N))) return FR_ERR_UNSUPPORTED;
    const int waves = packed ? g.waves_p : bw_waves(ns, ne);
    if (waves > BW_MAXWAVES) return FR_ERR_UNSUPPORTED;  // > 512 coefficient slots
    BwdArgs a;
    a.g = grad_vertex_proj; a.params = params; a.vproj = vertex_proj;
    a.pc_shape = pc_shape; a.pc_exp = pc_exp; a.R_override = R_override; a.grad_params = grad_params;
    char* ws = reinterpret_cast<char*>(workspace);
    a.dvT4 = reinterpret_cast<float4*>(ws);
    a.pose_part = reinterpret_cast<float*>(ws + g.dv_bytes);
    a.slab = reinterpret_cast<float*>(ws + g.dv_bytes + g.pose_bytes);
    a.B = B; a.N = N; a.ns = ns; a.ne = ne; a.im_size = im_size;
    a.pre_blocks = packed ? g.gemm_blocks_p : g.pre_blocks;   // (packed path: the fused kernel's workgroups write the pose partials)
    a.gemm_blocks = packed ? g.gemm_blocks_p : g.gemm_blocks; a.rows_per_block = g.rows_per_block;
    a.At = reinterpret_cast<const float4*>(packed_t);
    a.sbt = g.sbt; a.sbs = g.sbs;
    a.rbt = packed ? g.ngroups : g.rbt;
    a.rb_per_block = packed ? g.groups_per_block : g.rb_per_block;
    a.mu = packed ? mu : nullptr;   // (the mu form of d f exists on the packed path only)
    a.zpitch = zpitch;
    if (zpitch > 0 && !(packed && mu)) return FR_ERR_INVALID_ARG;   // (the z-only tile exists in the fused kernel's mu form only)
    a.exp_slot0 = packed ? 16 * g.sbs : bw_ns4(ns);
    a.nslots = packed ? 16 * g.cb_p * g.block_waves_p : 64 * bw_waves(ns, ne);
    for (int b0 = 0; b0 < B; b0 += 64) {
        a.b0 = b0;
        a.nbatch = min(B - b0, 64);
        const int nbt = (a.nbatch + 15) / 16;
        if (packed) {   // ONE launch: gradient tile -> dv rows in LDS -> MFMA reduction + the pose partial sums
            const int cb = bwd_pass_cb(a.nbatch);
            if (cb != g.cb_p) {
                g.cb_p = cb;
                g.block_waves_p = (g.sbt + cb - 1) / cb < 4 ? 4 : (g.sbt + cb - 1) / cb;
                a.nslots = 16 * cb * g.block_waves_p;
            }
            const dim3 gb(g.block_waves_p * 64);
#define FR_BWD_LAUNCH1(NBV, CBV)                                                                                      \
    {                                                                                                                 \
        if (zpitch > 0) hipLaunchKernelGGL((bwd_fused_z_kernel<NBV, CBV>), dim3(a.gemm_blocks), gb, 0, stream, a);   \
        else hipLaunchKernelGGL((bwd_fused_kernel<NBV, CBV>), dim3(a.gemm_blocks), gb, 0, stream, a);                 \
    }
#define FR_BWD_LAUNCH(NBV)                                                                                            \
    {                                                                                                                 \
        if (g.cb_p == 2) FR_BWD_LAUNCH1(NBV, 2)                                                                       \
        else FR_BWD_LAUNCH1(NBV, 4)                                                                                   \
    }
            if (nbt == 1) FR_BWD_LAUNCH(1)
            else if (nbt == 2) FR_BWD_LAUNCH(2)
            else if (nbt == 3) FR_BWD_LAUNCH(3)
            else FR_BWD_LAUNCH(4)
#undef FR_BWD_LAUNCH
#undef FR_BWD_LAUNCH1
        } else {
            hipLaunchKernelGGL(bwd_prepass_kernel, dim3(g.pre_blocks), dim3(256), 0, stream, a);
            if (waves > 0) {
                const dim3 gb(waves * 64);
                if (nbt == 1) hipLaunchKernelGGL(bwd_gemm_kernel<1>, dim3(g.gemm_blocks), gb, 0, stream, a);
                else if (nbt == 2) hipLaunchKernelGGL(bwd_gemm_kernel<2>, dim3(g.gemm_blocks), gb, 0, stream, a);
                else if (nbt == 3) hipLaunchKernelGGL(bwd_gemm_kernel<3>, dim3(g.gemm_blocks), gb, 0, stream, a);
                else hipLaunchKernelGGL(bwd_gemm_kernel<4>, dim3(g.gemm_blocks), gb, 0, stream, a);
            }
        }
        hipLaunchKernelGGL(bwd_reduce_kernel, dim3(4 + 64 * waves), dim3(RED_WAVES * 64), 0, stream, a);
    }
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

// ---- pose gradients: dL/dR and the three angles (opt-in; fr_decode_pose_backward, fr_decode_render_backward_pose) ----------------
// With q - t = f R v and dq = (g_x, -g_y, g_z), formed exactly as above:
//   pose moment  A[i][k] = sum_p dq_i,p (q_k,p - t_k)          (trace(A) / f is d f)
//   G = dL/dR    = f sum_p dq_p v_p^T = A R^-T = A cof(R) / det(R)      (cof(R) = R for a rotation; the cofactor form holds for
//                  any invertible R_override; f == 0 gives A = 0, G = 0: the true value; det(R) == 0 is DEFINED as G = 0)
//   d angle      = <G, d R / d angle>  with R = R_pitch R_yaw R_roll (network.py:276-290), only when the rotation is evaluated
//                  in-kernel; with R_override the angles do not enter the forward: exactly 0.
// Two launches, no float atomics (bit-reproducible):
//   bwd_pose_moment_kernel  streaming reduction, one workgroup per (face, chunk of PM_CHUNK vertices -- a constant of the code: the
//                           association of the sums depends on N alone, never on the batch or the part).  Thread t owns the vertex
//                           quads t, t + 256, ... of its chunk and adds their terms in ascending vertex order from +0; the wave total
//                           comes from wave_sum_to_lane63, the four waves meet in LDS and are added in wave order; one record of nine
//                           floats per (face, chunk) goes to the workspace.  DENSE: g and vertex_proj [B,3,N] -- N is odd for the
//                           model, so rows start at any 4-byte phase: the 16-byte loads are declared 4-byte aligned, and the one quad
//                           that straddles the row's end is loaded element by element.  ZONLY: g is the pitched z plane of the render
//                           backward, q the pitched vertex hand-off of the forward (both 128-byte aligned: one aligned 16-byte load
//                           per operand); rows 0 and 1 of A are +0 -- what the dense chain's sums of (+0) q and (-0) q from +0 give --
//                           so for finite inputs the record is bit-identical to the dense layout fed (0, 0, z).
//                           A slot without a vertex adds nothing (skipped, not 0 * x).
//   bwd_pose_finish_kernel  per face: chunk records summed in chunk order in float64, G and the angle derivatives in float64, ONE
//                           rounding to fp32; writes grad_R [B,3,3] and columns 0-2 of the face's grad_params row (the angle
//                           gradients, or zeros under R_override), no other column.
namespace fr {

constexpr int PM_THREADS = 256;                        // four waves
constexpr int PM_QPT = 2;                              // vertex quads per thread
constexpr int PM_CHUNK = PM_THREADS * PM_QPT * 4;      // 2,048 vertices per workgroup
// longest chain of rounded fp32 additions behind one element of a chunk record: a thread's 4 PM_QPT terms from +0 (the first
// addition is exact), six DPP steps of the wave sum, three additions across the four waves.  (The chunk records are then summed in float64.)
constexpr int PM_ADD_DEPTH = (4 * PM_QPT - 1) + 6 + 3;

struct PoseArgs {
    const float* g;          // DENSE [B,3,N]; ZONLY [B,pitch] (the z row)
    const float* q;          // DENSE [B,3,N] forward output; ZONLY [B,3,pitch] hand-off
    const float* params;     // [B,nd]
    const float* R_override; // [B,9] or null
    float* part;             // [B][chunks][9] chunk records
    float* grad_params;      // [B,nd] or null: columns 0-2 written
    float* grad_R;           // [B,9] or null
    int B, N, ns, ne, chunks;
    long long row;           // floats between the x / y / z rows of a face: N (DENSE) or the pitch (ZONLY)
    float im_size;
};

template <bool ZONLY>
__global__ __launch_bounds__(PM_THREADS) void bwd_pose_moment_kernel(PoseArgs a) {
    __shared__ float part[PM_THREADS / 64][9];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)(blockIdx.x / (unsigned)a.chunks), c = (int)(blockIdx.x % (unsigned)a.chunks);
    const int nd = FR_N_POSE + a.ns + a.ne;
    const int N = a.N;
    const float* pr = a.params + (size_t)b * nd;
    const float t0 = pr[3], t1 = pr[4], t2 = pr[5];
    const float* gb = a.g + (size_t)b * (ZONLY ? 1 : 3) * a.row;
    const float* qb = a.q + (size_t)b * 3 * a.row;
    constexpr int NG = ZONLY ? 1 : 3;
    f32x4 gv[PM_QPT][NG], qv[PM_QPT][3];
    // every load of the thread is requested before anything is added
#pragma unroll
    for (int i = 0; i < PM_QPT; i++) {
        const long long p0 = (long long)c * PM_CHUNK + 4ll * (tid + PM_THREADS * i);
        // DENSE: the whole quad lies inside the row.  ZONLY: the quad starts inside the row; its end is below the pitch (a multiple of 4)
        const bool vec = ZONLY ? p0 < N : p0 + 3 < N;
#pragma unroll
        for (int r = 0; r < NG; r++) gv[i][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; r++) qv[i][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (vec) {
            if constexpr (ZONLY) {
                gv[i][0] = *reinterpret_cast<const f32x4*>(gb + p0);
#pragma unroll
                for (int r = 0; r < 3; r++) qv[i][r] = *reinterpret_cast<const f32x4*>(qb + r * a.row + p0);
            } else {
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    gv[i][r] = *reinterpret_cast<const f32x4u4*>(gb + r * a.row + p0);
                    qv[i][r] = *reinterpret_cast<const f32x4u4*>(qb + r * a.row + p0);
                }
            }
        } else if (p0 < N) {   // (DENSE only) the quad that straddles the end of the rows
#pragma unroll
            for (int e = 0; e < 3; e++)
                if (p0 + e < N) {
#pragma unroll
                    for (int r = 0; r < NG; r++) gv[i][r][e] = gb[r * a.row + p0 + e];
#pragma unroll
                    for (int r = 0; r < 3; r++) qv[i][r][e] = qb[r * a.row + p0 + e];
                }
        }
    }
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = 0.f;
    const float imm1 = a.im_size - 1.0f;
#pragma unroll
    for (int i = 0; i < PM_QPT; i++) {
        const long long p0 = (long long)c * PM_CHUNK + 4ll * (tid + PM_THREADS * i);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (p0 + e < N) {
                // (q - t): q_0 = out_x, q_1 = (im - 1) - out_y, q_2 = out_z -- the expressions of bwd_fused_kernel
                const float q0 = qv[i][0][e] - t0;
                const float q1 = (imm1 - qv[i][1][e]) - t1;
                const float q2 = qv[i][2][e] - t2;
                if constexpr (!ZONLY) {
                    const float dq0 = gv[i][0][e], dq1 = -gv[i][1][e];
                    acc[0] += dq0 * q0; acc[1] += dq0 * q1; acc[2] += dq0 * q2;
                    acc[3] += dq1 * q0; acc[4] += dq1 * q1; acc[5] += dq1 * q2;
                }
                const float dq2 = gv[i][NG - 1][e];
                acc[6] += dq2 * q0; acc[7] += dq2 * q1; acc[8] += dq2 * q2;
            }
        }
    }
#pragma unroll
    for (int k = ZONLY ? 6 : 0; k < 9; k++) {
        const float s = wave_sum_to_lane63(acc[k]);
        if (lane == 63) part[wave][k] = s;
    }
    __syncthreads();
    if (tid < 9) {
        float s = 0.f;   // (ZONLY: rows 0 and 1 are +0)
        if (!ZONLY || tid >= 6) {
            s = part[0][tid];
#pragma unroll
            for (int w = 1; w < PM_THREADS / 64; w++) s += part[w][tid];
        }
        a.part[((size_t)b * a.chunks + c) * 9 + tid] = s;
    }
}

__device__ __forceinline__ void pose_mul3(const double* X, const double* Y, double* Z) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Z[3 * i + j] = (X[3 * i] * Y[j] + X[3 * i + 1] * Y[3 + j]) + X[3 * i + 2] * Y[6 + j];
}
__device__ __forceinline__ double pose_dot9(const double* X, const double* Y) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) s += X[i] * Y[i];
    return s;
}

__global__ __launch_bounds__(64) void bwd_pose_finish_kernel(PoseArgs a) {
    __shared__ double As[9];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < 9) {
        double s = 0.0;
        const float* src = a.part + (size_t)b * a.chunks * 9 + tid;
        for (int c = 0; c < a.chunks; c++) s += (double)src[(size_t)c * 9];
        As[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const int nd = FR_N_POSE + a.ns + a.ne;
    BwdArgs ba;   // (bwd_rotation reads these five fields: the fp32 rotation the forward used)
    ba.params = a.params; ba.R_override = a.R_override; ba.ns = a.ns; ba.ne = a.ne; ba.b0 = 0;
    float R9[9];
    bwd_rotation(ba, b, R9);
    double r[9], A[9], cf[9], G[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { r[i] = (double)R9[i]; A[i] = As[i]; }
    cf[0] = r[4] * r[8] - r[5] * r[7]; cf[1] = r[5] * r[6] - r[3] * r[8]; cf[2] = r[3] * r[7] - r[4] * r[6];
    cf[3] = r[2] * r[7] - r[1] * r[8]; cf[4] = r[0] * r[8] - r[2] * r[6]; cf[5] = r[1] * r[6] - r[0] * r[7];
    cf[6] = r[1] * r[5] - r[2] * r[4]; cf[7] = r[2] * r[3] - r[0] * r[5]; cf[8] = r[0] * r[4] - r[1] * r[3];
    const double det = (r[0] * cf[0] + r[1] * cf[1]) + r[2] * cf[2];
    pose_mul3(A, cf, G);
#pragma unroll
    for (int i = 0; i < 9; i++) G[i] = det == 0.0 ? 0.0 : G[i] / det;   // det(R) == 0: G := 0 (include/fr_hotpath.h)
    if (a.grad_R) {
#pragma unroll
        for (int i = 0; i < 9; i++) a.grad_R[(size_t)b * 9 + i] = (float)G[i];
    }
    if (a.grad_params) {
        float* gp = a.grad_params + (size_t)b * nd;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        if (!a.R_override && det != 0.0) {
            const float* pr = a.params + (size_t)b * nd;
            double sp, cp, sy, cy, st, ct;
            sincos((double)pr[0], &sp, &cp);
            sincos((double)pr[1], &sy, &cy);
            sincos((double)pr[2], &st, &ct);
            const double Rp[9] = {1, 0, 0, 0, cp, sp, 0, -sp, cp}, dRp[9] = {0, 0, 0, 0, -sp, cp, 0, -cp, -sp};
            const double Ry[9] = {cy, 0, -sy, 0, 1, 0, sy, 0, cy}, dRy[9] = {-sy, 0, -cy, 0, 0, 0, cy, 0, -sy};
            const double Rr[9] = {ct, st, 0, -st, ct, 0, 0, 0, 1}, dRr[9] = {-st, ct, 0, -ct, -st, 0, 0, 0, 0};
            double T[9], D[9];
            pose_mul3(dRp, Ry, T); pose_mul3(T, Rr, D); d0 = pose_dot9(G, D);
            pose_mul3(Rp, dRy, T); pose_mul3(T, Rr, D); d1 = pose_dot9(G, D);
            pose_mul3(Rp, Ry, T); pose_mul3(T, dRr, D); d2 = pose_dot9(G, D);
        }
        gp[0] = (float)d0; gp[1] = (float)d1; gp[2] = (float)d2;
    }
}

}  // namespace fr

// test hook (include/fr_hotpath.h): the pose-moment launch geometry, a function of N alone
extern "C" void fr_debug_pose_bwd_geom(int B, int N, int* out) {
    (void)B;
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (N <= 0) return;
    out[0] = fr::PM_CHUNK; out[1] = (int)(((long long)N + fr::PM_CHUNK - 1) / fr::PM_CHUNK); out[2] = fr::PM_THREADS;
    out[3] = fr::PM_ADD_DEPTH;
}

size_t fr_decode_pose_backward_workspace_impl(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    const size_t chunks = (size_t)(((long long)N + fr::PM_CHUNK - 1) / fr::PM_CHUNK);
    return ((size_t)B * chunks * 9 * sizeof(float) + 15) & ~(size_t)15;
}

// g / q: dense [B,3,N] tensors (pitch == 0), or the pitched z plane [B,pitch] and the pitched hand-off [B,3,pitch] (pitch > 0)
int fr_launch_decode_pose_backward(const float* g, const float* q, const float* params, const float* R_override, int B, int N,
                                   int ns, int ne, float im_size, float* grad_params, float* grad_R, void* workspace,
                                   hipStream_t stream, int pitch) {
    using namespace fr;
    if (B == 0) return FR_OK;
    PoseArgs a;
    a.g = g; a.q = q; a.params = params; a.R_override = R_override;
    a.part = reinterpret_cast<float*>(workspace); a.grad_params = grad_params; a.grad_R = grad_R;
    a.B = B; a.N = N; a.ns = ns; a.ne = ne; a.im_size = im_size;
    a.chunks = N > 0 ? (int)(((long long)N + PM_CHUNK - 1) / PM_CHUNK) : 0;
    a.row = pitch > 0 ? pitch : N;
    if ((long long)B * a.chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (a.chunks > 0) {
        const dim3 grid((unsigned)((long long)B * a.chunks));
        if (pitch > 0) hipLaunchKernelGGL(bwd_pose_moment_kernel<true>, grid, dim3(PM_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(bwd_pose_moment_kernel<false>, grid, dim3(PM_THREADS), 0, stream, a);
    }
    hipLaunchKernelGGL(bwd_pose_finish_kernel, dim3(B), dim3(64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
