// The owner-scatter scheme of the render backwards, stated once.  fr_render_bwd.hip (depth), fr_render_nbwd.hip (normal),
// fr_render_tbwd.hip (texture), fr_depth_interp.hip (interpolated depth) and fr_attr_interp.hip (interpolated attributes) are built from these pieces; none of the pieces knows which gradient it serves -- what differs
// between them enters as a template parameter, a value or a functor.
//
// The scheme: a pixel covered by triangle t adds fp32 terms to the three vertices of t.  The reference is a serial loop (one
// fixed summation order); float atomics would make the per-vertex order depend on the schedule.  Here the sum is made
// ORDER-INDEPENDENT instead:
//   records pass   one pass over the batch's pixels resolves each pixel's triangle to its three vertex ids (the scattered
//                  gathers, done once) and writes 16-byte planes of per-pixel records, the first {p1, p2, p3, term} with
//                  p1 = -1 for a pixel that contributes nothing; per 1,024-pixel chunk it publishes the largest finite |term|
//                  and a non-finite flag.
//   owner pass     one workgroup owns one (group, vertex range) pair -- a group is a face, or a slice of faces: it STREAMS the id
//                  plane of its group and keeps only the terms that land in its range, so no two workgroups ever add to the same
//                  element and nothing needs zeroing.  Every term is converted EXACTLY to a 64-bit fixed-point integer (term * 2^k
//                  is exact in double; one rounding to the grid), the integers are added with LDS integer atomics (associative =>
//                  bit-reproducible whatever the order), and the total is rounded to fp32 once.  k is chosen per scope from the
//                  published maxima so that the scope's largest term lands just below 2^TOP, under the int64 headroom the
//                  possible terms need.
// A scope with an Inf / NaN term cannot be scaled: it takes float atomics in the same LDS (the class of the result -- NaN /
// +-Inf -- does not depend on the order; its bits do).
#pragma once
#include "fr_common.h"

namespace fr {

constexpr int OWNER_BLOCK = 1024;     // threads of an owner workgroup
constexpr int REC_PX = 1024;          // pixels per records-kernel workgroup (256 threads x 4)
constexpr int OWNER_TARGET_WG = 256;  // owner workgroups aimed at: one per CU

// ---- which pixel contributes ---------------------------------------------------------------------------------------------------
// the triangle of pixel value `tv` (a float-stored triangle index, -1 on the background), or -1: the pixel is not covered
__device__ __forceinline__ int pixel_tri(float tv, int ntri) {
    const int t = f2i_x86(tv);
    return (t >= 0 && t < ntri) ? t : -1;
}

// the three vertex ids of pixel value `tv` (an uncovered pixel reads triangle 0: the gathers stay in bounds and unconditional).
// covered: the pixel names a triangle of the table; ok: and all three of its ids lie in [0, nver) -- only an ok pixel contributes.
struct PixelTri {
    bool covered, ok;
};
__device__ __forceinline__ PixelTri pixel_tri_ids(float tv, const float* __restrict__ tri0, const float* __restrict__ tri1,
                                                  const float* __restrict__ tri2, int ntri, int nver, int (&ids)[3]) {
    const int t = pixel_tri(tv, ntri);
    const int tt = max(t, 0);
    ids[0] = f2i_x86(tri0[tt]); ids[1] = f2i_x86(tri1[tt]); ids[2] = f2i_x86(tri2[tt]);
    const bool ok = t >= 0 && (unsigned)ids[0] < (unsigned)nver && (unsigned)ids[1] < (unsigned)nver && (unsigned)ids[2] < (unsigned)nver;
    return {t >= 0, ok};
}

// ---- the largest finite |term| and the non-finite flag -------------------------------------------------------------------------
__device__ __forceinline__ void track_term(uint32_t bits, uint32_t& m, uint32_t& bad) {
    const uint32_t v = bits & 0x7FFFFFFFu;
    if (v >= 0x7F800000u) bad = 1; else m = max(m, v);
}

// {max of m, or of bad} over the NT threads of the workgroup, the same value in every thread; red: 2 * NT / 64 words of LDS
template <int NT>
__device__ __forceinline__ uint2 block_max(uint32_t m, uint32_t bad, uint32_t* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m = max(m, (uint32_t)__shfl_xor((int)m, d));
        bad |= (uint32_t)__shfl_xor((int)bad, d);
    }
    if (lane == 0) { red[wave] = m; red[NT / 64 + wave] = bad; }
    __syncthreads();
    m = 0; bad = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) { m = max(m, red[w]); bad |= red[NT / 64 + w]; }
    return make_uint2(m, bad);
}

// tail of a records kernel (256 threads): the chunk's {largest finite |term| bits, non-finite flag} to its slot; red: 8 words
__device__ __forceinline__ void chunk_publish(uint32_t m, uint32_t bad, uint32_t* red, uint2* partial_slot) {
    const uint2 mb = block_max<256>(m, bad, red);
    if (threadIdx.x == 0) *partial_slot = mb;
}

// head of an owner: the scope's {largest finite |term| bits, non-finite flag} from `count` chunk records
template <int NT>
__device__ __forceinline__ uint2 scope_max(const uint2* __restrict__ partial, int count, uint32_t* red) {
    uint32_t m = 0, bad = 0;
    for (int c = threadIdx.x; c < count; c += NT) {
        const uint2 pm = partial[c];
        m = max(m, pm.x); bad |= pm.y;
    }
    return block_max<NT>(m, bad, red);
}

// ---- block -> (group, owner) ---------------------------------------------------------------------------------------------------
// Blocks that share blockIdx % 8 share an XCD and its L2: with a group count that is a multiple of 8 the owners of a group are given
// ids of one residue class, so the group's planes / records are fetched into ONE L2 and re-read there, instead of once per owner.
__host__ __device__ inline bool owner_xcd_map(int groups) { return (groups & 7) == 0; }
__device__ __forceinline__ void owner_block_map(int groups, int splits, int* group, int* owner) {
    if (owner_xcd_map(groups)) {
        const int xcd = (int)blockIdx.x & 7, q = (int)blockIdx.x >> 3;
        *group = (q / splits) * 8 + xcd;
        *owner = q % splits;
    } else {
        *group = (int)blockIdx.x / splits;
        *owner = (int)blockIdx.x - *group * splits;
    }
}

// ---- the fixed-point contract --------------------------------------------------------------------------------------------------
// Scale 2^k from e = floor(log2 M), M the scope's largest finite |term| given by its bits `m` (-127 for subnormals / zero): M lands
// in [2^(TOP-shift), 2^(TOP+1-shift)).  `shift`: headroom bits given up by scopes of more than 2^20 pixels (owner_geom).
template <int TOP>
struct FixedScale {
    double scale, inv_scale;
    __device__ __forceinline__ FixedScale(uint32_t m, int shift) {
        const int e = (int)(m >> 23) - 127;
        scale = ldexp(1.0, TOP - shift - e);
        inv_scale = ldexp(1.0, e - TOP + shift);
    }
    // the term has 24 significant bits and the scale is a power of two: the product is exact, one rounding to the grid
    __device__ __forceinline__ unsigned long long to_fixed(float t) const {
        return (unsigned long long)__double2ll_rn((double)t * scale);
    }
    // fixed point -> fp32: one rounding to 24 bits (int64 -> fp32), then an exact power-of-two scaling in double (one more
    // rounding only where the result is subnormal)
    __device__ __forceinline__ float round(unsigned long long s) const { return (float)((double)(float)(long long)s * inv_scale); }
};
// one term to one LDS accumulator (integer addition: exact, any order)
__device__ __forceinline__ void fixed_add(unsigned long long* slot, unsigned long long q) {
    if (q) atomicAdd(slot, q);
}

// ---- the owner's record stream -------------------------------------------------------------------------------------------------
// Streams the `npix` records of id plane `r0` through the workgroup, eight per lane per trip with all loads issued before the first
// use, and calls f(i, q0, in1, in2, in3) for the pixels that contribute to [v0, v1): q0 = r0[i] = {p1, p2, p3, term}, in_k = p_k is
// owned.  Ownership first: every owner of a group sees every pixel, but only ~1 / splits of them land in its range -- whatever else
// a pixel needs (a division, further planes, the fixed-point conversion) is done for those only.
template <int NT, class F>
__device__ __forceinline__ void owner_stream(const int4* __restrict__ r0, int npix, int v0, int v1, F&& f) {
    constexpr int QU = 8;
    for (int i0 = threadIdx.x; i0 < npix; i0 += QU * NT) {
        int4 q0[QU];
#pragma unroll
        for (int u = 0; u < QU; u++) q0[u] = r0[min(i0 + u * NT, npix - 1)];
#pragma unroll
        for (int u = 0; u < QU; u++) {
            const int i = i0 + u * NT;
            const int p1 = q0[u].x, p2 = q0[u].y, p3 = q0[u].z;
            if (i >= npix || p1 < 0) continue;
            const bool in1 = p1 >= v0 && p1 < v1, in2 = p2 >= v0 && p2 < v1, in3 = p3 >= v0 && p3 < v1;
            if (!(in1 || in2 || in3)) continue;
            f(i, q0[u], in1, in2, in3);
        }
    }
}

// ---- the owner of nine terms per pixel over three rows --------------------------------------------------------------------------
// What the normal backward (fr_render_nbwd.hip) and the interpolated-depth backward (fr_depth_interp.hip) share beyond the pieces
// above: their records kernels differ (what a term is), their owner is this one.  Record planes [B][3][npix] of 16 bytes:
// {p1 p2 p3 t1x | t1y t1z t2x t2y | t2z t3x t3y t3z}, t_k the (x, y, z) terms of vertex p_k; vertex_grad dense [B,3,nver].
constexpr int ROWS3_RANGE_MAX = 6656;  // vertices per owner: 3 accumulators x 8 B each = 156 KiB of the CU's 160 KiB of LDS
constexpr int ROWS3_TOP = 39;          // the face's largest finite |term| lands in [2^39, 2^40); an element receives at most three terms
                                       // per pixel (a triangle naming one vertex three times), 3 * 2^20 of them stay below 2^62
struct OwnerRows3 {
    int4* rec;
    uint2* partial;         // [B,chunks] {largest finite |term| bits, non-finite flag}
    float* vertex_grad;
    int B, chunks, nver, npix;
    int splits, range, shift;
    int accumulate;
};
// one workgroup of OWNER_BLOCK threads per (face, vertex range); acc: the kernel's dynamic LDS (the launcher raises the limit to the
// CU's 160 KiB): [3][range] 64-bit accumulators, then the reduction array
__device__ __forceinline__ void owner_rows3(const OwnerRows3& a, unsigned long long* acc) {
    uint32_t* red = reinterpret_cast<uint32_t*>(acc + 3 * (size_t)a.range);  // [2 * OWNER_BLOCK / 64]
    const int tid = threadIdx.x;
    int b, sp;
    owner_block_map(a.B, a.splits, &b, &sp);
    const int range = a.range, npix = a.npix, nver = a.nver;
    const int v0 = sp * range;
    const int v1 = min(nver, v0 + range);
    const int n = v1 - v0;
    for (int i = tid; i < 3 * range; i += OWNER_BLOCK) acc[i] = 0ull;
    const uint2 mb = scope_max<OWNER_BLOCK>(a.partial + (size_t)b * a.chunks, a.chunks, red);
    const uint32_t m = mb.x, bad = mb.y;
    const FixedScale<ROWS3_TOP> fx(m, a.shift);
    float* facc = reinterpret_cast<float*>(acc);   // a face with an Inf / NaN term: fp32 LDS atomics, [3][range] floats
    if (bad) {
        __syncthreads();
        for (int i = tid; i < 3 * range; i += OWNER_BLOCK) facc[i] = 0.0f;
    }
    __syncthreads();
    const int4* __restrict__ r0 = a.rec + (size_t)b * 3 * npix;
    const int4* __restrict__ r1 = r0 + npix;
    const int4* __restrict__ r2 = r1 + npix;
    auto add3 = [&](int local, float tx, float ty, float tz) {
        if (bad) {
            atomicAdd(&facc[local], tx);
            atomicAdd(&facc[range + local], ty);
            atomicAdd(&facc[2 * range + local], tz);
        } else {
            const unsigned long long qx = fx.to_fixed(tx), qy = fx.to_fixed(ty), qz = fx.to_fixed(tz);
            fixed_add(&acc[local], qx);
            fixed_add(&acc[range + local], qy);
            fixed_add(&acc[2 * range + local], qz);
        }
    };
    if (m != 0 || bad) {
        // the two term planes are fetched for the pixels that land in this range only
        owner_stream<OWNER_BLOCK>(r0, npix, v0, v1, [&](int i, const int4& q0, bool in1, bool in2, bool in3) {
            const int4 q1 = r1[i], q2 = r2[i];
            if (in1) add3(q0.x - v0, __int_as_float(q0.w), __int_as_float(q1.x), __int_as_float(q1.y));
            if (in2) add3(q0.y - v0, __int_as_float(q1.z), __int_as_float(q1.w), __int_as_float(q2.x));
            if (in3) add3(q0.z - v0, __int_as_float(q2.y), __int_as_float(q2.z), __int_as_float(q2.w));
        });
    }
    __syncthreads();
    float* out = a.vertex_grad + (size_t)b * 3 * nver;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float* row = out + (size_t)c * nver + v0;
        for (int i = tid; i < n; i += OWNER_BLOCK) {
            const float v = bad ? facc[c * range + i] : fx.round(acc[c * range + i]);
            row[i] = a.accumulate ? row[i] + v : v;
        }
    }
}
// the nine fp32 terms of an ok pixel to its three record planes
__device__ __forceinline__ void store_rows3(int4* __restrict__ r0, int4* __restrict__ r1, int4* __restrict__ r2, int i,
                                            const int (&id)[3], const float (&t)[9]) {
    r0[i] = make_int4(id[0], id[1], id[2], (int)__float_as_uint(t[0]));
    r1[i] = make_int4((int)__float_as_uint(t[1]), (int)__float_as_uint(t[2]), (int)__float_as_uint(t[3]), (int)__float_as_uint(t[4]));
    r2[i] = make_int4((int)__float_as_uint(t[5]), (int)__float_as_uint(t[6]), (int)__float_as_uint(t[7]), (int)__float_as_uint(t[8]));
}

// ---- host: the launch geometry -------------------------------------------------------------------------------------------------
struct OwnerGeom {
    int splits, range;  // owner workgroups per group, vertices per owner
    int shift;          // headroom bits given up by scopes above 2^20 pixels
    int chunks;         // 1,024-pixel chunks of a face in the records kernel
    size_t lds;         // dynamic LDS of an owner
};
// groups: what the owners of one vertex range are multiplied by (parallelism); npix: pixels of a face; terms: pixels of a scope (an
// element receives at most three terms per pixel: a triangle naming one vertex three times); range_max: vertices per owner the
// LDS holds at `accs` 8-byte accumulators each; range_min: no owner streams a whole id plane for fewer vertices than this
inline OwnerGeom owner_geom(int groups, int nver, long long npix, long long terms, int range_max, int range_min, int accs) {
    OwnerGeom g{};
    // the int64 headroom covers 3 * 2^20 terms per element at the full resolution; larger scopes give up one bit of resolution per
    // doubling (the forward renders such images through the scan fallback, so the backward must take them too)
    while ((1ll << (20 + g.shift)) < terms) g.shift++;
    // owners per group: enough for the LDS budget, and for ~one workgroup per CU on small batches
    int splits = (nver + range_max - 1) / range_max;
    const int want = (OWNER_TARGET_WG + groups - 1) / groups;
    if (splits < want) splits = want;
    const int most = (nver + range_min - 1) / range_min;
    if (splits > most) splits = most;
    g.range = (nver + splits - 1) / splits;
    g.splits = (nver + g.range - 1) / g.range;
    g.chunks = (int)((npix + REC_PX - 1) / REC_PX);
    g.lds = (size_t)accs * g.range * sizeof(unsigned long long) + 2 * (OWNER_BLOCK / 64) * sizeof(uint32_t) + 16;
    return g;
}
// a test hook's common part: out = {owners per group, vertices per owner, shift, chunks, LDS bytes of an owner, XCD-map flag}
inline void owner_geom_report(const OwnerGeom& g, int groups, int* out) {
    out[0] = g.splits; out[1] = g.range; out[2] = g.shift; out[3] = g.chunks; out[4] = (int)g.lds; out[5] = owner_xcd_map(groups) ? 1 : 0;
}
// the three-row owner's geometry (the splits are clamped to one vertex per owner) and the workspace of its call: the three record
// planes, then the chunk partials
inline OwnerGeom rows3_geom(int B, int nver, long long npix) { return owner_geom(B, nver, npix, npix, ROWS3_RANGE_MAX, 1, 3); }
inline size_t rows3_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t npix = (size_t)H * W, chunks = (npix + REC_PX - 1) / REC_PX;
    return (size_t)B * npix * 3 * sizeof(int4) + (size_t)B * chunks * sizeof(uint2);
}
// no term exists: zeros, or (accumulate) the tensor as it is
inline int owner_no_terms(float* out, size_t bytes, bool accumulate, hipStream_t stream) {
    if (accumulate || !bytes) return FR_OK;
    return hipMemsetAsync(out, 0, bytes, stream) == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // namespace fr
