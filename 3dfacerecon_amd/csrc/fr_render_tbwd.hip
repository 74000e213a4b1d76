// render_depth texture backward (opt-in; include/fr_hotpath.h, "texture gradients"): the adjoint of the rasteriser's texture
// lookup tritex_c = (t_c[p1] + t_c[p2] + t_c[p3]) / 3.0f -- the gradient of the op's `tex_img` plane with respect to `texture`.
// The reference has no such gradient (its "LSE for alpha" block, nets/network.py:436-445, gives up on exactly this scatter).
//
// The scheme of fr_render_nbwd.hip with one term per row instead of three per vertex:
//   tbwd_records_kernel   one pass over the batch's pixels: triangle -> three vertex ids (the only gathers of the call, done once),
//                         the pixel's three fp32 terms div3(g_c), written as a 16-byte plane {p1 p2 p3 term0} and an 8-byte plane
//                         {term1 term2}; the largest finite |term| and a non-finite flag per 1,024-pixel chunk.
//   tbwd_owner_kernel     one workgroup per (face group, vertex range): streams the id plane of its faces, fetches the second plane
//                         of the pixels that land in its range only, and adds the terms as 64-bit fixed-point integers to three LDS
//                         accumulators per owned vertex (integer addition: exact, any order).
//                           tex_batch == B: a group is one face and the owner rounds and writes its part of texture_grad itself;
//                           tex_batch == 1: a group is a slice of consecutive faces and the owner stores its raw 64-bit slab
//                                           [3][range] in the workspace with plain stores;
//   tbwd_finish_kernel    (tex_batch == 1 only) adds a vertex's slabs over the slices -- integers again -- and rounds once.
// No two workgroups write the same element, nothing needs zeroing, no float atomics on the finite path.  A scope with an Inf / NaN
// term takes float64 LDS atomics in the same accumulators (the bits are then not predictable, the classes and the bound are).
#include "fr_common.h"

namespace fr {

constexpr int TB_BLOCK = 1024;
constexpr int TB_RANGE_MAX = 6656;  // vertices per owner: 3 accumulators x 8 B each = 156 KiB of the CU's 160 KiB of LDS
constexpr int TB_REC_PX = 1024;     // pixels per records-kernel workgroup (256 threads x 4)
constexpr int TB_TARGET_WG = 256;   // owner workgroups aimed at: one per CU
constexpr int TB_RANGE_MIN = 256;   // ... but no owner streams a whole id plane for fewer vertices than this (a small mesh: one owner)

struct TbwdArgs {
    const float* tgrad;     // three floats per pixel, `gstride` floats between pixels
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    float* texture_grad;    // [tex_batch,3,nver]
    int4* rec0;             // [B][npix] {p1, p2, p3, term0}
    uint2* rec1;            // [B][npix] {term1, term2}
    uint2* partial;         // [B,chunks] {largest finite |term| bits, non-finite flag}
    unsigned long long* slab;  // [slices][3][nver] (shared texture only)
    int gstride;
    int B, chunks, nver, ntri, npix;
    int splits, range, shift;
    int groups, fpg;        // face groups and faces per group: (B, 1) per face, (slices, ceil(B / slices)) for the shared texture
    int shared, accumulate;
};

__global__ __launch_bounds__(256) void tbwd_records_kernel(TbwdArgs a) {
    __shared__ uint32_t red[8];
    const int b = (int)blockIdx.x / a.chunks, ch = (int)blockIdx.x - b * a.chunks;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npix = a.npix, ntri = a.ntri, nver = a.nver;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    const float* __restrict__ gp = a.tgrad + (size_t)b * npix * a.gstride;
    int4* __restrict__ r0 = a.rec0 + (size_t)b * npix;
    uint2* __restrict__ r1 = a.rec1 + (size_t)b * npix;
    constexpr int PU = TB_REC_PX / 256;
    const int i0 = ch * TB_REC_PX + tid;   // lane-consecutive pixels: a gather instruction's 64 lanes hold neighbouring triangles
    float tq[PU], g[PU][3];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = min(i0 + u * 256, npix - 1);
        tq[u] = ti[i];
        const float* gi = gp + (size_t)i * a.gstride;
        g[u][0] = gi[0]; g[u][1] = gi[1]; g[u][2] = gi[2];
    }
    uint32_t m = 0, bad = 0;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = i0 + u * 256;
        const int t = f2i_x86(tq[u]);
        const bool covered = t >= 0 && t < ntri && i < npix;
        const int tt = covered ? t : 0;
        const int p1 = f2i_x86(tri0[tt]), p2 = f2i_x86(tri1[tt]), p3 = f2i_x86(tri2[tt]);
        const bool ok = covered && (unsigned)p1 < (unsigned)nver && (unsigned)p2 < (unsigned)nver && (unsigned)p3 < (unsigned)nver;
        if (i >= npix) continue;
        if (!ok) {   // background, a triangle index or a vertex id out of range: contributes nothing, its second plane is never read
            r0[i] = make_int4(-1, 0, 0, 0);
            continue;
        }
        uint32_t tb[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            tb[c] = __float_as_uint(div3(g[u][c]));   // the forward's own division (fr_common.h)
            const uint32_t v = tb[c] & 0x7FFFFFFFu;
            if (v >= 0x7F800000u) bad = 1; else m = max(m, v);
        }
        r0[i] = make_int4(p1, p2, p3, (int)tb[0]);
        r1[i] = make_uint2(tb[1], tb[2]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m = max(m, (uint32_t)__shfl_xor((int)m, d));
        bad |= (uint32_t)__shfl_xor((int)bad, d);
    }
    if (lane == 0) { red[wave] = m; red[4 + wave] = bad; }
    __syncthreads();
    if (tid == 0)
        a.partial[(size_t)b * a.chunks + ch] = make_uint2(max(max(red[0], red[1]), max(red[2], red[3])),
                                                          red[4] | red[5] | red[6] | red[7]);
}

// {largest finite |term| bits, non-finite flag} of `count` chunk records, the same value in every thread of the workgroup;
// red: 2 * NT / 64 words of LDS
template <int NT>
__device__ __forceinline__ uint2 tbwd_scope_max(const uint2* __restrict__ partial, int count, uint32_t* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t m = 0, bad = 0;
    for (int c = tid; c < count; c += NT) {
        const uint2 pm = partial[c];
        m = max(m, pm.x); bad |= pm.y;
    }
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

// fixed point -> fp32: one rounding to 24 bits (int64 -> fp32), then an exact power-of-two scaling in double (one more rounding
// only where the result is subnormal)
__device__ __forceinline__ float tbwd_round(unsigned long long s, double inv_scale) {
    return (float)((double)(float)(long long)s * inv_scale);
}

__global__ __launch_bounds__(TB_BLOCK) void tbwd_owner_kernel(TbwdArgs a) {
    // all LDS is dynamic (the launcher raises the limit to the CU's 160 KiB): [3][range] accumulators, then the reduction array
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // [3 * range]
    uint32_t* red = reinterpret_cast<uint32_t*>(acc + 3 * (size_t)a.range);  // [2 * TB_BLOCK / 64]
    const int tid = threadIdx.x;
    // block -> (group, owner) as in nbwd_owner_kernel: with a group count that is a multiple of 8 the owners of a group share
    // blockIdx % 8, hence an XCD and its L2, where the group's records are fetched once and re-read by the other owners
    int gr, sp;
    if ((a.groups & 7) == 0) {
        const int xcd = (int)blockIdx.x & 7, q = (int)blockIdx.x >> 3;
        gr = (q / a.splits) * 8 + xcd;
        sp = q % a.splits;
    } else {
        gr = (int)blockIdx.x / a.splits;
        sp = (int)blockIdx.x - gr * a.splits;
    }
    const int range = a.range, npix = a.npix, nver = a.nver;
    const int v0 = sp * range;
    const int v1 = min(nver, v0 + range);
    const int n = v1 - v0;
    const int b0 = gr * a.fpg, b1 = min(a.B, b0 + a.fpg);
    for (int i = tid; i < 3 * range; i += TB_BLOCK) acc[i] = 0ull;   // (+0.0 as a double as well)
    // the scope's scale: one face, or the whole batch for the shared texture
    const uint2 mb = a.shared ? tbwd_scope_max<TB_BLOCK>(a.partial, a.B * a.chunks, red)
                              : tbwd_scope_max<TB_BLOCK>(a.partial + (size_t)gr * a.chunks, a.chunks, red);
    const uint32_t m = mb.x, bad = mb.y;
    // scale 2^k from e = floor(log2 M), M the scope's largest finite |term|: M lands in [2^(39-shift), 2^(40-shift)); an element
    // receives at most three terms per pixel (a triangle naming one vertex three times), 3 * 2^(20+shift) of them stay below 2^62
    const int e = (int)(m >> 23) - 127;
    const double scale = ldexp(1.0, 39 - a.shift - e);
    const double inv_scale = ldexp(1.0, e - 39 + a.shift);
    double* dacc = reinterpret_cast<double*>(acc);   // a scope with an Inf / NaN term: float64 LDS atomics in the same array
    __syncthreads();
    auto add1 = [&](int slot, float t) {
        if (bad) {
            atomicAdd(&dacc[slot], (double)t);
        } else {
            // the term has 24 significant bits and the scale is a power of two: the product is exact, one rounding to the grid
            const unsigned long long q = (unsigned long long)__double2ll_rn((double)t * scale);
            if (q) atomicAdd(&acc[slot], q);
        }
    };
    if (m != 0 || bad) {
        constexpr int QU = 8;
        for (int b = b0; b < b1; b++) {
            const int4* __restrict__ r0 = a.rec0 + (size_t)b * npix;
            const uint2* __restrict__ r1 = a.rec1 + (size_t)b * npix;
            for (int i0 = tid; i0 < npix; i0 += QU * TB_BLOCK) {
                int4 q0[QU];
#pragma unroll
                for (int u = 0; u < QU; u++) q0[u] = r0[min(i0 + u * TB_BLOCK, npix - 1)];
#pragma unroll
                for (int u = 0; u < QU; u++) {
                    const int i = i0 + u * TB_BLOCK;
                    const int p1 = q0[u].x, p2 = q0[u].y, p3 = q0[u].z;
                    if (i >= npix || p1 < 0) continue;
                    // ownership first: every owner sees every pixel, ~1 / splits of them land in its range -- the second plane
                    // is fetched for those only
                    const bool in1 = p1 >= v0 && p1 < v1, in2 = p2 >= v0 && p2 < v1, in3 = p3 >= v0 && p3 < v1;
                    if (!(in1 || in2 || in3)) continue;
                    const uint2 q1 = r1[i];
                    const float t0 = __int_as_float(q0[u].w), t1 = __uint_as_float(q1.x), t2 = __uint_as_float(q1.y);
                    // every vertex of the triangle receives the pixel's term of each row (one vertex named three times: three)
                    if (in1) { add1(p1 - v0, t0); add1(range + p1 - v0, t1); add1(2 * range + p1 - v0, t2); }
                    if (in2) { add1(p2 - v0, t0); add1(range + p2 - v0, t1); add1(2 * range + p2 - v0, t2); }
                    if (in3) { add1(p3 - v0, t0); add1(range + p3 - v0, t1); add1(2 * range + p3 - v0, t2); }
                }
            }
        }
    }
    __syncthreads();
    if (a.shared) {   // the raw sums (integers, or doubles of a non-finite scope) go to this slice's slab; the finish kernel rounds
        unsigned long long* out = a.slab + (size_t)gr * 3 * nver;
#pragma unroll
        for (int c = 0; c < 3; c++)
            for (int i = tid; i < n; i += TB_BLOCK) out[(size_t)c * nver + v0 + i] = acc[c * range + i];
        return;
    }
    float* out = a.texture_grad + (size_t)gr * 3 * nver;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float* row = out + (size_t)c * nver + v0;
        for (int i = tid; i < n; i += TB_BLOCK) {
            const float v = bad ? (float)dacc[c * range + i] : tbwd_round(acc[c * range + i], inv_scale);
            row[i] = a.accumulate ? row[i] + v : v;
        }
    }
}

__global__ __launch_bounds__(256) void tbwd_finish_kernel(TbwdArgs a) {
    __shared__ uint32_t red[8];
    const uint2 mb = tbwd_scope_max<256>(a.partial, a.B * a.chunks, red);
    const int e = (int)(mb.x >> 23) - 127;
    const double inv_scale = ldexp(1.0, e - 39 + a.shift);
    const size_t total = 3 * (size_t)a.nver;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v;
    if (mb.y) {   // slices in ascending order
        double s = 0.0;
        for (int k = 0; k < a.groups; k++) s = s + __longlong_as_double((long long)a.slab[(size_t)k * total + i]);
        v = (float)s;
    } else {
        unsigned long long s = 0ull;
        for (int k = 0; k < a.groups; k++) s += a.slab[(size_t)k * total + i];
        v = tbwd_round(s, inv_scale);
    }
    a.texture_grad[i] = a.accumulate ? a.texture_grad[i] + v : v;
}

}  // namespace fr

// The launch geometry, chosen in ONE place: the launcher, the workspace size and the test hook all read it from here.
namespace {
struct TbwdGeom {
    int splits, range, shift, chunks, slices, fpg;
    size_t lds;
    bool xcd_map, shared;
};
TbwdGeom tbwd_geom(int B, int nver, long long npix, int tex_batch) {
    using namespace fr;
    TbwdGeom g{};
    g.shared = tex_batch == 1 && B > 1;   // (one face: its own scope either way)
    const long long count = g.shared ? (long long)B * npix : npix;
    while ((1ll << (20 + g.shift)) < count) g.shift++;
    // owners per face: enough for the LDS budget, and for ~one workgroup per CU on small batches
    int splits = (nver + TB_RANGE_MAX - 1) / TB_RANGE_MAX;
    const int want = (TB_TARGET_WG + B - 1) / B;
    if (splits < want) splits = want;
    const int most = (nver + TB_RANGE_MIN - 1) / TB_RANGE_MIN;
    if (splits > most) splits = most;
    g.range = (nver + splits - 1) / splits;
    g.splits = (nver + g.range - 1) / g.range;
    g.chunks = (int)((npix + TB_REC_PX - 1) / TB_REC_PX);
    g.lds = 3 * (size_t)g.range * sizeof(unsigned long long) + 2 * (TB_BLOCK / 64) * sizeof(uint32_t) + 16;
    if (g.shared) {
        // face slices: every slice costs a [3][nver] slab written and read once (8 bytes an element), every face of a slice is
        // one more pass of its owners over an id plane -- as many slices as keep ~one workgroup per CU, no more
        int slices = TB_TARGET_WG / g.splits;
        if (slices < 1) slices = 1;
        if (slices > B) slices = B;
        g.fpg = (B + slices - 1) / slices;
        g.slices = (B + g.fpg - 1) / g.fpg;
        g.xcd_map = (g.slices & 7) == 0;
    } else {
        g.fpg = 1;
        g.xcd_map = (B & 7) == 0;
    }
    return g;
}
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
}  // namespace

size_t fr_render_texture_backward_workspace_impl(int B, int nver, int H, int W, int tex_batch) {
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0) return 0;
    const size_t npix = (size_t)H * W;
    const TbwdGeom g = tbwd_geom(B, nver, (long long)npix, tex_batch);
    return (size_t)B * npix * (sizeof(int4) + sizeof(uint2)) + up16((size_t)B * g.chunks * sizeof(uint2)) +
           (size_t)g.slices * 3 * (size_t)nver * sizeof(unsigned long long);
}

// test hook (tests/test_texture_backward_*.py): out = {owners per face (or per face slice), vertices per owner, shift, 1,024-pixel
// record chunks per face, LDS bytes of an owner, XCD-map flag, face slices (0: no cross-face reduction)}; all zero for a shape that
// launches no kernel or is refused
extern "C" void fr_debug_render_texture_bwd_geom(int B, int nver, int H, int W, int tex_batch, int* out) {
    for (int i = 0; i < 7; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll || (tex_batch != 1 && tex_batch != B)) return;
    const TbwdGeom g = tbwd_geom(B, nver, npix, tex_batch);
    out[0] = g.splits; out[1] = g.range; out[2] = g.shift; out[3] = g.chunks; out[4] = (int)g.lds; out[5] = g.xcd_map ? 1 : 0;
    out[6] = g.slices;
}

int fr_launch_render_texture_backward(const float* tex_grad, int grad_stride, const float* tri, const float* tri_ind,
                                      float* texture_grad, int B, int nver, int ntri, int H, int W, int tex_batch, int accumulate,
                                      void* workspace, hipStream_t stream) {
    using namespace fr;
    const long long npix = (long long)H * W;
    if (npix == 0 || ntri == 0) {   // no term exists: zeros, or the tensor as it is
        if (accumulate) return FR_OK;
        return hipMemsetAsync(texture_grad, 0, (size_t)tex_batch * 3 * nver * sizeof(float), stream) == hipSuccess ? FR_OK
                                                                                                                 : FR_ERR_LAUNCH;
    }
    if (npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    const TbwdGeom geo = tbwd_geom(B, nver, npix, tex_batch);
    const int groups = geo.shared ? geo.slices : B;
    if ((long long)groups * geo.splits > 0x7FFFFFFFll || (long long)B * geo.chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    TbwdArgs a;
    a.tgrad = tex_grad; a.gstride = grad_stride; a.tri = tri; a.tri_ind = tri_ind; a.texture_grad = texture_grad;
    char* ws = reinterpret_cast<char*>(workspace);
    a.rec0 = reinterpret_cast<int4*>(ws);
    ws += (size_t)B * npix * sizeof(int4);
    a.rec1 = reinterpret_cast<uint2*>(ws);
    ws += (size_t)B * npix * sizeof(uint2);
    a.partial = reinterpret_cast<uint2*>(ws);
    ws += up16((size_t)B * geo.chunks * sizeof(uint2));
    a.slab = reinterpret_cast<unsigned long long*>(ws);
    a.B = B; a.chunks = geo.chunks; a.nver = nver; a.ntri = ntri; a.npix = (int)npix;
    a.splits = geo.splits; a.range = geo.range; a.shift = geo.shift;
    a.groups = groups; a.fpg = geo.fpg; a.shared = geo.shared ? 1 : 0; a.accumulate = accumulate;
    static fr_lds_flags_t lds_ok[64];
    hipLaunchKernelGGL(tbwd_records_kernel, dim3((unsigned)(B * geo.chunks)), dim3(256), 0, stream, a);
    if (fr_allow_full_lds(reinterpret_cast<const void*>(&tbwd_owner_kernel), lds_ok) != hipSuccess) return FR_ERR_LAUNCH;
    hipLaunchKernelGGL(tbwd_owner_kernel, dim3((unsigned)(groups * geo.splits)), dim3(TB_BLOCK), geo.lds, stream, a);
    if (geo.shared) {
        const size_t total = 3 * (size_t)nver;
        hipLaunchKernelGGL(tbwd_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    }
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
