// render_depth texture backward (opt-in; include/fr_hotpath.h, "texture gradients"): the adjoint of the rasteriser's texture
// lookup tritex_c = (t_c[p1] + t_c[p2] + t_c[p3]) / 3.0f -- the gradient of the op's `tex_img` plane with respect to `texture`.
// The reference has no such gradient (its "LSE for alpha" block, nets/network.py:436-445, gives up on exactly this scatter).
//
// The owner-scatter scheme of fr_owner_scatter.h with one term per row and pixel (every vertex of the triangle receives all three):
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
#include "fr_owner_scatter.h"

namespace fr {

constexpr int TB_BLOCK = OWNER_BLOCK;
constexpr int TB_RANGE_MAX = 6656;  // vertices per owner: 3 accumulators x 8 B each = 156 KiB of the CU's 160 KiB of LDS
constexpr int TB_RANGE_MIN = 256;   // no owner streams a whole id plane for fewer vertices than this (a small mesh: one owner)
constexpr int TB_TOP = 39;          // the scope's largest finite |term| lands in [2^(39-shift), 2^(40-shift)); an element receives at
                                    // most three terms per pixel (a triangle naming one vertex three times), 3 * 2^(20+shift) of them
                                    // stay below 2^62

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
    const int tid = threadIdx.x;
    const int npix = a.npix, ntri = a.ntri, nver = a.nver;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    const float* __restrict__ gp = a.tgrad + (size_t)b * npix * a.gstride;
    int4* __restrict__ r0 = a.rec0 + (size_t)b * npix;
    uint2* __restrict__ r1 = a.rec1 + (size_t)b * npix;
    constexpr int PU = REC_PX / 256;
    const int i0 = ch * REC_PX + tid;   // lane-consecutive pixels: a gather instruction's 64 lanes hold neighbouring triangles
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
        int id[3];
        const bool ok = pixel_tri_ids(tq[u], tri0, tri1, tri2, ntri, nver, id).ok;
        if (i >= npix) continue;
        if (!ok) {   // background, a triangle index or a vertex id out of range: contributes nothing, its second plane is never read
            r0[i] = make_int4(-1, 0, 0, 0);
            continue;
        }
        uint32_t tb[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            tb[c] = __float_as_uint(div3(g[u][c]));   // the forward's own division (fr_common.h)
            track_term(tb[c], m, bad);                // over the OK pixels
        }
        r0[i] = make_int4(id[0], id[1], id[2], (int)tb[0]);
        r1[i] = make_uint2(tb[1], tb[2]);
    }
    chunk_publish(m, bad, red, &a.partial[(size_t)b * a.chunks + ch]);
}

__global__ __launch_bounds__(TB_BLOCK) void tbwd_owner_kernel(TbwdArgs a) {
    // all LDS is dynamic (the launcher raises the limit to the CU's 160 KiB): [3][range] accumulators, then the reduction array
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // [3 * range]
    uint32_t* red = reinterpret_cast<uint32_t*>(acc + 3 * (size_t)a.range);  // [2 * TB_BLOCK / 64]
    const int tid = threadIdx.x;
    int gr, sp;
    owner_block_map(a.groups, a.splits, &gr, &sp);
    const int range = a.range, npix = a.npix, nver = a.nver;
    const int v0 = sp * range;
    const int v1 = min(nver, v0 + range);
    const int n = v1 - v0;
    const int b0 = gr * a.fpg, b1 = min(a.B, b0 + a.fpg);
    for (int i = tid; i < 3 * range; i += TB_BLOCK) acc[i] = 0ull;   // (+0.0 as a double as well)
    // the scope's scale: one face, or the whole batch for the shared texture
    const uint2 mb = a.shared ? scope_max<TB_BLOCK>(a.partial, a.B * a.chunks, red)
                              : scope_max<TB_BLOCK>(a.partial + (size_t)gr * a.chunks, a.chunks, red);
    const uint32_t m = mb.x, bad = mb.y;
    const FixedScale<TB_TOP> fx(m, a.shift);
    double* dacc = reinterpret_cast<double*>(acc);   // a scope with an Inf / NaN term: float64 LDS atomics in the same array
    __syncthreads();
    auto add1 = [&](int slot, float t) {
        if (bad) atomicAdd(&dacc[slot], (double)t);
        else fixed_add(&acc[slot], fx.to_fixed(t));
    };
    if (m != 0 || bad) {
        for (int b = b0; b < b1; b++) {
            const uint2* __restrict__ r1 = a.rec1 + (size_t)b * npix;
            // the second plane is fetched for the pixels that land in this range only
            owner_stream<TB_BLOCK>(a.rec0 + (size_t)b * npix, npix, v0, v1, [&](int i, const int4& q0, bool in1, bool in2, bool in3) {
                const uint2 q1 = r1[i];
                const float t0 = __int_as_float(q0.w), t1 = __uint_as_float(q1.x), t2 = __uint_as_float(q1.y);
                // every vertex of the triangle receives the pixel's term of each row (one vertex named three times: three)
                const int p1 = q0.x - v0, p2 = q0.y - v0, p3 = q0.z - v0;
                if (in1) { add1(p1, t0); add1(range + p1, t1); add1(2 * range + p1, t2); }
                if (in2) { add1(p2, t0); add1(range + p2, t1); add1(2 * range + p2, t2); }
                if (in3) { add1(p3, t0); add1(range + p3, t1); add1(2 * range + p3, t2); }
            });
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
            const float v = bad ? (float)dacc[c * range + i] : fx.round(acc[c * range + i]);
            row[i] = a.accumulate ? row[i] + v : v;
        }
    }
}

__global__ __launch_bounds__(256) void tbwd_finish_kernel(TbwdArgs a) {
    __shared__ uint32_t red[8];
    const uint2 mb = scope_max<256>(a.partial, a.B * a.chunks, red);
    const FixedScale<TB_TOP> fx(mb.x, a.shift);
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
        v = fx.round(s);
    }
    a.texture_grad[i] = a.accumulate ? a.texture_grad[i] + v : v;
}

}  // namespace fr

// The launch geometry, chosen in ONE place: the launcher, the workspace size and the test hook all read it from here.
namespace {
struct TbwdGeom : fr::OwnerGeom {
    int slices, fpg;   // face slices (0: no cross-face reduction) and faces per slice
    bool shared;
    int groups(int B) const { return shared ? slices : B; }
};
TbwdGeom tbwd_geom(int B, int nver, long long npix, int tex_batch) {
    using namespace fr;
    const bool shared = tex_batch == 1 && B > 1;   // (one face: its own scope either way)
    TbwdGeom g{owner_geom(B, nver, npix, shared ? (long long)B * npix : npix, TB_RANGE_MAX, TB_RANGE_MIN, 3), 0, 1, shared};
    if (g.shared) {
        // face slices: every slice costs a [3][nver] slab written and read once (8 bytes an element), every face of a slice is
        // one more pass of its owners over an id plane -- as many slices as keep ~one workgroup per CU, no more
        int slices = OWNER_TARGET_WG / g.splits;
        if (slices < 1) slices = 1;
        if (slices > B) slices = B;
        g.fpg = (B + slices - 1) / slices;
        g.slices = (B + g.fpg - 1) / g.fpg;
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
    fr::owner_geom_report(g, g.groups(B), out);
    out[6] = g.slices;
}

int fr_launch_render_texture_backward(const float* tex_grad, int grad_stride, const float* tri, const float* tri_ind,
                                      float* texture_grad, int B, int nver, int ntri, int H, int W, int tex_batch, int accumulate,
                                      void* workspace, hipStream_t stream) {
    using namespace fr;
    const long long npix = (long long)H * W;
    if (npix == 0 || ntri == 0) return owner_no_terms(texture_grad, (size_t)tex_batch * 3 * nver * sizeof(float), accumulate, stream);
    if (npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    const TbwdGeom geo = tbwd_geom(B, nver, npix, tex_batch);
    const int groups = geo.groups(B);
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
