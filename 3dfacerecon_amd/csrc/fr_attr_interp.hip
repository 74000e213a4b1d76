// Interpolated vertex attributes (opt-in; include/fr_hotpath.h, "smooth planes"): a three-channel per-vertex attribute (a texture, a
// vertex normal, the vertices themselves) evaluated at the pixel by the barycentric weights of the winning triangle, with gradients
// to the attribute and to the x and y of the triangle's vertices.  A post-pass over tri_ind, as fr_depth_interp.hip: which triangle
// wins a pixel stays the render forward's business.
//
//   ainterp_forward_kernel   one lane per pixel: triangle -> three vertex ids -> six vertex coordinates and nine attribute values
//                            (gathers out of L2), the weights of fr_point_weight.h, three stores.  No LDS, no atomics.
//   ainterp_records_kernel   the records pass of the owner-scatter scheme (fr_owner_scatter.h): the same gathers once, then the
//                            pixel's nine fp32 terms of each requested output -- one set of record planes and chunk maxima per
//                            output, so that an output's fixed-point scale is its own whether or not the other is asked for.
//   ainterp_owner_kernel     owner_rows3, launched once per requested output on that output's set.
#include "fr_owner_scatter.h"
#include "fr_point_weight.h"

namespace fr {

struct AinterpFwdArgs {
    const float* vertex;    // [B,3,vpitch]
    const float* attr;      // [B,3,apitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    float* out;             // [B,H,W,3]
    long long vpitch, apitch;
    int blocks;             // 256-pixel blocks of a face
    int nver, ntri, npix, W;
};

__global__ __launch_bounds__(256) void ainterp_forward_kernel(AinterpFwdArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int i = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (i >= a.npix) return;
    const size_t o = (size_t)b * a.npix + i;
    float r[3] = {0.0f, 0.0f, 0.0f};
    if (a.ntri > 0) {   // (an empty table has no triangle 0 to read)
        int id[3];
        const bool ok = pixel_tri_ids(a.tri_ind[o], a.tri, a.tri + a.ntri, a.tri + 2 * (size_t)a.ntri, a.ntri, a.nver, id).ok;
        if (ok) {
            float P[3][3], A[3][3];
            gather_tri(a.vertex + (size_t)b * 3 * a.vpitch, a.vpitch, id, P);
            gather_tri(a.attr + (size_t)b * 3 * a.apitch, a.apitch, id, A);
            const int row = i / a.W;
            const PointWeight s = point_weight(P, i - row * a.W, row);
#pragma unroll
            for (int c = 0; c < 3; c++)
                r[c] = s.flat ? div3((A[0][c] + A[1][c]) + A[2][c])
                              : (float)((s.w[0] * (double)A[0][c] + s.w[1] * (double)A[1][c]) + s.w[2] * (double)A[2][c]);
        }
    }
    float* __restrict__ out = a.out + 3 * o;
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2];
}

struct AinterpBwdArgs {
    const float* grad;      // [B,H,W,3]
    const float* vertex;    // [B,3,vpitch]
    const float* attr;      // [B,3,apitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    long long vpitch, apitch;
    int W;
    int ntri;
    OwnerRows3 oa, ov;      // the attribute's set and the vertex's (rec == NULL: not requested); they share the geometry
};

// The terms of one ok pixel (include/fr_hotpath.h): ta = {channel 0, 1, 2 of p1 | of p2 | of p3}, tv = {x, y, z of p1 | p2 | p3}.
template <bool ATTR, bool VERT>
__device__ __forceinline__ void ainterp_terms(const float (&P)[3][3], const float (&A)[3][3], const float (&g)[3], int px, int py,
                                              float (&ta)[9], float (&tv)[9]) {
    const PointWeight s = point_weight(P, px, py);
    if (s.flat) {   // the render's own texture lookup: a third of the gradient to each vertex, nothing through x and y
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (ATTR) ta[3 * k + c] = div3(g[c] * 1.0f);
                if (VERT) tv[3 * k + c] = 0.0f;
            }
        return;
    }
    const double G[3] = {(double)g[0], (double)g[1], (double)g[2]};
    if (ATTR) {
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) ta[3 * k + c] = (float)(G[c] * s.w[k]);
    }
    if (VERT) {
        const WeightSlopes q = weight_slopes(s);
        double Ax[3], Ay[3];   // channel c's screen-space slope
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double a1 = (double)A[0][c], d2 = (double)A[1][c] - a1, d3 = (double)A[2][c] - a1;
            Ax[c] = d2 * q.gvx + d3 * q.gux;
            Ay[c] = d2 * q.gvy + d3 * q.guy;
        }
        const double Sx = (G[0] * Ax[0] + G[1] * Ax[1]) + G[2] * Ax[2];
        const double Sy = (G[0] * Ay[0] + G[1] * Ay[1]) + G[2] * Ay[2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            tv[3 * k] = (float)(-(s.w[k] * Sx));
            tv[3 * k + 1] = (float)(-(s.w[k] * Sy));
            tv[3 * k + 2] = 0.0f;
        }
    }
}

// dinterp_records_kernel's shape: 256 threads x 4 lane-consecutive pixels, every gather issued before the first use
template <bool ATTR, bool VERT>
__global__ __launch_bounds__(256) void ainterp_records_kernel(AinterpBwdArgs a) {
    __shared__ uint32_t red[8];
    const OwnerRows3& o = ATTR ? a.oa : a.ov;
    const int chunks = o.chunks, npix = o.npix, nver = o.nver, ntri = a.ntri;
    const int b = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - b * chunks;
    const int tid = threadIdx.x;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    const float* __restrict__ gp = a.grad + (size_t)b * npix * 3;
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    const float* __restrict__ ab = a.attr + (size_t)b * 3 * a.apitch;
    int4* __restrict__ ra = ATTR ? a.oa.rec + (size_t)b * 3 * npix : nullptr;
    int4* __restrict__ rv = VERT ? a.ov.rec + (size_t)b * 3 * npix : nullptr;
    constexpr int PU = REC_PX / 256;
    const int i0 = ch * REC_PX + tid;
    float tq[PU], g[PU][3];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = min(i0 + u * 256, npix - 1);
        tq[u] = ti[i];
#pragma unroll
        for (int c = 0; c < 3; c++) g[u][c] = gp[3 * (size_t)i + c];
    }
    int id[PU][3];
    bool ok[PU];
#pragma unroll
    for (int u = 0; u < PU; u++) ok[u] = pixel_tri_ids(tq[u], tri0, tri1, tri2, ntri, nver, id[u]).ok && i0 + u * 256 < npix;
    float P[PU][3][3], A[PU][3][3];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int safe[3] = {ok[u] ? id[u][0] : 0, ok[u] ? id[u][1] : 0, ok[u] ? id[u][2] : 0};   // (nver > 0: the launcher's)
        gather_tri(vb, a.vpitch, safe, P[u]);
        if (VERT) gather_tri(ab, a.apitch, safe, A[u]);   // (the attribute's own gradient does not read the attribute)
    }
    uint32_t ma = 0, bada = 0, mv = 0, badv = 0;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = i0 + u * 256;
        if (i >= npix) continue;
        if (!ok[u]) {   // contributes nothing, its term planes are never read
            if (ATTR) ra[i] = make_int4(-1, 0, 0, 0);
            if (VERT) rv[i] = make_int4(-1, 0, 0, 0);
            continue;
        }
        float ta[9], tv[9];
        const int row = i / a.W;
        ainterp_terms<ATTR, VERT>(P[u], A[u], g[u], i - row * a.W, row, ta, tv);
        if (ATTR) {
#pragma unroll
            for (int j = 0; j < 9; j++) track_term(__float_as_uint(ta[j]), ma, bada);
            store_rows3(ra, ra + npix, ra + 2 * (size_t)npix, i, id[u], ta);
        }
        if (VERT) {
#pragma unroll
            for (int j = 0; j < 9; j++) track_term(__float_as_uint(tv[j]), mv, badv);
            store_rows3(rv, rv + npix, rv + 2 * (size_t)npix, i, id[u], tv);
        }
    }
    if (ATTR) chunk_publish(ma, bada, red, a.oa.partial + (size_t)b * chunks + ch);
    if (ATTR && VERT) __syncthreads();   // (red is read by every thread of the first reduction before the second writes it)
    if (VERT) chunk_publish(mv, badv, red, a.ov.partial + (size_t)b * chunks + ch);
}

__global__ __launch_bounds__(OWNER_BLOCK) void ainterp_owner_kernel(OwnerRows3 o) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // all LDS is dynamic: owner_rows3's
    owner_rows3(o, acc);
}

}  // namespace fr

// ---- C ABI (include/fr_hotpath.h) ---------------------------------------------------------------------------------------------
extern "C" {

int fr_attr_interp_forward(const float* vertex, int vertex_pitch, const float* attr, int attr_pitch, const float* tri,
                           const float* tri_ind, int B, int nver, int ntri, int H, int W, float* out, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0 || vertex_pitch < nver || attr_pitch < nver) return FR_ERR_INVALID_ARG;
    const long long npix = (long long)H * W;
    if (B == 0 || npix == 0) return FR_OK;
    if (!tri_ind || !out || (ntri > 0 && (!tri || (nver > 0 && (!vertex || !attr))))) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;   // float-stored ids stop being exact
    const long long blocks = (npix + 255) / 256;
    if (npix > 0x7FFFFFFFll || (long long)B * blocks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    AinterpFwdArgs a;
    a.vertex = vertex; a.attr = attr; a.tri = tri; a.tri_ind = tri_ind; a.out = out; a.vpitch = vertex_pitch; a.apitch = attr_pitch;
    a.blocks = (int)blocks; a.nver = nver; a.ntri = ntri; a.npix = (int)npix; a.W = W;
    hipLaunchKernelGGL(ainterp_forward_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

// out[6] as fr_debug_depth_interp_bwd_geom; all zero for a shape that launches no kernel or is refused
void fr_debug_attr_interp_bwd_geom(int B, int nver, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll) return;
    fr::owner_geom_report(fr::rows3_geom(B, nver, npix), B, out);
}

int fr_attr_interp_backward(const float* grad, const float* vertex, int vertex_pitch, const float* attr, int attr_pitch,
                            const float* tri, const float* tri_ind, float* attr_grad, int attr_accumulate, float* vertex_grad,
                            int vertex_accumulate, int B, int nver, int ntri, int H, int W, int* records, unsigned int* partial,
                            void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if ((attr_accumulate != 0 && attr_accumulate != 1) || (vertex_accumulate != 0 && vertex_accumulate != 1)) return FR_ERR_INVALID_ARG;
    if (vertex_pitch < nver || attr_pitch < nver) return FR_ERR_INVALID_ARG;
    const long long npix = (long long)H * W;
    if (B == 0 || npix == 0) return FR_OK;
    if (nver == 0) return FR_OK;   // empty gradients: nothing to write
    if (!attr_grad && !vertex_grad) return FR_ERR_INVALID_ARG;
    if (ntri > 0 && (!grad || !vertex || !attr || !tri || !tri_ind)) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24) || npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (ntri > 0 && (!records || ((uintptr_t)records & 15) || !partial || ((uintptr_t)partial & 7))) return FR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t out_bytes = (size_t)B * 3 * nver * sizeof(float);
    if (ntri == 0) {
        const int rc = attr_grad ? owner_no_terms(attr_grad, out_bytes, attr_accumulate, st) : FR_OK;
        return rc != FR_OK || !vertex_grad ? rc : owner_no_terms(vertex_grad, out_bytes, vertex_accumulate, st);
    }
    const OwnerGeom geo = rows3_geom(B, nver, npix);
    if ((long long)B * geo.splits > 0x7FFFFFFFll || (long long)B * geo.chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    AinterpBwdArgs a;
    a.grad = grad; a.vertex = vertex; a.vpitch = vertex_pitch; a.attr = attr; a.apitch = attr_pitch; a.tri = tri; a.tri_ind = tri_ind;
    a.W = W; a.ntri = ntri;
    // set 0 is the attribute's, set 1 the vertex's, whichever are requested
    const size_t set_rec = (size_t)B * 3 * npix, set_partial = (size_t)B * geo.chunks;
    OwnerRows3 o;
    o.B = B; o.chunks = geo.chunks; o.nver = nver; o.npix = (int)npix;
    o.splits = geo.splits; o.range = geo.range; o.shift = geo.shift;
    a.oa = o; a.ov = o;
    a.oa.rec = attr_grad ? reinterpret_cast<int4*>(records) : nullptr;
    a.oa.partial = reinterpret_cast<uint2*>(partial);
    a.oa.vertex_grad = attr_grad; a.oa.accumulate = attr_accumulate;
    a.ov.rec = vertex_grad ? reinterpret_cast<int4*>(records) + set_rec : nullptr;
    a.ov.partial = reinterpret_cast<uint2*>(partial) + set_partial;
    a.ov.vertex_grad = vertex_grad; a.ov.accumulate = vertex_accumulate;
    const dim3 grid((unsigned)(B * geo.chunks));
    if (attr_grad && vertex_grad) hipLaunchKernelGGL((ainterp_records_kernel<true, true>), grid, dim3(256), 0, st, a);
    else if (attr_grad) hipLaunchKernelGGL((ainterp_records_kernel<true, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ainterp_records_kernel<false, true>), grid, dim3(256), 0, st, a);
    static fr_lds_flags_t lds_ok[64];
    if (fr_allow_full_lds(reinterpret_cast<const void*>(&ainterp_owner_kernel), lds_ok) != hipSuccess) return FR_ERR_LAUNCH;
    if (attr_grad) hipLaunchKernelGGL(ainterp_owner_kernel, dim3((unsigned)(B * geo.splits)), dim3(OWNER_BLOCK), geo.lds, st, a.oa);
    if (vertex_grad) hipLaunchKernelGGL(ainterp_owner_kernel, dim3((unsigned)(B * geo.splits)), dim3(OWNER_BLOCK), geo.lds, st, a.ov);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
