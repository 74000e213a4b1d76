// Interpolated depth (opt-in; include/fr_hotpath.h, "interpolated depth"): the z of the winning triangle's plane at the pixel,
// by the barycentric weights the reference's get_point_weight (render_depth_op.cc:29-74) computes and nothing calls, and its
// gradient with respect to all three coordinates of the triangle's vertices.  A post-pass over tri_ind: which triangle wins a
// pixel stays the render forward's business (the flat h), this file only re-evaluates the depth of the winner.
//
//   dinterp_forward_kernel   one lane per pixel: triangle -> three vertex ids -> nine vertex coordinates (gathers out of L2:
//                            neighbouring lanes hold neighbouring triangles), ~40 fp64 operations, one store.  No LDS, no atomics.
//   dinterp_records_kernel   the records pass of the owner-scatter scheme (fr_owner_scatter.h): the same gathers once, the pixel's
//                            nine fp32 terms, the three record planes of the normal backward.
//   dinterp_owner_kernel     owner_rows3: the normal backward's owner, instantiated here for this file's records.
#include "fr_owner_scatter.h"
#include "fr_point_weight.h"

namespace fr {

struct DinterpFwdArgs {
    const float* vertex;    // [B,3,vpitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    float* depth;           // [B,H,W,1]
    long long vpitch;
    int blocks;             // 256-pixel blocks of a face
    int nver, ntri, npix, W;
};

__global__ __launch_bounds__(256) void dinterp_forward_kernel(DinterpFwdArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int i = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (i >= a.npix) return;
    const size_t o = (size_t)b * a.npix + i;
    float d = bg_depth();
    if (a.ntri > 0) {   // (an empty table has no triangle 0 to read)
        int id[3];
        const bool ok = pixel_tri_ids(a.tri_ind[o], a.tri, a.tri + a.ntri, a.tri + 2 * (size_t)a.ntri, a.ntri, a.nver, id).ok;
        if (ok) {
            float P[3][3];
            gather_tri(a.vertex + (size_t)b * 3 * a.vpitch, a.vpitch, id, P);
            const int row = i / a.W;
            const PointWeight s = point_weight(P, i - row * a.W, row);
            const double z1 = (double)P[0][2], z2 = (double)P[1][2], z3 = (double)P[2][2];
            d = s.flat ? div3((P[0][2] + P[1][2]) + P[2][2]) : (float)((s.w[0] * z1 + s.w[1] * z2) + s.w[2] * z3);
        }
    }
    a.depth[o] = d;
}

struct DinterpBwdArgs {
    const float* dgrad;     // [B,H,W,1]
    const float* vertex;    // [B,3,vpitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    long long vpitch;
    int W;
    int ntri;
    OwnerRows3 o;
};

// The nine terms of one ok pixel (include/fr_hotpath.h): t = {x, y, z of p1 | of p2 | of p3}.
__device__ __forceinline__ void dinterp_terms(const float (&P)[3][3], float g, int px, int py, float (&t)[9]) {
    const PointWeight s = point_weight(P, px, py);
    if (s.flat) {   // the flat backward's term on the z row, nothing on x and y
        const float z = div3(g * 1.0f);
#pragma unroll
        for (int k = 0; k < 3; k++) { t[3 * k] = 0.0f; t[3 * k + 1] = 0.0f; t[3 * k + 2] = z; }
        return;
    }
    const WeightSlopes q = weight_slopes(s);
    const double z1 = (double)P[0][2], d2 = (double)P[1][2] - z1, d3 = (double)P[2][2] - z1;
    const double Ax = d2 * q.gvx + d3 * q.gux, Ay = d2 * q.gvy + d3 * q.guy;   // the plane's screen-space slope
    const double G = (double)g;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double c = G * s.w[k];
        t[3 * k] = (float)(-(c * Ax));
        t[3 * k + 1] = (float)(-(c * Ay));
        t[3 * k + 2] = (float)c;
    }
}

// nbwd_records_kernel's shape: 256 threads x 4 lane-consecutive pixels, every gather issued before the first use
__global__ __launch_bounds__(256) void dinterp_records_kernel(DinterpBwdArgs a) {
    __shared__ uint32_t red[8];
    const int chunks = a.o.chunks, npix = a.o.npix, nver = a.o.nver, ntri = a.ntri;
    const int b = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - b * chunks;
    const int tid = threadIdx.x;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    const float* __restrict__ gp = a.dgrad + (size_t)b * npix;
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    int4* __restrict__ r0 = a.o.rec + (size_t)b * 3 * npix;
    int4* __restrict__ r1 = r0 + npix;
    int4* __restrict__ r2 = r1 + npix;
    constexpr int PU = REC_PX / 256;
    const int i0 = ch * REC_PX + tid;
    float tq[PU], g[PU];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = min(i0 + u * 256, npix - 1);
        tq[u] = ti[i];
        g[u] = gp[i];
    }
    int id[PU][3];
    bool ok[PU];
#pragma unroll
    for (int u = 0; u < PU; u++) ok[u] = pixel_tri_ids(tq[u], tri0, tri1, tri2, ntri, nver, id[u]).ok && i0 + u * 256 < npix;
    float P[PU][3][3];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int safe[3] = {ok[u] ? id[u][0] : 0, ok[u] ? id[u][1] : 0, ok[u] ? id[u][2] : 0};   // (nver > 0: the launcher's)
        gather_tri(vb, a.vpitch, safe, P[u]);
    }
    uint32_t m = 0, bad = 0;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = i0 + u * 256;
        if (i >= npix) continue;
        if (!ok[u]) {   // contributes nothing, its term planes are never read
            r0[i] = make_int4(-1, 0, 0, 0);
            continue;
        }
        float t[9];
        const int row = i / a.W;
        dinterp_terms(P[u], g[u], i - row * a.W, row, t);
#pragma unroll
        for (int j = 0; j < 9; j++) track_term(__float_as_uint(t[j]), m, bad);
        store_rows3(r0, r1, r2, i, id[u], t);
    }
    chunk_publish(m, bad, red, a.o.partial + (size_t)b * chunks + ch);
}

__global__ __launch_bounds__(OWNER_BLOCK) void dinterp_owner_kernel(OwnerRows3 o) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // all LDS is dynamic: owner_rows3's
    owner_rows3(o, acc);
}

}  // namespace fr

// ---- C ABI (include/fr_hotpath.h) ---------------------------------------------------------------------------------------------
extern "C" {

int fr_depth_interp_forward(const float* vertex, int vertex_pitch, const float* tri, const float* tri_ind, int B, int nver,
                            int ntri, int H, int W, float* depth, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0 || vertex_pitch < nver) return FR_ERR_INVALID_ARG;
    const long long npix = (long long)H * W;
    if (B == 0 || npix == 0) return FR_OK;
    if (!tri_ind || !depth || (ntri > 0 && (!tri || (nver > 0 && !vertex)))) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;   // float-stored ids stop being exact
    const long long blocks = (npix + 255) / 256;
    if (npix > 0x7FFFFFFFll || (long long)B * blocks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    DinterpFwdArgs a;
    a.vertex = vertex; a.tri = tri; a.tri_ind = tri_ind; a.depth = depth; a.vpitch = vertex_pitch;
    a.blocks = (int)blocks; a.nver = nver; a.ntri = ntri; a.npix = (int)npix; a.W = W;
    hipLaunchKernelGGL(dinterp_forward_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

size_t fr_depth_interp_backward_workspace_bytes(int B, int nver, int H, int W) {
    (void)nver;
    return fr::rows3_workspace_bytes(B, H, W);
}

// out = {owners per face, vertices per owner, shift, 1,024-pixel record chunks, LDS bytes of an owner, XCD-map flag}; all zero for
// a shape that launches no kernel or is refused
void fr_debug_depth_interp_bwd_geom(int B, int nver, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll) return;
    fr::owner_geom_report(fr::rows3_geom(B, nver, npix), B, out);
}

int fr_depth_interp_backward(const float* depth_grad, const float* vertex, int vertex_pitch, const float* tri,
                             const float* tri_ind, float* vertex_grad, int B, int nver, int ntri, int H, int W, int accumulate,
                             void* workspace, size_t ws_bytes, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if ((accumulate != 0 && accumulate != 1) || vertex_pitch < nver) return FR_ERR_INVALID_ARG;
    const long long npix = (long long)H * W;
    if (B == 0 || npix == 0) return FR_OK;
    if (nver == 0) return FR_OK;   // an empty vertex_grad: nothing to write
    if (!vertex_grad) return FR_ERR_INVALID_ARG;
    if (ntri > 0 && (!depth_grad || !vertex || !tri || !tri_ind)) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24) || npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (ntri > 0 && !ws_ok(workspace, ws_bytes, rows3_workspace_bytes(B, H, W), 16)) return FR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (ntri == 0) return owner_no_terms(vertex_grad, (size_t)B * 3 * nver * sizeof(float), accumulate, st);
    const OwnerGeom geo = rows3_geom(B, nver, npix);
    if ((long long)B * geo.splits > 0x7FFFFFFFll || (long long)B * geo.chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    DinterpBwdArgs a;
    a.dgrad = depth_grad; a.vertex = vertex; a.vpitch = vertex_pitch; a.tri = tri; a.tri_ind = tri_ind; a.W = W; a.ntri = ntri;
    int4* rec = reinterpret_cast<int4*>(workspace);
    a.o.rec = rec;
    a.o.partial = reinterpret_cast<uint2*>(rec + (size_t)B * 3 * npix);
    a.o.vertex_grad = vertex_grad;
    a.o.B = B; a.o.chunks = geo.chunks; a.o.nver = nver; a.o.npix = (int)npix;
    a.o.splits = geo.splits; a.o.range = geo.range; a.o.shift = geo.shift; a.o.accumulate = accumulate;
    static fr_lds_flags_t lds_ok[64];
    hipLaunchKernelGGL(dinterp_records_kernel, dim3((unsigned)(B * geo.chunks)), dim3(256), 0, st, a);
    if (fr_allow_full_lds(reinterpret_cast<const void*>(&dinterp_owner_kernel), lds_ok) != hipSuccess) return FR_ERR_LAUNCH;
    hipLaunchKernelGGL(dinterp_owner_kernel, dim3((unsigned)(B * geo.splits)), dim3(OWNER_BLOCK), geo.lds, st, a.o);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
