// render_depth normal backward (opt-in; include/fr_hotpath.h, "normal-map gradients"): the gradient of the op's `normal`
// plane -- or of the normalised map the rendering layer makes of it -- with respect to all three coordinates of the
// winning triangle's vertices.  The reference has no such gradient (render_depth_op.cc:359-363 writes zeros into the x / y
// rows and never reads normal_grad); fr_render_depth_backward keeps that definition, this call ADDS the missing part.
//
// Two kernels, the owner-scatter scheme of fr_owner_scatter.h with nine terms per pixel:
//   nbwd_records_kernel   one pass over the batch's pixels: triangle -> three vertex ids -> nine vertex coordinates
//                         (the only gathers of the call, done once), the pixel's nine fp32 terms formed in double, written
//                         as three 16-byte planes {p1 p2 p3 t1x | t1y t1z t2x t2y | t2z t3x t3y t3z}; the largest |term|
//                         and a non-finite flag per 1,024-pixel chunk.
//   nbwd_owner_kernel     one workgroup per (face, vertex range): streams the face's id plane, fetches the two term planes
//                         of the pixels that land in its range only, and adds the terms as 64-bit fixed-point integers to
//                         three LDS accumulators per owned vertex (integer addition: exact, any order).  No two workgroups
//                         write the same element, nothing needs zeroing, no float atomics on the finite path.
#include "fr_owner_scatter.h"

namespace fr {

constexpr int NB_BLOCK = OWNER_BLOCK;

struct NbwdArgs {
    const float* ngrad;     // three floats per pixel, `gstride` floats between pixels
    const float* vertex;    // [B,3,vpitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    float* vertex_grad;     // [B,3,nver]
    int4* rec;              // [B][3][npix]
    uint2* partial;         // [B,chunks] {largest finite |term| bits, non-finite flag}
    long long vpitch;
    int gstride;
    int B, chunks, nver, ntri, npix;
    int splits, range, shift;
    int mode, accumulate;
};

// The nine terms of one pixel (include/fr_hotpath.h): a = fl32(P1 - P2), b = fl32(P1 - P3); all products and sums in double,
// each rounded on its own (this TU is compiled without contraction), one rounding to fp32 per term.
__device__ __forceinline__ void nbwd_terms(const float (&P)[3][3] /*[vertex][xyz]*/, const float (&g)[3], int mode, float (&t)[9]) {
    const double ax = (double)(P[0][0] - P[1][0]), ay = (double)(P[0][1] - P[1][1]), az = (double)(P[0][2] - P[1][2]);
    const double bx = (double)(P[0][0] - P[2][0]), by = (double)(P[0][1] - P[2][1]), bz = (double)(P[0][2] - P[2][2]);
    double Gx = (double)g[0], Gy = (double)g[1], Gz = (double)g[2];
    if (mode == 1) {
        // the forward's normal, by the forward's own expression (resolve_pixel), and post_normal's branch on its fp32 |m|^2
        const float nx = (float)(ay * bz - az * by), ny = (float)(az * bx - ax * bz), nz = (float)(ax * by - ay * bx);
        const float sf = (nz < 0.0f) ? -1.0f : 1.0f;
        const float mxf = sf * nx, myf = sf * ny, mzf = sf * nz;
        const float mag32 = (mxf * mxf + myf * myf) + mzf * mzf;
        const double s = (double)sf, m0 = (double)mxf, m1 = (double)myf, m2 = (double)mzf;
        const double eps = (double)1e-6f;
        if (mag32 > 1e-6f) {
            const double r = sqrt(m0 * m0 + m1 * m1 + m2 * m2);
            const double d = r + eps;
            const double k = (Gx * m0 + Gy * m1 + Gz * m2) / (d * d * r);
            Gx = s * (Gx / d - m0 * k);
            Gy = s * (Gy / d - m1 * k);
            Gz = s * (Gz / d - m2 * k);
        } else {
            const double d = 1.0 + eps;
            Gx = s * (Gx / d); Gy = s * (Gy / d); Gz = s * (Gz / d);
        }
    }
    const double dax = by * Gz - bz * Gy, day = bz * Gx - bx * Gz, daz = bx * Gy - by * Gx;   // da = b x G
    const double dbx = Gy * az - Gz * ay, dby = Gz * ax - Gx * az, dbz = Gx * ay - Gy * ax;   // db = G x a
    t[0] = (float)(dax + dbx); t[1] = (float)(day + dby); t[2] = (float)(daz + dbz);
    t[3] = (float)(-dax); t[4] = (float)(-day); t[5] = (float)(-daz);
    t[6] = (float)(-dbx); t[7] = (float)(-dby); t[8] = (float)(-dbz);
}

__global__ __launch_bounds__(256) void nbwd_records_kernel(NbwdArgs a) {
    __shared__ uint32_t red[8];
    const int b = (int)blockIdx.x / a.chunks, ch = (int)blockIdx.x - b * a.chunks;
    const int tid = threadIdx.x;
    const int npix = a.npix, ntri = a.ntri, nver = a.nver;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    const float* __restrict__ gp = a.ngrad + (size_t)b * npix * a.gstride;
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    int4* __restrict__ r0 = a.rec + (size_t)b * 3 * npix;
    int4* __restrict__ r1 = r0 + npix;
    int4* __restrict__ r2 = r1 + npix;
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
    int id[PU][3];
    bool ok[PU];
#pragma unroll
    for (int u = 0; u < PU; u++) ok[u] = pixel_tri_ids(tq[u], tri0, tri1, tri2, ntri, nver, id[u]).ok && i0 + u * 256 < npix;
    float P[PU][3][3];
#pragma unroll
    for (int u = 0; u < PU; u++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int p = ok[u] ? id[u][k] : 0;
#pragma unroll
            for (int c = 0; c < 3; c++) P[u][k][c] = vb[(size_t)c * a.vpitch + p];
        }
    uint32_t m = 0, bad = 0;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = i0 + u * 256;
        if (i >= npix) continue;
        if (!ok[u]) {   // background, a triangle index or a vertex id out of range: contributes nothing, its term planes are never read
            r0[i] = make_int4(-1, 0, 0, 0);
            continue;
        }
        float t[9];
        nbwd_terms(P[u], g[u], a.mode, t);
#pragma unroll
        for (int j = 0; j < 9; j++) track_term(__float_as_uint(t[j]), m, bad);   // over the OK pixels
        store_rows3(r0, r1, r2, i, id[u], t);
    }
    chunk_publish(m, bad, red, &a.partial[(size_t)b * a.chunks + ch]);
}

__global__ __launch_bounds__(NB_BLOCK) void nbwd_owner_kernel(NbwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // all LDS is dynamic: owner_rows3's
    owner_rows3({a.rec, a.partial, a.vertex_grad, a.B, a.chunks, a.nver, a.npix, a.splits, a.range, a.shift, a.accumulate}, acc);
}

}  // namespace fr

// The launch geometry is chosen in ONE place (fr_owner_scatter.h rows3_geom): the launcher and the test hook both read it there.
size_t fr_render_normal_backward_workspace_impl(int B, int H, int W) { return fr::rows3_workspace_bytes(B, H, W); }

// test hook (tests/test_normal_backward_*.py): out = {owners per face, vertices per owner, shift, 1,024-pixel record chunks,
// LDS bytes of an owner, XCD-map flag}; all zero for a shape that launches no kernel or is refused
extern "C" void fr_debug_render_normal_bwd_geom(int B, int nver, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll) return;
    fr::owner_geom_report(fr::rows3_geom(B, nver, npix), B, out);
}

int fr_launch_render_normal_backward(const float* normal_grad, int grad_stride, const float* vertex, int vertex_pitch,
                                     const float* tri, const float* tri_ind, float* vertex_grad, int B, int nver, int ntri,
                                     int H, int W, int mode, int accumulate, void* workspace, hipStream_t stream) {
    using namespace fr;
    const long long npix = (long long)H * W;
    if (npix == 0 || ntri == 0) return owner_no_terms(vertex_grad, (size_t)B * 3 * nver * sizeof(float), accumulate, stream);
    if (npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    const OwnerGeom geo = fr::rows3_geom(B, nver, npix);
    if ((long long)B * geo.splits > 0x7FFFFFFFll || (long long)B * geo.chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    NbwdArgs a;
    a.ngrad = normal_grad; a.gstride = grad_stride; a.vertex = vertex; a.vpitch = vertex_pitch;
    a.tri = tri; a.tri_ind = tri_ind; a.vertex_grad = vertex_grad;
    a.rec = reinterpret_cast<int4*>(workspace);
    a.partial = reinterpret_cast<uint2*>(a.rec + (size_t)B * 3 * npix);
    a.B = B; a.chunks = geo.chunks; a.nver = nver; a.ntri = ntri; a.npix = (int)npix;
    a.splits = geo.splits; a.range = geo.range; a.shift = geo.shift;
    a.mode = mode; a.accumulate = accumulate;
    static fr_lds_flags_t lds_ok[64];
    hipLaunchKernelGGL(nbwd_records_kernel, dim3((unsigned)(B * geo.chunks)), dim3(256), 0, stream, a);
    if (fr_allow_full_lds(reinterpret_cast<const void*>(&nbwd_owner_kernel), lds_ok) != hipSuccess) return FR_ERR_LAUNCH;
    hipLaunchKernelGGL(nbwd_owner_kernel, dim3((unsigned)(B * geo.splits)), dim3(NB_BLOCK), geo.lds, stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
