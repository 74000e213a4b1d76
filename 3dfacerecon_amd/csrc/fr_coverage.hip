// Soft coverage (opt-in; include/fr_hotpath.h, "soft coverage"): the silhouette of the rendered face as a plane in [0, 1] that depends
// on the x and y of the vertices, and its gradient.  A post-pass over tri_ind, as the interpolated depth: which triangle wins a pixel
// stays the render forward's business; this file looks only at PAIRS of 4-neighbours of which one is OK and the other is not, and
// asks where on the segment between the two centres the OK pixel's triangle ends.
//
//   cov_forward_kernel    one lane per pixel in tiles of 32 x 8.  The workgroup stages its tile of tri_ind with a one-pixel halo in
//                         LDS as "the triangle if the pixel is OK, else -1" (a covered pixel costs the three id gathers that decide
//                         OK, out of the L2-resident table; an uncovered one nothing), then a lane whose four neighbours share its
//                         state stores 1 or +0 and is done.  Only a border lane gathers vertices: the x, y of its own triangle (an OK
//                         pixel), or of its OK neighbours' (a not-OK pixel: all four together, ids first, then vertices).
//   cov_records_kernel    the records pass of the owner-scatter scheme (fr_owner_scatter.h) over 1,024-pixel chunks: an OK pixel with
//                         a not-OK neighbour evaluates its pairs again (the forward's device function: the same s), forms its six
//                         x, y terms and writes the three record planes; every other pixel writes p1 = -1 and no term plane.
//   cov_owner_kernel      owner_rows3: the normal backward's owner, instantiated here for this file's records.
#include "fr_owner_scatter.h"

namespace fr {

constexpr int COV_TW = 32, COV_TH = 8;   // the forward's tile: 256 lanes, rows of 32 consecutive pixels

// neighbour k = 0, 1, 2, 3 of a pixel: left, right, up, down -- the order every sum below takes them in
__device__ __forceinline__ int cov_dx(int k) { return k == 0 ? -1 : (k == 1 ? 1 : 0); }
__device__ __forceinline__ int cov_dy(int k) { return k == 2 ? -1 : (k == 3 ? 1 : 0); }

// e(A, B, X) of the header: fp64, every difference, product and the final difference rounded on its own
__device__ __forceinline__ double cov_edge(double ax, double ay, double bx, double by, double xx, double xy) {
    return (bx - ax) * (xy - ay) - (by - ay) * (xx - ax);
}

// The pair (c, n) of the header for the triangle P (x, y of its three vertices, widened): where the segment c -> n leaves it.
struct CovPair {
    bool live;        // not inert: the triangle has area and an edge is a candidate
    int k;            // the winning edge, 0 .. 2 = (P1,P2), (P2,P3), (P3,P1)
    double s;         // Fc / (Fc - Fn) of the winning edge, before the clamp
    double fc, fn;    // of the winning edge
    double sigma;     // the sign of the area
};
__device__ __forceinline__ CovPair cov_pair(const double (&P)[3][2], int cx, int cy, int nx, int ny) {
    CovPair r;
    r.live = false; r.k = 0; r.s = 0.0; r.fc = 0.0; r.fn = 0.0; r.sigma = 0.0;
    const double area = cov_edge(P[0][0], P[0][1], P[1][0], P[1][1], P[2][0], P[2][1]);
    if (area == 0 || !isfinite(area)) return r;
    r.sigma = area > 0 ? 1.0 : -1.0;
    const double xc = (double)cx, yc = (double)cy, xn = (double)nx, yn = (double)ny;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int j = (k + 1) % 3;
        const double fc = r.sigma * cov_edge(P[k][0], P[k][1], P[j][0], P[j][1], xc, yc);
        const double fn = r.sigma * cov_edge(P[k][0], P[k][1], P[j][0], P[j][1], xn, yn);
        if (!(fn < 0 && fc > fn)) continue;
        const double sk = fc / (fc - fn);
        if (!isfinite(sk)) continue;
        if (!r.live || sk < r.s) { r.live = true; r.k = k; r.s = sk; r.fc = fc; r.fn = fn; }   // (a tie keeps the lowest k)
    }
    return r;
}
__device__ __forceinline__ double cov_clamp01(double s) {
    const double lo = s > 0.0 ? s : 0.0;
    return lo < 1.0 ? lo : 1.0;
}

// the x, y of the three vertices of an OK pixel's triangle, widened
__device__ __forceinline__ void cov_gather_xy(const float* __restrict__ vb, long long vpitch, const int (&id)[3], double (&P)[3][2]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        P[k][0] = (double)vb[id[k]];
        P[k][1] = (double)vb[(size_t)vpitch + id[k]];
    }
}

struct CovFwdArgs {
    const float* vertex;    // [B,3,vpitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    float* cov;             // [B,H,W,1]
    long long vpitch;
    int tiles_x, tiles;     // tiles across, tiles of a face
    int nver, ntri, H, W;
};

__global__ __launch_bounds__(COV_TW * COV_TH) void cov_forward_kernel(CovFwdArgs a) {
    __shared__ int okt[COV_TH + 2][COV_TW + 2];   // the triangle of an OK pixel, -1 for a not-OK one, -2 outside the image
    const int b = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - b * a.tiles;
    const int ty0 = (tile / a.tiles_x) * COV_TH, tx0 = (tile % a.tiles_x) * COV_TW;
    const int tid = threadIdx.x;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * a.H * a.W;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + a.ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)a.ntri;
    for (int e = tid; e < (COV_TH + 2) * (COV_TW + 2); e += COV_TW * COV_TH) {
        const int ly = e / (COV_TW + 2), lx = e - ly * (COV_TW + 2);
        const int y = ty0 + ly - 1, x = tx0 + lx - 1;
        int v = -2;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            v = -1;
            const int t = a.ntri > 0 ? pixel_tri(ti[(size_t)y * a.W + x], a.ntri) : -1;   // (an empty table has no triangle to read)
            if (t >= 0) {
                const int p1 = f2i_x86(tri0[t]), p2 = f2i_x86(tri1[t]), p3 = f2i_x86(tri2[t]);
                if ((unsigned)p1 < (unsigned)a.nver && (unsigned)p2 < (unsigned)a.nver && (unsigned)p3 < (unsigned)a.nver) v = t;
            }
        }
        okt[ly][lx] = v;
    }
    __syncthreads();
    const int ly = tid / COV_TW, lx = tid - ly * COV_TW;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= a.H || x >= a.W) return;
    const int me = okt[ly + 1][lx + 1];
    int nb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) nb[k] = okt[ly + 1 + cov_dy(k)][lx + 1 + cov_dx(k)];
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    double acc = 0.0;
    float out;
    if (me >= 0) {
        if (nb[0] == -1 || nb[1] == -1 || nb[2] == -1 || nb[3] == -1) {
            const int id[3] = {f2i_x86(tri0[me]), f2i_x86(tri1[me]), f2i_x86(tri2[me])};
            double P[3][2];
            cov_gather_xy(vb, a.vpitch, id, P);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (nb[k] != -1) continue;
                const CovPair pr = cov_pair(P, x, y, x + cov_dx(k), y + cov_dy(k));
                if (!pr.live) continue;
                const double d = 0.5 - cov_clamp01(pr.s);
                acc = acc + (d > 0.0 ? d : 0.0);
            }
        }
        const double v = 1.0 - acc;
        out = (float)(v > 0.0 ? v : 0.0);
    } else {
        if (nb[0] >= 0 || nb[1] >= 0 || nb[2] >= 0 || nb[3] >= 0) {
            // the gathers of the (up to) four OK neighbours are issued together, ids first, then vertices: two dependent trips to
            // L2 instead of eight (a neighbour that is not OK repeats an OK one's addresses and is not evaluated)
            int first = nb[0] >= 0 ? nb[0] : (nb[1] >= 0 ? nb[1] : (nb[2] >= 0 ? nb[2] : nb[3]));
            int id[4][3];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = nb[k] >= 0 ? nb[k] : first;
                id[k][0] = f2i_x86(tri0[t]); id[k][1] = f2i_x86(tri1[t]); id[k][2] = f2i_x86(tri2[t]);
            }
            double P[4][3][2];
#pragma unroll
            for (int k = 0; k < 4; k++) cov_gather_xy(vb, a.vpitch, id[k], P[k]);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (nb[k] < 0) continue;
                const CovPair pr = cov_pair(P[k], x + cov_dx(k), y + cov_dy(k), x, y);
                if (!pr.live) continue;
                const double d = cov_clamp01(pr.s) - 0.5;
                acc = acc + (d > 0.0 ? d : 0.0);
            }
        }
        out = (float)(acc < 1.0 ? acc : 1.0);
    }
    a.cov[(size_t)b * a.H * a.W + (size_t)y * a.W + x] = out;
}

struct CovBwdArgs {
    const float* cgrad;     // [B,H,W,1]
    const float* cov;       // [B,H,W,1], the forward's
    const float* vertex;    // [B,3,vpitch]
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W,1]
    long long vpitch;
    int H, W;
    int ntri;
    OwnerRows3 o;
};

// dinterp_records_kernel's shape: 256 threads x 4 lane-consecutive pixels.  Most pixels end after one or four loads; the pair
// work is done by the border pixels alone.
__global__ __launch_bounds__(256) void cov_records_kernel(CovBwdArgs a) {
    __shared__ uint32_t red[8];
    const int chunks = a.o.chunks, npix = a.o.npix, nver = a.o.nver, ntri = a.ntri, W = a.W, H = a.H;
    const int b = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - b * chunks;
    const int tid = threadIdx.x;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    const float* __restrict__ gp = a.cgrad + (size_t)b * npix;
    const float* __restrict__ cp = a.cov + (size_t)b * npix;
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    int4* __restrict__ r0 = a.o.rec + (size_t)b * 3 * npix;
    int4* __restrict__ r1 = r0 + npix;
    int4* __restrict__ r2 = r1 + npix;
    constexpr int PU = REC_PX / 256;
    uint32_t m = 0, bad = 0;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = ch * REC_PX + u * 256 + tid;
        if (i >= npix) continue;
        int id[3];
        bool wrote = false;
        if (pixel_tri_ids(ti[i], tri0, tri1, tri2, ntri, nver, id).ok) {
            const int y = i / W, x = i - y * W;
            // which neighbours exist and are not OK (the ids of a covered neighbour are read to decide it)
            bool open[4];
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int nx = x + cov_dx(k), ny = y + cov_dy(k);
                open[k] = false;
                if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
                int nid[3];
                open[k] = !pixel_tri_ids(ti[i + cov_dy(k) * W + cov_dx(k)], tri0, tri1, tri2, ntri, nver, nid).ok;
                any = any || open[k];
            }
            if (any) {
                double P[3][2];
                cov_gather_xy(vb, a.vpitch, id, P);
                const float cc = cp[i];
                const double Gc = (double)gp[i];
                double slot[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!open[k]) continue;
                    const int nx = x + cov_dx(k), ny = y + cov_dy(k);
                    const CovPair pr = cov_pair(P, x, y, nx, ny);
                    if (!pr.live || !(pr.s > 0.0 && pr.s < 1.0)) continue;
                    const int in = i + cov_dy(k) * W + cov_dx(k);
                    double q = 0.0;
                    if (pr.s < 0.5 && cc > 0.0f) q = q + Gc;
                    if (pr.s > 0.5 && cp[in] < 1.0f) q = q + (double)gp[in];
                    const int ka = pr.k, kb = (pr.k + 1) % 3;
                    // (selected by comparison: a run-time index would put P in scratch)
                    const double ax = ka == 0 ? P[0][0] : (ka == 1 ? P[1][0] : P[2][0]), ay = ka == 0 ? P[0][1] : (ka == 1 ? P[1][1] : P[2][1]);
                    const double bx = kb == 0 ? P[0][0] : (kb == 1 ? P[1][0] : P[2][0]), by = kb == 0 ? P[0][1] : (kb == 1 ? P[1][1] : P[2][1]);
                    const double xc = (double)x, yc = (double)y, xn = (double)nx, yn = (double)ny;
                    const double D = pr.fc - pr.fn, DD = D * D, nfn = -pr.fn;
                    // d e(X) / d (Ax, Ay, Bx, By) = (By - Xy, Xx - Bx, Xy - Ay, Ax - Xx)
                    const double dec[4] = {by - yc, xc - bx, yc - ay, ax - xc};
                    const double den[4] = {by - yn, xn - bx, yn - ay, ax - xn};
                    double ds[4];
#pragma unroll
                    for (int v = 0; v < 4; v++) ds[v] = (pr.sigma * (nfn * dec[v] + pr.fc * den[v])) / DD;
                    // (static slot indices: the winning edge selects by comparison, not by address)
#pragma unroll
                    for (int e = 0; e < 3; e++) {
                        if (e == ka) { slot[e][0] = slot[e][0] + q * ds[0]; slot[e][1] = slot[e][1] + q * ds[1]; }
                        if (e == kb) { slot[e][0] = slot[e][0] + q * ds[2]; slot[e][1] = slot[e][1] + q * ds[3]; }
                    }
                }
                float t[9];
                bool zero = true;
#pragma unroll
                for (int e = 0; e < 3; e++) {
                    t[3 * e] = (float)slot[e][0];
                    t[3 * e + 1] = (float)slot[e][1];
                    t[3 * e + 2] = 0.0f;
                    zero = zero && t[3 * e] == 0.0f && t[3 * e + 1] == 0.0f;
                }
                if (!zero) {
#pragma unroll
                    for (int j = 0; j < 9; j++) track_term(__float_as_uint(t[j]), m, bad);
                    store_rows3(r0, r1, r2, i, id, t);
                    wrote = true;
                }
            }
        }
        if (!wrote) r0[i] = make_int4(-1, 0, 0, 0);   // contributes nothing, its term planes are never read
    }
    chunk_publish(m, bad, red, a.o.partial + (size_t)b * chunks + ch);
}

__global__ __launch_bounds__(OWNER_BLOCK) void cov_owner_kernel(OwnerRows3 o) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // all LDS is dynamic: owner_rows3's
    owner_rows3(o, acc);
}

}  // namespace fr

// ---- C ABI (include/fr_hotpath.h) ---------------------------------------------------------------------------------------------
extern "C" {

int fr_coverage_forward(const float* vertex, int vertex_pitch, const float* tri, const float* tri_ind, int B, int nver, int ntri,
                        int H, int W, float* cov, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0 || vertex_pitch < nver) return FR_ERR_INVALID_ARG;
    const long long npix = (long long)H * W;
    if (B == 0 || npix == 0) return FR_OK;
    if (!tri_ind || !cov || (ntri > 0 && (!tri || (nver > 0 && !vertex)))) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;   // float-stored ids stop being exact
    const long long tx = ((long long)W + COV_TW - 1) / COV_TW, ty = ((long long)H + COV_TH - 1) / COV_TH;
    if (npix > 0x7FFFFFFFll || tx * ty > 0x7FFFFFFFll || (long long)B * tx * ty > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    CovFwdArgs a;
    a.vertex = vertex; a.tri = tri; a.tri_ind = tri_ind; a.cov = cov; a.vpitch = vertex_pitch;
    a.tiles_x = (int)tx; a.tiles = (int)(tx * ty); a.nver = nver; a.ntri = ntri; a.H = H; a.W = W;
    hipLaunchKernelGGL(cov_forward_kernel, dim3((unsigned)(B * tx * ty)), dim3(COV_TW * COV_TH), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

size_t fr_coverage_backward_workspace_bytes(int B, int nver, int H, int W) {
    (void)nver;
    return fr::rows3_workspace_bytes(B, H, W);
}

// out = {owners per face, vertices per owner, shift, 1,024-pixel record chunks, LDS bytes of an owner, XCD-map flag}; all zero for
// a shape that launches no kernel or is refused
void fr_debug_coverage_bwd_geom(int B, int nver, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll) return;
    fr::owner_geom_report(fr::rows3_geom(B, nver, npix), B, out);
}

int fr_coverage_backward(const float* cov_grad, const float* cov, const float* vertex, int vertex_pitch, const float* tri,
                         const float* tri_ind, float* vertex_grad, int B, int nver, int ntri, int H, int W, int accumulate,
                         void* workspace, size_t ws_bytes, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if ((accumulate != 0 && accumulate != 1) || vertex_pitch < nver) return FR_ERR_INVALID_ARG;
    const long long npix = (long long)H * W;
    if (B == 0 || npix == 0) return FR_OK;
    if (nver == 0) return FR_OK;   // an empty vertex_grad: nothing to write
    if (!vertex_grad) return FR_ERR_INVALID_ARG;
    if (ntri > 0 && (!cov_grad || !cov || !vertex || !tri || !tri_ind)) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24) || npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    if (ntri > 0 && !ws_ok(workspace, ws_bytes, rows3_workspace_bytes(B, H, W), 16)) return FR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (ntri == 0) return owner_no_terms(vertex_grad, (size_t)B * 3 * nver * sizeof(float), accumulate, st);
    const OwnerGeom geo = rows3_geom(B, nver, npix);
    if ((long long)B * geo.splits > 0x7FFFFFFFll || (long long)B * geo.chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    CovBwdArgs a;
    a.cgrad = cov_grad; a.cov = cov; a.vertex = vertex; a.vpitch = vertex_pitch; a.tri = tri; a.tri_ind = tri_ind;
    a.H = H; a.W = W; a.ntri = ntri;
    int4* rec = reinterpret_cast<int4*>(workspace);
    a.o.rec = rec;
    a.o.partial = reinterpret_cast<uint2*>(rec + (size_t)B * 3 * npix);
    a.o.vertex_grad = vertex_grad;
    a.o.B = B; a.o.chunks = geo.chunks; a.o.nver = nver; a.o.npix = (int)npix;
    a.o.splits = geo.splits; a.o.range = geo.range; a.o.shift = geo.shift; a.o.accumulate = accumulate;
    static fr_lds_flags_t lds_ok[64];
    hipLaunchKernelGGL(cov_records_kernel, dim3((unsigned)(B * geo.chunks)), dim3(256), 0, st, a);
    if (fr_allow_full_lds(reinterpret_cast<const void*>(&cov_owner_kernel), lds_ok) != hipSuccess) return FR_ERR_LAUNCH;
    hipLaunchKernelGGL(cov_owner_kernel, dim3((unsigned)(B * geo.splits)), dim3(OWNER_BLOCK), geo.lds, st, a.o);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
