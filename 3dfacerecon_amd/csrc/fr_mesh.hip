// Fine mesh (opt-in; include/fr_hotpath.h, "fine mesh"): the fine depth map lifted back onto the vertices through the rasteriser's
// tri_ind, with a per-vertex visibility and per-vertex normals.  Forward only, but for the normals (the smooth planes' route to the
// vertices).
//
//   mesh_visible_kernel    one lane per pixel in 256-pixel blocks, as dinterp_forward_kernel: an OK pixel stores the byte 1 at its
//                          three vertex ids (the plane is zeroed by the launcher on the same stream first).  The only race is several
//                          lanes storing the same value.
//   mesh_lift_kernel       one lane per (face, vertex): rows x and y copied, the z row moved by the bilinear sample of
//                          fine - coarse at the vertex's own position, over the corners that hold a triangle.  A gather.
//   mesh_normals_kernel    one lane per (face, vertex): walks the vertex's triangles in the order of a CSR adjacency table (shared by
//                          the faces) and adds their area-weighted normals in float64.  A gather: no atomics.
//   mesh_normals_bwd_*     its adjoint as two gathers around a float64 plane h [B,3,nver]: the first recomputes the forward's sums
//                          per (face, vertex) and writes the gradient with respect to the unnormalised sum; the second walks the
//                          vertex's triangles again and adds, per triangle, the cross products of an edge with the sum of h over
//                          the triangle's vertices.  One fixed chain per element: no atomics.
// No LDS, no atomics; the only scratch is h.
#include "fr_owner_scatter.h"

namespace fr {

struct MeshVisibleArgs {
    const float* tri;       // [3,ntri]
    const float* tri_ind;   // [B,H,W]
    unsigned char* visible; // [B,nver]
    int blocks;             // 256-pixel blocks of a face
    int nver, ntri, npix;
};

__global__ __launch_bounds__(256) void mesh_visible_kernel(MeshVisibleArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int i = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (i >= a.npix) return;
    int id[3];   // (ntri > 0: the launcher's)
    const bool ok = pixel_tri_ids(a.tri_ind[(size_t)b * a.npix + i], a.tri, a.tri + a.ntri, a.tri + 2 * (size_t)a.ntri, a.ntri,
                                  a.nver, id).ok;
    if (!ok) return;
    unsigned char* vis = a.visible + (size_t)b * a.nver;
    vis[id[0]] = 1; vis[id[1]] = 1; vis[id[2]] = 1;
}

struct MeshLiftArgs {
    const float* vertex;          // [B,3,vpitch]
    const float* tri_ind;         // [B,H,W]
    const unsigned char* visible; // [B,nver]
    const float* fine;            // [B,H,W]
    const float* coarse;          // [B,H,W]
    float* out;                   // [B,3,opitch]
    unsigned char* state;         // [B,nver]
    long long vpitch, opitch;
    int blocks;                   // 256-vertex blocks of a face
    int nver, ntri, H, W;
};

__global__ __launch_bounds__(256) void mesh_lift_kernel(MeshLiftArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int v = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (v >= a.nver) return;
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    float* __restrict__ ob = a.out + (size_t)b * 3 * a.opitch;
    const float x = vb[v], y = vb[a.vpitch + v], z = vb[2 * a.vpitch + v];
    const unsigned char vis = a.visible[(size_t)b * a.nver + v];
    float zo = z;
    unsigned char st = 0;
    if (vis) {
        st = 2;
        if (isfinite(x) && isfinite(y) && a.ntri > 0) {   // (an empty table: no corner holds a triangle, tri_ind is not read)
            const double c0 = floor((double)x), r0 = floor((double)y);
            const double fx = (double)x - c0, fy = (double)y - r0;
            const double gx = 1.0 - fx, gy = 1.0 - fy;
            const double w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
            const size_t face = (size_t)b * a.H * a.W;
            double num = 0.0, den = 0.0;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double r = r0 + (double)(k >> 1), c = c0 + (double)(k & 1);
                // (compared as doubles: a coordinate beyond the int range never becomes an index)
                if (!(r >= 0.0 && r < (double)a.H && c >= 0.0 && c < (double)a.W) || w[k] == 0.0) continue;
                const size_t o = face + (size_t)((int)r * a.W + (int)c);
                if (pixel_tri(a.tri_ind[o], a.ntri) < 0) continue;
                const double d = (double)a.fine[o] - (double)a.coarse[o];
                num = num + w[k] * d;
                den = den + w[k];
                any = true;
            }
            if (any) {
                st = 1;
                zo = (float)((double)z + num / den);
            }
        }
    }
    ob[v] = x;
    ob[a.opitch + v] = y;
    ob[2 * a.opitch + v] = zo;
    a.state[(size_t)b * a.nver + v] = st;
}

struct MeshNormalsArgs {
    const float* vertex;     // [B,3,vpitch]
    const float* tri;        // [3,ntri]
    const int* adj_start;    // [nver+1]
    const int* adj_tri;      // [3 ntri]
    float* normal;           // [B,3,opitch]
    long long vpitch, opitch;
    int blocks;              // 256-vertex blocks of a face
    int nver, ntri;
};

// The mesh of a vertex-normal walk: the triangle list, the adjacency table and one face's vertex rows.
struct MeshWalk {
    const float* tri;        // [3,ntri]
    const int* adj_start;    // [nver+1]
    const int* adj_tri;      // [3 ntri]
    const float* vb;         // one face's [3,vpitch]
    long long vpitch;
    int nver, ntri;
};

// Calls f(id, P) for the triangles of vertex v in table order: id the three vertex ids, all in [0, nver), P their positions widened
// to float64.  (The binding has checked the table; the clamps keep a table that was not from reading out of bounds.)
template <class F>
__device__ __forceinline__ void mesh_walk(const MeshWalk& m, int v, F&& f) {
    if (m.ntri <= 0) return;
    const int e0 = max(m.adj_start[v], 0), e1 = min(m.adj_start[v + 1], 3 * m.ntri);
    for (int e = e0; e < e1; e++) {
        const int t = m.adj_tri[e];
        if ((unsigned)t >= (unsigned)m.ntri) continue;
        const int id[3] = {f2i_x86(m.tri[t]), f2i_x86(m.tri[(size_t)m.ntri + t]), f2i_x86(m.tri[2 * (size_t)m.ntri + t])};
        if ((unsigned)id[0] >= (unsigned)m.nver || (unsigned)id[1] >= (unsigned)m.nver || (unsigned)id[2] >= (unsigned)m.nver)
            continue;
        double P[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) P[k][c] = (double)m.vb[(size_t)c * m.vpitch + id[k]];
        f(id, P);
    }
}

// The forward's three float64 chains of vertex v and their length: N = sum of (P2 - P1) x (P3 - P1) in table order, s = |N|.
struct NormalSum {
    double nx, ny, nz, s;
    bool unit;   // s > 0 and finite: the forward wrote N / s, else (+0, +0, +0)
};
__device__ __forceinline__ NormalSum mesh_normal_sum(const MeshWalk& m, int v) {
    double nx = 0.0, ny = 0.0, nz = 0.0;
    mesh_walk(m, v, [&](const int (&)[3], const double (&P)[3][3]) {
        const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
        const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
        nx = nx + (ay * bz - az * by);
        ny = ny + (az * bx - ax * bz);
        nz = nz + (ax * by - ay * bx);
    });
    NormalSum r;
    r.nx = nx; r.ny = ny; r.nz = nz;
    r.s = sqrt((nx * nx + ny * ny) + nz * nz);
    r.unit = r.s > 0.0 && isfinite(r.s);
    return r;
}

__global__ __launch_bounds__(256) void mesh_normals_kernel(MeshNormalsArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int v = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (v >= a.nver) return;
    const MeshWalk m = {a.tri, a.adj_start, a.adj_tri, a.vertex + (size_t)b * 3 * a.vpitch, a.vpitch, a.nver, a.ntri};
    float* __restrict__ ob = a.normal + (size_t)b * 3 * a.opitch;
    const NormalSum n = mesh_normal_sum(m, v);
    ob[v] = n.unit ? (float)(n.nx / n.s) : 0.0f;
    ob[a.opitch + v] = n.unit ? (float)(n.ny / n.s) : 0.0f;
    ob[2 * a.opitch + v] = n.unit ? (float)(n.nz / n.s) : 0.0f;
}

struct MeshNormalsBwdArgs {
    const float* grad;       // [B,3,gpitch]
    const float* vertex;     // [B,3,vpitch]
    const float* tri;        // [3,ntri]
    const int* adj_start;    // [nver+1]
    const int* adj_tri;      // [3 ntri]
    double* h;               // [B,3,nver]
    float* vertex_grad;      // [B,3,opitch]
    long long gpitch, vpitch, opitch;
    int blocks;              // 256-vertex blocks of a face
    int nver, ntri;
    int accumulate;
};

// launch 1: the gradient of the loss with respect to the unnormalised sum N of (face, vertex u), through n^ = N / s
__global__ __launch_bounds__(256) void mesh_normals_bwd_h_kernel(MeshNormalsBwdArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int u = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (u >= a.nver) return;
    const MeshWalk m = {a.tri, a.adj_start, a.adj_tri, a.vertex + (size_t)b * 3 * a.vpitch, a.vpitch, a.nver, a.ntri};
    const NormalSum n = mesh_normal_sum(m, u);
    double hx = 0.0, hy = 0.0, hz = 0.0;
    if (n.unit) {
        const float* __restrict__ gb = a.grad + (size_t)b * 3 * a.gpitch;
        const double gx = (double)gb[u], gy = (double)gb[a.gpitch + u], gz = (double)gb[2 * a.gpitch + u];
        const double ux = n.nx / n.s, uy = n.ny / n.s, uz = n.nz / n.s;
        const double d = (ux * gx + uy * gy) + uz * gz;
        hx = (gx - ux * d) / n.s;
        hy = (gy - uy * d) / n.s;
        hz = (gz - uz * d) / n.s;
    }
    double* __restrict__ hb = a.h + (size_t)b * 3 * a.nver;
    hb[u] = hx;
    hb[(size_t)a.nver + u] = hy;
    hb[2 * (size_t)a.nver + u] = hz;
}

// launch 2: (face, vertex v) gathers, from each of its triangles, the cross products its own positions in the triangle receive
__global__ __launch_bounds__(256) void mesh_normals_bwd_gather_kernel(MeshNormalsBwdArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int v = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (v >= a.nver) return;
    const MeshWalk m = {a.tri, a.adj_start, a.adj_tri, a.vertex + (size_t)b * 3 * a.vpitch, a.vpitch, a.nver, a.ntri};
    const double* __restrict__ hb = a.h + (size_t)b * 3 * a.nver;
    const size_t nv = (size_t)a.nver;
    double rx = 0.0, ry = 0.0, rz = 0.0;
    mesh_walk(m, v, [&](const int (&id)[3], const double (&P)[3][3]) {
        // every distinct vertex of the triangle counted the triangle once in its own sum
        double Hx = hb[id[0]], Hy = hb[nv + id[0]], Hz = hb[2 * nv + id[0]];
        if (id[1] != id[0]) { Hx = Hx + hb[id[1]]; Hy = Hy + hb[nv + id[1]]; Hz = Hz + hb[2 * nv + id[1]]; }
        if (id[2] != id[0] && id[2] != id[1]) { Hx = Hx + hb[id[2]]; Hy = Hy + hb[nv + id[2]]; Hz = Hz + hb[2 * nv + id[2]]; }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (id[k] != v) continue;
            // p x q: (P2 - P3) x Hs for P1, (P3 - P1) x Hs for P2, Hs x (P2 - P1) for P3
            double px, py, pz, qx, qy, qz;
            if (k == 0) { px = P[1][0] - P[2][0]; py = P[1][1] - P[2][1]; pz = P[1][2] - P[2][2]; qx = Hx; qy = Hy; qz = Hz; }
            else if (k == 1) { px = P[2][0] - P[0][0]; py = P[2][1] - P[0][1]; pz = P[2][2] - P[0][2]; qx = Hx; qy = Hy; qz = Hz; }
            else { px = Hx; py = Hy; pz = Hz; qx = P[1][0] - P[0][0]; qy = P[1][1] - P[0][1]; qz = P[1][2] - P[0][2]; }
            rx = rx + (py * qz - pz * qy);
            ry = ry + (pz * qx - px * qz);
            rz = rz + (px * qy - py * qx);
        }
    });
    float* __restrict__ ob = a.vertex_grad + (size_t)b * 3 * a.opitch;
    const float o[3] = {(float)rx, (float)ry, (float)rz};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float* p = ob + (size_t)c * a.opitch + v;
        *p = a.accumulate ? *p + o[c] : o[c];
    }
}

}  // namespace fr

namespace {
// 256-lane blocks of `n` items per face, or -1 where B faces of them do not fit one grid
inline long long mesh_blocks(int B, long long n) {
    const long long blocks = (n + 255) / 256;
    return (long long)B * blocks > 0x7FFFFFFFll ? -1 : blocks;
}
}  // namespace

// ---- C ABI (include/fr_hotpath.h) ---------------------------------------------------------------------------------------------
extern "C" {

int fr_mesh_visible(const float* tri, const float* tri_ind, int B, int nver, int ntri, int H, int W, unsigned char* visible,
                    void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (B == 0 || nver == 0) return FR_OK;
    const long long npix = (long long)H * W;
    if (!visible || (ntri > 0 && npix > 0 && (!tri || !tri_ind))) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24) || npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    const long long blocks = mesh_blocks(B, npix);
    if (blocks < 0) return FR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(visible, 0, (size_t)B * nver, st) != hipSuccess) return FR_ERR_LAUNCH;
    if (ntri == 0 || npix == 0) return FR_OK;
    MeshVisibleArgs a;
    a.tri = tri; a.tri_ind = tri_ind; a.visible = visible;
    a.blocks = (int)blocks; a.nver = nver; a.ntri = ntri; a.npix = (int)npix;
    hipLaunchKernelGGL(mesh_visible_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_mesh_lift(const float* vertex, int vertex_pitch, const float* tri_ind, const unsigned char* visible, const float* fine_depth,
                 const float* coarse_depth, int B, int nver, int ntri, int H, int W, float* vertex_out, int out_pitch,
                 unsigned char* state, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || H < 0 || W < 0 || vertex_pitch < nver || out_pitch < nver) return FR_ERR_INVALID_ARG;
    if (B == 0 || nver == 0) return FR_OK;
    const long long npix = (long long)H * W;
    if (!vertex || !visible || !vertex_out || !state) return FR_ERR_INVALID_ARG;
    if (ntri > 0 && npix > 0 && (!tri_ind || !fine_depth || !coarse_depth)) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24) || npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    const long long blocks = mesh_blocks(B, nver);
    if (blocks < 0) return FR_ERR_UNSUPPORTED;
    MeshLiftArgs a;
    a.vertex = vertex; a.tri_ind = tri_ind; a.visible = visible; a.fine = fine_depth; a.coarse = coarse_depth;
    a.out = vertex_out; a.state = state; a.vpitch = vertex_pitch; a.opitch = out_pitch;
    a.blocks = (int)blocks; a.nver = nver; a.ntri = ntri; a.H = H; a.W = W;
    hipLaunchKernelGGL(mesh_lift_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_mesh_vertex_normals(const float* vertex, int vertex_pitch, const float* tri, const int* adj_start, const int* adj_tri, int B,
                           int nver, int ntri, float* normal, int out_pitch, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || vertex_pitch < nver || out_pitch < nver) return FR_ERR_INVALID_ARG;
    if (B == 0 || nver == 0) return FR_OK;
    if (!vertex || !normal || (ntri > 0 && (!tri || !adj_start || !adj_tri))) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;
    const long long blocks = mesh_blocks(B, nver);
    if (blocks < 0) return FR_ERR_UNSUPPORTED;
    MeshNormalsArgs a;
    a.vertex = vertex; a.tri = tri; a.adj_start = adj_start; a.adj_tri = adj_tri; a.normal = normal;
    a.vpitch = vertex_pitch; a.opitch = out_pitch; a.blocks = (int)blocks; a.nver = nver; a.ntri = ntri;
    hipLaunchKernelGGL(mesh_normals_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_mesh_vertex_normals_backward(const float* normal_grad, int grad_pitch, const float* vertex, int vertex_pitch, const float* tri,
                                    const int* adj_start, const int* adj_tri, int B, int nver, int ntri, double* h,
                                    float* vertex_grad, int out_pitch, int accumulate, void* stream) {
    using namespace fr;
    if (B < 0 || nver < 0 || ntri < 0 || grad_pitch < nver || vertex_pitch < nver || out_pitch < nver) return FR_ERR_INVALID_ARG;
    if (accumulate != 0 && accumulate != 1) return FR_ERR_INVALID_ARG;
    if (B == 0 || nver == 0) return FR_OK;
    if (!normal_grad || !vertex || !vertex_grad || (ntri > 0 && (!tri || !adj_start || !adj_tri))) return FR_ERR_INVALID_ARG;
    if (ntri >= (1 << 24)) return FR_ERR_UNSUPPORTED;
    const long long blocks = mesh_blocks(B, nver);
    if (blocks < 0) return FR_ERR_UNSUPPORTED;
    if (!h || ((uintptr_t)h & 7)) return FR_ERR_WORKSPACE;
    MeshNormalsBwdArgs a;
    a.grad = normal_grad; a.vertex = vertex; a.tri = tri; a.adj_start = adj_start; a.adj_tri = adj_tri; a.h = h;
    a.vertex_grad = vertex_grad; a.gpitch = grad_pitch; a.vpitch = vertex_pitch; a.opitch = out_pitch;
    a.blocks = (int)blocks; a.nver = nver; a.ntri = ntri; a.accumulate = accumulate;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_normals_bwd_h_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mesh_normals_bwd_gather_kernel, dim3((unsigned)(B * blocks)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

}  // extern "C"
