// Fine mesh (opt-in; include/fr_hotpath.h, "fine mesh"): the fine depth map lifted back onto the vertices through the rasteriser's
// tri_ind, with a per-vertex visibility and per-vertex normals.  Forward only.
//
//   mesh_visible_kernel    one lane per pixel in 256-pixel blocks, as dinterp_forward_kernel: an OK pixel stores the byte 1 at its
//                          three vertex ids (the plane is zeroed by the launcher on the same stream first).  The only race is several
//                          lanes storing the same value.
//   mesh_lift_kernel       one lane per (face, vertex): rows x and y copied, the z row moved by the bilinear sample of
//                          fine - coarse at the vertex's own position, over the corners that hold a triangle.  A gather.
//   mesh_normals_kernel    one lane per (face, vertex): walks the vertex's triangles in the order of a CSR adjacency table (shared by
//                          the faces) and adds their area-weighted normals in float64.  A gather: no atomics.
// No LDS, no atomics, no workspace.
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

__global__ __launch_bounds__(256) void mesh_normals_kernel(MeshNormalsArgs a) {
    const int b = (int)blockIdx.x / a.blocks;
    const int v = ((int)blockIdx.x - b * a.blocks) * 256 + (int)threadIdx.x;
    if (v >= a.nver) return;
    const float* __restrict__ vb = a.vertex + (size_t)b * 3 * a.vpitch;
    float* __restrict__ ob = a.normal + (size_t)b * 3 * a.opitch;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (a.ntri > 0) {
        // (the binding has checked the table; the clamps keep a table that was not from reading out of bounds)
        const int e0 = max(a.adj_start[v], 0), e1 = min(a.adj_start[v + 1], 3 * a.ntri);
        for (int e = e0; e < e1; e++) {
            const int t = a.adj_tri[e];
            if ((unsigned)t >= (unsigned)a.ntri) continue;
            const int id[3] = {f2i_x86(a.tri[t]), f2i_x86(a.tri[(size_t)a.ntri + t]), f2i_x86(a.tri[2 * (size_t)a.ntri + t])};
            if ((unsigned)id[0] >= (unsigned)a.nver || (unsigned)id[1] >= (unsigned)a.nver || (unsigned)id[2] >= (unsigned)a.nver)
                continue;
            double P[3][3];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) P[k][c] = (double)vb[(size_t)c * a.vpitch + id[k]];
            const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
            const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
            nx = nx + (ay * bz - az * by);
            ny = ny + (az * bx - ax * bz);
            nz = nz + (ax * by - ay * bx);
        }
    }
    const double s = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool unit = s > 0.0 && isfinite(s);
    ob[v] = unit ? (float)(nx / s) : 0.0f;
    ob[a.opitch + v] = unit ? (float)(ny / s) : 0.0f;
    ob[2 * a.opitch + v] = unit ? (float)(nz / s) : 0.0f;
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

}  // extern "C"
