// Depth-map normals (opt-in; include/fr_hotpath.h, "depth-map normals"): the normal map of a depth map on the pixel grid, in the
// renderer's conventions, masked to the face and exact at the mask's edges, with its backward.  One streaming pass per direction.
//
//   depth_normals_forward_kernel    a workgroup owns a DN_TW x DN_TH = 32 x 16 pixel tile of one face, one lane per pixel (a wave is
//                                   two 32-pixel row segments: 2 x 384 contiguous bytes of the normal plane).  Every lane reads its own
//                                   five-point stencil straight from global memory (the neighbours' lines are the workgroup's own
//                                   L1 lines) in two rounds -- the five mask words together, then the valid depths together -- and
//                                   stores three floats.  No LDS, no barrier.
//   depth_normals_backward_kernel   the same tile.  CHOICE: the per-pixel adjoints e_x, e_y are STAGED IN LDS, not recomputed by their
//                                   readers.  A pixel's gradient gathers e_x of its left / right and e_y of its upper / lower
//                                   neighbour; each e costs the whole forward of its pixel (a float64 square root and five float64
//                                   divisions), so recomputing would run that five times per output.  Instead every lane evaluates its
//                                   own pixel once, the first 2 DN_TH + 2 DN_TW = 96 threads evaluate the halo (the columns left and
//                                   right of the tile for e_x, the rows above and below for e_y; no corners), each e already scaled by
//                                   the magnitude of its coefficient (0.5 central, 1 one-sided; exact), and after one barrier every lane
//                                   adds its six terms in the header's order: 1.19 evaluations per output instead of 5, in 8,960 bytes
//                                   of static LDS.
// A gather: no atomics, no workspace.  Each output is a function of the 13-point neighbourhood of its pixel and of nothing else --
// the halo lanes run the SAME device function on the same inputs as the lane that owns the pixel in the neighbouring tile.
#include "fr_common.h"

#include <cmath>

namespace fr {

constexpr int DN_TW = 32, DN_TH = 16;          // tile: one lane per pixel
constexpr int DN_THREADS = DN_TW * DN_TH;      // 8 waves
constexpr int DN_HALO = 2 * DN_TH + 2 * DN_TW; // halo evaluations of a backward workgroup

struct DnArgs {
    const float* depth;   // [B,H,W]
    const float* mask;    // [B,H,W] or null
    const float* gn;      // [B,H,W,3]   (backward)
    float* normal;        // [B,H,W,3]   (forward)
    float* gd;            // [B,H,W]     (backward)
    int H, W;
};

// one face's planes
struct DnFace {
    const float* depth;
    const float* mask;
    int H, W;
};

// The validity of a pixel and of its four neighbours.  valid: inside the image and (no mask or mask >= 0; a NaN compares false).
// The five mask words are read TOGETHER, before anything depends on one of them (one memory round trip, not two); L, R, U, D mean
// something only where P holds.
struct DnStencil {
    bool P, L, R, U, D;
    size_t at;   // the pixel's element offset in its face (0 outside the image)
};
__device__ __forceinline__ DnStencil dn_stencil(const DnFace& f, int r, int c) {
    DnStencil s;
    const bool ip = r >= 0 && r < f.H && c >= 0 && c < f.W;
    const bool il = ip && c > 0, ir = ip && c + 1 < f.W, iu = ip && r > 0, id = ip && r + 1 < f.H;
    s.at = ip ? (size_t)r * f.W + c : 0;
    if (!f.mask) {
        s.P = ip; s.L = il; s.R = ir; s.U = iu; s.D = id;
        return s;
    }
    // (unconditional loads at clamped offsets -- a neighbour outside the image reads the pixel's own word, a pixel outside the image
    // word 0 -- so that the five go out together; a predicated load each would wait for the one before it)
    const float* m = f.mask + s.at;
    const float m0 = m[0], m1 = m[il ? -1 : 0], m2 = m[ir ? 1 : 0];
    const float m3 = m[iu ? -(ptrdiff_t)f.W : 0], m4 = m[id ? (ptrdiff_t)f.W : 0];
    const float mp = ip ? m0 : -1.0f, ml = il ? m1 : -1.0f, mr = ir ? m2 : -1.0f, mu = iu ? m3 : -1.0f, md = id ? m4 : -1.0f;
    s.P = mp >= 0.0f; s.L = ml >= 0.0f; s.R = mr >= 0.0f; s.U = mu >= 0.0f; s.D = md >= 0.0f;
    return s;
}

// the difference along one axis: lo / hi = validity of the neighbour before / after the pixel, z_lo / z_hi / z_p the depths (z_lo and
// z_hi mean something only where valid; z_p enters a one-sided difference only; what is not used is selected away, never multiplied)
__device__ __forceinline__ double dn_diff(bool lo, bool hi, double z_lo, double z_hi, double z_p) {
    return (lo && hi) ? (z_hi - z_lo) * 0.5 : (hi ? z_hi - z_p : (lo ? z_p - z_lo : 0.0));
}

// the forward's quantities at a VALID pixel.  The five depths are read together, at clamped offsets: an invalid neighbour's depth is
// never read -- the pixel's own is read in its place and selected away in dn_diff.
struct DnPix {
    double dx, dy, s;
};
__device__ __forceinline__ DnPix dn_pixel(const DnFace& f, const DnStencil& v) {
    const float* z = f.depth + v.at;
    const float zp = z[0], zl = z[v.L ? -1 : 0], zr = z[v.R ? 1 : 0];
    const float zu = z[v.U ? -(ptrdiff_t)f.W : 0], zd = z[v.D ? (ptrdiff_t)f.W : 0];
    DnPix p;
    p.dx = dn_diff(v.L, v.R, (double)zl, (double)zr, (double)zp);
    p.dy = dn_diff(v.U, v.D, (double)zu, (double)zd, (double)zp);
    p.s = sqrt((p.dx * p.dx + p.dy * p.dy) + 1.0);
    return p;
}

// the backward's quantities of one pixel q: wx = |coefficient of dx(q) on a neighbour| * e_x(q) (0.5 central, 1 one-sided), wy alike;
// ox, oy = the pixel's own terms; its neighbours' validity.  An invalid q (or one outside the image) gives zeros and reads nothing
// but its mask.
struct DnAdj {
    double wx, wy, ox, oy;
    bool valid, L, R, U, D;
};
__device__ __forceinline__ DnAdj dn_adjoint(const DnFace& f, const float* gn, int r, int c) {
    DnAdj a;
    a.wx = 0.0; a.wy = 0.0; a.ox = 0.0; a.oy = 0.0;
    a.L = a.R = a.U = a.D = false;
    const DnStencil v = dn_stencil(f, r, c);
    a.valid = v.P;
    if (!v.P) return a;
    a.L = v.L; a.R = v.R; a.U = v.U; a.D = v.D;
    const float* g = gn + v.at * 3;
    const float g0 = g[0], g1 = g[1], g2 = g[2];   // (issued beside the depth reads of dn_pixel)
    const DnPix p = dn_pixel(f, v);
    const double gx = (double)g0, gy = (double)g1, gz = (double)g2;
    const double nx = -p.dx / p.s, ny = -p.dy / p.s, nz = 1.0 / p.s;   // float64, NOT rounded to fp32
    const double d = (gx * nx + gy * ny) + gz * nz;
    const double ex = -((gx - nx * d) / p.s);
    const double ey = -((gy - ny * d) / p.s);
    a.wx = (v.L && v.R) ? ex * 0.5 : ex;
    a.wy = (v.U && v.D) ? ey * 0.5 : ey;
    a.ox = (v.R && !v.L) ? -ex : ((v.L && !v.R) ? ex : 0.0);   // own coefficient: -1 "R only", +1 "L only", else the term is +0.0
    a.oy = (v.D && !v.U) ? -ey : ((v.U && !v.D) ? ey : 0.0);
    return a;
}

__global__ __launch_bounds__(DN_THREADS) void depth_normals_forward_kernel(DnArgs a) {
    const int c = blockIdx.x * DN_TW + threadIdx.x, r = blockIdx.y * DN_TH + threadIdx.y;
    if (r >= a.H || c >= a.W) return;   // (no barrier in this kernel)
    const size_t face = (size_t)blockIdx.z * ((size_t)a.H * a.W);
    const DnFace f{a.depth + face, a.mask ? a.mask + face : nullptr, a.H, a.W};
    const DnStencil v = dn_stencil(f, r, c);
    float* o = a.normal + (face + v.at) * 3;
    if (!v.P) {
        o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
        return;
    }
    const DnPix p = dn_pixel(f, v);
    o[0] = (float)(-p.dx / p.s);
    o[1] = (float)(-p.dy / p.s);
    o[2] = (float)(1.0 / p.s);
}

__global__ __launch_bounds__(DN_THREADS) void depth_normals_backward_kernel(DnArgs a) {
    __shared__ double wx[DN_TH][DN_TW + 2];   // column 0 / DN_TW + 1: the halo left / right of the tile
    __shared__ double wy[DN_TH + 2][DN_TW];   // row 0 / DN_TH + 1: the halo above / below
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c0 = blockIdx.x * DN_TW, r0 = blockIdx.y * DN_TH;
    const size_t face = (size_t)blockIdx.z * ((size_t)a.H * a.W);
    const DnFace f{a.depth + face, a.mask ? a.mask + face : nullptr, a.H, a.W};
    const float* gn = a.gn + face * 3;
    const DnAdj me = dn_adjoint(f, gn, r0 + ty, c0 + tx);
    wx[ty][tx + 1] = me.wx;
    wy[ty + 1][tx] = me.wy;
    const int t = ty * DN_TW + tx;   // the first DN_HALO threads (waves 0 and 1) evaluate one halo pixel each, through ONE call
    if (t < DN_HALO) {
        const bool col_halo = t < 2 * DN_TH;   // left / right columns: e_x; else the rows above / below: e_y
        const int k = t - 2 * DN_TH;
        const int row = col_halo ? (t >> 1) : (k / DN_TW ? DN_TH : -1);
        const int col = col_halo ? ((t & 1) ? DN_TW : -1) : k % DN_TW;
        const DnAdj h = dn_adjoint(f, gn, r0 + row, c0 + col);
        if (col_halo) wx[row][col + 1] = h.wx;
        else wy[row + 1][col] = h.wy;
    }
    __syncthreads();
    const int r = r0 + ty, c = c0 + tx;
    if (r >= a.H || c >= a.W) return;
    float* o = a.gd + face + (size_t)r * a.W + c;
    if (!me.valid) {
        *o = 0.0f;
        return;
    }
    const double from_left = me.L ? wx[ty][tx] : 0.0;
    const double from_right = me.R ? -wx[ty][tx + 2] : 0.0;
    const double from_up = me.U ? wy[ty][tx] : 0.0;
    const double from_down = me.D ? -wy[ty + 2][tx] : 0.0;
    *o = (float)(((((me.ox + me.oy) + from_left) + from_right) + from_up) + from_down);
}

}  // namespace fr

// The launch geometry, chosen in ONE place: the launchers and the test hook both read it from here.
namespace {
struct DnGeom {
    int tiles_x, tiles_y;
};
DnGeom dn_geom(int H, int W) {
    return DnGeom{(W + fr::DN_TW - 1) / fr::DN_TW, (H + fr::DN_TH - 1) / fr::DN_TH};
}
// more than 2^31 - 65 pixels per face, or a grid the runtime does not take (faces in z, tile rows in y: 65,535 each)
bool dn_size_ok(int B, int H, int W) {
    return (long long)H * W <= 0x7FFFFFFFll - 64 && B <= 65535 && (H + fr::DN_TH - 1) / fr::DN_TH <= 65535;
}
constexpr size_t DN_LDS_BWD = (size_t)(fr::DN_TH * (fr::DN_TW + 2) + (fr::DN_TH + 2) * fr::DN_TW) * sizeof(double);

// What the two entry points share, in the order both answer: a negative size (FR_ERR_INVALID_ARG), an empty shape (FR_OK,
// nothing launched), the entry point's own pointers (FR_ERR_INVALID_ARG), a shape beyond one grid (FR_ERR_UNSUPPORTED); then
// the geometry, H and W of `a`, and the launch.
template <typename Kernel>
int dn_launch(Kernel kernel, fr::DnArgs& a, int B, int H, int W, bool pointers_ok, void* hip_stream) {
    if (B < 0 || H < 0 || W < 0) return FR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return FR_OK;
    if (!pointers_ok) return FR_ERR_INVALID_ARG;
    if (!dn_size_ok(B, H, W)) return FR_ERR_UNSUPPORTED;
    const DnGeom geo = dn_geom(H, W);
    a.H = H; a.W = W;
    hipLaunchKernelGGL(kernel, dim3((unsigned)geo.tiles_x, (unsigned)geo.tiles_y, (unsigned)B), dim3(fr::DN_TW, fr::DN_TH, 1), 0,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}
}  // namespace

extern "C" {

// test hook: out = {tile width, tile height, threads per workgroup, tiles across, tiles down, static LDS bytes of a backward
// workgroup}; zeros for an empty shape or one the launchers refuse
void fr_debug_depth_normals_geom(int B, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    if (B <= 0 || H <= 0 || W <= 0 || !dn_size_ok(B, H, W)) return;
    const DnGeom g = dn_geom(H, W);
    out[0] = fr::DN_TW; out[1] = fr::DN_TH; out[2] = fr::DN_THREADS; out[3] = g.tiles_x; out[4] = g.tiles_y;
    out[5] = (int)DN_LDS_BWD;
}

int fr_depth_normals_forward(const float* depth, const float* mask, int B, int H, int W, float* normal, void* hip_stream) {
    fr::DnArgs a{};
    a.depth = depth; a.mask = mask; a.normal = normal;
    return dn_launch(fr::depth_normals_forward_kernel, a, B, H, W, depth && normal, hip_stream);
}

int fr_depth_normals_backward(const float* grad_normal, const float* depth, const float* mask, int B, int H, int W,
                              float* grad_depth, void* hip_stream) {
    fr::DnArgs a{};
    a.depth = depth; a.mask = mask; a.gn = grad_normal; a.gd = grad_depth;
    return dn_launch(fr::depth_normals_backward_kernel, a, B, H, W, grad_normal && depth && grad_depth, hip_stream);
}

}  // extern "C"
