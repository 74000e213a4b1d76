// The barycentric weights of a pixel in its winning triangle, stated once.  fr_depth_interp.hip (interpolated depth) and
// fr_attr_interp.hip (interpolated vertex attributes) evaluate the same lines on the same gathers: what they interpolate differs,
// the weights and their screen-space derivatives do not.  A TU that includes this is compiled without contraction.
#pragma once
#include "fr_common.h"

namespace fr {

// get_point_weight in its source order (fp64 on the widened fp32 inputs; every product and sum rounds on its own).
// P: [vertex][xyz]; (px, py) = (column, row).
struct PointWeight {
    double v0x, v0y, v1x, v1y;
    double dot00, dot01, dot11, inv;
    double w[3];   // (1 - u - v, v, u)
    bool flat;     // den == 0: no plane, the op's own flat value stands
};
__device__ __forceinline__ PointWeight point_weight(const float (&P)[3][3], int px, int py) {
    PointWeight s;
    const double x1 = (double)P[0][0], y1 = (double)P[0][1];
    s.v0x = (double)P[2][0] - x1; s.v0y = (double)P[2][1] - y1;
    s.v1x = (double)P[1][0] - x1; s.v1y = (double)P[1][1] - y1;
    const double v2x = (double)px - x1, v2y = (double)py - y1;
    s.dot00 = s.v0x * s.v0x + s.v0y * s.v0y;
    s.dot01 = s.v0x * s.v1x + s.v0y * s.v1y;
    const double dot02 = s.v0x * v2x + s.v0y * v2y;
    s.dot11 = s.v1x * s.v1x + s.v1y * s.v1y;
    const double dot12 = s.v1x * v2x + s.v1y * v2y;
    const double den = s.dot00 * s.dot11 - s.dot01 * s.dot01;
    s.flat = den == 0;
    s.inv = s.flat ? 0.0 : 1 / den;
    const double u = (s.dot11 * dot02 - s.dot01 * dot12) * s.inv;
    const double v = (s.dot00 * dot12 - s.dot01 * dot02) * s.inv;
    s.w[0] = (1 - u) - v; s.w[1] = v; s.w[2] = u;
    return s;
}

// d u / d (pixel) and d v / d (pixel) of a triangle with area: what a quantity interpolated by w moves by per pixel step
struct WeightSlopes {
    double gux, guy, gvx, gvy;
};
__device__ __forceinline__ WeightSlopes weight_slopes(const PointWeight& s) {
    WeightSlopes g;
    g.gux = (s.dot11 * s.v0x - s.dot01 * s.v1x) * s.inv; g.guy = (s.dot11 * s.v0y - s.dot01 * s.v1y) * s.inv;
    g.gvx = (s.dot00 * s.v1x - s.dot01 * s.v0x) * s.inv; g.gvy = (s.dot00 * s.v1y - s.dot01 * s.v0y) * s.inv;
    return g;
}

// the nine values of an ok pixel out of three rows of pitch `pitch`: vertex coordinates, or any three-channel per-vertex attribute
__device__ __forceinline__ void gather_tri(const float* __restrict__ vb, long long vpitch, const int (&id)[3], float (&P)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) P[k][c] = vb[(size_t)c * vpitch + id[k]];
}

}  // namespace fr
