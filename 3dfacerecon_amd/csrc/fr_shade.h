// The per-pixel shading models of include/fr_hotpath.h, each stated ONCE: the gray one ("synthetic batches", SHADE) and the colour one
// ("colour shading", MODEL).  The shaders (fr_synth.hip) and the photometric losses (fr_photo.hip) run these functions, so the image a
// loss compares is its shader's image bit for bit.  fp32, every operation rounded on its own (-ffp-contract=off), IEEE division and
// square root.  Both models share the normal's part (shade_normal).
// A model is a TYPE (GrayModel, ColourModel, at the end): its sizes, its state, its arithmetic and the two pieces of the loss's
// backward that are not the same expression in both.  The shader and the loss are written once, over that type.
#pragma once
#include "fr_common.h"

namespace fr {

struct ShadeNormal {
    float nx, ny, nz;   // the normal, flipped to n_z >= 0
    float hx, hy, hz;   // n^ = n / d
    float mag, d;       // mag after its replacement by 1; d = sqrtf(mag) + 1e-6f
    bool flipped;       // n_z < 0 on input
    bool unit;          // mag was replaced by 1 (not mag > 1e-6f)
};

struct Shade : ShadeNormal {
    float a;            // clamped channel mean
    float s;            // ((l0 + l1 n^x) + l2 n^y) + l3 n^z
};

struct ShadeRGB : ShadeNormal {
    float a[3];         // the clamped albedo, per channel
    float s[3];         // the nine-term chain, per channel
    float h[9];         // the basis H0 .. H8 (h[0] = 1 is never multiplied)
};

// the flip, mag, its replacement by 1, d and n^
__device__ __forceinline__ void shade_normal(float nx, float ny, float nz, ShadeNormal& o) {
    o.flipped = nz < 0.0f;
    if (o.flipped) { nx = -nx; ny = -ny; nz = -nz; }
    float mag = (nx * nx + ny * ny) + nz * nz;
    o.unit = !(mag > 1e-6f);
    mag = o.unit ? 1.0f : mag;
    const float d = sqrtf(mag) + 1e-6f;
    o.nx = nx; o.ny = ny; o.nz = nz;
    o.mag = mag; o.d = d;
    o.hx = nx / d; o.hy = ny / d; o.hz = nz / d;
}

// -> I = a * (s < 0 ? 0 : s); the caller applies gain and offset.  l = light[b], four floats.
__device__ __forceinline__ float shade_pixel(float t0, float t1, float t2, float nx, float ny, float nz, const float* l, Shade& o) {
    // (x < 1e-6 ? 1e-6 : x: a NaN stays a NaN, as torch.clamp_min)
    o.a = fr::div3(((t0 < 1e-6f ? 1e-6f : t0) + (t1 < 1e-6f ? 1e-6f : t1)) + (t2 < 1e-6f ? 1e-6f : t2));
    shade_normal(nx, ny, nz, o);
    o.s = ((l[0] + l[1] * o.hx) + l[2] * o.hy) + l[3] * o.hz;
    return o.a * (o.s < 0.0f ? 0.0f : o.s);
}

// The colour model: per-channel albedo under a second-order lighting per channel.  The basis is the nine polynomials
//   H0 = 1, H1 = n^x, H2 = n^y, H3 = n^z, H4 = n^x n^y, H5 = n^x n^z, H6 = n^y n^z, H7 = n^x n^x - n^y n^y, H8 = 3 (n^z n^z) - 1
// -- the real spherical harmonics up to order two WITHOUT their normalisation: those constants, and the cosine lobe's, are folded
// into the coefficients.  l = light[b], [3][9] channel-major.  -> I[c] = a_c (s_c < 0 ? 0 : s_c); the caller applies gain and offset.
__device__ __forceinline__ void shade_pixel_rgb(float t0, float t1, float t2, float nx, float ny, float nz, const float* l, ShadeRGB& o,
                                                float (&I)[3]) {
    o.a[0] = t0 < 1e-6f ? 1e-6f : t0;
    o.a[1] = t1 < 1e-6f ? 1e-6f : t1;
    o.a[2] = t2 < 1e-6f ? 1e-6f : t2;
    shade_normal(nx, ny, nz, o);
    o.h[0] = 1.0f; o.h[1] = o.hx; o.h[2] = o.hy; o.h[3] = o.hz;
    o.h[4] = o.hx * o.hy; o.h[5] = o.hx * o.hz; o.h[6] = o.hy * o.hz;
    o.h[7] = o.hx * o.hx - o.hy * o.hy;
    o.h[8] = 3.0f * (o.hz * o.hz) - 1.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float s = l[9 * c] + l[9 * c + 1] * o.h[1];
#pragma unroll
        for (int k = 2; k < 9; k++) s = s + l[9 * c + k] * o.h[k];
        o.s[c] = s;
        I[c] = o.a[c] * (s < 0.0f ? 0.0f : s);
    }
}

// the gray of an RGB pixel (the weights of utils/data_process.py)
__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.3f * r + 0.59f * g) + 0.11f * b; }

// ---- a model as a type ----------------------------------------------------------------------------------------------------------------
// NC image channels, NK lighting terms per channel (light[b] is [NC][NK], a pixel of the image [NC]); State, what shade() leaves of
// a covered pixel; albedo / chain: a_c and s_c; basis: H_k, k >= 1 (H_0 = 1 is never multiplied).  The backward's two pieces, in
// float64 on the widened values, of image channel c with dI = d sse / d I_c and lit = s_c > 0:
//   tex_gradient    writes the elements of gt that channel c reaches.  NOT one expression: the gray image reads all three texture
//                   channels through their mean -- ONE value (dI s) (1 / 3), gated by each channel's own clamp -- the colour image's
//                   channel c reads texture channel c alone: dI s_c.
//   chain_gradient  q = lit ? dI a_c : 0 times the derivative of s_c with respect to n^, into g~.  NOT one accumulation: the gray
//                   model ASSIGNS its one product, the colour model ADDS each channel's to g~, which starts at +0.0.  On an unlit
//                   pixel q = 0.0 and a negative coefficient makes the product -0.0: assigned it stays -0.0, added to +0.0 it becomes
//                   +0.0, and ph_normal_backward carries the sign into grad_normal.  Either model written the other's way moves bits.
struct GrayModel {
    static constexpr int NC = 1, NK = 4;
    using State = Shade;
    static __device__ __forceinline__ void shade(const float* t, const float* n, const float* l, State& o, float (&I)[NC]) {
        I[0] = shade_pixel(t[0], t[1], t[2], n[0], n[1], n[2], l, o);
    }
    static __device__ __forceinline__ float albedo(const State& o, int) { return o.a; }
    static __device__ __forceinline__ float chain(const State& o, int) { return o.s; }
    static __device__ __forceinline__ float basis(const State& o, int k) { return k == 1 ? o.hx : k == 2 ? o.hy : o.hz; }
    static __device__ __forceinline__ void tex_gradient(const State& o, int, double dI, bool lit, const float* t, float (&gt)[3]) {
        const float gc = (float)((dI * (double)o.s) * (1.0 / 3.0));
#pragma unroll
        for (int k = 0; k < 3; k++) gt[k] = (lit && !(t[k] < 1e-6f)) ? gc : 0.0f;
    }
    static __device__ __forceinline__ void chain_gradient(const State&, const float* l, double q, double& gx, double& gy, double& gz) {
        gx = q * (double)l[1]; gy = q * (double)l[2]; gz = q * (double)l[3];
    }
};

struct ColourModel {
    static constexpr int NC = 3, NK = 9;
    using State = ShadeRGB;
    static __device__ __forceinline__ void shade(const float* t, const float* n, const float* l, State& o, float (&I)[NC]) {
        shade_pixel_rgb(t[0], t[1], t[2], n[0], n[1], n[2], l, o, I);
    }
    static __device__ __forceinline__ float albedo(const State& o, int c) { return o.a[c]; }
    static __device__ __forceinline__ float chain(const State& o, int c) { return o.s[c]; }
    static __device__ __forceinline__ float basis(const State& o, int k) { return o.h[k]; }
    static __device__ __forceinline__ void tex_gradient(const State& o, int c, double dI, bool lit, const float* t, float (&gt)[3]) {
        gt[c] = (lit && !(t[c] < 1e-6f)) ? (float)(dI * (double)o.s[c]) : 0.0f;
    }
    // l = light[b][c]
    static __device__ __forceinline__ void chain_gradient(const State& o, const float* l, double q, double& gx, double& gy, double& gz) {
        const double hx = (double)o.hx, hy = (double)o.hy, hz = (double)o.hz;
        const double l1 = (double)l[1], l2 = (double)l[2], l3 = (double)l[3], l4 = (double)l[4], l5 = (double)l[5], l6 = (double)l[6],
                     l7 = (double)l[7], l8 = (double)l[8];
        const double dx = ((l1 + l4 * hy) + l5 * hz) + (2.0 * l7) * hx;
        const double dy = ((l2 + l4 * hx) + l6 * hz) - (2.0 * l7) * hy;
        const double dz = ((l3 + l5 * hx) + l6 * hy) + (6.0 * l8) * hz;
        gx = gx + q * dx; gy = gy + q * dy; gz = gz + q * dz;
    }
};

}  // namespace fr
