// The per-pixel shading models of include/fr_hotpath.h, each stated ONCE: the gray one ("synthetic batches", SHADE) and the colour one
// ("colour shading", MODEL).  The shaders (fr_synth.hip) and the photometric losses (fr_photo.hip) run these functions, so the image a
// loss compares is its shader's image bit for bit.  fp32, every operation rounded on its own (-ffp-contract=off), IEEE division and
// square root.  Both models share the normal's part (shade_normal).
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

}  // namespace fr
