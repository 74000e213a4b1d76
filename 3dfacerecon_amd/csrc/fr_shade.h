// The per-pixel shading model of include/fr_hotpath.h ("synthetic batches", SHADE), stated ONCE: the shader (fr_synth.hip) and the
// photometric loss (fr_photo.hip) run this function, so the image the loss compares is the shader's image bit for bit.  fp32, every
// operation rounded on its own (-ffp-contract=off), IEEE division and square root.
#pragma once
#include "fr_common.h"

namespace fr {

struct Shade {
    float a;            // clamped channel mean
    float nx, ny, nz;   // the normal, flipped to n_z >= 0
    float hx, hy, hz;   // n^ = n / d
    float mag, d;       // mag after its replacement by 1; d = sqrtf(mag) + 1e-6f
    float s;            // ((l0 + l1 n^x) + l2 n^y) + l3 n^z
    bool flipped;       // n_z < 0 on input
    bool unit;          // mag was replaced by 1 (not mag > 1e-6f)
};

// -> I = a * (s < 0 ? 0 : s); the caller applies gain and offset.  l = light[b], four floats.
__device__ __forceinline__ float shade_pixel(float t0, float t1, float t2, float nx, float ny, float nz, const float* l, Shade& o) {
    // (x < 1e-6 ? 1e-6 : x: a NaN stays a NaN, as torch.clamp_min)
    o.a = fr::div3(((t0 < 1e-6f ? 1e-6f : t0) + (t1 < 1e-6f ? 1e-6f : t1)) + (t2 < 1e-6f ? 1e-6f : t2));
    o.flipped = nz < 0.0f;
    if (o.flipped) { nx = -nx; ny = -ny; nz = -nz; }
    float mag = (nx * nx + ny * ny) + nz * nz;
    o.unit = !(mag > 1e-6f);
    mag = o.unit ? 1.0f : mag;
    const float d = sqrtf(mag) + 1e-6f;
    o.nx = nx; o.ny = ny; o.nz = nz;
    o.mag = mag; o.d = d;
    o.hx = nx / d; o.hy = ny / d; o.hz = nz / d;
    o.s = ((l[0] + l[1] * o.hx) + l[2] * o.hy) + l[3] * o.hz;
    return o.a * (o.s < 0.0f ? 0.0f : o.s);
}

}  // namespace fr
