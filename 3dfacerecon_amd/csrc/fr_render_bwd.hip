// render_depth backward: zeros + scatter-add of g/3 to the z row (render_depth_op.cc:345-363), by the owner-scatter scheme of
// fr_owner_scatter.h with ONE term per pixel, c = (g * 1.0f) / 3.0f (fp32, as :361 computes it), and one accumulator per vertex.
// k is chosen per face from max|g| so that the largest term has at least 38 significant bits below the int64 headroom the H*W*3
// possible terms need: every term is represented to 2^-39 of the face's largest term, i.e. the result is the exactly rounded
// real sum up to  n_terms * 2^-39 * max|c|  -- at least as close to the real-number sum as the reference's sequential fp32 order
// (whose error grows with the partial sums), and identical run to run.
// The owner writes its range of all three rows (x and y rows: zeros, render_depth_op.cc:359-363), or of the z row alone.
// A face whose gradients contain Inf / NaN takes fp32 LDS atomics.
//   bwd_records_kernel, bwd_records_form_kernel + render_backward_kernel<true>    with a workspace: the owners stream records
//   render_backward_kernel<false>                                                 without: every owner gathers the ids itself
#include "fr_owner_scatter.h"

namespace fr {

constexpr int BWD_BLOCK = OWNER_BLOCK;
constexpr int BWD_RANGE_MAX = 16 * 1024;  // vertices per owner workgroup (8 B each: 128 KiB of LDS)
constexpr int BWD_TOP = 40;               // c = g/3 is at most two binades below max|g|: the largest term lands in [2^38, 2^40); up
                                          // to 2^21 terms (3 per pixel) stay below 2^62

struct BwdRenderArgs {
    const float* depth_grad;  // [B,H,W,1]
    const int4* rec;          // [B,H,W] per-pixel records {p1,p2,p3,g bits} (bwd_records_kernel), or null: float ids
    const uint2* partial;     // [B,chunks] {largest |g| bits, Inf/NaN flag} of each 1,024-pixel chunk
    int B, chunks;
    const float* tri;         // [3,ntri]
    const float* tri_ind;     // [B,H,W,1]
    float* vertex_grad;       // [B,3,nver]
    int nver, ntri, npix;     // npix = H*W
    int splits, range;        // owner workgroups per face, vertices per owner
    int shift;                // headroom bits given up by images above 2^20 pixels: ceil(log2 npix) - 20, else 0
    // fr_decode_render_backward: the records pass FORMS the pixel gradient from up to three planes (each may be null) ...
    const float* g_net;       // [B,H,W,7] gradient of net_input: channel 0 only
    const float* g_dimg;      // [B,H,W,1] gradient of depth_img
    const float* im_gray;     // [B,H,W,1]
    const float* depth;       // [B,H,W,1] forward output
    // ... and the owners write ONLY the z row, face b at vertex_grad + b * zpitch (0: the dense [B,3,nver] tensor, x / y zeroed)
    long long zpitch;
};

// Per-face scan of the plain (no-workspace) variant: largest |g| over the covered pixels (deviation 2: tri_ind < 0 is not
// covered) + an Inf/NaN flag, by one 1,024-thread workgroup, no atomics (nothing to zero).
__device__ __forceinline__ uint2 bwd_face_max(const BwdRenderArgs& a, int b, uint32_t* red /*[2 * BWD_BLOCK / 64]*/) {
    const int tid = threadIdx.x, npix = a.npix;
    const float* __restrict__ g = a.depth_grad + (size_t)b * npix;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
    uint32_t m = 0, bad = 0;
    constexpr int PU = 8;  // pixels per lane per trip, all loads issued before the first use
    for (int i0 = tid; i0 < npix; i0 += PU * BWD_BLOCK) {
        float gq[PU], tq[PU];
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const int i = min(i0 + u * BWD_BLOCK, npix - 1);
            gq[u] = g[i];
            tq[u] = ti[i];
        }
#pragma unroll
        for (int u = 0; u < PU; u++)
            if (i0 + u * BWD_BLOCK < npix && pixel_tri(tq[u], a.ntri) >= 0) track_term(__float_as_uint(gq[u]), m, bad);
    }
    return block_max<BWD_BLOCK>(m, bad, red);
}

// Records pass of the workspace variant: a 16-byte record {p1, p2, p3, g bits} per pixel -- p1 = -1 for pixels that contribute
// nothing (background; deviation 3: an id outside [0,nver)).  Lane-consecutive pixels: a gather instruction's 64 lanes hold
// neighbouring triangles.
// FORM (fr_decode_render_backward): g is not read from depth_grad but formed here, per pixel, in fp32 without contraction --
//   g = +0;  g += (g_net[..,0] * im_gray) * m1, m1 = (1e-6f <= depth && depth <= 1.0f);  g += g_dimg * m2, m2 = (depth >= 1e-6f);
//   g += g_depth -- absent planes skipped, the masks MULTIPLIED in as 1.0f / 0.0f (an infinite gradient on a masked pixel is a
// NaN, as in the torch expression this replaces).  The extra planes are streamed like g and tri_ind: lane-consecutive pixels
// (the 7-channel plane at a 28-byte stride: seven lines per 64 lanes, each line shared by the lanes that touch it).
template <bool FORM>
__device__ __forceinline__ void bwd_records_body(const BwdRenderArgs& a, int4* rec, uint2* partial, int chunks) {
    __shared__ uint32_t red[8];
    const int b = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - b * chunks;
    const int tid = threadIdx.x;
    const float* __restrict__ tri0 = a.tri;
    const float* __restrict__ tri1 = a.tri + a.ntri;
    const float* __restrict__ tri2 = a.tri + 2 * (size_t)a.ntri;
    const float* __restrict__ g = a.depth_grad + (size_t)b * a.npix;
    const float* __restrict__ ti = a.tri_ind + (size_t)b * a.npix;
    int4* __restrict__ out = rec + (size_t)b * a.npix;
    constexpr int PU = REC_PX / 256;
    const int i0 = ch * REC_PX + tid;
    float gq[PU], tq[PU];
    if constexpr (!FORM) {
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const int i = min(i0 + u * 256, a.npix - 1);
            gq[u] = g[i];
            tq[u] = ti[i];
        }
    } else {
        const bool hn = a.g_net != nullptr, hi = a.g_dimg != nullptr, hd = a.depth_grad != nullptr;   // (uniform)
        float gn[PU], gi[PU], gd[PU], im[PU], dp[PU];
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const size_t i = (size_t)b * a.npix + min(i0 + u * 256, a.npix - 1);
            tq[u] = a.tri_ind[i];
            gn[u] = gi[u] = gd[u] = im[u] = dp[u] = 0.f;
            if (hn) { gn[u] = a.g_net[i * 7]; im[u] = a.im_gray[i]; }
            if (hi) gi[u] = a.g_dimg[i];
            if (hn || hi) dp[u] = a.depth[i];
            if (hd) gd[u] = a.depth_grad[i];
        }
#pragma unroll
        for (int u = 0; u < PU; u++) {
            float gg = 0.f;
            if (hn) gg = gg + (gn[u] * im[u]) * ((1e-6f <= dp[u] && dp[u] <= 1.0f) ? 1.0f : 0.0f);
            if (hi) gg = gg + gi[u] * ((dp[u] >= 1e-6f) ? 1.0f : 0.0f);
            if (hd) gg = gg + gd[u];
            gq[u] = gg;
        }
    }
    int id[PU][3];
    PixelTri px[PU];
#pragma unroll
    for (int u = 0; u < PU; u++) px[u] = pixel_tri_ids(tq[u], tri0, tri1, tri2, a.ntri, a.nver, id[u]);
    uint32_t m = 0, bad = 0;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int i = i0 + u * 256;
        if (i < a.npix) {
            out[i] = make_int4(px[u].ok ? id[u][0] : -1, id[u][1], id[u][2], (int)__float_as_uint(gq[u]));
            // the face's largest |g| over the COVERED pixels (the predicate of bwd_face_max), in parts
            if (px[u].covered) track_term(__float_as_uint(gq[u]), m, bad);
        }
    }
    chunk_publish(m, bad, red, &partial[(size_t)b * chunks + ch]);
}
__global__ __launch_bounds__(256) void bwd_records_kernel(BwdRenderArgs a, int4* rec, uint2* partial, int chunks) {
    bwd_records_body<false>(a, rec, partial, chunks);
}
__global__ __launch_bounds__(256) void bwd_records_form_kernel(BwdRenderArgs a, int4* rec, uint2* partial, int chunks) {
    bwd_records_body<true>(a, rec, partial, chunks);
}

// PACKED (workspace variant): the owners stream the per-pixel records of bwd_records_kernel (the id gathers -- repeated by
// every owner of the face, they are what the plain variant spends its time on -- were done once); otherwise float ids
// gathered in-kernel.
template <bool PACKED>
__global__ __launch_bounds__(BWD_BLOCK) void render_backward_kernel(BwdRenderArgs a) {
    // all LDS is dynamic (the launcher raises the dynamic limit to the CU's full 160 KiB, which leaves no room for
    // static objects): [range] accumulators, then two small per-wave reduction arrays
    extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // [range]
    uint32_t* red = reinterpret_cast<uint32_t*>(acc + a.range);               // [2 * BWD_BLOCK / 64]
    const int tid = threadIdx.x;
    int b, sp;
    owner_block_map(a.B, a.splits, &b, &sp);
    const int v0 = sp * a.range;
    const int v1 = min(a.nver, v0 + a.range);
    const int npix = a.npix, ntri = a.ntri, nver = a.nver;
    for (int i = tid; i < v1 - v0; i += BWD_BLOCK) acc[i] = 0ull;

    // the face's largest |g| over the covered pixels (max is order independent); c = g/3 is at most two binades below,
    // which the scale accounts for -- so the scan needs no division
    const uint2 mb = PACKED ? scope_max<BWD_BLOCK>(a.partial + (size_t)b * a.chunks, a.chunks, red) : bwd_face_max(a, b, red);
    const uint32_t m = mb.x, bad = mb.y;
    const FixedScale<BWD_TOP> fx(m, a.shift);
    float* facc = reinterpret_cast<float*>(acc);  // Inf / NaN gradients: fp32 LDS atomics in the same buffer
    if (bad) {
        __syncthreads();
        for (int i = tid; i < v1 - v0; i += BWD_BLOCK) facc[i] = 0.0f;
    }
    __syncthreads();
    // one contribution: c = (g * 1.0f) / 3.0f to the vertices of the pixel's triangle that this workgroup owns -- the division
    // and the fixed-point conversion come after the ownership test
    auto add = [&](float gv, int p1, int p2, int p3, bool in1, bool in2, bool in3) {
        const float c = gv * 1.0f / 3.0f;
        if (bad) {
            if (in1) atomicAdd(&facc[p1 - v0], c);
            if (in2) atomicAdd(&facc[p2 - v0], c);
            if (in3) atomicAdd(&facc[p3 - v0], c);
        } else {
            const unsigned long long q = fx.to_fixed(c);
            if (in1) fixed_add(&acc[p1 - v0], q);
            if (in2) fixed_add(&acc[p2 - v0], q);
            if (in3) fixed_add(&acc[p3 - v0], q);
        }
    };
    if ((m != 0 || bad) && PACKED) {
        // the owners stream the face's records: no gathers, no dependent loads
        owner_stream<BWD_BLOCK>(a.rec + (size_t)b * npix, npix, v0, v1, [&](int, const int4& q0, bool in1, bool in2, bool in3) {
            add(__uint_as_float((uint32_t)q0.w), q0.x, q0.y, q0.z, in1, in2, in3);
        });
    }
    if ((m != 0 || bad) && !PACKED) {
        // The scan.  Lane l of a trip's u-th slice takes pixel i0 + u * BLOCK: the 64 lanes of a gather instruction hold
        // 64 CONSECUTIVE pixels -> neighbouring triangles -> a few cache lines of the id table per instruction (four
        // pixels per lane, the obvious 16-byte-load mapping, puts every lane of a gather on its own line and runs the
        // texture addresser at one lane per cycle).  Software pipelined: the (g, tri_ind) values of the NEXT trip are
        // requested before the id gathers of the current one are consumed.
        const float* __restrict__ g = a.depth_grad + (size_t)b * npix;
        const float* __restrict__ ti = a.tri_ind + (size_t)b * npix;
        const float* __restrict__ tri0 = a.tri;
        const float* __restrict__ tri1 = a.tri + ntri;
        const float* __restrict__ tri2 = a.tri + 2 * (size_t)ntri;
        constexpr int QU = 8;
        float gv[QU], tv[QU];
#pragma unroll
        for (int u = 0; u < QU; u++) {
            const int i = tid + u * BWD_BLOCK;
            gv[u] = 0.f; tv[u] = -1.f;
            if (i < npix) { gv[u] = g[i]; tv[u] = ti[i]; }
        }
        for (int i0 = tid; i0 < npix; i0 += QU * BWD_BLOCK) {
            int id[QU][3];
            PixelTri px[QU];
            float gc[QU];
#pragma unroll
            for (int u = 0; u < QU; u++) {
                px[u] = pixel_tri_ids(tv[u], tri0, tri1, tri2, ntri, nver, id[u]);
                gc[u] = gv[u];
            }
#pragma unroll
            for (int u = 0; u < QU; u++) {
                const int in = i0 + (QU + u) * BWD_BLOCK;
                tv[u] = -1.f;
                if (in < npix) { gv[u] = g[in]; tv[u] = ti[in]; }
            }
#pragma unroll
            for (int u = 0; u < QU; u++) {
                if (!px[u].ok) continue;
                const int p1 = id[u][0], p2 = id[u][1], p3 = id[u][2];
                const bool in1 = p1 >= v0 && p1 < v1, in2 = p2 >= v0 && p2 < v1, in3 = p3 >= v0 && p3 < v1;
                if (in1 || in2 || in3) add(gc[u], p1, p2, p3, in1, in2, in3);
            }
        }
    }
    __syncthreads();
    auto total = [&](int i) { return bad ? facc[i] : fx.round(acc[i]); };
    if (a.zpitch > 0) {   // (uniform) z-only mode: the x / y rows -- zeros -- are neither written here nor read by the consumer
        float* zrow = a.vertex_grad + (size_t)b * a.zpitch;
        for (int i = tid; i < v1 - v0; i += BWD_BLOCK) zrow[v0 + i] = total(i);
        return;
    }
    float* gx = a.vertex_grad + (size_t)b * 3 * nver;
    float* gy = gx + nver;
    float* gz = gy + nver;
    for (int i = tid; i < v1 - v0; i += BWD_BLOCK) {
        gx[v0 + i] = 0.0f;
        gy[v0 + i] = 0.0f;
        gz[v0 + i] = total(i);
    }
}

}  // namespace fr

// workspace of the ws variant: one 16-byte record per pixel of the batch + one {max, flag} pair per 1,024-pixel chunk
size_t fr_render_backward_workspace_bytes_impl(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t npix = (size_t)H * W, chunks = (npix + fr::REC_PX - 1) / fr::REC_PX;
    return (size_t)B * npix * sizeof(int4) + (size_t)B * chunks * sizeof(uint2);
}

// The launch geometry of the backward, chosen in ONE place: the launcher below and the test hook
// fr_debug_render_bwd_geom both read it from here.  (The splits are clamped to one vertex per owner.)
static fr::OwnerGeom render_bwd_geom(int B, int nver, long long npix) {
    return fr::owner_geom(B, nver, npix, npix, fr::BWD_RANGE_MAX, 1, 1);
}

// test hook (tests/test_capi_cpu.py, tests/test_render_backward_exact_gpu.py): the geometry the backward launcher would
// choose, without a GPU.  out = {splits, range, shift, chunks, lds_bytes, xcd_map}; all zero for a shape that launches
// no kernel or is refused
extern "C" void fr_debug_render_bwd_geom(int B, int nver, int H, int W, int* out) {
    for (int i = 0; i < 6; i++) out[i] = 0;
    const long long npix = (long long)H * W;
    if (B <= 0 || nver <= 0 || H <= 0 || W <= 0 || npix > 0x7FFFFFFFll) return;
    fr::owner_geom_report(render_bwd_geom(B, nver, npix), B, out);
}

static int launch_render_backward_impl(const FrPixelGrad* pg, const float* depth_grad, const float* tri, const float* tri_ind,
                                       float* vertex_grad, long long zpitch, int B, int nver, int ntri, int H, int W,
                                       void* workspace, size_t ws_bytes, hipStream_t stream) {
    using namespace fr;
    // (z-only mode: `vertex_grad` is the [B, zpitch] plane; its pad floats are never written or read)
    const size_t bytes = zpitch > 0 ? (size_t)B * zpitch * sizeof(float) : (size_t)B * 3 * nver * sizeof(float);
    const long long npix = (long long)H * W;
    if (npix * B == 0 || ntri == 0 || nver == 0) return owner_no_terms(vertex_grad, bytes, false, stream);
    if (npix > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    const OwnerGeom geo = render_bwd_geom(B, nver, npix);
    const int splits = geo.splits, chunks = geo.chunks;
    if ((long long)B * splits > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
    BwdRenderArgs a;
    a.depth_grad = depth_grad; a.tri = tri; a.tri_ind = tri_ind; a.vertex_grad = vertex_grad;
    a.nver = nver; a.ntri = ntri; a.npix = (int)npix; a.splits = splits; a.range = geo.range; a.shift = geo.shift;
    a.g_net = pg ? pg->g_net_input : nullptr; a.g_dimg = pg ? pg->g_depth_img : nullptr;
    a.im_gray = pg ? pg->im_gray : nullptr; a.depth = pg ? pg->depth : nullptr;
    a.zpitch = zpitch;
    // with a workspace one pre-kernel resolves every pixel to its vertex ids once (instead of once per owner workgroup)
    // and the owners stream 16-byte records
    const bool packed = workspace && ws_bytes >= fr_render_backward_workspace_bytes_impl(B, H, W) &&
                        (((uintptr_t)workspace) & 15) == 0;
    if (pg && !packed) return FR_ERR_WORKSPACE;   // (the formed gradient exists in the records only)
    int4* rec = reinterpret_cast<int4*>(workspace);
    uint2* partial = reinterpret_cast<uint2*>(rec + (size_t)B * npix);
    a.rec = packed ? rec : nullptr;
    a.partial = packed ? partial : nullptr;
    a.B = B; a.chunks = chunks;
    const size_t lds = geo.lds;
    static fr_lds_flags_t lds_ok[2][64];
    if (packed) {
        if ((long long)B * chunks > 0x7FFFFFFFll) return FR_ERR_UNSUPPORTED;
        if (pg) hipLaunchKernelGGL(bwd_records_form_kernel, dim3((unsigned)(B * chunks)), dim3(256), 0, stream, a, rec, partial, chunks);
        else hipLaunchKernelGGL(bwd_records_kernel, dim3((unsigned)(B * chunks)), dim3(256), 0, stream, a, rec, partial, chunks);
        if (fr_allow_full_lds(reinterpret_cast<const void*>(&render_backward_kernel<true>), lds_ok[1]) != hipSuccess)
            return FR_ERR_LAUNCH;
        hipLaunchKernelGGL(render_backward_kernel<true>, dim3((unsigned)(B * splits)), dim3(BWD_BLOCK), lds, stream, a);
    } else {
        if (fr_allow_full_lds(reinterpret_cast<const void*>(&render_backward_kernel<false>), lds_ok[0]) != hipSuccess)
            return FR_ERR_LAUNCH;
        hipLaunchKernelGGL(render_backward_kernel<false>, dim3((unsigned)(B * splits)), dim3(BWD_BLOCK), lds, stream, a);
    }
    return hipGetLastError() == hipSuccess ? FR_OK : FR_ERR_LAUNCH;
}

int fr_launch_render_backward(const float* depth_grad, const float* tri, const float* tri_ind, float* vertex_grad,
                              int B, int nver, int ntri, int H, int W, void* workspace, size_t ws_bytes,
                              hipStream_t stream) {
    return launch_render_backward_impl(nullptr, depth_grad, tri, tri_ind, vertex_grad, 0, B, nver, ntri, H, W, workspace,
                                       ws_bytes, stream);
}

// fr_decode_render_backward's first half: pixel gradient formed in the records pass, owners write the pitched z plane only
int fr_launch_render_backward_z(const FrPixelGrad& pg, const float* tri, const float* tri_ind, float* zplane, int zpitch,
                                int B, int nver, int ntri, int H, int W, void* workspace, size_t ws_bytes, hipStream_t stream) {
    return launch_render_backward_impl(&pg, pg.g_depth, tri, tri_ind, zplane, zpitch, B, nver, ntri, H, W, workspace, ws_bytes,
                                       stream);
}
