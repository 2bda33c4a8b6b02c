// HBM-bound resampling kernels: layout conversion, F.interpolate modes, pooling, the two warps.
// All are one-thread-per-output-vector gathers with coalesced (row-contiguous) stores; HWC maps
// move 16 bytes (8 channels) per lane.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// layout conversion
// ------------------------------------------------------------------------------------------------
__global__ void pack_nhwc16_kernel(const float* __restrict__ src, int c, int hw, f16* __restrict__ dst, int cs) {
    const int ngroups = cs / 8;
    const size_t total = (size_t)hw * ngroups;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / ngroups;
        const int g = (int)(i - pix * ngroups);
        f16x8 v;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ch = g * 8 + k;
            v[k] = ch < c ? (f16)src[(size_t)ch * hw + pix] : (f16)0.f;
        }
        *reinterpret_cast<f16x8*>(dst + pix * cs + g * 8) = v;
    }
}

extern "C" int refvsr_pack_nhwc16(const float* src, int c, int h, int w, void* dst, int cs, void* stream) {
    RV_CHECK(src && dst && c > 0 && h > 0 && w > 0 && cs % 8 == 0 && cs >= c, "pack_nhwc16: bad args");
    const size_t total = (size_t)h * w * (cs / 8);
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(pack_nhwc16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, c, h * w, (f16*)dst, cs);
    RV_LAUNCH_CHECK();
    return 0;
}

__global__ void pack_nhwc32_kernel(const float* __restrict__ src, int c, int hw, float* __restrict__ dst, int cs) {
    const int ngroups = cs / 4;
    const size_t total = (size_t)hw * ngroups;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / ngroups;
        const int g = (int)(i - pix * ngroups);
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ch = g * 4 + k;
            v[k] = ch < c ? src[(size_t)ch * hw + pix] : 0.f;
        }
        *reinterpret_cast<f32x4*>(dst + pix * cs + g * 4) = v;
    }
}

extern "C" int refvsr_pack_nhwc32(const float* src, int c, int h, int w, float* dst, int cs, void* stream) {
    RV_CHECK(src && dst && c > 0 && h > 0 && w > 0 && cs % 4 == 0 && cs >= c, "pack_nhwc32: bad args");
    const size_t total = (size_t)h * w * (cs / 4);
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(pack_nhwc32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, c, h * w, dst, cs);
    RV_LAUNCH_CHECK();
    return 0;
}

__global__ void unpack_nhwc16_kernel(const f16* __restrict__ src, int hw, int cs, int c, float* __restrict__ dst) {
    const size_t total = (size_t)hw * c;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t ch = i / hw;
        const size_t pix = i - ch * hw;
        dst[i] = (float)src[pix * cs + ch];
    }
}

extern "C" int refvsr_unpack_nhwc16(const void* src, int h, int w, int cs, int c, float* dst, void* stream) {
    RV_CHECK(src && dst && c > 0 && h > 0 && w > 0 && cs >= c, "unpack_nhwc16: bad args");
    const size_t total = (size_t)h * w * c;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(unpack_nhwc16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f16*)src, h * w, cs, c, dst);
    RV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// F.interpolate restatement (ATen upsample_{bicubic,bilinear,nearest}2d semantics)
// ------------------------------------------------------------------------------------------------
struct ResizeArgs {
    const float* src; void* dst;
    int c, h, w, oh, ow, mode;
    float sy, sx;
    int has_norm; float mean[4], stdv[4];
    int has_mul; float mul[4];
    int clamp01, out_nhwc16, out_c;
};

// 1-D source taps for output index o: up to 4 (index, weight) pairs.
__device__ __forceinline__ int src_taps(int mode, int o, int n_in, int n_out, float scale, int* idx, float* wgt) {
    if (mode == REFVSR_RS_BICUBIC) {
        rv_cubic_src(o, n_in, scale, idx, wgt);      // common.h (shared with the confidence-fusion kernel of conv24.hip)
        return 4;
    }
    if (mode == REFVSR_RS_NEAREST) {
        idx[0] = min((int)floorf((float)o * scale), n_in - 1);
        wgt[0] = 1.0f;
        return 1;
    }
    if (mode == REFVSR_RS_BILINEAR_AC) {         // align_corners=True: common.h (shared with refvsr_warp_nhwc16_up2)
        float l1;
        rv_bilinear_ac_src(o, n_in, n_out, idx[0], idx[1], l1);
        wgt[0] = 1.0f - l1; wgt[1] = l1;
        return 2;
    }
    const float x = fmaxf(((float)o + 0.5f) * scale - 0.5f, 0.0f);
    const int i0 = min((int)x, n_in - 1);
    const int i1 = min(i0 + 1, n_in - 1);
    const float l1 = x - (float)i0;
    idx[0] = i0; idx[1] = i1;
    wgt[0] = 1.0f - l1; wgt[1] = l1;
    return 2;
}

// One thread per output pixel, all channels; MODE is a template parameter so that the tap loops (4 x 4 bicubic, 2 x 2
// bilinear, 1 nearest) are fully unrolled with the weights in registers (as a runtime-mode loop the x4 bicubic base of a
// 1080p frame took 59 us = 0.45 TB/s; the taps of neighbouring pixels are L1 / L2 hits, the kernel is instruction bound).
template <int MODE>
__global__ __launch_bounds__(256) void resize_kernel(ResizeArgs a) {
    constexpr int NT = MODE == REFVSR_RS_BICUBIC ? 4 : (MODE == REFVSR_RS_NEAREST ? 1 : 2);
    const int ox = blockIdx.x * blockDim.x + threadIdx.x;
    const int oy = blockIdx.y;
    if (ox >= a.ow) return;
    int iy[4], ix[4];
    float wy[4], wx[4];
    src_taps(MODE, oy, a.h, a.oh, a.sy, iy, wy);
    src_taps(MODE, ox, a.w, a.ow, a.sx, ix, wx);
    const size_t plane = (size_t)a.h * a.w;
    float outv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        if (ch < a.c) {
            const float* s = a.src + ch * plane;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {               // explicit FMA chains: the same arithmetic wherever this sum is restated
                float r = 0.0f;                          // (rv_bicubic_at, common.h)
                const float* row = s + (size_t)iy[j] * a.w;
#pragma unroll
                for (int i = 0; i < NT; ++i) r = fmaf(wx[i], row[ix[i]], r);
                acc = fmaf(wy[j], r, acc);
            }
            if (a.has_norm) acc = (acc - a.mean[ch & 3]) / a.stdv[ch & 3];
            if (a.has_mul) acc *= a.mul[ch & 3];
            if (a.clamp01) acc = fminf(fmaxf(acc, 0.0f), 1.0f);
            outv[ch] = acc;
            if (!a.out_nhwc16)
                reinterpret_cast<float*>(a.dst)[ch * (size_t)a.oh * a.ow + (size_t)oy * a.ow + ox] = acc;
        }
    }
    if (a.out_nhwc16) {
        f16x8 v;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = k < a.c ? (f16)outv[k] : (f16)0.f;
        f16* d = reinterpret_cast<f16*>(a.dst) + ((size_t)oy * a.ow + ox) * a.out_c;
        *reinterpret_cast<f16x8*>(d) = v;
        for (int g = 8; g < a.out_c; g += 8) *reinterpret_cast<f16x8*>(d + g) = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
}

extern "C" int refvsr_resize(const float* src, int c, int h, int w, void* dst, int oh, int ow, int mode,
                             float src_scale_y, float src_scale_x, const float* mean, const float* std,
                             const float* chan_mul, int clamp01, int out_nhwc16, int out_c, void* stream) {
    RV_CHECK(src && dst && c > 0 && c <= 8 && h > 0 && w > 0 && oh > 0 && ow > 0, "resize: bad sizes (c <= 8)");
    RV_CHECK(mode >= 0 && mode <= 3, "resize: bad mode %d", mode);
    RV_CHECK((mean == nullptr) == (std == nullptr), "resize: mean/std must come together");
    RV_CHECK(!(mean || chan_mul) || c <= 4, "resize: per-channel params support c <= 4");
    RV_CHECK(!out_nhwc16 || (c <= 8 && out_c % 8 == 0 && out_c >= 8), "resize: nhwc16 output needs c <= 8");
    ResizeArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.dst = dst; a.c = c; a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.mode = mode;
    a.sy = src_scale_y; a.sx = src_scale_x;
    if (mean) { a.has_norm = 1; for (int i = 0; i < c; ++i) { a.mean[i] = mean[i]; a.stdv[i] = std[i]; } }
    if (chan_mul) { a.has_mul = 1; for (int i = 0; i < c; ++i) a.mul[i] = chan_mul[i]; }
    a.clamp01 = clamp01; a.out_nhwc16 = out_nhwc16; a.out_c = out_c;
    const dim3 grid(rv_cdiv(ow, 256), oh), block(256);
    if (mode == REFVSR_RS_BICUBIC) hipLaunchKernelGGL(resize_kernel<REFVSR_RS_BICUBIC>, grid, block, 0, (hipStream_t)stream, a);
    else if (mode == REFVSR_RS_BILINEAR) hipLaunchKernelGGL(resize_kernel<REFVSR_RS_BILINEAR>, grid, block, 0, (hipStream_t)stream, a);
    else if (mode == REFVSR_RS_BILINEAR_AC) hipLaunchKernelGGL(resize_kernel<REFVSR_RS_BILINEAR_AC>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(resize_kernel<REFVSR_RS_NEAREST>, grid, block, 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

__global__ void pool2_kernel(const float* __restrict__ src, int c, int h, int w, float* __restrict__ dst, int is_max) {
    const int oh = h / 2, ow = w / 2;
    const size_t total = (size_t)c * oh * ow;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % ow);
        const int y = (int)((i / ow) % oh);
        const int ch = (int)(i / ((size_t)ow * oh));
        const float* s = src + ((size_t)ch * h + 2 * y) * w + 2 * x;
        const float a = s[0], b = s[1], cc = s[w], d = s[w + 1];
        dst[i] = is_max ? fmaxf(fmaxf(a, b), fmaxf(cc, d)) : 0.25f * (a + b + cc + d);
    }
}

static int launch_pool(const float* src, int c, int h, int w, float* dst, int is_max, void* stream) {
    RV_CHECK(src && dst && c > 0 && h >= 2 && w >= 2, "pool2: bad args");
    const size_t total = (size_t)c * (h / 2) * (w / 2);
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(pool2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, c, h, w, dst, is_max);
    RV_LAUNCH_CHECK();
    return 0;
}
extern "C" int refvsr_avgpool2(const float* src, int c, int h, int w, float* dst, void* stream) {
    return launch_pool(src, c, h, w, dst, 0, stream);
}
extern "C" int refvsr_maxpool2(const float* src, int c, int h, int w, float* dst, void* stream) {
    return launch_pool(src, c, h, w, dst, 1, stream);
}

__global__ void max2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        o[i] = fmaxf(a[i], b[i]);
}
extern "C" int refvsr_max2(const float* a, const float* b, float* out, size_t n, void* stream) {
    RV_CHECK(a && b && out && n > 0, "max2: bad args");
    const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(max2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
    RV_LAUNCH_CHECK();
    return 0;
}

// bit-exact equality of two float buffers -> flag (1 = equal).  Used to key the per-frame cache: frames of
// consecutive sliding windows are recognised by content, so the drop-in forward() needs no frame ids.
#define EQ_MAX_PAIRS 32
struct EqArgs { const uint4* a[EQ_MAX_PAIRS]; const uint4* b[EQ_MAX_PAIRS]; size_t n16; int* flags; };

__global__ void buffers_equal_kernel(EqArgs e) {
    const uint4* a = e.a[blockIdx.y];
    const uint4* b = e.b[blockIdx.y];
    bool diff = false;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < e.n16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 x = a[i], y = b[i];
        diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
    }
    // every writer stores the same value, so a plain store suffices (26k contended atomics cost > 100 us here)
    if (__any(diff) && (threadIdx.x & 63) == 0) e.flags[blockIdx.y] = 0;
}

extern "C" int refvsr_buffers_equal(const void* const* a, const void* const* b, int n_pairs, size_t n_bytes,
                                    int32_t* flags, void* stream) {
    RV_CHECK(a && b && flags && n_pairs > 0 && n_pairs <= EQ_MAX_PAIRS, "buffers_equal: 1..%d pairs per call", EQ_MAX_PAIRS);
    RV_CHECK(n_bytes > 0 && n_bytes % 16 == 0, "buffers_equal: size must be a multiple of 16 bytes");
    EqArgs e;
    memset(&e, 0, sizeof(e));
    for (int i = 0; i < n_pairs; ++i) {
        RV_CHECK(a[i] && b[i] && ((uintptr_t)a[i] % 16 == 0) && ((uintptr_t)b[i] % 16 == 0), "buffers_equal: unaligned buffer");
        e.a[i] = (const uint4*)a[i];
        e.b[i] = (const uint4*)b[i];
    }
    e.n16 = n_bytes / 16;
    e.flags = flags;
    const int gx = (int)((e.n16 + 255) / 256 > 256 ? 256 : (e.n16 + 255) / 256);
    hipLaunchKernelGGL(buffers_equal_kernel, dim3(gx, n_pairs), dim3(256), 0, (hipStream_t)stream, e);
    RV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// warp (models/utils.py:35-43): zeros padding, align_corners=False sampling of a linspace(-1,1) grid
// ------------------------------------------------------------------------------------------------
// Up to REFVSR_MAX_MAPS (map, flow) pairs of one geometry per launch (blockIdx.z = pair; ABI 11: the propagation chains of consecutive
// output frames warp their states in one launch per layer).  The single-pair entry points are the batch = 1 case of the same kernels.
struct WarpArgs {
    const void* x[REFVSR_MAX_MAPS]; const float* flow[REFVSR_MAX_MAPS]; void* out[REFVSR_MAX_MAPS];
    int c, hin, win, cs, hf, wf;         // c: planar channels (warp_planar); cs: channel stride (nhwc16); hf x wf: the flow map (up2: hl x wl)
};
static_assert(REFVSR_MAX_MAPS == 4, "WARP_SEL selects among exactly four table entries");
#define WARP_SEL(tbl, bi) ((bi) == 0 ? (tbl)[0] : (bi) == 1 ? (tbl)[1] : (bi) == 2 ? (tbl)[2] : (tbl)[3])

__global__ void warp_nhwc16_kernel(WarpArgs a) {
    const int bi = blockIdx.z;
    const f16* __restrict__ x = (const f16*)WARP_SEL(a.x, bi);
    const float* __restrict__ flow = WARP_SEL(a.flow, bi);
    f16* __restrict__ out = (f16*)WARP_SEL(a.out, bi);
    const int hin = a.hin, win = a.win, cs = a.cs, hf = a.hf, wf = a.wf;
    const int ng = cs / 8;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (pixel-in-row, group)
    const int y = blockIdx.y;
    if (i >= wf * ng) return;
    const int px = i / ng;
    const int g = i - px * ng;
    const WarpCoord c = warp_coord(flow, hf, wf, hin, win, y, px);
    *reinterpret_cast<uint4*>(out + ((size_t)y * wf + px) * cs + g * 8) =
        warp_group16(reinterpret_cast<const unsigned char*>(x), cs * 2, hin, win, c, g * 16);
}

static int warp_fill(WarpArgs& a, const char* who, const void* const* x, const float* const* flow, void* const* out, int batch) {
    RV_CHECK(x && flow && out && batch >= 1 && batch <= REFVSR_MAX_MAPS, "%s: 1..%d (map, flow) pairs per launch", who, REFVSR_MAX_MAPS);
    memset(&a, 0, sizeof(a));
    for (int b = 0; b < batch; ++b) {
        RV_CHECK(x[b] && flow[b] && out[b], "%s: null pointer (pair %d)", who, b);
        a.x[b] = x[b]; a.flow[b] = flow[b]; a.out[b] = out[b];
    }
    return 0;
}

extern "C" int refvsr_warp_nhwc16_batch(const void* const* x, int batch, int hin, int win, int cs, const float* const* flow, int hf, int wf,
                                        void* const* out, void* stream) {
    RV_CHECK(hin > 1 && win > 1 && hf > 1 && wf > 1 && cs % 8 == 0 && cs > 0, "warp_nhwc16: bad args");
    WarpArgs a;
    if (warp_fill(a, "warp_nhwc16", x, flow, out, batch)) return 1;
    a.hin = hin; a.win = win; a.cs = cs; a.hf = hf; a.wf = wf;
    const int ng = cs / 8;
    hipLaunchKernelGGL(warp_nhwc16_kernel, dim3(rv_cdiv(wf * ng, 256), hf, batch), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_warp_nhwc16(const void* x, int hin, int win, int cs, const float* flow, int hf, int wf,
                                  void* out, void* stream) {
    RV_CHECK(x && flow && out, "warp_nhwc16: bad args");
    return refvsr_warp_nhwc16_batch(&x, 1, hin, win, cs, &flow, hf, wf, &out, stream);
}

// warp(x, flow_up2(flow_lr)) without the 2x flow map: the flow of grid pixel (y, px) is F.interpolate(flow_lr, x2, bilinear,
// align_corners=True) * 2 evaluated in place (RefVSR.py:220,254,259: the 2x state is warped by the up-sampled LR flow) --
// the arithmetic of refvsr_resize(BILINEAR_AC, chan_mul = 2) followed by refvsr_warp_nhwc16, bit for bit
__global__ void warp_nhwc16_up2_kernel(WarpArgs a) {
    const int bi = blockIdx.z;
    const f16* __restrict__ x = (const f16*)WARP_SEL(a.x, bi);
    const float* __restrict__ flow_lr = WARP_SEL(a.flow, bi);
    f16* __restrict__ out = (f16*)WARP_SEL(a.out, bi);
    const int hin = a.hin, win = a.win, cs = a.cs, hl = a.hf, wl = a.wf;
    const int ng = cs / 8;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int hf = 2 * hl, wf = 2 * wl;
    if (i >= wf * ng) return;
    const int px = i / ng;
    const int g = i - px * ng;
    float u = rv_bilinear_ac2_at(flow_lr, hl, wl, y, px) * 2.0f;
    float v = rv_bilinear_ac2_at(flow_lr + (size_t)hl * wl, hl, wl, y, px) * 2.0f;
    asm volatile("" : "+v"(u), "+v"(v));             // the values a flow map would hold: nothing downstream may fuse with their making
    const WarpCoord c = warp_coord_uv(u, v, hf, wf, hin, win, y, px);
    *reinterpret_cast<uint4*>(out + ((size_t)y * wf + px) * cs + g * 8) =
        warp_group16(reinterpret_cast<const unsigned char*>(x), cs * 2, hin, win, c, g * 16);
}

extern "C" int refvsr_warp_nhwc16_up2_batch(const void* const* x, int batch, int hin, int win, int cs, const float* const* flow_lr, int hl,
                                            int wl, void* const* out, void* stream) {
    RV_CHECK(hin > 1 && win > 1 && hl > 0 && wl > 0 && cs % 8 == 0 && cs > 0, "warp_nhwc16_up2: bad args");
    WarpArgs a;
    if (warp_fill(a, "warp_nhwc16_up2", x, flow_lr, out, batch)) return 1;
    a.hin = hin; a.win = win; a.cs = cs; a.hf = hl; a.wf = wl;
    const int ng = cs / 8;
    hipLaunchKernelGGL(warp_nhwc16_up2_kernel, dim3(rv_cdiv(2 * wl * ng, 256), 2 * hl, batch), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_warp_nhwc16_up2(const void* x, int hin, int win, int cs, const float* flow_lr, int hl, int wl,
                                      void* out, void* stream) {
    RV_CHECK(x && flow_lr && out, "warp_nhwc16_up2: bad args");
    return refvsr_warp_nhwc16_up2_batch(&x, 1, hin, win, cs, &flow_lr, hl, wl, &out, stream);
}

__global__ void warp_planar_kernel(WarpArgs a) {
    const int bi = blockIdx.z;
    const float* __restrict__ x = (const float*)WARP_SEL(a.x, bi);
    const float* __restrict__ flow = WARP_SEL(a.flow, bi);
    float* __restrict__ out = (float*)WARP_SEL(a.out, bi);
    const int c = a.c, hin = a.hin, win = a.win, hf = a.hf, wf = a.wf;
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (px >= wf) return;
    const WarpCoord k = warp_coord(flow, hf, wf, hin, win, y, px);
    for (int ch = 0; ch < c; ++ch) {
        const float* s = x + (size_t)ch * hin * win;
        float acc = 0.0f;
        if (k.v00) acc += k.w00 * s[(size_t)k.y0 * win + k.x0];
        if (k.v01) acc += k.w01 * s[(size_t)k.y0 * win + k.x0 + 1];
        if (k.v10) acc += k.w10 * s[(size_t)(k.y0 + 1) * win + k.x0];
        if (k.v11) acc += k.w11 * s[(size_t)(k.y0 + 1) * win + k.x0 + 1];
        out[((size_t)ch * hf + y) * wf + px] = acc;
    }
}

extern "C" int refvsr_warp_planar_batch(const float* const* x, int batch, int c, int hin, int win, const float* const* flow, int hf, int wf,
                                        float* const* out, void* stream) {
    RV_CHECK(c > 0 && hin > 1 && win > 1 && hf > 1 && wf > 1, "warp_planar: bad args");
    WarpArgs a;
    if (warp_fill(a, "warp_planar", (const void* const*)x, flow, (void* const*)out, batch)) return 1;
    a.c = c; a.hin = hin; a.win = win; a.hf = hf; a.wf = wf;
    hipLaunchKernelGGL(warp_planar_kernel, dim3(rv_cdiv(wf, 128), hf, batch), dim3(128), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_warp_planar(const float* x, int c, int hin, int win, const float* flow, int hf, int wf,
                                  float* out, void* stream) {
    RV_CHECK(x && flow && out, "warp_planar: bad args");
    return refvsr_warp_planar_batch(&x, 1, c, hin, win, &flow, hf, wf, &out, stream);
}

// ------------------------------------------------------------------------------------------------
// SPyNet level input: x2 align_corners flow upsample (*2) + border-clamped flow_warp + concat
// ------------------------------------------------------------------------------------------------
#define SPY_MAX_PAIRS 8
struct SpyLevelArgs {                   // up to 8 independent (ref, supp) pairs of one pyramid level per launch (blockIdx.z)
    const float* ref[SPY_MAX_PAIRS]; const float* supp[SPY_MAX_PAIRS];
    const float* flow_prev;             // [batch][2][h/2][w/2] or NULL
    f16* out8; float* flow_up;          // [batch][h][w][8], [batch][2][h][w]
    int h, w;
};

__global__ void spynet_level_input_kernel(SpyLevelArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int h = a.h, w = a.w;
    if (x >= w) return;
    const int bi = blockIdx.z;
#define SPY_SEL(t) (bi == 0 ? (t)[0] : bi == 1 ? (t)[1] : bi == 2 ? (t)[2] : bi == 3 ? (t)[3] : bi == 4 ? (t)[4] : bi == 5 ? (t)[5] : bi == 6 ? (t)[6] : (t)[7])
    const float* __restrict__ ref = SPY_SEL(a.ref);
    const float* __restrict__ supp = SPY_SEL(a.supp);
#undef SPY_SEL
    const float* __restrict__ flow_prev = a.flow_prev ? a.flow_prev + (size_t)bi * 2 * (h / 2) * (w / 2) : nullptr;
    f16* __restrict__ out8 = a.out8 + (size_t)bi * h * w * 8;
    float* __restrict__ flow_up = a.flow_up + (size_t)bi * 2 * h * w;
    const size_t plane = (size_t)h * w;
    const size_t pix = (size_t)y * w + x;
    float u = 0.0f, v = 0.0f;
    if (flow_prev) {
        const int hp = h / 2, wp = w / 2;
        int iy[2], ix[2];
        float wy[2], wx[2];
        src_taps(REFVSR_RS_BILINEAR_AC, y, hp, h, 0.f, iy, wy);
        src_taps(REFVSR_RS_BILINEAR_AC, x, wp, w, 0.f, ix, wx);
        const float* f0 = flow_prev;
        const float* f1 = flow_prev + (size_t)hp * wp;
        u = wy[0] * (wx[0] * f0[(size_t)iy[0] * wp + ix[0]] + wx[1] * f0[(size_t)iy[0] * wp + ix[1]]) +
            wy[1] * (wx[0] * f0[(size_t)iy[1] * wp + ix[0]] + wx[1] * f0[(size_t)iy[1] * wp + ix[1]]);
        v = wy[0] * (wx[0] * f1[(size_t)iy[0] * wp + ix[0]] + wx[1] * f1[(size_t)iy[0] * wp + ix[1]]) +
            wy[1] * (wx[0] * f1[(size_t)iy[1] * wp + ix[0]] + wx[1] * f1[(size_t)iy[1] * wp + ix[1]]);
        u *= 2.0f;
        v *= 2.0f;
    }
    flow_up[pix] = u;
    flow_up[plane + pix] = v;
    // flow_warp (mmedit flow_warp.py:36-46): normalise with align_corners=True, border padding
    const float gx = 2.0f * ((float)x + u) / (float)max(w - 1, 1) - 1.0f;
    const float gy = 2.0f * ((float)y + v) / (float)max(h - 1, 1) - 1.0f;
    float xs = (gx + 1.0f) / 2.0f * (float)(w - 1);
    float ys = (gy + 1.0f) / 2.0f * (float)(h - 1);
    xs = fminf(fmaxf(xs, 0.0f), (float)(w - 1));
    ys = fminf(fmaxf(ys, 0.0f), (float)(h - 1));
    const int x0 = (int)floorf(xs), y0 = (int)floorf(ys);
    const float tx = xs - (float)x0, ty = ys - (float)y0;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    f16x8 o;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        o[ch] = (f16)ref[ch * plane + pix];
        const float* s = supp + ch * plane;
        const float val = (1.0f - ty) * ((1.0f - tx) * s[(size_t)y0 * w + x0] + tx * s[(size_t)y0 * w + x1]) +
                          ty * ((1.0f - tx) * s[(size_t)y1 * w + x0] + tx * s[(size_t)y1 * w + x1]);
        o[3 + ch] = (f16)val;
    }
    o[6] = (f16)u;
    o[7] = (f16)v;
    *reinterpret_cast<f16x8*>(out8 + pix * 8) = o;
}

extern "C" int refvsr_spynet_level_input_batch(const float* const* ref, const float* const* supp, int batch, const float* flow_prev,
                                               int h, int w, void* out8, float* flow_up, void* stream) {
    RV_CHECK(ref && supp && out8 && flow_up && h > 0 && w > 0 && batch >= 1 && batch <= SPY_MAX_PAIRS, "spynet_level_input: bad args");
    RV_CHECK(flow_prev == nullptr || (h % 2 == 0 && w % 2 == 0), "spynet_level_input: odd level size");
    SpyLevelArgs a;
    memset(&a, 0, sizeof(a));
    for (int b = 0; b < batch; ++b) {
        RV_CHECK(ref[b] && supp[b], "spynet_level_input: null frame pointer (pair %d)", b);
        a.ref[b] = ref[b]; a.supp[b] = supp[b];
    }
    a.flow_prev = flow_prev; a.out8 = (f16*)out8; a.flow_up = flow_up; a.h = h; a.w = w;
    hipLaunchKernelGGL(spynet_level_input_kernel, dim3(rv_cdiv(w, 128), h, batch), dim3(128), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_spynet_level_input(const float* ref, const float* supp, const float* flow_prev, int h, int w,
                                         void* out8, float* flow_up, void* stream) {
    RV_CHECK(ref && supp, "spynet_level_input: bad args");
    return refvsr_spynet_level_input_batch(&ref, &supp, 1, flow_prev, h, w, out8, flow_up, stream);
}

// ------------------------------------------------------------------------------------------------
// fp32 result -> fp16 | uint8 (REFVSR_RESULT_*, ABI 14): the conversion of the fused output heads (rv_store_result) for results that
// come out of the generic head
// ------------------------------------------------------------------------------------------------
__global__ void convert_result_kernel(const float* __restrict__ src, size_t n, int fmt, void* __restrict__ out) {
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(src + i0);
        const float c[4] = {fminf(fmaxf(v.x, 0.f), 1.f), fminf(fmaxf(v.y, 0.f), 1.f), fminf(fmaxf(v.z, 0.f), 1.f), fminf(fmaxf(v.w, 0.f), 1.f)};
        if (fmt == REFVSR_RESULT_F16) {
            union { f16 h[4]; uint2 u; } o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.h[k] = (f16)c[k];
            *reinterpret_cast<uint2*>(reinterpret_cast<f16*>(out) + i0) = o.u;
        } else {
            union { unsigned char b[4]; unsigned u; } o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.b[k] = (unsigned char)__float2int_rn(c[k] * 255.0f);
            *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(out) + i0) = o.u;
        }
    } else {
        for (size_t i = i0; i < n; ++i) rv_store_result(out, i, fminf(fmaxf(src[i], 0.f), 1.f), fmt);
    }
}

extern "C" int refvsr_convert_result(const float* src, size_t n, int out_fmt, void* out, void* stream) {
    RV_CHECK(src && out && n > 0, "convert_result: bad args");
    RV_CHECK(out_fmt == REFVSR_RESULT_F16 || out_fmt == REFVSR_RESULT_U8, "convert_result: format must be REFVSR_RESULT_F16 | REFVSR_RESULT_U8");
    RV_CHECK(((uintptr_t)src & 15) == 0 && ((uintptr_t)out & 7) == 0, "convert_result: src must be 16-byte, out 8-byte aligned");
    const size_t nq = (n + 3) / 4;
    hipLaunchKernelGGL(convert_result_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n, out_fmt, out);
    RV_LAUNCH_CHECK();
    return 0;
}

// ... into the interleaved layout (REFVSR_RESULT_HWC; extension, no ABI bump): planar fp32 [3][h][w] -> [h][w][3] fp32 | fp16 | uint8 with
// the same clamp and rounding (rv_store_result).  One thread per pixel: a wave reads 64 consecutive floats of each plane (three
// coalesced 256-byte reads) and writes the 192 consecutive elements of its 64 pixels, three per lane.  Element stores only: `out`
// needs the natural alignment of its samples, for any w.
__global__ void __launch_bounds__(256) convert_result_hwc_kernel(const float* __restrict__ src, int npix, int fmt, void* __restrict__ out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= npix) return;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        rv_store_result(out, (size_t)i * 3 + c, fminf(fmaxf(src[(size_t)c * npix + i], 0.f), 1.f), fmt);
}

extern "C" int refvsr_convert_result_hwc(const float* src, int h, int w, int out_fmt, void* out, void* stream) {
    RV_CHECK(src && out && h > 0 && w > 0 && (const void*)src != out, "convert_result_hwc: bad args");
    RV_CHECK(rv_result_fmt_ok(out_fmt), "convert_result_hwc: unknown result format %d", out_fmt);
    RV_CHECK((long long)h * w * 3 < (1ll << 31), "convert_result_hwc: frame too large (3 h w must stay below 2^31)");
    const int f = out_fmt & REFVSR_RESULT_FMT_MASK;
    RV_CHECK(((uintptr_t)src & 3) == 0 && ((uintptr_t)out & (f == REFVSR_RESULT_F32 ? 3 : f == REFVSR_RESULT_F16 ? 1 : 0)) == 0,
             "convert_result_hwc: src must be 4-byte aligned, out aligned to its samples");
    const int npix = h * w;
    hipLaunchKernelGGL(convert_result_hwc_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, npix, out_fmt, out);
    RV_LAUNCH_CHECK();
    return 0;
}
