// Confidence maps as images on the device: up to REFVSR_COLORMAP_MAX_MAPS fp32 [h][w] maps of one geometry are min/max-normalised and
// coloured with matplotlib's `inferno` table in one entry point (two launches), so that an evaluation loop moves 3 bytes per pixel to
// the host instead of the map.  Replaces evaluation/eval_quan_conf_map.py:64-100 (x - x.min(), / x.max(), colormap(x)[:, :, :3]) and
// :126,148-165 (x * 255 through cv2.imwrite's rounding cast), which the reference runs on the host on a map it first copies there.
//
// Definition, all fp32, per map (finite inputs):  lo = min x;  a = x - lo;  span = max a (= fl(max x - lo): rounding is monotonic);
// y = a / span, the correctly rounded quotient;  idx = min((int)(y * 256), 255) (matplotlib: xa *= N, xa[xa == N] = N - 1, truncate);
// out = u8[idx], the table of colormap_table.h.  A constant map has span = 0 and y = 0 / 0 = NaN: matplotlib paints its "bad" colour
// (0, 0, 0, 0) there, three zero bytes.  0 <= y <= 1 otherwise, so the under / over colours never occur.
// The file is built without any fast-math flag: `/` is the IEEE quotient (hipcc's default), subnormals are kept, and contraction is
// off, so the three operations are the written ones.  refvsr_amd/metrics.py:conf_colormap_model restates them in numpy.
//
// Pass 1, colormap_minmax_kernel: grid (blocks per map, n) x 256 threads.  Floats of a map up to its first 16-byte boundary (head) and
// past its last whole float4 (tail) are read as scalars by the first threads of block 0, everything between as one 16-byte load per
// lane, consecutive lanes on consecutive float4s, grid-strided.  {min, max} per thread -> __shfl_down tree per wave -> four waves
// through LDS -> two floats per block to the workspace with a plain vector store.
// Pass 2, colormap_paint_kernel: grid (blocks per map, n) x 256 threads.  Every workgroup folds its map's <= CM_MAX_PART partial pairs
// itself (wave 0, the same tree) and holds the table in LDS as 256 packed dwords (R | G << 8 | B << 16).  A lane colours four
// consecutive pixels: one 16-byte load where the map's base allows it (four dword loads otherwise), four table reads, 12 bytes = three
// dword stores where the image's base is 4-byte aligned (byte stores otherwise); the last h w % 4 pixels go out as byte stores.
// min and max are exact and order-independent and a pixel is a function of (x, lo, span) alone: a map's bytes do not depend on the
// other maps of the launch, on the stream or on the run.  No atomics, no inline assembly.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the figures next to the kernels.
#include "common.h"
#include "colormap_table.h"

#pragma clang fp contract(off)

#define CM_THREADS 256
#define CM_MAX_PART 64                 // partial {min, max} pairs per map (= blocks per map of pass 1, at most)
#define CM_VEC_PER_BLOCK 1024          // float4s per block of pass 1 before the grid stride starts (four loads in flight per lane)
#define CM_MAX_PAINT_BLOCKS 1024       // blocks per map of pass 2, at most

struct ColormapPacked { uint32_t v[256]; };
static constexpr ColormapPacked colormap_packed() {
    ColormapPacked p{};
    const ColormapTable t = colormap_table();
    for (int i = 0; i < 256; ++i) p.v[i] = (uint32_t)t.v[i][0] | ((uint32_t)t.v[i][1] << 8) | ((uint32_t)t.v[i][2] << 16);
    return p;
}
__constant__ ColormapPacked kColormap = colormap_packed();
static const ColormapTable kColormapHost = colormap_table();

struct ColormapArgs {
    const float* map[REFVSR_COLORMAP_MAX_MAPS];
    unsigned char* rgb[REFVSR_COLORMAP_MAX_MAPS];
    float* part;                       // [n][nblk][2] partial {min, max}
    int npx;                           // h * w < 2^31
    int nblk;                          // blocks per map of pass 1, 1 .. CM_MAX_PART
};

static inline int cm_blocks(long npx) {                       // pass 1: blocks per map
    const long want = (npx / 4 + CM_VEC_PER_BLOCK - 1) / CM_VEC_PER_BLOCK;
    return (int)(want < 1 ? 1 : want > CM_MAX_PART ? CM_MAX_PART : want);
}

// {min, max} over the 64 lanes of a wave; the result is valid in lane 0
__device__ __forceinline__ void cm_wave_minmax(float& lo, float& hi) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo = fminf(lo, __shfl_down(lo, s, 64));
        hi = fmaxf(hi, __shfl_down(hi, s, 64));
    }
}

// colormap_minmax_kernel: 12 VGPRs, 22 SGPRs, no scratch, 32 B LDS (figures of the build this file was written against)
__global__ void __launch_bounds__(CM_THREADS) colormap_minmax_kernel(ColormapArgs s) {
    __shared__ float red[2][CM_THREADS / 64];
    const int tid = (int)threadIdx.x, m = (int)blockIdx.y;
    const float* __restrict__ x = s.map[m];
    const int npx = s.npx;
    // floats before the first 16-byte boundary (the base is 4-byte aligned), whole float4s, floats after them
    int head = (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
    head = head < npx ? head : npx;
    const int nvec = (npx - head) >> 2;
    const int tail0 = head + 4 * nvec;                        // tail: [tail0, npx), at most 3 floats
    float lo = INFINITY, hi = -INFINITY;
    if (blockIdx.x == 0) {
        if (tid < head) {
            const float v = x[tid];
            lo = v; hi = v;
        }
        if (tid >= 64 && (long)tail0 + (tid - 64) < npx) {    // (wave 1: the head's lanes stay on one path)
            const float v = x[(long)tail0 + (tid - 64)];
            lo = fminf(lo, v); hi = fmaxf(hi, v);
        }
    }
    const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
    for (int i = (int)blockIdx.x * CM_THREADS + tid; i < nvec; i += (int)gridDim.x * CM_THREADS) {
        const float4 v = xv[i];
        lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    cm_wave_minmax(lo, hi);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = lo;
        red[1][tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
        lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        *reinterpret_cast<float2*>(s.part + 2 * ((size_t)m * s.nblk + blockIdx.x)) = make_float2(lo, hi);
    }
}

// the colour of one sample, packed R | G << 8 | B << 16; 0 where y is NaN (span = 0)
__device__ __forceinline__ uint32_t cm_colour(const uint32_t* tbl, const float x, const float lo, const float span) {
    const float y = (x - lo) / span;
    const int idx = (int)fminf(y * 256.0f, 255.0f);           // (fminf drops a NaN operand: the conversion is always defined)
    return y == y ? tbl[idx & 255] : 0u;
}

// colormap_paint_kernel: 23 VGPRs, 30 SGPRs, no scratch, 1 032 B LDS; the quotient is the v_div_scale / v_div_fmas / v_div_fixup
// sequence with fp32 denormals on (figures of the build this file was written against)
__global__ void __launch_bounds__(CM_THREADS) colormap_paint_kernel(ColormapArgs s) {
    __shared__ uint32_t tbl[256];
    __shared__ float mm[2];
    const int tid = (int)threadIdx.x, m = (int)blockIdx.y;
    tbl[tid] = kColormap.v[tid];
    if (tid < 64) {                                           // wave 0 folds the map's partial pairs (nblk <= 64)
        float lo = INFINITY, hi = -INFINITY;
        if (tid < s.nblk) {
            const float2 p = *reinterpret_cast<const float2*>(s.part + 2 * ((size_t)m * s.nblk + tid));
            lo = p.x; hi = p.y;
        }
        cm_wave_minmax(lo, hi);
        if (tid == 0) {
            mm[0] = lo;
            mm[1] = hi;
        }
    }
    __syncthreads();
    const float lo = mm[0];
    const float span = mm[1] - lo;                            // = max (x - lo): x -> fl(x - lo) is monotonic
    const float* __restrict__ x = s.map[m];
    unsigned char* __restrict__ out = s.rgb[m];
    const int npx = s.npx, ngrp = npx >> 2;
    const bool in16 = ((uintptr_t)x & 15u) == 0, out4 = ((uintptr_t)out & 3u) == 0;      // (workgroup-uniform)
    for (int g = (int)blockIdx.x * CM_THREADS + tid; g < ngrp; g += (int)gridDim.x * CM_THREADS) {
        float4 v;
        if (in16) {
            v = reinterpret_cast<const float4*>(x)[g];
        } else {
            const float* q = x + 4 * (size_t)g;
            v = make_float4(q[0], q[1], q[2], q[3]);
        }
        const uint32_t c0 = cm_colour(tbl, v.x, lo, span), c1 = cm_colour(tbl, v.y, lo, span);
        const uint32_t c2 = cm_colour(tbl, v.z, lo, span), c3 = cm_colour(tbl, v.w, lo, span);
        // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        const uint32_t d0 = c0 | (c1 << 24), d1 = (c1 >> 8) | (c2 << 16), d2 = (c2 >> 16) | (c3 << 8);
        unsigned char* o = out + 12 * (size_t)g;
        if (out4) {
            uint32_t* od = reinterpret_cast<uint32_t*>(o);
            od[0] = d0; od[1] = d1; od[2] = d2;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = (unsigned char)(d0 >> (8 * k));
                o[4 + k] = (unsigned char)(d1 >> (8 * k));
                o[8 + k] = (unsigned char)(d2 >> (8 * k));
            }
        }
    }
    if (blockIdx.x == 0 && 4 * (long)ngrp + tid < npx) {      // the last npx % 4 pixels
        const long i = 4 * (long)ngrp + tid;
        const uint32_t c = cm_colour(tbl, x[i], lo, span);
        unsigned char* o = out + 3 * (size_t)i;
        o[0] = (unsigned char)c;
        o[1] = (unsigned char)(c >> 8);
        o[2] = (unsigned char)(c >> 16);
    }
}

static bool cm_args_ok(int n, int h, int w) {
    return n >= 1 && n <= REFVSR_COLORMAP_MAX_MAPS && h >= 1 && w >= 1 && (long long)h * w < (1ll << 31);
}

extern "C" int refvsr_colormap_table(unsigned char* out768) {
    RV_CHECK(out768, "colormap_table: null output");
    memcpy(out768, kColormapHost.v, 768);
    return 0;
}

extern "C" size_t refvsr_conf_colormap_workspace_bytes(int n, int h, int w) {
    if (!cm_args_ok(n, h, w)) return 0;
    return (size_t)n * cm_blocks((long)h * w) * 2 * sizeof(float);
}

extern "C" int refvsr_conf_colormap(const void* const* maps, int n, int h, int w, void* const* rgb, void* ws, size_t ws_bytes,
                                    void* stream) {
    RV_CHECK(maps && rgb, "conf_colormap: null map / image table");
    RV_CHECK(n >= 1 && n <= REFVSR_COLORMAP_MAX_MAPS, "conf_colormap: 1..%d maps per launch (got %d)", REFVSR_COLORMAP_MAX_MAPS, n);
    RV_CHECK(h >= 1 && w >= 1, "conf_colormap: h, w must be at least 1 (got %d x %d)", h, w);
    RV_CHECK((long long)h * w < (1ll << 31), "conf_colormap: h * w must be below 2^31 (got %d x %d)", h, w);
    RV_CHECK(ws, "conf_colormap: null workspace");
    RV_CHECK(((uintptr_t)ws & 7) == 0, "conf_colormap: workspace must be 8-byte aligned");
    RV_CHECK(ws_bytes >= refvsr_conf_colormap_workspace_bytes(n, h, w), "conf_colormap: workspace too small (%zu bytes, %zu needed)",
             ws_bytes, refvsr_conf_colormap_workspace_bytes(n, h, w));
    ColormapArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; ++i) {
        RV_CHECK(maps[i] && rgb[i], "conf_colormap: null pointer (map %d)", i);
        RV_CHECK(((uintptr_t)maps[i] & 3) == 0, "conf_colormap: maps must be 4-byte aligned (map %d)", i);
        a.map[i] = (const float*)maps[i];
        a.rgb[i] = (unsigned char*)rgb[i];
    }
    a.part = (float*)ws;
    a.npx = h * w;
    a.nblk = cm_blocks(a.npx);
    hipLaunchKernelGGL(colormap_minmax_kernel, dim3(a.nblk, n), dim3(CM_THREADS), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    const long want = ((long)(a.npx >> 2) + CM_THREADS - 1) / CM_THREADS;
    const int gx = (int)(want < 1 ? 1 : want > CM_MAX_PAINT_BLOCKS ? CM_MAX_PAINT_BLOCKS : want);
    hipLaunchKernelGGL(colormap_paint_kernel, dim3(gx, n), dim3(CM_THREADS), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}
