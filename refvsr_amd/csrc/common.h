// Shared helpers for the gfx950 RefVSR kernels.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include <utility>

#include "../../include/refvsr_hip.h"
#include "plan_common.h"

typedef _Float16 f16;
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define RV_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            refvsr_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

#define RV_LAUNCH_CHECK() RV_HIP(hipGetLastError())

// f(std::integral_constant<int, I>{}) for every I of the sequence, in order: a loop whose index is a compile-time constant
template <class F, int... I>
__device__ __forceinline__ void rv_static_for(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }

// Per-device caches (function attributes, occupancy, CU count): one process may drive several GPUs.
#define RV_MAX_DEVICES 16
static inline int rv_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= RV_MAX_DEVICES) d = 0;
    return d;
}
static inline int rv_num_cus() {
    static int n_cu[RV_MAX_DEVICES] = {};
    const int d = rv_device();
    if (n_cu[d] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess) n_cu[d] = prop.multiProcessorCount;
        if (n_cu[d] <= 0) n_cu[d] = 256;
    }
    return n_cu[d];
}

// CUs the persistent launchers may count on for a launch on `st`: the budget registered for a CU-masked stream
// (refvsr_stream_create_cu_range / refvsr_stream_set_cu_budget, runtime.hip), otherwise the whole device.
int rv_stream_cus(hipStream_t st);

// Grid cap of a persistent launcher on `st`, with the launcher's per-device one-time set-up (a process may drive several GPUs): the
// kernel's dynamic-LDS attribute (attr_lds bytes) and its occupancy with `lds` bytes (block = 0: one workgroup per CU by
// construction, nothing is asked).  *cap = CUs of the stream x occupancy / div, a multiple of 8 (XCDs), at least 8; div = the
// grid's extent in y and z.  cap = nullptr: the attribute alone (one workgroup per tile, no cap to compute).
// The occupancies of the last four LDS sizes are kept: the generic conv launches one instantiation with several carves in turn, and
// the runtime's occupancy query sits on the launch path.
// One RvLaunchCap per kernel instantiation (a function-local static of its launcher).
struct RvLaunchCap {
    bool attr_done[RV_MAX_DEVICES];
    int occ[RV_MAX_DEVICES][4];                    // 0 = empty entry
    size_t occ_lds[RV_MAX_DEVICES][4];
    int next[RV_MAX_DEVICES];                      // entries are replaced in turn
};
template <typename Kernel>
static int rv_launch_cap(RvLaunchCap& c, Kernel kernel, int block, size_t attr_lds, size_t lds, hipStream_t st, int* cap, int div = 1) {
    const int dev = rv_device();
    if (!c.attr_done[dev]) {
        RV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_lds));
        c.attr_done[dev] = true;
    }
    if (!cap) return 0;
    int occ = block == 0 ? 1 : 0;
    for (int i = 0; i < 4 && !occ; ++i)
        if (c.occ_lds[dev][i] == lds) occ = c.occ[dev][i];
    if (!occ) {
        RV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, block, lds));
        if (occ < 1) occ = 1;
        const int i = c.next[dev]++ & 3;
        c.occ_lds[dev][i] = lds;
        c.occ[dev][i] = occ;
    }
    *cap = (rv_stream_cus(st) * occ / div) & ~7;
    if (*cap < 8) *cap = 8;
    return 0;
}

// Host driver of a chain of fused blocks (resblock24.hip, resblock48.hip): n blocks x <- x + conv2(act(conv1 x)) on `batch` fp16 HWC
// maps of one geometry, pxb bytes per pixel (batch = 1: the plain chain); block i's parameters are the blob at blobs + i * blob_stride
// (>= min_blob bytes).  n launches on the caller's stream, each over ALL maps: launch(a, st) with a.bsrc / a.bout / a.src / a.out /
// a.blob of block i; intermediates ping-pong between scratch0 / scratch1 ([batch] maps each, contiguous; blocks cannot run in
// place: neighbouring tiles read the input halo).  name: the entry point, as the error messages call it.
template <typename Args, typename Launch>
static int rv_resblock_chain(const char* name, int pxb, int min_blob, const void* const* src, int batch, int h, int w, int n,
                             const void* blobs, size_t blob_stride, float act_slope, void* scratch0, void* scratch1, void* const* out,
                             void* stream, Launch launch) {
    RV_CHECK(src && out && blobs && h > 0 && w > 0 && n >= 1 && batch >= 1 && batch <= REFVSR_MAX_MAPS, "%s: bad args", name);
    RV_CHECK(blob_stride >= (size_t)min_blob && blob_stride % 16 == 0 && ((uintptr_t)blobs & 15) == 0,
             "%s: blobs must be 16-byte aligned, stride >= %d", name, min_blob);
    RV_CHECK(act_slope >= 0.f && act_slope <= 1.f, "%s: activation slope must lie in [0, 1]", name);
    RV_CHECK(n == 1 || scratch0, "%s: n >= 2 needs scratch0", name);
    RV_CHECK(n <= 2 || scratch1, "%s: n >= 3 needs scratch1", name);
    const size_t mapb = (size_t)h * w * pxb;
    for (int b = 0; b < batch; ++b) {
        RV_CHECK(src[b] && out[b], "%s: null map pointer (map %d)", name, b);
        for (int c = 0; c < batch; ++c) {
            const unsigned char* s0 = scratch0 ? (const unsigned char*)scratch0 + c * mapb : nullptr;
            const unsigned char* s1 = scratch1 ? (const unsigned char*)scratch1 + c * mapb : nullptr;
            RV_CHECK(src[b] != out[c] && s0 != out[b] && s1 != out[b] && (n < 2 || s0 != src[b]) && (n < 3 || s1 != src[b]) &&
                     (c == b || out[b] != out[c]), "%s: buffers must be distinct", name);
        }
    }
    RV_CHECK(n < 3 || scratch0 != scratch1, "%s: buffers must be distinct", name);
    RV_CHECK((long long)h * w * pxb < (1ll << 31), "%s: map too large for 32-bit offsets", name);
    RV_CHECK(refvsr_init() == 0, "init failed");
    Args a;
    memset(&a, 0, sizeof(a));
    a.h = h; a.w = w; a.act_slope = act_slope; a.batch = batch;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* cur[REFVSR_MAX_MAPS];
    for (int b = 0; b < batch; ++b) cur[b] = (const unsigned char*)src[b];
    for (int i = 0; i < n; ++i) {
        unsigned char* sc = (unsigned char*)((i & 1) ? scratch1 : scratch0);
        for (int b = 0; b < batch; ++b) {
            a.bsrc[b] = cur[b];
            a.bout[b] = (i == n - 1) ? (unsigned char*)out[b] : sc + b * mapb;
        }
        a.src = a.bsrc[0]; a.out = a.bout[0]; a.blob = (const unsigned char*)blobs + (size_t)i * blob_stride;
        const int rc = launch(a, st);
        if (rc) return rc;
        for (int b = 0; b < batch; ++b) cur[b] = a.bout[b];
    }
    return 0;
}

// Persistent tile walk, XCD-aware and balanced.  Workgroup b runs on XCD b % 8 (observed placement, used for speed only):
// the workgroups of one XCD get consecutive ranks, rank r walks the CONTIGUOUS tile range [r*n/g, (r+1)*n/g), so every
// workgroup has floor or ceil(n/g) tiles (a strided walk inside fixed eighths of the frame left single workgroups with
// twice the tiles of the others whenever g ~ n) and the tiles in flight on one XCD are neighbours sharing halo rows in
// that XCD's L2.
// (g = gridDim.x, passed in the kernel's own argument struct: read from the hidden dispatch arguments it costs a
// separate scalar-load round trip)
__device__ __forceinline__ void rv_tile_range(const int n_tiles, const int g, int& t_begin, int& t_end) {
    const int b = (int)blockIdx.x;
    int rank = b;
    if (g >= 8) {
        const int xcd = b & 7;
        rank = b >> 3;
        for (int y = 0; y < xcd; ++y) rank += (g - y + 7) >> 3;
    }
    // 32-bit unsigned divisions (~30 instructions each; the 64-bit ones hipcc expands to several hundred instructions
    // PER WAVE, at the head of every persistent launch: an s_memtime probe put ~4 000 cycles between kernel entry and the
    // first x-tile load).  rank * n_tiles < 2^31: at most 1 024 workgroups x 2 M tiles -- checked by the callers' hosts.
    const unsigned un = (unsigned)n_tiles, ug = (unsigned)g;
    t_begin = (int)(((unsigned)rank * un) / ug);
    t_end = (int)(((unsigned)(rank + 1) * un) / ug);
}

// ReflectionPad2d index (no edge repeat): -1 -> 1, n -> n-2.  Valid for -n < i < 2n-1.
__device__ __forceinline__ int rv_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

__device__ __forceinline__ float rv_lrelu(float v, float slope) { return v >= 0.f ? v : v * slope; }

// torch.linspace(-1, 1, n)[j] as computed by ATen's CPU kernel (symmetric two-sided evaluation).
__device__ __forceinline__ float rv_linspace_m1p1(int j, int n) {
    const float step = 2.0f / (float)(n - 1);
    return (j < n / 2) ? (-1.0f + step * (float)j) : (1.0f - step * (float)(n - 1 - j));
}

// warp (models/utils.py:35-43): zeros padding, align_corners=False sampling of a linspace(-1,1) grid displaced by the flow.
// Shared by the stand-alone warp kernels (resample.hip) and the conv kernels that warp a source while staging it.
struct WarpCoord { int x0, y0; float w00, w01, w10, w11; bool v00, v01, v10, v11; };

__device__ __forceinline__ WarpCoord warp_coord_uv(const float u, const float v, int hf, int wf, int hin, int win, int y, int x);
__device__ __forceinline__ WarpCoord warp_coord(const float* flow, int hf, int wf, int hin, int win, int y, int x) {
    const size_t fp = (size_t)y * wf + x;
    return warp_coord_uv(flow[fp], flow[(size_t)hf * wf + fp], hf, wf, hin, win, y, x);
}
// (u, v): the flow at grid pixel (y, x)
__device__ __forceinline__ WarpCoord warp_coord_uv(const float u, const float v, int hf, int wf, int hin, int win, int y, int x) {
    const float gx = rv_linspace_m1p1(x, wf) + u / (((float)win - 1.0f) / 2.0f);
    const float gy = rv_linspace_m1p1(y, hf) + v / (((float)hin - 1.0f) / 2.0f);
    const float xs = ((gx + 1.0f) * (float)win - 1.0f) / 2.0f;
    const float ys = ((gy + 1.0f) * (float)hin - 1.0f) / 2.0f;
    const float fx = floorf(xs), fy = floorf(ys);
    const float tx = xs - fx, ty = ys - fy;
    WarpCoord c;
    // clamp before the int conversion so wild flows cannot overflow; such taps are out of range anyway
    c.x0 = (int)fminf(fmaxf(fx, -2.0f), (float)win + 1.0f);
    c.y0 = (int)fminf(fmaxf(fy, -2.0f), (float)hin + 1.0f);
    const bool xin0 = c.x0 >= 0 && c.x0 < win, xin1 = c.x0 + 1 >= 0 && c.x0 + 1 < win;
    const bool yin0 = c.y0 >= 0 && c.y0 < hin, yin1 = c.y0 + 1 >= 0 && c.y0 + 1 < hin;
    c.v00 = xin0 && yin0; c.v01 = xin1 && yin0; c.v10 = xin0 && yin1; c.v11 = xin1 && yin1;
    c.w00 = (1.0f - ty) * (1.0f - tx); c.w01 = (1.0f - ty) * tx;
    c.w10 = ty * (1.0f - tx); c.w11 = ty * tx;
    return c;
}

// one 16-byte channel group of warp(x, flow) at grid pixel (y, px): fp32 blend in tap order 00, 01, 10, 11, then fp16
__device__ __forceinline__ uint4 warp_group16(const unsigned char* x, int pixb, int hin, int win, const WarpCoord& c, int goff) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto tap = [&](bool valid, int yy, int xx, float wgt) {
        if (valid) {
            const f16x8 v = *reinterpret_cast<const f16x8*>(x + ((size_t)yy * win + xx) * pixb + goff);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += wgt * (float)v[k];
        }
    };
    tap(c.v00, c.y0, c.x0, c.w00);
    tap(c.v01, c.y0, c.x0 + 1, c.w01);
    tap(c.v10, c.y0 + 1, c.x0, c.w10);
    tap(c.v11, c.y0 + 1, c.x0 + 1, c.w11);
    union { f16x8 h; uint4 u; } o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = (f16)acc[k];
    return o.u;
}

// align_corners=True bilinear taps of output index o (n_in -> n_out samples): shared by resample.hip's resize_kernel and by the
// kernels that evaluate the up-sampled map in place.  Contraction is switched OFF here: under hipcc's default -ffp-contract=fast
// `x - (float)i0` may or may not fuse with the product that made x, depending on the code around the inlined copy -- two
// kernels restating the same taps then differ by an ulp (found on the GPU: refvsr_warp_nhwc16_up2 vs resize + warp).
__device__ __forceinline__ void rv_bilinear_ac_src(int o, int n_in, int n_out, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
    const float sc = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f;
    const float x = (float)o * sc;
    i0 = min((int)x, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    l1 = x - (float)i0;
}
// F.interpolate(s, scale_factor=2, mode='bilinear', align_corners=True) of a planar fp32 map [h][w] at output pixel (oy, ox)
// of the [2h][2w] grid: the taps and FMA chains of resample.hip's resize_kernel<BILINEAR_AC> (flow_up2 of the engine)
__device__ __forceinline__ float rv_bilinear_ac2_at(const float* __restrict__ s, int h, int w, int oy, int ox) {
    int y0, y1, x0, x1;
    float ly, lx;
    rv_bilinear_ac_src(oy, h, 2 * h, y0, y1, ly);
    rv_bilinear_ac_src(ox, w, 2 * w, x0, x1, lx);
    const float wy0 = 1.0f - ly, wx0 = 1.0f - lx;
    const float r0 = fmaf(lx, s[(size_t)y0 * w + x1], fmaf(wx0, s[(size_t)y0 * w + x0], 0.0f));
    const float r1 = fmaf(lx, s[(size_t)y1 * w + x1], fmaf(wx0, s[(size_t)y1 * w + x0], 0.0f));
    return fmaf(ly, r1, fmaf(wy0, r0, 0.0f));
}

// ---- bicubic F.interpolate taps (ATen upsample_bicubic2d, A = -0.75, align_corners=False): shared by resample.hip's
// resize_kernel and the kernels that evaluate the up-sampled map on the fly (conv24.hip: CONF variant)
__device__ __forceinline__ void rv_cubic_taps(float t, float* wgt) {
    const float A = -0.75f;
    float x = t + 1.0f;
    wgt[0] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
    x = t;
    wgt[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    x = 1.0f - t;
    wgt[2] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    x = 2.0f - t;
    wgt[3] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}
// source indices (clamped) and weights of output index o; scale = source step per output sample
__device__ __forceinline__ void rv_cubic_src(int o, int n_in, float scale, int* idx, float* wgt) {
    const float x = ((float)o + 0.5f) * scale - 0.5f;
    const float fl = floorf(x);
    const int ix = (int)fl;
    rv_cubic_taps(x - fl, wgt);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(ix - 1 + k, 0), n_in - 1);
}
// one bicubic sample of a planar fp32 map [h][w] at output pixel (oy, ox): the FMA chains of resize_kernel<BICUBIC>
__device__ __forceinline__ float rv_bicubic_at(const float* __restrict__ s, int h, int w, int oy, int ox, float sy, float sx) {
    int iy[4], ix[4];
    float wy[4], wx[4];
    rv_cubic_src(oy, h, sy, iy, wy);
    rv_cubic_src(ox, w, sx, ix, wx);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float r = 0.0f;
        const float* row = s + (size_t)iy[j] * w;
#pragma unroll
        for (int i = 0; i < 4; ++i) r = fmaf(wx[i], row[ix[i]], r);
        acc = fmaf(wy[j], r, acc);
    }
    return acc;
}

// ---- result formats of the output head (ABI 14, REFVSR_RESULT_*): one value v in [0, 1] of the planar [3][h][w] result at element e.
// U8 = what the reference's consumers make of the fp32 frame on the CPU (evaluation/eval_qual_quan.py:117-119: cv2.imwrite of
// output * 255 = saturate_cast<uchar>, round to nearest even): rint(v * 255) in fp32, the same two roundings.
// `fmt` may carry REFVSR_RESULT_HWC: the layout decides the element (rv_result_index), never the value or its rounding.
__device__ __forceinline__ void rv_store_result(void* out, const size_t e, const float v, const int fmt) {
    const int f = fmt & REFVSR_RESULT_FMT_MASK;
    if (f == REFVSR_RESULT_F32) reinterpret_cast<float*>(out)[e] = v;
    else if (f == REFVSR_RESULT_F16) reinterpret_cast<f16*>(out)[e] = (f16)v;
    else reinterpret_cast<unsigned char*>(out)[e] = (unsigned char)__float2int_rn(v * 255.0f);
}
// element of channel c at (y, x) of a 3 x h x w result: planar [3][h][w], or interleaved [h][w][3] with REFVSR_RESULT_HWC
__host__ __device__ __forceinline__ size_t rv_result_index(const int fmt, const int c, const int y, const int x, const int h, const int w) {
    return (fmt & REFVSR_RESULT_HWC) ? ((size_t)y * w + x) * 3 + c : ((size_t)c * h + y) * w + x;
}
// host-side check of an out_fmt argument: a known sample format, optionally | REFVSR_RESULT_HWC
static inline bool rv_result_fmt_ok(const int fmt) {
    return fmt >= 0 && (fmt & ~(REFVSR_RESULT_FMT_MASK | REFVSR_RESULT_HWC)) == 0 && (fmt & REFVSR_RESULT_FMT_MASK) <= REFVSR_RESULT_U8;
}
// bytes of one sample of a checked result format
static inline size_t rv_result_sample_bytes(const int fmt) {
    const int f = fmt & REFVSR_RESULT_FMT_MASK;
    return f == REFVSR_RESULT_F32 ? 4 : f == REFVSR_RESULT_F16 ? 2 : 1;
}
// f(RvType<T>{}, std::bool_constant<HWC>{}) for the sample type and the layout of a checked result format: the launchers that are
// templates over both (yuv.hip, resize.hip) name their instance with `typename decltype(t)::type` and `decltype(hwc)::value`
template <typename T>
struct RvType { typedef T type; };
template <class F>
static auto rv_result_dispatch(const int fmt, F&& f) {
    const int s = fmt & REFVSR_RESULT_FMT_MASK;
    const bool hwc = (fmt & REFVSR_RESULT_HWC) != 0;
    if (s == REFVSR_RESULT_F32) return hwc ? f(RvType<float>{}, std::true_type{}) : f(RvType<float>{}, std::false_type{});
    if (s == REFVSR_RESULT_F16) return hwc ? f(RvType<f16>{}, std::true_type{}) : f(RvType<f16>{}, std::false_type{});
    return hwc ? f(RvType<unsigned char>{}, std::true_type{}) : f(RvType<unsigned char>{}, std::false_type{});
}
// The frame tables of a launcher that reads nframes frames of sbytes bytes (samples of ssize bytes) and writes as many of dbytes
// bytes (samples of dsize bytes): src[] and dst[] go to the argument struct's tables once every frame is there and aligned to its
// samples, and no destination lies over a source or another destination.  `name` in front of the refusals.
static int rv_frame_tables(const char* name, const void* const* src, void* const* dst, const int nframes, const size_t ssize,
                           const size_t dsize, const size_t sbytes, const size_t dbytes, const void** a_src, void** a_dst) {
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(src[i] && dst[i], "%s: null pointer (frame %d)", name, i);
        RV_CHECK(((uintptr_t)src[i] & (ssize - 1)) == 0 && ((uintptr_t)dst[i] & (dsize - 1)) == 0,
                 "%s: source and destination must be aligned to their samples (frame %d)", name, i);
        a_src[i] = src[i];
        a_dst[i] = dst[i];
    }
    for (int i = 0; i < nframes; ++i) {
        const uintptr_t d0 = (uintptr_t)dst[i];
        for (int j = 0; j < nframes; ++j) {
            const uintptr_t s0 = (uintptr_t)src[j], d1 = (uintptr_t)dst[j];
            RV_CHECK(d0 + dbytes <= s0 || s0 + sbytes <= d0, "%s: destination %d overlaps source %d", name, i, j);
            RV_CHECK(i == j || d0 + dbytes <= d1 || d1 + dbytes <= d0, "%s: destinations %d and %d overlap", name, i, j);
        }
    }
    return 0;
}

// lane l: a[l] + a[l ^ 32]   (v_mov, v_permlane32_swap, v_add per register): the fold of an accumulator whose lanes 32-63 hold the
// lo sums (resblock24.hip, conv24.hip).  The two results are taken out of the builtin's vector as plain unsigned values first:
// __builtin_bit_cast on `pr[1]` directly made hipcc (ROCm 7.2) read element 0 twice.
__device__ __forceinline__ float rv_fold1(const float a) {
    const unsigned u = __float_as_uint(a);
    const auto pr = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const unsigned x0 = pr[0], x1 = pr[1];
    return __uint_as_float(x0) + __uint_as_float(x1);
}

// MFMA column n (= lane & 15) -> pixel of the 16-pixel tile: the lanes a ds_read_b128 group takes from one K-block
// ({0-3, 12-15} | {4-11}) land on the even | odd pixels.
__device__ __forceinline__ int rv_pix16(int n) { return (n < 4 || n >= 12) ? ((n & 7) << 1) : (((n - 4) << 1) | 1); }
