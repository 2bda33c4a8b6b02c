// Y'CbCr 4:2:0 result frames (extension: the reference's consumer writes PNG / JPG from the RGB result, evaluation/
// eval_qual_quan.py:117-119; a video consumer converts that RGB to 4:2:0 on the CPU first).  refvsr_result_to_yuv420 turns up to
// REFVSR_YUV420_MAX_FRAMES result frames of one geometry -- any of the six forms the output head stores, float32 | float16 | uint8,
// planar or interleaved -- into NV12 | I420 | P010 | I420P10 buffers in one launch.
//
// Exactness: the kernel returns the bits of refvsr_amd/yuv.py:rgb_to_yuv420.  Everything is float64 with every operation rounded on
// its own: contraction is OFF for this file (one fused multiply-add moves rint at a tie).  A byte u is the float64 quotient u / 255.0
// (a 256-entry LDS table filled by that division), a float widens exactly.
//
// Shape: bandwidth-bound, no reuse.  A thread owns NPX pixels of two source rows (NPX / 2 chroma blocks): 16 pixels of a byte source,
// 8 of a float one.  Whole, aligned groups load 16 bytes at a time from each row (planar: from each plane and row) and store the
// group's Y row pieces and chroma as one vector each.  A ragged row end goes element by element.  So does a source row's load when
// its address (planar: any of its three planes' addresses) misses 16 bytes -- each of the two rows decides for itself -- and so do
// the group's stores when any of them (two Y row pieces, the chroma piece or pieces) misses min(16, the piece's bytes): the stores
// decide together, because one branch per store costs 1.5 x the registers (140 -> 229 VGPRs for byte sources) on the path every
// real frame takes.  A frame whose row pitches, source and destination, are multiples of 16 bytes on 16-byte bases (every result
// of the engine at 1080p / 8K) is all vectors; float32 rows of w = 2 (mod 4) load every even row wide and every odd row by element
// and store by element.  Grid-stride over the frame's groups, sized to the stream's CUs; blockIdx.y is the frame.  Plain vector
// stores only.
#pragma clang fp contract(off)
#include "common.h"

struct YuvArgs {
    const void* src[REFVSR_YUV420_MAX_FRAMES];
    void* dst[REFVSR_YUV420_MAX_FRAMES];
    int h, w;
    double k[9];             // kr, kg, kb, icb, icr, oy, sy, oc, sc
};

template <typename T> struct YuvSrc { static constexpr int NPX = 8; };
template <> struct YuvSrc<unsigned char> { static constexpr int NPX = 16; };

template <typename T>
__device__ __forceinline__ double yuv_value(T v, const double* tbl) {
    if constexpr (std::is_same<T, unsigned char>::value) return tbl[v];
    else return (double)v;
}

// BYTES (a multiple of 16) from a 16-byte aligned address
template <int BYTES>
__device__ __forceinline__ void yuv_load(const void* p, void* regs) {
#pragma unroll
    for (int q = 0; q < BYTES / 16; ++q) reinterpret_cast<uint4*>(regs)[q] = reinterpret_cast<const uint4*>(p)[q];
}

// BYTES = 4 | 8 | 16 | 32 to an address aligned to min(BYTES, 16)
template <int BYTES>
__device__ __forceinline__ void yuv_store(void* p, const void* regs) {
    if constexpr (BYTES == 4) *reinterpret_cast<uint32_t*>(p) = *reinterpret_cast<const uint32_t*>(regs);
    else if constexpr (BYTES == 8) *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(regs);
    else {
#pragma unroll
        for (int q = 0; q < BYTES / 16; ++q) reinterpret_cast<uint4*>(p)[q] = reinterpret_cast<const uint4*>(regs)[q];
    }
}

template <typename S, int SHIFT>
__device__ __forceinline__ S yuv_code(double v, double maxc) {
    const double c = fmin(fmax(rint(v), 0.0), maxc);                 // rint: half to even; the clamp comes before the cast
    return (S)((unsigned)(int)c << SHIFT);
}

template <typename T, bool HWC, int FMT>
__global__ void __launch_bounds__(256) yuv420_kernel(YuvArgs a) {
    constexpr int NPX = YuvSrc<T>::NPX;
    constexpr bool D10 = FMT == REFVSR_YUV_P010 || FMT == REFVSR_YUV_I420P10;
    constexpr bool SEMI = FMT == REFVSR_YUV_NV12 || FMT == REFVSR_YUV_P010;
    constexpr int SHIFT = FMT == REFVSR_YUV_P010 ? 6 : 0;
    using S = typename std::conditional<D10, uint16_t, uint8_t>::type;
    constexpr int SRC_BYTES = NPX * (int)sizeof(T);                  // one plane's piece of a row; interleaved: three of them
    constexpr int ROW_BYTES = NPX * (int)sizeof(S);                  // a Y row piece, and the interleaved chroma of the group
    constexpr int PLANE_BYTES = ROW_BYTES / 2;                       // a Cb or Cr piece of the planar formats
    constexpr uintptr_t ROW_MASK = (ROW_BYTES < 16 ? ROW_BYTES : 16) - 1, PLANE_MASK = (PLANE_BYTES < 16 ? PLANE_BYTES : 16) - 1;
    constexpr bool U8 = std::is_same<T, unsigned char>::value;
    __shared__ double tbl[U8 ? 256 : 1];
    if constexpr (U8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) tbl[i] = (double)i / 255.0;
        __syncthreads();
    }
    const T* __restrict__ src = reinterpret_cast<const T*>(a.src[blockIdx.y]);
    S* __restrict__ dst = reinterpret_cast<S*>(a.dst[blockIdx.y]);
    const int h = a.h, w = a.w, w2 = w >> 1;
    const long hw = (long)h * w;
    const double kr = a.k[0], kg = a.k[1], kb = a.k[2], icb = a.k[3], icr = a.k[4], oy = a.k[5], sy = a.k[6], oc = a.k[7], sc = a.k[8];
    const double maxc = D10 ? 1023.0 : 255.0;
    const int gpr = (w + NPX - 1) / NPX;                             // groups per row pair
    const long items = (long)(h >> 1) * gpr;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < items; k += (long)gridDim.x * blockDim.x) {
        const int by = (int)(k / gpr);
        const int x0 = (int)(k - (long)by * gpr) * NPX;
        const int n = w - x0 < NPX ? w - x0 : NPX;                   // pixels of the group per row (even)
        const long p0 = (long)(2 * by) * w + x0;                     // the group's first pixel; the second row's is p0 + w
        S* const y0 = dst + p0;
        S* const c0 = dst + hw + (SEMI ? (long)by * w + x0 : (long)by * w2 + (x0 >> 1));       // interleaved CbCr, or Cb
        S* const c1 = c0 + (hw >> 2);                                                         // Cr of the planar formats

        // A whole group (n == NPX) loads a row as vectors where that row's addresses are 16-byte aligned, each row for itself, and
        // stores as vectors where all of its store addresses are aligned (the header comment has the cases and the reason).
        const bool full = n == NPX;
        alignas(16) T v[2][3][NPX];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long pr = p0 + (long)r * w;
            uintptr_t mis;
            if constexpr (HWC) mis = (uintptr_t)(src + 3 * pr) & 15;
            else mis = ((uintptr_t)(src + pr) | (uintptr_t)(src + hw + pr) | (uintptr_t)(src + 2 * hw + pr)) & 15;
            if (full && mis == 0) {
                if constexpr (HWC) {
                    alignas(16) T t[3 * NPX];
                    yuv_load<3 * SRC_BYTES>(src + 3 * pr, t);
#pragma unroll
                    for (int i = 0; i < NPX; ++i) { v[r][0][i] = t[3 * i]; v[r][1][i] = t[3 * i + 1]; v[r][2][i] = t[3 * i + 2]; }
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) yuv_load<SRC_BYTES>(src + c * hw + pr, v[r][c]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int i = 0; i < NPX; ++i) v[r][c][i] = i < n ? (HWC ? src[3 * (pr + i) + c] : src[c * hw + pr + i]) : (T)0;
            }
        }

        alignas(16) S yy[2][NPX], cc[NPX];                           // cc: Cb Cr pairs (semi-planar), or [Cb piece | Cr piece]
#pragma unroll
        for (int j = 0; j < NPX / 2; ++j) {
            double scb = 0.0, scr = 0.0;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                double eb[2], er[2];
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int i = 2 * j + d;
                    const double R = yuv_value(v[r][0][i], tbl), G = yuv_value(v[r][1][i], tbl), B = yuv_value(v[r][2][i], tbl);
                    const double ey = (kr * R + kg * G) + kb * B;
                    yy[r][i] = yuv_code<S, SHIFT>(oy + sy * ey, maxc);
                    eb[d] = (B - ey) * icb;
                    er[d] = (R - ey) * icr;
                }
                // ((e00 + e01) + (e10 + e11)): the first row's pair sum, then + the second row's
                scb = r == 0 ? eb[0] + eb[1] : scb + (eb[0] + eb[1]);
                scr = r == 0 ? er[0] + er[1] : scr + (er[0] + er[1]);
            }
            const S cb = yuv_code<S, SHIFT>(oc + sc * (scb * 0.25), maxc), cr = yuv_code<S, SHIFT>(oc + sc * (scr * 0.25), maxc);
            if constexpr (SEMI) { cc[2 * j] = cb; cc[2 * j + 1] = cr; }
            else { cc[j] = cb; cc[NPX / 2 + j] = cr; }
        }

        uintptr_t smis = ((uintptr_t)y0 | (uintptr_t)(y0 + w)) & ROW_MASK;
        smis |= SEMI ? (uintptr_t)c0 & ROW_MASK : ((uintptr_t)c0 | (uintptr_t)c1) & PLANE_MASK;
        if (full && smis == 0) {
            yuv_store<ROW_BYTES>(y0, yy[0]);
            yuv_store<ROW_BYTES>(y0 + w, yy[1]);
            if constexpr (SEMI) {
                yuv_store<ROW_BYTES>(c0, cc);
            } else {
                yuv_store<PLANE_BYTES>(c0, cc);
                yuv_store<PLANE_BYTES>(c1, cc + NPX / 2);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPX; ++i)
                if (i < n) { y0[i] = yy[0][i]; y0[w + i] = yy[1][i]; }
#pragma unroll
            for (int j = 0; j < NPX / 2; ++j)
                if (2 * j < n) {
                    if constexpr (SEMI) { c0[2 * j] = cc[2 * j]; c0[2 * j + 1] = cc[2 * j + 1]; }
                    else { c0[j] = cc[j]; c1[j] = cc[NPX / 2 + j]; }
                }
        }
    }
}

static inline bool yuv_fmt_ok(int f) { return f >= REFVSR_YUV_NV12 && f <= REFVSR_YUV_I420P10; }
static inline size_t yuv_sample_bytes(int f) { return f == REFVSR_YUV_P010 || f == REFVSR_YUV_I420P10 ? 2 : 1; }

extern "C" int refvsr_yuv420_max_frames(void) { return REFVSR_YUV420_MAX_FRAMES; }

extern "C" size_t refvsr_yuv420_bytes(int h, int w, int yuv_fmt) {
    if (h <= 0 || w <= 0 || h % 2 || w % 2 || !yuv_fmt_ok(yuv_fmt)) return 0;
    return (size_t)h * w / 2 * 3 * yuv_sample_bytes(yuv_fmt);
}

template <typename T, bool HWC>
static void yuv_launch(int yuv_fmt, dim3 grid, hipStream_t st, const YuvArgs& a) {
    switch (yuv_fmt) {
        case REFVSR_YUV_NV12: hipLaunchKernelGGL((yuv420_kernel<T, HWC, REFVSR_YUV_NV12>), grid, dim3(256), 0, st, a); break;
        case REFVSR_YUV_I420: hipLaunchKernelGGL((yuv420_kernel<T, HWC, REFVSR_YUV_I420>), grid, dim3(256), 0, st, a); break;
        case REFVSR_YUV_P010: hipLaunchKernelGGL((yuv420_kernel<T, HWC, REFVSR_YUV_P010>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((yuv420_kernel<T, HWC, REFVSR_YUV_I420P10>), grid, dim3(256), 0, st, a); break;
    }
}

extern "C" int refvsr_result_to_yuv420(const void* const* src, int src_fmt, void* const* dst, int nframes, int h, int w, int yuv_fmt,
                                       const double* coef9, void* stream) {
    RV_CHECK(src && dst, "result_to_yuv420: null frame table");
    RV_CHECK(coef9, "result_to_yuv420: null coefficients");
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_YUV420_MAX_FRAMES, "result_to_yuv420: 1..%d frames per launch", REFVSR_YUV420_MAX_FRAMES);
    RV_CHECK(rv_result_fmt_ok(src_fmt), "result_to_yuv420: unknown result format %d", src_fmt);
    RV_CHECK(yuv_fmt_ok(yuv_fmt), "result_to_yuv420: unknown yuv format %d", yuv_fmt);
    RV_CHECK(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "result_to_yuv420: h, w must be even and positive (got %d x %d)", h, w);
    const int f = src_fmt & REFVSR_RESULT_FMT_MASK;
    const size_t es = f == REFVSR_RESULT_F32 ? 4 : f == REFVSR_RESULT_F16 ? 2 : 1;
    RV_CHECK((long long)h * w * 3 * (long long)es < (1ll << 31), "result_to_yuv420: frame too large for 32-bit offsets");
    const size_t sbytes = (size_t)h * w * 3 * es, dbytes = refvsr_yuv420_bytes(h, w, yuv_fmt);
    YuvArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(src[i] && dst[i], "result_to_yuv420: null pointer (frame %d)", i);
        RV_CHECK(((uintptr_t)src[i] & (es - 1)) == 0 && ((uintptr_t)dst[i] & (yuv_sample_bytes(yuv_fmt) - 1)) == 0,
                 "result_to_yuv420: source and destination must be aligned to their samples (frame %d)", i);
        a.src[i] = src[i];
        a.dst[i] = dst[i];
    }
    for (int i = 0; i < nframes; ++i) {
        const uintptr_t d0 = (uintptr_t)dst[i];
        for (int j = 0; j < nframes; ++j) {
            const uintptr_t s0 = (uintptr_t)src[j], d1 = (uintptr_t)dst[j];
            RV_CHECK(d0 + dbytes <= s0 || s0 + sbytes <= d0, "result_to_yuv420: destination %d overlaps source %d", i, j);
            RV_CHECK(i == j || d0 + dbytes <= d1 || d1 + dbytes <= d0, "result_to_yuv420: destinations %d and %d overlap", i, j);
        }
    }
    a.h = h;
    a.w = w;
    for (int i = 0; i < 9; ++i) a.k[i] = coef9[i];
    hipStream_t st = (hipStream_t)stream;
    const int npx = f == REFVSR_RESULT_U8 ? YuvSrc<unsigned char>::NPX : YuvSrc<float>::NPX;
    const long items = (long)(h / 2) * ((w + npx - 1) / npx);
    const long want = (items + 255) / 256;
    long cap = (long)rv_stream_cus(st) * 8 / nframes;                // eight workgroups per CU over all frames
    if (cap < 32) cap = 32;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)nframes);
    const bool hwc = (src_fmt & REFVSR_RESULT_HWC) != 0;
    if (f == REFVSR_RESULT_F32) hwc ? yuv_launch<float, true>(yuv_fmt, grid, st, a) : yuv_launch<float, false>(yuv_fmt, grid, st, a);
    else if (f == REFVSR_RESULT_F16) hwc ? yuv_launch<f16, true>(yuv_fmt, grid, st, a) : yuv_launch<f16, false>(yuv_fmt, grid, st, a);
    else hwc ? yuv_launch<unsigned char, true>(yuv_fmt, grid, st, a) : yuv_launch<unsigned char, false>(yuv_fmt, grid, st, a);
    RV_LAUNCH_CHECK();
    return 0;
}
