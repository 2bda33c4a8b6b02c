// Y'CbCr result frames (extension: the reference's consumer writes PNG / JPG from the RGB result, evaluation/eval_qual_quan.py:117-119;
// a video consumer converts that RGB to 4:2:0, 4:2:2 or 4:4:4 on the CPU first).  refvsr_result_to_yuv turns up to
// REFVSR_YUV420_MAX_FRAMES result frames of one geometry -- any of the six forms the output head stores, float32 | float16 | uint8,
// planar or interleaved -- into frames of one format, sampling and siting in one launch; refvsr_result_to_yuv420 is its 4:2:0 /
// centre form: NV12 | I420 | P010 | I420P10 buffers.  ONE kernel template, an instance per (source, format, sampling, siting).
//
// Exactness: the kernel returns the bits of refvsr_amd/yuv.py:rgb_to_yuv.  Everything is float64 with every operation rounded on its
// own: contraction is OFF for this file (one fused multiply-add moves rint at a tie).  A byte u is the float64 quotient u / 255.0
// (a 256-entry LDS table filled by that division), a float widens exactly.
//
// Shape: bandwidth-bound, no reuse.  A thread owns NPX pixels of ROWS source rows (two for 4:2:0, one for 4:2:2 / 4:4:4): 16 pixels
// of a byte source, 8 of a float one.  Whole, aligned groups load 16 bytes at a time from each row (planar: from each plane and row)
// and store the group's Y row pieces and chroma as one vector each.  A ragged row end goes element by element.  So does a source
// row's load when its address (planar: any of its three planes' addresses) misses 16 bytes -- each row decides for itself -- and so
// do the group's stores when any of them (the Y row pieces, the chroma piece or pieces) misses min(16, the piece's bytes): the stores
// decide together, because one branch per store costs 1.5 x the registers (140 -> 229 VGPRs for byte sources) on the path every
// real frame takes.  A frame whose row pitches, source and destination, are multiples of 16 bytes on 16-byte bases (every result
// of the engine at 1080p / 8K) is all vectors; float32 rows of w = 2 (mod 4) load every even row wide and every odd row by element
// and store by element.  Grid-stride over the frame's groups, sized to the stream's CUs; blockIdx.y is the frame.  Plain vector
// stores only.
//
// The mean one chroma sample stands for, e = ecb | ecr unquantised:
//   4:4:4          e
//   4:2:2 centre   (e[2j] + e[2j+1]) 0.5
//   4:2:0 centre   ((e00 + e01) + (e10 + e11)) 0.25: the first row's pair sum, then + the second row's.  NOT the column sums below:
//                  that is another float64 function and moves ties
//   left           the odd column LEFT of the pair joins: m = ((v[l] + v[2j+1]) + (v[2j] + v[2j])) scale, l = max(2j - 1, 0), v = e
//                  (4:2:2, scale 0.25) or the sum of the pair's two rows (4:2:0, 0.125).  Inside a group that column is the pair
//                  before; for the group's first pair it is the pixel in front of the group, x0 - 1 of the same rows -- another
//                  thread's, or another workgroup's, pixel -- which the thread loads for itself (three samples per row, element by
//                  element, from the cache line its neighbour reads) and converts again.  The first group of a row has no such
//                  pixel: l = 0, the pair's own even column.
#pragma clang fp contract(off)
#include "yuv_common.h"

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

template <typename T, bool HWC, int FMT, int SAMP, bool LEFT>
__global__ void __launch_bounds__(256) yuv_kernel(YuvArgs a) {
    constexpr int NPX = YuvSrc<T>::NPX;
    constexpr bool D10 = yuv_d10(FMT), SEMI = yuv_semi(FMT);
    constexpr bool C444 = SAMP == REFVSR_YUV_SAMPLING_444, V2 = SAMP == REFVSR_YUV_SAMPLING_420;
    static_assert(!SEMI || V2, "semi-planar frames are 4:2:0");
    static_assert(!(C444 && LEFT), "4:4:4 has no siting");
    constexpr int SHIFT = FMT == REFVSR_YUV_P010 ? 6 : 0;
    constexpr int ROWS = V2 ? 2 : 1;
    constexpr int NC = C444 ? NPX : NPX / 2;                         // chroma samples of the group per plane
    using S = typename std::conditional<D10, uint16_t, uint8_t>::type;
    constexpr int SRC_BYTES = NPX * (int)sizeof(T);                  // one plane's piece of a row; interleaved: three of them
    constexpr int ROW_BYTES = NPX * (int)sizeof(S);                  // a Y row piece, and the interleaved chroma of the group
    constexpr int PLANE_BYTES = NC * (int)sizeof(S);                 // a Cb or Cr piece of the planar formats
    constexpr uintptr_t ROW_MASK = (ROW_BYTES < 16 ? ROW_BYTES : 16) - 1, PLANE_MASK = (PLANE_BYTES < 16 ? PLANE_BYTES : 16) - 1;
    constexpr double SCALE = V2 ? 0.125 : 0.25;                      // of the left-sited mean
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
    const long cplane = yuv_chroma_plane(hw, SAMP);
    const double kr = a.k[0], kg = a.k[1], kb = a.k[2], icb = a.k[3], icr = a.k[4], oy = a.k[5], sy = a.k[6], oc = a.k[7], sc = a.k[8];
    const double maxc = D10 ? 1023.0 : 255.0;
    const int gpr = (w + NPX - 1) / NPX;                             // groups per row (4:2:0: per row pair)
    const long items = (long)(h / ROWS) * gpr;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < items; k += (long)gridDim.x * blockDim.x) {
        const int by = (int)(k / gpr);
        const int x0 = (int)(k - (long)by * gpr) * NPX;
        const int n = w - x0 < NPX ? w - x0 : NPX;                   // pixels of the group per row (even)
        const long p0 = (long)(ROWS * by) * w + x0;                  // the group's first pixel; a second row's is p0 + w
        S* const y0 = dst + p0;
        S* const c0 = dst + hw + (SEMI || C444 ? (long)by * w + x0 : (long)by * w2 + (x0 >> 1));       // interleaved CbCr, or Cb
        S* const c1 = c0 + cplane;                                                                    // Cr of the planar formats

        // A whole group (n == NPX) loads a row as vectors where that row's addresses are 16-byte aligned, each row for itself, and
        // stores as vectors where all of its store addresses are aligned (the header comment has the cases and the reason).
        const bool full = n == NPX;
        alignas(16) T v[ROWS][3][NPX];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
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

        // left siting: v[x0 - 1], the odd column in front of the group (x0 >= NPX here: the pixel exists, in the group's own rows)
        double lb = 0.0, lr = 0.0;
        if constexpr (LEFT) {
            if (x0 > 0) {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const long q = p0 + (long)r * w - 1;
                    const double R = yuv_value(HWC ? src[3 * q] : src[q], tbl), G = yuv_value(HWC ? src[3 * q + 1] : src[hw + q], tbl),
                                 B = yuv_value(HWC ? src[3 * q + 2] : src[2 * hw + q], tbl);
                    const double ey = (kr * R + kg * G) + kb * B;
                    const double eb = (B - ey) * icb, er = (R - ey) * icr;
                    lb = r == 0 ? eb : lb + eb;
                    lr = r == 0 ? er : lr + er;
                }
            }
        }

        alignas(16) S yy[ROWS][NPX], cc[2 * NC];                     // cc: Cb Cr pairs (semi-planar), or [Cb piece | Cr piece]
#pragma unroll
        for (int j = 0; j < NPX / 2; ++j) {
            double vb[2], vr[2];                                     // v of the pair's even and odd column; 4:2:0 / centre: the rows' pair sums
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int i = 2 * j + d;
                    const double R = yuv_value(v[r][0][i], tbl), G = yuv_value(v[r][1][i], tbl), B = yuv_value(v[r][2][i], tbl);
                    const double ey = (kr * R + kg * G) + kb * B;
                    yy[r][i] = yuv_code<S, SHIFT>(oy + sy * ey, maxc);
                    const double eb = (B - ey) * icb, er = (R - ey) * icr;
                    if constexpr (V2 && !LEFT) {                     // e[r][2j] + e[r][2j+1]
                        vb[r] = d == 0 ? eb : vb[r] + eb;
                        vr[r] = d == 0 ? er : vr[r] + er;
                    } else {                                         // 4:2:0: e[2i][x] + e[2i+1][x]
                        vb[d] = r == 0 ? eb : vb[d] + eb;
                        vr[d] = r == 0 ? er : vr[d] + er;
                    }
                }
            }
            if constexpr (C444) {
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    cc[2 * j + d] = yuv_code<S, SHIFT>(oc + sc * vb[d], maxc);
                    cc[NC + 2 * j + d] = yuv_code<S, SHIFT>(oc + sc * vr[d], maxc);
                }
            } else {
                double mb, mr;
                if constexpr (LEFT) {
                    if (j == 0 && x0 == 0) { lb = vb[0]; lr = vr[0]; }          // l = max(2j - 1, 0) = 0
                    mb = ((lb + vb[1]) + (vb[0] + vb[0])) * SCALE;
                    mr = ((lr + vr[1]) + (vr[0] + vr[0])) * SCALE;
                    lb = vb[1];
                    lr = vr[1];
                } else {                                             // centre: the pair (4:2:2), the two rows' pair sums (4:2:0)
                    mb = (vb[0] + vb[1]) * (V2 ? 0.25 : 0.5);
                    mr = (vr[0] + vr[1]) * (V2 ? 0.25 : 0.5);
                }
                const S cb = yuv_code<S, SHIFT>(oc + sc * mb, maxc), cr = yuv_code<S, SHIFT>(oc + sc * mr, maxc);
                if constexpr (SEMI) { cc[2 * j] = cb; cc[2 * j + 1] = cr; }
                else { cc[j] = cb; cc[NC + j] = cr; }
            }
        }

        uintptr_t smis = ((uintptr_t)y0 | (uintptr_t)(y0 + (ROWS - 1) * w)) & ROW_MASK;
        smis |= SEMI ? (uintptr_t)c0 & ROW_MASK : ((uintptr_t)c0 | (uintptr_t)c1) & PLANE_MASK;
        if (full && smis == 0) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) yuv_store<ROW_BYTES>(y0 + r * w, yy[r]);
            if constexpr (SEMI) {
                yuv_store<ROW_BYTES>(c0, cc);
            } else {
                yuv_store<PLANE_BYTES>(c0, cc);
                yuv_store<PLANE_BYTES>(c1, cc + NC);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPX; ++i)
                if (i < n) {
#pragma unroll
                    for (int r = 0; r < ROWS; ++r) y0[r * w + i] = yy[r][i];
                }
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if ((C444 ? j : 2 * j) < n) {
                    if constexpr (SEMI) { c0[2 * j] = cc[2 * j]; c0[2 * j + 1] = cc[2 * j + 1]; }
                    else { c0[j] = cc[j]; c1[j] = cc[NC + j]; }
                }
        }
    }
}

extern "C" int refvsr_yuv420_max_frames(void) { return REFVSR_YUV420_MAX_FRAMES; }

extern "C" size_t refvsr_yuv420_bytes(int h, int w, int yuv_fmt) { return yuv_frame_bytes(h, w, yuv_fmt, REFVSR_YUV_SAMPLING_420); }

extern "C" size_t refvsr_yuv_frame_bytes(int h, int w, int yuv_fmt, int sampling) { return yuv_frame_bytes(h, w, yuv_fmt, sampling); }

template <typename T, bool HWC>
static void yuv_launch(int yuv_fmt, int sampling, bool left, dim3 grid, hipStream_t st, const YuvArgs& a) {
#define YUV_GO(F, S, L)                                                                           \
    if (yuv_fmt == REFVSR_YUV_##F && sampling == REFVSR_YUV_SAMPLING_##S && left == L)            \
        hipLaunchKernelGGL((yuv_kernel<T, HWC, REFVSR_YUV_##F, REFVSR_YUV_SAMPLING_##S, L>), grid, dim3(256), 0, st, a);
    YUV_INSTANCES(YUV_GO)
#undef YUV_GO
}

// The checked launch of both entries, `name` in front of its messages.  yuv_fmt is checked again where the 4:2:0 entry has always
// checked it: behind the result format.
static int yuv_convert(const char* name, const void* const* src, int src_fmt, void* const* dst, int nframes, int h, int w, int yuv_fmt,
                       int sampling, int siting, const double* coef9, void* stream) {
    RV_CHECK(src && dst, "%s: null frame table", name);
    RV_CHECK(coef9, "%s: null coefficients", name);
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_YUV420_MAX_FRAMES, "%s: 1..%d frames per launch", name, REFVSR_YUV420_MAX_FRAMES);
    RV_CHECK(rv_result_fmt_ok(src_fmt), "%s: unknown result format %d", name, src_fmt);
    RV_CHECK(yuv_fmt_ok(yuv_fmt), "%s: unknown yuv format %d", name, yuv_fmt);
    RV_CHECK(yuv_geometry_ok(h, w), "%s: h, w must be even and positive (got %d x %d)", name, h, w);
    const size_t es = rv_result_sample_bytes(src_fmt);
    RV_CHECK((long long)h * w * 3 * (long long)es < (1ll << 31), "%s: frame too large for 32-bit offsets", name);
    YuvArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = rv_frame_tables(name, src, dst, nframes, es, yuv_sample_bytes(yuv_fmt), (size_t)h * w * 3 * es,
                                   yuv_frame_bytes(h, w, yuv_fmt, sampling), a.src, a.dst);
    if (rc) return rc;
    a.h = h;
    a.w = w;
    for (int i = 0; i < 9; ++i) a.k[i] = coef9[i];
    hipStream_t st = (hipStream_t)stream;
    const int npx = (src_fmt & REFVSR_RESULT_FMT_MASK) == REFVSR_RESULT_U8 ? YuvSrc<unsigned char>::NPX : YuvSrc<float>::NPX;
    const long items = (long)(sampling == REFVSR_YUV_SAMPLING_420 ? h / 2 : h) * ((w + npx - 1) / npx);
    const long want = (items + 255) / 256;
    long cap = (long)rv_stream_cus(st) * 8 / nframes;                // eight workgroups per CU over all frames
    if (cap < 32) cap = 32;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)nframes);
    const bool left = siting == REFVSR_YUV_SITING_LEFT && sampling != REFVSR_YUV_SAMPLING_444;
    rv_result_dispatch(src_fmt, [&](auto t, auto hwc) {
        yuv_launch<typename decltype(t)::type, decltype(hwc)::value>(yuv_fmt, sampling, left, grid, st, a);
    });
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_result_to_yuv420(const void* const* src, int src_fmt, void* const* dst, int nframes, int h, int w, int yuv_fmt,
                                       const double* coef9, void* stream) {
    return yuv_convert("result_to_yuv420", src, src_fmt, dst, nframes, h, w, yuv_fmt, REFVSR_YUV_SAMPLING_420, REFVSR_YUV_SITING_CENTRE, coef9, stream);
}

extern "C" int refvsr_result_to_yuv(const void* const* src, int src_fmt, void* const* dst, int nframes, int h, int w, int yuv_fmt,
                                    int sampling, int siting, const double* coef9, void* stream) {
    RV_CHECK(yuv_fmt_ok(yuv_fmt), "result_to_yuv: unknown yuv format %d", yuv_fmt);
    RV_CHECK(yuv_sampling_ok(sampling), "result_to_yuv: sampling must be REFVSR_YUV_SAMPLING_420 | _422 | _444 (got %d)", sampling);
    RV_CHECK(yuv_siting_ok(siting), "result_to_yuv: siting must be REFVSR_YUV_SITING_CENTRE | REFVSR_YUV_SITING_LEFT (got %d)", siting);
    RV_CHECK(sampling == REFVSR_YUV_SAMPLING_420 || !yuv_semi(yuv_fmt),
             "result_to_yuv: semi-planar frames (NV12, P010) are 4:2:0 only (format %d, sampling %d)", yuv_fmt, sampling);
    // (4:2:0 / centre answers in the 4:2:0 entry's name)
    const bool plain = sampling == REFVSR_YUV_SAMPLING_420 && siting == REFVSR_YUV_SITING_CENTRE;
    return yuv_convert(plain ? "result_to_yuv420" : "result_to_yuv", src, src_fmt, dst, nframes, h, w, yuv_fmt, sampling, siting, coef9, stream);
}
