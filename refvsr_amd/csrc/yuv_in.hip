// Y'CbCr input frames (extension: the reference's loader reads PNGs, data_loader/utils.py:12-41; a video decoder delivers NV12 or P010
// and a .y4m file holds I420, 4:2:2 or 4:4:4 planes, 1.5 to 3 samples per pixel).  refvsr_yuv_to_rgb turns up to
// REFVSR_YUV420_IN_MAX_FRAMES frames of one geometry, format, sampling and siting into the planar fp32 frames the engine owns, in one
// launch -- the twin of refvsr_ingest_u8 on the way in and the inverse of refvsr_result_to_yuv (yuv.hip) on the way out;
// refvsr_yuv420_to_rgb is its 4:2:0 / centre form: NV12 | I420 | P010 | I420P10.  ONE kernel template, an instance per (format,
// sampling, siting).
//
// Exactness: the kernel returns the bits of refvsr_amd/yuv.py:yuv_to_rgb.  The chroma tap sum (below 2^15) is formed in integers and
// is exact in any order; everything behind it is float64 with every operation rounded on its own, in the model's order, the nine
// coefficients computed once in Python (no division on the device).  Contraction is OFF for this file by construction, to keep the
// kernel the same function as the model -- but no test can pin that: the final rounding to float32 hides nearly every one-ulp
// float64 difference a fused multiply-add could make.  float32 arithmetic is NOT the same function (it differs on about 42 % of
// random samples).
//
// Shape: bandwidth-bound (1.5 to 6 bytes in, 12 out per pixel), no reuse worth LDS.  A thread owns 8 columns of ROWS luma rows (two
// for 4:2:0, which share their chroma row pair -- the three chroma rows above, own, below come from cache; one for 4:2:2 / 4:4:4).  A
// workgroup is 64 column groups (512 pixels) x 4 rows (pairs), so every wave walks ONE row (pair) and the address phase of each of
// its loads is wave-uniform: a source frame lies at any multiple of its sample size (8-bit frames inside a [t, 3h/2, w] window are
// 3hw/2 bytes apart: 702 at 18 x 26) and w is only even, so a row piece is loaded with the widest of 16 / 8 / 4 / 2 / 1-byte loads
// its address allows; a ragged row end goes element by element.  Destination rows are 8-byte aligned: float4 stores where
// w % 4 == 0, float2 otherwise.  One work item per thread, the grid sized by the work (no loop); blockIdx.y is the frame.  Plain
// vector stores only.
//
// The integer tap sum 16 m: a horizontal sum (of weight 4) of a chroma row, then the vertical 3 : 1 of 4:2:0 with the row above an
// even y or below an odd one (4:2:2: the row's own sum, x 4), neighbours clamped at the frame's edges:
//   centre       3 C[cx] + C[cx'],  cx' the block on the pixel's side        (4:2:0: 9 C[cy,cx] + 3 C[cy',cx] + 3 C[cy,cx'] + C[cy',cx'])
//   left even x  4 C[cx]            odd x  2 C[cx] + 2 C[cxr],  cxr = min(cx + 1, w/2 - 1)
// The blocks beside a group's own are its neighbours' (another thread's, or across a 512-pixel span another workgroup's): each
// thread loads them for itself.  4:4:4 has no taps: 16 C[y][x]; REFVSR_YUV_CHROMA_NEAREST: 16 x the own sample, every sampling.
#pragma clang fp contract(off)
#include "yuv_common.h"

struct YuvInArgs {
    const void* src[REFVSR_YUV420_IN_MAX_FRAMES];
    float* dst[REFVSR_YUV420_IN_MAX_FRAMES];
    int h, w;
    int gpr;                 // column groups of 8 per row (pair)
    int gxb;                 // workgroups along a row (pair)
    int nearest;             // chroma mode: 0 bilinear, 1 nearest
    double k[9];             // oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg
};

template <int L> struct YinWord;
template <> struct YinWord<16> { using T = uint4; };
template <> struct YinWord<8> { using T = uint2; };
template <> struct YinWord<4> { using T = uint32_t; };
template <> struct YinWord<2> { using T = uint16_t; };
template <> struct YinWord<1> { using T = uint8_t; };

template <int L, int B>
__device__ __forceinline__ void yin_words(const void* p, void* v) {
    using T = typename YinWord<L>::T;
#pragma unroll
    for (int q = 0; q < B / L; ++q) reinterpret_cast<T*>(v)[q] = reinterpret_cast<const T*>(p)[q];
}

// N samples (2 .. 16 bytes) from an address aligned to its sample: all of them (n == N) with the widest loads the address allows, or
// the first n element by element (the rest are 0)
template <typename S, int N>
__device__ __forceinline__ void yin_load(const S* __restrict__ p, int n, S* v) {
    constexpr int B = N * (int)sizeof(S);
    const uintptr_t a = (uintptr_t)p;
    if (n == N) {
        if (B >= 16 && (a & 15) == 0) yin_words<B >= 16 ? 16 : B, B>(p, v);
        else if (B >= 8 && (a & 7) == 0) yin_words<B >= 8 ? 8 : B, B>(p, v);
        else if (B >= 4 && (a & 3) == 0) yin_words<B >= 4 ? 4 : B, B>(p, v);
        else if (sizeof(S) == 2 || (a & 1) == 0) yin_words<2, B>(p, v);
        else yin_words<1, B>(p, v);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = i < n ? p[i] : (S)0;
    }
}

template <int FMT, typename S>
__device__ __forceinline__ int yin_code(S s) {
    if constexpr (FMT == REFVSR_YUV_P010) return (int)s >> 6;                  // the low six bits are ignored, whatever they hold
    else if constexpr (FMT == REFVSR_YUV_I420P10) return (int)s & 1023;
    else return (int)s;
}

template <int FMT, int SAMP, bool LEFT>
__global__ void __launch_bounds__(256) yuv_in_kernel(YuvInArgs a) {
    constexpr bool D10 = yuv_d10(FMT), SEMI = yuv_semi(FMT);
    constexpr bool C444 = SAMP == REFVSR_YUV_SAMPLING_444, V2 = SAMP == REFVSR_YUV_SAMPLING_420;
    static_assert(!SEMI || V2, "semi-planar frames are 4:2:0");
    static_assert(!(C444 && LEFT), "4:4:4 has no siting");
    constexpr int ROWS = V2 ? 2 : 1;
    constexpr int NQ = V2 ? 3 : 1, OWN = V2 ? 1 : 0;                           // chroma rows in registers, and the pixel's own among them
    constexpr int NCOL = C444 ? 8 : 6;
    using S = typename std::conditional<D10, uint16_t, uint8_t>::type;
    const int h = a.h, w = a.w, hr = h / ROWS, w2 = w >> 1;
    const int by = (int)(blockIdx.x / a.gxb) * 4 + (int)threadIdx.y;           // the row (4:2:0: the row pair): one per wave
    const int g = (int)(blockIdx.x % a.gxb) * 64 + (int)threadIdx.x;
    if (by >= hr || g >= a.gpr) return;
    const S* __restrict__ src = reinterpret_cast<const S*>(a.src[blockIdx.y]);
    float* __restrict__ dst = a.dst[blockIdx.y];
    const size_t hw = (size_t)h * w;
    const size_t cplane = yuv_chroma_plane(hw, SAMP);
    const int x0 = g * 8;
    const int n = w - x0 < 8 ? w - x0 : 8;                                     // pixels of the group per row (even)
    const int nb = n >> 1;                                                     // its chroma blocks
    const int bx0 = x0 >> 1;
    const int cxl = bx0 > 0 ? bx0 - 1 : 0, cxr = bx0 + nb < w2 ? bx0 + nb : w2 - 1;       // the clamped neighbour columns

    alignas(16) S yv[ROWS][8];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) yin_load<S, 8>(src + (size_t)(ROWS * by + r) * w + x0, n, yv[r]);

    // chroma codes.  4:4:4: the row's eight samples.  Otherwise [left neighbour | the group's four blocks | right neighbour] of the
    // row (4:2:0: of the rows above (clamped), own, below (clamped))
    int cb[NQ][NCOL], cr[NQ][NCOL];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int cy = !V2 ? by : q == 0 ? (by > 0 ? by - 1 : 0) : q == 1 ? by : (by + 1 < hr ? by + 1 : hr - 1);
        if constexpr (C444) {
            const S* rowb = src + hw + (size_t)cy * w;
            alignas(16) S c0[8], c1[8];
            yin_load<S, 8>(rowb + x0, n, c0);
            yin_load<S, 8>(rowb + cplane + x0, n, c1);
#pragma unroll
            for (int i = 0; i < 8; ++i) { cb[q][i] = yin_code<FMT>(c0[i]); cr[q][i] = yin_code<FMT>(c1[i]); }
        } else {
            int rb, rr;
            cb[q][5] = cr[q][5] = 0;                                           // (read by the unused pixels of a ragged group)
            if constexpr (SEMI) {
                const S* row = src + hw + (size_t)cy * w;
                alignas(16) S c[8];
                alignas(4) S l[2], e[2];
                yin_load<S, 8>(row + x0, n, c);
                yin_load<S, 2>(row + 2 * cxl, 2, l);
                yin_load<S, 2>(row + 2 * cxr, 2, e);
#pragma unroll
                for (int j = 0; j < 4; ++j) { cb[q][1 + j] = yin_code<FMT>(c[2 * j]); cr[q][1 + j] = yin_code<FMT>(c[2 * j + 1]); }
                cb[q][0] = yin_code<FMT>(l[0]);
                cr[q][0] = yin_code<FMT>(l[1]);
                rb = yin_code<FMT>(e[0]);
                rr = yin_code<FMT>(e[1]);
            } else {
                const S* rowb = src + hw + (size_t)cy * w2;
                const S* rowr = rowb + cplane;
                alignas(8) S c0[4], c1[4];
                yin_load<S, 4>(rowb + bx0, nb, c0);
                yin_load<S, 4>(rowr + bx0, nb, c1);
#pragma unroll
                for (int j = 0; j < 4; ++j) { cb[q][1 + j] = yin_code<FMT>(c0[j]); cr[q][1 + j] = yin_code<FMT>(c1[j]); }
                cb[q][0] = yin_code<FMT>(rowb[cxl]);
                cr[q][0] = yin_code<FMT>(rowr[cxl]);
                rb = yin_code<FMT>(rowb[cxr]);
                rr = yin_code<FMT>(rowr[cxr]);
            }
            // the right neighbour stands behind the group's last block (a ragged group ends the row: its neighbour is that block again)
#pragma unroll
            for (int j = 1; j <= 4; ++j)
                if (j == nb) { cb[q][1 + j] = rb; cr[q][1 + j] = rr; }
        }
    }

    const double oy = a.k[0], iy = a.k[1], oc = a.k[2], ic = a.k[3], cr_r = a.k[4], cb_b = a.k[5], kr = a.k[6], kb = a.k[7], ikg = a.k[8];
    const bool w4 = (w & 3) == 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int f = !V2 ? 0 : r == 0 ? 0 : 2;                                // the far chroma row: above an even y, below an odd one
        alignas(16) float o[3][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int mb, mr;
            if constexpr (C444) {
                mb = 16 * cb[0][i];
                mr = 16 * cr[0][i];
            } else {
                const int c = 1 + (i >> 1);                                    // own block
                if (a.nearest) {
                    mb = 16 * cb[OWN][c];
                    mr = 16 * cr[OWN][c];
                } else if constexpr (V2 && !LEFT) {
                    // (written out: as 3 hs(own) + hs(far) below it costs a wave of occupancy, 93 -> 97 VGPRs for I420)
                    const int e = (i & 1) ? c + 1 : c - 1;                     // the neighbour on the pixel's side
                    mb = 9 * cb[1][c] + 3 * cb[f][c] + 3 * cb[1][e] + cb[f][e];
                    mr = 9 * cr[1][c] + 3 * cr[f][c] + 3 * cr[1][e] + cr[f][e];
                } else {
                    // the horizontal sum (of weight 4) of one chroma row
                    auto hs = [&](const int* row) {
                        if constexpr (LEFT) return (i & 1) ? 2 * row[c] + 2 * row[c + 1] : 4 * row[c];
                        else return 3 * row[c] + row[(i & 1) ? c + 1 : c - 1];
                    };
                    if constexpr (V2) {
                        mb = 3 * hs(cb[OWN]) + hs(cb[f]);
                        mr = 3 * hs(cr[OWN]) + hs(cr[f]);
                    } else {
                        mb = 4 * hs(cb[OWN]);
                        mr = 4 * hs(cr[OWN]);
                    }
                }
            }
            const double ey = ((double)yin_code<FMT>(yv[r][i]) - oy) * iy;
            const double ecb = ((double)mb * 0.0625 - oc) * ic;
            const double ecr = ((double)mr * 0.0625 - oc) * ic;
            const double R = ey + cr_r * ecr;
            const double B = ey + cb_b * ecb;
            const double G = ((ey - kr * R) - kb * B) * ikg;
            o[0][i] = (float)fmin(fmax(R, 0.0), 1.0);
            o[1][i] = (float)fmin(fmax(G, 0.0), 1.0);
            o[2][i] = (float)fmin(fmax(B, 0.0), 1.0);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* p = dst + c * hw + (size_t)(ROWS * by + r) * w + x0;
            if (n == 8 && w4) {
                reinterpret_cast<float4*>(p)[0] = reinterpret_cast<const float4*>(o[c])[0];
                reinterpret_cast<float4*>(p)[1] = reinterpret_cast<const float4*>(o[c])[1];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nb) reinterpret_cast<float2*>(p)[j] = reinterpret_cast<const float2*>(o[c])[j];
            }
        }
    }
}

extern "C" int refvsr_yuv420_in_max_frames(void) { return REFVSR_YUV420_IN_MAX_FRAMES; }

// The checked launch of both entries, `name` in front of its messages.  yuv_fmt is checked again where the 4:2:0 entry has always
// checked it: behind the geometry.
static int yuv_decode(const char* name, const void* const* src, float* const* dst, int nframes, int h, int w, int yuv_fmt, int sampling,
                      int siting, int chroma, const double* coef9, void* stream) {
    RV_CHECK(src && dst, "%s: null frame table", name);
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_YUV420_IN_MAX_FRAMES, "%s: 1..%d frames per launch", name, REFVSR_YUV420_IN_MAX_FRAMES);
    RV_CHECK(yuv_geometry_ok(h, w) && (long)h * w <= (1L << 29), "%s: h, w must be even and positive, h * w <= 2^29 (got %d x %d)", name, h, w);
    RV_CHECK(yuv_fmt_ok(yuv_fmt), "%s: unknown yuv format %d", name, yuv_fmt);
    RV_CHECK(chroma == REFVSR_YUV_CHROMA_BILINEAR || chroma == REFVSR_YUV_CHROMA_NEAREST,
             "%s: chroma must be REFVSR_YUV_CHROMA_BILINEAR | REFVSR_YUV_CHROMA_NEAREST (got %d)", name, chroma);
    RV_CHECK(coef9, "%s: null coefficients", name);
    YuvInArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(src[i] && dst[i], "%s: null pointer (frame %d)", name, i);
        RV_CHECK(((uintptr_t)src[i] & (yuv_sample_bytes(yuv_fmt) - 1)) == 0 && ((uintptr_t)dst[i] & 15) == 0,
                 "%s: source must be aligned to its samples, destination to 16 bytes (frame %d)", name, i);
        a.src[i] = src[i];
        a.dst[i] = dst[i];
    }
    a.h = h;
    a.w = w;
    a.gpr = (w + 7) / 8;
    a.gxb = (a.gpr + 63) / 64;
    a.nearest = chroma == REFVSR_YUV_CHROMA_NEAREST;
    for (int i = 0; i < 9; ++i) a.k[i] = coef9[i];
    const int hr = sampling == REFVSR_YUV_SAMPLING_420 ? h / 2 : h;           // rows (4:2:0: row pairs), four per workgroup
    const dim3 grid((unsigned)(a.gxb * ((hr + 3) / 4)), (unsigned)nframes), block(64, 4);
    hipStream_t st = (hipStream_t)stream;
    const bool left = siting == REFVSR_YUV_SITING_LEFT && sampling != REFVSR_YUV_SAMPLING_444;
#define YUV_IN_GO(F, S, L)                                                                        \
    if (yuv_fmt == REFVSR_YUV_##F && sampling == REFVSR_YUV_SAMPLING_##S && left == L)            \
        hipLaunchKernelGGL((yuv_in_kernel<REFVSR_YUV_##F, REFVSR_YUV_SAMPLING_##S, L>), grid, block, 0, st, a);
    YUV_INSTANCES(YUV_IN_GO)
#undef YUV_IN_GO
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_yuv420_to_rgb(const void* const* src, float* const* dst, int nframes, int h, int w, int format, int chroma,
                                    const double* coef, void* stream) {
    return yuv_decode("yuv420_to_rgb", src, dst, nframes, h, w, format, REFVSR_YUV_SAMPLING_420, REFVSR_YUV_SITING_CENTRE, chroma, coef, stream);
}

extern "C" int refvsr_yuv_to_rgb(const void* const* src, float* const* dst, int nframes, int h, int w, int yuv_fmt, int sampling,
                                 int siting, int chroma, const double* coef9, void* stream) {
    RV_CHECK(yuv_fmt_ok(yuv_fmt), "yuv_to_rgb: unknown yuv format %d", yuv_fmt);
    RV_CHECK(yuv_sampling_ok(sampling), "yuv_to_rgb: sampling must be REFVSR_YUV_SAMPLING_420 | _422 | _444 (got %d)", sampling);
    RV_CHECK(yuv_siting_ok(siting), "yuv_to_rgb: siting must be REFVSR_YUV_SITING_CENTRE | REFVSR_YUV_SITING_LEFT (got %d)", siting);
    RV_CHECK(sampling == REFVSR_YUV_SAMPLING_420 || !yuv_semi(yuv_fmt),
             "yuv_to_rgb: semi-planar frames (NV12, P010) are 4:2:0 only (format %d, sampling %d)", yuv_fmt, sampling);
    // (4:2:0 / centre answers in the 4:2:0 entry's name)
    const bool plain = sampling == REFVSR_YUV_SAMPLING_420 && siting == REFVSR_YUV_SITING_CENTRE;
    return yuv_decode(plain ? "yuv420_to_rgb" : "yuv_to_rgb", src, dst, nframes, h, w, yuv_fmt, sampling, siting, chroma, coef9, stream);
}
