// Antialiased separable bicubic resize of RGB frames (extension: the reference ships its LRx4 folders ready-made -- configs/config.py:
// 120-152 reads them -- and leaves the resize of a result to its consumer, behind evaluation/eval_qual_quan.py:117-119).
// refvsr_resize_aa resamples up to REFVSR_RESIZE_MAX_FRAMES frames of one geometry -- any of the six forms the other frame kernels take,
// float32 | float16 | uint8, planar or interleaved -- to planar float32 or uint8 frames of another size in one launch.
//
// Exactness: the kernel returns the bits of refvsr_amd/resize.py:resize_aa_model.  The taps (first source index, count, normalised
// float64 weights per output row and column) come from the host (resize.py:aa_taps); the device computes no weight.  Everything is
// float64 with every operation rounded on its own: contraction is OFF for this file.  A byte is the float32 of ingest_table.h, widened.
//
// Shape: a workgroup owns a RS_TH x RS_TW output tile of one channel of one frame.  Its four waves walk the source rows the tile's taps
// reach, RS_RPW rows per wave and step: a wave stages its rows' segments (the columns the tile's taps reach) into its own LDS strips
// as float32, with lane-consecutive loads, and then forms the rows' RS_TW horizontal sums from the strips -- lane = column, a run-time
// loop over that column's taps, the rows as independent chains -- into the tile's T buffer in LDS, float64, never rounded.  The
// vertical pass reads T: lane = column, so the 8-byte LDS accesses of a wave are 64 consecutive doubles (no bank conflict), a wave's
// four output rows together; the strip reads of the horizontal pass step by the ratio and do conflict, on 4-byte words.  There is no intermediate in global memory, and a source sample is fetched only by the
// workgroups whose tile or halo holds it.  LDS: span_y x RS_TW x 8 bytes of T (ratio 4: 78 rows, 40 KB; ratio 8: 154 rows, 79 KB) + sixteen
// strips (18 KB, 34 KB) + the tile's weights (9 KB, 21 KB), sized per launch from the ratio; dynamic, up to the 160 KiB of a CU.
// The three channel workgroups of a tile are eight apart in blockIdx.x: the same XCD (observed placement, used for speed only), so
// an interleaved source's lines are fetched into one L2 once.
// The tables are device memory the host cannot check: every index they yield is clamped into the staged rows and columns, so a wrong
// table gives wrong samples, never an access outside the buffers.  Plain vector stores only.
#pragma clang fp contract(off)
#include "common.h"
#include "ingest_table.h"

#define RS_TH 16
#define RS_TW 64
#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / 64)
#define RS_RPW 4                       // source rows per wave and step of the horizontal pass
#define RS_MAX_RATIO 8
#define RS_MAX_TAPS 33

__constant__ IngestTable kResizeTable = ingest_table();

struct ResizeArgs {
    const void* src[REFVSR_RESIZE_MAX_FRAMES];
    void* dst[REFVSR_RESIZE_MAX_FRAMES];
    const int* lo_x; const int* cnt_x; const double* wx;
    const int* lo_y; const int* cnt_y; const double* wy;
    int h, w, oh, ow;
    int maxcnt_x, maxcnt_y;
    int span_x, span_y;          // columns per strip, rows of T: what the launch's LDS holds
    int ntx, ntiles;
    int clamp;
};

template <typename T>
__device__ __forceinline__ float rs_value(T v) {
    if constexpr (std::is_same<T, unsigned char>::value) return kResizeTable.v[v];
    else return (float)v;
}

template <typename T, bool HWC, typename D>
__global__ void __launch_bounds__(RS_THREADS) resize_aa_kernel(ResizeArgs a) {
    extern __shared__ double rs_lds[];
    const int b = (int)blockIdx.x;
    const int q = b >> 3;
    const int c = q % 3;
    const int tile = (q / 3) * 8 + (b & 7);
    if (tile >= a.ntiles) return;                                    // (whole workgroups: nothing below is reached by a part of one)
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = a.h, w = a.w, oh = a.oh, ow = a.ow;
    const int ty0 = (tile / a.ntx) * RS_TH, tx0 = (tile % a.ntx) * RS_TW;
    const int th = min(RS_TH, oh - ty0), tw = min(RS_TW, ow - tx0);
    const T* __restrict__ src = reinterpret_cast<const T*>(a.src[blockIdx.y]);
    D* __restrict__ dst = reinterpret_cast<D*>(a.dst[blockIdx.y]);

    // the source rows and columns the tile's taps reach: lo and lo + cnt do not decrease along an axis, so the first output's lo and
    // the last one's end bound them all
    const int r0 = min(max(a.lo_y[ty0], 0), h - 1);
    const int nrows = min(min(max(a.lo_y[ty0 + th - 1] + a.cnt_y[ty0 + th - 1], r0 + 1), h) - r0, a.span_y);
    const int c0 = min(max(a.lo_x[tx0], 0), w - 1);
    const int ncols = min(min(max(a.lo_x[tx0 + tw - 1] + a.cnt_x[tx0 + tw - 1], c0 + 1), w) - c0, a.span_x);

    double* const tbuf = rs_lds;                                     // [span_y][RS_TW]
    double* const wxl = tbuf + (size_t)a.span_y * RS_TW;             // [maxcnt_x][RS_TW]: tap k of the tile's column j at [k][j]
    double* const wyl = wxl + (size_t)a.maxcnt_x * RS_TW;            // [RS_TH][maxcnt_y]: the tile's rows of wy
    float* const strip = reinterpret_cast<float*>(wyl + (size_t)RS_TH * a.maxcnt_y) + (size_t)wave * RS_RPW * a.span_x;      // [RS_RPW][span_x]

    // the tile's weights, once, with consecutive loads (read from global memory inside the tap loops: 1.1 .. 1.2 x the kernel's time,
    // measured); wxl transposed, so that a wave reads a tap as 64 consecutive doubles.  The first
    // barrier of the row loop stands between these stores and their first use
    for (int e = tid; e < tw * a.maxcnt_x; e += RS_THREADS) {
        const int j = e / a.maxcnt_x, k = e - j * a.maxcnt_x;
        wxl[k * RS_TW + j] = a.wx[(size_t)tx0 * a.maxcnt_x + e];
    }
    for (int e = tid; e < th * a.maxcnt_y; e += RS_THREADS) wyl[e] = a.wy[(size_t)ty0 * a.maxcnt_y + e];

    // this lane's column of the horizontal pass
    const bool col = lane < tw;
    int xlo = 0, xcnt = 1;
    const double* const xw = wxl + lane;                             // tap k at xw[k * RS_TW]
    if (col) {
        xlo = a.lo_x[tx0 + lane] - c0;
        xcnt = min(max(a.cnt_x[tx0 + lane], 1), a.maxcnt_x);
    }

    // RS_RPW rows per wave and step: their loads are in flight together, a tap's weight is loaded once for all of them, and the rows'
    // sums are independent chains (one row per wave and step: 1.7 x the time at 1080p -> 270p, 1.2 x at 8K -> 4K, measured)
    for (int rb = 0; rb < nrows; rb += RS_WAVES * RS_RPW) {          // (nrows is the workgroup's: every wave meets every barrier)
        const int rw = rb + wave * RS_RPW;                           // this wave's first row of the step
#pragma unroll
        for (int q = 0; q < RS_RPW; ++q) {
            if (rw + q < nrows) {
                const size_t row = HWC ? ((size_t)(r0 + rw + q) * w + c0) * 3 + c : ((size_t)c * h + (r0 + rw + q)) * w + c0;
                for (int i = lane; i < ncols; i += 64) strip[q * a.span_x + i] = rs_value(src[HWC ? row + 3 * (size_t)i : row + i]);
            }
        }
        __syncthreads();
        if (rw < nrows && col) {                                     // (rows past nrows: stale strip values, summed and not stored)
            double acc[RS_RPW];
            const int s0 = min(max(xlo, 0), ncols - 1);
            const double w0 = xw[0];
#pragma unroll
            for (int q = 0; q < RS_RPW; ++q) acc[q] = w0 * (double)strip[q * a.span_x + s0];
            for (int k = 1; k < xcnt; ++k) {
                const int sk = min(max(xlo + k, 0), ncols - 1);
                const double wk = xw[k * RS_TW];
#pragma unroll
                for (int q = 0; q < RS_RPW; ++q) acc[q] = acc[q] + wk * (double)strip[q * a.span_x + sk];
            }
#pragma unroll
            for (int q = 0; q < RS_RPW; ++q)
                if (rw + q < nrows) tbuf[(rw + q) * RS_TW + lane] = acc[q];
        }
        __syncthreads();
    }

    if (!col) return;
    // the vertical pass: a wave's RS_TH / RS_WAVES output rows together, each its own chain; a row whose taps have run out keeps its sum
    constexpr int NV = RS_TH / RS_WAVES;
    int ylo[NV], ycnt[NV], kmax = 1;
    const double* yw[NV];
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int li = min(wave + q * RS_WAVES, th - 1);             // (a row past the tile repeats its last one and is not stored)
        ylo[q] = a.lo_y[ty0 + li] - r0;
        ycnt[q] = min(max(a.cnt_y[ty0 + li], 1), a.maxcnt_y);
        yw[q] = wyl + li * a.maxcnt_y;
        kmax = max(kmax, ycnt[q]);
        acc[q] = yw[q][0] * tbuf[min(max(ylo[q], 0), nrows - 1) * RS_TW + lane];
    }
    for (int k = 1; k < kmax; ++k) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const double v = acc[q] + yw[q][k] * tbuf[min(max(ylo[q] + k, 0), nrows - 1) * RS_TW + lane];
            acc[q] = k < ycnt[q] ? v : acc[q];
        }
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int oy = ty0 + wave + q * RS_WAVES;
        if (oy >= oh) continue;
        const size_t e = ((size_t)c * oh + oy) * ow + tx0 + lane;
        if constexpr (std::is_same<D, float>::value) {
            dst[e] = (float)(a.clamp ? fmin(fmax(acc[q], 0.0), 1.0) : acc[q]);            // one rounding
        } else {
            dst[e] = (unsigned char)(int)rint(255.0 * fmin(fmax(acc[q], 0.0), 1.0));      // rint: half to even
        }
    }
}

extern "C" int refvsr_resize_max_frames(void) { return REFVSR_RESIZE_MAX_FRAMES; }

// rows (columns) of the source the taps of `tile` consecutive outputs reach, at most: lo > c - support - 0.5 of the first output and
// lo + cnt <= c + support + 0.5 of the last are less than (tile - 1) scale + 2 support + 1 apart (resize.py:aa_taps)
static int rs_span(int n_in, int n_out, int tile) {
    const double scale = (double)n_in / (double)n_out;
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
    const long s = (long)ceil((double)(tile - 1) * scale + 2.0 * support + 1.0) + 1;
    return (int)(s < n_in ? s : n_in);
}

template <typename T, bool HWC, typename D>
static int rs_launch(const ResizeArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    static RvLaunchCap cap;
    const int rc = rv_launch_cap(cap, resize_aa_kernel<T, HWC, D>, RS_THREADS, 160 * 1024, lds, st, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL((resize_aa_kernel<T, HWC, D>), grid, dim3(RS_THREADS), lds, st, a);
    RV_LAUNCH_CHECK();
    return 0;
}

template <typename T, bool HWC>
static int rs_launch_dst(int dst_fmt, const ResizeArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    return dst_fmt == REFVSR_RESULT_F32 ? rs_launch<T, HWC, float>(a, grid, lds, st) : rs_launch<T, HWC, unsigned char>(a, grid, lds, st);
}

extern "C" int refvsr_resize_aa(const void* const* src, int src_fmt, void* const* dst, int dst_fmt, int nframes, int h, int w, int oh,
                                int ow, const int32_t* lo_x, const int32_t* cnt_x, const double* wx, const int32_t* lo_y,
                                const int32_t* cnt_y, const double* wy, int maxcnt_x, int maxcnt_y, int clamp, void* stream) {
    RV_CHECK(src && dst, "resize_aa: null frame table");
    RV_CHECK(lo_x && cnt_x && wx && lo_y && cnt_y && wy, "resize_aa: null tap table");
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_RESIZE_MAX_FRAMES, "resize_aa: 1..%d frames per launch", REFVSR_RESIZE_MAX_FRAMES);
    RV_CHECK(rv_result_fmt_ok(src_fmt), "resize_aa: unknown source format %d", src_fmt);
    RV_CHECK(dst_fmt == REFVSR_RESULT_F32 || dst_fmt == REFVSR_RESULT_U8,
             "resize_aa: the destination is planar REFVSR_RESULT_F32 or REFVSR_RESULT_U8 (got %d)", dst_fmt);
    RV_CHECK(h >= 1 && w >= 1 && oh >= 1 && ow >= 1, "resize_aa: sizes must be positive (got %d x %d -> %d x %d)", h, w, oh, ow);
    RV_CHECK((long long)h <= (long long)RS_MAX_RATIO * oh && (long long)w <= (long long)RS_MAX_RATIO * ow,
             "resize_aa: the down-scale ratio is at most %d per axis (got %d x %d -> %d x %d)", RS_MAX_RATIO, h, w, oh, ow);
    RV_CHECK(clamp == 0 || clamp == 1, "resize_aa: clamp must be 0 or 1 (got %d)", clamp);
    const size_t es = rv_result_sample_bytes(src_fmt), ds = rv_result_sample_bytes(dst_fmt);
    RV_CHECK((long long)h * w * 3 * (long long)es < (1ll << 31) && (long long)oh * ow * 3 * (long long)ds < (1ll << 31),
             "resize_aa: frame too large for 32-bit offsets");
    // a column's (row's) taps: at least one, at most 2 support + 1 of the axis -- what resize.py:aa_taps makes -- and never more than
    // the table's row holds
    const int span1_x = rs_span(w, ow, 1), span1_y = rs_span(h, oh, 1);
    RV_CHECK(maxcnt_x >= 1 && maxcnt_x <= RS_MAX_TAPS && maxcnt_x <= span1_x && maxcnt_y >= 1 && maxcnt_y <= RS_MAX_TAPS && maxcnt_y <= span1_y,
             "resize_aa: cnt exceeds maxcnt: maxcnt_x, maxcnt_y must lie in 1..%d and 1..%d for these sizes (got %d, %d)",
             span1_x < RS_MAX_TAPS ? span1_x : RS_MAX_TAPS, span1_y < RS_MAX_TAPS ? span1_y : RS_MAX_TAPS, maxcnt_x, maxcnt_y);
    RV_CHECK((((uintptr_t)lo_x | (uintptr_t)cnt_x | (uintptr_t)lo_y | (uintptr_t)cnt_y) & 3) == 0 && (((uintptr_t)wx | (uintptr_t)wy) & 7) == 0,
             "resize_aa: tap tables must be aligned to their elements");
    ResizeArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = rv_frame_tables("resize_aa", src, dst, nframes, es, ds, (size_t)h * w * 3 * es, (size_t)oh * ow * 3 * ds, a.src, a.dst);
    if (rc) return rc;
    a.lo_x = lo_x; a.cnt_x = cnt_x; a.wx = wx;
    a.lo_y = lo_y; a.cnt_y = cnt_y; a.wy = wy;
    a.h = h; a.w = w; a.oh = oh; a.ow = ow;
    a.maxcnt_x = maxcnt_x; a.maxcnt_y = maxcnt_y;
    a.span_x = rs_span(w, ow, RS_TW);
    a.span_y = rs_span(h, oh, RS_TH);
    a.ntx = (ow + RS_TW - 1) / RS_TW;
    const long ntiles = (long)a.ntx * ((oh + RS_TH - 1) / RS_TH);
    RV_CHECK(ntiles < (1l << 24), "resize_aa: too many tiles");
    a.ntiles = (int)ntiles;
    a.clamp = clamp;
    const size_t lds = (size_t)a.span_y * RS_TW * sizeof(double) + (size_t)RS_WAVES * RS_RPW * a.span_x * sizeof(float) +
                       ((size_t)maxcnt_x * RS_TW + (size_t)RS_TH * maxcnt_y) * sizeof(double);
    RV_CHECK(lds <= 160 * 1024, "resize_aa: tile does not fit the LDS (%zu bytes)", lds);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((ntiles + 7) / 8) * 8 * 3), (unsigned)nframes);
    return rv_result_dispatch(src_fmt, [&](auto t, auto hwc) {
        return rs_launch_dst<typename decltype(t)::type, decltype(hwc)::value>(dst_fmt, a, grid, lds, st);
    });
}
