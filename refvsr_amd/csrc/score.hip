// Frame scores on the device: the mean squared error and the SSIM of up to REFVSR_SCORE_MAX_FRAMES (result, ground truth) pairs of one
// 3 x h x w geometry in one launch (+ one tiny launch that sums the workgroups' partial sums), so that an evaluation loop moves 16 bytes
// per frame to the host instead of the frame.  Replaces trainers/trainer.py:252-254 (PSNR = 10 log10(1 / mse); the log stays on the
// host) and evaluation/metrics.py:17-18 (skimage.metrics.structural_similarity defaults: 7 x 7 uniform window over the valid positions,
// sample covariance, K1 = 0.01, K2 = 0.03, data range 1, mean over channels), as evalrun.psnr / evalrun.ssim restate them.
//
// Arithmetic: float64 throughout, on the float32 value of every input sample (fp16 widened exactly, a byte u through the ingest table
// T[u] = (float)((double)u / 255.0), ingest_table.h).  The products a a, b b, a b of two float32 values are exact in float64; contraction
// is switched off for the whole file, so the sums below are the written ones, in the written order.
//
// Tile: one workgroup (256 threads = 4 waves) scores the 32 x 64 window origins of one tile of one channel from a 38 x 70 input tile
// (halo factor 38 * 70 / (32 * 64) = 1.30: every sample is read from global memory once plus halo) staged in LDS as float32
// (2 x 10 640 B + 1 KB table + 2 KB reduction = 24 352 B per workgroup: six workgroups per CU by LDS, four by registers).  Lane = column, wave = 8 output rows:
// a thread forms the five horizontal 7-tap sums (a, b, a a, b b, a b) of the 14 input rows it needs as DIRECT 7-term sums left to
// right, keeps the last seven rows in registers, and sums those top to bottom for every output row -- no running add-subtract window
// anywhere, so the rounding error of a window does not depend on the image size.  Wave-wide LDS reads are 64 consecutive floats
// (ds_read_b32, conflict free for any row pitch).
// Loads are one element per lane (4-, 2- or 1-byte, consecutive lanes on consecutive samples of a tile row; an interleaved ground truth
// at a 3-byte stride, an interleaved result -- out_fmt | REFVSR_RESULT_HWC -- at a stride of three samples: the staging index alone
// differs, so the scores are the planar frame's bits), so pointers only need the natural alignment of their element type: fp32 4 bytes, fp16 2 bytes, bytes none.
//
// MSE: every sample belongs to exactly one tile (the last tile of a row / column of tiles owns its 6 halo columns / rows); the thread
// that stages it adds (a - b)^2 to its own float64 sum.
// Reduction (deterministic, no floating-point atomics): per workgroup a fixed LDS tree over the 256 threads, the two sums go to
// workspace[frame][channel][tile] with a plain vector store; score_finish_kernel (one workgroup per frame) sums a frame's partial sums
// in a fixed strided order + the same tree and divides by the counts.  A frame's bits therefore do not depend on the other frames of
// the launch, on the stream or on the run.  refvsr_amd/metrics.py:score_frames_model restates the decomposition and the order in numpy.
//
//
// Down-scaled scoring (refvsr_score_frames_down, the flag_HD_in configs whose result is `down` = 2 | 4 times the ground truth): the
// kernel is a template on DOWN.  DOWN = 1 is the kernel described above, statement for statement.  DOWN > 1 differs in the staging
// alone: the thread that stages element (y, x) of the 38 x 70 tile forms D(y, x), the bicubic down-scale of the big result frame
// [3][DOWN h][DOWN w] that models/loss/Loss.py:91-92 (F.interpolate(sr, scale_factor = 1 / scale, mode = 'bicubic', align_corners =
// False)) and evaluation/eval_qual_quan.py:85-92 (cv2.resize(.., fx = fy = 1 / scale, INTER_CUBIC)) compute: at an exact integer factor
// both are Keys' cubic with A = -0.75 at half-pixel centres without anti-aliasing, whose source coordinate DOWN x + DOWN / 2 - 1 / 2
// has the fraction 1 / 2 -- four taps i0 .. i0 + 3, i0 = DOWN x + DOWN / 2 - 2, clamped into the frame, with the weights (-3, 19, 19,
// -3) / 32, exact in binary.  float64 on the float32 value of every tap: the products are exact, a row's four are added left to right,
// the four row sums weighted and added top to bottom, and D is rounded ONCE to float32 (the reference's float32 image, correctly
// rounded; refvsr_amd/metrics.py:down_bicubic_model).  ta holds (float)D -- the SSIM is that of the unclamped image (eval_qual_quan.py
// does not clamp) -- and the owned samples add (clamp01(D) - b)^2 (Loss.py:92 clamps before get_psnr, :141).  Everything after the
// staging is the same code, so the summation order and the determinism are the ones above, and the scores are bit for bit those of
// DOWN = 1 on the uploaded D / clamp01(D).  Every index into the big frame is size_t.  Taps are loaded element by element (natural
// alignment); for DOWN = 4, where a row's four taps 4 x .. 4 x + 3 are one aligned group of four, as ONE 16- / 8- / 4-byte load when
// the entry point has seen every result pointer aligned to four samples (ScoreArgs::avec; the same values, hence the same bits).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the figures next to score_tile_kernel;
// score_finish_kernel: 14 VGPRs, 2 KB LDS, no scratch.
#include "common.h"
#include "ingest_table.h"

#pragma clang fp contract(off)

#define SC_TH 32                       // window origins per tile
#define SC_TW 64
#define SC_IH (SC_TH + 6)              // input rows / columns per tile
#define SC_IW (SC_TW + 6)
#define SC_ROWS 8                      // output rows per thread (SC_TH / 4 waves)
#define SC_THREADS 256

__constant__ IngestTable kScoreTable = ingest_table();

enum { SC_GT_F32 = 0, SC_GT_U8_PLANAR = 1, SC_GT_U8_HWC = 2 };

struct ScoreArgs {
    const void* a[REFVSR_SCORE_MAX_FRAMES];
    const void* b[REFVSR_SCORE_MAX_FRAMES];
    double* part;                      // [nframes][3][nty * ntx][2] partial sums {sum (a - b)^2, sum ssim}
    int h, w, ntx, nty;
    int afmt;                          // REFVSR_RESULT_* (the sample format alone)
    int ahwc;                          // results are interleaved [h][w][3] (REFVSR_RESULT_HWC)
    int bkind;                         // SC_GT_*
    int win;                           // 7 | 0
    int avec;                          // DOWN = 4: every result pointer is aligned to four samples (one load per tap row)
};

static inline int sc_tiles(int n, int t) { return (n - 6 + t - 1) / t; }    // tiles over n - 6 window origins

// fixed-order sum of one double per thread; the result is valid in thread 0
__device__ __forceinline__ double sc_block_sum(double* red, const int tid, const double v) {
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = SC_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// D(y, x) of result plane c, rounded once to float32: the bicubic down-scale by DOWN = 2 | 4 of the big frame [3][DOWN h][DOWN w] at
// ground-truth position (y, x) (the file header).  avec (DOWN = 4 only): one load per tap row
template <int DOWN>
__device__ __forceinline__ float sc_down_sample(const unsigned char* __restrict__ pa, const float* tbl, const int afmt, const int avec, const int ahwc,
                                                const int c, const int y, const int x, const int h, const int w) {
    static_assert(DOWN == 2 || DOWN == 4, "integer factors whose source coordinate has the fraction 1 / 2");
    constexpr double W0 = -3.0 / 32.0, W1 = 19.0 / 32.0;
    const int bh = DOWN * h, bw = DOWN * w;                       // (h w <= 2^29 and h, w >= 7: both fit an int)
    const int i0y = DOWN * y + DOWN / 2 - 2, i0x = DOWN * x + DOWN / 2 - 2;
    int xi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xi[k] = DOWN == 4 ? i0x + k : min(max(i0x + k, 0), bw - 1);      // DOWN = 4: 4 x .. 4 x + 3, inside
    double rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = DOWN == 4 ? i0y + j : min(max(i0y + j, 0), bh - 1);
        // planar [3][bh][bw]: element row + x; interleaved [bh][bw][3]: element row + 3 x (avec is off: a tap row is not one group)
        const size_t row = ahwc ? (size_t)yy * (size_t)bw * 3 + (size_t)c : ((size_t)c * bh + yy) * (size_t)bw;
        const size_t xs = ahwc ? 3 : 1;
        float t[4];
        if (DOWN == 4 && avec) {                                  // row + xi[0] is a multiple of 4 samples, the pointer of 4 samples
            const size_t i4 = (row + (size_t)xi[0]) >> 2;
            if (afmt == REFVSR_RESULT_F32) {
                const f32x4 v = reinterpret_cast<const f32x4*>(pa)[i4];
                t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
            } else if (afmt == REFVSR_RESULT_F16) {
                const f16x4 v = reinterpret_cast<const f16x4*>(pa)[i4];
                t[0] = (float)v[0]; t[1] = (float)v[1]; t[2] = (float)v[2]; t[3] = (float)v[3];
            } else {
                const unsigned v = reinterpret_cast<const unsigned*>(pa)[i4];
                t[0] = tbl[v & 255u]; t[1] = tbl[(v >> 8) & 255u]; t[2] = tbl[(v >> 16) & 255u]; t[3] = tbl[v >> 24];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t ip = row + xs * (size_t)xi[k];
                if (afmt == REFVSR_RESULT_F32) t[k] = reinterpret_cast<const float*>(pa)[ip];
                else if (afmt == REFVSR_RESULT_F16) t[k] = (float)reinterpret_cast<const f16*>(pa)[ip];
                else t[k] = tbl[pa[ip]];
            }
        }
        double acc = W0 * (double)t[0] + W1 * (double)t[1];       // exact products, added left to right
        acc = acc + W1 * (double)t[2];
        acc = acc + W0 * (double)t[3];
        rs[j] = acc;
    }
    double d = W0 * rs[0] + W1 * rs[1];                           // the four row sums, top to bottom
    d = d + W1 * rs[2];
    d = d + W0 * rs[3];
    return (float)d;
}

// score_tile_kernel<1>: 104 VGPRs, 47 SGPRs, no scratch, no spills, 24 352 B LDS, 4 waves per SIMD by registers (figures of the build
// this file was written against -- re-check with -Rpass-analysis=kernel-resource-usage after a change; re-checked when the kernel
// became a template: the same figures as before it).  score_tile_kernel<2>: 104 VGPRs, 59 SGPRs; score_tile_kernel<4>: 104 VGPRs,
// 61 SGPRs (re-checked with the interleaved result layout: 4-6 SGPRs more, nothing else moved); both no scratch, 24 352 B LDS, 4 waves per SIMD -- the sixteen taps live only in the staging loop, before the row ring
template <int DOWN>
__global__ void __launch_bounds__(SC_THREADS) score_tile_kernel(ScoreArgs s) {
    __shared__ float tbl[256];
    __shared__ float ta[SC_IH * SC_IW], tb[SC_IH * SC_IW];
    __shared__ double red[SC_THREADS];
    const int tid = (int)threadIdx.x;
    const int tile = (int)blockIdx.x, c = (int)blockIdx.y, f = (int)blockIdx.z;
    const int ty = tile / s.ntx, tx = tile - ty * s.ntx;
    const int y0 = ty * SC_TH, x0 = tx * SC_TW;
    const int h = s.h, w = s.w;
    tbl[tid] = kScoreTable.v[tid];
    __syncthreads();

    // ---- stage the tile, sum (a - b)^2 over the samples this tile owns
    const int own_h = ty == s.nty - 1 ? h - y0 : SC_TH;          // <= SC_IH
    const int own_w = tx == s.ntx - 1 ? w - x0 : SC_TW;          // <= SC_IW
    const unsigned char* __restrict__ pa = (const unsigned char*)s.a[f];
    const unsigned char* __restrict__ pb = (const unsigned char*)s.b[f];
    double mse = 0.0;
    for (int e = tid; e < SC_IH * SC_IW; e += SC_THREADS) {
        const int r = e / SC_IW, q = e - r * SC_IW;
        const int y = y0 + r, x = x0 + q;
        float va = 0.0f, vb = 0.0f;
        if (y < h && x < w) {
            const size_t ip = ((size_t)c * h + y) * w + x;       // planar [3][h][w]
            if constexpr (DOWN == 1) {
                const size_t ia = s.ahwc ? ((size_t)y * w + x) * 3 + c : ip;     // interleaved [h][w][3] result
                if (s.afmt == REFVSR_RESULT_F32) va = reinterpret_cast<const float*>(pa)[ia];
                else if (s.afmt == REFVSR_RESULT_F16) va = (float)reinterpret_cast<const f16*>(pa)[ia];
                else va = tbl[pa[ia]];
            } else {
                va = sc_down_sample<DOWN>(pa, tbl, s.afmt, s.avec, s.ahwc, c, y, x, h, w);
            }
            if (s.bkind == SC_GT_F32) vb = reinterpret_cast<const float*>(pb)[ip];
            else if (s.bkind == SC_GT_U8_PLANAR) vb = tbl[pb[ip]];
            else vb = tbl[pb[((size_t)y * w + x) * 3 + c]];      // interleaved [h][w][3]
            if (r < own_h && q < own_w) {
                const double d = (double)(DOWN == 1 ? va : fminf(fmaxf(va, 0.0f), 1.0f)) - (double)vb;
                mse = mse + d * d;
            }
        }
        ta[e] = va;
        tb[e] = vb;
    }
    __syncthreads();

    // ---- SSIM of the window origins (y0 + 8 wave + o, x0 + lane)
    double ss = 0.0;
    if (s.win) {
        const int col = tid & 63, rg = tid >> 6;
        const bool col_ok = x0 + col <= w - 7;
        constexpr double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
        constexpr double norm = 49.0 / 48.0;
        double hs[7][5];                                          // horizontal sums of the last seven input rows (static indices)
#pragma unroll
        for (int i = 0; i < SC_ROWS + 6; ++i) {
            const float* ra = ta + (rg * SC_ROWS + i) * SC_IW + col;
            const float* rb = tb + (rg * SC_ROWS + i) * SC_IW + col;
            double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const double a = (double)ra[k], b = (double)rb[k];
                sa = sa + a;
                sb = sb + b;
                saa = saa + a * a;
                sbb = sbb + b * b;
                sab = sab + a * b;
            }
            double* hrow = hs[i % 7];
            hrow[0] = sa; hrow[1] = sb; hrow[2] = saa; hrow[3] = sbb; hrow[4] = sab;
            if (i >= 6) {
                double t[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    double acc = hs[(i - 6) % 7][j];
#pragma unroll
                    for (int k = 5; k >= 0; --k) acc = acc + hs[(i - k) % 7][j];
                    t[j] = acc;
                }
                const double ua = t[0] / 49.0, ub = t[1] / 49.0;
                const double va = norm * (t[2] / 49.0 - ua * ua);
                const double vb = norm * (t[3] / 49.0 - ub * ub);
                const double vab = norm * (t[4] / 49.0 - ua * ub);
                const double num = (2.0 * ua * ub + c1) * (2.0 * vab + c2);
                const double den = (ua * ua + ub * ub + c1) * (va + vb + c2);
                const int oy = y0 + rg * SC_ROWS + (i - 6);
                if (col_ok && oy <= h - 7) ss = ss + num / den;
            }
        }
    }

    const double m_all = sc_block_sum(red, tid, mse);
    __syncthreads();
    const double s_all = sc_block_sum(red, tid, ss);
    if (tid == 0) {
        const size_t nt = (size_t)s.ntx * s.nty;
        *reinterpret_cast<double2*>(s.part + (((size_t)f * 3 + c) * nt + tile) * 2) = make_double2(m_all, s_all);
    }
}

// one workgroup per frame: the frame's n = 3 nty ntx partial sums -> {mse, ssim}
__global__ void __launch_bounds__(SC_THREADS) score_finish_kernel(const double* __restrict__ part, int n, int h, int w, int win,
                                                                  double* __restrict__ scores) {
    __shared__ double red[SC_THREADS];
    const int tid = (int)threadIdx.x, f = (int)blockIdx.x;
    const double* p = part + (size_t)f * n * 2;
    double m = 0.0, ss = 0.0;
    for (int i = tid; i < n; i += SC_THREADS) {
        m = m + p[2 * i];
        ss = ss + p[2 * i + 1];
    }
    const double m_all = sc_block_sum(red, tid, m);
    __syncthreads();
    const double s_all = sc_block_sum(red, tid, ss);
    if (tid == 0) {
        const double ns = 3.0 * (double)h * (double)w, nw = 3.0 * (double)(h - 6) * (double)(w - 6);
        *reinterpret_cast<double2*>(scores + 2 * (size_t)f) = make_double2(m_all / ns, win ? s_all / nw : 0.0);
    }
}

static bool sc_geometry_ok(int h, int w) { return h >= 7 && w >= 7 && (long)h * w <= (1L << 29); }

extern "C" int refvsr_score_max_frames(void) { return REFVSR_SCORE_MAX_FRAMES; }

extern "C" size_t refvsr_score_workspace_bytes(int nframes, int h, int w) {
    if (nframes < 1 || !sc_geometry_ok(h, w)) return 0;
    return (size_t)nframes * 3 * sc_tiles(h, SC_TH) * sc_tiles(w, SC_TW) * 2 * sizeof(double);
}

// What every scoring entry point checks of its frames, and the frame table of its argument struct (ScoreArgs | RegionArgs: a, b, afmt,
// ahwc, bkind).  `who` names the caller in the messages, `res` its result array ("scores" | "sums"), `needed` its workspace size;
// own_checks() holds the caller's own arguments and runs where they always have: behind the geometry, ahead of the formats.
template <typename Args, typename OwnChecks>
static int sc_frames(const char* who, const char* res, Args& a, const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout,
                     int nframes, int h, int w, OwnChecks own_checks, const void* workspace, size_t workspace_bytes, size_t needed,
                     const void* results) {
    RV_CHECK(out && gt, "%s: null frame table", who);
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_SCORE_MAX_FRAMES, "%s: 1..%d frames per launch", who, REFVSR_SCORE_MAX_FRAMES);
    RV_CHECK(sc_geometry_ok(h, w), "%s: h, w must be at least 7 (the SSIM window) and h * w at most 2^29", who);
    if (int rc = own_checks()) return rc;
    RV_CHECK(rv_result_fmt_ok(out_fmt), "%s: unknown result format %d (REFVSR_RESULT_F32 | _F16 | _U8, optionally | REFVSR_RESULT_HWC)", who, out_fmt);
    const int ahwc = (out_fmt & REFVSR_RESULT_HWC) != 0;
    out_fmt &= REFVSR_RESULT_FMT_MASK;
    RV_CHECK(gt_fmt == REFVSR_RESULT_F32 || gt_fmt == REFVSR_RESULT_U8, "%s: ground-truth format must be REFVSR_RESULT_F32 | _U8", who);
    RV_CHECK(gt_layout == REFVSR_INGEST_PLANAR || gt_layout == REFVSR_INGEST_HWC,
             "%s: ground-truth layout must be REFVSR_INGEST_PLANAR | REFVSR_INGEST_HWC", who);
    RV_CHECK(!(gt_fmt == REFVSR_RESULT_F32 && gt_layout == REFVSR_INGEST_HWC), "%s: the interleaved layout is for uint8 ground truth", who);
    RV_CHECK(workspace && results, "%s: null workspace / %s", who, res);
    RV_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)results & 15) == 0, "%s: workspace and %s must be 16-byte aligned", who, res);
    RV_CHECK(workspace_bytes >= needed, "%s: workspace too small (%zu bytes, %zu needed)", who, workspace_bytes, needed);
    memset(&a, 0, sizeof(a));
    const uintptr_t amask = out_fmt == REFVSR_RESULT_F32 ? 3 : out_fmt == REFVSR_RESULT_F16 ? 1 : 0;
    const uintptr_t bmask = gt_fmt == REFVSR_RESULT_F32 ? 3 : 0;
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(out[i] && gt[i], "%s: null pointer (frame %d)", who, i);
        RV_CHECK(((uintptr_t)out[i] & amask) == 0 && ((uintptr_t)gt[i] & bmask) == 0,
                 "%s: fp32 frames must be 4-byte, fp16 frames 2-byte aligned (frame %d)", who, i);
        a.a[i] = out[i];
        a.b[i] = gt[i];
    }
    a.afmt = out_fmt; a.ahwc = ahwc;
    a.bkind = gt_fmt == REFVSR_RESULT_F32 ? SC_GT_F32 : gt_layout == REFVSR_INGEST_PLANAR ? SC_GT_U8_PLANAR : SC_GT_U8_HWC;
    return 0;
}

// the two entry points' launches; `who` names the caller in the messages, down = 1 | 2 | 4
static int sc_run(const char* who, const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes, int h, int w,
                  int down, int win, void* workspace, size_t workspace_bytes, double* scores, void* stream) {
    ScoreArgs a;
    auto own_checks = [&]() {
        RV_CHECK(win == 7 || win == 0, "%s: win must be 7, or 0 for the mse alone", who);
        return 0;
    };
    if (int rc = sc_frames(who, "scores", a, out, out_fmt, gt, gt_fmt, gt_layout, nframes, h, w, own_checks, workspace, workspace_bytes,
                           refvsr_score_workspace_bytes(nframes, h, w), scores))
        return rc;
    a.avec = down == 4 && !a.ahwc;                               // (an interleaved tap row is not one aligned group of four)
    const uintptr_t quad = a.afmt == REFVSR_RESULT_F32 ? 15 : a.afmt == REFVSR_RESULT_F16 ? 7 : 3;
    for (int i = 0; i < nframes; ++i)
        if ((uintptr_t)out[i] & quad) a.avec = 0;                // a frame not aligned to four samples: element loads for all
    a.part = (double*)workspace;
    a.h = h; a.w = w;
    a.ntx = sc_tiles(w, SC_TW); a.nty = sc_tiles(h, SC_TH);
    a.win = win;
    const int nt = a.ntx * a.nty;
    const dim3 grid(nt, 3, nframes);
    if (down == 1) hipLaunchKernelGGL(score_tile_kernel<1>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    else if (down == 2) hipLaunchKernelGGL(score_tile_kernel<2>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(score_tile_kernel<4>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_finish_kernel, dim3(nframes), dim3(SC_THREADS), 0, (hipStream_t)stream, (const double*)workspace, 3 * nt, h, w, win,
                       scores);
    RV_LAUNCH_CHECK();
    return 0;
}

extern "C" int refvsr_score_frames(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes,
                                   int h, int w, int win, void* workspace, size_t workspace_bytes, double* scores, void* stream) {
    return sc_run("score_frames", out, out_fmt, gt, gt_fmt, gt_layout, nframes, h, w, 1, win, workspace, workspace_bytes, scores, stream);
}

// results [3][down h][down w], ground truths [3][h][w] (h, w name the ground truth: the tiling, the workspace and the counts are its)
extern "C" int refvsr_score_frames_down(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes,
                                        int h, int w, int down, int win, void* workspace, size_t workspace_bytes, double* scores,
                                        void* stream) {
    RV_CHECK(down == 2 || down == 4, "score_frames_down: down must be 2 or 4 (the result must be `down` times the ground truth)");
    return sc_run("score_frames_down", out, out_fmt, gt, gt_fmt, gt_layout, nframes, h, w, down, win, workspace, workspace_bytes, scores, stream);
}

// ------------------------------------------------------------------------------------------------ rectangle sums (FOV evaluation)
// refvsr_score_regions: per frame and per axis-aligned rectangle r (at most REFVSR_SCORE_MAX_RECTS) the RAW sums { sum (a - b)^2,
// sum S } over the three channels and the pixels of r, where S is the FULL SSIM map of evaluation/metrics.py:18-30 (ssim_masked:
// structural_similarity(full=True), a value at every pixel, the 3-pixel border through scipy's uniform_filter 'reflect' = the
// symmetric extension d c b a | a b c d | d c b a).  The masked scores of evaluation/eval_quan_FOV.py:155-192 are sums and differences
// of such sums (refvsr_amd/metrics.py:fov_table).
//
// Same arithmetic as score_tile_kernel (float64 on the float32 value of every sample, direct 7-term sums left to right, then top to
// bottom, the same five moments and formula).  What differs: a tile is 32 x 64 PIXEL CENTRES (ceil(h / 32) x ceil(w / 64) tiles), its
// 38 x 70 input tile starts 3 rows / columns before the first centre and is staged through the symmetric-reflect index (i < 0 ->
// -i - 1, i >= n -> 2 n - 1 - i; rows that only out-of-frame centres read are clamped into the frame and never used).  The thread of
// centre (y, x) adds S(y, x) and the centre's own (a - b)^2 (read back from the staged tile: every sample is the centre of exactly one
// thread of one tile) to the accumulators of the rectangles that hold (y, x): the column test once per thread, the row test on the
// wave-uniform row (scalar compares), and a rectangle that does not meet the tile -- decided from blockIdx and the arguments alone --
// is skipped by the whole workgroup, so the order of summation never depends on data.
// Reduction (deterministic, no floating-point atomics): per sum a fixed-order __shfl_down tree inside each wave (offsets 32 .. 1), the
// four wave results through LDS as ((w0 + w1) + w2) + w3, one barrier for all 16 sums; plain vector stores to
// workspace[frame][channel][tile][rect][2]; regions_finish_kernel (one workgroup per frame) gives partial sum i to slice i mod 64,
// sums a slice in order and the 64 slices in order.  refvsr_amd/metrics.py:score_regions_model restates all of it in numpy.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the figures next to regions_tile_kernel;
// regions_finish_kernel: 34 VGPRs, 8 KB LDS, no scratch.
struct RegionArgs {
    const void* a[REFVSR_SCORE_MAX_FRAMES];
    const void* b[REFVSR_SCORE_MAX_FRAMES];
    double* part;                      // [nframes][3][nty * ntx][nrects][2] partial sums {sum (a - b)^2, sum S}
    int h, w, ntx, nty;
    int afmt;                          // REFVSR_RESULT_* (the sample format alone)
    int ahwc;                          // results are interleaved [h][w][3] (REFVSR_RESULT_HWC)
    int bkind;                         // SC_GT_*
    int nrects;
    int rect[REFVSR_SCORE_MAX_RECTS][4];   // y0, y1, x0, x1 (half-open); entries past nrects are empty
};

static inline int rg_tiles(int n, int t) { return (n + t - 1) / t; }        // tiles over n pixel centres

__device__ __forceinline__ int rg_reflect(int i, const int n) {             // scipy.ndimage 'reflect' (numpy 'symmetric'), then clamped
    i = i < 0 ? -i - 1 : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return i < 0 ? 0 : i;
}

// fixed-order sum over the 64 lanes of a wave; the result is valid in lane 0
__device__ __forceinline__ double rg_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
    return v;
}

// regions_tile_kernel: 132 VGPRs, 64 SGPRs, no scratch, no spills, 22 816 B LDS, 3 waves per SIMD by registers (figures of the build
// this file was written against -- re-check with -Rpass-analysis=kernel-resource-usage after a change).  The 16 accumulators (32
// VGPRs) on top of the 35 doubles of the row ring put it past 128 VGPRs, one wave per SIMD fewer than score_tile_kernel: a stated
// choice -- the kernel streams LDS into float64 adds, three workgroups per CU keep the float64 pipe fed, and a sixteen-sum spill to
// LDS per output row would cost more than the fourth wave brings.
__global__ void __launch_bounds__(SC_THREADS) regions_tile_kernel(RegionArgs s) {
    __shared__ float tbl[256];
    __shared__ float ta[SC_IH * SC_IW], tb[SC_IH * SC_IW];
    __shared__ double red[4][2 * REFVSR_SCORE_MAX_RECTS];
    const int tid = (int)threadIdx.x;
    const int tile = (int)blockIdx.x, c = (int)blockIdx.y, f = (int)blockIdx.z;
    const int ty = tile / s.ntx, tx = tile - ty * s.ntx;
    const int y0 = ty * SC_TH, x0 = tx * SC_TW;                  // first pixel centre of the tile
    const int h = s.h, w = s.w;
    tbl[tid] = kScoreTable.v[tid];
    __syncthreads();

    // ---- stage the 38 x 70 input tile around the centres, symmetric-reflect at the frame's border
    const unsigned char* __restrict__ pa = (const unsigned char*)s.a[f];
    const unsigned char* __restrict__ pb = (const unsigned char*)s.b[f];
    for (int e = tid; e < SC_IH * SC_IW; e += SC_THREADS) {
        const int r = e / SC_IW, q = e - r * SC_IW;
        const int y = rg_reflect(y0 - 3 + r, h), x = rg_reflect(x0 - 3 + q, w);      // 0 <= y < h, 0 <= x < w
        const size_t ip = ((size_t)c * h + y) * w + x;           // planar [3][h][w]
        const size_t ia = s.ahwc ? ((size_t)y * w + x) * 3 + c : ip;             // interleaved [h][w][3] result
        float va, vb;
        if (s.afmt == REFVSR_RESULT_F32) va = reinterpret_cast<const float*>(pa)[ia];
        else if (s.afmt == REFVSR_RESULT_F16) va = (float)reinterpret_cast<const f16*>(pa)[ia];
        else va = tbl[pa[ia]];
        if (s.bkind == SC_GT_F32) vb = reinterpret_cast<const float*>(pb)[ip];
        else if (s.bkind == SC_GT_U8_PLANAR) vb = tbl[pb[ip]];
        else vb = tbl[pb[((size_t)y * w + x) * 3 + c]];          // interleaved [h][w][3]
        ta[e] = va;
        tb[e] = vb;
    }
    __syncthreads();

    // ---- S and (a - b)^2 of the pixel centres (y0 + 8 wave + o, x0 + lane), added to the rectangles that hold them
    const int col = tid & 63, rg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ox = x0 + col;
    bool touch[REFVSR_SCORE_MAX_RECTS], col_in[REFVSR_SCORE_MAX_RECTS];
    double acc[REFVSR_SCORE_MAX_RECTS][2];
#pragma unroll
    for (int r = 0; r < REFVSR_SCORE_MAX_RECTS; ++r) {
        // (blockIdx and arguments only: workgroup-uniform)
        touch[r] = s.rect[r][0] < y0 + SC_TH && s.rect[r][1] > y0 && s.rect[r][2] < x0 + SC_TW && s.rect[r][3] > x0;
        col_in[r] = ox >= s.rect[r][2] && ox < s.rect[r][3];
        acc[r][0] = 0.0;
        acc[r][1] = 0.0;
    }
    constexpr double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
    constexpr double norm = 49.0 / 48.0;
    double hs[7][5];                                              // horizontal sums of the last seven input rows (static indices)
#pragma unroll
    for (int i = 0; i < SC_ROWS + 6; ++i) {
        const float* ra = ta + (rg * SC_ROWS + i) * SC_IW + col;
        const float* rb = tb + (rg * SC_ROWS + i) * SC_IW + col;
        double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double a = (double)ra[k], b = (double)rb[k];
            sa = sa + a;
            sb = sb + b;
            saa = saa + a * a;
            sbb = sbb + b * b;
            sab = sab + a * b;
        }
        double* hrow = hs[i % 7];
        hrow[0] = sa; hrow[1] = sb; hrow[2] = saa; hrow[3] = sbb; hrow[4] = sab;
        if (i >= 6) {
            double t[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                double a5 = hs[(i - 6) % 7][j];
#pragma unroll
                for (int k = 5; k >= 0; --k) a5 = a5 + hs[(i - k) % 7][j];
                t[j] = a5;
            }
            const double ua = t[0] / 49.0, ub = t[1] / 49.0;
            const double va = norm * (t[2] / 49.0 - ua * ua);
            const double vb = norm * (t[3] / 49.0 - ub * ub);
            const double vab = norm * (t[4] / 49.0 - ua * ub);
            const double num = (2.0 * ua * ub + c1) * (2.0 * vab + c2);
            const double den = (ua * ua + ub * ub + c1) * (va + vb + c2);
            const double ss = num / den;
            // the centre's own sample: input row i - 3 of this thread's rows, column + 3
            const double d = (double)ta[(rg * SC_ROWS + i - 3) * SC_IW + col + 3] - (double)tb[(rg * SC_ROWS + i - 3) * SC_IW + col + 3];
            const double d2 = d * d;
            const int oy = y0 + rg * SC_ROWS + (i - 6);
#pragma unroll
            for (int r = 0; r < REFVSR_SCORE_MAX_RECTS; ++r) {
                if (touch[r]) {
                    const bool in = col_in[r] && oy >= s.rect[r][0] && oy < s.rect[r][1];      // (inside the frame: rectangles are)
                    acc[r][0] = acc[r][0] + (in ? d2 : 0.0);
                    acc[r][1] = acc[r][1] + (in ? ss : 0.0);
                }
            }
        }
    }

    // ---- 16 sums: wave trees, then the four waves through LDS
#pragma unroll
    for (int r = 0; r < REFVSR_SCORE_MAX_RECTS; ++r) {
        double m = 0.0, q = 0.0;
        if (touch[r]) {
            m = rg_wave_sum(acc[r][0]);
            q = rg_wave_sum(acc[r][1]);
        }
        if (col == 0) {
            red[rg][2 * r] = m;
            red[rg][2 * r + 1] = q;
        }
    }
    __syncthreads();
    if (tid < 2 * s.nrects) {
        const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const size_t nt = (size_t)s.ntx * s.nty;
        s.part[(((size_t)f * 3 + c) * nt + tile) * (2 * s.nrects) + tid] = v;
    }
}

// one workgroup per frame: the frame's n = 3 nty ntx partial sums of each of the m = 2 nrects sums -> sums[frame][rect][2].  64 slices per
// sum (1024 threads) and four loads in flight per thread: the walk over a 1080p frame's 3 060 partial sums is bound by load latency
#define RG_SLICES 64
__global__ void __launch_bounds__(16 * RG_SLICES) regions_finish_kernel(const double* __restrict__ part, int n, int m, double* __restrict__ sums) {
    __shared__ double red[RG_SLICES][2 * REFVSR_SCORE_MAX_RECTS];
    const int tid = (int)threadIdx.x, f = (int)blockIdx.x;
    const int j = tid & 15, g = tid >> 4;                         // sum j, slice g: partial sums g, g + 64, .. in order
    const double* p = part + (size_t)f * n * m;
    double v = 0.0;
    if (j < m) {
        int i = g;
        for (; i + 3 * RG_SLICES < n; i += 4 * RG_SLICES) {
            const double q0 = p[(size_t)i * m + j], q1 = p[(size_t)(i + RG_SLICES) * m + j];
            const double q2 = p[(size_t)(i + 2 * RG_SLICES) * m + j], q3 = p[(size_t)(i + 3 * RG_SLICES) * m + j];
            v = v + q0;
            v = v + q1;
            v = v + q2;
            v = v + q3;
        }
        for (; i < n; i += RG_SLICES) v = v + p[(size_t)i * m + j];
    }
    red[g][j] = v;
    __syncthreads();
    if (tid < m) {
        double t = red[0][tid];
#pragma unroll 8
        for (int k = 1; k < RG_SLICES; ++k) t = t + red[k][tid];
        sums[(size_t)f * m + tid] = t;
    }
}

extern "C" int refvsr_score_max_rects(void) { return REFVSR_SCORE_MAX_RECTS; }

extern "C" size_t refvsr_score_regions_workspace_bytes(int nframes, int h, int w, int nrects) {
    if (nframes < 1 || !sc_geometry_ok(h, w) || nrects < 1 || nrects > REFVSR_SCORE_MAX_RECTS) return 0;
    return (size_t)nframes * 3 * rg_tiles(h, SC_TH) * rg_tiles(w, SC_TW) * nrects * 2 * sizeof(double);
}

extern "C" int refvsr_score_regions(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes,
                                    int h, int w, const int* rects, int nrects, void* workspace, size_t workspace_bytes, double* sums,
                                    void* stream) {
    RegionArgs a;                                                // (sc_frames zeroes it: rectangles past nrects are empty, met by no tile)
    auto own_checks = [&]() {
        RV_CHECK(nrects >= 1 && nrects <= REFVSR_SCORE_MAX_RECTS, "score_regions: 1..%d rectangles", REFVSR_SCORE_MAX_RECTS);
        RV_CHECK(rects, "score_regions: null rectangle table");
        for (int r = 0; r < nrects; ++r) {
            const int* q = rects + 4 * r;
            RV_CHECK(q[0] < q[1] && q[2] < q[3], "score_regions: rectangle %d is empty", r);
            RV_CHECK(q[0] >= 0 && q[1] <= h && q[2] >= 0 && q[3] <= w, "score_regions: rectangle %d leaves the frame", r);
        }
        return 0;
    };
    if (int rc = sc_frames("score_regions", "sums", a, out, out_fmt, gt, gt_fmt, gt_layout, nframes, h, w, own_checks, workspace, workspace_bytes,
                           refvsr_score_regions_workspace_bytes(nframes, h, w, nrects), sums))
        return rc;
    a.part = (double*)workspace;
    a.h = h; a.w = w;
    a.ntx = rg_tiles(w, SC_TW); a.nty = rg_tiles(h, SC_TH);
    a.nrects = nrects;
    for (int r = 0; r < nrects; ++r)
        for (int k = 0; k < 4; ++k) a.rect[r][k] = rects[4 * r + k];
    const int nt = a.ntx * a.nty;
    hipLaunchKernelGGL(regions_tile_kernel, dim3(nt, 3, nframes), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(regions_finish_kernel, dim3(nframes), dim3(16 * RG_SLICES), 0, (hipStream_t)stream, (const double*)workspace, 3 * nt,
                       2 * nrects, sums);
    RV_LAUNCH_CHECK();
    return 0;
}
