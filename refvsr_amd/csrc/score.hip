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
// at a 3-byte stride), so pointers only need the natural alignment of their element type: fp32 4 bytes, fp16 2 bytes, bytes none.
//
// MSE: every sample belongs to exactly one tile (the last tile of a row / column of tiles owns its 6 halo columns / rows); the thread
// that stages it adds (a - b)^2 to its own float64 sum.
// Reduction (deterministic, no floating-point atomics): per workgroup a fixed LDS tree over the 256 threads, the two sums go to
// workspace[frame][channel][tile] with a plain vector store; score_finish_kernel (one workgroup per frame) sums a frame's partial sums
// in a fixed strided order + the same tree and divides by the counts.  A frame's bits therefore do not depend on the other frames of
// the launch, on the stream or on the run.  refvsr_amd/metrics.py:score_frames_model restates the decomposition and the order in numpy.
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
    int afmt;                          // REFVSR_RESULT_*
    int bkind;                         // SC_GT_*
    int win;                           // 7 | 0
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

// score_tile_kernel: 104 VGPRs, 43 SGPRs, no scratch, no spills, 24 352 B LDS, 4 waves per SIMD by registers (figures of the build
// this file was written against -- re-check with -Rpass-analysis=kernel-resource-usage after a change)
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
            if (s.afmt == REFVSR_RESULT_F32) va = reinterpret_cast<const float*>(pa)[ip];
            else if (s.afmt == REFVSR_RESULT_F16) va = (float)reinterpret_cast<const f16*>(pa)[ip];
            else va = tbl[pa[ip]];
            if (s.bkind == SC_GT_F32) vb = reinterpret_cast<const float*>(pb)[ip];
            else if (s.bkind == SC_GT_U8_PLANAR) vb = tbl[pb[ip]];
            else vb = tbl[pb[((size_t)y * w + x) * 3 + c]];      // interleaved [h][w][3]
            if (r < own_h && q < own_w) {
                const double d = (double)va - (double)vb;
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

extern "C" int refvsr_score_frames(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes,
                                   int h, int w, int win, void* workspace, size_t workspace_bytes, double* scores, void* stream) {
    RV_CHECK(out && gt, "score_frames: null frame table");
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_SCORE_MAX_FRAMES, "score_frames: 1..%d frames per launch", REFVSR_SCORE_MAX_FRAMES);
    RV_CHECK(sc_geometry_ok(h, w), "score_frames: h, w must be at least 7 (the SSIM window) and h * w at most 2^29");
    RV_CHECK(win == 7 || win == 0, "score_frames: win must be 7, or 0 for the mse alone");
    RV_CHECK(out_fmt == REFVSR_RESULT_F32 || out_fmt == REFVSR_RESULT_F16 || out_fmt == REFVSR_RESULT_U8,
             "score_frames: result format must be REFVSR_RESULT_F32 | _F16 | _U8");
    RV_CHECK(gt_fmt == REFVSR_RESULT_F32 || gt_fmt == REFVSR_RESULT_U8, "score_frames: ground-truth format must be REFVSR_RESULT_F32 | _U8");
    RV_CHECK(gt_layout == REFVSR_INGEST_PLANAR || gt_layout == REFVSR_INGEST_HWC,
             "score_frames: ground-truth layout must be REFVSR_INGEST_PLANAR | REFVSR_INGEST_HWC");
    RV_CHECK(!(gt_fmt == REFVSR_RESULT_F32 && gt_layout == REFVSR_INGEST_HWC), "score_frames: the interleaved layout is for uint8 ground truth");
    RV_CHECK(workspace && scores, "score_frames: null workspace / scores");
    RV_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)scores & 15) == 0, "score_frames: workspace and scores must be 16-byte aligned");
    RV_CHECK(workspace_bytes >= refvsr_score_workspace_bytes(nframes, h, w), "score_frames: workspace too small (%zu bytes, %zu needed)",
             workspace_bytes, refvsr_score_workspace_bytes(nframes, h, w));
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    const uintptr_t amask = out_fmt == REFVSR_RESULT_F32 ? 3 : out_fmt == REFVSR_RESULT_F16 ? 1 : 0;
    const uintptr_t bmask = gt_fmt == REFVSR_RESULT_F32 ? 3 : 0;
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(out[i] && gt[i], "score_frames: null pointer (frame %d)", i);
        RV_CHECK(((uintptr_t)out[i] & amask) == 0 && ((uintptr_t)gt[i] & bmask) == 0,
                 "score_frames: fp32 frames must be 4-byte, fp16 frames 2-byte aligned (frame %d)", i);
        a.a[i] = out[i];
        a.b[i] = gt[i];
    }
    a.part = (double*)workspace;
    a.h = h; a.w = w;
    a.ntx = sc_tiles(w, SC_TW); a.nty = sc_tiles(h, SC_TH);
    a.afmt = out_fmt;
    a.bkind = gt_fmt == REFVSR_RESULT_F32 ? SC_GT_F32 : gt_layout == REFVSR_INGEST_PLANAR ? SC_GT_U8_PLANAR : SC_GT_U8_HWC;
    a.win = win;
    const int nt = a.ntx * a.nty;
    hipLaunchKernelGGL(score_tile_kernel, dim3(nt, 3, nframes), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_finish_kernel, dim3(nframes), dim3(SC_THREADS), 0, (hipStream_t)stream, (const double*)workspace, 3 * nt, h, w, win,
                       scores);
    RV_LAUNCH_CHECK();
    return 0;
}
