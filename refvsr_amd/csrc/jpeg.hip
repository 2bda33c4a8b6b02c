// Baseline JPEG of Y'CbCr frames on the device (extension: the reference's consumer writes a JPEG per frame on the host,
// evaluation/eval_qual_quan.py:107-129).  refvsr_jpeg_encode turns up to REFVSR_JPEG_MAX_FRAMES dense 8-bit I420 / I444 frames of one
// geometry -- what refvsr_result_to_yuv writes -- into the entropy-coded data of one JPEG scan each, RST markers included; headers and
// EOI are the host's (refvsr_amd/jpeg.py:header).  The specification is the numpy model refvsr_amd/jpeg.py (encode_model); the kernels
// return its bytes.  Built with -ffp-contract=off, as the file's own pragma says: the transform rounds every product and every sum.
//
// Five launches on the caller's stream, no host synchronisation where dst_capacity covers the frames' upper bound:
//   jp_transform_kernel      8 lanes per 8 x 8 block, 32 blocks per workgroup.  Lane y loads row y of the block byte by byte (rows and
//                            columns clamped into the plane: the edge replication of the model; any address: frames may be views at odd
//                            offsets), level-shifts and forms t[y][u] for u = 0..7; the block is transposed through LDS; lane u forms
//                            F[v][u] for v = 0..7, divides by Q, rounds with rint (half to even), clamps, and writes the int16 at its
//                            zigzag position into an LDS copy of the block, which leaves as eight 16-byte stores: workspace
//                            coef[frame][MCU][block of the MCU][64], the order the scan codes them in.  The DCT matrix and the
//                            quantisation tables are read from the host's float64 tables (no cosine, no reciprocal on the device).
//   jp_entropy_kernel<false> one wave (= one workgroup) per restart interval, one lane per zigzag position; counts the interval's bytes.
//   jp_scan_kernel           one workgroup per frame: exclusive prefix sum of its interval sizes -> ioff, the frame's size -> sizes.
//   jp_offsets_kernel        offsets[f] = sum of sizes[< f].
//   jp_entropy_kernel<true>  the same code again, writing every interval at its final offset: no worst-case slots, no compaction copy.
// The entropy pass, per block of the interval (serial: the DC predictor and the bit position carry from block to block):
//   * lane k holds coefficient k; __ballot of the non-zero AC lanes gives every lane the position of the non-zero coefficient ahead of
//     it, so its run, its ZRLs and its (run, size) symbol are lane-local bit arithmetic; lane 0 codes the DC difference; lane 63 adds
//     the EOB when it holds a zero.  A lane's bits -- at most three ZRLs (33), a code (16) and a value (10) -- fit one 64-bit word.
//   * a wave prefix sum of the lengths places the bits; every lane ORs its word into a 64-dword LDS bit buffer (LDS atomics: lanes
//     share dwords there), most significant bit first.
//   * the whole bytes of the buffer leave it, one byte per lane and round: a __ballot of the 0xFF bytes gives every lane the number of
//     stuffed zeros ahead of it; a lane stores its byte, and the 0x00 behind a 0xFF, with plain byte stores at addresses no other lane
//     writes.  The open byte (< 8 bits) moves to the front of the cleared buffer.
//   At the interval's end the open byte is padded with 1-bits (and stuffed), and RSTm follows unless the interval is the frame's last.
// A block takes at most 22 + 63 * 26 = 1660 bits (jpeg.py:MAX_BLOCK_BITS); with the 7 open bits ahead of it the buffer's highest dword
// touched is 54.  A frame that does not fit dst_capacity behind the frames ahead of it is not written at all; its size is reported.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; figures of the build this file was written
// against): jp_transform_kernel 69 VGPRs, 32 SGPRs, 23 040 B LDS; jp_entropy_kernel<false> / <true> 32 VGPRs, 56 / 60 SGPRs, 4 352 B LDS;
// jp_scan_kernel 24 VGPRs, 16 B LDS; jp_offsets_kernel 4 VGPRs; no scratch, no spills anywhere.
#include "yuv_common.h"
#pragma clang fp contract(off)

#define JP_TBLOCKS 32                               // 8 x 8 blocks per transform workgroup (8 lanes each)
#define JP_MAX_BLOCK_BITS (22 + 63 * 26)
#define JP_LUT 1024                                 // huffman LUT words: DC luma, AC luma, DC chroma, AC chroma, 256 each

struct JpegArgs {
    const unsigned char* src[REFVSR_JPEG_MAX_FRAMES];
    const double* qtab;                             // [2][64] natural order: luma, chroma
    const double* dct;                              // [8][8]
    const uint32_t* lut;                            // [4][256] length << 16 | code
    int16_t* coef;                                  // [n][nblocks][64]
    uint32_t* isz;                                  // [n][nint] bytes of every interval, its RST marker included
    uint32_t* ioff;                                 // [n][nint] offset of every interval inside its frame's data
    unsigned char* dst;
    long long* sizes;                               // [n]
    long long* offsets;                             // [n]
    long long cap;
    int n, h, w, s444;
    int mx, nmcu, bpm, nblocks;                     // MCU columns, MCUs, blocks per MCU, blocks of a frame
    int restart, nint;
};

__constant__ unsigned char jp_zigzag_of[64] = {     // natural index 8 v + u -> zigzag position
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__global__ void __launch_bounds__(JP_TBLOCKS * 8) jp_transform_kernel(JpegArgs g) {
    __shared__ double C[64];
    __shared__ double t[JP_TBLOCKS][8][9];          // [block][y][u], a row padded to 9 doubles
    __shared__ alignas(16) int16_t zz[JP_TBLOCKS][64];
    const int tid = (int)threadIdx.x, lb = tid >> 3, l = tid & 7;
    if (tid < 64) C[tid] = g.dct[tid];
    const int blk = (int)blockIdx.x * JP_TBLOCKS + lb;
    const bool on = blk < g.nblocks;
    const int mcu = blk / g.bpm, b = blk - mcu * g.bpm;
    const int my = mcu / g.mx, mxi = mcu - my * g.mx;
    // the block's plane (0 Y, 1 Cb, 2 Cr), its block coordinates and the plane's size
    int comp, by, bx, ph = g.h, pw = g.w;
    if (g.s444) { comp = b; by = my; bx = mxi; }
    else if (b < 4) { comp = 0; by = 2 * my + (b >> 1); bx = 2 * mxi + (b & 1); }
    else { comp = b - 3; by = my; bx = mxi; ph >>= 1; pw >>= 1; }
    const size_t hw = (size_t)g.h * g.w, cp = g.s444 ? hw : hw >> 2;
    __syncthreads();
    if (on) {
        const unsigned char* __restrict__ p = g.src[blockIdx.y] + (comp == 0 ? 0 : hw + (size_t)(comp - 1) * cp);
        const int y = min(by * 8 + l, ph - 1);
        double s[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) s[x] = (double)((int)p[(size_t)y * pw + min(bx * 8 + x, pw - 1)] - 128);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            double acc = s[0] * C[u * 8];
#pragma unroll
            for (int x = 1; x < 8; ++x) acc = acc + s[x] * C[u * 8 + x];
            t[lb][l][u] = acc;
        }
    }
    __syncthreads();
    if (on) {
        const double* __restrict__ q = g.qtab + (comp ? 64 : 0);
        double ty[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) ty[y] = t[lb][y][l];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            double acc = ty[0] * C[v * 8];
#pragma unroll
            for (int y = 1; y < 8; ++y) acc = acc + ty[y] * C[v * 8 + y];
            const int nat = v * 8 + l;
            double r = rint(acc / q[nat]);
            r = fmin(fmax(r, nat == 0 ? -1024.0 : -1023.0), 1023.0);
            zz[lb][jp_zigzag_of[nat]] = (int16_t)(int)r;
        }
    }
    __syncthreads();
    if (on) {
        uint4* __restrict__ o = reinterpret_cast<uint4*>(g.coef + ((size_t)blockIdx.y * g.nblocks + blk) * 64);
        o[l] = reinterpret_cast<const uint4*>(zz[lb])[l];
    }
}

// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t jp_wave_scan(uint32_t v, const int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// `nbytes` whole bytes of the bit buffer -> the stream at `pos`, 0xFF followed by 0x00; returns the bytes the stream grew by
template <bool WRITE>
__device__ __forceinline__ uint32_t jp_flush(const uint32_t* words, const uint32_t nbytes, unsigned char* __restrict__ out, const uint32_t pos,
                                             const uint32_t lim, const int lane) {
    uint32_t grown = 0;
    for (uint32_t b0 = 0; b0 < nbytes; b0 += 64) {                      // (wave-uniform trip count)
        const uint32_t i = b0 + (uint32_t)lane;
        const bool have = i < nbytes;
        const uint32_t byte = have ? (words[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu : 0u;
        const unsigned long long ff = __ballot(have && byte == 0xffu);
        const uint32_t ahead = (uint32_t)__popcll(ff & ((1ull << lane) - 1ull));
        if (WRITE && have) {
            const uint32_t at = pos + grown + (uint32_t)lane + ahead;
            if (at < lim) out[at] = (unsigned char)byte;
            if (byte == 0xffu && at + 1 < lim) out[at + 1] = 0;
        }
        grown += min(64u, nbytes - b0) + (uint32_t)__popcll(ff);
    }
    return grown;
}

// jp_entropy_kernel<false> counts isz[frame][interval]; <true> writes the interval at offsets[frame] + ioff[frame][interval]
template <bool WRITE>
__global__ void __launch_bounds__(64) jp_entropy_kernel(JpegArgs g) {
    __shared__ uint32_t lut[JP_LUT];
    __shared__ uint32_t words[64];
    const int lane = (int)threadIdx.x;
    const int iv = (int)blockIdx.x, f = (int)blockIdx.y;
#pragma unroll
    for (int i = 0; i < JP_LUT / 64; ++i) lut[i * 64 + lane] = g.lut[i * 64 + lane];
    words[lane] = 0;
    const int m0 = iv * g.restart, m1 = min(m0 + g.restart, g.nmcu);
    const int nblk = (m1 - m0) * g.bpm;
    const int16_t* __restrict__ co = g.coef + ((size_t)f * g.nblocks + (size_t)m0 * g.bpm) * 64;
    unsigned char* out = nullptr;
    uint32_t lim = 0;
    if (WRITE) {
        const long long off = g.offsets[f], size = g.sizes[f];
        if (off + size > g.cap) return;                                  // the frame does not fit: nothing of it is written
        out = g.dst + off;
        lim = (uint32_t)size;
    }
    uint32_t pos = WRITE ? g.ioff[(size_t)f * g.nint + iv] : 0u;
    const uint32_t pos0 = pos;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    uint32_t open = 0;                                                   // bits of the open byte at the front of the buffer
    __syncthreads();
    for (int k = 0, b = 0; k < nblk; ++k, b = (b + 1 == g.bpm ? 0 : b + 1)) {
        const int comp = g.s444 ? b : (b < 4 ? 0 : b - 3);
        const uint32_t* __restrict__ ac = lut + (comp ? 768 : 256);
        const uint32_t* __restrict__ dc = lut + (comp ? 512 : 0);
        const int v = (int)co[(size_t)k * 64 + lane];
        const int dcv = __shfl(v, 0, 64);
        const int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
        if (comp == 0) pred0 = dcv; else if (comp == 1) pred1 = dcv; else pred2 = dcv;
        const int val = lane == 0 ? dcv - pred : v;
        const unsigned long long nz = __ballot(lane > 0 && v != 0);
        const uint32_t mag = (uint32_t)(val < 0 ? -val : val);
        const uint32_t size = 32u - (uint32_t)__clz((int)mag);         // (__clz(0) = 32: size 0)
        const uint32_t vbits = (uint32_t)(val < 0 ? val - 1 : val) & ((1u << size) - 1u);
        unsigned long long code = 0;
        uint32_t len = 0;
        if (lane == 0) {
            const uint32_t e = dc[size];
            code = ((unsigned long long)(e & 0xffffu) << size) | vbits;
            len = (e >> 16) + size;
        } else if (v != 0) {
            const unsigned long long below = nz & ((1ull << lane) - 1ull);
            const int last = below ? 63 - __clzll((long long)below) : 0;
            const int run = lane - last - 1;
            const uint32_t z = ac[0xf0];
            for (int i = 0; i < (run >> 4); ++i) {
                code = (code << (z >> 16)) | (z & 0xffffu);
                len += z >> 16;
            }
            const uint32_t e = ac[((run & 15) << 4) | size];
            code = (((code << (e >> 16)) | (e & 0xffffu)) << size) | vbits;
            len += (e >> 16) + size;
        } else if (lane == 63) {
            const uint32_t e = ac[0];
            code = e & 0xffffu;
            len = e >> 16;
        }
        const uint32_t incl = jp_wave_scan(len, lane);
        const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
        if (len) {
            const uint32_t o = open + incl - len;
            const unsigned long long x = code << (64u - len);
            const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x, j = o >> 5, s = o & 31u;
            const uint32_t w0 = hi >> s, w1 = s ? (hi << (32u - s)) | (lo >> s) : lo, w2 = s ? lo << (32u - s) : 0u;
            if (w0 && j < 64) atomicOr(&words[j], w0);
            if (w1 && j + 1 < 64) atomicOr(&words[j + 1], w1);
            if (w2 && j + 2 < 64) atomicOr(&words[j + 2], w2);
        }
        __syncthreads();
        const uint32_t bits = open + total, nbytes = bits >> 3;
        pos += jp_flush<WRITE>(words, nbytes, out, pos, lim, lane);
        const uint32_t carry = (words[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xffu;      // the open byte (every lane reads it)
        __syncthreads();
        words[lane] = lane == 0 ? carry << 24 : 0u;
        open = bits & 7u;
        __syncthreads();
    }
    if (open) {                                                          // pad with 1-bits, through the stuffing rule
        const uint32_t byte = (words[0] >> 24) | ((1u << (8u - open)) - 1u);
        if (WRITE && lane == 0) {
            if (pos < lim) out[pos] = (unsigned char)byte;
            if (byte == 0xffu && pos + 1 < lim) out[pos + 1] = 0;
        }
        pos += byte == 0xffu ? 2u : 1u;
    }
    if (iv + 1 < g.nint) {
        if (WRITE && lane == 0) {
            if (pos < lim) out[pos] = 0xff;
            if (pos + 1 < lim) out[pos + 1] = (unsigned char)(0xd0 + (iv & 7));
        }
        pos += 2;
    }
    if (!WRITE && lane == 0) g.isz[(size_t)f * g.nint + iv] = pos - pos0;
}

// one workgroup per frame: ioff = the exclusive prefix sum of isz, sizes[frame] = the total
__global__ void __launch_bounds__(256) jp_scan_kernel(JpegArgs g) {
    __shared__ uint32_t wsum[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t* __restrict__ isz = g.isz + (size_t)blockIdx.x * g.nint;
    uint32_t* __restrict__ ioff = g.ioff + (size_t)blockIdx.x * g.nint;
    unsigned long long run = 0;
    for (int i0 = 0; i0 < g.nint; i0 += 256) {                           // (workgroup-uniform trip count)
        const int i = i0 + tid;
        const uint32_t v = i < g.nint ? isz[i] : 0u;
        const uint32_t incl = jp_wave_scan(v, lane);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t ahead = 0;
        for (int k = 0; k < wv; ++k) ahead += wsum[k];
        if (i < g.nint) ioff[i] = (uint32_t)run + ahead + incl - v;
        run += (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) g.sizes[blockIdx.x] = (long long)run;
}

__global__ void __launch_bounds__(64) jp_offsets_kernel(JpegArgs g) {
    const int f = (int)threadIdx.x;
    if (f >= g.n) return;
    long long off = 0;
    for (int k = 0; k < f; ++k) off += g.sizes[k];
    g.offsets[f] = off;
}

struct JpegGeometry { int mx, nmcu, bpm, nblocks, nint; };

static bool jp_geometry(int h, int w, int sampling, int restart, JpegGeometry* q) {
    if (!yuv_geometry_ok(h, w) || h > 65535 || w > 65535) return false;
    if (sampling != REFVSR_YUV_SAMPLING_420 && sampling != REFVSR_YUV_SAMPLING_444) return false;
    if (restart < 1 || restart > 65535) return false;
    const int m = sampling == REFVSR_YUV_SAMPLING_420 ? 16 : 8;
    q->mx = (w + m - 1) / m;
    const long nmcu = (long)((h + m - 1) / m) * q->mx;
    q->bpm = sampling == REFVSR_YUV_SAMPLING_420 ? 6 : 3;
    if (nmcu * q->bpm > (1L << 23)) return false;                       // (a frame's data stays below 2^32 bytes even at the bound)
    q->nmcu = (int)nmcu;
    q->nblocks = q->nmcu * q->bpm;
    q->nint = (q->nmcu + restart - 1) / restart;
    return true;
}

static size_t jp_align(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" int refvsr_jpeg_max_frames(void) { return REFVSR_JPEG_MAX_FRAMES; }

extern "C" size_t refvsr_jpeg_capacity(int h, int w, int sampling, int restart) {
    JpegGeometry q;
    if (!jp_geometry(h, w, sampling, restart, &q)) return 0;
    const size_t full = (size_t)(q.nmcu / restart), last = (size_t)(q.nmcu % restart);
    auto per = [&](size_t mcus) { return 2 * ((mcus * q.bpm * JP_MAX_BLOCK_BITS + 7) / 8) + 2; };
    return full * per((size_t)restart) + (last ? per(last) : 0);
}

extern "C" size_t refvsr_jpeg_workspace_bytes(int nframes, int h, int w, int sampling, int restart) {
    JpegGeometry q;
    if (nframes < 1 || nframes > REFVSR_JPEG_MAX_FRAMES || !jp_geometry(h, w, sampling, restart, &q)) return 0;
    return jp_align((size_t)nframes * q.nblocks * 64 * sizeof(int16_t)) + 2 * jp_align((size_t)nframes * q.nint * sizeof(uint32_t));
}

extern "C" int refvsr_jpeg_encode(const void* const* src, int nframes, int h, int w, int sampling, const double* qtables, const double* dct,
                                  const uint32_t* huffman_lut, int restart, void* dst, size_t dst_capacity, long long* sizes,
                                  long long* offsets, void* workspace, size_t workspace_bytes, void* stream) {
    RV_CHECK(src, "jpeg_encode: null frame table");
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_JPEG_MAX_FRAMES, "jpeg_encode: 1..%d frames per call (got %d)", REFVSR_JPEG_MAX_FRAMES, nframes);
    RV_CHECK(sampling == REFVSR_YUV_SAMPLING_420 || sampling == REFVSR_YUV_SAMPLING_444, "jpeg_encode: sampling must be 4:2:0 or 4:4:4 (got %d)", sampling);
    RV_CHECK(restart >= 1 && restart <= 65535, "jpeg_encode: restart interval must be 1..65535 MCUs (got %d)", restart);
    JpegGeometry q;
    RV_CHECK(jp_geometry(h, w, sampling, restart, &q), "jpeg_encode: h, w must be even, 2..65535, at most 2^23 blocks (got %d x %d)", h, w);
    RV_CHECK(qtables && dct && huffman_lut, "jpeg_encode: null table");
    RV_CHECK(((uintptr_t)qtables & 7) == 0 && ((uintptr_t)dct & 7) == 0 && ((uintptr_t)huffman_lut & 3) == 0, "jpeg_encode: tables must be aligned to their elements");
    RV_CHECK(sizes && offsets && workspace, "jpeg_encode: null sizes / offsets / workspace");
    RV_CHECK(dst || dst_capacity == 0, "jpeg_encode: null dst");
    RV_CHECK(((uintptr_t)sizes & 7) == 0 && ((uintptr_t)offsets & 7) == 0, "jpeg_encode: sizes and offsets must be 8-byte aligned");
    RV_CHECK(((uintptr_t)workspace & 15) == 0, "jpeg_encode: workspace must be 16-byte aligned");
    const size_t needed = refvsr_jpeg_workspace_bytes(nframes, h, w, sampling, restart);
    RV_CHECK(workspace_bytes >= needed, "jpeg_encode: workspace too small (%zu bytes, %zu needed)", workspace_bytes, needed);
    RV_CHECK(dst_capacity < ((size_t)1 << 62), "jpeg_encode: dst_capacity out of range");
    JpegArgs g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(src[i], "jpeg_encode: null pointer (frame %d)", i);
        g.src[i] = (const unsigned char*)src[i];
    }
    unsigned char* ws = (unsigned char*)workspace;
    const size_t coef_bytes = jp_align((size_t)nframes * q.nblocks * 64 * sizeof(int16_t));
    const size_t iv_bytes = jp_align((size_t)nframes * q.nint * sizeof(uint32_t));
    g.qtab = qtables; g.dct = dct; g.lut = huffman_lut;
    g.coef = (int16_t*)ws;
    g.isz = (uint32_t*)(ws + coef_bytes);
    g.ioff = (uint32_t*)(ws + coef_bytes + iv_bytes);
    g.dst = (unsigned char*)dst; g.sizes = sizes; g.offsets = offsets; g.cap = (long long)dst_capacity;
    g.n = nframes; g.h = h; g.w = w; g.s444 = sampling == REFVSR_YUV_SAMPLING_444;
    g.mx = q.mx; g.nmcu = q.nmcu; g.bpm = q.bpm; g.nblocks = q.nblocks; g.restart = restart; g.nint = q.nint;
    RV_CHECK(refvsr_init() == 0, "init failed");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jp_transform_kernel, dim3((unsigned)((q.nblocks + JP_TBLOCKS - 1) / JP_TBLOCKS), (unsigned)nframes), dim3(JP_TBLOCKS * 8), 0, st, g);
    RV_LAUNCH_CHECK();
    const dim3 egrid((unsigned)q.nint, (unsigned)nframes);
    hipLaunchKernelGGL(jp_entropy_kernel<false>, egrid, dim3(64), 0, st, g);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jp_scan_kernel, dim3((unsigned)nframes), dim3(256), 0, st, g);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jp_offsets_kernel, dim3(1), dim3(64), 0, st, g);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jp_entropy_kernel<true>, egrid, dim3(64), 0, st, g);
    RV_LAUNCH_CHECK();
    // a capacity below the frames' upper bound can overflow: only then the call waits for the sizes and reports it
    if (dst_capacity < (size_t)nframes * refvsr_jpeg_capacity(h, w, sampling, restart)) {
        long long hs[REFVSR_JPEG_MAX_FRAMES];
        RV_HIP(hipMemcpyAsync(hs, sizes, sizeof(long long) * nframes, hipMemcpyDeviceToHost, st));
        RV_HIP(hipStreamSynchronize(st));
        long long total = 0;
        for (int i = 0; i < nframes; ++i) {
            total += hs[i];
            if (total > (long long)dst_capacity) {
                refvsr_set_error("jpeg_encode: frame %d does not fit dst_capacity (%lld bytes needed for frames 0..%d, %zu given)", i, total, i, dst_capacity);
                return REFVSR_JPEG_OVERFLOW;
            }
        }
    }
    return 0;
}
