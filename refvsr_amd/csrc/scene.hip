// Scene cuts (extension: the reference's loader serves one folder per clip, data_loader/datasets.py:222-234, and never meets a cut; a
// video file has them).  refvsr_luma_sad gives the sum of absolute luma differences of up to REFVSR_SCENE_MAX_PAIRS pairs of 4:2:0
// frames of one geometry -- the quantity refvsr_amd/scene.py turns into a scene score -- from the frames videorun has on the device
// anyway, so that 8 bytes per frame come back instead of a host-side pass over both luma planes.
//
//   sad[i] = sum over the h w luma codes of |Ya_i - Yb_i|      (exact: integers, the same bits in every order of summation)
//
// The luma plane is the first h w samples of a frame in all four REFVSR_YUV_* formats; a P010 code is sample >> 6, an I420P10 code
// sample & 1023 (yuv_in.hip's yin_code; refvsr_amd/yuv.py:luma_sad is the numpy model).  No floating point, no atomics.
//
// Shape: a pure stream of the two planes, nothing is reused.  A frame lies at any multiple of its sample size (frames inside a
// [t, 3h/2, w] window are 3 h w / 2 samples apart), so a pair is cut at frame a's 16-byte boundaries: `head` samples ahead of the
// first boundary (< 16 bytes), nvec 16-byte groups, `tail` samples behind the last (< 16 bytes).  A group of a is ONE 16-byte load;
// the same samples of b come with the widest of 16 / 8 / 4 / 2 / 1-byte loads b's own phase allows (a wave-uniform choice -- in fact
// one per pair -- as in yuv_in.hip; frames of one window at the usual sizes share their phase and take the 16-byte path).
// Workgroup (chunk c, pair i), 256 threads = 4 waves, owns groups [c SN_VPC, (c + 1) SN_VPC): SN_VPT = 2 groups per thread,
// consecutive lanes on consecutive groups, all four loads issued before the first use.  Chunk 0 also takes the head and the tail,
// element by element.  A 32-bit word holds four 8-bit or two 10-bit codes (P010 shifted, both 10-bit formats masked, two codes per
// instruction) and goes through v_sad_u8 / v_sad_u16 (__builtin_amdgcn_sad_u8 / _u16), which add into the thread's 32-bit sum.
// Overflow: a workgroup sees at most SN_VPC * 16 + 30 = 8 222 samples of at most 1 023 each -- below 2^23, far from 2^32 / 1 023
// samples -- so its partial sum is 32-bit; the total (up to 2^29 * 1 023 > 2^38) is 64-bit.
// Reduction: __shfl_down tree inside each wave, the four waves through LDS, one plain 4-byte vector store per workgroup to
// workspace[pair][chunk]; sn_finish_kernel (one workgroup per pair) adds a pair's partial sums in 64 bits and stores sad[pair].  The
// grid is sized by the largest group count any phase can give (a workgroup past a pair's own count stores 0), so the finishing kernel
// reads initialised words only.  The scheme of fingerprint.hip and score.hip.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the figures next to the kernels.
#include "yuv_common.h"

#define SN_THREADS 256
#define SN_VPT 2                              // 16-byte groups of frame a per thread
#define SN_VPC (SN_THREADS * SN_VPT)          // ... per workgroup

struct SceneArgs {
    const void* a[REFVSR_SCENE_MAX_PAIRS];
    const void* b[REFVSR_SCENE_MAX_PAIRS];
    uint32_t* part;                           // [npairs][nchunks]
    uint32_t n;                               // h * w luma samples
    int nchunks;
};

enum { SN_U8 = 0, SN_P010 = 1, SN_I420P10 = 2 };

// chunks of a pair of n samples of `ssize` bytes: the most 16-byte groups any phase leaves, over SN_VPC, at least one
static inline int sn_chunks(long n, int ssize) {
    const long nvec = n * ssize / 16;
    return (int)(nvec <= SN_VPC ? 1 : (nvec + SN_VPC - 1) / SN_VPC);
}

template <int L> struct SnWord;
template <> struct SnWord<16> { using T = uint4; };
template <> struct SnWord<8> { using T = uint2; };
template <> struct SnWord<4> { using T = uint32_t; };
template <> struct SnWord<2> { using T = uint16_t; };
template <> struct SnWord<1> { using T = uint8_t; };

template <int L>
__device__ __forceinline__ void sn_words(const unsigned char* __restrict__ p, uint32_t* v) {
    using T = typename SnWord<L>::T;
#pragma unroll
    for (int q = 0; q < 16 / L; ++q) reinterpret_cast<T*>(v)[q] = reinterpret_cast<const T*>(p)[q];
}

// 16 bytes from an address aligned to `ph` = its lowest set bit's worth of bytes (16, 8, 4, 2, 1: workgroup-uniform)
__device__ __forceinline__ void sn_load16(const unsigned char* __restrict__ p, const int ph, uint32_t* v) {
    if (ph == 16) sn_words<16>(p, v);
    else if (ph == 8) sn_words<8>(p, v);
    else if (ph == 4) sn_words<4>(p, v);
    else if (ph == 2) sn_words<2>(p, v);
    else sn_words<1>(p, v);
}

template <int MODE, typename S>
__device__ __forceinline__ uint32_t sn_code(const S s) {
    if constexpr (MODE == SN_P010) return (uint32_t)s >> 6;
    else if constexpr (MODE == SN_I420P10) return (uint32_t)s & 1023u;
    else return (uint32_t)s;
}

// acc + the absolute differences of the four 8-bit or two 10-bit codes in the words x, y
template <int MODE>
__device__ __forceinline__ uint32_t sn_sad_word(uint32_t x, uint32_t y, const uint32_t acc) {
    if constexpr (MODE == SN_U8) return __builtin_amdgcn_sad_u8(x, y, acc);
    if constexpr (MODE == SN_P010) { x >>= 6; y >>= 6; }
    return __builtin_amdgcn_sad_u16(x & 0x03ff03ffu, y & 0x03ff03ffu, acc);
}

// sum of one value per thread over the workgroup, valid in thread 0 (any order gives the same bits: integers)
template <typename T>
__device__ __forceinline__ T sn_block_sum(T* red, const int tid, T v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (T)__shfl_down(v, s, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// sn_sad_kernel<SN_U8>, <SN_P010>, <SN_I420P10>: 35 VGPRs, 22 SGPRs each, no scratch, no spills, 16 B LDS, 8 waves per SIMD (figures
// of the build this file was written against -- re-check with -Rpass-analysis=kernel-resource-usage after a change)
template <int MODE>
__global__ void __launch_bounds__(SN_THREADS) sn_sad_kernel(SceneArgs g) {
    using S = typename std::conditional<MODE == SN_U8, uint8_t, uint16_t>::type;
    constexpr uint32_t VS = 16 / sizeof(S);                      // samples per 16-byte group
    __shared__ uint32_t red[SN_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const uint32_t chunk = blockIdx.x;
    const S* __restrict__ pa = reinterpret_cast<const S*>(g.a[blockIdx.y]);      // (workgroup-uniform: scalar loads)
    const S* __restrict__ pb = reinterpret_cast<const S*>(g.b[blockIdx.y]);
    const uint32_t n = g.n;
    // samples ahead of a's first 16-byte boundary (at most n), 16-byte groups, samples behind the last group (< VS)
    const uint32_t mis = (uint32_t)((uintptr_t)pa & 15) / (uint32_t)sizeof(S);
    const uint32_t head = min(n, (VS - mis) & (VS - 1));
    const uint32_t nvec = (n - head) / VS;
    const uint32_t tail0 = head + VS * nvec;                     // first tail sample; n - tail0 < VS
    uint32_t sum = 0;
    if (chunk == 0) {
        if ((uint32_t)tid < head) sum = sn_sad_word<SN_I420P10>(sn_code<MODE>(pa[tid]), sn_code<MODE>(pb[tid]), sum);
        const uint32_t e = tail0 + (uint32_t)tid;
        if (e < n) sum = sn_sad_word<SN_I420P10>(sn_code<MODE>(pa[e]), sn_code<MODE>(pb[e]), sum);
    }
    const unsigned char* __restrict__ va = reinterpret_cast<const unsigned char*>(pa + head);
    const unsigned char* __restrict__ vb = reinterpret_cast<const unsigned char*>(pb + head);
    const uintptr_t ab = (uintptr_t)vb;
    const int ph = (ab & 15) == 0 ? 16 : (ab & 7) == 0 ? 8 : (ab & 3) == 0 ? 4 : (ab & 1) == 0 ? 2 : 1;
    const uint32_t v0 = chunk * SN_VPC + (uint32_t)tid;
    alignas(16) uint32_t x[SN_VPT][4], y[SN_VPT][4];
#pragma unroll
    for (int k = 0; k < SN_VPT; ++k) {
        const uint32_t v = v0 + (uint32_t)k * SN_THREADS;
        if (v < nvec) {
            sn_words<16>(va + (size_t)v * 16, x[k]);
            sn_load16(vb + (size_t)v * 16, ph, y[k]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) x[k][q] = y[k][q] = 0;
        }
    }
#pragma unroll
    for (int k = 0; k < SN_VPT; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) sum = sn_sad_word<MODE>(x[k][q], y[k][q], sum);
    const uint32_t all = sn_block_sum(red, tid, sum);
    if (tid == 0) g.part[(size_t)blockIdx.y * g.nchunks + chunk] = all;
}

// one workgroup per pair: its nchunks partial sums -> sad[pair].  sn_finish_kernel: 9 VGPRs, 17 SGPRs, no scratch, 32 B LDS
__global__ void __launch_bounds__(SN_THREADS) sn_finish_kernel(const uint32_t* __restrict__ part, int nchunks, unsigned long long* __restrict__ sad) {
    __shared__ unsigned long long red[SN_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const uint32_t* __restrict__ p = part + (size_t)blockIdx.x * nchunks;
    unsigned long long sum = 0;
    for (int i = tid; i < nchunks; i += SN_THREADS) sum += p[i];
    const unsigned long long all = sn_block_sum(red, tid, sum);
    if (tid == 0) sad[blockIdx.x] = all;
}

static bool sn_geometry_ok(int h, int w) { return yuv_geometry_ok(h, w) && (long)h * w <= (1L << 29); }

extern "C" int refvsr_scene_max_pairs(void) { return REFVSR_SCENE_MAX_PAIRS; }

// (the format is not an argument: the size is that of the 16-bit formats, the larger one)
extern "C" size_t refvsr_luma_sad_workspace_bytes(int npairs, int h, int w) {
    if (npairs < 1 || npairs > REFVSR_SCENE_MAX_PAIRS || !sn_geometry_ok(h, w)) return 0;
    const size_t bytes = (size_t)npairs * sn_chunks((long)h * w, 2) * sizeof(uint32_t);
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int refvsr_luma_sad(const void* const* a, const void* const* b, int npairs, int h, int w, int yuv_fmt, void* workspace,
                               size_t workspace_bytes, unsigned long long* sad, void* stream) {
    RV_CHECK(a && b, "luma_sad: null frame table");
    RV_CHECK(npairs >= 1 && npairs <= REFVSR_SCENE_MAX_PAIRS, "luma_sad: 1..%d pairs per call (got %d)", REFVSR_SCENE_MAX_PAIRS, npairs);
    RV_CHECK(sn_geometry_ok(h, w), "luma_sad: h, w must be even and positive, h * w <= 2^29 (got %d x %d)", h, w);
    RV_CHECK(yuv_fmt_ok(yuv_fmt), "luma_sad: unknown yuv format %d", yuv_fmt);
    RV_CHECK(workspace && sad, "luma_sad: null workspace / sad");
    RV_CHECK(((uintptr_t)workspace & 15) == 0, "luma_sad: workspace must be 16-byte aligned");
    RV_CHECK(((uintptr_t)sad & 7) == 0, "luma_sad: sad must be 8-byte aligned");
    const size_t needed = refvsr_luma_sad_workspace_bytes(npairs, h, w);
    RV_CHECK(workspace_bytes >= needed, "luma_sad: workspace too small (%zu bytes, %zu needed)", workspace_bytes, needed);
    const bool d10 = yuv_d10(yuv_fmt);
    const uintptr_t smask = yuv_sample_bytes(yuv_fmt) - 1;
    SceneArgs g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < npairs; ++i) {
        RV_CHECK(a[i] && b[i], "luma_sad: null pointer (pair %d)", i);
        RV_CHECK(((uintptr_t)a[i] & smask) == 0 && ((uintptr_t)b[i] & smask) == 0, "luma_sad: frames must be aligned to their samples (pair %d)", i);
        g.a[i] = a[i];
        g.b[i] = b[i];
    }
    g.part = (uint32_t*)workspace;
    g.n = (uint32_t)((long)h * w);
    g.nchunks = sn_chunks((long)h * w, d10 ? 2 : 1);             // (<= the count the workspace was sized by)
    const dim3 grid((unsigned)g.nchunks, (unsigned)npairs), block(SN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (!d10) hipLaunchKernelGGL(sn_sad_kernel<SN_U8>, grid, block, 0, st, g);
    else if (yuv_fmt == REFVSR_YUV_P010) hipLaunchKernelGGL(sn_sad_kernel<SN_P010>, grid, block, 0, st, g);
    else hipLaunchKernelGGL(sn_sad_kernel<SN_I420P10>, grid, block, 0, st, g);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(sn_finish_kernel, dim3(npairs), block, 0, st, (const uint32_t*)workspace, g.nchunks, sad);
    RV_LAUNCH_CHECK();
    return 0;
}
