// Parameter fingerprint: one 64-bit value over a table of fp32 tensors, so that the model shell can tell whether the parameters it
// packed are still the parameters it holds (refvsr_amd/model.py: an in-place write through `.data`, the loader idiom next to
// ckpt_manager.py:50-60, moves no version counter and no pointer).
//
//   F = sum over all words of mix64((uint64(g) << 32) | word)   (mod 2^64)
//
// word: the 32-bit pattern of an element (patterns, not values: -0 and NaN payloads count); g: the element's index over the
// concatenated table, in table order, below 2^32; mix64: splitmix64's finaliser (Steele, Lea, Flood 2014; Vigna's constants)
//   z ^= z >> 30;  z *= 0xbf58476d1ce4e5b9;  z ^= z >> 27;  z *= 0x94d049bb133111eb;  z ^= z >> 31
// -- xor-shifts and odd multipliers, a bijection of the 64-bit words.  Two tables that differ in one word therefore differ in F, the
// position term separates swapped contents, and the sum mod 2^64 is the same bits in every order of summation: no floating point,
// no atomics, nothing that depends on the launch or the stream.  refvsr_amd/fingerprint.py restates it in numpy.
//
// Launch shape: the host cuts the table into chunks of at most REFVSR_FINGERPRINT_CHUNK_WORDS words (fingerprint.py:chunk_table; one
// 16-byte entry each: first word's address, first global index, word count) and keeps them in device memory; one workgroup (256
// threads = 4 waves) sums one chunk -- the 4 KB-word kernels of a conv and the 2-word biases cost a workgroup each, the walk over a
// parameter set is 1 000 - 2 000 workgroups of at most 16 words per thread.  A chunk is read with 16-byte loads from its first
// 16-byte aligned word on (consecutive lanes on consecutive 16 bytes), its unaligned head (<= 3 words: views at odd storage offsets
// are 4-byte aligned only) and its tail (<= 3 words) with 4-byte loads.  Reduction: __shfl_down tree inside each wave, the four
// waves through LDS, one plain 8-byte vector store per workgroup to workspace[chunk]; fp_finish_kernel (one workgroup) sums the
// partial sums and writes F.  The scheme of score.hip, in integers.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the figures next to the kernels.
#include "common.h"

#define FP_THREADS 256

struct FpChunk {                       // one table entry, 16 bytes (fingerprint.py:CHUNK_DTYPE)
    const uint32_t* base;              // first word of the chunk (4-byte aligned)
    uint32_t g0;                       // global index of that word
    uint32_t n;                        // words, 1 .. REFVSR_FINGERPRINT_CHUNK_WORDS
};
static_assert(sizeof(FpChunk) == 16, "the host writes 16-byte entries");

__host__ __device__ __forceinline__ uint64_t fp_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ uint64_t fp_term(const uint32_t g, const uint32_t word) { return fp_mix64(((uint64_t)g << 32) | (uint64_t)word); }

// sum of one value per thread over the workgroup, valid in thread 0 (any order gives the same bits: integers mod 2^64)
__device__ __forceinline__ uint64_t fp_block_sum(uint64_t* red, const int tid, uint64_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, s, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// fp_chunk_kernel: 26 VGPRs, 30 SGPRs, no scratch, no spills, 32 B LDS, 8 waves per SIMD (figures of the build this file was written
// against -- re-check with -Rpass-analysis=kernel-resource-usage after a change)
__global__ void __launch_bounds__(FP_THREADS) fp_chunk_kernel(const FpChunk* __restrict__ chunks, uint64_t* __restrict__ part) {
    __shared__ uint64_t red[FP_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const FpChunk c = chunks[blockIdx.x];                        // (workgroup-uniform: scalar loads)
    const uint32_t* __restrict__ p = c.base;
    const uint32_t n = c.n;
    // words ahead of the first 16-byte boundary (0..3, at most n), 16-byte groups, words behind the last group (0..3)
    const uint32_t mis = (uint32_t)(((uintptr_t)p >> 2) & 3);
    const uint32_t head = min(n, (4u - mis) & 3u);
    const uint32_t nvec = (n - head) >> 2;
    const uint32_t tail0 = head + 4u * nvec;                     // first tail word; n - tail0 <= 3
    uint64_t sum = 0;
    if ((uint32_t)tid < head) sum += fp_term(c.g0 + (uint32_t)tid, p[tid]);
    const uint4* __restrict__ pv = reinterpret_cast<const uint4*>(p + head);
    for (uint32_t v = (uint32_t)tid; v < nvec; v += FP_THREADS) {
        const uint4 q = pv[v];
        const uint32_t g = c.g0 + head + 4u * v;
        sum += fp_term(g, q.x);
        sum += fp_term(g + 1u, q.y);
        sum += fp_term(g + 2u, q.z);
        sum += fp_term(g + 3u, q.w);
    }
    if (tail0 + (uint32_t)tid < n) sum += fp_term(c.g0 + tail0 + (uint32_t)tid, p[tail0 + (uint32_t)tid]);
    const uint64_t all = fp_block_sum(red, tid, sum);
    if (tid == 0) part[blockIdx.x] = all;
}

// one workgroup: the n partial sums -> F.  fp_finish_kernel: 9 VGPRs, 15 SGPRs, no scratch, 32 B LDS
__global__ void __launch_bounds__(FP_THREADS) fp_finish_kernel(const uint64_t* __restrict__ part, int n, uint64_t* __restrict__ out) {
    __shared__ uint64_t red[FP_THREADS / 64];
    const int tid = (int)threadIdx.x;
    uint64_t sum = 0;
    for (int i = tid; i < n; i += FP_THREADS) sum += part[i];
    const uint64_t all = fp_block_sum(red, tid, sum);
    if (tid == 0) out[0] = all;
}

extern "C" size_t refvsr_param_fingerprint_workspace_bytes(int nchunks) {
    if (nchunks < 1 || nchunks > REFVSR_FINGERPRINT_MAX_CHUNKS) return 0;
    return (size_t)nchunks * sizeof(uint64_t);
}

extern "C" int refvsr_param_fingerprint(const void* chunks, int nchunks, void* workspace, size_t workspace_bytes, void* out, void* stream) {
    RV_CHECK(chunks, "param_fingerprint: null chunk table");
    RV_CHECK(nchunks >= 1 && nchunks <= REFVSR_FINGERPRINT_MAX_CHUNKS, "param_fingerprint: 1..%d chunks (got %d)", REFVSR_FINGERPRINT_MAX_CHUNKS,
             nchunks);
    RV_CHECK(((uintptr_t)chunks & 15) == 0, "param_fingerprint: chunk table must be 16-byte aligned");
    RV_CHECK(workspace && out, "param_fingerprint: null workspace / out");
    RV_CHECK(((uintptr_t)workspace & 15) == 0, "param_fingerprint: workspace must be 16-byte aligned");
    RV_CHECK(((uintptr_t)out & 7) == 0, "param_fingerprint: out must be 8-byte aligned");
    const size_t needed = refvsr_param_fingerprint_workspace_bytes(nchunks);
    RV_CHECK(workspace_bytes >= needed, "param_fingerprint: workspace too small (%zu bytes, %zu needed)", workspace_bytes, needed);
    hipLaunchKernelGGL(fp_chunk_kernel, dim3(nchunks), dim3(FP_THREADS), 0, (hipStream_t)stream, (const FpChunk*)chunks, (uint64_t*)workspace);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(fp_finish_kernel, dim3(1), dim3(FP_THREADS), 0, (hipStream_t)stream, (const uint64_t*)workspace, nchunks, (uint64_t*)out);
    RV_LAUNCH_CHECK();
    return 0;
}
