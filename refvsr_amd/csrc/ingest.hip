// 8-bit input frames (data_loader/utils.py:12-41 reads PNGs as bytes and divides by 255 in float64; models/archs/RefVSR.py:151
// then gets float frames in [0, 1]).  refvsr_ingest_u8 turns up to REFVSR_INGEST_MAX_FRAMES byte frames of one geometry into the
// planar fp32 frames the engine owns, in one launch; refvsr_bytes_equal is the content compare of the byte copies the engine keeps.
//
// Exactness: every byte u maps through T[u] = (float)((double)u / 255.0) -- the reference loader's float64 quotient rounded to the
// float32 the network computes in (and what numpy's float32 `/ 255.` gives: the float32 quotient of two exact operands is the
// correctly rounded quotient, and float64 -> float32 rounding of the float64 quotient gives the same value for all 256 bytes,
// tests/test_input_u8.py).  u * (1 / 255.f) is NOT the same function (it differs on 126 of the 256 values).
#include "common.h"
#include "ingest_table.h"

static constexpr IngestTable kIngestHost = ingest_table();
__constant__ IngestTable kIngestDev = ingest_table();

struct IngestArgs {
    const unsigned char* src[REFVSR_INGEST_MAX_FRAMES];
    float* dst[REFVSR_INGEST_MAX_FRAMES];
    int hw;                  // pixels per plane (h * w, a multiple of 4)
};

__device__ __forceinline__ void ingest_load_table(float* tbl) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) tbl[i] = kIngestDev.v[i];
    __syncthreads();
}

__device__ __forceinline__ float4 ingest4(const float* tbl, uint32_t d) {
    return make_float4(tbl[d & 255], tbl[(d >> 8) & 255], tbl[(d >> 16) & 255], tbl[d >> 24]);
}

// planar [3][h][w] bytes -> planar fp32: one flat run of n = 3 h w samples.  Thread k owns the 16 source bytes of the k-th 16-byte
// aligned block of the source ADDRESS space that meets the frame (the first and the last one may be partial): whole blocks are
// one 16-byte load, partial ones dword loads (the frame starts and ends on a 4-byte boundary).  The first sample of a block has an
// index that is a multiple of 4, so every group of four samples is one float4 store.
__global__ void __launch_bounds__(256) ingest_planar_kernel(IngestArgs a) {
    __shared__ float tbl[256];
    ingest_load_table(tbl);
    const unsigned char* __restrict__ src = a.src[blockIdx.y];
    float* __restrict__ dst = a.dst[blockIdx.y];
    const long n = 3L * a.hw;
    const long r = (long)((uintptr_t)src & 15);
    const long nblk = (n + r + 15) >> 4;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < nblk; k += (long)gridDim.x * blockDim.x) {
        const long b0 = 16 * k - r;                      // sample index of the block's first byte (< 0 in a partial head)
        if (b0 >= 0 && b0 + 16 <= n) {
            const uint4 q = *reinterpret_cast<const uint4*>(src + b0);
            float4* o = reinterpret_cast<float4*>(dst + b0);
            o[0] = ingest4(tbl, q.x);
            o[1] = ingest4(tbl, q.y);
            o[2] = ingest4(tbl, q.z);
            o[3] = ingest4(tbl, q.w);
        } else {
            for (int j = 0; j < 4; ++j) {
                const long e = b0 + 4 * j;
                if (e >= 0 && e < n)
                    *reinterpret_cast<float4*>(dst + e) = ingest4(tbl, *reinterpret_cast<const uint32_t*>(src + e));
            }
        }
    }
}

// 48 source bytes (16 interleaved pixels) at a 4-byte aligned address with (address % 16) == 4 * (4 - HD) % 16: HD leading dwords,
// two or three 16-byte loads, the trailing dwords
template <int HD>
__device__ __forceinline__ void ingest_load48(const unsigned char* p, uint32_t (&d)[12]) {
    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < HD; ++j) d[j] = p32[j];
    constexpr int NQ = (12 - HD) / 4;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + 4 * HD + 16 * q);
        d[HD + 4 * q] = v.x; d[HD + 4 * q + 1] = v.y; d[HD + 4 * q + 2] = v.z; d[HD + 4 * q + 3] = v.w;
    }
#pragma unroll
    for (int j = HD + 4 * NQ; j < 12; ++j) d[j] = p32[j];
}

__device__ __forceinline__ uint32_t ingest_byte(const uint32_t (&d)[12], int i) { return (d[i >> 2] >> (8 * (i & 3))) & 255; }

// interleaved [h][w][3] bytes -> planar fp32: thread k owns pixels [16 k, 16 k + 16) of the frame (48 source bytes; a frame of
// h w % 16 != 0 pixels ends in a group of 4, 8 or 12, loaded dword by dword).  The source offset 48 k keeps the address's
// 16-byte phase, which is uniform over the frame (HD, a template argument); every plane gets four float4 stores per group.
template <int HD>
__device__ __forceinline__ void ingest_hwc_frame(const float* tbl, const unsigned char* __restrict__ src, float* __restrict__ dst, int hw) {
    const long ng = (hw + 15) / 16;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < ng; k += (long)gridDim.x * blockDim.x) {
        const long p0 = 16 * k;
        const int np = (int)(hw - p0 < 16 ? hw - p0 : 16);        // 4, 8, 12 or 16
        uint32_t d[12];
        if (np == 16) {
            ingest_load48<HD>(src + 3 * p0, d);
        } else {
            const uint32_t* p32 = reinterpret_cast<const uint32_t*>(src + 3 * p0);
#pragma unroll
            for (int j = 0; j < 12; ++j) d[j] = j < 3 * np / 4 ? p32[j] : 0u;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (4 * g < np) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int i0 = 12 * g + c;
                    *reinterpret_cast<float4*>(dst + (long)c * hw + p0 + 4 * g) =
                        make_float4(tbl[ingest_byte(d, i0)], tbl[ingest_byte(d, i0 + 3)], tbl[ingest_byte(d, i0 + 6)], tbl[ingest_byte(d, i0 + 9)]);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) ingest_hwc_kernel(IngestArgs a) {
    __shared__ float tbl[256];
    ingest_load_table(tbl);
    const unsigned char* src = a.src[blockIdx.y];
    float* dst = a.dst[blockIdx.y];
    switch ((uintptr_t)src & 15) {                       // (block-uniform: one frame per blockIdx.y)
        case 0: ingest_hwc_frame<0>(tbl, src, dst, a.hw); break;
        case 4: ingest_hwc_frame<3>(tbl, src, dst, a.hw); break;
        case 8: ingest_hwc_frame<2>(tbl, src, dst, a.hw); break;
        default: ingest_hwc_frame<1>(tbl, src, dst, a.hw); break;
    }
}

extern "C" int refvsr_ingest_max_frames(void) { return REFVSR_INGEST_MAX_FRAMES; }

extern "C" int refvsr_ingest_table(float* out) {
    RV_CHECK(out, "ingest_table: null pointer");
    memcpy(out, kIngestHost.v, sizeof(kIngestHost.v));
    return 0;
}

extern "C" int refvsr_ingest_u8(const void* const* src, float* const* dst, int nframes, int h, int w, int layout, void* stream) {
    RV_CHECK(src && dst, "ingest_u8: null frame table");
    RV_CHECK(nframes >= 1 && nframes <= REFVSR_INGEST_MAX_FRAMES, "ingest_u8: 1..%d frames per launch", REFVSR_INGEST_MAX_FRAMES);
    RV_CHECK(layout == REFVSR_INGEST_PLANAR || layout == REFVSR_INGEST_HWC, "ingest_u8: layout must be REFVSR_INGEST_PLANAR | REFVSR_INGEST_HWC");
    RV_CHECK(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && (long)h * w <= (1L << 29), "ingest_u8: h, w must be even and positive");
    IngestArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nframes; ++i) {
        RV_CHECK(src[i] && dst[i], "ingest_u8: null pointer (frame %d)", i);
        RV_CHECK(((uintptr_t)src[i] & 3) == 0 && ((uintptr_t)dst[i] & 15) == 0,
                 "ingest_u8: source must be 4-byte, destination 16-byte aligned (frame %d)", i);
        a.src[i] = (const unsigned char*)src[i];
        a.dst[i] = dst[i];
    }
    a.hw = h * w;
    const long work = layout == REFVSR_INGEST_PLANAR ? (3L * a.hw + 15 + 15) / 16 : (a.hw + 15) / 16;   // threads per frame
    const long want = (work + 255) / 256;
    const int gx = (int)(want < 1024 ? want : 1024);
    if (layout == REFVSR_INGEST_PLANAR)
        hipLaunchKernelGGL(ingest_planar_kernel, dim3(gx, nframes), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ingest_hwc_kernel, dim3(gx, nframes), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// byte-granular content compare: any length, any alignment of either buffer, up to EQ8_MAX_PAIRS pairs per launch
// ------------------------------------------------------------------------------------------------
#define EQ8_MAX_PAIRS 32
struct Eq8Args { const unsigned char* a[EQ8_MAX_PAIRS]; const unsigned char* b[EQ8_MAX_PAIRS]; size_t n; int* flags; };

// Thread k owns the k-th 16-byte aligned block of a's address space that meets the buffer: a whole block is one 16-byte load of a
// and, depending on b's phase there, one 16-byte load, four dword loads or 16 byte loads of b; partial blocks go byte by byte.
__global__ void __launch_bounds__(256) bytes_equal_kernel(Eq8Args e) {
    const unsigned char* __restrict__ a = e.a[blockIdx.y];
    const unsigned char* __restrict__ b = e.b[blockIdx.y];
    const long n = (long)e.n;
    const long r = (long)((uintptr_t)a & 15);
    const long nblk = (n + r + 15) >> 4;
    const int rb = (int)(((uintptr_t)b - (uintptr_t)a) & 15);          // b's phase where a is 16-byte aligned (block-uniform)
    bool diff = false;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < nblk; k += (long)gridDim.x * blockDim.x) {
        const long o = 16 * k - r;
        if (o >= 0 && o + 16 <= n) {
            const uint4 x = *reinterpret_cast<const uint4*>(a + o);
            uint4 y;
            if (rb == 0) {
                y = *reinterpret_cast<const uint4*>(b + o);
            } else if ((rb & 3) == 0) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(b + o);
                y = make_uint4(q[0], q[1], q[2], q[3]);
            } else {
                uint32_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = (uint32_t)b[o + 4 * j] | ((uint32_t)b[o + 4 * j + 1] << 8) | ((uint32_t)b[o + 4 * j + 2] << 16) |
                           ((uint32_t)b[o + 4 * j + 3] << 24);
                y = make_uint4(v[0], v[1], v[2], v[3]);
            }
            diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
        } else {
            for (int j = 0; j < 16; ++j) {
                const long i = o + j;
                if (i >= 0 && i < n) diff |= a[i] != b[i];
            }
        }
    }
    // every writer stores the same value (as in buffers_equal_kernel)
    if (__any(diff) && (threadIdx.x & 63) == 0) e.flags[blockIdx.y] = 0;
}

extern "C" int refvsr_bytes_equal(const void* const* a, const void* const* b, int n_pairs, size_t n_bytes, int32_t* flags, void* stream) {
    RV_CHECK(a && b && flags && n_pairs > 0 && n_pairs <= EQ8_MAX_PAIRS, "bytes_equal: 1..%d pairs per call", EQ8_MAX_PAIRS);
    RV_CHECK(n_bytes > 0, "bytes_equal: empty buffers");
    Eq8Args e;
    memset(&e, 0, sizeof(e));
    for (int i = 0; i < n_pairs; ++i) {
        RV_CHECK(a[i] && b[i], "bytes_equal: null pointer (pair %d)", i);
        e.a[i] = (const unsigned char*)a[i];
        e.b[i] = (const unsigned char*)b[i];
    }
    e.n = n_bytes;
    e.flags = flags;
    const size_t nblk = (n_bytes + 15 + 15) / 16;
    const int gx = (int)((nblk + 255) / 256 > 256 ? 256 : (nblk + 255) / 256);
    hipLaunchKernelGGL(bytes_equal_kernel, dim3(gx, n_pairs), dim3(256), 0, (hipStream_t)stream, e);
    RV_LAUNCH_CHECK();
    return 0;
}
