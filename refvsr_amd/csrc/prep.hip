// Per-frame preparation that is launch-latency bound when done one small kernel at a time: the SPyNet image pyramid and the
// layout / MeanShift passes over the two 3-channel frames.  Both kernels restate the arithmetic of the launches they replace
// (pool2_kernel, conv_direct_kernel with a 1x1 filter, pack_nhwc16_kernel, pack_nhwc32_kernel) expression by expression, so their
// outputs are the same bits (tests/test_gpu_match_prep.py).  Contraction is switched off in every restated expression: none of
// the originals contains a product that feeds a sum other than through an explicit fmaf.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// five 2x2 average pools in one launch (SPyNet.py:117-126: the pyramid below the /32-padded level 0)
// ------------------------------------------------------------------------------------------------
// One workgroup per 32 x 32 tile of the level-0 map and channel: level k + 1 is computed from the STORED fp32 values of level k
// (kept in LDS as well) as 0.25f * (a + b + cc + d), a, b the upper pair, cc, d the lower -- pool2_kernel's expression.
struct PyrArgs { const float* src; float* dst[5]; int h, w; };

__device__ __forceinline__ float pool4(float a, float b, float cc, float d) {
#pragma clang fp contract(off)
    return 0.25f * (a + b + cc + d);
}

__global__ __launch_bounds__(256) void avgpool_pyramid_kernel(PyrArgs a) {
    __shared__ float s1[16 * 16], s2[8 * 8], s3[4 * 4], s4[2 * 2];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x, ty = blockIdx.y, ch = blockIdx.z;
    const int h = a.h, w = a.w;
    {
        const int ox = tid & 15, oy = tid >> 4;
        const float* s = a.src + ((size_t)ch * h + ty * 32 + 2 * oy) * w + tx * 32 + 2 * ox;
        const float2 r0 = *reinterpret_cast<const float2*>(s), r1 = *reinterpret_cast<const float2*>(s + w);
        const float v = pool4(r0.x, r0.y, r1.x, r1.y);
        a.dst[0][((size_t)ch * (h >> 1) + ty * 16 + oy) * (w >> 1) + tx * 16 + ox] = v;
        s1[tid] = v;
    }
    __syncthreads();
    if (tid < 64) {
        const int ox = tid & 7, oy = tid >> 3;
        const float* s = s1 + (2 * oy) * 16 + 2 * ox;
        const float v = pool4(s[0], s[1], s[16], s[17]);
        a.dst[1][((size_t)ch * (h >> 2) + ty * 8 + oy) * (w >> 2) + tx * 8 + ox] = v;
        s2[tid] = v;
    }
    __syncthreads();
    if (tid < 16) {
        const int ox = tid & 3, oy = tid >> 2;
        const float* s = s2 + (2 * oy) * 8 + 2 * ox;
        const float v = pool4(s[0], s[1], s[8], s[9]);
        a.dst[2][((size_t)ch * (h >> 3) + ty * 4 + oy) * (w >> 3) + tx * 4 + ox] = v;
        s3[tid] = v;
    }
    __syncthreads();
    if (tid < 4) {
        const int ox = tid & 1, oy = tid >> 1;
        const float* s = s3 + (2 * oy) * 4 + 2 * ox;
        const float v = pool4(s[0], s[1], s[4], s[5]);
        a.dst[3][((size_t)ch * (h >> 4) + ty * 2 + oy) * (w >> 4) + tx * 2 + ox] = v;
        s4[tid] = v;
    }
    __syncthreads();
    if (tid == 0) a.dst[4][((size_t)ch * (h >> 5) + ty) * (w >> 5) + tx] = pool4(s4[0], s4[1], s4[2], s4[3]);
}

extern "C" int refvsr_avgpool_pyramid(const float* src, int c, int h, int w, float* const* dst, void* stream) {
    RV_CHECK(src && dst && c > 0 && c <= 65535 && h > 0 && w > 0, "avgpool_pyramid: bad args");
    RV_CHECK(h % 32 == 0 && w % 32 == 0 && h / 32 <= 65535, "avgpool_pyramid: the map must be a whole number of 32 x 32 tiles (got %d x %d)", h, w);
    RV_CHECK(((uintptr_t)src & 7) == 0, "avgpool_pyramid: src must be 8-byte aligned");
    PyrArgs a;
    a.src = src; a.h = h; a.w = w;
    for (int k = 0; k < 5; ++k) {
        RV_CHECK(dst[k], "avgpool_pyramid: null level pointer (level %d)", k + 1);
        a.dst[k] = dst[k];
    }
    hipLaunchKernelGGL(avgpool_pyramid_kernel, dim3(w / 32, h / 32, c), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// frame preparation: lr8, ref8, MeanShift(lr) packed, avg_pool2(MeanShift(ref)) packed
// ------------------------------------------------------------------------------------------------
// What seven launches did with seven passes over the two 3-channel frames (pack_nhwc16 x 2; conv_direct with the 1x1 MeanShift
// filter x 2, common.py:84-94; avg_pool2 of the reference map, attention.py:70; pack_nhwc32 x 2).  Threads [0, h w) take one LR
// pixel each, threads behind them one 2 x 2 quad of the reference frame (a partial quad at an odd edge only feeds ref8).
struct PrepArgs {
    const float* lr; const float* ref; const float* wgt; const float* bias;
    f16* lr8; f16* ref8; float* lr_n; float* ref_n;
    int h, w, hr, wr;
};

// conv_direct_kernel for k = 1, cin = cout = 3, slope 1: acc = fmaf(x[ci], w[co][ci], acc) over ci from acc = 0, then acc + bias
// (rv_lrelu with slope 1 returns its argument)
__device__ __forceinline__ void mean_shift3(const float (&x)[3], const float (&wg)[9], const float (&b)[3], float (&o)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        float acc = 0.0f;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) acc = fmaf(x[ci], wg[co * 3 + ci], acc);
        o[co] = rv_lrelu(acc + b[co], 1.0f);
    }
}

__device__ __forceinline__ f16x8 pack8(const float (&x)[3]) {
    f16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (f16)0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (f16)x[k];
    return v;
}

__global__ __launch_bounds__(256) void frame_prep_kernel(PrepArgs a) {
    const int n_lr = a.h * a.w;
    const int qw = (a.wr + 1) >> 1, qh = (a.hr + 1) >> 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lr + qw * qh) return;
    float wg[9], b[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) wg[k] = a.wgt[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = a.bias[k];
    if (i < n_lr) {
        float x[3], m[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) x[ch] = a.lr[(size_t)ch * n_lr + i];
        mean_shift3(x, wg, b, m);
        *reinterpret_cast<f16x8*>(a.lr8 + (size_t)i * 8) = pack8(x);
        *reinterpret_cast<f32x4*>(a.lr_n + (size_t)i * 4) = (f32x4){m[0], m[1], m[2], 0.f};
        return;
    }
    const int q = i - n_lr;
    const int qy = q / qw, qx = q - qy * qw;
    const size_t plane = (size_t)a.hr * a.wr;
    float m[4][3];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int y = 2 * qy + (t >> 1), x_ = 2 * qx + (t & 1);
        if (y < a.hr && x_ < a.wr) {
            const size_t pix = (size_t)y * a.wr + x_;
            float x[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) x[ch] = a.ref[ch * plane + pix];
            mean_shift3(x, wg, b, m[t]);
            *reinterpret_cast<f16x8*>(a.ref8 + pix * 8) = pack8(x);
        }
    }
    if (2 * qy + 1 < a.hr && 2 * qx + 1 < a.wr) {
        float* o = a.ref_n + ((size_t)qy * (a.wr >> 1) + qx) * 4;
        *reinterpret_cast<f32x4*>(o) = (f32x4){pool4(m[0][0], m[1][0], m[2][0], m[3][0]), pool4(m[0][1], m[1][1], m[2][1], m[3][1]),
                                               pool4(m[0][2], m[1][2], m[2][2], m[3][2]), 0.f};
    }
}

extern "C" int refvsr_frame_prep(const float* lr, int h, int w, const float* ref, int hr, int wr, const float* wgt, const float* bias,
                                 void* lr8, void* ref8, float* lr_n, float* ref_n, void* stream) {
    RV_CHECK(lr && ref && wgt && bias && lr8 && ref8 && lr_n && ref_n, "frame_prep: null pointer");
    RV_CHECK(h > 0 && w > 0 && hr >= 2 && wr >= 2, "frame_prep: bad sizes");
    RV_CHECK((long long)h * w + (long long)((hr + 1) / 2) * ((wr + 1) / 2) < (1ll << 30), "frame_prep: frames too large");
    RV_CHECK((((uintptr_t)lr8 | (uintptr_t)ref8 | (uintptr_t)lr_n | (uintptr_t)ref_n) & 15) == 0, "frame_prep: outputs must be 16-byte aligned");
    PrepArgs a;
    a.lr = lr; a.ref = ref; a.wgt = wgt; a.bias = bias;
    a.lr8 = (f16*)lr8; a.ref8 = (f16*)ref8; a.lr_n = lr_n; a.ref_n = ref_n;
    a.h = h; a.w = w; a.hr = hr; a.wr = wr;
    const int total = h * w + ((hr + 1) / 2) * ((wr + 1) / 2);
    hipLaunchKernelGGL(frame_prep_kernel, dim3(rv_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}
