// What yuv.hip, yuv_in.hip and scene.hip know about a Y'CbCr frame: the REFVSR_YUV_* format predicates, sample and frame bytes and the
// size of a chroma plane.  constexpr: the kernels' template constants and the entries' checks read the same lines.
#pragma once
#include "common.h"

constexpr bool yuv_fmt_ok(int f) { return f >= REFVSR_YUV_NV12 && f <= REFVSR_YUV_I420P10; }
constexpr bool yuv_semi(int f) { return f == REFVSR_YUV_NV12 || f == REFVSR_YUV_P010; }                // interleaved CbCr
constexpr bool yuv_d10(int f) { return f == REFVSR_YUV_P010 || f == REFVSR_YUV_I420P10; }              // 10-bit codes in uint16
constexpr size_t yuv_sample_bytes(int f) { return yuv_d10(f) ? 2 : 1; }
constexpr bool yuv_sampling_ok(int s) { return s >= REFVSR_YUV_SAMPLING_420 && s <= REFVSR_YUV_SAMPLING_444; }
constexpr bool yuv_siting_ok(int s) { return s == REFVSR_YUV_SITING_CENTRE || s == REFVSR_YUV_SITING_LEFT; }
constexpr bool yuv_geometry_ok(int h, int w) { return h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0; }

// Every (format, sampling, left-sited) a kernel of either direction is built for, X(format, sampling, left): semi-planar frames are
// 4:2:0, 4:4:4 has no siting (an entry launches its centre instance for both).  The dispatch of each direction is this list.
#define YUV_INSTANCES(X)                                                                                          \
    X(NV12, 420, false) X(I420, 420, false) X(P010, 420, false) X(I420P10, 420, false)                            \
    X(NV12, 420, true) X(I420, 420, true) X(P010, 420, true) X(I420P10, 420, true)                                \
    X(I420, 422, false) X(I420P10, 422, false) X(I420, 422, true) X(I420P10, 422, true)                           \
    X(I420, 444, false) X(I420P10, 444, false)

// samples of one chroma plane of a frame of hw luma samples
template <typename I>
constexpr I yuv_chroma_plane(I hw, int sampling) {
    return hw >> (sampling == REFVSR_YUV_SAMPLING_444 ? 0 : sampling == REFVSR_YUV_SAMPLING_420 ? 2 : 1);
}

// bytes of one frame: Y and two chroma planes; 0 for what no entry takes (odd or non-positive h, w, unknown ids, semi-planar 4:2:2 / 4:4:4)
static inline size_t yuv_frame_bytes(int h, int w, int f, int sampling) {
    if (!yuv_geometry_ok(h, w) || !yuv_fmt_ok(f) || !yuv_sampling_ok(sampling)) return 0;
    if (sampling != REFVSR_YUV_SAMPLING_420 && yuv_semi(f)) return 0;
    const size_t hw = (size_t)h * w;
    return (hw + 2 * yuv_chroma_plane(hw, sampling)) * yuv_sample_bytes(f);
}
