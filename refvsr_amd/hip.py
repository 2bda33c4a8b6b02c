"""ctypes binding of librefvsr_hip.so (the C-ABI declared in include/refvsr_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  Build it with `make -C refvsr_amd/csrc` (or `__graft_entry__.build()`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'librefvsr_hip.so')

OUT_NHWC16, OUT_NHWC16_SHUFFLE2, OUT_PLANAR32 = 0, 1, 2
RS_BICUBIC, RS_BILINEAR, RS_BILINEAR_AC, RS_NEAREST = 0, 1, 2, 3
RESULT_F32, RESULT_F16, RESULT_U8 = 0, 1, 2
RESULT_HWC = 0x10                           # REFVSR_RESULT_HWC: flag bit of an out_fmt, the result is interleaved [h][w][3]
INGEST_PLANAR, INGEST_HWC = 0, 1
YUV_NV12, YUV_I420, YUV_P010, YUV_I420P10 = range(4)       # REFVSR_YUV_*: `yuv_fmt` of refvsr_result_to_yuv420, `format` of refvsr_yuv420_to_rgb
YUV_CHROMA_BILINEAR, YUV_CHROMA_NEAREST = 0, 1             # REFVSR_YUV_CHROMA_*: `chroma` of refvsr_yuv420_to_rgb
YUV_SAMPLING_420, YUV_SAMPLING_422, YUV_SAMPLING_444 = range(3)      # REFVSR_YUV_SAMPLING_*: `sampling` of refvsr_result_to_yuv / refvsr_yuv_to_rgb
YUV_SITING_CENTRE, YUV_SITING_LEFT = 0, 1                  # REFVSR_YUV_SITING_*: `siting` of the same two
C24_CONV24, C24_CONV32, C24_CONV48, C24_SHUFFLE2, C24_CONF_ALPHA, C24_CONV_LAST = range(6)      # REFVSR_C24_*: `op` of refvsr_conv24_variant
MATCH_KP, MATCH_ROWCHUNK, MATCH_COLBLOCK = 152, 256, 512
ABI_VERSION = 15
MAX_MAPS = 4
INGEST_MAX_FRAMES = 16                      # REFVSR_INGEST_MAX_FRAMES: byte frames per refvsr_ingest_u8 launch
SCORE_MAX_FRAMES = 16                       # REFVSR_SCORE_MAX_FRAMES: frame pairs per refvsr_score_frames launch
SCORE_MAX_RECTS = 8                         # REFVSR_SCORE_MAX_RECTS: rectangles per refvsr_score_regions launch
COLORMAP_MAX_MAPS = 16                      # REFVSR_COLORMAP_MAX_MAPS: maps per refvsr_conf_colormap launch
YUV420_MAX_FRAMES = 16                      # REFVSR_YUV420_MAX_FRAMES: result frames per refvsr_result_to_yuv420 launch
YUV420_IN_MAX_FRAMES = 16                   # REFVSR_YUV420_IN_MAX_FRAMES: 4:2:0 input frames per refvsr_yuv420_to_rgb launch
SCENE_MAX_PAIRS = 16                        # REFVSR_SCENE_MAX_PAIRS: frame pairs per refvsr_luma_sad call
RESIZE_MAX_FRAMES = 16                      # REFVSR_RESIZE_MAX_FRAMES: frames per refvsr_resize_aa launch
JPEG_MAX_FRAMES = 16                        # REFVSR_JPEG_MAX_FRAMES: frames per refvsr_jpeg_encode call
JPEG_OVERFLOW = 3                           # REFVSR_JPEG_OVERFLOW: the return code of a frame that did not fit dst_capacity
FINGERPRINT_CHUNK_WORDS = 4096              # REFVSR_FINGERPRINT_CHUNK_WORDS: words per chunk-table entry of refvsr_param_fingerprint
RESBLOCK24_BLOB_BYTES = 43264
RESBLOCK24_F16W_BLOB_BYTES = 28928          # the fp16 weight format (ABI 15)
RESBLOCK48_BLOB_BYTES = 172544


class RefvsrConv(C.Structure):
    """Mirror of `struct RefvsrConv` (include/refvsr_hip.h)."""
    _fields_ = [
        ('src0', C.c_void_p), ('c0', C.c_int),
        ('src1', C.c_void_p), ('c1', C.c_int),
        ('h_in', C.c_int), ('w_in', C.c_int),
        ('h_out', C.c_int), ('w_out', C.c_int),
        ('ksize', C.c_int), ('stride', C.c_int), ('pad', C.c_int),
        ('wpack', C.c_void_p), ('bias', C.c_void_p),
        ('cout', C.c_int), ('mt_per_block', C.c_int), ('ksteps', C.c_int),
        ('act_slope', C.c_float),
        ('mul', C.c_void_p), ('mul_c', C.c_int),
        ('res', C.c_void_p), ('res_c', C.c_int),
        ('post_slope', C.c_float),
        ('out_mode', C.c_int),
        ('out', C.c_void_p), ('out_c', C.c_int),
        ('res_planar', C.c_void_p),
        ('f32', C.c_int),
        ('add_const', C.c_float), ('clamp_lo', C.c_float), ('clamp_hi', C.c_float),
        ('batch', C.c_int), ('bs_src0', C.c_size_t), ('bs_src1', C.c_size_t), ('bs_out', C.c_size_t), ('bs_res_planar', C.c_size_t),
    ]


_P, _I, _F, _Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> argtypes; every function returns int (0 = ok) except the two listed in _SPECIAL
SIGNATURES = {
    'refvsr_init': [],
    'refvsr_max_maps': [],                       # returns REFVSR_MAX_MAPS
    'refvsr_num_cus': [],                        # returns the CU count
    'refvsr_stream_create_cu_range': [_I, _I, C.POINTER(C.c_void_p)],
    'refvsr_stream_set_cu_budget': [_P, _I],
    'refvsr_stream_destroy': [_P],
    'refvsr_conv_mfma': [C.POINTER(RefvsrConv), _P],
    'refvsr_set_conv_workgroup_cap': [_I],
    'refvsr_conv_variant': [C.POINTER(RefvsrConv), C.POINTER(C.c_int)],      # the planned kernel variant's key (added symbol, ABI 15 unchanged)
    # the same for the fixed-channel kernels (added symbols, ABI 15 unchanged): op (C24_*), x0, x1, mm, wf, batch, h, w -> key, n_tiles,
    # lds | head, wf, relu, batch, h, w, stream -> key, n_tiles, lds
    'refvsr_conv24_variant': [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'refvsr_resblock24_variant': [_I, _I, _I, _I, _I, _I, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    # and for the two other fused blocks (added symbols, ABI 15 unchanged): act_slope, batch, h, w, stream -> key, n_tiles, grid, lds |
    # c, h, w, stream -> key, n_tiles, grid, lds (grid = None: host only)
    'refvsr_resblock48_variant': [_F, _I, _I, _I, _P] + [C.POINTER(C.c_int)] * 4,
    'refvsr_resblock_lean_variant': [_I, _I, _I, _P] + [C.POINTER(C.c_int)] * 4,
    'refvsr_kslot': [_I, _I, _I, _I, _I],        # returns the slot, not a status
    'refvsr_ksteps': [_I, _I],                   # returns the K-step count
    'refvsr_set_probe': [_P, _I],
    'refvsr_resblock_lean_fits': [_I],
    'refvsr_set_resblock_waves': [_I],
    'refvsr_resblock_lean': [_P, _I, _I, _I, _P, _P, _P, _P, _I, _F, _F, _P, _P],
    'refvsr_resblock_chain': [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _P],
    'refvsr_resblock24_chain': [_P, _I, _I, _I, _P, _Z, _F, _P, _P, _P, _P],
    'refvsr_resblock48_chain': [_P, _I, _I, _I, _P, _Z, _F, _P, _P, _P, _P],
    'refvsr_resblock24_kblock': [_I, _I],        # returns the packed K-block, not a status
    'refvsr_set_resblock24_waves': [_I],
    'refvsr_set_resblock24_store': [_I],
    'refvsr_conv24_supported': [_I, _I],         # returns 0 / 1
    'refvsr_conv24_blob_bytes': [_I, _I],        # returns the size
    'refvsr_conv24_kblock': [_I, _I, _I],        # returns the packed K-block
    'refvsr_conv24': [_P, _I, _P, _I, _I, _I, _P, _F, _P, _P, _F, _P, _P],
    'refvsr_conv32_supported': [_I, _I],         # returns 0 / 1
    'refvsr_conv32_blob_bytes': [_I, _I],        # returns the size
    'refvsr_conv32': [_P, _I, _P, _I, _I, _I, _P, _F, _P, _P, _F, _P, _P],
    'refvsr_conv48_supported': [_I, _I],         # returns 0 / 1
    'refvsr_conv48_blob_bytes': [_I, _I],        # returns the size
    'refvsr_conv48': [_P, _I, _P, _I, _I, _I, _P, _F, _P, _P, _F, _P, _P],
    'refvsr_conv_shuffle2_supported': [_I],      # returns 0 / 1
    'refvsr_conv_shuffle2_blob_bytes': [_I],     # returns the size
    'refvsr_conv_shuffle2': [_P, _I, _I, _I, _P, _F, _P, _P],
    'refvsr_conv_direct_f32': [_P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _F, _P, _I, _I, _P],
    'refvsr_conv1x1_f32': [_P, _I, _I, _I, _P, _P, _F, _P, _P],
    'refvsr_pack_nhwc16': [_P, _I, _I, _I, _P, _I, _P],
    'refvsr_pack_nhwc32': [_P, _I, _I, _I, _P, _I, _P],
    'refvsr_unpack_nhwc16': [_P, _I, _I, _I, _I, _P, _P],
    'refvsr_resize': [_P, _I, _I, _I, _P, _I, _I, _I, _F, _F, _P, _P, _P, _I, _I, _I, _P],
    'refvsr_avgpool2': [_P, _I, _I, _I, _P, _P],
    'refvsr_maxpool2': [_P, _I, _I, _I, _P, _P],
    'refvsr_max2': [_P, _P, _P, _Z, _P],
    'refvsr_buffers_equal': [_P, _P, _I, _Z, _P, _P],
    'refvsr_warp_nhwc16': [_P, _I, _I, _I, _P, _I, _I, _P, _P],
    'refvsr_warp_nhwc16_up2': [_P, _I, _I, _I, _P, _I, _I, _P, _P],
    'refvsr_warp_planar': [_P, _I, _I, _I, _P, _I, _I, _P, _P],
    'refvsr_spynet_level_input': [_P, _P, _P, _I, _I, _P, _P, _P],
    'refvsr_conv_hr_last': [_P, _I, _I, _P, _F, _P, _I, _I, _P, _P],
    'refvsr_conv_last_supported': [_I],          # returns 0 / 1
    'refvsr_conv_last_blob_bytes': [_I],         # returns the size
    'refvsr_conv_last': [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P],
    'refvsr_conv_last_fmt': [_P, _I, _I, _I, _P, _P, _I, _I, _P, _I, _P],
    'refvsr_conv_hr_last_fmt': [_P, _I, _I, _P, _F, _P, _I, _I, _P, _I, _P],
    'refvsr_convert_result': [_P, _Z, _I, _P, _P],
    'refvsr_convert_result_hwc': [_P, _I, _I, _I, _P, _P],      # channels-last results (added symbol, ABI 15 unchanged)
    'refvsr_conf_alpha': [_P, _P, _I, _I, _I, _P, _P, _F, _P, _I, _F, _P, _P, _P],
    'refvsr_spynet_level_input_batch': [_P, _P, _I, _P, _I, _I, _P, _P, _P],
    # multi-map launches (ABI 11): host arrays of `batch` device pointers
    'refvsr_resblock24_chain_batch': [_P, _I, _I, _I, _I, _P, _Z, _F, _P, _P, _P, _P],
    'refvsr_resblock48_chain_batch': [_P, _I, _I, _I, _I, _P, _Z, _F, _P, _P, _P, _P],      # ABI 12
    'refvsr_conv24_batch': [_P, _I, _P, _I, _I, _I, _I, _P, _F, _P, _P, _F, _P, _P],
    'refvsr_conv_shuffle2_batch': [_P, _I, _I, _I, _I, _P, _F, _P, _P],
    'refvsr_conf_alpha_batch': [_P, _P, _I, _I, _I, _I, _P, _P, _F, _P, _I, _F, _P, _P, _P],
    'refvsr_warp_nhwc16_batch': [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P],
    'refvsr_warp_nhwc16_up2_batch': [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P],
    'refvsr_warp_planar_batch': [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P],
    'refvsr_match_patches': [_P, _I, _I, _P, _P, _P, _P],
    'refvsr_match_top2': [_P, _I, _P, _I, _I, _P, _P, _P],
    'refvsr_match_refine': [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P],
    'refvsr_match_exact': [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    'refvsr_match_naive': [_P, _I, _I, _P, _I, _I, _P, _P, _P],
    'refvsr_block_gather_nhwc16': [_P, _I, _I, _I, _P, _I, _I, _I, _P, _P],
    'refvsr_block_gather_rgb': [_P, _I, _I, _P, _I, _I, _I, _P, _P, _P],
    'refvsr_aligned_sample': [_P, _I, _I, _I, _I, _P, _P, _P],
    'refvsr_dcn_sample': [_P, _I, _I, _I, _P, _I, _P, _P],
    'refvsr_tsa_weight': [_P, _P, _P, _I, _I, _I, _P, _P],
    'refvsr_pool3s2_nhwc16': [_P, _I, _I, _I, _P, _I, _I, _I, _P],
    'refvsr_up2_bilinear_nhwc16': [_P, _I, _I, _I, _F, _P, _P],
    'refvsr_tsa_blend': [_P, _P, _P, _Z, _P, _P],
    # fp16 weight format (ABI 15): blob sizes; the _f16w twins of _F16W_TWINS follow the dict
    'refvsr_resblock24_f16w_blob_bytes': [],     # returns the size
    'refvsr_conv24_f16w_blob_bytes': [_I, _I],   # returns the size
    'refvsr_conv32_f16w_blob_bytes': [_I, _I],   # returns the size
    'refvsr_conv_shuffle2_f16w_blob_bytes': [_I],   # returns the size
    # 8-bit input frames (added symbols, ABI 15 unchanged)
    'refvsr_ingest_u8': [_P, _P, _I, _I, _I, _I, _P],
    'refvsr_ingest_table': [_P],                 # copies the 256-entry byte -> float table to host memory
    'refvsr_ingest_max_frames': [],              # returns REFVSR_INGEST_MAX_FRAMES
    'refvsr_bytes_equal': [_P, _P, _I, _Z, _P, _P],
    # frame scores on the device (added symbols, ABI 15 unchanged)
    'refvsr_score_frames': [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _P, _P],
    'refvsr_score_max_frames': [],               # returns REFVSR_SCORE_MAX_FRAMES
    # the same with the bicubic down-scale of a `down` times larger result fused in (added symbol, ABI 15 unchanged)
    'refvsr_score_frames_down': [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _Z, _P, _P],
    # rectangle sums for the field-of-view evaluation (added symbols, ABI 15 unchanged)
    'refvsr_score_regions': [_P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P, _Z, _P, _P],
    'refvsr_score_max_rects': [],                # returns REFVSR_SCORE_MAX_RECTS
    # matching rows through LDS, flagged lo rows, one-launch pyramid and frame preparation (added symbols, ABI 15 unchanged)
    'refvsr_set_match_patches_kernel': [_I],
    'refvsr_match_lo_rows': [_P, _I, _I, _P, _P, _P, _P],
    'refvsr_avgpool_pyramid': [_P, _I, _I, _I, _P, _P],
    'refvsr_frame_prep': [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    # confidence maps as images (added symbols, ABI 15 unchanged)
    'refvsr_conf_colormap': [_P, _I, _I, _I, _P, _P, _Z, _P],
    'refvsr_colormap_table': [_P],               # copies the 256 x 3 byte colour table to host memory
    # parameter fingerprint (added symbols, ABI 15 unchanged): device chunk table, chunks, workspace, its bytes, out, stream
    'refvsr_param_fingerprint': [_P, _I, _P, _Z, _P, _P],
    # Y'CbCr 4:2:0 result frames (added symbols, ABI 15 unchanged): src table, src_fmt, dst table, frames, h, w, yuv_fmt, coef9, stream
    'refvsr_result_to_yuv420': [_P, _I, _P, _I, _I, _I, _I, C.POINTER(C.c_double), _P],
    'refvsr_yuv420_max_frames': [],              # returns REFVSR_YUV420_MAX_FRAMES
    # Y'CbCr 4:2:0 input frames (added symbols, ABI 15 unchanged): src table, dst table, frames, h, w, format, chroma, coef9, stream
    'refvsr_yuv420_to_rgb': [_P, _P, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _P],
    'refvsr_yuv420_in_max_frames': [],           # returns REFVSR_YUV420_IN_MAX_FRAMES
    # luma SAD of frame pairs for the scene cuts (added symbols, ABI 15 unchanged): a table, b table, pairs, h, w, yuv_fmt, workspace,
    # its bytes, sad, stream
    'refvsr_luma_sad': [_P, _P, _I, _I, _I, _I, _P, _Z, _P, _P],
    'refvsr_scene_max_pairs': [],                # returns REFVSR_SCENE_MAX_PAIRS
    # 4:2:2 / 4:4:4 / left-sited frames (added symbols, ABI 15 unchanged): the two 4:2:0 signatures with sampling, siting behind yuv_fmt
    'refvsr_result_to_yuv': [_P, _I, _P, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _P],
    'refvsr_yuv_to_rgb': [_P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _P],
    # antialiased bicubic resize (added symbols, ABI 15 unchanged): src table, src_fmt, dst table, dst_fmt, frames, h, w, oh, ow, lo_x,
    # cnt_x, wx, lo_y, cnt_y, wy (device tables of resize.aa_taps), maxcnt_x, maxcnt_y, clamp, stream
    'refvsr_resize_aa': [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    'refvsr_resize_max_frames': [],              # returns REFVSR_RESIZE_MAX_FRAMES
    # baseline JPEG of Y'CbCr frames (added symbols, ABI 15 unchanged): src table, frames, h, w, sampling, qtables, dct, huffman LUT
    # (device tables of jpeg.py), restart, dst, its capacity, sizes, offsets (device int64), workspace, its bytes, stream
    'refvsr_jpeg_encode': [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _Z, _P, _P, _P, _Z, _P],
    'refvsr_jpeg_max_frames': [],                # returns REFVSR_JPEG_MAX_FRAMES
}
# fp16 weight format (ABI 15): <name>_f16w twins with the signature of the function they are named after
_F16W_TWINS = ('refvsr_resblock24_chain', 'refvsr_resblock24_chain_batch', 'refvsr_conv24', 'refvsr_conv24_batch', 'refvsr_conv32',
               'refvsr_conv_shuffle2', 'refvsr_conv_shuffle2_batch', 'refvsr_conf_alpha', 'refvsr_conf_alpha_batch')
SIGNATURES.update((name + '_f16w', SIGNATURES[name]) for name in _F16W_TWINS)
_SPECIAL = {'refvsr_abi_version': (C.c_int, []), 'refvsr_last_error': (C.c_char_p, []),
            'refvsr_score_workspace_bytes': (C.c_size_t, [_I, _I, _I]),
            'refvsr_score_regions_workspace_bytes': (C.c_size_t, [_I, _I, _I, _I]),
            'refvsr_conf_colormap_workspace_bytes': (C.c_size_t, [_I, _I, _I]),
            'refvsr_param_fingerprint_workspace_bytes': (C.c_size_t, [_I]),
            'refvsr_yuv420_bytes': (C.c_size_t, [_I, _I, _I]),
            'refvsr_yuv_frame_bytes': (C.c_size_t, [_I, _I, _I, _I]),
            'refvsr_luma_sad_workspace_bytes': (C.c_size_t, [_I, _I, _I]),
            'refvsr_jpeg_capacity': (C.c_size_t, [_I, _I, _I, _I]),
            'refvsr_jpeg_workspace_bytes': (C.c_size_t, [_I, _I, _I, _I, _I])}
EXPORTS = tuple(sorted(list(SIGNATURES) + list(_SPECIAL)))

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'refvsr_amd: %s not found -- the HIP extension is required (no CPU fallback). '
                'Build it with `make -C refvsr_amd/csrc` or `python -c "import __graft_entry__ as g; g.build()"`.'
                % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(h, name)
            fn.argtypes = args
            fn.restype = C.c_int
        for name, (res, args) in _SPECIAL.items():
            fn = getattr(h, name)
            fn.argtypes = args
            fn.restype = res
        for query, const, name in ((h.refvsr_abi_version, ABI_VERSION, 'ABI'), (h.refvsr_max_maps, MAX_MAPS, 'REFVSR_MAX_MAPS'),
                                   (h.refvsr_ingest_max_frames, INGEST_MAX_FRAMES, 'REFVSR_INGEST_MAX_FRAMES'),
                                   (h.refvsr_score_max_frames, SCORE_MAX_FRAMES, 'REFVSR_SCORE_MAX_FRAMES'),
                                   (h.refvsr_score_max_rects, SCORE_MAX_RECTS, 'REFVSR_SCORE_MAX_RECTS'),
                                   (h.refvsr_yuv420_max_frames, YUV420_MAX_FRAMES, 'REFVSR_YUV420_MAX_FRAMES'),
                                   (h.refvsr_yuv420_in_max_frames, YUV420_IN_MAX_FRAMES, 'REFVSR_YUV420_IN_MAX_FRAMES'),
                                   (h.refvsr_scene_max_pairs, SCENE_MAX_PAIRS, 'REFVSR_SCENE_MAX_PAIRS'),
                                   (h.refvsr_resize_max_frames, RESIZE_MAX_FRAMES, 'REFVSR_RESIZE_MAX_FRAMES'),
                                   (h.refvsr_jpeg_max_frames, JPEG_MAX_FRAMES, 'REFVSR_JPEG_MAX_FRAMES')):
            if query() != const:
                raise RuntimeError('refvsr_amd: %s mismatch (library %d, binding %d)' % (name, query(), const))
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().refvsr_last_error()
        raise RuntimeError('refvsr_hip.%s failed (rc=%d): %s' % (what, rc, msg.decode() if msg else '?'))
