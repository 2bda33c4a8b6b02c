/*
 * refvsr_hip.h -- C-ABI of the MI355X (gfx950) RefVSR inference hot path.
 *
 * The reference (codeslake/RefVSR) is pure Python + ATen ops; it has no FFI of its own.  The entry
 * points below are what a ctypes/cffi binding of the hot path binds instead of the ATen calls made
 * by models/archs/RefVSR.py:Network.forward (paths relative to the reference tree).  Every function
 * cites the reference code it replaces.  Plain pointers (device memory), ints, floats; no torch
 * types.  All kernels are enqueued on `stream` (a hipStream_t passed as void*) and return
 * immediately; 0 = success, non-zero = error (message via refvsr_last_error()).
 *
 * Device data layouts
 *   planar  : float32 [C][H][W]                  (frames, flows, confidence maps, VGG features)
 *   nhwc16  : _Float16 [H][W][Cs], Cs % 8 == 0   (all C-channel feature maps; "HWC tiles")
 * Batch size is 1 at this level (the host loops over n, as the reference's eval does).
 */
#ifndef REFVSR_HIP_H
#define REFVSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REFVSR_ABI_VERSION 15  /* 2: K-block order of packed conv weights (refvsr_amd/packing.py:kslot);
                                  3: exact matching (match_refine flagging, match_exact), lean ResBlock;
                                  4: hi + lo patch rows (match_patches rows_lo), split-fp16 match_exact;
                                  5: compile-time-specialised 24-channel ResBlock (resblock24 blob);
                                  6: RefvsrConv.warp_* (inter-frame warp fused into the conv's tile staging);
                                  7: refvsr_conv24 / refvsr_conv48 (compile-time-specialised 3x3 convs);
                                  8: RefvsrConv.f32 = 2 (plain fp16 weights in the streamed convs);
                                  9: refvsr_conv_shuffle2 (compile-time-specialised C -> 4 C conv + pixel shuffle), refvsr_conv32;
                                  10: RefvsrConv.batch (one launch over several images that share the weights),
                                      refvsr_spynet_level_input_batch, refvsr_conf_alpha, refvsr_warp_nhwc16's flow_scale;
                                  11: multi-map launches (REFVSR_MAX_MAPS maps of one geometry behind one launch and one weight fill):
                                      refvsr_resblock24_chain_batch, refvsr_conv24_batch, refvsr_conv_shuffle2_batch,
                                      refvsr_conf_alpha_batch, refvsr_warp_nhwc16_batch, refvsr_warp_nhwc16_up2_batch,
                                      refvsr_warp_planar_batch; RefvsrConv.warp_* (ABI 6: the inter-frame warp fused into a conv's tile
                                      staging) REMOVED: bit-identical to warp + conv but measured slower in every configuration
                                      (169 vs 176 frames/s, profiles/r03_fused_warp_ab.txt);
                                  12: refvsr_resblock48_chain_batch (the multi-map form of the 48-channel block);
                                  13: CU partitions: refvsr_stream_create_cu_range / refvsr_stream_set_cu_budget /
                                      refvsr_stream_destroy / refvsr_num_cus;
                                  14: result formats of the output head (REFVSR_RESULT_*): refvsr_conv_last_fmt,
                                      refvsr_conv_hr_last_fmt, refvsr_convert_result;
                                  15: the fp16 weight format (config.weight_precision = 'fp16'): *_f16w twins of the specialised
                                      entry points of the mid_channels = 24 family and their blob-size queries */

int refvsr_abi_version(void);
/* REFVSR_MAX_MAPS of the built library (a value, not a status): bindings check their own copy against it at load time. */
int refvsr_max_maps(void);
const char* refvsr_last_error(void);
/* One-time per-process setup (raises dynamic-LDS limits).  Called lazily by every entry point. */
int refvsr_init(void);

/* CU partitions (ABI 13; no reference counterpart -- the reference leaves kernel placement to the CUDA runtime).
 * The path runs three internal streams (per-frame preparation, forward branch, backward branch: models/archs/RefVSR.py:196-204 is
 * independent of :211-238 of the previous frames); kernels of two streams only run side by side if both fit a CU, which the
 * LDS-heavy kernels of this library never do.  A stream created here executes on CUs [first_cu, first_cu + n_cus) only (both
 * multiples of 8: an equal share of every XCD) and the persistent launchers of this library size their grids for n_cus CUs on it.
 * refvsr_stream_set_cu_budget overrides the CU count the launchers assume on any stream (0 = forget the stream).
 * Results never depend on the partition.  refvsr_num_cus returns the CU count of the current device (a value, not a status). */
int refvsr_num_cus(void);
int refvsr_stream_create_cu_range(int first_cu, int n_cus, void** stream);
int refvsr_stream_set_cu_budget(void* stream, int n_cus);
int refvsr_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on v_mfma_f32_16x16x32_f16, fp32 accumulate).
 * Replaces every nn.Conv2d on C-channel maps: ResidualBlocksWithInputConv (RefVSR.py:327-360),
 * ResBlock/ResList/BasicBlock (RefVSR_/common.py:25-109), PixelShufflePack (mmedit upsample.py:36-51),
 * SPyNetBasicModule (SPyNet.py:142-202), AlignedConv2d.conv1/p_conv (RefVSR_/alignment.py:18-24),
 * fusion_UP/conv_hr/conv_last (RefVSR.py:87-92), with the surrounding elementwise work fused:
 * torch.cat of two inputs, bias, (Leaky)ReLU, `x + alpha*y` (RefVSR.py:131,143), residual adds,
 * pixel_shuffle, `+ base` and clamp (RefVSR.py:118,297).
 * ------------------------------------------------------------------------------------------ */
enum { REFVSR_OUT_NHWC16 = 0, REFVSR_OUT_NHWC16_SHUFFLE2 = 1, REFVSR_OUT_PLANAR32 = 2 };

typedef struct RefvsrConv {
    const void* src0; int c0;          /* nhwc16 input, channel stride c0 (multiple of 8)            */
    const void* src1; int c1;          /* optional 2nd input concatenated after src0 (or NULL, 0)    */
    int h_in, w_in;                    /* input spatial size                                         */
    int h_out, w_out;                  /* conv output spatial size (before pixel shuffle)            */
    int ksize, stride, pad;
    const void* wpack;                 /* packed fp16 weights, see refvsr_amd/packing.py             */
    const float* bias;                 /* fp32 [n_mtiles*16], packed row order                        */
    int cout;                          /* valid output rows (packed row order)                        */
    int mt_per_block;                  /* 1, 2 or 3 sixteen-row tiles handled per block               */
    int ksteps;                        /* number of 32-deep K steps in wpack                          */
    float act_slope;                   /* y<0 ? y*slope : y   (1 = linear, 0 = ReLU)                  */
    const void* mul; int mul_c;        /* optional nhwc16 multiplier (alpha) and its channel stride   */
    const void* res; int res_c;        /* optional nhwc16 residual added after mul                    */
    float post_slope;                  /* activation applied after the residual add (1 = none)        */
    int out_mode;                      /* REFVSR_OUT_*                                                */
    void* out; int out_c;              /* nhwc16 modes: channel stride of out                          */
    const float* res_planar;           /* PLANAR32: optional planar fp32 residual [cout][h][w]        */
    int f32;                           /* 0: nhwc16 maps, fp16 hi+lo weights on 16x16x32 f16 MFMA;
                                          1: the same maps in fp32 ("nhwc32", channel stride % 4 == 0), fp32 weights,
                                             exact fp32 products on v_mfma_f32_16x16x4_f32 (src/mul/res/out all fp32);
                                          2 (ABI 8): like 0 with plain fp16 weights (no lo term; wpack [nz][S][MT][1][64][8]):
                                             half the weight stream and half the MFMAs -- streamed convs only (more than 16
                                             K-steps, stride 1, mt_per_block <= 2); used for SPyNet's 7x7 convs, whose
                                             contribution to the end-to-end error budget is measured in DESIGN.md section 2 */
    float add_const;                   /* PLANAR32: constant added after the residual                 */
    float clamp_lo, clamp_hi;          /* PLANAR32: clamp when clamp_lo < clamp_hi                    */
    /* Batch (ABI 10): batch > 1 runs the same conv over `batch` images in ONE launch (blockIdx.y = image); image b reads
     * src0 + b * bs_src0 (src1 + b * bs_src1) and writes out + b * bs_out, res_planar + b * bs_res_planar (byte strides).
     * mul / res must be NULL then.  batch = 0 or 1: a single image (strides ignored).  Used for the two SPyNet
     * flows a frame needs (SPyNet.py:49-104 is called per pair by the reference; same weights, same shapes): the coarse
     * pyramid levels are launches of 2-36 workgroups, two images per launch fill twice the CUs for the same latency. */
    int batch; size_t bs_src0, bs_src1, bs_out, bs_res_planar;
} RefvsrConv;

int refvsr_conv_mfma(const RefvsrConv* d, void* stream);
/* Tuning / test knob (no reference counterpart): upper bound on the workgroups one single-chunk conv launches; each
 * workgroup walks the remaining pixel tiles.  0 = automatic (occupancy x CUs).  Results do not depend on it. */
int refvsr_set_conv_workgroup_cap(int cap);
/* Test query (added symbol, ABI 15 unchanged; no reference counterpart): which conv_mfma_kernel instantiation refvsr_conv_mfma
 * would launch for `d` under this process's REFVSR_CONV_* knobs, as the packed key of refvsr_amd/csrc/conv_plan.h
 * (conv_variant_key: MT | TILES << 2 | NW << 6 | EPI << 11 | F32 << 12 | GATHER << 13 | RESIDENT << 14 | HI1 << 15).  The same
 * plan function and the same knob object as the launcher.  Host only: no launch, no device call.  A descriptor the launcher
 * rejects is rejected here with the same message (returns 1). */
int refvsr_conv_variant(const RefvsrConv* d, int* key);
/* The same for the fixed-channel kernels (added symbols, ABI 15 unchanged; no reference counterpart; host only: no launch, no
 * refvsr_init -- the block query asks for the device's CU count where `stream` has no CU budget, as its launcher does).  `op` names
 * the entry point and gives (x0, x1) their meaning: */
enum {
    REFVSR_C24_CONV24 = 0,      /* refvsr_conv24*:        (c0, c1) input channels of the two sources                     */
    REFVSR_C24_CONV32 = 1,      /* refvsr_conv32*:        (c0, c1)                                                       */
    REFVSR_C24_CONV48 = 2,      /* refvsr_conv48:         (c0, c1)                                                       */
    REFVSR_C24_SHUFFLE2 = 3,    /* refvsr_conv_shuffle2*: (c, 0)                                                         */
    REFVSR_C24_CONF_ALPHA = 4,  /* refvsr_conf_alpha*:    (cout, up); h x w = the confidence maps                        */
    REFVSR_C24_CONV_LAST = 5    /* refvsr_conv_last*:     (c, 0)                                                         */
};
/* refvsr_conv24_variant: which conv24_kernel instantiation that entry point (mm = 1: its `_batch` form over `batch` maps, wf = 1: its
 * `_f16w` twin) would launch on h x w maps under this process's REFVSR_CONV48_WAVES, as the packed key of
 * refvsr_amd/csrc/fixed_plan.h (c24_variant_key: COUT | NCG0 << 6 | NCG1 << 10 | NWV << 14 | TH << 19 | WPS << 24 | SHUF << 27 |
 * CONF << 33 | HALF << 35 | MM << 36 | WF << 37), with the launch's tile count and dynamic LDS bytes (n_tiles, lds: optional).  The
 * same plan function and the same knob object as the entry points, whose first failing shape check it reports with their message;
 * a shape without a kernel in the asked weight format is an error with the message the dispatch gives (returns 1).
 * refvsr_resblock24_variant: which resblock24_kernel instantiation a refvsr_resblock24_chain* launch over `batch` maps (head = 0; wf,
 * relu = act_slope == 0) or refvsr_conv_hr_last (head = 1) would run on `stream` right now -- under refvsr_set_resblock24_waves /
 * _store, a probe buffer being set (refvsr_set_probe) and the CU budget of `stream` -- as rb24_variant_key: RELU | NWV << 1 |
 * PROBE << 6 | TH << 7 | STORE << 12 | HEAD << 13 | WF << 14. */
int refvsr_conv24_variant(int op, int x0, int x1, int mm, int wf, int batch, int h, int w, long long* key, int* n_tiles, int* lds);
int refvsr_resblock24_variant(int head, int wf, int relu, int batch, int h, int w, void* stream, int* key, int* n_tiles, int* lds);
/* The same for the two other fused-block kernels (added symbols, ABI 15 unchanged).  refvsr_resblock48_variant: which
 * resblock48_kernel<RELU, PROBE> a refvsr_resblock48_chain* launch over `batch` maps would run right now, as RELU | PROBE << 1 (RELU =
 * act_slope == 0; PROBE = a probe buffer is set (refvsr_set_probe) AND RELU: the leaky kernel has no probe form).
 * refvsr_resblock_lean_variant: which resblock_lean_kernel<MT, WIDE, NWV> refvsr_resblock_lean / refvsr_resblock_chain would run on
 * c-channel maps under refvsr_set_resblock_waves, as MT | WIDE << 2 | NWV << 3.  n_tiles, lds (dynamic LDS bytes) and grid (the
 * workgroups a launch on `stream` would get: min(n_tiles, CUs of the stream x occupancy, a multiple of 8, at least 8)) are optional.
 * The launchers plan through the same function.  With grid == NULL the query is host only (no launch, no refvsr_init); with it the
 * kernel's LDS attribute is set and, for the lean kernel, the runtime is asked for its occupancy, as at a launch. */
int refvsr_resblock48_variant(float act_slope, int batch, int h, int w, void* stream, int* key, int* n_tiles, int* grid, int* lds);
int refvsr_resblock_lean_variant(int c, int h, int w, void* stream, int* key, int* n_tiles, int* grid, int* lds);
/* Packing contract of `wpack` (host-side helpers, no GPU needed): K-slot of K-block (ty, tx, cg) of a ks x ks conv over
 * ncg 16-byte channel groups, and the number of 4-slot K-steps; refvsr_amd/packing.py:kslot/ksteps are the same closed
 * forms and tests/test_capi.py pins the two against each other.  Return the value (>= 0), not a status. */
int refvsr_kslot(int ty, int tx, int cg, int ksize, int ncg);
int refvsr_ksteps(int ksize, int ncg);

/* Fused residual block  out = post( x + conv2( act( conv1(x) ) ) ),  3x3, C -> C, stride 1, in ONE launch (the intermediate map
 * lives in LDS): ResidualBlockNoBN (mmedit sr_backbone_utils.py:42-97) and ResBlock (RefVSR_/common.py:25-39).  w1 / w2: fp16 hi + lo
 * packed weights of the two convs, b1 / b2 packed biases.  Runtime-generic kernel for C in {8, 16, 24, 32} (refvsr_resblock_lean_fits):
 * 8 waves on an 8 x 32 tile, both weight sets + one activation tile in LDS (the intermediate map overwrites the input tile): two
 * workgroups per CU, so one's epilogue runs under the other's MFMAs.  Same arithmetic as two refvsr_conv_mfma launches up to fp32 summation order.  Slopes must
 * lie in [0, 1].  (Round 1's 16 x 32-tile kernel, refvsr_resblock_mfma, was the reference of the bit-identity tests until round 4 and
 * is gone: every shape it ran is covered by this kernel and by refvsr_resblock24_chain.) */
int refvsr_resblock_lean_fits(int c);
/* n fused blocks behind one call (n launches, intermediates ping-pong between scratch0 / scratch1: each [h][w][c] fp16,
 * scratch0 needed for n >= 2, scratch1 for n >= 3; src, scratch*, out pairwise distinct).  w1 / b1 / w2 / b2: host arrays of
 * n device pointers.  Same results as n calls of refvsr_resblock_lean; saves n - 1 FFI crossings and n - 2 allocations. */
int refvsr_resblock_chain(const void* src, int c, int h, int w, int n, const void* const* w1, const float* const* b1,
                          const void* const* w2, const float* const* b2, int ksteps, float act_slope, float post_slope,
                          void* scratch0, void* scratch1, void* out, void* stream);
/* Tuning knob: waves per workgroup of the lean kernel, 8 (default: half the tiles per wave, <= 128 VGPRs, four waves per
 * SIMD) or 4.  Results do not depend on it. */
int refvsr_set_resblock_waves(int waves);
int refvsr_resblock_lean(const void* src, int c, int h, int w, const void* w1, const float* b1,
                         const void* w2, const float* b2, int ksteps, float act_slope, float post_slope,
                         void* out, void* stream);
/* The 24-channel fused block of RefVSR_small (mid_channels = 24: configs/config_RefVSR_small_*.py) with every geometry
 * constant fixed at compile time -- ResidualBlockNoBN (mmedit sr_backbone_utils.py:42-97, act_slope 0 = ReLU) and ResBlock
 * (RefVSR_/common.py:25-39, act_slope 0.2), out = x + conv2(act(conv1 x)), n blocks behind one call like
 * refvsr_resblock_chain.  Block i's parameters are ONE blob of REFVSR_RESBLOCK24_BLOB_BYTES at blobs + i * blob_stride
 * (device memory, 16-byte aligned): [conv1: 7 K-steps x 3 fragments x 64 lanes x 8 halfs][conv2: same][b1: 32 floats,
 * 24..31 = 0][b2: 32 floats]; fragments 0 / 1 = hi / lo halves of output channels 0-15, fragment 2 = rows 0-7 hi, rows 8-15
 * lo of channels 16-23; lane l = (q = l >> 4, row r = l & 15) holds K-block refvsr_resblock24_kblock(s, q) of row r
 * (refvsr_amd/packing.py:pack_resblock24 builds it).  Same arithmetic as refvsr_resblock_lean up to fp32 summation order. */
#define REFVSR_RESBLOCK24_BLOB_BYTES 43264
int refvsr_resblock24_chain(const void* src, int h, int w, int n, const void* blobs, size_t blob_stride, float act_slope,
                            void* scratch0, void* scratch1, void* out, void* stream);
/* Multi-map launches (ABI 11).  The propagation branches of CONSECUTIVE output frames are independent chains over identical
 * weights (the backward branch restarts from zeros in every window, RefVSR.py:211-238), and so are the n samples of a batch
 * (lrs [n,t,3,h,w], RefVSR.py:151): `batch` <= REFVSR_MAX_MAPS maps of one geometry run behind ONE launch per layer.  A workgroup
 * walks its share of the batch x tiles on one weight fill (at 270 x 480 a launch is one 8 x 32 tile per workgroup and a third of its
 * life is the fill).  Maps are given as HOST arrays of `batch` device pointers (they need not be contiguous: per-frame cached maps
 * enter the chains).  Map b of a batched call == the single-map call on map b, bit for bit (tests/test_gpu_ops.py). */
#define REFVSR_MAX_MAPS 4
/* refvsr_resblock24_chain over `batch` maps: src / out host arrays of batch pointers ([h][w][24] fp16 each), scratch0 / scratch1:
 * [batch][h][w][24] contiguous (needed as in the single-map call). */
int refvsr_resblock24_chain_batch(const void* const* src, int batch, int h, int w, int n, const void* blobs, size_t blob_stride,
                                  float act_slope, void* scratch0, void* scratch1, void* const* out, void* stream);
/* (ty << 16 | tx << 8 | cg) of K-block (K-step s = 0..6, quarter q = 0..3) of the blob's K order, -1 for the zero block. */
int refvsr_resblock24_kblock(int s, int q);
/* The fp16 weight format (ABI 15; config.weight_precision = 'fp16').  Every _f16w function below has the
 * signature of the function it is named after and takes blobs with plain fp16 weights in ONE fragment per 16 output rows -- no lo
 * halves, no fold: resblock24 [conv1: 7 K-steps x 2 fragments (rows 0-15, rows 16-23 + 8 zero rows) x 64 lanes x 8 halfs][conv2: same]
 * [b1: 32 floats][b2: 32 floats] = REFVSR_RESBLOCK24_F16W_BLOB_BYTES (refvsr_amd/packing.py:pack_resblock24_f16w); conv24 / conv32 /
 * conv_shuffle2: 2 / 2 / 3 fragments per K-step with the bias tails of the hi + lo layout (refvsr_*_f16w_blob_bytes).  Same K order,
 * accumulator initial values and fold order as the hi + lo kernels: on weights w with fp16(w) == w the results are bit-identical to
 * the hi + lo entry points (whose lo MFMAs then add exact zeros), with two thirds (24 outputs) or half (32 | 48) of the MFMAs. */
#define REFVSR_RESBLOCK24_F16W_BLOB_BYTES 28928
int refvsr_resblock24_f16w_blob_bytes(void);
int refvsr_resblock24_chain_f16w(const void* src, int h, int w, int n, const void* blobs, size_t blob_stride, float act_slope,
                                 void* scratch0, void* scratch1, void* out, void* stream);
int refvsr_resblock24_chain_batch_f16w(const void* const* src, int batch, int h, int w, int n, const void* blobs, size_t blob_stride,
                                       float act_slope, void* scratch0, void* scratch1, void* const* out, void* stream);
/* Tuning knob: workgroup shape of the 24-channel kernel.  0 (default): by map size -- 8 waves on 8 x 32-pixel tiles, or 16
 * waves on 16 x 32 tiles (one workgroup per CU) when the map has at least four 8 x 32 tiles per CU; 4 | 8 | 16 force a
 * shape.  Results do not depend on it (bit-identical). */
int refvsr_set_resblock24_waves(int waves);
/* The 48-channel fused block (ABI 10; mid_channels = 48: configs/config_RefVSR_{L1,MFID,MFID_8K}.py, 30 ResidualBlockNoBN per
 * branch + the ResBlocks of the ResLists): out = x + conv2(act(conv1 x)) in ONE launch per block.  One conv's 84 KB of hi + lo
 * fragments is resident at a time; the two sets swap per 8 x 32-pixel tile by LDS-DMA under the phases that do not read them
 * (csrc/resblock48.hip).  Block i's parameters are ONE blob of REFVSR_RESBLOCK48_BLOB_BYTES at blobs + i * blob_stride:
 * [conv1: 14 K-steps x 6 fragments x 64 lanes x 8 halfs][conv2: same][b1: 64 floats, 48.. = 0][b2: 64 floats] -- the fragment
 * parts of the two refvsr_conv48 blobs (K-blocks by refvsr_conv24_kblock(6, s, q)); refvsr_amd/packing.py:pack_resblock48.
 * Same arithmetic as two refvsr_conv48 launches (bit-identical: same K order, same fp16 rounding of the intermediate). */
#define REFVSR_RESBLOCK48_BLOB_BYTES 172544
int refvsr_resblock48_chain(const void* src, int h, int w, int n, const void* blobs, size_t blob_stride, float act_slope,
                            void* scratch0, void* scratch1, void* out, void* stream);
/* refvsr_resblock48_chain over `batch` <= REFVSR_MAX_MAPS maps of one geometry (ABI 12; the backward branches of consecutive output
 * frames of the mid_channels = 48 models, like refvsr_resblock24_chain_batch): ONE launch per block over all maps -- the launch's fixed
 * cost, the first 86 KB weight fill and the tail are shared (the two weight sets still swap per tile).  src / out: host arrays of
 * batch device pointers ([h][w][48] fp16 each), scratch0 / scratch1: [batch][h][w][48] contiguous.  Map b == the single-map call on
 * map b, bit for bit. */
int refvsr_resblock48_chain_batch(const void* const* src, int batch, int h, int w, int n, const void* blobs, size_t blob_stride,
                                  float act_slope, void* scratch0, void* scratch1, void* const* out, void* stream);
/* Tuning knob: how the 24-channel kernel stores its output tile.  0: 8-byte stores (one per lane and pixel group); 1: 16-byte
 * stores after a v_permlane16_swap exchange between neighbouring lane rows (half the store instructions; default).  Results do not
 * depend on it (bit-identical). */
int refvsr_set_resblock24_store(int mode);
/* 3x3 stride-1 pad-1 convolutions with 24 output channels on fp16 HWC maps, compile-time specialised like the block above
 * (csrc/conv24.hip): the ResList tails (RefVSR_/common.py:80-82), feat_fusion / conf_fusion / fusion_UP convs (RefVSR.py:47-62,87),
 * ref encoders, conv_hr and the input conv of ResidualBlocksWithInputConv (RefVSR.py:340-343) of the mid_channels = 24 family.
 * out = post( act(conv(cat[src0, src1]) + bias) * mul + res ); (c0, c1) in {(24,0), (16,0), (8,24), (24,24)} = channel strides of
 * the sources (src1 NULL when c1 = 0); out / mul / res: 24-channel maps [h][w][24] fp16 (mul, res optional).  blob: the conv's
 * parameters, refvsr_conv24_blob_bytes(c0, c1) bytes, 16-byte aligned: [S K-steps x 3 fragments x 64 lanes x 8 halfs][32 bias
 * floats]; fragment rows as in the resblock24 blob, lane (q, r) of K-step s holds K-block refvsr_conv24_kblock(ncg, s, q)
 * (ty << 16 | tx << 8 | cg over the (c0 + c1) / 8 channel groups of the concatenated sources; -1 = zero block);
 * refvsr_amd/packing.py:pack_conv24 builds it.  Same arithmetic as refvsr_conv_mfma up to fp32 summation order. */
int refvsr_conv24_supported(int c0, int c1);
int refvsr_conv24_blob_bytes(int c0, int c1);
int refvsr_conv24_kblock(int ncg, int s, int q);
int refvsr_conv24(const void* src0, int c0, const void* src1, int c1, int h, int w, const void* blob, float act_slope,
                  const void* mul, const void* res, float post_slope, void* out, void* stream);
/* refvsr_conv24 over `batch` maps (ABI 11; 24 output channels): every per-map operand is a host array of `batch` device pointers --
 * src0, src1 (NULL array when c1 = 0), mul / res (NULL array = none; else every entry non-NULL), out. */
int refvsr_conv24_batch(const void* const* src0, int c0, const void* const* src1, int c1, int batch, int h, int w, const void* blob,
                        float act_slope, const void* const* mul, const void* const* res, float post_slope, void* const* out,
                        void* stream);
/* The output head in ONE launch (ABI 10): RefVSR.py:92,118,288,297 --
 *   out = clamp( conv_last(src) + clamp(F.interpolate(lr_centre, scale_factor=scale, mode='bicubic'), 0, 1), 0, 1 )
 * -- planar fp32 [3][h][w].  src: fp16 HWC [h][w][c], c = 24 | 48; base_lr: planar fp32 [3][bh][bw], h / bh == w / bw = the SR factor;
 * blob: refvsr_conv_last_blob_bytes(c) bytes = [S K-steps x ONE fragment x 64 lanes x 8 halfs][32 bias floats], fragment rows
 * 0-2 = hi(W[r]), rows 8-10 = lo(W[r - 8]) (folded by the kernel), K-blocks by refvsr_conv24_kblock(c / 8, s, q);
 * refvsr_amd/packing.py:pack_conv_last.  The base map (refvsr_resize bicubic x4: 25 MB written and read back at 1080p) is
 * evaluated per output value instead.  Same arithmetic as refvsr_resize + refvsr_conv_mfma's planar mode up to the fp32
 * summation order of the conv. */
int refvsr_conv_last_supported(int c);
int refvsr_conv_last_blob_bytes(int c);
int refvsr_conv_last(const void* src, int c, int h, int w, const void* blob, const float* base_lr, int bh, int bw,
                     float* out, void* stream);
/* conv_hr AND the head in one launch (ABI 10; mid_channels = 24): RefVSR.py:91-92,116-118,288,297 --
 *   out = clamp( conv_last( lrelu_{act_slope}( conv_hr(src) ) ) + clamp(F.interpolate(lr_centre, bicubic), 0, 1), 0, 1 )
 * on the two-conv skeleton of refvsr_resblock24_chain: the intermediate HR map (100 MB at 1080 x 1920) stays in LDS.  src: fp16
 * HWC [h][w][24]; blob: REFVSR_RESBLOCK24_BLOB_BYTES in the block layout with conv1 = conv_hr and conv2's fragment slot (s, 0) =
 * [rows 0-2: hi(W_last), rows 8-10: lo(W_last)], slots (s, 1), (s, 2) zero, b1 = conv_hr's bias, b2 = [b_last, 0 ...]
 * (refvsr_amd/packing.py:pack_conv_hr_last); base_lr / out as in refvsr_conv_last. */
int refvsr_conv_hr_last(const void* src, int h, int w, const void* blob, float act_slope, const float* base_lr, int bh, int bw,
                        float* out, void* stream);
/* Result formats of the output head (ABI 14; extension -- the reference returns fp32 and its consumers quantise on the CPU:
 * evaluation/eval_qual_quan.py:117-119 hands cv2.imwrite `output * 255`, i.e. saturate_cast<uchar> = round to nearest even).
 * The _fmt forms of the two head launches store the planar [3][h][w] result as fp32 (== the plain forms), fp16, or uint8 =
 * rint(255 v) of the clamped fp32 value -- the bytes the reference's PNG writer produces -- so that 1/2 or 1/4 of the bytes cross
 * PCIe; refvsr_convert_result does the same conversion on an fp32 result (the generic head of configurations without a fused one). */
enum { REFVSR_RESULT_F32 = 0, REFVSR_RESULT_F16 = 1, REFVSR_RESULT_U8 = 2 };
/* Channels-last results (extension, no ABI bump: an added flag bit and an added symbol; without the bit every entry point behaves as
 * before).  REFVSR_RESULT_HWC is OR-ed into an `out_fmt` argument: the 3 x h x w result is then the dense interleaved array
 * [h][w][3] -- element (y w + x) 3 + c instead of c h w + y w + x -- which is what image writers, encoders and raw-video pipes
 * consume (the layout REFVSR_INGEST_HWC names on the way in).  The layout decides the address alone: every value and its rounding
 * are those of the planar result, bit for bit.
 *   refvsr_conv_last_fmt / refvsr_conv_hr_last_fmt: `out` is [h][w][3] of the format's samples; one element per lane, the three
 *     channels of a pixel from neighbouring lane quarters (48 contiguous bytes per 16-pixel group at uint8).  Only element stores:
 *     `out` needs the natural alignment of its samples, for any w;
 *   refvsr_convert_result_hwc(src, h, w, out_fmt, out, stream): the generic head -- planar fp32 [3][h][w] `src` -> interleaved
 *     [h][w][3] fp32 | fp16 | uint8 with the fused heads' clamp and rounding (refvsr_convert_result has no geometry argument);
 *     out_fmt with or without the bit, src 4-byte aligned, out naturally aligned, src != out, 3 h w < 2^31;
 *   refvsr_score_frames / refvsr_score_frames_down / refvsr_score_regions: out_fmt | REFVSR_RESULT_HWC reads interleaved results (at
 *     down = 2 | 4: [down h][down w][3]).  Only the staging index changes; the order of summation depends on position alone, so the
 *     scores and sums are the float64 bits of the planar frame of the same values.
 * Any other bit in an out_fmt is refused ("unknown result format"). */
#define REFVSR_RESULT_FMT_MASK 0x0f
#define REFVSR_RESULT_HWC 0x10
int refvsr_convert_result_hwc(const float* src, int h, int w, int out_fmt, void* out, void* stream);
int refvsr_conv_last_fmt(const void* src, int c, int h, int w, const void* blob, const float* base_lr, int bh, int bw,
                         void* out, int out_fmt, void* stream);
int refvsr_conv_hr_last_fmt(const void* src, int h, int w, const void* blob, float act_slope, const float* base_lr, int bh, int bw,
                            void* out, int out_fmt, void* stream);
int refvsr_convert_result(const float* src, size_t n, int out_fmt, void* out, void* stream);

/* The confidence fusions in ONE launch (ABI 10): conf_fusion / conf_fusion2 / conf_fusion_BWFW of RefVSR.py:47-52, called at
 * :130, :141-142 and :107-109 as  conv_{16->C}(lrelu(conv_{2->16}(cat[conf_a, conf_b])))  on the LR grid (up = 1) and on
 * clamp(F.interpolate(cat[conf_a, conf_b], scale_factor=2, mode='bicubic'), 0, 1) (up = 2).  conf_a / conf_b: planar fp32
 * [h][w]; w0 / b0: the 2 -> 16 conv's fp32 weights [16][2][3][3] / bias [16] (device); blob: the 16 -> cout blob of refvsr_conv24 /
 * refvsr_conv48 (cout = 24 | 48); alpha: fp16 HWC [up h][up w][cout]; conf_max (optional, up = 1 only): max(conf_a, conf_b)
 * [h][w], the propagated confidence of RefVSR.py:147.  The 16-channel map, the concatenated and the up-sampled pair never
 * exist in HBM; results are bit-identical to torch.cat + [refvsr_resize +] refvsr_conv_direct_f32 + refvsr_conv24/48
 * [+ refvsr_max2] (tests/test_gpu_ops.py). */
int refvsr_conf_alpha(const float* conf_a, const float* conf_b, int h, int w, int up, const float* w0, const float* b0,
                      float slope0, const void* blob, int cout, float slope1, void* alpha, float* conf_max, void* stream);
/* refvsr_conf_alpha over `batch` map pairs (ABI 11, cout = 24): conf_a / conf_b / alpha / conf_max (NULL array = none) are host
 * arrays of `batch` device pointers. */
int refvsr_conf_alpha_batch(const float* const* conf_a, const float* const* conf_b, int batch, int h, int w, int up, const float* w0,
                            const float* b0, float slope0, const void* blob, int cout, float slope1, void* const* alpha,
                            float* const* conf_max, void* stream);
/* The same for 48 output channels (mid_channels = 48: configs/config_RefVSR_{L1,MFID,MFID_8K}.py -- the two convs of every
 * ResidualBlockNoBN, sr_backbone_utils.py:42-97, and conf_fusion*.1): (c0, c1) in {(48,0), (16,0)}; out / mul / res are
 * 48-channel maps; blob: [S x 6 fragments x 64 lanes x 8 halfs][64 bias floats], fragments [hi | lo] of output channels 0-15,
 * 16-31, 32-47, K-blocks by refvsr_conv24_kblock(ncg, s, q).  48 -> 48 keeps its 84 KB weight set resident next to a
 * 16 x 32-pixel tile walked by sixteen waves (one workgroup per CU).
 * Two-source forms (ABI 10): (8, 48) -- the input conv of ResidualBlocksWithInputConv on cat([lr, feat]), RefVSR.py:340-343: the
 * same blob layout on the ncg = 7 plan (18 K-steps, one zero block per tap) -- and (48, 48) -- feat_fusion*.0 / feat_fusion2_1 /
 * fusion_UP on cat([a, b]), RefVSR.py:53-62,87: one conv's 166 KB of weights have no resident form, so the OUTPUT channels are
 * computed in two halves of 24 on blockIdx.y; blob = two blobs of the 24-output layout (refvsr_conv24's: [27 K-steps x 3 fragments
 * x 64 lanes x 8 halfs][32 bias floats], ncg = 12 plan) for channels 0-23 and 24-47, back to back. */
/* The same for 32 output channels (AlignedConv2d, RefVSR_/alignment.py:18-24,53-100: the RGB stem and the 32 -> 32 convs of its
 * ResBlocks, at the 2x / HD resolutions): (c0, c1) in {(32,0), (8,0)}; blob: [S x 4 fragments x 64 lanes x 8 halfs][32 bias floats],
 * fragments [hi | lo] of output channels 0-15, 16-31. */
int refvsr_conv32_supported(int c0, int c1);
int refvsr_conv32_blob_bytes(int c0, int c1);
int refvsr_conv32(const void* src0, int c0, const void* src1, int c1, int h, int w, const void* blob, float act_slope,
                  const void* mul, const void* res, float post_slope, void* out, void* stream);
int refvsr_conv48_supported(int c0, int c1);
int refvsr_conv48_blob_bytes(int c0, int c1);
int refvsr_conv48(const void* src0, int c0, const void* src1, int c1, int h, int w, const void* blob, float act_slope,
                  const void* mul, const void* res, float post_slope, void* out, void* stream);
/* PixelShufflePack (mmedit upsample.py:36-51; RefVSR.py:89-90 upsample1 / upsample2, used at :114,116,138): the C -> 4 C 3x3 conv
 * and F.pixel_shuffle(2) in one launch of the same kernel family, C = 24 | 48: src [h][w][C] fp16 HWC -> out [2h][2w][C], bias +
 * optional leaky activation (act_slope in [0, 1], 1 = none: it commutes with the shuffle, RefVSR.py:116).  blobs: refvsr_conv_shuffle2_blob_bytes(C) bytes = 2 (C = 24) or 4 (C = 48) conv48-style blobs of 48 output rows each,
 * back to back, rows ordered sub-pixel-major: C = 24: blob z = output row parity dy, rows [dx = 0: channels 0-23][dx = 1: 0-23]
 * (row R of blob z = weight row 4 (R % 24) + 2 z + R / 24 of the reference conv); C = 48: blob z = sub-pixel 2 dy + dx, row R =
 * weight row 4 R + z (refvsr_amd/packing.py:pack_conv_shuffle2).  Same arithmetic as refvsr_conv_mfma's SHUFFLE2 output mode
 * up to fp32 summation order. */
int refvsr_conv_shuffle2_supported(int c);
int refvsr_conv_shuffle2_blob_bytes(int c);
int refvsr_conv_shuffle2(const void* src, int c, int h, int w, const void* blobs, float act_slope, void* out, void* stream);
/* refvsr_conv_shuffle2 over `batch` maps (ABI 11, c = 24): src / out host arrays of `batch` device pointers. */
int refvsr_conv_shuffle2_batch(const void* const* src, int batch, int c, int h, int w, const void* blobs, float act_slope,
                               void* const* out, void* stream);
/* fp16-weight twins of the conv24 family (ABI 15, see refvsr_resblock24_chain_f16w): the shapes of the mid_channels = 24 models --
 * conv_shuffle2 c = 24 only, conf_alpha cout = 24 only (-1 / an error otherwise). */
int refvsr_conv24_f16w_blob_bytes(int c0, int c1);
int refvsr_conv32_f16w_blob_bytes(int c0, int c1);
int refvsr_conv_shuffle2_f16w_blob_bytes(int c);
int refvsr_conv24_f16w(const void* src0, int c0, const void* src1, int c1, int h, int w, const void* blob, float act_slope,
                       const void* mul, const void* res, float post_slope, void* out, void* stream);
int refvsr_conv24_batch_f16w(const void* const* src0, int c0, const void* const* src1, int c1, int batch, int h, int w, const void* blob,
                             float act_slope, const void* const* mul, const void* const* res, float post_slope, void* const* out,
                             void* stream);
int refvsr_conv32_f16w(const void* src0, int c0, const void* src1, int c1, int h, int w, const void* blob, float act_slope,
                       const void* mul, const void* res, float post_slope, void* out, void* stream);
int refvsr_conv_shuffle2_f16w(const void* src, int c, int h, int w, const void* blobs, float act_slope, void* out, void* stream);
int refvsr_conv_shuffle2_batch_f16w(const void* const* src, int batch, int c, int h, int w, const void* blobs, float act_slope,
                                    void* const* out, void* stream);
int refvsr_conf_alpha_f16w(const float* conf_a, const float* conf_b, int h, int w, int up, const float* w0, const float* b0,
                           float slope0, const void* blob, int cout, float slope1, void* alpha, float* conf_max, void* stream);
int refvsr_conf_alpha_batch_f16w(const float* const* conf_a, const float* const* conf_b, int batch, int h, int w, int up, const float* w0,
                                 const float* b0, float slope0, const void* blob, int cout, float slope1, void* const* alpha,
                                 float* const* conf_max, void* stream);
/* Debug knob (no reference counterpart): when buf != NULL every workgroup of the PROBE instantiations of the fused-block kernels records s_memtime
 * stamps (entry, loads issued, loads landed, conv1 K loop, conv1 epilogue, barrier, conv2 K loop, stores issued) of its
 * iter-th tile at buf[12 * workgroup + i] (uint64; [8], [9] = 100 MHz s_memrealtime at entry / exit, [10] = s_memtime at exit) -- tools/probe_resblock.py.  NULL switches it off (default). */
int refvsr_set_probe(void* buf, int iter);

/* fp32 direct convolution on planar maps (VGG feature extractor + MeanShift of FeatureMatching,
 * attention.py:28-50,62-70, and the 2->16 confidence convs RefVSR.py:47-52).  Kept in fp32 because
 * the arg-max of the matching is discontinuous in these features.
 * w: fp32 [cout][cin][k][k]; out: planar fp32 [cout][ho][wo] or nhwc16 [ho][wo][out_c]. */
int refvsr_conv_direct_f32(const float* src, int cin, int h, int w,
                           const float* wgt, const float* bias, int cout, int ksize, int stride, int pad,
                           float act_slope, void* out, int out_nhwc16, int out_c, void* stream);
/* 1x1 conv cin -> 16 + LeakyReLU in fp32 (ABI 10): the map64 / map128 block that ends the matching's feature extractor
 * (RefVSR_/attention.py:41-42).  src: fp32 HWC [h][w][cin] (cin % 4 == 0, the f32 conv mode's output), wgt: fp32 [16][cin], bias [16];
 * out: planar fp32 [16][h][w].  Channels are summed in order with fp32 FMAs. */
int refvsr_conv1x1_f32(const float* src, int cin, int h, int w, const float* wgt, const float* bias, float act_slope,
                       float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Layout conversion
 * ------------------------------------------------------------------------------------------ */
/* planar fp32 [c][h][w] -> nhwc16 [h][w][cs] (channels >= c zero-filled). */
int refvsr_pack_nhwc16(const float* src, int c, int h, int w, void* dst, int cs, void* stream);
/* planar fp32 [c][h][w] -> fp32 HWC [h][w][cs], cs % 4 == 0 (input of the f32 conv mode). */
int refvsr_pack_nhwc32(const float* src, int c, int h, int w, float* dst, int cs, void* stream);
/* nhwc16 [h][w][cs] -> planar fp32 [c][h][w]. */
int refvsr_unpack_nhwc16(const void* src, int h, int w, int cs, int c, float* dst, void* stream);

/* ------------------------------------------------------------------------------------------
 * Resampling (F.interpolate / avg_pool2d / max_pool2d call sites)
 * ------------------------------------------------------------------------------------------ */
enum { REFVSR_RS_BICUBIC = 0, REFVSR_RS_BILINEAR = 1, REFVSR_RS_BILINEAR_AC = 2, REFVSR_RS_NEAREST = 3 };
/* dst = post(interp(src)); post: (v - mean[c]) / std[c] if mean != NULL (host arrays of c floats),
 * then v * mul, then clamp to [0,1] if clamp01.  src_scale_{y,x}: source step per output sample
 * (1/scale_factor, or in/out when the reference passes size=); ignored for BILINEAR_AC.
 * dst is planar fp32 [c][oh][ow], or nhwc16 [oh][ow][out_c] when out_nhwc16 != 0. */
int refvsr_resize(const float* src, int c, int h, int w, void* dst, int oh, int ow, int mode,
                  float src_scale_y, float src_scale_x, const float* mean, const float* std,
                  const float* chan_mul, int clamp01, int out_nhwc16, int out_c, void* stream);
int refvsr_avgpool2(const float* src, int c, int h, int w, float* dst, void* stream);
int refvsr_maxpool2(const float* src, int c, int h, int w, float* dst, void* stream);
/* Five refvsr_avgpool2 calls in one launch (added symbol, ABI 15 unchanged): src planar fp32 [c][h][w] with h, w multiples of 32;
 * dst: host array of five device pointers, dst[k] = planar [c][h >> (k + 1)][w >> (k + 1)], each level pooled from the stored
 * values of the one before.  The same bits as the five calls. */
int refvsr_avgpool_pyramid(const float* src, int c, int h, int w, float* const* dst, void* stream);
/* Everything the per-frame preparation derives from the two planar fp32 frames lr [3][h][w] and ref [3][hr][wr] alone, in one
 * launch (added symbol, ABI 15 unchanged): lr8 [h][w][8], ref8 [hr][wr][8] = refvsr_pack_nhwc16(., cs = 8); lr_n [h][w][4] =
 * refvsr_pack_nhwc32(MeanShift(lr), cs = 4); ref_n [hr/2][wr/2][4] = refvsr_pack_nhwc32(refvsr_avgpool2(MeanShift(ref)), cs = 4),
 * MeanShift = refvsr_conv_direct_f32 with the 1x1 filter wgt [3][3] / bias [3] (device, fp32).  The same bits as those launches. */
int refvsr_frame_prep(const float* lr, int h, int w, const float* ref, int hr, int wr, const float* wgt, const float* bias,
                      void* lr8, void* ref8, float* lr_n, float* ref_n, void* stream);
/* flags[i] &= (a[i][0..n_bytes) == b[i][0..n_bytes)) for i < n_pairs (<= 32) in one launch; the caller presets
 * flags to 1.  a, b: HOST arrays of device pointers (16-byte aligned buffers, n_bytes % 16 == 0).
 * Keys the per-frame cache (frames of consecutive sliding windows are recognised by content). */
int refvsr_buffers_equal(const void* const* a, const void* const* b, int n_pairs, size_t n_bytes,
                         int32_t* flags, void* stream);
/* Byte-granular form of refvsr_buffers_equal (extension, no ABI bump: added symbols only): flags[i] &= (a[i][0..n_bytes) ==
 * b[i][0..n_bytes)) for i < n_pairs (<= 32) in one launch, the caller presets flags to 1.  Any n_bytes > 0, any alignment of
 * either buffer.  Keys the per-frame cache for 8-bit input frames (their byte copies, see refvsr_ingest_u8). */
int refvsr_bytes_equal(const void* const* a, const void* const* b, int n_pairs, size_t n_bytes,
                       int32_t* flags, void* stream);
/* out = max(a, b) elementwise on n floats (confidence accumulation, RefVSR.py:147). */
int refvsr_max2(const float* a, const float* b, float* out, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8-bit input frames (extension, no ABI bump: added symbols only).  Replaces the loader's conversion of decoded PNG bytes,
 * data_loader/utils.py:12-41 (`img / 255.` in float64, then float32 tensors in [0, 1] reach models/archs/RefVSR.py:151).
 * refvsr_ingest_u8 converts nframes <= REFVSR_INGEST_MAX_FRAMES byte frames of one h x w (h, w even) in one launch:
 *   src[i]: HOST array of device pointers, 4-byte aligned, to 3 h w bytes laid out as
 *           REFVSR_INGEST_PLANAR  [3][h][w]   (a contiguous [n, t, 3, h, w] uint8 tensor), or
 *           REFVSR_INGEST_HWC     [h][w][3]   (the decoders' interleaved layout: [n, t, h, w, 3] passed as its permute(0, 1, 4, 2, 3)),
 *   dst[i]: HOST array of device pointers, 16-byte aligned, to planar float32 [3][h][w];
 *   dst = T[src] with T[u] = (float)((double)u / 255.0), bit for bit the reference loader's value of every byte.
 * refvsr_ingest_table copies T (256 floats) to host memory `out` (no device work).  refvsr_ingest_max_frames returns
 * REFVSR_INGEST_MAX_FRAMES of the built library (a value, not a status).
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_INGEST_MAX_FRAMES 16
enum { REFVSR_INGEST_PLANAR = 0, REFVSR_INGEST_HWC = 1 };
int refvsr_ingest_u8(const void* const* src, float* const* dst, int nframes, int h, int w, int layout, void* stream);
int refvsr_ingest_table(float* out);
int refvsr_ingest_max_frames(void);

/* ------------------------------------------------------------------------------------------
 * Frame scores on the device (extension, no ABI bump: added symbols only).  Replaces the host-side scoring of the evaluation loop:
 * trainers/trainer.py:252-254 (PSNR = 10 log10(1 / mse)) and evaluation/metrics.py:17-18 (skimage structural_similarity defaults:
 * 7 x 7 uniform window over the valid positions, sample covariance, K1 = 0.01, K2 = 0.03, data range 1, mean over the channels),
 * which evaluation/eval_qual_quan.py:86-101 calls on a frame it first copies to the host.
 * refvsr_score_frames scores nframes <= REFVSR_SCORE_MAX_FRAMES (result, ground truth) pairs of one 3 x h x w geometry (h, w >= 7,
 * any parity) in one launch plus one tiny reduction launch and leaves scores[i] = {mse, ssim} (float64) on the device:
 *   mse  = mean over the 3 h w samples of (a - b)^2                      (the PSNR's log stays on the host)
 *   ssim = mean over the 3 (h - 6)(w - 6) windows of ((2 ua ub + c1)(2 vab + c2)) / ((ua^2 + ub^2 + c1)(va + vb + c2)), box means u,
 *          v = 49/48 (E[xy] - ux uy), c1 = 1e-4, c2 = 9e-4;  win = 7.  win = 0: mse only, the ssim field is 0.
 *   out[i]: HOST array of device pointers to planar [3][h][w] results as the output head stores them, out_fmt = REFVSR_RESULT_F32 |
 *           _F16 | _U8; a byte u means T[u] = (float)((double)u / 255.0), the table of refvsr_ingest_u8;
 *   gt[i]:  HOST array of device pointers, gt_fmt = REFVSR_RESULT_F32 (planar) | REFVSR_RESULT_U8 with gt_layout =
 *           REFVSR_INGEST_PLANAR [3][h][w] | REFVSR_INGEST_HWC [h][w][3] (the decoders' layout: the ground truth uploaded as bytes);
 *   pointers need the natural alignment of their samples only (fp32 4, fp16 2 bytes, bytes none);
 *   workspace: device, 16-byte aligned, workspace_bytes >= refvsr_score_workspace_bytes(nframes, h, w) (host only; 0 for a geometry
 *           that refvsr_score_frames rejects); scores: device, 16-byte aligned, [nframes][2].
 * Exactness: float64 arithmetic on the float32 value of every sample, direct 7-term window sums, fixed-order reduction without
 * floating-point atomics: a pair's two numbers are the same bits on every run, on every stream and at every position of a launch;
 * they agree with the float64 host definition (refvsr_amd/evalrun.py:ssim) to ~1e-13 (summation order).
 * refvsr_score_max_frames returns REFVSR_SCORE_MAX_FRAMES of the built library (a value, not a status).
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_SCORE_MAX_FRAMES 16
size_t refvsr_score_workspace_bytes(int nframes, int h, int w);
int refvsr_score_max_frames(void);
int refvsr_score_frames(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes, int h, int w,
                        int win, void* workspace, size_t workspace_bytes, double* scores, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frame scores of the flag_HD_in configurations (extension, no ABI bump: an added symbol only), whose result is `down` = scale times
 * the size of the ground truth.  Replaces models/loss/Loss.py:91-92,141 (sr_down = F.interpolate(sr, scale_factor = 1 / scale, mode =
 * 'bicubic', align_corners = False).clamp(0, 1), then get_psnr(sr_down, hr)) and evaluation/eval_qual_quan.py:85-92 (ssim of
 * cv2.resize(output, fx = fy = 1 / scale, INTER_CUBIC), not clamped, against the ground truth), both computed on a frame first copied
 * to the host.  refvsr_score_frames_down is refvsr_score_frames with the bicubic down-scale fused into the kernel's tile staging:
 *   out[i]: planar [3][down h][down w] results; gt[i]: [3][h][w] ground truths -- h, w name the GROUND TRUTH, and the workspace is
 *           refvsr_score_workspace_bytes(nframes, h, w) as for refvsr_score_frames; down = 2 | 4;
 *   D(y, x) = sum_j W[j] (sum_k W[k] out[clamp(down y + down / 2 - 2 + j)][clamp(down x + down / 2 - 2 + k)]), W = (-3, 19, 19, -3) / 32
 *           (Keys' cubic, A = -0.75, half-pixel centres, no anti-aliasing: what both reference lines compute at an exact integer
 *           factor), float64 on the float32 value of every tap, k left to right, j top to bottom, rounded once to float32;
 *   mse  = mean of (clamp(D, 0, 1) - gt)^2;  ssim = the SSIM of refvsr_score_frames on the unclamped D.
 *   Every other argument, check and alignment rule is that of refvsr_score_frames (results aligned to four samples are read with
 *   wider loads at down = 4; the scores do not depend on it).
 * Exactness: the scores are bit for bit those of refvsr_score_frames on D (ssim) and on clamp(D, 0, 1) with win = 0 (mse), with D as
 * refvsr_amd/metrics.py:down_bicubic_model computes it; the same determinism.
 * ------------------------------------------------------------------------------------------ */
int refvsr_score_frames_down(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes, int h,
                             int w, int down, int win, void* workspace, size_t workspace_bytes, double* scores, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rectangle sums for the field-of-view evaluation (extension, no ABI bump: added symbols only).  Replaces the host-side masked
 * scoring of evaluation/eval_quan_FOV.py:155-192, which calls evaluation/metrics.py:18-30 (psnr_masked = 10 log10(sum mask /
 * sum (a - b)^2 mask); ssim_masked = sum S mask / sum mask with S the FULL map of skimage structural_similarity: a value at every
 * pixel, the 3-pixel border through scipy.ndimage.uniform_filter's default 'reflect' = the symmetric extension d c b a | a b c d |
 * d c b a) 16 times per frame on a frame it first copies to the host.  Every one of those masks is a rectangle or the difference of
 * two, so refvsr_score_regions leaves RAW sums over rectangles on the device and the host forms the 16 means
 * (refvsr_amd/metrics.py:fov_rects / fov_table):
 *   sums[f][r] = { sum (a - b)^2, sum S } over the three channels and the pixels y0 <= y < y1, x0 <= x < x1 of rectangle r (float64);
 *   rects: HOST array [nrects][4] = y0, y1, x0, x1 (half-open), 1 <= nrects <= REFVSR_SCORE_MAX_RECTS, every rectangle non-empty
 *          and inside the frame; rectangles may overlap or nest in any way;
 *   out / gt / formats / layouts / alignment / nframes <= REFVSR_SCORE_MAX_FRAMES / h, w >= 7: exactly as refvsr_score_frames;
 *   workspace: device, 16-byte aligned, workspace_bytes >= refvsr_score_regions_workspace_bytes(nframes, h, w, nrects) (host only; 0
 *          for arguments that refvsr_score_regions rejects); sums: device, 16-byte aligned, [nframes][nrects][2].
 * Exactness: the arithmetic of refvsr_score_frames (float64 on the float32 value of every sample, direct 7-term window sums) at every
 * pixel centre, fixed-order reduction without floating-point atomics: a frame's sums are the same bits on every run, on every stream
 * and at every position of a launch.  The window sums of the valid crop [3, h - 3) x [3, w - 3) are those of refvsr_score_frames; the
 * tiles, hence the last bits of their total, differ.
 * refvsr_score_max_rects returns REFVSR_SCORE_MAX_RECTS of the built library (a value, not a status).
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_SCORE_MAX_RECTS 8
size_t refvsr_score_regions_workspace_bytes(int nframes, int h, int w, int nrects);
int refvsr_score_max_rects(void);
int refvsr_score_regions(const void* const* out, int out_fmt, const void* const* gt, int gt_fmt, int gt_layout, int nframes, int h, int w,
                         const int* rects, int nrects, void* workspace, size_t workspace_bytes, double* sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * Confidence maps as images (extension, no ABI bump: added symbols only).  Replaces the host-side normalisation and colouring of
 * evaluation/eval_quan_conf_map.py:64-100 (x - x.min(), / x.max(), matplotlib's colormap(x)[:, :, :3] with `inferno`) and
 * :126,148-165 (x * 255 in float32 through cv2.imwrite's round-to-nearest cast), which it runs on maps it first copies to the host.
 * refvsr_conf_colormap colours n <= REFVSR_COLORMAP_MAX_MAPS maps of one h x w geometry (h, w >= 1, h * w < 2^31) in two launches:
 *   maps[k]: HOST array of device pointers, 4-byte aligned, to contiguous fp32 [h][w];
 *   rgb[k]:  HOST array of device pointers (any alignment) to contiguous uint8 [h][w][3], RGB order;
 *   per map, all fp32: lo = min x, a = x - lo, span = max a, y = a / span (the correctly rounded quotient),
 *           idx = min((int)(y * 256), 255), rgb = T[idx]; a constant map (span = 0, y = NaN) is matplotlib's "bad" colour: zero bytes;
 *   T[i][c] = rint(float32(float32(lut64[i][c]) * 255)) with lut64 matplotlib's 256-entry inferno table (csrc/colormap_table.h);
 *   ws: device, 8-byte aligned, ws_bytes >= refvsr_conf_colormap_workspace_bytes(n, h, w) (host only; 0 for arguments that
 *           refvsr_conf_colormap rejects).
 * Exactness: bit for bit the reference's bytes for finite maps; min / max are exact, so a map's bytes are the same on every run, on
 * every stream and at every position of a launch.  refvsr_colormap_table copies T (768 bytes, row-major RGB) to host memory `out768`
 * (no device work).
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_COLORMAP_MAX_MAPS 16
int refvsr_conf_colormap(const void* const* maps, int n, int h, int w, void* const* rgb, void* ws, size_t ws_bytes, void* stream);
size_t refvsr_conf_colormap_workspace_bytes(int n, int h, int w);
int refvsr_colormap_table(unsigned char* out768);

/* ------------------------------------------------------------------------------------------
 * Parameter fingerprint (extension, no ABI bump: added symbols only).  Protects the packed weights against the loaders that
 * write parameters in place: ckpt_manager.py:50-60 goes through load_state_dict, whose copy_ moves the tensors' version
 * counters, but `p.data.copy_(w)` and `p.data = w` -- the same loader written by hand -- move none, and a host-side detector
 * cannot see them.  refvsr_param_fingerprint reads the parameters themselves:
 *   F = sum over all words of mix64(((uint64)g << 32) | word)  (mod 2^64)
 *   word: the 32-bit pattern of an fp32 element (-0 and NaN payloads count); g: the element's index over the concatenated
 *   table, in table order, < 2^32; mix64: splitmix64's finaliser, a bijection of the 64-bit words:
 *       z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31.
 *   One changed word changes F; swapped contents change F (the position term); every summation order gives the same bits.
 *   chunks: DEVICE array of nchunks 16-byte entries { const uint32_t* base; uint32_t g0; uint32_t n; } -- n <=
 *           REFVSR_FINGERPRINT_CHUNK_WORDS words at the 4-byte aligned address base, the first of them global index g0
 *           (refvsr_amd/fingerprint.py:chunk_table); 16-byte aligned; 1 <= nchunks <= REFVSR_FINGERPRINT_MAX_CHUNKS.  The entries
 *           are read by the kernel: their contents are the caller's responsibility.
 *   workspace: device, 16-byte aligned, workspace_bytes >= refvsr_param_fingerprint_workspace_bytes(nchunks) (host only; 0 for a
 *           chunk count that refvsr_param_fingerprint rejects); out: device, 8-byte aligned, one 64-bit word.
 * Two launches on `stream` (one workgroup per chunk: 16-byte loads from a chunk's first aligned word on, 4-byte loads for the
 * <= 3 words before and after; one workgroup that sums the partial sums), integer arithmetic only, plain vector stores, no
 * atomics.  Every argument is checked before the first launch.
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_FINGERPRINT_CHUNK_WORDS 4096
#define REFVSR_FINGERPRINT_MAX_CHUNKS (1 << 22)
size_t refvsr_param_fingerprint_workspace_bytes(int nchunks);
int refvsr_param_fingerprint(const void* chunks, int nchunks, void* workspace, size_t workspace_bytes, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Y'CbCr 4:2:0 result frames (extension, no ABI bump: added symbols only).  The reference's consumer hands the RGB result to an
 * image writer (evaluation/eval_qual_quan.py:117-119, cv2.imwrite of `output * 255`); a video consumer -- an encoder, a raw-video
 * pipe, a .y4m file -- takes 4:2:0 instead and today converts those 3 bytes per pixel on the CPU.  The three entry points replace
 * that host-side conversion (cv2.cvtColor(.., COLOR_RGB2YUV_I420) and its like) behind the result: 1.5 samples per pixel leave
 * the device.  The specification is the numpy model refvsr_amd/yuv.py; the kernel returns its bits.
 *   A frame is ONE dense buffer of 3 h w / 2 samples (h, w even):
 *     REFVSR_YUV_NV12     Y [h][w], then interleaved CbCr [h/2][w/2][2]     8-bit
 *     REFVSR_YUV_I420     Y [h][w], Cb [h/2][w/2], Cr [h/2][w/2]            8-bit
 *     REFVSR_YUV_P010     the NV12 layout, 16-bit little-endian samples, the 10-bit code in the high bits (code << 6)
 *     REFVSR_YUV_I420P10  the I420 layout, 16-bit little-endian samples, the code in the low bits
 *   coef9: HOST array of nine doubles kr, kg, kb, icb, icr, oy, sy, oc, sc (yuv.py:coefficients: matrix, range and depth).
 *   Source value in float64: a float32 / float16 result widened exactly, a uint8 byte u as u / 255.0.  Per pixel, every operation
 *   rounded on its own (no fused multiply-add):  ey = (kr r + kg g) + kb b;  Y = rint(oy + sy ey);  ecb = (b - ey) icb;
 *   ecr = (r - ey) icr;  per 2 x 2 block (centre-sited)  m = ((e00 + e01) + (e10 + e11)) 0.25;  C = rint(oc + sc m);  rint rounds
 *   half to even and every code is clamped to [0, 2^d - 1] before the cast.
 * refvsr_yuv420_max_frames: replaces nothing -- REFVSR_YUV420_MAX_FRAMES of the built library (a value, not a status).
 * refvsr_yuv420_bytes: replaces the consumer's own buffer arithmetic (h * w * 3 / 2 samples) -- the bytes of one frame, 0 for odd
 *   or non-positive h, w or an unknown format (host only).
 * refvsr_result_to_yuv420: replaces the consumer's RGB -> 4:2:0 conversion of nframes <= REFVSR_YUV420_MAX_FRAMES results of one
 *   h x w in ONE launch on `stream`:
 *     src: HOST array of device pointers to the results, src_fmt = REFVSR_RESULT_F32 | F16 | U8, optionally | REFVSR_RESULT_HWC
 *          ([3][h][w] or [h][w][3]: the six forms a result can have), aligned to their samples;
 *     dst: HOST array of device pointers to refvsr_yuv420_bytes(h, w, yuv_fmt) bytes each, aligned to their samples (a group of pixels
 *          whose addresses miss the vectors' alignment is written element by element); no destination may overlap a source or
 *          another destination.
 *   Every argument is checked before any device work: null table, null entry, frame count, unknown formats, odd or non-positive
 *   h / w, alignment, overlap, 3 h w samples beyond 32-bit byte offsets.
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_YUV420_MAX_FRAMES 16
enum { REFVSR_YUV_NV12 = 0, REFVSR_YUV_I420 = 1, REFVSR_YUV_P010 = 2, REFVSR_YUV_I420P10 = 3 };
int refvsr_yuv420_max_frames(void);
size_t refvsr_yuv420_bytes(int h, int w, int yuv_fmt);
int refvsr_result_to_yuv420(const void* const* src, int src_fmt, void* const* dst, int nframes, int h, int w, int yuv_fmt,
                            const double* coef9, void* stream);

/* ------------------------------------------------------------------------------------------
 * Y'CbCr 4:2:0 input frames (extension, no ABI bump: added symbols only).  The reference's loader reads PNGs into RGB bytes
 * (data_loader/utils.py:12-41); a video decoder delivers NV12 or P010 and a .y4m file holds I420.  The two entry points stand in for
 * that loader for video sources: they replace the consumer's host-side Y'CbCr -> RGB conversion (cv2.cvtColor(..,
 * COLOR_YUV2RGB_NV12) and its like) in front of the network, so that 1.5 samples per pixel reach the device instead of 3.  The
 * specification is the numpy model refvsr_amd/yuv.py:yuv420_to_rgb; the kernel returns its bits.
 *   Frames and formats as above (REFVSR_YUV_*); a P010 sample's code is sample >> 6 (the low six bits are ignored), an I420P10
 *   sample's is sample & 1023.
 *   coef: HOST array of nine doubles oy, iy = 1 / sy, oc, ic = 1 / sc, cr_r = 2 (1 - kr), cb_b = 2 (1 - kb), kr, kb, ikg = 1 / kg
 *   (yuv.py:decode_coefficients): no division happens on the device.
 *   Chroma at luma pixel (y, x), centre-sited (the inverse siting of the box average refvsr_result_to_yuv420 takes): (cy, cx) =
 *   (y >> 1, x >> 1), cy' = clamp(cy + (y & 1 ? 1 : -1), 0, h / 2 - 1), cx' likewise,
 *   m = (9 C[cy][cx] + 3 C[cy'][cx] + 3 C[cy][cx'] + C[cy'][cx']) / 16 (an integer below 2^15 times a power of two: exact);
 *   REFVSR_YUV_CHROMA_NEAREST: m = C[cy][cx].
 *   Per pixel in float64, every operation rounded on its own (no fused multiply-add):  ey = (Y - oy) iy;  ecb = (mcb - oc) ic;
 *   ecr = (mcr - oc) ic;  r = ey + cr_r ecr;  b = ey + cb_b ecb;  g = ((ey - kr r) - kb b) ikg;  each of r, g, b clamped to [0, 1]
 *   (decoded video is routinely out of gamut), then rounded once to float32.
 * refvsr_yuv420_in_max_frames: replaces nothing -- REFVSR_YUV420_IN_MAX_FRAMES of the built library (a value, not a status).
 * refvsr_yuv420_to_rgb: nframes <= REFVSR_YUV420_IN_MAX_FRAMES frames of one h x w (even, >= 2, h w <= 2^29) in ONE launch on `stream`:
 *     src: HOST array of device pointers, one dense frame each at any multiple of its sample size (8-bit frames inside a
 *          [t, 3h/2, w] window are 3 h w / 2 bytes apart: odd phases are the normal case);
 *     dst: HOST array of device pointers to planar fp32 [3][h][w], 16-byte aligned: the engine's own frame format, what
 *          refvsr_ingest_u8 writes.
 *   Every argument is checked before any device work: null table, null entry, frame count, odd or non-positive h / w, unknown
 *   format or chroma mode, null coefficients, alignment.
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_YUV420_IN_MAX_FRAMES 16
enum { REFVSR_YUV_CHROMA_BILINEAR = 0, REFVSR_YUV_CHROMA_NEAREST = 1 };
int refvsr_yuv420_in_max_frames(void);
int refvsr_yuv420_to_rgb(const void* const* src, float* const* dst, int nframes, int h, int w, int format, int chroma,
                         const double* coef, void* stream);

/* ------------------------------------------------------------------------------------------
 * Y'CbCr 4:2:2 and 4:4:4 frames, and left-sited chroma, out and in (extension, no ABI bump: added symbols only).  The two 4:2:0
 * sections above know one chroma convention, 4:2:0 sited in the centre of its 2 x 2 block (Y4M's C420jpeg).  Video decoders and most
 * files site chroma on the even luma columns instead (MPEG-2 siting, C420mpeg2: every NV12 / P010 buffer of a hardware decoder), and
 * results are kept as 4:2:2 or 4:4:4.  The three entry points are the 4:2:0 ones with a sampling and a siting; they replace the same
 * things in the reference: refvsr_result_to_yuv the consumer's host-side RGB -> Y'CbCr conversion behind the image writer
 * (evaluation/eval_qual_quan.py:117-119), refvsr_yuv_to_rgb the consumer's Y'CbCr -> RGB conversion in front of the loader's frames
 * (data_loader/utils.py:12-41).  The specification is the numpy model refvsr_amd/yuv.py (rgb_to_yuv, yuv_to_rgb); the kernels return
 * its bits.
 *   yuv_fmt: REFVSR_YUV_* as above -- depth, semi-planarity and shift.  The semi-planar ids (NV12, P010) exist for 4:2:0 only.
 *   sampling: a frame is ONE dense buffer, Y [h][w], Cb [h/cv][w/ch], Cr [h/cv][w/ch]; h, w even for every sampling (4:4:4 would
 *   not need it; the engine's frame checks and refvsr_luma_sad do):
 *     REFVSR_YUV_SAMPLING_420   (cv, ch) = (2, 2)   3 h w / 2 samples
 *     REFVSR_YUV_SAMPLING_422   (cv, ch) = (1, 2)   2 h w samples
 *     REFVSR_YUV_SAMPLING_444   (cv, ch) = (1, 1)   3 h w samples
 *   siting: REFVSR_YUV_SITING_CENTRE (a chroma sample lies in the middle of its luma pair) | REFVSR_YUV_SITING_LEFT (on the pair's
 *   even column); vertically a 4:2:0 sample lies between its two rows in both.  Checked, then ignored, for 4:4:4.
 *   The way out, e = ecb | ecr of the 4:2:0 section, unquantised, float64, every operation rounded on its own, l = max(2j - 1, 0):
 *     4:4:4          m = e[y][x]
 *     4:2:2 centre   m = (e[y][2j] + e[y][2j+1]) 0.5
 *     4:2:2 left     m = ((e[y][l] + e[y][2j+1]) + (e[y][2j] + e[y][2j])) 0.25
 *     4:2:0 left     v[x] = e[2i][x] + e[2i+1][x];  m = ((v[l] + v[2j+1]) + (v[2j] + v[2j])) 0.125
 *     4:2:0 centre   as refvsr_result_to_yuv420
 *   then C = rint(oc + sc m) and the clamp, as there.
 *   The way in, the integer tap sum 16 m at luma pixel (y, x) (below 2^15, exact in any order); everything behind it as
 *   refvsr_yuv420_to_rgb; cx = x >> 1, cx' = clamp(cx + (x & 1 ? 1 : -1)), cxr = min(cx + 1, w/2 - 1), cy and cy' as there:
 *     4:4:4                  16 C[y][x]
 *     4:2:2 centre           12 C[y][cx] + 4 C[y][cx']
 *     4:2:2 left    even x   16 C[y][cx]                     odd x   8 C[y][cx] + 8 C[y][cxr]
 *     4:2:0 left    even x   12 C[cy][cx] + 4 C[cy'][cx]     odd x   6 C[cy][cx] + 2 C[cy'][cx] + 6 C[cy][cxr] + 2 C[cy'][cxr]
 *     4:2:0 centre           as refvsr_yuv420_to_rgb
 *     REFVSR_YUV_CHROMA_NEAREST, every sampling: 16 x the pixel's own sample
 * refvsr_yuv_frame_bytes: replaces the consumer's own buffer arithmetic -- the bytes of one frame; 0 for odd or non-positive h, w,
 *   an unknown format or sampling, or a semi-planar format with a sampling other than 4:2:0 (host only).  With
 *   REFVSR_YUV_SAMPLING_420 it is refvsr_yuv420_bytes.
 * refvsr_result_to_yuv: refvsr_result_to_yuv420 with a sampling and a siting -- its arguments, limits (REFVSR_YUV420_MAX_FRAMES
 *   frames, ONE launch) and checks, dst of refvsr_yuv_frame_bytes(h, w, yuv_fmt, sampling) bytes each.  With 4:2:0 / centre it IS
 *   refvsr_result_to_yuv420: one checked launch stands behind both symbols, the same kernel instance runs, and a refusal carries
 *   that entry's name.
 * refvsr_yuv_to_rgb: refvsr_yuv420_to_rgb with a sampling and a siting -- its arguments, limits (REFVSR_YUV420_IN_MAX_FRAMES frames,
 *   ONE launch) and checks.  With 4:2:0 / centre it IS refvsr_yuv420_to_rgb, in the same sense.
 *   Both check every argument before any device work, and refuse an unknown sampling or siting and a semi-planar format with a
 *   sampling other than 4:2:0.
 * ------------------------------------------------------------------------------------------ */
enum { REFVSR_YUV_SAMPLING_420 = 0, REFVSR_YUV_SAMPLING_422 = 1, REFVSR_YUV_SAMPLING_444 = 2 };
enum { REFVSR_YUV_SITING_CENTRE = 0, REFVSR_YUV_SITING_LEFT = 1 };
size_t refvsr_yuv_frame_bytes(int h, int w, int yuv_fmt, int sampling);
int refvsr_result_to_yuv(const void* const* src, int src_fmt, void* const* dst, int nframes, int h, int w, int yuv_fmt, int sampling,
                         int siting, const double* coef9, void* stream);
int refvsr_yuv_to_rgb(const void* const* src, float* const* dst, int nframes, int h, int w, int yuv_fmt, int sampling, int siting,
                      int chroma, const double* coef9, void* stream);

/* ------------------------------------------------------------------------------------------
 * Antialiased bicubic resize of RGB frames (extension, no ABI bump: added symbols only).  Replaces two things of the reference's
 * world that are not in its code: the offline step that made the dataset's LRx4 folders (the 4x bicubic down-scales the *_L1 configs
 * are trained and scored on, configs/config.py:120-152 reads them ready-made), and the consumer's resize of a result behind the image
 * writer (evaluation/eval_qual_quan.py:117-119).  The filter is Keys' cubic with a = -0.5 stretched by the down-scale ratio (support
 * 2 scale, weights normalised per output sample): Pillow's, MATLAB imresize's and F.interpolate(mode='bicubic', antialias=True,
 * align_corners=False)'s.  It is NOT the bicubic of refvsr_resize / refvsr_score_frames_down (A = -0.75, four taps, no antialias).
 * The specification is the numpy model refvsr_amd/resize.py (aa_taps, resize_aa_model); the kernel returns its bits.
 * refvsr_resize_max_frames: replaces nothing -- REFVSR_RESIZE_MAX_FRAMES of the built library (a value, not a status).
 * refvsr_resize_aa: nframes <= REFVSR_RESIZE_MAX_FRAMES frames of one h x w -> oh x ow in ONE launch on `stream`, no host
 *   synchronisation, no intermediate in global memory (the horizontal sums of a tile live in LDS as float64):
 *     src: HOST array of device pointers, one dense 3 x h x w frame each in src_fmt = REFVSR_RESULT_F32 | _F16 | _U8, planar or
 *          | REFVSR_RESULT_HWC, at any multiple of its sample size; a byte means the float32 refvsr_ingest_u8 gives it;
 *     dst: HOST array of device pointers to dense planar [3][oh][ow] frames, dst_fmt = REFVSR_RESULT_F32 (any 4-byte alignment) or
 *          REFVSR_RESULT_U8 (any address);
 *     lo_x, cnt_x [ow] int32, wx [ow][maxcnt_x] float64, lo_y, cnt_y [oh], wy [oh][maxcnt_y]: DEVICE tables, the taps of
 *          resize.py:aa_taps(w, ow) and aa_taps(h, oh): output column j is the sum over k < cnt_x[j] of wx[j][k] src[lo_x[j] + k],
 *          added in ascending k from the first product, every operation rounded on its own; rows the same over the unrounded
 *          horizontal sums.  The device computes no weight.  The host cannot read the tables: the kernel clamps every index they
 *          yield into the rows and columns it staged, so a wrong table gives wrong samples, never an access outside the frames;
 *     clamp: 1: float32(clamp(D, 0, 1)), one rounding; 0: float32(D).  A byte destination is rint(255 clamp(D, 0, 1)), half to
 *          even, whatever `clamp` says.
 *   Limits: h <= 8 oh and w <= 8 ow (at most 33 taps), no limit on up-scaling, frames below 2^31 bytes.
 *   Every argument is checked before any device work: null tables, frame count, format ids, sizes and ratio, clamp, cnt against
 *   maxcnt (maxcnt_x, maxcnt_y in 1 .. min(33, the taps an axis of these sizes can have)), table alignment, null entries, entries
 *   not aligned to their samples, overlaps.
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_RESIZE_MAX_FRAMES 16
int refvsr_resize_max_frames(void);
int refvsr_resize_aa(const void* const* src, int src_fmt, void* const* dst, int dst_fmt, int nframes, int h, int w, int oh, int ow,
                     const int32_t* lo_x, const int32_t* cnt_x, const double* wx, const int32_t* lo_y, const int32_t* cnt_y,
                     const double* wy, int maxcnt_x, int maxcnt_y, int clamp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG of Y'CbCr frames (extension, no ABI bump: added symbols only).  Replaces the consumer's host-side JPEG writer
 * (evaluation/eval_qual_quan.py:107-129: a JPEG per frame through the image library): the entropy-coded data of one JPEG scan per frame
 * is made on the device from the frames refvsr_result_to_yuv wrote, so that about a tenth of the 4:2:0 bytes crosses to the host.  The
 * specification is the numpy model refvsr_amd/jpeg.py (encode_model); the kernels return its bytes.  JFIF means BT.601, full range,
 * centre-sited chroma: the caller converts with those.  Headers (SOI .. SOS) and EOI are the host's (jpeg.py:header).
 * refvsr_jpeg_max_frames: replaces nothing -- REFVSR_JPEG_MAX_FRAMES of the built library (a value, not a status).
 * refvsr_jpeg_capacity: host only, replaces nothing; an upper bound of one frame's entropy-coded bytes (jpeg.py:capacity says how it
 *   is derived), 0 for arguments the call rejects.
 * refvsr_jpeg_workspace_bytes: host only, replaces nothing; the workspace of a call with these arguments, 0 for arguments it rejects.
 * refvsr_jpeg_encode: nframes <= REFVSR_JPEG_MAX_FRAMES frames of one h x w (even, 2..65535, at most 2^23 blocks) in FIVE launches on
 *   `stream` (transform; entropy pass counting bytes per restart interval; prefix sums; offsets; entropy pass writing at the final
 *   offsets), plain vector stores only:
 *     src: HOST array of device pointers, one dense 8-bit planar frame each (REFVSR_YUV_I420's layout at sampling
 *          REFVSR_YUV_SAMPLING_420 | _444; 4:2:2 is not built), at any address;
 *     qtables [2][64] float64 (luma, chroma; natural order), dct [8][8] float64 (jpeg.py:dct_table), huffman_lut [4][256] uint32
 *          (jpeg.py:huffman_lut: length << 16 | code of DC luma, AC luma, DC chroma, AC chroma): DEVICE tables made by the host; the
 *          device computes no cosine and no table.  A wrong table gives wrong bytes, never an access outside the buffers: every
 *          store is checked against the frame's counted size;
 *     restart: MCUs per restart interval, 1..65535; every interval is one wave's work;
 *     dst: DEVICE, dst_capacity bytes: the data of the frames back to back, RST markers included, no header, no EOI;
 *     sizes, offsets: DEVICE, 8-byte aligned, nframes 64-bit words each: frame i's data is dst[offsets[i] .. offsets[i] + sizes[i]).
 *          A frame that does not fit dst_capacity behind the frames ahead of it is not written; sizes still holds what it needs.
 *          Nothing is written past dst + dst_capacity;
 *     workspace: DEVICE, 16-byte aligned, workspace_bytes >= refvsr_jpeg_workspace_bytes(nframes, h, w, sampling, restart).
 *   With dst_capacity >= nframes * refvsr_jpeg_capacity(..) nothing can overflow and the call does not wait.  With less it waits for
 *   the stream, reads the sizes and returns REFVSR_JPEG_OVERFLOW (with a message) if a frame did not fit.
 *   Every argument is checked before any device work.
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_JPEG_MAX_FRAMES 16
#define REFVSR_JPEG_OVERFLOW 3
int refvsr_jpeg_max_frames(void);
size_t refvsr_jpeg_capacity(int h, int w, int sampling, int restart);
size_t refvsr_jpeg_workspace_bytes(int nframes, int h, int w, int sampling, int restart);
int refvsr_jpeg_encode(const void* const* src, int nframes, int h, int w, int sampling, const double* qtables, const double* dct,
                       const uint32_t* huffman_lut, int restart, void* dst, size_t dst_capacity, long long* sizes, long long* offsets,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scene cuts: luma SAD of frame pairs (extension, no ABI bump: added symbols only).  Replaces nothing in the reference: its loader
 * serves one folder per clip, replicates frames at the clip's edges (data_loader/datasets.py:222-234) and starts every clip with
 * is_first = True, so it never meets a cut.  A video file has cuts; refvsr_amd/videorun.py (--scene_cut) runs every scene as the
 * reference would run a clip, and finds the scenes from the sum of absolute luma differences of consecutive LR frames
 * (refvsr_amd/scene.py turns the sums into the scene score).  The three entry points serve that detector alone.  The specification is
 * the numpy model refvsr_amd/yuv.py:luma_sad; the kernel returns its integers.
 *   Frames and formats as above (REFVSR_YUV_*).  Only the luma plane is read: the first h w samples of a frame in every format; a
 *   P010 sample's code is sample >> 6, an I420P10 sample's is sample & 1023 (as refvsr_yuv420_to_rgb reads them).
 * refvsr_scene_max_pairs: replaces nothing -- REFVSR_SCENE_MAX_PAIRS of the built library (a value, not a status).
 * refvsr_luma_sad_workspace_bytes: host only; the workspace of a call with these arguments (any format), 0 for arguments the call
 *   rejects.
 * refvsr_luma_sad: sad[i] = sum over the h w luma codes of |Ya_i - Yb_i| for 1 <= npairs <= REFVSR_SCENE_MAX_PAIRS pairs of one h x w
 *   (even, >= 2, h w <= 2^29), an exact 64-bit integer, in TWO launches on `stream` (partial sums per 16-byte-group chunk with plain
 *   vector stores, 32-bit: a chunk holds 8 222 samples at most; one workgroup per pair adds them in 64 bits), no host
 *   synchronisation, no floating point, no atomics:
 *     a, b: HOST arrays of device pointers, one dense frame each at any multiple of its sample size (frames inside a [t, 3h/2, w]
 *          window are 3 h w / 2 samples apart: phases that are not 16-byte aligned are the normal case); a[i] == b[i] is allowed
 *          and gives 0;
 *     workspace: device, 16-byte aligned, workspace_bytes >= refvsr_luma_sad_workspace_bytes(npairs, h, w);
 *     sad: device, 8-byte aligned, npairs 64-bit words.
 *   Every argument is checked before any device work: null tables, pair count, odd or non-positive h / w, unknown format, null
 *   workspace or sad, their alignment, the workspace size, null entries, entries not aligned to their samples.
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_SCENE_MAX_PAIRS 16
int refvsr_scene_max_pairs(void);
size_t refvsr_luma_sad_workspace_bytes(int npairs, int h, int w);
int refvsr_luma_sad(const void* const* a, const void* const* b, int npairs, int h, int w, int yuv_fmt, void* workspace,
                    size_t workspace_bytes, unsigned long long* sad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Inter-frame alignment
 * ------------------------------------------------------------------------------------------ */
/* models/utils.py:35-43 `warp`: linspace(-1,1) base grid + flow/((Win-1)/2), grid_sample(bilinear,
 * zeros, align_corners=False).  Output size = flow size [hf][wf]; input may be a different size
 * (RefVSR.py:254).  flow: planar fp32 [2][hf][wf]. */
int refvsr_warp_nhwc16(const void* x, int hin, int win, int cs, const float* flow, int hf, int wf,
                       void* out, void* stream);
/* warp(x, F.interpolate(flow_lr, scale_factor=2, mode='bilinear', align_corners=True) * 2) in one launch (ABI 10): the 2x
 * propagation state is warped by the up-sampled LR flow (RefVSR.py:220,254,259); the [2][2hl][2wl] flow map is evaluated per
 * pixel instead of being written and read back.  flow_lr: planar fp32 [2][hl][wl]; out [2hl][2wl][cs].  Bit-identical to
 * refvsr_resize(BILINEAR_AC, chan_mul 2) + refvsr_warp_nhwc16. */
int refvsr_warp_nhwc16_up2(const void* x, int hin, int win, int cs, const float* flow_lr, int hl, int wl,
                           void* out, void* stream);
int refvsr_warp_planar(const float* x, int c, int hin, int win, const float* flow, int hf, int wf,
                       float* out, void* stream);
/* The three warps over `batch` (map, flow) pairs in one launch each (ABI 11; blockIdx.z = pair): x / flow / out are host arrays of
 * `batch` device pointers, all pairs of one geometry.  Pair b == the single call, bit for bit. */
int refvsr_warp_nhwc16_batch(const void* const* x, int batch, int hin, int win, int cs, const float* const* flow, int hf, int wf,
                             void* const* out, void* stream);
int refvsr_warp_nhwc16_up2_batch(const void* const* x, int batch, int hin, int win, int cs, const float* const* flow_lr, int hl, int wl,
                                 void* const* out, void* stream);
int refvsr_warp_planar_batch(const float* const* x, int batch, int c, int hin, int win, const float* const* flow, int hf, int wf,
                             float* const* out, void* stream);
/* One SPyNet pyramid level input (SPyNet.py:83-103): flow_up = 2*bilinear_x2(flow_prev, align_corners)
 * (or zeros when flow_prev == NULL), warped = flow_warp(supp, flow_up, border, align_corners=True)
 * (mmedit flow_warp.py:6-47); writes cat[ref, warped, flow_up] as nhwc16 [h][w][8] and flow_up as
 * planar fp32 [2][h][w].  ref/supp: planar fp32 [3][h][w]; flow_prev: planar [2][h/2][w/2]. */
int refvsr_spynet_level_input(const float* ref, const float* supp, const float* flow_prev, int h, int w,
                              void* out8, float* flow_up, void* stream);
/* The same for `batch` (1..8; 4 until ABI 10) independent (ref, supp) pairs of one pyramid level in one launch: ref / supp are host arrays of
 * `batch` device pointers; flow_prev [batch][2][h/2][w/2] (or NULL), out8 [batch][h][w][8], flow_up [batch][2][h][w] are
 * contiguous batches.  Image b == refvsr_spynet_level_input of pair b, bit for bit. */
int refvsr_spynet_level_input_batch(const float* const* ref, const float* const* supp, int batch, const float* flow_prev,
                                    int h, int w, void* out8, float* flow_up, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reference matching  (FeatureMatching.forward, RefVSR_/attention.py:72-91)
 * ------------------------------------------------------------------------------------------ */
#define REFVSR_MATCH_KP 152       /* 144 = 16 ch x 3x3 patch, padded to 152 halfs (304-byte rows)   */
#define REFVSR_MATCH_ROWCHUNK 256 /* reference rows are padded to a multiple of this               */
#define REFVSR_MATCH_COLBLOCK 512 /* LR columns are padded to a multiple of this                    */
/* feat: planar fp32 [16][h][w].  Writes rows [h*w][KP] fp16 of L2-normalised reflect-padded 3x3
 * patches (channel order c*9+ky*3+kx, RefVSR_/utils.py:29-57), inv_norm[h*w] = 1/max(|p|,1e-12) and, when rows_lo != NULL,
 * the low halves of the fp16 hi + lo split of the same normalised patches, rows_lo [h*w][KP] fp16 =
 * fp16((p - rows) * 2^11) (second operand of refvsr_match_exact; allocate it padded like rows). */
int refvsr_match_patches(const float* feat, int h, int w, void* rows, float* inv_norm, void* rows_lo, void* stream);
/* Tuning knob (added symbol, ABI 15 unchanged): which kernel refvsr_match_patches launches.  0: one pixel per thread with global
 * gathers; 1: a 256-pixel strip staged in LDS (default).  Results do not depend on it (bit-identical). */
int refvsr_set_match_patches_kernel(int mode);
/* rows_lo of the columns in the flagged list of refvsr_match_refine only (added symbol, ABI 15 unchanged): the values
 * refvsr_match_patches writes with rows_lo != NULL, at the same offsets of the [h*w][KP] buffer; every other row is left
 * untouched.  refvsr_match_exact reads lr_rows_lo at the flagged columns alone, so this stands in for the full LR array.
 * inv_norm: as written by refvsr_match_patches for feat.  The count is read on the device. */
int refvsr_match_lo_rows(const float* feat, int h, int w, const float* inv_norm, const int32_t* flagged, void* rows_lo,
                         void* stream);
/* Fused cosine GEMM + column top-2 (never materialises the [n_ref x n_lr] matrix).
 * ref_rows: [n_ref_pad][KP], lr_rows: [n_lr_pad][KP] (pads zero).  row_splits >= 1 partitions the
 * reference rows over blockIdx.y.  cand_idx / cand_val: [n_lr][2*row_splits] (first-max-wins order). */
int refvsr_match_top2(const void* ref_rows, int n_ref, const void* lr_rows, int n_lr, int row_splits,
                      int32_t* cand_idx, float* cand_val, void* stream);
/* Exact fp32 re-rank of the candidates: conf[p] = max_c <lr_patch p, ref_patch c> (normalised),
 * idx[p] = that candidate (smallest index on ties, like torch.max).  When flagged != NULL (int32 [1 + h*w], [0] = 0 on
 * entry): columns whose re-ranked maximum does not clear the runner-up's fp16 score (cand_val) by `margin` -- i.e. where
 * a row outside the candidate list could still be the true arg-max -- are appended to flagged[1..], flagged[0] counts. */
int refvsr_match_refine(const float* lr_feat, int h, int w, const float* ref_feat, int hr, int wr,
                        const float* inv_lr, const float* inv_ref, const int32_t* cand_idx, const float* cand_val,
                        int ncand, float margin, int32_t* flagged, float* conf, int32_t* idx, void* stream);
/* Exhaustive fp32-grade arg-max for the flagged columns: both operands split into fp16 hi + lo, three fp16 MFMAs with fp32
 * accumulation per product (dropped term 2^-22).  The winner of every flagged column is re-evaluated with the exact fp32
 * dot product of refvsr_match_refine and replaces that column's conf / idx if it is better (smaller index on ties).
 * lr_rows / lr_rows_lo, ref_rows / ref_rows_lo: the fp16 hi / lo patch rows of refvsr_match_patches (reference rows padded
 * to a multiple of 256); keys: uint64 [h*w] zeroed scratch.  The flagged count is read on the device (no host
 * synchronisation); with no flagged column the launches are no-ops. */
int refvsr_match_exact(const float* lr_feat, int h, int w, const float* ref_feat, int hr, int wr, const void* lr_rows,
                       const void* lr_rows_lo, const void* ref_rows, const void* ref_rows_lo, const float* inv_lr,
                       const float* inv_ref, const int32_t* flagged, void* keys, float* conf, int32_t* idx, void* stream);
/* Unfused fp32 reference kernel of the same op (test / debugging aid, O(n_ref*n_lr*144) VALU). */
int refvsr_match_naive(const float* lr_feat, int h, int w, const float* ref_feat, int hr, int wr,
                       float* conf, int32_t* idx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reference alignment  (AlignedAttention / AlignedConv2d, attention.py:131-159, alignment.py:39-178)
 * ------------------------------------------------------------------------------------------ */
/* unfold(k=s,stride=s) -> gather(index) -> fold == block gather:
 * out[s*y+ky][s*x+kx][:] = value[s*ry+ky][s*rx+kx][:], (ry,rx) = divmod(idx[y*gw+x], wv/s). */
int refvsr_block_gather_nhwc16(const void* value, int hv, int wv, int cs, const int32_t* idx, int gh, int gw,
                               int s, void* out, void* stream);
/* same gather on a planar fp32 RGB frame, written as nhwc16 [gh*s][gw*s][8] (3 valid channels; out8, may be NULL)
 * and / or as an exact planar fp32 copy [3][gh*s][gw*s] (out_planar, may be NULL: the `vis` samples RefVSR.py:305-309). */
int refvsr_block_gather_rgb(const float* value, int hv, int wv, const int32_t* idx, int gh, int gw, int s,
                            void* out8, float* out_planar, void* stream);
/* affine-deformable bilinear patch sampler (alignment.py:53-100,102-178).
 * x: nhwc16 [h*ks][w*ks][cs]; affine: planar fp32 [3][h][w] already (+1, clamped to [-3,3]). */
int refvsr_aligned_sample(const void* x, int h, int w, int ks, int cs, const float* affine, void* out,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * RefVSR_IR: EDVR-M feature extractor pieces that are not convolutions (models/archs/edvr_net.py)
 * ------------------------------------------------------------------------------------------ */
/* Sampling half of mmcv's modulated deformable convolution (edvr_net.py:49-56, ModulatedDCNPack; 3x3, stride 1, pad 1):
 * cols[y][x][k*c + ch] = sigmoid(mask) * bilinear(x, tap position + offset) for tap k, 8 channels per deformable group;
 * offset_mask = raw conv_offset output, planar fp32 [3*groups*9][h][w] ([o1 | o2 | mask]).  The contraction with the
 * [cout][c*9] weight is a 1x1 refvsr_conv_mfma over cols. */
int refvsr_dcn_sample(const void* x, int h, int w, int c, const float* offset_mask, int deform_groups, void* cols,
                      void* stream);
/* TSAFusion temporal attention (edvr_net.py:259-272): out[.., i*c + ch] = aligned_i * sigmoid(sum_ch emb_i * emb_ref);
 * aligned / emb: HOST arrays of t device pointers (nhwc16 [npix][c]). */
int refvsr_tsa_weight(const void* const* aligned, const void* const* emb, const void* emb_ref, int t, int c, int npix,
                      void* out, void* stream);
/* MaxPool2d / AvgPool2d(3, stride 2, padding 1) of an nhwc16 map into channels [c_off, c_off + c) of out (channel
 * stride out_c) (edvr_net.py:214-215,277-279). */
int refvsr_pool3s2_nhwc16(const void* x, int h, int w, int c, void* out, int out_c, int c_off, int is_max, void* stream);
/* nn.Upsample(x2, bilinear, align_corners=False) * mul of an nhwc16 map (edvr_net.py:131,179-181,246). */
int refvsr_up2_bilinear_nhwc16(const void* x, int h, int w, int c, float mul, void* out, void* stream);
/* out = feat * sigmoid(attn) * 2 + add on n halfs (edvr_net.py:294-299). */
int refvsr_tsa_blend(const void* feat, const void* attn, const void* add, size_t n, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REFVSR_HIP_H */
