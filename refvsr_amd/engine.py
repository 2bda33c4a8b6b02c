"""The MI355X RefVSR pipeline: `Network.forward` of the reference re-expressed as launches of the
HIP kernels behind the C-ABI (refvsr_amd/ops.py), one sample (n=1) at a time.

Follows /root/reference/models/archs/RefVSR.py:151-325 step by step (the comments cite the lines).
What differs from the reference's *execution* (never its results):

  * only the flows the network consumes are computed (RefVSR.py:182-191 computes 2(t-1), uses
    t//2 + 1 in steady state), and
  * everything that depends on a single frame only -- SPyNet pyramids, matching (conf, index),
    the reference encoders, and both AlignedAttention outputs (aa1 gather, aa2 gather +
    AlignedConv2d), which are functions of (lr_i, ref_i) alone -- is cached per frame and reused
    across overlapping sliding windows and across the backward/forward branches
    (`config.cache_windows`).  Frames are recognised by exact content
    equality with the previous window, so the drop-in call signature needs no frame ids.

Feature maps live in HBM as fp16 HWC ("nhwc16"); frames, flows and confidence maps as planar fp32.
"""
import collections
import itertools
import os

import torch

from . import inputs, ops, yuv
from .config import resolve_weight_precision
from .knobs import env_flag
from .packing import pack_conv, pack_conv_hr_last, pack_conv_last
from .weights import VGG_MEAN, VGG_STD, round16

_uid = itertools.count()


def _timed_event(stream):
    e = torch.cuda.Event(enable_timing=True)
    e.record(stream)
    return e


def _flow_pairs(fr, restart):
    """The flows one window consumes (RefVSR.py:182-191): the backward flows from the centre on and the forward flow of the carried
    state (forward_flows[:, ctr], :279-283); a window whose forward branch restarts also walks its first frames."""
    t = len(fr)
    ctr = t // 2
    need = [(fr[i], fr[i + 1]) for i in range(ctr, t - 1)] + [(fr[ctr + 1], fr[ctr])]
    if restart:
        need += [(fr[i], fr[i - 1]) for i in range(1, ctr + 1)]
    return need


# ---- layout of the device messages (state hand-off, contexts): a spec [(name, shape, dtype)] of parts that lie back to back in a
#      uint8 buffer, each padded to `align` bytes
def _part_nbytes(shape, dtype, align):
    n = dtype.itemsize
    for d in shape:
        n *= d
    return (n + align - 1) // align * align


def msg_nbytes(spec, align=1):
    return sum(_part_nbytes(shape, dtype, align) for _, shape, dtype in spec)


def msg_pack(buf, offset, tensors, align=1):
    """Copy the tensors into buf from byte `offset` on, one part each (current stream); returns the offset behind the last part."""
    for t in tensors:
        n = t.numel() * t.element_size()
        buf[offset:offset + n].view(t.dtype).copy_(t.reshape(-1))
        offset += _part_nbytes(t.shape, t.dtype, align)
    return offset


def msg_views(buf, offset, spec, align=1, clone=False):
    """{name: tensor} of the parts of `spec` from byte `offset` of buf on: views into buf, or copies of their own (clone)."""
    out = {}
    for name, shape, dtype in spec:
        t = buf[offset:offset + _part_nbytes(shape, dtype, 1)].view(dtype).view(shape)
        out[name] = t.clone() if clone else t
        offset += _part_nbytes(shape, dtype, align)
    return out


class FrameCtx(object):
    """Per-frame data (functions of one (lr, ref) frame pair only)."""

    def __init__(self, lr, ref, ingest=None, yuv=None):
        self.uid = next(_uid)
        # the context OWNS its frames (clones): it outlives the call in the window cache, and a caller that refills one
        # static input buffer in place must neither change cached data nor make the content compare see "equal" frames.
        # A kind that keeps the copies as `src` (8-bit, 4:2:0: they key the content compare) decodes the planar fp32 frames [3,h,w]
        # from them -- now, or in the one launch over a call's new frames when the caller collects the pairs in `ingest`
        source = inputs.source_of(lr, ref, yuv)             # (yuv: config.input_yuv resolved, Engine.input_yuv)
        self.kind = source.key
        copies = (lr.clone(), ref.clone())
        self.src = copies if source.keeps_source else None
        (self.lr, self.ref), pairs = source.frames(copies)
        if ingest is None:
            source.decode(pairs)
        else:
            ingest.extend(pairs)
        self.lr8 = None         # nhwc16 [h,w,8]
        self.pyr = None         # SPyNet pyramid of lr, coarse -> fine
        self.conf = None        # planar [1,h,w]
        self.idx = None         # int32 [Hf*Wf]
        self.aligned = None     # aa1 output nhwc16 [h,w,C]
        self.aligned_up = None  # aa2 output nhwc16 [2h,2w,C]
        self.bw_head = None     # pipelined mode: (n, map) -- the first n layers of the backward branch's first step on this frame
        self.ready = None       # pipelined mode: HIP event recorded on the preparation stream once all of the above exist


class Weights(object):
    """All parameters of the network packed for the kernels (built from a reference-keyed state dict)."""

    def __init__(self, config, sd, device):
        self.device = device
        self.C = config.mid_channels
        self.nb = config.num_blocks
        self.conv = {}
        self.raw = {}
        self.chains = {}            # runs of fused blocks -> ops.ResblockChain pointer tables (Engine._block_chain)
        # weight format, resolved once per packing (config.resolve_weight_precision): 'fp16' packs round16(sd) -- every packer below
        # then sees fp16-representable weights (lo halves = 0) -- and the specialised C = 24 kernels take their fp16-format blobs
        # (no lo fragments), which every launch picks from the ConvWeights / chain it is handed
        self.wfmt = resolve_weight_precision(config)
        if self.wfmt == 'fp16':
            sd = round16(sd)
        C = self.C
        g = lambda n: (sd['Network.' + n + '.weight'], sd['Network.' + n + '.bias'])

        def mf(name, srcs, shuffle=False, mt=None):
            w, b = g(name)
            self.conv[name] = ops.ConvWeights(pack_conv(w, b, srcs, shuffle, mt=mt), device, wfmt=self.wfmt)

        def dr(name):
            w, b = g(name)
            self.raw[name] = (w.detach().to(device, torch.float32).contiguous(),
                              b.detach().to(device, torch.float32).contiguous())

        def mf32(name, srcs):
            w, b = g(name)
            self.conv[name] = ops.ConvWeights(pack_conv(w, b, srcs, f32=True), device)

        chans = [(32, 8), (64, 32), (32, 64), (16, 32), (2, 16)]
        # SPyNet's streamed 7x7 convs (every conv but the first of a level) on plain fp16 weights: half the weight stream and
        # half the MFMAs of the kernels that are bound by both.  Their share of the end-to-end error budget is measured
        # (tools/lo_term_study.py); config.spynet_hi_lo = True / REFVSR_SPYNET_HILO=1 restores hi + lo.
        hi_only = not (bool(getattr(config, 'spynet_hi_lo', False)) or env_flag('REFVSR_SPYNET_HILO'))
        for lvl in range(6):
            for j, (co, ci) in enumerate(chans):
                name = 'FlowNet.basic_module.%d.basic_module.%d.conv' % (lvl, j)
                w, b = g(name)
                self.conv[name] = ops.ConvWeights(pack_conv(w, b, [ci], hi_only=hi_only and j > 0), device)
                if co > 16 and ci > 8:
                    # the streamed 7x7 convs of the coarse pyramid levels (a handful of pixel tiles): 16 output channels per
                    # workgroup, so that 2-4x as many CUs share the 200-400 KB weight stream (Engine.flow picks per level)
                    self.conv[name + '/mt1'] = ops.ConvWeights(pack_conv(w, b, [ci], mt=1, hi_only=hi_only), device)
        fe = 'feature_match.feature_extract.'
        self.hd = bool(config.flag_HD_in)
        self.vgg7 = self.hd or config.scale != 4          # attention.py:31-35
        dr('feature_match.sub_mean')
        mf32(fe + '0', [3])
        mf32(fe + '2', [64])
        if self.vgg7:                     # VGG19[0:7] + map128 (attention.py:33-40)
            mf32(fe + '5', [64])
            mf32(fe + 'map128.0', [128])
            self.raw[fe + 'map128.0'] = tuple(t.detach().to(device, torch.float32).contiguous() for t in
                                              (g(fe + 'map128.0')[0].reshape(16, 128), g(fe + 'map128.0')[1]))
        else:
            mf32(fe + 'map64.0', [64])
            self.raw[fe + 'map64.0'] = tuple(t.detach().to(device, torch.float32).contiguous() for t in
                                             (g(fe + 'map64.0')[0].reshape(16, 64), g(fe + 'map64.0')[1]))

        def aligned(prefix, stride):
            mf(prefix + '.conv1.0', [3])
            mf(prefix + '.conv1.2.conv1', [32])
            mf(prefix + '.conv1.2.conv2', [32])
            # the strided 5x5 predictor conv (alignment.py:20: 64 -> 32, stride = the patch size): with 32 output channels per workgroup
            # its staged input tile + a weight ring exceeds the LDS and the generic kernel runs in gather mode (B fragments from global
            # memory inside the K loop); at stride 2 sixteen output channels per workgroup (mt = 1) fit the 4 x 32 tile mode: 116.6 ->
            # 94.9 us at 540 x 960, bit-identical (profiles/r05_pconv_mt1_ab.txt; at stride 4 no tile fits either way and mt = 1 only
            # doubles the gathers: 196 vs 421 us at 1080 x 1920).  REFVSR_PCONV_MT = 1 | 2 forces one packing (A/B knob)
            mt_p = int(os.environ.get('REFVSR_PCONV_MT', '1' if stride == 2 else '2'))
            mf(prefix + '.p_conv.0', [32, 32], mt=mt_p)
            mf(prefix + '.p_conv.2.conv1', [32])
            mf(prefix + '.p_conv.2.conv2', [32])
            mf(prefix + '.p_conv.4', [32])
        aligned('aa2.align', config.matching_ksize)
        if config.matching_ksize // 2 > 1:     # RefVSR.py:39 -- aa1 aligns only when its patch is larger than 1 px
            aligned('aa1.align', config.matching_ksize // 2)

        def reslist(name, n):
            for i in range(n):
                mf('%s.RBs.%d.conv1' % (name, i), [C])
                mf('%s.RBs.%d.conv2' % (name, i), [C])
            mf(name + '.conv_tail', [C])

        mf('ref_encoder1.0.0', [3])
        mf('ref_encoder1.1.0', [C])
        reslist('res1', 4)
        mf('ref_encoder2.0.0', [C])
        mf('ref_encoder2.1.0', [C])
        reslist('res2', 4)
        for nm in ('conf_fusion', 'conf_fusion2', 'conf_fusion_BWFW'):
            dr(nm + '.0.0')
            mf(nm + '.1.0', [16])
        for nm in ('feat_fusion', 'feat_fusion2', 'feat_fusion_BWFW'):
            mf(nm + '.0.0', [C, C])
            mf(nm + '.1.0', [C])
        mf('feat_fusion2_1.0.0', [C, C])
        reslist('feat_decoder', 8)
        reslist('feat_decoder2', 4)
        reslist('feat_decoder_BWFW', 4)
        for br in ('backward_resblocks', 'forward_resblocks'):
            cin = sd['Network.' + br + '.main.0.weight'].shape[1]
            if cin == C + 3:
                mf(br + '.main.0', [3, C])
            else:                        # RefVSR_IR forward branch: cat([lr, backward features, state]) (RefVSR_IR.py:354); the
                assert cin == 2 * C + 3  # kernel takes two maps, so [lr | backward features] are handed over as one HWC map
                mf(br + '.main.0', [3, C, C])
                cw = self.conv[br + '.main.0']
                cw.cpads = [cw.cpads[0] + cw.cpads[1], cw.cpads[2]]
            for i in range(self.nb):
                mf('%s.main.2.%d.conv1' % (br, i), [C])
                mf('%s.main.2.%d.conv2' % (br, i), [C])
        mf('fusion_UP', [C, C])
        mf('upsample1.upsample_conv', [C], shuffle=True)
        if config.scale == 4:                             # RefVSR.py:89-90
            mf('upsample2.upsample_conv', [C], shuffle=True)
        mf('conv_hr', [C])
        mf('conv_last', [C])


class Engine(object):
    """Stateful per-stream executor (one stream of consecutive frames, like a reference module
    instance: RefVSR.py:96-101,279-283)."""
    input_yuv = None            # config.input_yuv resolved by __init__: None (off) or (format, matrix, range, chroma)

    def __init__(self, config, weights):
        if config.scale not in (2, 4):
            raise NotImplementedError('SR scale must be 2 or 4 (configs/config_RefVSR_*.py: "SR scale (2 | 4)")')
        self.cfg = config
        self.W = weights
        self.C = config.mid_channels
        self.nb = config.num_blocks
        self.ks = config.matching_ksize
        self.hd = bool(config.flag_HD_in)
        self.vgg7 = self.hd or config.scale != 4           # matching on VGG19[0:7] features: grid = half the (resized) frame
        self.cache = bool(getattr(config, 'cache_windows', True))
        self.match_row_splits = 1
        self.match_margin = float(getattr(config, 'match_exact_margin', ops.MATCH_EXACT_MARGIN))
        self.chain_calls = bool(getattr(config, 'chain_calls', not env_flag('REFVSR_NO_CHAIN_CALLS')))
        self.fuse_resblocks = (bool(getattr(config, 'fuse_resblocks', True)) and ops.resblock_fits(self.C)
                               and not env_flag('REFVSR_NO_FUSE'))
        self.rb24 = not env_flag('REFVSR_NO_RB24')               # A/B knob: the generic lean kernel for C = 24 as well
        self.rb48 = (bool(getattr(config, 'fuse_resblocks', True)) and not env_flag('REFVSR_NO_FUSE')
                     and not env_flag('REFVSR_NO_RB48'))                 # A/B knob: C = 48 blocks as two refvsr_conv48 launches (round 3)
        self.rb48_max_pixels = int(os.environ.get('REFVSR_RB48_MAX_PIXELS', str(540 * 960)))
        self.rb48_multimap = not env_flag('REFVSR_NO_RB48_MULTIMAP')      # A/B knob: frame groups of C = 48 run their blocks map by map
        # SPyNet levels up to this many pixels run their streamed convs with 16 output channels per workgroup (A/B knob; 0 = never)
        self.spynet_mt1_pixels = int(os.environ.get('REFVSR_SPYNET_MT1_PIXELS', str(72 * 120)))
        # pipelined mode: the backward branch restarts from zeros at the window's LAST frame (RefVSR.py:211-214), so the first
        # layers of that step are a function of that frame alone: its input conv + the first `bw_head_blocks` residual blocks run
        # with the frame's preparation on the P stream -- load balance between the two internal streams (results identical).
        # Measured (profiles/r04_knobs_ab.txt, same box, two rounds of five passes each): off 199.2 / 199.2 frames/s, 0 blocks 200.0 /
        # 199.5, 12 blocks 205.8 / 206.2, all 24 blocks 203.6 / 203.6 -> 12 (M 4.66 ms per call, P + F 4.63).  -1 = off.
        self.bw_head_blocks = min(self.nb, max(-1, int(getattr(config, 'bw_head_blocks', None) if getattr(config, 'bw_head_blocks', None) is not None
                                                         else os.environ.get('REFVSR_BW_HEAD_BLOCKS', '12'))))
        self.warp_up2 = not env_flag('REFVSR_NO_WARP_UP2')          # A/B knob: flow_up2 as its own launch + 2x flow map (round 3)
        self.fuse_head = not env_flag('REFVSR_NO_FUSE_HEAD')        # A/B knob: bicubic base map + generic planar conv (round 3)
        # conv_hr + head as ONE launch on the fused block's skeleton (refvsr_conv_hr_last): bit-identical to the two launches, 112 vs
        # 132 us stand-alone at 1080p, but NEUTRAL in the frame (209.3 / 209.9 vs 210.1 / 210.1 frames/s, profiles/
        # r04_tail_and_mfid_run.log: the HR intermediate it saves is 6 % of a launch pair that a 19 % larger conv1 pays for) -> opt-in
        self.fuse_tail = self.fuse_head and (env_flag('REFVSR_FUSE_TAIL') or bool(getattr(config, 'fuse_tail', False)))
        self.fuse_conf = not env_flag('REFVSR_NO_FUSE_CONF')        # A/B knob: confidence fusions as separate launches (round 3)
        # the 1x1 map that ends the matching's feature extractor on its own HBM-bound kernel (refvsr_conv1x1_f32) instead of the
        # generic conv's fp32 mode (118 us at 270 x 480 for 33 MB of reads); A/B knob REFVSR_NO_MAP1X1=1
        self.map1x1 = not env_flag('REFVSR_NO_MAP1X1')
        # A/B knob REFVSR_LEGACY_PREP=1: the per-frame preparation's launch list before the one-launch pyramid / frame preparation, the
        # LDS-tile patch-row kernel and the flagged-only LR lo rows (bit-identical results, profiles/match_prep_ab.txt)
        self.legacy_prep = env_flag('REFVSR_LEGACY_PREP')
        self.last_flagged = None                            # flagged list of the last feature_match (int32 [1 + n], [0] = count; tests)
        self.spynet_batch = not env_flag('REFVSR_NO_SPYNET_BATCH')   # A/B knob: one SPyNet pass per flow, as in round 3
        self.overlap = bool(getattr(config, 'overlap_streams', True)) and not env_flag('REFVSR_NO_OVERLAP')
        self._side = None
        # pipelined mode (opt-in, see forward()): internal streams M (backward branch + upsampler), F (forward branch),
        # P (per-frame preparation + flows); the caller's stream only receives the result
        self.pipelined = bool(getattr(config, 'pipelined', False))
        self._zero_maps = {}
        # result format (round 6, extension; default 'float32' = the reference's): 'float16' | 'uint8' -- the output head stores
        # rint(255 v) itself (REFVSR_RESULT_U8: the bytes eval_qual_quan.py:117-119 writes to the PNG), a quarter of the bytes to copy
        self.result_dtype = str(getattr(config, 'result_dtype', None) or 'float32').replace('torch.', '')
        ops.result_format(self.result_dtype)
        # result layout (extension; default 'chw' = planar): 'hwc' -- the output head stores the frame interleaved (REFVSR_RESULT_HWC),
        # the result is the [3, sh, sw] view of dense [sh, sw, 3] memory: what image writers and encoders consume, the same values
        self.result_layout = ops.check_result_layout(getattr(config, 'result_layout', None))
        # Y'CbCr 4:2:0 copies of the results (extension; default None = off, no launch): the network calls also return 'yuv', one
        # refvsr_result_to_yuv420 launch per call on the stream that receives 'result' (model.py:Network._with_yuv)
        self.result_yuv = yuv.resolve(getattr(config, 'result_yuv', None), getattr(config, 'yuv_matrix', None), getattr(config, 'yuv_range', None))
        # (its chroma siting, checked while the feature is off too and read by Network._with_yuv beside the format: both are this
        # engine's, from its construction; anything but 4:2:0 / centre goes through refvsr_result_to_yuv)
        self.result_yuv_siting = yuv.resolve_siting(getattr(config, 'yuv_siting', None))
        # Y'CbCr 4:2:0 input frames (extension; default None = off): the windows' input source (inputs.py) is the 4:2:0 one
        self.input_yuv = yuv.resolve_input(getattr(config, 'input_yuv', None), getattr(config, 'input_yuv_matrix', None),
                                           getattr(config, 'input_yuv_range', None), getattr(config, 'input_yuv_chroma', None),
                                           getattr(config, 'input_yuv_siting', None))
        self._pipe = None
        # stream layout of the pipelined mode when nothing is configured: 'pf_m' for one forward() per frame (round 4); an engine that
        # is driven through forward_group switches to 'pfm' (P | F | M) at its first group: with the backward branches batched the
        # P + F stream is the critical path (P 2.9 + F 1.9 ms per frame = the frame, M idle a third of the time); with F on its own
        # stream the forward-branch chain runs under the preparation of the group's new frames -- same box, G = 4: 213.1 (pf_m) /
        # 216.9 (p_fm) / 227.5 (pfm) frames/s, 228.9 with the backward head on M as well (profiles/r05_group_layout_ab.txt)
        self._layout_default = None               # None: by model (see _pipe_streams); forward_group / forward_multi set 'pfm'
        self.pipe_depth = max(1, int(getattr(config, 'pipe_depth', None) or os.environ.get('REFVSR_PIPE_DEPTH') or 3))
        self._inflight = collections.deque()
        self.stream_events = None      # bench.py: list collecting per-call section events of the pipelined mode's streams
        self.kernel_events = None      # bench.py: list collecting (start, end) HIP events of match_top2 launches
        self.chain_events = None       # bench.py: list collecting (start, end, blocks, h, w) of the fused-ResBlock runs
        self.reset_state()

    # ------------------------------------------------------------------ state
    def reset_state(self):
        self.fw_feat = None
        self.fw_flow = None
        self.fw_feat_up = None
        self.fw_conf = None
        self.frame_itr_num = 0
        self.max_frame_itr_num = self.cfg.reset_branch
        self.prev_window = []
        self.flow_cache = {}
        self.id_cache = {}
        self.ctx_pinned = {}
        self.ctx_strict = False
        self._fw_up_wait = None              # split hand-off: makes the current stream wait for fw_feat_up's arrival (import_state_head)

    def drain(self):
        """The host waits for everything this engine has in flight on its internal streams.  Called before the packed weights are
        replaced: the calls in flight read the old blobs on the internal streams, where nothing records them for the allocator."""
        for st in set(self._pipe or ()) | ({self._side} if self._side is not None else set()):
            st.synchronize()
        self._inflight.clear()

    def set_pipelined(self, on=True):
        """Opt in to cross-call pipelining: forward() is then given `frame_ids` (one hashable id per window frame; equal ids
        <=> equal (lr, ref) content within a stream) and spreads consecutive calls over the engine's internal streams.
        Inputs: forward(..., input_ready=) says when lrs / refs are final -- None (default): the internal streams wait for the
        caller's stream as it stands at the call (always safe; since that stream also waits for the previous result, calls then
        overlap only internally); 'materialised': the caller asserts the tensors are final (pre-loaded clip; what bench.py's
        headline does); an event / stream: the producer's, e.g. a copy stream (shard.EngineExecutor).  Results are bit-identical
        to the default mode in every case."""
        self.pipelined = bool(on)

    def export_state(self):
        """Forward-branch state as planar fp32 tensors (what RefVSR.py:279-283 keeps; RefVSR_IR adds its key-frame indices,
        RefVSR_IR.py:262-272)."""
        if self.fw_feat is None:
            return None
        self._await_fw_up(self.fw_feat_up)
        st = dict(feat=ops.unpack_nhwc16(self.fw_feat, self.C), flow=self.fw_flow, feat_up=ops.unpack_nhwc16(self.fw_feat_up, self.C),
                  conf=self.fw_conf, frame_itr_num=self.frame_itr_num)
        kf = getattr(self, 'keyframe_idx', None)
        if kf is not None:
            st['keyframe_idx'] = [int(k) for k in kf]
        return st

    def import_state(self, st):
        cs = (self.C + 7) // 8 * 8                              # channel stride of the maps (C = 36 -> 40, zero padding)
        self.fw_feat = ops.pack_nhwc16(st['feat'].contiguous(), cs)
        self.fw_flow = st['flow'].contiguous()
        self.fw_feat_up = ops.pack_nhwc16(st['feat_up'].contiguous(), cs)
        self.fw_conf = st['conf'].contiguous()
        self.frame_itr_num = int(st['frame_itr_num'])
        if st.get('keyframe_idx') is not None and hasattr(self, 'keyframe_idx'):
            import numpy as np
            self.keyframe_idx = np.asarray(st['keyframe_idx'], dtype=np.int64)

    # ---- the same state as ONE contiguous device buffer in the engine's native layouts (the multi-GPU hand-off message):
    #      [64-byte header: int32 frame_itr_num, h, w, Cs (channel STRIDE of the maps: 24 / 48 / 40 for C = 36), number of
    #       key-frame indices, up to 11 key-frame indices (RefVSR_IR)] [feat fp16 HWC] [feat_up fp16 HWC] [flow fp32 planar]
    #      [conf fp32 planar] = (5 Cs * 2 + 12) * h*w + 64 bytes -- half the bytes of the planar fp32 export, no unpack / pack
    #      kernels, one message
    STATE_HEADER = 64

    def _state_cs(self):
        return (self.C + 7) // 8 * 8

    def _state_spec(self, h, w, head=False):
        """Message parts behind the header, named after the attributes they carry (head: the small message, without the 2x state)."""
        cs = self._state_cs()
        return [('fw_feat', (h, w, cs), torch.float16)] + ([] if head else [('fw_feat_up', (2 * h, 2 * w, cs), torch.float16)]) + \
               [('fw_flow', (2, h, w), torch.float32), ('fw_conf', (1, h, w), torch.float32)]

    def state_nbytes(self, h, w):
        """64 + h w (10 Cs + 12)"""
        return self.STATE_HEADER + msg_nbytes(self._state_spec(h, w))

    def _export_state_msg(self, head, kf):
        """[header | the parts of _state_spec] in a new uint8 device buffer."""
        h, w, cs = self.fw_feat.shape
        assert cs == self._state_cs() and self.fw_feat_up.shape[2] == cs and len(kf) <= 11
        spec = self._state_spec(h, w, head)
        buf = torch.empty(self.STATE_HEADER + msg_nbytes(spec), dtype=torch.uint8, device=self.fw_feat.device)
        hdr = [self.frame_itr_num, h, w, cs, len(kf)] + kf + [0] * (11 - len(kf))
        buf[:self.STATE_HEADER].view(torch.int32).copy_(torch.tensor(hdr, dtype=torch.int32), non_blocking=False)
        msg_pack(buf, self.STATE_HEADER, [getattr(self, k) for k, _, _ in spec])
        return buf

    def _import_state_msg(self, buf, head, feat_up=None):
        """Install the parts of a received state message (copies of their own), checked against this model; returns its header."""
        hdr = buf[:self.STATE_HEADER].view(torch.int32).cpu().tolist()
        itr, h, w, cs = hdr[:4]
        spec = self._state_spec(h, w, head)
        assert cs == self._state_cs() and buf.numel() == self.STATE_HEADER + msg_nbytes(spec), 'state buffer does not match this model'
        assert feat_up is None or (tuple(feat_up.shape) == (2 * h, 2 * w, cs) and feat_up.dtype == torch.float16)
        for k, t in msg_views(buf, self.STATE_HEADER, spec, clone=True).items():
            setattr(self, k, t)
        self.frame_itr_num = int(itr)
        return hdr

    def export_state_packed(self):
        if self.fw_feat is None:
            return None
        self._await_fw_up(self.fw_feat_up)
        kf = getattr(self, 'keyframe_idx', None)
        return self._export_state_msg(False, [int(k) for k in (kf if kf is not None else [])])

    def import_state_packed(self, buf):
        hdr = self._import_state_msg(buf, False)
        nk = hdr[4]
        if hasattr(self, 'keyframe_idx') and nk > 0:
            import numpy as np
            self.keyframe_idx = np.asarray(hdr[5:5 + nk], dtype=np.int64)

    # ---- the hand-off in two messages (shard.run_wavefront; VERDICT r3 "predicted >= 5.5 x": the restart-free clip is bound by its
    #      B1 chain): [header | feat | flow | conf] = (2 Cs + 12) h w + 64 bytes, what a forward-branch step touches FIRST, and the 2x
    #      state feat_up (8 Cs h w bytes, 76 % of the state, sent as it lies -- no packing copy), which the step reads only after
    #      its residual chain has been launched (_prop_step): the receiver starts its step when the small message is there and waits
    #      for the large one in the middle of it (_await_fw_up).
    split_state_ok = True                # (EngineIR reads fw_feat_up outside _prop_step: it keeps the one-message form)

    def state_head_nbytes(self, h, w):
        """64 + h w (2 Cs + 12)"""
        return self.STATE_HEADER + msg_nbytes(self._state_spec(h, w, head=True))

    def export_state_split(self):
        """(head: one uint8 device buffer, feat_up: the 2x state tensor itself)."""
        if self.fw_feat is None:
            return None
        self._await_fw_up(self.fw_feat_up)
        assert not hasattr(self, 'keyframe_idx')
        return self._export_state_msg(True, []), self.fw_feat_up

    def import_state_head(self, buf, feat_up, wait_feat_up):
        """The small message + the tensor the large one is being received into; wait_feat_up(): makes the CURRENT stream wait for
        it (called once, by the first reader of fw_feat_up)."""
        self._import_state_msg(buf, True, feat_up)
        self.fw_feat_up = feat_up
        self._fw_up_wait = wait_feat_up

    def _await_fw_up(self, feat_up):
        """Before the first read of a 2x state that may still be arriving (split hand-off)."""
        if self._fw_up_wait is not None and feat_up is self.fw_feat_up:
            w, self._fw_up_wait = self._fw_up_wait, None
            w()

    # ---- per-frame contexts ahead of their windows (shard.run_wavefront with exchange_contexts: every context is prepared by ONE
    #      rank and sent to the others whose windows need it).  A context = everything prepare_frame derives from one (lr_i, ref_i)
    #      pair (RefVSR.py:196-204,233-234,127,136); the message carries the four expensive maps [conf fp32 | idx int32 | aligned
    #      fp16 HWC | aligned_up fp16 HWC] as they lie in HBM (32.2 MB for RefVSR_small at 270p), the cheap ones (the 8-channel
    #      copy of the frame, the SPyNet pyramid) are rebuilt by the receiver from its own copy of the frame.
    CTX_FIELDS = ('conf', 'idx', 'aligned', 'aligned_up')

    def _ctx(self, fid):
        fr = self.id_cache.get(fid)
        return fr if fr is not None else self.ctx_pinned.get(fid)

    @torch.no_grad()
    def prepare_context(self, lr, ref, fid):
        """The context of frame `fid` -- its id in THIS engine's forward(frame_ids=...) / phase_a: Network names frame f of batch
        element b (b, f) -- prepared now on the current stream and kept until a window that contains the id has used it."""
        assert self.cache, 'contexts are kept by the id-keyed window cache (config.cache_windows)'
        fr = self._ctx(fid)
        if fr is None:
            fr = self.ctx_pinned[fid] = FrameCtx(lr, ref, yuv=self.input_yuv)
        with torch.cuda.device(lr.device), ops.on_stream(torch.cuda.current_stream(lr.device)):
            self.pyramid(fr)
            strict, self.ctx_strict = self.ctx_strict, False
            try:
                self.prepare_frame(fr)
            finally:
                self.ctx_strict = strict
        return fr

    def context_spec(self, fid):
        """[(field, shape, dtype)] of the message of a PREPARED context: what a receiver needs to size and slice it."""
        fr = self._ctx(fid)
        assert fr is not None and fr.conf is not None, 'context %r is not prepared' % (fid,)
        return [(k, tuple(getattr(fr, k).shape), getattr(fr, k).dtype) for k in self.CTX_FIELDS]

    @staticmethod
    def context_nbytes(spec):
        return msg_nbytes(spec, 16)                      # every part padded to 16 bytes

    @torch.no_grad()
    def export_context(self, fid):
        """One uint8 device buffer holding CTX_FIELDS of a prepared context, 16-byte aligned parts (current stream)."""
        spec = self.context_spec(fid)
        fr = self._ctx(fid)
        buf = torch.empty(self.context_nbytes(spec), dtype=torch.uint8, device=fr.conf.device)
        msg_pack(buf, 0, [getattr(fr, k) for k, _, _ in spec], 16)
        return buf

    @torch.no_grad()
    def import_context(self, lr, ref, fid, buf, spec):
        """Install a context another rank prepared: its maps are views into `buf` (kept alive by the context), the frame copy, its
        8-channel HWC form and the SPyNet pyramid are made here (current stream)."""
        assert self.cache and buf.dtype == torch.uint8 and buf.numel() == self.context_nbytes(spec)
        # A window that merely CONTAINS the frame (positions before its centre) leaves an unprepared FrameCtx in the id cache
        # (_frames): e.g. frame_num = 5 and a block starting one frame before a reset frame -- that context is filled in place,
        # like prepare_context does.  Only a context that is already PREPARED is a protocol error.
        fr = self._ctx(fid)
        assert fr is None or fr.conf is None, 'context %r exists already (prepared)' % (fid,)
        pinned = fr is None
        if fr is None:
            fr = FrameCtx(lr, ref, yuv=self.input_yuv)
        with torch.cuda.device(lr.device), ops.on_stream(torch.cuda.current_stream(lr.device)):
            if fr.lr8 is None:
                fr.lr8 = ops.pack_nhwc16(fr.lr, 8)
            self.pyramid(fr)
        for k, t in msg_views(buf, 0, spec, 16).items():
            setattr(fr, k, t)
        if pinned:
            self.ctx_pinned[fid] = fr
        return fr

    # ------------------------------------------------------------------ building blocks
    def cw(self, name):
        return self.W.conv[name]

    def _zeros(self, shape, dtype, dev):
        """Read-only zero maps (the start of a propagation branch, RefVSR.py:211-214,244-247): allocated and filled once per
        geometry instead of three fill launches (31 MB at 270p) per call.  Never written by any kernel; the one-time host
        synchronisation makes them valid on every stream."""
        key = (tuple(shape), dtype, str(dev))
        z = self._zero_maps.get(key)
        if z is None:
            if len(self._zero_maps) > 12:
                # kernels queued on the internal streams may still be reading the maps that are dropped here (they carry no
                # record_stream): the device is drained first, then the allocator may reuse them (reached only by a
                # process that walks through more than twelve geometries)
                torch.cuda.synchronize(dev)
                self._zero_maps.clear()
            z = self._zero_maps[key] = torch.zeros(shape, dtype=dtype, device=dev)
            torch.cuda.current_stream(dev).synchronize()
        return z

    def _chain(self, make, pairs, *dev):
        """The table of a run of fused blocks, make(pairs, *dev) (ops.ResblockChain: the generic kernel's pointer table; the ops.BlobChain
        of the 24- or the 48-channel kernel), built once per run and kept with the packed weights it points into."""
        chains = self.W.chains
        key = (make,) + tuple(id(c1) for c1, _ in pairs)
        ch = chains.get(key)
        if ch is None:
            ch = chains[key] = make(pairs, *dev)
        return ch

    def _head_blob(self, key, pack, names, dev):
        """A blob of the output head, pack(w, b, ...) of the raw weights of the convs `names`: packed once, kept with the weights."""
        blob = self.W.chains.get(key)
        if blob is None:
            blob = self.W.chains[key] = pack(*[t for n in names for t in self.cw(n).raw]).to(dev).contiguous()
        return blob

    def _block_chain(self, x, pairs, act):
        return self._block_chain_b([x], pairs, act)[0]

    def _block_chain_b(self, xs, pairs, act):
        """A run of residual blocks x <- x + conv2(act(conv1 x)) over the B >= 1 maps xs (list in, list out); pairs = [(conv1,
        conv2), ...] packed weights.  One launch per block over all maps (the 24- and 48-channel fused kernels), else map by map:
        one launch per block (generic fused kernel) or two (fuse_resblocks off / unsupported channel count).
        (A kernel chaining TWO blocks per launch with halo recomputation was built in round 1 and measured in round 2:
        29.3 us vs 2 x 14.7 us on the LR maps, slower on the 2x maps and 4 % slower end to end -- removed.)"""
        h, w, c = xs[0].shape
        if self.fuse_resblocks and self.rb24 and c == 24 and pairs[0][0].raw is not None:
            # mid_channels = 24 (the RefVSR_small family): the compile-time-specialised kernel, one blob per block
            ch = self._chain(ops.Resblock24Chain, pairs, xs[0].device)
            if self.chain_events is None:
                return list(ops.resblock24_chain_b(ch, xs, act, stack=False))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = list(ops.resblock24_chain_b(ch, xs, act, stack=False))
            e1.record()
            self.chain_events.append((e0, e1, len(pairs), h, w) + ((len(xs),) if len(xs) > 1 else ()))
            return out
        if self.rb48 and c == 48 and pairs[0][0].raw is not None and 0.0 <= act <= 1.0 and h * w <= self.rb48_max_pixels:
            # mid_channels = 48 (RefVSR / RefVSR_MFID / RefVSR_MFID_8K): one launch per block, the two 84 KB weight sets swap
            # per tile through LDS-DMA (csrc/resblock48.hip); the intermediate map never reaches HBM.  Maps up to 540 x 960:
            # per block 12.9 vs 23.5 us at 135 x 240, 26.7 vs 30.2 us at 270 x 480 (RefVSR_MFID 85.0 vs 83.2 frames/s); at
            # 1080 x 1920 the two forms are equal stand-alone (396 vs 405 us: 32 tiles per workgroup, each swapping 168 KB of
            # weights, against conv48's 16 x 32 tiles on sixteen waves) and the 1080p -> 8K frame is 0.7 % slower with the fused
            # block (6.76 vs 6.81 frames/s) -> the large maps keep the two launches (profiles/r04_resblock48.txt)
            ch = self._chain(ops.Resblock48Chain, pairs, xs[0].device)
            if len(xs) == 1 or self.rb48_multimap:
                return list(ops.resblock48_chain_b(ch, xs, act, stack=False))
            return [ops.resblock48_chain(ch, x, act) for x in xs]
        if self.fuse_resblocks and self.chain_calls and ops.resblock_chain_ok(c):
            # one library call per run (same launches, same results): 156 of the ~330 launches of a frame
            ch = self._chain(ops.ResblockChain, pairs)
            return [ops.resblock_chain(ch, x, act) for x in xs]
        out = []
        for x in xs:
            for c1, c2 in pairs:
                if self.fuse_resblocks:
                    x = ops.resblock(c1, c2, x, act=act)
                else:
                    t = ops.conv(c1, x, act=act)
                    x = ops.conv(c2, t, res=x)
            out.append(x)
        return out

    # The layers below are written ONCE, over lists of B >= 1 maps (`_b`: lists in, lists out): the ops.*_b wrappers issue one
    # multi-map launch per layer for B >= 2 and hand a list of one map straight to the single-map op.  The unsuffixed names are the
    # same layers for callers that hold single maps.
    def res_list_b(self, xs, name, n):
        """ResList (RefVSR_/common.py:64-82) with ResBlocks (:25-39)."""
        pairs = [(self.cw('%s.RBs.%d.conv1' % (name, i)), self.cw('%s.RBs.%d.conv2' % (name, i))) for i in range(n)]
        ys = self._block_chain_b(xs, pairs, 0.2)
        return list(ops.conv_b(self.cw(name + '.conv_tail'), ys, ress=xs, stack=False))

    def res_list(self, x, name, n):
        return self.res_list_b([x], name, n)[0]

    def resblocks_b(self, lr8s, feats, name, stop=None, resume=None):
        """ResidualBlocksWithInputConv (RefVSR.py:327-360); torch.cat([lr, feat]) fused as two sources.
        stop = n: only the input conv and the first n blocks (returns the intermediate maps); resume = (n, maps): the blocks from n
        on -- the two halves of one call, for running them on different streams (same launches, same results)."""
        pairs = [(self.cw('%s.main.2.%d.conv1' % (name, i)), self.cw('%s.main.2.%d.conv2' % (name, i)))
                 for i in range(self.nb)]
        if resume is not None:
            n, xs = resume
            return self._block_chain_b(xs, pairs[n:], 0.0) if n < self.nb else xs
        xs = list(ops.conv_b(self.cw(name + '.main.0'), lr8s, feats, act=0.1, stack=False))
        if stop is not None:
            return self._block_chain_b(xs, pairs[:stop], 0.0) if stop > 0 else xs
        return self._block_chain_b(xs, pairs, 0.0)

    def resblocks(self, lr8, feat, name, stop=None):
        return self.resblocks_b([lr8], [feat], name, stop)[0]

    def pyramid(self, fr):
        """SPyNet.forward resize-to-/32 + normalise + 5x avg_pool2d (SPyNet.py:62-81,117-126)."""
        if fr.pyr is None:
            h, w = fr.lr.shape[1:]
            w_up = w if w % 32 == 0 else 32 * (w // 32 + 1)
            h_up = h if h % 32 == 0 else 32 * (h // 32 + 1)
            lv = [ops.resize(fr.lr, (h_up, w_up), ops.RS_BILINEAR, mean=VGG_MEAN, std=VGG_STD)]
            if self.legacy_prep:
                for _ in range(5):
                    lv.append(ops.avgpool2(lv[-1]))
            else:
                lv += ops.avgpool_pyramid(lv[0])
            fr.pyr = lv[::-1]
        return fr.pyr

    def flow(self, fr_ref, fr_supp, share=None):
        """FlowNet(ref, supp) (SPyNet.py:49-139), cached per ordered frame pair.  `share`: streams that will consume
        the result besides the current one (pipelined mode): the tensor is recorded on them and carries an event."""
        key = (fr_ref.uid, fr_supp.uid)
        hit = self.flow_cache.get(key)
        if hit is not None:
            out, ev = hit
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
                out.record_stream(torch.cuda.current_stream())
            return out
        for f in (fr_ref, fr_supp):
            if f.ready is not None:
                torch.cuda.current_stream().wait_event(f.ready)
        pr, ps = self.pyramid(fr_ref), self.pyramid(fr_supp)
        h, w = fr_ref.lr.shape[1:]
        flow = None
        for lvl in range(6):
            x, fup = ops.spynet_level_input(pr[lvl], ps[lvl], flow)
            p = 'FlowNet.basic_module.%d.basic_module.' % lvl
            small = x.shape[0] * x.shape[1] <= self.spynet_mt1_pixels
            for j in range(4):
                cw = self.W.conv.get(p + '%d.conv/mt1' % j) if small else None
                x = ops.conv(cw if cw is not None else self.cw(p + '%d.conv' % j), x, act=0.0)
            flow = ops.conv(self.cw(p + '4.conv'), x, planar_out=True, res_planar=fup)
        h_up, w_up = flow.shape[1:]
        out = ops.resize(flow, (h, w), ops.RS_BILINEAR, chan_mul=[float(w) / float(w_up), float(h) / float(h_up)])
        ev = None
        if share:
            ev = torch.cuda.Event()
            ev.record()
            for st in share:
                out.record_stream(st)
        self.flow_cache[key] = (out, ev)
        return out

    def flows(self, pairs, share=None):
        """FlowNet for several ordered frame pairs [(ref frame, supp frame), ...].  The pairs that are not cached yet are
        computed TOGETHER, one launch per layer over all of them (RefvsrConv.batch; the reference calls SPyNet once per pair,
        SPyNet.py:49-104, RefVSR.py:182-191): same weights, same shapes, and the coarse pyramid levels are launches of 2-36
        workgroups -- two flows per launch cost about what one does.  Results equal flow() pair by pair, bit for bit."""
        todo = []
        for a, b in pairs:
            if (a.uid, b.uid) not in self.flow_cache and all((a.uid, b.uid) != (x.uid, y.uid) for x, y in todo):
                todo.append((a, b))
        if len(todo) >= 2 and self.spynet_batch:
            for i0 in range(0, len(todo), 8):         # (a frame group of four asks for eight flows: ONE pass -- the coarse levels are
                chunk = todo[i0:i0 + 8]               #  launches of 2-36 workgroups per image; 222.5 vs 220.6 frames/s with two passes of four)
                if len(chunk) >= 2:
                    self._flow_batch(chunk, share)
        return [self.flow(a, b, share) for a, b in pairs]

    def _flow_batch(self, todo, share):
        cur = torch.cuda.current_stream()
        for a, b in todo:
            for f in (a, b):
                if f.ready is not None:
                    cur.wait_event(f.ready)
        pr = [self.pyramid(a) for a, _ in todo]
        ps = [self.pyramid(b) for _, b in todo]
        B = len(todo)
        h, w = todo[0][0].lr.shape[1:]
        flow = None
        for lvl in range(6):
            x, fup = ops.spynet_level_input_batch([p_[lvl] for p_ in pr], [p_[lvl] for p_ in ps], flow)
            p = 'FlowNet.basic_module.%d.basic_module.' % lvl
            small = x.shape[1] * x.shape[2] <= self.spynet_mt1_pixels
            for j in range(4):
                cw = self.W.conv.get(p + '%d.conv/mt1' % j) if small else None
                x = ops.conv(cw if cw is not None else self.cw(p + '%d.conv' % j), x, act=0.0, batch=B)
            flow = ops.conv(self.cw(p + '4.conv'), x, planar_out=True, res_planar=fup, batch=B)
        h_up, w_up = flow.shape[2:]
        # back to the frame size, x / y components rescaled (SPyNet.py:128-137): refvsr_resize takes <= 4 channels with
        # per-channel factors = two flows per launch
        cm = [float(w) / float(w_up), float(h) / float(h_up)]
        outs = [ops.resize(flow[b0:b0 + 2].reshape(-1, h_up, w_up), (h, w), ops.RS_BILINEAR, chan_mul=cm * min(2, B - b0))
                for b0 in range(0, B, 2)]
        out = outs[0].view(-1, 2, h, w) if len(outs) == 1 else torch.cat([o_.view(-1, 2, h, w) for o_ in outs], 0)
        ev = None
        if share:
            ev = torch.cuda.Event()
            ev.record()
            for st in share:
                out.record_stream(st)
        for i, (a, b) in enumerate(todo):
            self.flow_cache[(a.uid, b.uid)] = (out[i], ev)

    def frame_prep(self, fr):
        """(lr8, ref8, packed MeanShift(lr), packed avg_pool2(MeanShift(ref))) of a frame in one launch; None where the matching
        resizes the normalised frames first (HD) or the legacy launch list is asked for."""
        if self.hd or self.legacy_prep:
            return None
        return ops.frame_prep(fr.lr, fr.ref, *self.W.raw['feature_match.sub_mean'])

    def feature_match(self, fr, prep=None):
        """FeatureMatching.forward (RefVSR_/attention.py:58-100), fused GEMM+argmax.  prep: self.frame_prep(fr) if the caller has it."""
        R = self.W.raw
        h, w = fr.lr.shape[1:]

        fe = 'feature_match.feature_extract.'

        def extract(x):       # VGG19 head + 1x1 map in exact fp32 on v_mfma_f32_16x16x4_f32 (attention.py:31-42); x: packed fp32 [h,w,4]
            x = ops.conv(self.cw(fe + '0'), x, act=0.0)
            if not self.vgg7:
                x = ops.conv(self.cw(fe + '2'), x, act=0.0)
                if self.map1x1:
                    return ops.conv1x1_f32(x, *R[fe + 'map64.0'], act=0.2)
                return ops.conv(self.cw(fe + 'map64.0'), x, act=0.2, planar_out=True)
            x = ops.conv(self.cw(fe + '2'), x, act=0.0, planar_out=True)
            x = ops.pack_nhwc32(ops.maxpool2(x))                                   # VGG19[4]
            x = ops.conv(self.cw(fe + '5'), x, act=0.0)
            if self.map1x1:
                return ops.conv1x1_f32(x, *R[fe + 'map128.0'], act=0.2)
            return ops.conv(self.cw(fe + 'map128.0'), x, act=0.2, planar_out=True)
        if prep is None:
            prep = self.frame_prep(fr)
        if prep is not None:
            lr_n, ref_n = prep[2], prep[3]
        else:
            lr_n = ops.conv_direct(fr.lr, *R['feature_match.sub_mean'])
            ref_n = ops.conv_direct(fr.ref, *R['feature_match.sub_mean'])
            if self.hd:                                                            # attention.py:65-67
                f = 1.0 / (self.cfg.scale // 2)
                oh, ow = int(h * f), int(w * f)
                lr_n = ops.resize(lr_n, (oh, ow), ops.RS_NEAREST, (1.0 / f, 1.0 / f))
                ref_n = ops.resize(ref_n, (oh, ow), ops.RS_NEAREST, (1.0 / f, 1.0 / f))
            lr_n, ref_n = ops.pack_nhwc32(lr_n, 4), ops.pack_nhwc32(ops.avgpool2(ref_n), 4)
        lr_f = extract(lr_n)
        ref_f = extract(ref_n)
        ops.set_match_patches_kernel(0 if self.legacy_prep else 1)
        if self.legacy_prep:
            lr_rows, inv_lr, lr_lo = ops.match_patches(lr_f, ops.hip.MATCH_COLBLOCK, want_lo=True)
        else:       # the search reads the LR lo rows of the flagged columns only: match_refine writes those after the flagging
            (lr_rows, inv_lr), lr_lo = ops.match_patches(lr_f, ops.hip.MATCH_COLBLOCK), None
        ref_rows, inv_ref, ref_lo = ops.match_patches(ref_f, ops.hip.MATCH_ROWCHUNK, want_lo=True)
        n_lr = lr_f.shape[1] * lr_f.shape[2]
        n_ref = ref_f.shape[1] * ref_f.shape[2]
        if self.kernel_events is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        cand, cand_val = ops.match_top2(ref_rows, n_ref, lr_rows, n_lr, self.match_row_splits)
        if self.kernel_events is not None:
            e1.record()
            self.kernel_events.append((e0, e1))
        # exact fp32 re-rank of the top-2 + exhaustive fp32-grade (split-fp16) search of the columns the fp16 GEMM cannot decide
        conf, idx, self.last_flagged = ops.match_refine(lr_f, ref_f, inv_lr, inv_ref, cand, cand_val, self.match_margin, (lr_rows, lr_lo),
                                                        (ref_rows, ref_lo))
        conf = conf.view(1, lr_f.shape[1], lr_f.shape[2])
        grid = (lr_f.shape[1], lr_f.shape[2])
        if grid[0] != h:                                                           # attention.py:96-98 (HD)
            conf = ops.bicubic_scale(conf, float(h) / grid[0], clamp01=True)
        return conf, idx, grid

    def aligned_conv(self, feats, query, rgb8, prefix, ks):
        """AlignedConv2d.forward (RefVSR_/alignment.py:39-100); query: planar fp32 [3,.,.] (bicubic x2 inside)."""
        def enc(z8):
            e = ops.conv(self.cw(prefix + '.conv1.0'), z8, act=0.2)
            t = ops.conv(self.cw(prefix + '.conv1.2.conv1'), e, act=0.2)
            return ops.conv(self.cw(prefix + '.conv1.2.conv2'), t, res=e, post=0.2)
        q = enc(ops.bicubic_scale(query, 2, clamp01=False, nhwc16_out=True))
        r = enc(rgb8)
        a = ops.conv(self.cw(prefix + '.p_conv.0'), r, q, stride=ks, act=0.2)
        t = ops.conv(self.cw(prefix + '.p_conv.2.conv1'), a, act=0.2)
        a = ops.conv(self.cw(prefix + '.p_conv.2.conv2'), t, res=a, post=0.2)
        affine = ops.conv(self.cw(prefix + '.p_conv.4'), a, planar_out=True, add_const=1.0, clamp=(-3.0, 3.0))
        return ops.aligned_sample(feats, affine, ks)

    def _ref_encoders(self, fr, ref8=None):
        """ref_feat = res1(ref_encoder1(ref)), ref_feat_down = res2(ref_encoder2(ref_feat))  (RefVSR.py:233-234)."""
        if ref8 is None:
            ref8 = ops.pack_nhwc16(fr.ref, 8)
        x = ops.conv(self.cw('ref_encoder1.0.0'), ref8, act=0.2)
        x = ops.conv(self.cw('ref_encoder1.1.0'), x, act=0.2)
        ref_feat = self.res_list(x, 'res1', 4)
        x = ops.conv(self.cw('ref_encoder2.0.0'), ref_feat, stride=2, act=0.2)
        x = ops.conv(self.cw('ref_encoder2.1.0'), x, act=0.2)
        return ref_feat, self.res_list(x, 'res2', 4)

    def prepare_frame(self, fr):
        """Everything that is a function of (lr_i, ref_i) only: matching (RefVSR.py:196-204), reference
        encoders (:233-234) and both AlignedAttention outputs (:127,136)."""
        if fr.conf is not None:
            return
        if self.ctx_strict:
            # shard.run_wavefront(exchange_contexts=True): every context a window needs was prepared ahead (prepare_context) or
            # received (import_context); preparing one here would silently redo another rank's work
            raise RuntimeError('a window needs a per-frame context that was neither prepared ahead nor imported (strict mode)')
        h, w = fr.lr.shape[1:]
        prep = self.frame_prep(fr)
        fr.lr8 = prep[0] if prep is not None else ops.pack_nhwc16(fr.lr, 8)
        # (running the reference encoders on a side stream underneath the matching kernel measured neutral, +0..1 %: removed in round 5)
        fr.conf, fr.idx, (gh, gw) = self.feature_match(fr, prep)
        ref_feat, ref_feat_down = self._ref_encoders(fr, prep[1] if prep is not None else None)
        s1, s2 = self.ks // 2, self.ks
        # aa1 (RefVSR.py:127, attention.py:142-157): gather of LR/2 reference features; with a patch > 1 px (HD)
        # also the affine AlignedConv2d, queried by bicubic x0.5 of the LR frame (RefVSR.py:125)
        feats1 = ops.block_gather_nhwc16(ref_feat_down, fr.idx, gh, gw, s1)
        if s1 > 1:
            rgb1 = ops.block_gather_rgb(fr.ref, fr.idx, gh, gw, s1)
            lr_down = ops.bicubic_scale(fr.lr, 0.5, clamp01=True)
            fr.aligned = self.aligned_conv(feats1, lr_down, rgb1, 'aa1.align', s1)
        else:
            fr.aligned = feats1
        feats2 = ops.block_gather_nhwc16(ref_feat, fr.idx, gh, gw, s2)                   # aa2 (RefVSR.py:136)
        rgb2 = ops.block_gather_rgb(fr.ref, fr.idx, gh, gw, s2)                          # attention.py:152-154
        fr.aligned_up = self.aligned_conv(feats2, fr.lr, rgb2, 'aa2.align', s2)

    def _conf_alpha(self, fused, name, up, conf_props, confs, pairs):
        """The alpha maps of the confidence fusion `name` (RefVSR.py:130, :140-142) for B maps.  fused: cat + both convs (+ the bicubic
        x2 for up = 2, + the torch.max of :147 for up = 1: returns (alphas, maxima)) in one launch.  Else the separate launches, map
        by map, on pairs[b] = cat[conf_prop, conf] [2,h,w] (REFVSR_NO_FUSE_CONF, blobs without the fused kernel)."""
        w0, cw = self.W.raw[name + '.0.0'], self.cw(name + '.1.0')
        if fused:
            return ops.conf_alpha_b(conf_props, confs, up, *w0, cw, want_max=up == 1, stack=False)
        alphas = []
        for p in pairs:
            if up == 2:
                p = ops.bicubic_scale(p, 2, clamp01=True)                                # :140-141
            a = ops.conv_direct(p, *w0, act=0.2, nhwc16_out=True)
            alphas.append(ops.conv(cw, a, act=0.2))
        return alphas

    def rap_b(self, fs, conf_props, feats, feat_ups):
        """AA_AF_conf_prop (RefVSR.py:123-149) of B independent (frame, carried maps) tuples."""
        confs = [f.conf for f in fs]
        fused = self.fuse_conf and ops.conf_alpha_ok(self.cw('conf_fusion.1.0')) and ops.conf_alpha_ok(self.cw('conf_fusion2.1.0'))
        pairs = None if fused else [torch.cat([p, c], 0) for p, c in zip(conf_props, confs)]     # [2,h,w] (:130)
        alpha = self._conf_alpha(fused, 'conf_fusion', 1, conf_props, confs, pairs)
        if fused:
            alpha, conf_next = alpha
        t = ops.conv_b(self.cw('feat_fusion.0.0'), feats, [f.aligned for f in fs], act=0.2, stack=False)
        feat = list(ops.conv_b(self.cw('feat_fusion.1.0'), list(t), act=0.2, muls=list(alpha), ress=feats, stack=False))     # :131
        feat = self.res_list_b(feat, 'feat_decoder', 8)
        up1 = ops.conv_b(self.cw('upsample1.upsample_conv'), feat, stack=False)          # :138 (pixel shuffle fused)
        feat_up = list(ops.conv_b(self.cw('feat_fusion2_1.0.0'), feat_ups, list(up1), act=0.2, stack=False))
        alpha2 = self._conf_alpha(fused, 'conf_fusion2', 2, conf_props, confs, pairs)    # :140-142
        t = ops.conv_b(self.cw('feat_fusion2.0.0'), feat_up, [f.aligned_up for f in fs], act=0.2, stack=False)
        feat_up = list(ops.conv_b(self.cw('feat_fusion2.1.0'), list(t), act=0.2, muls=list(alpha2), ress=feat_up, stack=False))   # :143
        feat_up = self.res_list_b(feat_up, 'feat_decoder2', 4)
        if not fused:
            conf_next = [ops.max2(p, c) for p, c in zip(conf_props, confs)]              # :147
        return feat, feat_up, list(conf_next)

    def rap(self, fr, conf_prop, feat, feat_up):
        feat, feat_up, conf_next = self.rap_b([fr], [conf_prop], [feat], [feat_up])
        return feat[0], feat_up[0], conf_next[0]

    def compute_up(self, bw_up, fw_up, conf_bw, conf_fw, lr_center):
        """compute_up + base (RefVSR.py:104-119,288) + final clamp (:297)."""
        R = self.W.raw
        fus = ops.conv(self.cw('fusion_UP'), bw_up, fw_up)
        if self.fuse_conf and ops.conf_alpha_ok(self.cw('conf_fusion_BWFW.1.0')):
            alpha = ops.conf_alpha(conf_bw, conf_fw, 2, *R['conf_fusion_BWFW.0.0'], self.cw('conf_fusion_BWFW.1.0'))   # :107-109
        else:
            pair_up = ops.bicubic_scale(torch.cat([conf_bw, conf_fw], 0), 2, clamp01=True)
            a = ops.conv_direct(pair_up, *R['conf_fusion_BWFW.0.0'], act=0.2, nhwc16_out=True)
            alpha = ops.conv(self.cw('conf_fusion_BWFW.1.0'), a, act=0.2)
        t = ops.conv(self.cw('feat_fusion_BWFW.0.0'), bw_up, fw_up, act=0.2)
        out = ops.conv(self.cw('feat_fusion_BWFW.1.0'), t, act=0.2, mul=alpha, res=fus)
        out = self.res_list(out, 'feat_decoder_BWFW', 4)
        if self.cfg.scale == 4:                                               # :114-115
            out = ops.conv(self.cw('upsample2.upsample_conv'), out, act=0.1)  # lrelu commutes with pixel_shuffle
        if self.fuse_tail and self.C == 24 and ops.conv_last_ok(24, out.shape[0], out.shape[1]):
            # conv_hr + conv_last + the bicubic base + the clamps in one launch: the HR map between the two convs stays in LDS
            blob = self._head_blob('conv_hr_last_blob', pack_conv_hr_last, ('conv_hr', 'conv_last'), out.device)
            return ops.conv_hr_last(blob, out, lr_center, act=0.1, result_dtype=self.result_dtype, result_layout=self.result_layout)
        out = ops.conv(self.cw('conv_hr'), out, act=0.1)
        if self.fuse_head and ops.conv_last_ok(self.C, out.shape[0], out.shape[1]):
            # conv_last + the bicubic base + the clamps in one launch: the base map is evaluated per output value
            blob = self._head_blob('conv_last_blob', pack_conv_last, ('conv_last',), out.device)
            return ops.conv_last(blob, out, lr_center, result_dtype=self.result_dtype, result_layout=self.result_layout)
        base = ops.bicubic_scale(lr_center, self.cfg.scale, clamp01=True)
        return ops.convert_result(ops.conv(self.cw('conv_last'), out, planar_out=True, res_planar=base, clamp=(0.0, 1.0)), self.result_dtype,
                                  self.result_layout)

    # ------------------------------------------------------------------ window bookkeeping
    def _frames(self, lrs, refs, frame_ids=None, ingest=None):
        """Wrap the t frames of this window, reusing per-frame contexts of the previous window (or of earlier positions in this window)
        whose content is identical -- or, when the caller supplies frame ids, whose id matches (no device work, no synchronisation).
        The new contexts' decodes (inputs.py) run as one launch at the end, or stay in the caller's `ingest` list (one over several windows)."""
        return self._frames_group([(lrs, refs, frame_ids)], ingest)[0]

    def _frames_group(self, wins, ingest=None):
        """_frames for the B >= 1 windows [(lrs, refs, frame_ids)] of a call; B >= 2: named by frame ids."""
        pend = [] if ingest is None else ingest
        out = [self._window_frames(*wins[0], pend)] if len(wins) == 1 else self._id_frames(wins, pend)
        if ingest is None:
            self._source(wins[0]).decode(pend)
        return out

    def _source(self, win):
        """The input source (inputs.source_of) of a window (lrs, refs, ..); the windows of one call are of one kind."""
        return inputs.source_of(win[0], win[1], self.input_yuv)

    def _geometry(self, lrs):
        """(t, h, w) of a window of any kind: [t,3,h,w] RGB frames, or [t, 3h/2, w] 4:2:0 frames under config.input_yuv."""
        return (lrs.shape[0],) + tuple(self._source((lrs, lrs)).geometry(lrs))

    def _id_frames(self, wins, pend):
        """The id-keyed lookup for B >= 1 windows: a frame's context comes from the id cache, else from the contexts prepared / imported
        ahead of their first window (prepare_context), else it is new.  The cache keeps the union of the windows' frames."""
        if self.id_cache and tuple(next(iter(self.id_cache.values())).lr.shape[1:]) != self._geometry(wins[0][0])[1:]:
            self.id_cache, self.flow_cache = {}, {}
        out = []
        for lrs, refs, ids in wins:
            assert len(ids) == lrs.shape[0]
            for i, fid in enumerate(ids):
                if fid not in self.id_cache:
                    self.id_cache[fid] = self.ctx_pinned.pop(fid, None) or FrameCtx(lrs[i], refs[i], pend, self.input_yuv)
            out.append([self.id_cache[fid] for fid in ids])
        keep = set(fid for _, _, ids in wins for fid in ids)
        self.id_cache = {k: v for k, v in self.id_cache.items() if k in keep}
        self._keep_flows(out)
        return out

    def _keep_flows(self, frs):
        """The flow cache keeps the pairs of the windows `frs`; the last one is the previous window of the next call."""
        live = set(f.uid for fr in frs for f in fr)
        self.flow_cache = {k2: v for k2, v in self.flow_cache.items() if k2[0] in live and k2[1] in live}
        self.prev_window = frs[-1]

    def _window_frames(self, lrs, refs, frame_ids, pend):
        t = lrs.shape[0]
        frames = [None] * t
        if frame_ids is not None and self.cache:
            return self._id_frames([(lrs, refs, frame_ids)], pend)[0]
        if not self.cache:
            self.flow_cache = {}
            return [FrameCtx(lrs[i], refs[i], pend, self.input_yuv) for i in range(t)]
        prev = self.prev_window
        if prev and tuple(prev[0].lr.shape[1:]) != self._geometry(lrs)[1:]:          # new clip geometry: nothing to reuse
            prev = []
            self.flow_cache = {}
        source = self._source((lrs, refs))                       # (8-bit and 4:2:0 frames: compared with the contexts' source copies)
        kind, same, own = source.key, source.equal, source.own
        if prev:
            # candidates in order of likelihood: the window slid by one (i+1), did not move (i), slid back (i-1);
            # all candidate pairs are compared by ONE kernel launch + one D2H sync
            cand = [(i, i + sh) for sh in (1, 0, -1) for i in range(t) if 0 <= i + sh < len(prev) and prev[i + sh].kind == kind]
            flags = same([x for i, j in cand for x in ((lrs[i], own(prev[j])[0]), (refs[i], own(prev[j])[1]))])
            for n_, (i, j) in enumerate(cand):
                if frames[i] is None and flags[2 * n_] and flags[2 * n_ + 1]:
                    frames[i] = prev[j]
        # repeated frames inside this window (clip edges replicate frames, datasets.py:233-234)
        fresh = [i for i in range(t) if frames[i] is None]
        if len(fresh) > 1:
            pp = [(a, b) for ai, a in enumerate(fresh) for b in fresh[ai + 1:]]
            eq = same([x for a, b in pp for x in ((lrs[a], lrs[b]), (refs[a], refs[b]))])
            for n_, (a, b) in enumerate(pp):
                if eq[2 * n_] and eq[2 * n_ + 1]:
                    if frames[a] is None:
                        frames[a] = FrameCtx(lrs[a], refs[a], pend, self.input_yuv)
                    if frames[b] is None:
                        frames[b] = frames[a]
        for i in range(t):
            if frames[i] is None:
                frames[i] = FrameCtx(lrs[i], refs[i], pend, self.input_yuv)
        self._keep_flows([frames])
        return frames

    # ------------------------------------------------------------------ pipelined forward (opt-in)
    def _pipe_streams(self, dev):
        """Internal streams of the pipelined mode: (M0, M1, F, P).

        Layout (REFVSR_PIPE_LAYOUT / config.pipe_layout), round 4:
          'pf_m' (default)  TWO internal streams: P carries the per-frame preparation AND the forward-branch step (F is P),
                            M the backward branch + upsampler.  With the caller's stream (which only receives the result) that
                            is three streams for the runtime's four hardware queues: which streams share a queue is no longer
                            decided per process.  Round 3 ran P, F and M as three streams (+ the caller's): on boxes where every
                            stream got its own hardware queue THREE kernels ran concurrently -- the 254-workgroup / 152 KB-LDS
                            matching kernel and two conv chains displacing each other CU by CU -- and the rate fell from 187-196 to
                            141-155 frames/s (BENCH_r03: 140.9; profiles/r03_one_vs_two_m_streams.txt).  The fast mode of round 3 was
                            the one in which F and P happened to share a hardware queue, i.e. exactly this layout.
          'pfm'             round 3: P, F, M on three streams (kept for the A/B and the slow-mode reproduction)
          'one'             P, F and M on ONE stream (measurement aid: bench.py times the multi-map launches of a group in it)
        Wider models (C = 48 / 36) additionally alternate two M streams (for mid_channels = 24 two M streams measured equal to one,
        209.5 / 210.2 vs 209.1 / 209.6 frames/s, profiles/r04_two_m_and_mfid_layout_ab.txt: no switch)."""
        # default: P | F | M for the mid_channels = 24 models (what their frame groups run on: an engine whose FIRST pipelined call is a
        # single forward() -- a caller that sends the first window alone -- must not lay its streams out differently and rebuild them at
        # the first group: the idle first set of streams changes the stream -> hardware-queue mapping, 212 vs 231 frames/s,
        # profiles/r05_group_cut_ab.txt); P + F | M for the wider models (round 4's layout, two alternating M streams)
        # The layout is decided ONCE, when the streams are built (re-deriving it per call cost weight look-ups per launch
        # list and could rebuild the streams mid-stream); another layout needs an explicit rebuild: `engine._pipe = None` after a
        # device synchronisation (bench.py's single-stream measurement does that), a new device, or a new engine.
        if self._pipe is not None and self._pipe[0].device == dev:
            return self._pipe
        layout = str(getattr(self.cfg, 'pipe_layout', None) or os.environ.get('REFVSR_PIPE_LAYOUT') or self._layout_default or
                     ('pfm' if (self.C == 24 and self.group_ok()) else 'pf_m'))
        if layout not in ('pf_m', 'pfm', 'one'):                 # ('p_fm', F on M's stream, measured slower in rounds 4-5: removed in round 6)
            raise ValueError('REFVSR_PIPE_LAYOUT must be pf_m | pfm | one, got %r' % layout)
        two = self.C != 24
        split = str(getattr(self.cfg, 'cu_split', None) or os.environ.get('REFVSR_CU_SPLIT') or '')
        if split and layout in ('pfm', 'pf_m'):
            # CU partitions (round 6, ABI 13; measurement knob, off by default -- DESIGN 5 "CU partitions"): 'p,f,m' CUs for the
            # three streams as disjoint ranges (multiples of 8 = an equal share of every XCD); f = 0 with layout pf_m
            cp, cf, cm = (int(v) for v in split.split(','))
            p_ = ops.CuStream(0, cp, dev)
            f_ = ops.CuStream(cp, cf, dev) if (layout == 'pfm' and cf > 0) else p_
            m = ops.CuStream(cp + (cf if f_ is not p_ else 0), cm, dev)
            self._pipe = [m, m, f_, p_]
            self.pipe_layout = layout
            self._pipe_calls = 0
            return self._pipe
        m = torch.cuda.Stream(device=dev)
        if layout == 'one':                       # measurement aid (bench.py): every section on ONE internal stream -- HIP events
            two = False                           # around a run of launches then bracket nothing but that run
        m2 = torch.cuda.Stream(device=dev) if two else m
        p_ = m if layout == 'one' else torch.cuda.Stream(device=dev)
        f_ = p_ if layout in ('pf_m', 'one') else torch.cuda.Stream(device=dev)
        self._pipe = [m, m2, f_, p_]
        self.pipe_layout = layout
        self._pipe_calls = 0
        return self._pipe

    def _pipe_begin(self, tensors, input_ready, depth, streams):
        """Start of a pipelined call, after _pipe_streams.  The host waits until fewer than `depth` calls are in flight (each call
        holds its intermediates until its `done` event), then lets the internal `streams` read the inputs `tensors`:
        input_ready = 'materialised' (the caller asserts the tensors are final, e.g. a pre-loaded clip): no wait.  An event / stream:
        the internal streams wait for it (a producer on a copy stream keeps the calls pipelined).  None: wait for the caller's stream
        as it stands -- always safe, but the caller's stream also carries the wait for the previous call's result, so consecutive
        calls then overlap only inside a call.  Returns the caller's stream."""
        while len(self._inflight) >= depth:
            self._inflight.popleft().synchronize()
        caller = torch.cuda.current_stream()
        uniq = []
        for st in streams:
            if all(st is not s_ for s_ in uniq):
                uniq.append(st)
        if input_ready is None:
            input_ready = torch.cuda.Event()
            input_ready.record(caller)
        if not isinstance(input_ready, str):
            for st in uniq:
                if isinstance(input_ready, torch.cuda.Stream):
                    st.wait_stream(input_ready)
                else:
                    st.wait_event(input_ready)
        elif input_ready != 'materialised':
            raise ValueError("input_ready must be None, 'materialised', a torch.cuda.Event or a torch.cuda.Stream")
        for x in tensors:
            for st in uniq:
                x.record_stream(st)
        return caller

    def _pipe_end(self, caller, M, outs, vis=None, timing=False):
        """End of a pipelined call whose last section ran on M: the caller's stream waits for the results (and the vis dicts' maps:
        one dict or one per window) and owns them from here on, and the call counts as in flight until its `done` event (returned)."""
        done = torch.cuda.Event(enable_timing=timing)
        done.record(M)
        caller.wait_event(done)
        for o in outs:
            o.record_stream(caller)
        for d in ([vis] if isinstance(vis, dict) else vis or ()):
            for v in d.values():
                v.record_stream(caller)
        self._inflight.append(done)
        return done

    @staticmethod
    def _await_inputs(input_ready):
        """Sequential path: the current stream waits for an input_ready event / stream (None, 'materialised': nothing to wait for)."""
        if isinstance(input_ready, torch.cuda.Stream):
            torch.cuda.current_stream().wait_stream(input_ready)
        elif isinstance(input_ready, torch.cuda.Event):
            torch.cuda.current_stream().wait_event(input_ready)

    def _publish(self, f, share):
        """Make a prepared frame context safe to free while any of the `share` streams may still read it (allocator)."""
        for x in [f.lr, f.ref, f.lr8, f.conf, f.idx, f.aligned, f.aligned_up] + list(f.pyr or ()):
            for st in share:
                x.record_stream(st)

    def _prepare_window(self, fr, start, share, n_ctx=None, head=False, pyramid_first=True, ready_if_prepared=False):
        """P section of a call for one window, on the current stream -- the one place that publishes a prepared frame and records its
        `ready`: prepares fr[start:] and publishes each frame for `share`; a frame prepared here carries `ready`, the event its
        consumers on the other streams wait for.  n_ctx: frames newer than that uid were cloned by this call, their copies are
        recorded on `share` up front (None: the caller records the windows' copies itself).  head: the frame at the window's end also
        runs the first `bw_head_blocks` layers of its backward step (a function of that frame alone: load balance between the
        streams).  pyramid_first: the SPyNet pyramid of a new frame before its preparation (pipelined calls), else behind it
        (phase_a_group).  ready_if_prepared: a frame that was prepared elsewhere without `ready` (on this stream, ahead of its window:
        prepare_context / import_context) gets the event as well (phase_a_group; a pipelined call only publishes it -- what it finds
        was prepared on M by a reference-order call, behind which every internal stream waited)."""
        if n_ctx is not None:
            for f in fr:
                if f.uid > n_ctx:
                    for st in share:
                        f.lr.record_stream(st)
                        f.ref.record_stream(st)
        t = len(fr)
        for i in range(start, t):          # (a restarting forward branch walks the first frames too: cached)
            f = fr[i]
            new = f.conf is None
            if new:
                if pyramid_first:
                    self.pyramid(f)
                self.prepare_frame(f)
                if head and i == t - 1 and self.bw_head_blocks >= 0:
                    h, w = f.lr.shape[1:]
                    zf = self._zeros((h, w, self._state_cs()), torch.float16, f.lr.device)
                    f.bw_head = (self.bw_head_blocks, self.resblocks(f.lr8, zf, 'backward_resblocks', stop=self.bw_head_blocks))
                    for st in share:
                        f.bw_head[1].record_stream(st)
            if f.ready is None:
                self.pyramid(f)
                self._publish(f, share)
                if new or ready_if_prepared:
                    f.ready = torch.cuda.Event()
                    f.ready.record()

    @torch.no_grad()
    def _forward_pipelined(self, lrs, refs, is_first_frame, want_vis, frame_ids, input_ready=None):
        """Same computation as _forward_seq, spread over the internal streams so that consecutive calls overlap: P prepares the
        window's new frame and its flows while M is still walking the previous call's backward branch and F its forward-branch step.
        Round 6: a steady call IS a frame group of one window (_pipe_call: the one implementation of the P | F | M schedule for one
        window per call, B windows per call and -- forward_multi -- n samples per call); only the gradio mode and a call without
        a carried state that is not a first frame (an error of the caller, reported by _forward_seq) take the reference order on M."""
        dev = lrs.device
        # A window whose forward branch restarts -- a reset_branch roll-over of a running stream (RefVSR.py:168-170) and, since round 6,
        # a caller's FIRST FRAME -- differs from a steady one only in its forward branch: t // 2 + 1 steps from zeros over the window's
        # first frames instead of one step from the carried state.  It stays on the three streams (`rst` in _pipe_call): no
        # drain of the calls in flight, no serial pass on M, no refill of the pipeline behind it (a first frame used to cost 11.5 ms of
        # serial launches on M at 270p; a clip's first call now overlaps like any other).
        if not bool(self.cfg.EVAL.is_gradio) and (is_first_frame or self.fw_feat is not None):
            outs, vis = self._forward_group_pipelined([(lrs, refs, frame_ids)], input_ready, want_vis, first=bool(is_first_frame))
            return outs[0], (vis[0] if vis else None)
        M0, M1, F_, P = self._pipe_streams(dev)
        M, Mo = (M0, M1) if (self._pipe_calls & 1) == 0 else (M1, M0)
        self._pipe_calls += 1
        caller = self._pipe_begin((lrs, refs), input_ready, self.pipe_depth, (M0, M1, F_, P))
        # restart of the forward branch: run the reference order on M, after everything in flight
        for st in (P, F_, Mo):
            M.wait_stream(st)
        with ops.on_stream(M):
            out, vis = self._forward_seq(lrs, refs, is_first_frame, want_vis, frame_ids)     # (a roll-over: _branch_restarts)
        for st in (F_, P, Mo):
            st.wait_stream(M)
        self._pipe_end(caller, M, [out], vis)
        return out, vis

    # ------------------------------------------------------------------ frame groups: multi-map launches (opt-in extension)
    # The backward branches of CONSECUTIVE output frames are independent chains over identical weights (each window restarts its
    # backward branch from zeros, RefVSR.py:211-238): step j of the B chains of a group of B consecutive windows runs as ONE launch
    # per layer over B maps (refvsr_*_batch, ABI 11) -- at 270 x 480 a launch is one 8 x 32 tile per workgroup, a group of four is
    # four tiles per weight fill and per launch (resblock24: 9.9 -> 7.4 us per map, profiles/r05_multimap_microbench.txt).  Only the
    # forward-branch step (which carries the state from frame to frame) stays one frame per launch.  Results are bit-identical to
    # B forward() calls (tests/test_gpu_e2e.py::test_frame_groups_are_bit_identical).
    def group_ok(self):
        """Whether B windows per call are SCHEDULED as a group.  The propagation layers take any configuration for any B (what has no
        multi-map kernel runs map by map -- same results); a group pays where its launches are multi-map: the default kernels of the
        mid_channels = 24 family (every launch of the backward branches) and of the mid_channels = 48 family (warps and fused blocks;
        its convs run map by map inside the group's schedule).  Other configurations keep one window per call."""
        return bool(((self.C == 24 and self.rb24 and self.fuse_resblocks) or (self.C == 48 and self.rb48)) and self.fuse_conf and self.warp_up2 and
                    ops.CONV24 and self.cache and self.overlap and not bool(self.cfg.EVAL.is_gradio) and
                    ops.conf_alpha_ok(self.cw('conf_fusion.1.0')) and ops.conf_alpha_ok(self.cw('conf_fusion2.1.0')))

    def _itr_after(self, k, first=False):
        """frame_itr_num as the k-th window from now will find it: the counter restarts at max_frame_itr_num and -- first -- at the next
        window, a caller's first frame (RefVSR.py:168-170,292-295).  The one place that advances the counter: a call over k windows
        leaves _itr_after(k, first) behind."""
        itr = int(self.frame_itr_num)
        for j in range(k):
            if (first and j == 0) or (self.max_frame_itr_num is not None and itr == self.max_frame_itr_num):
                itr = 0
            itr += 1
        return itr

    @torch.no_grad()
    def forward_group(self, wins, is_first_frame=False, input_ready=None, want_vis=False):
        """B consecutive windows of this stream in one call: wins = [(lrs [t,3,h,w], refs, frame_ids)] in stream order, every window
        as forward(lrs, refs, is_first, frame_ids=ids) would get it (is_first_frame applies to wins[0]).  Returns [result planar
        [3,s h,s w]] per window -- bit-identical to the B forward() calls.  Runs of >= 2 windows execute as a group (multi-map launches
        on the internal streams: needs set_pipelined(True); a reset_branch roll-over window and -- round 6 -- a caller's first frame stay
        in their group, only their forward branch is the long one); a stream without a carried state, the gradio mode and engines
        without the group schedule run one forward() each.
        input_ready: as in forward() (None | 'materialised' | event | stream), for all windows of the call.
        want_vis: returns (results, [the eval `vis` maps of every window, _conf_vis]) instead -- the maps forward(want_vis=True) gives
        for that window, bit for bit; off, the launch list is the one without it."""
        outs, vis = [None] * len(wins), [None] * len(wins)
        i = 0
        if is_first_frame:
            self.id_cache, self.flow_cache = {}, {}               # a new clip: ids of the previous one must not match (as in forward())
        grouped = self.group_ok() and self.pipelined                # (weight look-ups: once per call)
        if grouped:
            # before the first internal stream exists: an engine driven through forward_group runs P | F | M from its first call on
            # (a rebuild later would leave the first set of streams behind, and with more streams than hardware queues the
            # stream -> queue mapping decides which sections serialise); REFVSR_PIPE_LAYOUT / config.pipe_layout override it
            self._layout_default = 'pfm'
        with torch.cuda.device(wins[0][0].device):
            while i < len(wins):
                # the longest run of steady windows from i on (the iteration counter advances by one per window)
                j = i
                head = bool(i == 0 and is_first_frame)              # (round 6: a first frame is a member of its group like a roll-over)
                if grouped and (self.fw_feat is not None or head):         # (group_ok() excludes the gradio mode)
                    # (a roll-over window stays inside the group: only its forward branch is the long one, `rst` in _pipe_call)
                    while j < len(wins) and j - i < ops.hip.MAX_MAPS:
                        j += 1
                if j - i >= 2:
                    res, vs = self._forward_group_pipelined(wins[i:j], input_ready, want_vis, first=head)
                    outs[i:j] = res
                    if want_vis:
                        vis[i:j] = vs
                    i = j
                else:
                    lrs, refs, ids = wins[i]
                    outs[i], vis[i] = self.forward(lrs, refs, bool(is_first_frame) and i == 0, want_vis=want_vis, frame_ids=ids,
                                                   input_ready=input_ready)
                    i += 1
        return (outs, vis) if want_vis else outs

    def _forward_group_pipelined(self, wins, input_ready, want_vis=False, first=False):
        """B >= 1 windows of this stream on the internal streams (the group form of _pipe_call): P prepares the windows' new frames and
        flows, F walks the B forward-branch steps frame by frame, M the B backward branches -- multi-map launches for B >= 2, the
        single-map launch list for B = 1 (one forward() per frame: the first layers of its backward branch, a function of the new frame
        alone, run with the frame's preparation on P: `bw_head_blocks`) -- then the upsamplers.
        first: wins[0] is a caller's first frame (RefVSR.py:257-258,292-295): its forward branch starts from zeros like a roll-over's, the
        iteration counter restarts.  Returns (results, the windows' vis dicts -- None unless want_vis)."""
        B = len(wins)
        t, h, w = self._geometry(wins[0][0])
        for lrs, refs, _ in wins:
            assert self._geometry(lrs) == (t, h, w) and lrs.shape == wins[0][0].shape

        def f_step(frs, rst, share, timed):
            # the forward-branch steps, one frame after the other (the carried state); one hand-over event per window
            fws, evs = [], []
            for b, fr in enumerate(frs):
                self._carried_state_to(share[2], fr, rst[b])
                fw = self._forward_branch(fr, (lambda a, b_, fr=fr: self.flow(fr[a], fr[b_], share)), t, h, w, rst[b])
                for x in fw:
                    x.record_stream(share[0])
                    x.record_stream(share[1])
                e = torch.cuda.Event(enable_timing=timed)
                e.record()
                fws.append(fw)
                evs.append(e)
            return fws, evs
        # B = 1: the backward branch + upsampler of consecutive calls are independent of each other (only the forward branch carries
        # state): calls alternate between the two M streams of the wider models (mid_channels = 24: M0 is M1, see _pipe_streams).
        # Groups stay on one (two M streams alternating between groups: 210.5 vs 220.4 frames/s, profiles/r05_group_knobs_ab.txt)
        # The host may run at most pipe_depth calls ahead of the GPU (each call in flight holds its intermediates: ~0.3 GB at 270p; a
        # group holds B calls' worth).  Depth 3 since round 4: with 2 the host had ~2.4 ms of slack when it issued a call and a 6 ms
        # hiccup of the host reached the GPU as a gap (profiles/r04_stream_layout_ab.txt)
        return self._pipe_call([(self, win) for win in wins], [x for lrs, refs, _ in wins for x in (lrs, refs)], input_ready, f_step,
                               alternate_m=B == 1, depth=self.pipe_depth if B == 1 else max(1, self.pipe_depth - 1), first=first,
                               want_vis=want_vis, sev=self.stream_events)

    def _carried_state_to(self, F_, fr, restart):
        """Before a forward-branch step on F: the stream waits for the frames the step reads and owns the carried state."""
        ctr = len(fr) // 2
        for f in (fr[:ctr + 2] if restart else (fr[ctr], fr[ctr + 1])):
            if f.ready is not None:
                F_.wait_event(f.ready)
        for x in (self.fw_feat, self.fw_feat_up, self.fw_conf, self.fw_flow):
            if x is not None:                             # (None: a first frame without a previous clip)
                x.record_stream(F_)

    def _share_pipe(self, engines):
        """One set of internal streams, one queue of calls in flight and one call counter for all `engines`: this engine's."""
        for e in engines:
            if e is not self:
                e._layout_default, e._pipe, e._inflight = self._layout_default, self._pipe, self._inflight
                if self._pipe is not None:
                    e.pipe_layout, e._pipe_calls = self.pipe_layout, self._pipe_calls

    def _pipe_call(self, lanes, tensors, input_ready, f_step, alternate_m, depth, first=False, want_vis=False, sev=None):
        """The ONE implementation of the P | F | M schedule, over lanes = [(engine, window (lrs, refs, frame_ids))]: the B
        consecutive windows of one engine (a frame group; one window: a forward() call) or one window each of n engines (forward_multi).
        Stream set-up and _pipe_begin over the inputs `tensors`; P: every lane's frames, preparation (_prepare_window) and flows, engine
        by engine; F: f_step(frs, rst, share, timed) -> (per lane (feat, 2x feat, conf) of its forward-branch step, per lane the event
        behind which they are final) -- the one section in which the call forms differ; M: the lanes' backward branches step by step
        (multi-map launches for >= 2 lanes), then each lane's upsampler behind its hand-over event; counters; _pipe_end.
        alternate_m: consecutive calls alternate between the two M streams; depth: calls in flight; first: lane 0 is a caller's first
        frame; sev: bench.py's list of per-call section events.  Returns (results, the lanes' vis dicts -- None unless want_vis)."""
        engines = [e for b, (e, _) in enumerate(lanes) if all(e is not e2 for e2, _ in lanes[:b])]
        wins = [win for _, win in lanes]
        t, h, w = self._check_window(wins[0][0], wins[0][1])
        for lrs, refs, _ in wins[1:]:
            self._check_window(lrs, refs)
        ctr, dev = t // 2, wins[0][0].device
        # lanes at which the forward branch restarts (reset_branch roll-over, a caller's first frame): their backward branches are
        # chains like the others', their forward branch is the long one (from zeros over the window's first frames)
        rst = [e._branch_restarts(first and e is lanes[0][0], h, w, ahead=sum(1 for e2, _ in lanes[:b] if e2 is e)) for b, (e, _) in enumerate(lanes)]
        share = tuple(self._pipe_streams(dev))
        M0, M1, F_, P = share
        M = M0 if (not alternate_m or (self._pipe_calls & 1) == 0) else M1
        self._pipe_calls += 1
        self._share_pipe(engines)
        for e in engines:
            e._await_fw_up(e.fw_feat_up)
        caller = self._pipe_begin(tensors, input_ready, depth, share)
        mark = (lambda st: None) if sev is None else _timed_event     # bench.py: per-call (start, end) HIP events of the P / F / M sections
        tev = {'n': len(lanes)}
        # ---- P: everything that is a function of single frames / frame pairs, for all windows of the call
        with ops.on_stream(P):
            tev['P0'] = mark(P)
            n_ctx = next(_uid)
            pend, frs, held = [], [None] * len(lanes), []
            mine = [[b for b, (e2, _) in enumerate(lanes) if e2 is e] for e in engines]
            for e, bs in zip(engines, mine):                          # new frames are cloned here, on P
                for b, fr in zip(bs, e._frames_group([wins[b] for b in bs], pend)):
                    frs[b] = fr
            self._source(wins[0]).decode(pend)                        # (8-bit / 4:2:0 frames: the call's new frames in one launch)
            for e, bs in zip(engines, mine):
                for b in bs:
                    # (a group's own preparation computes no backward head: its whole first step is cheaper as multi-map launches)
                    e._prepare_window(frs[b], 0 if rst[b] else ctr, share, n_ctx, head=len(lanes) == 1)
                # the engine's new flows in batched SPyNet passes: the backward flows and the forward flow of every window (`held`:
                # kept until the end of the issue, the cache may trim them)
                held.append(e.flows([pr for b in bs for pr in _flow_pairs(frs[b], rst[b])], share))
            tev['P1'] = mark(P)
        # ---- F: the forward-branch steps (the carried state)
        with ops.on_stream(F_):
            tev['F0'] = mark(F_)
            fws, ev_fw = f_step(frs, rst, share, sev is not None)
            tev['F1'] = ev_fw[-1]
        # ---- M: the backward branches step by step (>= 2 lanes: multi-map launches), then the upsamplers
        outs, vis = [], None
        with ops.on_stream(M):
            tev['M0'] = mark(M)
            bw_ups, bw_confs = self._backward_chains(frs, lambda b, i: lanes[b][0].flow(frs[b][i], frs[b][i + 1], share), wait=True)
            for b, fr in enumerate(frs):
                if b == 0 or ev_fw[b] is not ev_fw[b - 1]:
                    M.wait_event(ev_fw[b])
                outs.append(self.compute_up(bw_ups[b], fws[b][1], bw_confs[b], fws[b][2], fr[ctr].lr))
            if want_vis:
                # (after the window's compute_up, on M: f.conf is `ready`, fws[b] was waited for above)
                vis = [self._conf_vis(fr[ctr], bw_confs[b], fws[b][2]) for b, fr in enumerate(frs)]
        del held
        for b, (e, _) in enumerate(lanes):                            # (through the roll-overs inside a group; RefVSR.py:292-295)
            e.frame_itr_num = e._itr_after(1, first and b == 0)
        done = self._pipe_end(caller, M, outs, vis, timing=sev is not None)
        if sev is not None:
            tev['M1'] = done
            sev.append(tev)
        return outs, vis

    # ------------------------------------------------------------------ n > 1: the samples of a batch as multi-map launches (round 5)
    # The n samples of a call (lrs [n,t,3,h,w], RefVSR.py:151) are n independent streams over identical weights: in steady state the
    # forward-branch step AND the backward branches of all samples run as multi-map launches (one launch per layer over n maps); only the
    # per-frame preparation stays per sample.  Same streams, events and hazards as a frame group; results equal one forward() per sample,
    # bit for bit (tests/test_gpu_e2e.py::test_batch_samples_as_multimap_launches).
    @staticmethod
    @torch.no_grad()
    def forward_multi(engines, lrs, refs, is_first_frame, frame_ids, input_ready=None):
        """engines: one Engine per sample (sharing one Weights); lrs, refs [n,t,3,h,w]; frame_ids: per-sample id lists.  Returns the n
        results.  Calls that restart a forward branch (first frame, reset_branch roll-over -- the samples' counters run in lock-step),
        more than REFVSR_MAX_MAPS samples and engines without the multi-map launch list run one forward() per sample."""
        n = len(engines)
        lead = engines[0]
        group_ok = lead.group_ok()
        if group_ok and lead.pipelined:
            for e in engines:                       # P | F | M from the first stream on, like an engine driven through forward_group
                e._layout_default = 'pfm'
        steady = (not is_first_frame and 2 <= n <= ops.hip.MAX_MAPS and group_ok and
                  all(e.pipelined and e.fw_feat is not None and e.W is lead.W and
                      (e.max_frame_itr_num is None or e.frame_itr_num != e.max_frame_itr_num) and
                      tuple(e.fw_feat.shape[:2]) == lead._geometry(lrs[0])[1:] for e in engines))
        lead._share_pipe(engines)                   # one set of internal streams for all samples: the lead's
        if not steady:
            outs = []
            for b, e in enumerate(engines):
                outs.append(e.forward(lrs[b], refs[b], bool(is_first_frame), frame_ids=frame_ids[b], input_ready=input_ready)[0])
                e._share_pipe(engines)              # (the lead may just have created the streams)
            return outs
        with torch.cuda.device(lrs.device):
            return lead._forward_multi_pipelined(engines, lrs, refs, frame_ids, input_ready)

    def _forward_multi_pipelined(self, engines, lrs, refs, frame_ids, input_ready):
        """The multi-sample form of _pipe_call: the forward-branch step of all samples as ONE multi-map _prop_step, one hand-over event."""
        ctr = lrs.shape[1] // 2

        def f_step(frs, rst, share, timed):
            for e, fr in zip(engines, frs):
                e._carried_state_to(share[2], fr, False)
            fw = self._prop_step([fr[ctr] for fr in frs], 'forward_resblocks', [e.fw_feat for e in engines],
                                 [e.fw_feat_up for e in engines], [e.fw_conf for e in engines], [e.fw_flow for e in engines])
            for b, (e, fr) in enumerate(zip(engines, frs)):                               # RefVSR.py:279-283
                e.fw_feat, e.fw_feat_up, e.fw_conf = fw[0][b], fw[1][b], fw[2][b]
                e.fw_flow = e.flow(fr[ctr + 1], fr[ctr], share)
            for x in list(fw[1]) + list(fw[2]):
                x.record_stream(share[0])
                x.record_stream(share[1])
            ev = torch.cuda.Event()
            ev.record()
            return list(zip(*fw)), [ev] * len(frs)
        return self._pipe_call([(e, (lrs[b], refs[b], frame_ids[b])) for b, e in enumerate(engines)], (lrs, refs), input_ready, f_step,
                               alternate_m=False, depth=self.pipe_depth)[0]

    def _side_stream(self, dev):
        """The one side stream of the sequential path (the forward-branch step under the new frame's preparation)."""
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        return self._side

    def _prop_step(self, fs, branch, feats, feat_ups, confs, fls, up_from_lr=False):
        """One propagation step (RefVSR.py:216-230 backward, :251-277 forward) of B >= 1 independent chains (lists of B frames / maps /
        flows in, lists out): warp the carried maps with `fls` (None: first step of a branch, nothing to warp),
        ResidualBlocksWithInputConv, AA_AF_conf_prop.  up_from_lr: the 2x state is warp(warp(feat, fl), flow_up2(fl)) -- the
        reference's :254 quirk (feat_ups is not read)."""
        lr8s = [f.lr8 for f in fs]
        if fls is None:
            # (frames that a one-frame-per-call window prepared carry the head of this step -- input conv + bw_head_blocks blocks, run
            #  with their preparation: used when every frame has one, of the same length; a group's own preparation computes none:
            #  the whole first step is cheaper as multi-map launches here)
            heads = [f.bw_head for f in fs] if branch == 'backward_resblocks' else [None]
            if all(hd is not None and hd[0] == heads[0][0] for hd in heads):
                xs = self.resblocks_b(None, None, branch, resume=(heads[0][0], [hd[1] for hd in heads]))
            else:
                xs = self.resblocks_b(lr8s, feats, branch)
            return self.rap_b(fs, confs, xs, feat_ups)
        confs = list(ops.warp_planar_b(confs, fls, stack=False))
        feats = list(ops.warp_nhwc16_b(feats, fls, stack=False))
        xs = self.resblocks_b(lr8s, feats, branch)
        if up_from_lr:
            feat_ups = feats                              # the reference's :254 quirk: the ALREADY WARPED LR state, on the 2x grid
        else:
            for u in feat_ups:
                self._await_fw_up(u)                      # (split hand-off: the 2x state may still be arriving -- first read here)
        # the 2x state is warped by flow_up2(fl): evaluated inside the warp kernel (no 2x flow map) unless REFVSR_NO_WARP_UP2=1
        if self.warp_up2:
            feat_ups = ops.warp_nhwc16_up2_b(feat_ups, fls, stack=False)
        else:
            feat_ups = ops.warp_nhwc16_b(feat_ups, [ops.flow_up2(fl) for fl in fls], stack=False)
        return self.rap_b(fs, confs, xs, list(feat_ups))

    def _backward_chains(self, frs, flow, wait=False):
        """Backward propagation branches (RefVSR.py:211-238) of B >= 1 windows: each restarts from zeros and walks from its last
        frame down to the centre, step by step over all B chains (_prop_step: one multi-map launch per layer for B >= 2, the
        single-map launches for B = 1).  flow(b, i): window b's flow from frame i to i + 1 (backward_flows[:, i] = FlowNet(lrs[i],
        lrs[i+1])).  wait: the frames were prepared on another stream, each step first waits for its frames' `ready`.  Returns the
        B 2x maps and the B confidence maps, on the current stream."""
        B, t = len(frs), len(frs[0])
        ctr, dev, cs_ = t // 2, frs[0][0].lr.device, self._state_cs()
        h, w = frs[0][0].lr.shape[1:]
        feats = [self._zeros((h, w, cs_), torch.float16, dev)] * B
        feat_ups = [self._zeros((2 * h, 2 * w, cs_), torch.float16, dev)] * B
        confs = [self._zeros((1, h, w), torch.float32, dev)] * B
        for i in range(t - 1, ctr - 1, -1):
            fs = [fr[i] for fr in frs]
            if wait:
                for f in fs:
                    if f.ready is not None:
                        torch.cuda.current_stream().wait_event(f.ready)
            fls = None if i == t - 1 else [flow(b, i) for b in range(B)]
            feats, feat_ups, confs = self._prop_step(fs, 'backward_resblocks', feats, feat_ups, confs, fls)
        return feat_ups, confs

    def _forward_branch(self, fr, flow, t, h, w, is_first_frame):
        """Forward propagation branch (RefVSR.py:240-283); updates the carried state.  Runs on the current stream."""
        ctr, dev, cs_ = t // 2, fr[0].lr.device, self._state_cs()
        if is_first_frame:
            feat = self._zeros((h, w, cs_), torch.float16, dev)
            feat_up = self._zeros((2 * h, 2 * w, cs_), torch.float16, dev)
            conf = self._zeros((1, h, w), torch.float32, dev)
            range_start = 0
        else:
            range_start = ctr

        def step(f, feat, feat_up, conf, fl, **kw):               # one chain through the list form
            return [m[0] for m in self._prop_step([f], 'forward_resblocks', [feat], [feat_up], [conf], None if fl is None else [fl], **kw)]
        for i in range(range_start, ctr + 1):
            if i > range_start:
                # forward_flows[:, i-1] = FlowNet(lrs[i], lrs[i-1]); :253-255 warps the ALREADY WARPED LR state onto the 2x grid
                feat, feat_up, conf = step(fr[i], feat, None, conf, flow(i, i - 1), up_from_lr=True)
            elif not is_first_frame:                                                # :257-260
                feat, feat_up, conf = step(fr[i], self.fw_feat, self.fw_feat_up, self.fw_conf, self.fw_flow)
            else:
                feat, feat_up, conf = step(fr[i], feat, feat_up, conf, None)
            if i == ctr:                                                            # :279-283
                self.fw_feat, self.fw_feat_up, self.fw_conf = feat, feat_up, conf
                self.fw_flow = flow(ctr + 1, ctr)         # forward_flows[:, ctr]
        return feat, feat_up, conf

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, lrs, refs, is_first_frame, want_vis=False, frame_ids=None, want_log=False, input_ready=None):
        """lrs, refs: cuda float32 [t,3,h,w] in [0,1], or uint8 [t,3,h,w] (value = byte / 255; contiguous or the channels-last view of
        [t,h,w,3] bytes); under config.input_yuv: [t, 3h/2, w] Y'CbCr 4:2:0 frames of that format (uint8 | uint16), dense and
        contiguous.  Returns (result planar [3,4h,4w], vis dict or None).
        frame_ids (optional): one hashable id per window frame -> the window cache is keyed by id instead of by
        content comparison; together with set_pipelined(True) it enables cross-call stream pipelining."""
        if is_first_frame and frame_ids is not None:
            # the caller starts a new clip: ids of the previous clip must not match (the internal reset_branch restart
            # of a running clip keeps the cache -- same clip, same ids)
            self.id_cache, self.flow_cache = {}, {}
        self._await_fw_up(self.fw_feat_up)           # (a state imported in two messages whose second part nobody has read yet)
        with torch.cuda.device(lrs.device):          # launches go to the tensors' device, whatever the current device is
            if self.takes_pipelined_path(frame_ids, want_log):
                return self._forward_pipelined(lrs, refs, is_first_frame, want_vis, frame_ids, input_ready)
            self._await_inputs(input_ready)
            with ops.on_stream(torch.cuda.current_stream()):
                return self._forward_seq(lrs, refs, is_first_frame, want_vis, frame_ids, want_log)

    def takes_pipelined_path(self, frame_ids, want_log=False):
        """True when forward() with these arguments runs on the internal streams (the only path that reads the inputs off the
        caller's stream order)."""
        return bool(self.pipelined and frame_ids is not None and self.cache and self.overlap and not want_log)

    # ------------------------------------------------------------------ two-phase forward (multi-GPU wavefront)
    def _check_window(self, lrs, refs):
        inputs.check_window(lrs, refs, self.input_yuv and self.input_yuv[0], 4, 'Engine', 't')
        if self.input_yuv is None:                               # (the engine converts nothing)
            assert lrs.is_cuda and lrs.dim() == 4 and lrs.shape == refs.shape
            if lrs.dtype != refs.dtype or lrs.dtype not in (torch.float32, torch.uint8):
                raise RuntimeError('lrs and refs must both be float32 or both uint8 (got %s, %s)' % (lrs.dtype, refs.dtype))
            if None in (self._source((lrs, refs)).key or ()):
                raise RuntimeError('uint8 windows must be contiguous [t,3,h,w] or the channels-last view of [t,h,w,3] bytes')
        t, h, w = self._geometry(lrs)
        assert t >= 3 and t % 2 == 1 and h % 2 == 0 and w % 2 == 0, 'need odd t >= 3 and even h, w'
        assert not self.hd or (h % 8 == 0 and w % 8 == 0), 'flag_HD_in needs h, w divisible by 8'
        assert not self.vgg7 or (h % 4 == 0 and w % 4 == 0), 'x2 / HD matching needs h, w divisible by 4'
        return t, h, w

    @torch.no_grad()
    def phase_a(self, lrs, refs, frame_ids=None, first_hint=False):
        """Everything of one forward() that does NOT depend on the carried forward-branch state: frame preparation
        (flows, matching, reference encoders, alignment -- cached across windows as usual) and the whole backward
        branch (RefVSR.py:182-238), i.e. 85-90 % of the work.  Returns a handle for phase_b.  Used by
        shard.run_wavefront: every rank runs phase A of all its frames concurrently, then the ranks run phase B one
        after the other along the state hand-off chain.  first_hint: the call is expected to be a first frame / reset
        frame, prepare frames 0..ctr-1 now instead of lazily in phase B."""
        return self._phase_a([(lrs, refs, frame_ids)], [bool(first_hint)])[0]

    @torch.no_grad()
    def phase_a_group(self, wins, first_hints=None, streams=None):
        """phase_a of B <= REFVSR_MAX_MAPS windows of one clip in ONE pass (round 6): wins = [(lrs [t,3,h,w], refs, frame_ids)] -- any
        windows of the clip, consecutive or not (a rank's frames of a block-cyclic partition are not): their backward branches are B
        independent chains over identical weights (RefVSR.py:211-238 restarts from zeros in every window) and run as multi-map launches
        (_prop_step: one launch per layer over B maps, the launch list of a frame group's M section), every flow the B windows ask for
        comes out of batched SPyNet passes.  Returns the B handles phase_a would return, bit for bit
        (tests/test_gpu_e2e.py::test_phase_a_group_equals_phase_a); engines without the multi-map launch list run window by window.
        streams=None: everything on the current stream, like phase_a.
        streams=(M, consumers): the stream layout of a frame group for the sharded executor -- the per-frame preparation and
        the flows on the CURRENT stream (the executor's lane a = P), the backward chains on M behind per-frame / per-flow events, so that
        the next group's preparation runs under this group's chains; every handle carries `ready`, an event on M after which all of
        the handle is final; `consumers`: the other streams that will read the contexts and flows (the B1 lane), for the allocator."""
        B = len(wins)
        hints = [False] * B if first_hints is None else [bool(v) for v in first_hints]
        if B > ops.hip.MAX_MAPS or not self.group_ok() or (B == 1 and streams is None):
            return [self._phase_a([win], [hints[b]])[0] for b, win in enumerate(wins)]
        return self._phase_a(wins, hints, streams, grouped=True)

    def _phase_a(self, wins, hints, streams=None, grouped=False):
        """The one body of phase A, for B >= 1 windows: frames -> flows -> preparation -> backward chains -> the pinned forward flows ->
        handles.  Takes the gradio mode (zero flows), a window without frame ids (B = 1: frames recognised by content) and engines
        without the group schedule (B = 1).  grouped: phase_a_group's schedule -- the preparation BEFORE the flows (one batched SPyNet
        pass over every flow the B windows ask for) and the chains in a stream section of their own, on streams[0] when `streams` is
        given (then the preparation is _prepare_window's, published for those streams); else phase_a's: flows first, one section."""
        t, h, w = self._check_window(wins[0][0], wins[0][1])
        for lrs, refs, ids in wins if grouped else ():
            assert self._check_window(lrs, refs) == (t, h, w) and ids is not None, 'a group needs windows of one geometry, named by frame ids'
        ctr, dev = t // 2, wins[0][0].device
        P = torch.cuda.current_stream(dev)
        M, share = P, None
        if streams is not None:
            M = streams[0]
            share = [P, M] + [st for st in streams[1] if st is not P and st is not M]
        gradio = bool(self.cfg.EVAL.is_gradio)
        zero_flow = fl_all = done_p = None

        def flow(fr, a, b):
            return zero_flow if gradio else self.flow(fr[a], fr[b], share)

        def chains():
            ready = None
            if share is not None:
                M.wait_event(done_p)                               # (everything this group reads was produced on P before this point)
                for fl in fl_all:
                    fl.record_stream(M)
            bw_ups, bw_confs = self._backward_chains(frs, lambda b, i: flow(frs[b], i, i + 1))
            if share is not None:
                ready = torch.cuda.Event()
                ready.record()
            out = []
            for b, fr in enumerate(frs):
                # the flows the forward branch will ask for, computed here (parallel phase) and pinned in the handle: the
                # flow cache only keeps pairs of the current window
                flows = {(ctr + 1, ctr): flow(fr, ctr + 1, ctr)}
                if hints[b]:
                    for i in range(1, ctr + 1):
                        flows[(i, i - 1)] = flow(fr, i, i - 1)
                out.append(dict(fr=fr, flows=flows, zero_flow=zero_flow, bw_up=bw_ups[b], conf_bw=bw_confs[b], t=t, h=h, w=w, ready=ready,
                                bw_flows=fl_all if share is not None else None))     # (alive until the executor's final synchronisation)
            return out
        with torch.cuda.device(dev), ops.on_stream(P):
            if gradio:
                zero_flow = torch.zeros((2, h, w), dtype=torch.float32, device=dev)
            frs = self._frames_group(wins)
            need = [pr for b, fr in enumerate(frs) for pr in _flow_pairs(fr, hints[b])]
            if not grouped and not gradio:
                self.flows(need)
            for b, fr in enumerate(frs):
                if share is not None:
                    # (also contexts prepared / imported ahead on this stream: safe on the other streams from here on)
                    self._prepare_window(fr, 0 if hints[b] else ctr, share, pyramid_first=False, ready_if_prepared=True)
                else:
                    for i in range(0 if hints[b] else ctr, t):
                        self.prepare_frame(fr[i])
            if not grouped:
                return chains()
            fl_all = self.flows(need, share)
            if share is not None:
                for fr in frs:                                     # frames a window merely contains: their copies are read by nobody else
                    for f in fr:
                        for x in (f.lr, f.ref):
                            for st in share:
                                x.record_stream(st)
                done_p = torch.cuda.Event()
                done_p.record()
        with torch.cuda.device(dev), ops.on_stream(M):
            return chains()

    @torch.no_grad()
    def phase_b1(self, pa, is_first_frame):
        """The state-dependent SERIAL part of forward(): the forward-branch step (RefVSR.py:240-283) and the iteration
        counter (:292-295).  Must be called in frame order; leaves the step's outputs in the handle for phase_b2.  The
        multi-GPU wavefront runs B1 of all local frames, hands the state over, and only then runs the upsamplers (B2), so
        that the serial chain over the ranks carries nothing but the forward-branch steps."""
        fr = pa['fr']
        restart = self._branch_restarts(is_first_frame, pa['h'], pa['w'])
        with ops.on_stream(torch.cuda.current_stream()):
            def flow(a, b):
                if pa['zero_flow'] is not None:
                    return pa['zero_flow']
                hit = pa['flows'].get((a, b))
                return hit if hit is not None else self.flow(fr[a], fr[b])
            if restart:
                for i in range(0, pa['t'] // 2):
                    self.prepare_frame(fr[i])                  # no-op when phase A had the hint
            self._b1(pa, flow, restart)
        return pa

    def _b1(self, pa, flow, restart):
        """The forward-branch step of a handle on the current stream and the iteration counter (RefVSR.py:240-283,292-295); leaves the
        step's outputs in the handle and returns them."""
        fw = self._forward_branch(pa['fr'], flow, pa['t'], pa['h'], pa['w'], restart)
        self.frame_itr_num = self._itr_after(1, restart)
        pa['fw_up'], pa['conf_fw'] = fw[1:]
        return fw

    def _b2(self, pa, want_vis):
        """BW/FW fusion + upsampler (RefVSR.py:288-297) of a handle on the current stream, and the eval `vis` maps when asked for."""
        f = pa['fr'][pa['t'] // 2]
        out = self.compute_up(pa['bw_up'], pa['fw_up'], pa['conf_bw'], pa['conf_fw'], f.lr)
        return out, (self._conf_vis(f, pa['conf_bw'], pa['conf_fw']) if want_vis else None)

    @torch.no_grad()
    def phase_b2(self, pa, want_vis=False):
        """BW/FW fusion + upsampler (RefVSR.py:288-297) of a frame whose phase_b1 has run: independent of the carried state
        and of the other frames."""
        with ops.on_stream(torch.cuda.current_stream()):
            return self._b2(pa, want_vis)

    @torch.no_grad()
    def phase_b(self, pa, is_first_frame, want_vis=False, after_state=None):
        """The state-dependent rest of forward() = phase_b1 + phase_b2; (phase_a, phase_b) of a frame == forward() of that
        frame.  after_state: callable invoked once the carried state of this frame is final (before the upsampler is
        enqueued)."""
        self.phase_b1(pa, is_first_frame)
        if after_state is not None:
            after_state()
        return self.phase_b2(pa, want_vis)

    def _branch_restarts(self, is_first_frame, h, w, ahead=0):
        """Whether the window `ahead` windows from now restarts the forward branch: the next window when it is a caller's first frame
        (is_first_frame), any window at a reset_branch roll-over (RefVSR.py:168-170).  A next window that does not restart must find a
        carried state of its frame size."""
        is_first_frame = bool(is_first_frame and ahead == 0) or (self.max_frame_itr_num is not None and
                                                                 self._itr_after(ahead, is_first_frame) == self.max_frame_itr_num)
        if ahead > 0:
            return is_first_frame
        if not is_first_frame and self.fw_feat is None:
            raise RuntimeError('is_first_frame=False but no forward state is held (first call of a stream '
                               'must pass is_first_frame=True, cf. RefVSR.py:257-258)')
        if not is_first_frame and tuple(self.fw_feat.shape[:2]) != (h, w):
            raise RuntimeError('frame size changed from %s to %s without is_first_frame=True'
                               % (tuple(self.fw_feat.shape[:2]), (h, w)))
        return is_first_frame

    @staticmethod
    def _conf_vis(f, conf_bw, conf_fw):
        """The eval `vis` maps of centre frame f (RefVSR.py:318-322)."""
        vis = collections.OrderedDict()
        vis['conf_map'] = f.conf
        vis['conf_map_prop'] = ops.max2(conf_bw, conf_fw)
        vis['conf_map_prop_backward'] = conf_bw
        vis['conf_map_prop_forward'] = conf_fw
        return vis

    def _sample_vis(self, f, conf_bw, conf_fw):
        """The save_sample block of the `vis` samples (RefVSR.py:301-316; identical in RefVSR_IR.py:367-384) for centre frame f."""
        vis = collections.OrderedDict()
        h, w = f.lr.shape[1:]
        hm, wm = (h // (self.cfg.scale // 2), w // (self.cfg.scale // 2)) if self.hd else (h, w)
        gh, gw = (hm // 2, wm // 2) if self.vgg7 else (hm, wm)
        s1, s2 = self.ks // 2, self.ks
        lr_down = ops.bicubic_scale(f.lr, 0.5, clamp01=True)
        ref_down = ops.bicubic_scale(f.ref, 0.5, clamp01=True)
        vis['FW_aa1_fm_ref_aligned'] = ops.block_gather_rgb(ref_down, f.idx, gh, gw, s1, planar=True)
        if s1 > 1:
            fm8 = ops.block_gather_rgb(ref_down, f.idx, gh, gw, s1)
            rgb8 = ops.block_gather_rgb(f.ref, f.idx, gh, gw, s1)
            vis['FW_aa1_ref_aligned'] = ops.unpack_nhwc16(self.aligned_conv(fm8, lr_down, rgb8, 'aa1.align', s1), 3)
        vis['FW_aa2_fm_ref_aligned'] = ops.block_gather_rgb(f.ref, f.idx, gh, gw, s2, planar=True)
        rgb8 = ops.block_gather_rgb(f.ref, f.idx, gh, gw, s2)
        vis['FW_aa2_ref_aligned'] = ops.unpack_nhwc16(self.aligned_conv(rgb8, f.lr, rgb8, 'aa2.align', s2), 3)

        def norm(x):
            x = x - x.min()
            return x / x.max()
        vis['conf_map_norm'] = norm(f.conf)
        vis['conf_map_prop_backward_norm'] = norm(conf_bw)
        vis['conf_map_prop_forward_norm'] = norm(conf_fw)
        vis['conf_map_prop_norm'] = norm(ops.max2(conf_bw, conf_fw))
        return vis

    def _debug_vis(self, fr, t, is_first_frame, range_start, fw_flow_in, flow, conf_bw, conf_fw, save_sample):
        """The `vis` debugging samples of Network.forward (RefVSR.py:219-221,262-263,301-316), is_log only; planar fp32
        [C,H,W] maps.  (The min/max normalisation of the four confidence maps, models/utils.py:23-32, uses torch
        reductions: debug output, not the hot path.)"""
        ctr = t // 2
        vis = collections.OrderedDict()
        if ctr < t - 1:
            vis['BW_LR_next_warp'] = ops.warp_planar(fr[ctr + 1].lr, flow(ctr, ctr + 1))
        fl = flow(ctr, ctr - 1) if ctr > range_start else (None if is_first_frame else fw_flow_in)
        if fl is not None:
            vis['FW_LR_prev_warp'] = ops.warp_planar(fr[ctr - 1].lr, fl)
        if save_sample:
            vis.update(self._sample_vis(fr[ctr], conf_bw, conf_fw))
        return vis

    def _forward_seq(self, lrs, refs, is_first_frame, want_vis=False, frame_ids=None, want_log=False):
        t, h, w = self._check_window(lrs, refs)
        ctr = t // 2
        dev = lrs.device
        is_first_frame = self._branch_restarts(is_first_frame, h, w)
        gradio = bool(self.cfg.EVAL.is_gradio)
        zero_flow = torch.zeros((2, h, w), dtype=torch.float32, device=dev) if gradio else None
        fr = self._frames(lrs, refs, frame_ids)
        range_start = 0 if is_first_frame else ctr                                  # :173-176
        # Two-stream overlap (steady state): the forward-branch step depends only on cached per-frame data and
        # the carried state, not on this window's new frame, so it runs on a side stream while the main stream
        # prepares the new frame (matching, encoders, alignment) and walks the backward branch.
        main = torch.cuda.current_stream()
        overlap = (self.overlap and not is_first_frame and fr[ctr].conf is not None)
        # with two streams every flow carries an event and is recorded on both: at a clip end the window repeats its
        # last frame, the two branches then ask for the SAME pair (fr[ctr], fr[ctr+1]) and the second one takes the
        # first one's tensor out of the cache -- from the other stream
        share = (main, self._side_stream(dev)) if overlap else None
        flow = (lambda a, b: zero_flow) if gradio else (lambda a, b: self.flow(fr[a], fr[b], share))   # :183-191
        fw_flow_in = self.fw_flow
        if not gradio and t > 1:
            # every flow this call consumes, in one batched SPyNet pass before the streams fork (cached pairs cost nothing)
            self.flows(_flow_pairs(fr, is_first_frame), share)
        pa = dict(fr=fr, t=t, h=h, w=w)                    # the call as phase A + B1 + B2 on one handle
        if overlap:
            for i in range(ctr, t):
                self.pyramid(fr[i])                        # shared by both streams: build on main before the fork
            side = self._side_stream(dev)
            side.wait_stream(main)
            with ops.on_stream(side):
                for x in (self.fw_feat, self.fw_feat_up, self.fw_conf, self.fw_flow):
                    x.record_stream(side)
                fw = self._b1(pa, flow, False)
        for i in range(range_start, t):                                             # :196-204 (+ per-frame RAP parts)
            self.prepare_frame(fr[i])
        [pa['bw_up']], [pa['conf_bw']] = self._backward_chains([fr], lambda b, i: flow(i, i + 1))
        if overlap:
            main.wait_stream(side)
            for x in fw:
                x.record_stream(main)
        else:
            self._b1(pa, flow, is_first_frame)                                      # :240-283,292-295
        out, vis = self._b2(pa, want_vis)                                           # :288-289,297
        if want_log:
            dbg = self._debug_vis(fr, t, is_first_frame, range_start, fw_flow_in, flow, pa['conf_bw'], pa['conf_fw'], want_vis)
            return out, (vis, dbg)
        return out, vis
