"""Config system for the RefVSR inference path (model fields + eval flags only).

Mirrors the *surface* of the reference config builders so that `run.py`/`eval.py`
style callers keep working:

  * global defaults           <- /root/reference/configs/config.py:8-118  (get_config)
  * per-model overrides       <- /root/reference/configs/config_RefVSR_{small_L1,small_MFID,L1,
                                 MFID,MFID_8K,small_MFID_8K}.py (model fields: scale, flag_HD_in,
                                 matching_ksize, num_blocks, mid_channels, reset_branch, frame_num,
                                 is_amp, network)
  * RealMCVSR folder layout   <- /root/reference/configs/config.py:120-152 (set_data_path)

Training-only fields (losses, LR schedules, log dirs) are intentionally not reproduced:
the tier scope is the inference hot path.
"""
import os


class AttrDict(dict):
    """Attribute-access dict (stand-in for easydict.EasyDict used by the reference)."""

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v

    def __setitem__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, AttrDict):
            v = AttrDict(v)
        super().__setitem__(k, v)

    __setattr__ = __setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


# model-specific fields; values transcribed from the per-model config files cited above.
_MODELS = {
    #                         C   blocks  HD     frame_itr  frame_num  reset      amp
    'config_RefVSR_small_L1':      dict(mid_channels=24, num_blocks=24, flag_HD_in=False, frame_itr_num=26, frame_num=13, reset='itr', is_amp=True),
    'config_RefVSR_small_MFID':    dict(mid_channels=24, num_blocks=24, flag_HD_in=False, frame_itr_num=9, frame_num=7, reset='itr', is_amp=True),
    'config_RefVSR_L1':            dict(mid_channels=48, num_blocks=30, flag_HD_in=False, frame_itr_num=26, frame_num=13, reset='itr', is_amp=False),
    'config_RefVSR_MFID':          dict(mid_channels=48, num_blocks=30, flag_HD_in=False, frame_itr_num=9, frame_num=7, reset='itr', is_amp=False),
    'config_RefVSR_MFID_8K':       dict(mid_channels=48, num_blocks=30, flag_HD_in=True, frame_itr_num=9, frame_num=7, reset=None, is_amp=False),
    'config_RefVSR_small_MFID_8K': dict(mid_channels=24, num_blocks=24, flag_HD_in=True, frame_itr_num=9, frame_num=3, reset='itr', is_amp=True),
    # RefVSR_IR (IconVSR-style: information refill from an EDVR-M feature extractor, configs/config_RefVSR_IR_{L1,MFID}.py)
    'config_RefVSR_IR_L1':         dict(mid_channels=36, num_blocks=30, flag_HD_in=False, frame_itr_num=26, frame_num=13, reset='itr', is_amp=False,
                                        network='RefVSR_IR', keyframe_stride=5),
    'config_RefVSR_IR_MFID':       dict(mid_channels=36, num_blocks=30, flag_HD_in=False, frame_itr_num=5, frame_num=9, reset='itr', is_amp=False,
                                        network='RefVSR_IR', keyframe_stride=5),
}

CONFIG_NAMES = tuple(_MODELS)


def base_config(project='', mode='', config_='', data='', LRS='', batch_size=8):
    """Global defaults (reference configs/config.py:8-118), inference-relevant subset."""
    c = AttrDict()
    c.project, c.mode, c.config = project, mode, config_
    c.is_train = False
    c.thread_num = batch_size
    c.cuda = True
    c.dist = False
    c.manual_seed = 0
    c.is_verbose = False
    c.save_sample = False
    c.is_amp = False
    c.device = 'cuda'
    c.trainer = ''
    c.network = ''
    c.batch_size = batch_size
    c.batch_size_test = 1
    c.data = 'RealMCVSR'
    c.data_offset = '/data1/junyonglee'
    c.LRS = LRS
    c.wi = None
    c.win = None
    c.EVAL = AttrDict(eval_mode='quan_qual', is_qual=False, is_quan=True, is_debug=True,
                      is_gradio=False, is_replicate=False, data='RealMCVSR', test_set='test',
                      load_ckpt_by_score=True, ckpt_name=None, ckpt_epoch=None,
                      ckpt_abs_name=None, low_res=False, ckpt_load_path=None,
                      HR_data_path=None, LR_data_path=None)
    c.output_offset = os.path.join('.', 'result')
    # build-specific knobs (not in the reference)
    c.cache_windows = True      # de-duplicate flows/matching/ref encodings across sliding windows
    c.compute_dtype = 'f16'     # storage/MFMA operand type of feature maps on the GPU
    c.overlap_streams = True    # forward-branch step on a side HIP stream, concurrent with the new frame's preparation
    c.fuse_resblocks = True     # conv-act-conv+residual pairs in one launch where the LDS budget allows
    c.result_dtype = 'float32'  # 'float16' | 'uint8': the output head stores rint(255 v) itself (extension; host consumers quantise anyway)
    c.result_layout = 'chw'     # 'hwc': the result is the [.., 3, sh, sw] view of dense [.., sh, sw, 3] memory (extension; what image writers consume)
    c.result_yuv = None         # 'nv12' | 'i420' | 'p010' | 'i420p10': the calls also return 'yuv', the results as Y'CbCr 4:2:0 frames (extension; what video consumers take)
    c.yuv_matrix = 'bt709'      # 'bt601': luma coefficients of 'yuv'
    c.yuv_range = 'limited'     # 'full': code range of 'yuv'
    c.yuv_siting = 'centre'     # 'left': chroma of 'yuv' on the even luma columns (MPEG-2 siting); result_yuv also takes 'i422' | 'i444' | 'i422p10' | 'i444p10' ([.., 2h, w] / [.., 3h, w] frames)
    c.input_yuv = None          # 'nv12' | 'i420' | 'p010' | 'i420p10': the windows are Y'CbCr 4:2:0 frames [.., t, 3h/2, w], decoded on the device (extension; what video decoders deliver)
    c.input_yuv_matrix = 'bt709'    # 'bt601': luma coefficients of the input frames
    c.input_yuv_range = 'limited'   # 'full': code range of the input frames
    c.input_yuv_chroma = 'bilinear' # 'nearest': chroma up-sampling of the input frames (bilinear: centre-sited, the inverse siting of 'yuv')
    c.input_yuv_siting = 'centre'   # 'left': the input frames' chroma lies on the even luma columns -- every NV12 / P010 buffer of a hardware decoder; input_yuv also takes 'i422' | 'i444' | 'i422p10' | 'i444p10'
    c.weight_precision = 'hi_lo'  # 'fp16' | 'amp': plain fp16 conv weights, the reference's AMP arithmetic (resolve_weight_precision)
    c.weight_check = 'auto'     # 'sync' | 'off': when the packed weights are checked against the parameters' device fingerprint (fingerprint.weight_check_policy)
    return c


def get_config(project='', mode='', config='', data='', LRS='', batch_size=8):
    """Same signature as the per-model `get_config` of the reference
    (configs/config_RefVSR_small_L1.py:8)."""
    if config not in _MODELS:
        raise KeyError('unknown RefVSR config %r (known: %s)' % (config, ', '.join(_MODELS)))
    m = _MODELS[config]
    c = base_config(project, mode, config, data, LRS, batch_size)
    c.is_amp = m['is_amp']
    c.frame_itr_num = m['frame_itr_num']
    c.frame_num = m['frame_num']
    c.flag_HD_in = m['flag_HD_in']
    c.scale = 4
    c.matching_ksize = 4 if c.scale == 2 else 2          # must be even
    c.refine_val_lr = 1
    c.refine_val_hr = 1
    if c.flag_HD_in:
        c.matching_ksize *= c.scale
    c.trainer = 'trainer'
    c.network = m.get('network', 'RefVSR')
    if 'keyframe_stride' in m:
        c.keyframe_stride = m['keyframe_stride']
    c.num_blocks = m['num_blocks']
    c.mid_channels = m['mid_channels']
    c.reset_branch = c.frame_itr_num if m['reset'] == 'itr' else None
    return c


WEIGHT_PRECISIONS = ('hi_lo', 'fp16', 'amp')


def resolve_weight_precision(c):
    """config.weight_precision -> 'hi_lo' | 'fp16' (extension).
      'hi_lo' (default): every fp16-operand conv carries hi + lo weights (~22 bits).
      'fp16' : plain fp16 conv weights -- what the reference computes under fp16 autocast (is_amp, trainers/trainer.py:237-239);
               the engine's output equals, bit for bit, the default engine's output on round16(sd) (weights.round16).
      'amp'  : 'fp16' when config.is_amp, else 'hi_lo'.
    A resolved 'fp16' exists for the mid_channels = 24 family only (RefVSR_small*); ValueError elsewhere.  Read once, when the
    engine's weights are packed: torch.autocast does not switch it."""
    mode = c.get('weight_precision') or 'hi_lo'
    if mode not in WEIGHT_PRECISIONS:
        raise ValueError('weight_precision must be one of %s, got %r' % (', '.join(WEIGHT_PRECISIONS), mode))
    if mode == 'amp':
        mode = 'fp16' if c.get('is_amp') else 'hi_lo'
    if mode == 'fp16' and (c.get('mid_channels') != 24 or c.get('network') == 'RefVSR_IR'):
        raise ValueError("weight_precision 'fp16' is supported for the mid_channels = 24 RefVSR models only "
                         "(config %r: network %r, mid_channels %r)" % (c.get('config'), c.get('network'), c.get('mid_channels')))
    return mode


def set_scale(c, scale):
    """The reference's config files hard-code `config.scale = 4 # SR scale (2 | 4)` and derive the matching patch size
    from it (configs/config_RefVSR_small_L1.py:30-39); x2 is selected by editing that line.  This does the same edit on a
    built config: scale, matching_ksize (4 for x2, 2 for x4; times scale with flag_HD_in)."""
    assert scale in (2, 4)
    c.scale = scale
    c.matching_ksize = 4 if scale == 2 else 2
    if c.flag_HD_in:
        c.matching_ksize *= scale
    return c


def set_data_path(config, data, is_train=False):
    """RealMCVSR folder layout for evaluation (reference configs/config.py:120-152)."""
    if data != 'RealMCVSR':
        return config
    if not config.flag_HD_in:
        lr_path = 'LRx2' if config.scale == 2 else 'LRx4'
        ref_w, ref_t = 'LRx2', 'LRx4'
    else:
        lr_path = ref_w = ref_t = 'HR'
    root = os.path.join(config.data_offset, data, config.EVAL.test_set)
    config.EVAL.LR_data_path = os.path.join(root, lr_path)
    config.EVAL.HR_data_path = os.path.join(root, 'HR')
    config.EVAL.HR_ref_data_W_path = os.path.join(root, ref_w)
    config.EVAL.HR_ref_data_T_path = os.path.join(root, ref_t)
    if 'vid_name' not in config.EVAL:       # the reference resets it here (configs/config.py:146), which defeats --vid_name
        config.EVAL.vid_name = None
    config.UW_path, config.W_path, config.T_path = 'UW', 'W', 'T'
    return config
