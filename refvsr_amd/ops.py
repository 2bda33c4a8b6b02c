"""Tensor-level wrappers over the C-ABI (refvsr_amd/hip.py).  torch is used only for device memory
(caching allocator) and the current HIP stream; every computation is a kernel of librefvsr_hip.so.

Layouts: `planar` = float32 [C,H,W];  `nhwc16` = float16 [H,W,Cs] (Cs % 8 == 0).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import fingerprint, hip, yuv
from .knobs import env_flag
from .packing import BlobFlags, blob_plan, pack_conv24, pack_conv_shuffle2, pack_resblock
from .hip import (OUT_NHWC16, OUT_NHWC16_SHUFFLE2, OUT_PLANAR32, RS_BICUBIC, RS_BILINEAR,  # noqa: F401
                  RS_BILINEAR_AC, RS_NEAREST)


_STREAM = None        # cached hipStream_t of the stream selected with on_stream(); None -> ask torch every time


def _stream():
    if _STREAM is not None:
        return _STREAM
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class on_stream(object):
    """`with ops.on_stream(s):` == `with torch.cuda.stream(s):` + caches the raw stream handle for the kernel
    launches inside (torch.cuda.current_stream() costs ~8 us of host time per call, x ~350 launches per frame)."""

    def __init__(self, stream):
        self.stream = stream
        self.ctx = torch.cuda.stream(stream)

    def __enter__(self):
        global _STREAM
        self.prev = _STREAM
        self.ctx.__enter__()
        _STREAM = C.c_void_p(self.stream.cuda_stream)
        return self.stream

    def __exit__(self, *exc):
        global _STREAM
        _STREAM = self.prev
        return self.ctx.__exit__(*exc)


def num_cus():
    """CU count of the current device as the library sees it."""
    return int(hip.lib().refvsr_num_cus())


class CuStream(torch.cuda.ExternalStream):
    """A HIP stream restricted to the CUs [first_cu, first_cu + n_cus) (refvsr_stream_create_cu_range: both multiples of 8 = an equal
    share of every XCD).  The persistent launchers of the library size their grids for n_cus CUs on it.  A torch stream in every other
    respect (events, wait_stream, record_stream, `with ops.on_stream(s)`).  The HIP stream lives as long as the process: engines keep
    their streams for their whole life and the allocator may hold record_stream references to it."""

    def __new__(cls, first_cu, n_cus, device=None):
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        out = C.c_void_p(0)
        with torch.cuda.device(dev):
            hip.check(hip.lib().refvsr_stream_create_cu_range(int(first_cu), int(n_cus), C.byref(out)), 'stream_create_cu_range')
        self = super().__new__(cls, out.value, device=dev)
        self.first_cu, self.n_cus = int(first_cu), int(n_cus)
        return self


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _planar(t, c=None):
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous(), \
        'expected contiguous cuda float32 [C,H,W], got %s %s' % (t.dtype, tuple(t.shape))
    if c is not None:
        assert t.shape[0] == c
    return t


def _nhwc(t, f32=False):
    if f32:
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous() and t.shape[2] % 4 == 0, \
            'expected contiguous cuda float32 [H,W,C%%4==0], got %s %s' % (t.dtype, tuple(t.shape))
        return t
    assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 3 and t.is_contiguous() and t.shape[2] % 8 == 0, \
        'expected contiguous cuda float16 [H,W,C%%8==0], got %s %s' % (t.dtype, tuple(t.shape))
    return t


def _round_up(a, b):
    return (a + b - 1) // b * b


def _farr(vals):
    if vals is None:
        return None
    return (C.c_float * len(vals))(*[float(v) for v in vals])


CONV24 = not env_flag('REFVSR_NO_CONV24')      # A/B knob: the generic conv kernel for the conv24 shapes as well


class ConvWeights(object):
    """Packed weights of one conv on the device (see packing.pack_conv)."""
    __slots__ = ('wpack', 'bias', 'cout', 'ksteps', 'mt', 'ksize', 'cpads', 'shuffle', 'f32', 'hi_only', 'desc', 'odtype', 'raw', 'blob24',
                 'wfmt', 'blob_wfmt', 'blob_kind')

    def __init__(self, pk, device, wfmt='hi_lo'):
        self.wpack = pk['wpack'].to(device).contiguous()
        self.bias = pk['bias'].to(device).contiguous()
        self.cout, self.ksteps, self.mt, self.ksize = pk['cout'], pk['ksteps'], pk['mt'], pk['ksize']
        self.cpads, self.shuffle, self.f32 = pk['cpads'], pk['shuffle'], bool(pk.get('f32', False))
        self.hi_only = bool(pk.get('hi_only', False))      # plain fp16 weights (descriptor weight mode 2)
        # launch descriptor with the per-weight fields filled once (the C side copies it at every call)
        d = self.desc = hip.RefvsrConv()
        d.wpack, d.bias = self.wpack.data_ptr(), self.bias.data_ptr()
        d.cout, d.mt_per_block, d.ksteps, d.ksize = self.cout, self.mt, self.ksteps, self.ksize
        d.f32 = 2 if self.hi_only else int(self.f32)
        self.odtype = torch.float32 if self.f32 else torch.float16
        self.raw = pk.get('raw')      # (weight, bias) fp32 cpu tensors when the packer kept them (repacking for specialised kernels)
        # the shapes of packing.blob_plan also carry the blob of their specialised kernel (conv24.hip; the attribute keeps its first
        # name), in the format blob_wfmt, which every launch of this conv then picks its entry point by.  wfmt: the engine's weight
        # format (Weights.wfmt)
        self.wfmt = wfmt
        self.blob_kind, self.blob_wfmt, self.blob24 = None, 'hi_lo', None
        srcs = pk.get('src_channels')
        if self.raw is not None and srcs is not None:
            flags = BlobFlags(not CONV24, env_flag('REFVSR_NO_CONV32'), env_flag('REFVSR_NO_CONV48X2'), env_flag('REFVSR_NO_CONV_SHUFFLE2'))
            self.blob_kind, self.blob_wfmt = blob_plan(tuple(self.raw[0].shape), srcs, self.shuffle, self.f32, self.hi_only, wfmt, flags)
            if self.blob_kind == 'conv24':
                self.blob24 = pack_conv24(*self.raw, srcs, wfmt=self.blob_wfmt).to(device).contiguous()
            elif self.blob_kind == 'shuffle2':
                self.blob24 = pack_conv_shuffle2(*self.raw, wfmt=self.blob_wfmt).to(device).contiguous()


def _entry(name, f16w):
    """Entry point `name` of the library, or its _f16w twin (ABI 15: the same signature over fp16-format blobs)."""
    return getattr(hip.lib(), name + '_f16w' if f16w else name)


def _c24(cw, name):
    """Entry point `name` of the conv24 family, or its _f16w twin when cw's blob is in the fp16 weight format."""
    return _entry(name, cw.blob_wfmt == 'fp16')


_CONV_ENTRY = {24: 'conv24', 32: 'conv32', 48: 'conv48'}


def _conv_route(cw, c0, c1, mul, res, h, w, stride, pad, planar, act, post, B=None):
    """The library entry (its name without 'refvsr_') a conv call on h x w maps takes.  conv() (B None): 'conv_shuffle2' | 'conv24' |
    'conv32' | 'conv48' | 'conv_mfma' (the generic kernel).  conv_b() over B >= 2 maps: 'conv_shuffle2_batch' | 'conv24_batch' |
    'per_map' (conv() map by map).  c0, c1: the sources' channel strides (c1 None: one source); mul, res: the operand (of map 0) or
    None; planar: a planar output or residual."""
    miss = 'conv_mfma' if B is None else 'per_map'
    if cw.blob24 is None or stride != 1 or pad != 1 or planar or not 0.0 <= act <= 1.0:
        return miss
    if B is not None and not multimap_ok(B):            # conv_b only: the multi-map kernels take 2 .. REFVSR_MAX_MAPS maps
        return miss
    co = cw.cout
    if cw.shuffle:
        # the 2^31 bound (32-bit element offsets in the specialised kernels: 8K HR maps go generic) is over cout alone here: the
        # [2h, 2w, C] output has the bytes of h x w x 4 C, the largest map of the call
        if c1 is not None or mul is not None or res is not None or post != 1.0 or h * w * co * 2 >= 2 ** 31:
            return miss
        if B is None:
            return 'conv_shuffle2'
        return 'conv_shuffle2_batch' if c0 == 24 else miss      # conv_b only: the multi-map kernel exists for C = 24 alone
    if not 0.0 <= post <= 1.0:
        return miss
    if B is not None:
        # conv_b only: 24 outputs alone have a multi-map kernel; the sources must match the packed ones (conv() asserts that before it
        # asks) and be on the library's own list
        if co != 24 or [c0] + ([] if c1 is None else [c1]) != list(cw.cpads) or not hip.lib().refvsr_conv24_supported(c0, c1 or 0):
            return miss
    # here the bound is over the widest map of the call, sources included (8 + 24 -> 24, 48 + 48 -> 48 ...)
    if (mul is not None and mul.shape[2] != co) or (res is not None and res.shape[2] != co) or h * w * max(co, c0, c1 or 0) * 2 >= 2 ** 31:
        return miss
    return _CONV_ENTRY[co] if B is None else 'conv24_batch'


def conv(cw, src0, src1=None, stride=1, pad=None, act=1.0, mul=None, res=None, post=1.0,
         planar_out=False, res_planar=None, add_const=0.0, clamp=None, batch=None):
    """refvsr_conv_mfma.  Returns nhwc16 [ho,wo,cout] (or [2ho,2wo,cout/4] for pixel-shuffle weights),
    or planar fp32 [cout,ho,wo] when planar_out.  For f32-packed weights all maps are fp32 HWC.
    batch = B: src0 is a contiguous batch [B,h,w,c] (res_planar [B,cout,h,w]) of images sharing the weights: ONE launch
    (RefvsrConv.batch), output [B,...]; image b == conv of image b alone, bit for bit."""
    if batch is not None:
        return _conv_batch(cw, src0, int(batch), stride, pad, act, post, planar_out, res_planar, add_const, clamp,
                           src1, mul, res)
    f32 = cw.f32
    _nhwc(src0, f32)
    if src1 is not None:
        _nhwc(src1, f32)
    c0 = src0.shape[2]
    c1 = src1.shape[2] if src1 is not None else 0
    h, w = src0.shape[:2]
    assert src1 is None or src1.shape[:2] == src0.shape[:2]
    assert [c0] + ([c1] if src1 is not None else []) == list(cw.cpads), \
        'conv input channels %s do not match packed weights %s' % ([c0, c1], cw.cpads)
    if pad is None:
        pad = cw.ksize // 2
    entry = _conv_route(cw, c0, None if src1 is None else c1, mul, res, h, w, stride, pad, planar_out or res_planar is not None, act, post)
    if entry == 'conv_shuffle2':
        # C -> 4 C conv + pixel shuffle on the compile-time-specialised kernel (csrc/conv24.hip, SHUF variant)
        out = torch.empty((2 * h, 2 * w, c0), dtype=torch.float16, device=src0.device)
        hip.check(_c24(cw, 'refvsr_conv_shuffle2')(_ptr(src0), c0, h, w, _ptr(cw.blob24), act, _ptr(out), _stream()), entry)
        return out
    if entry != 'conv_mfma':
        # compile-time-specialised kernel (24 | 32 | 48 output channels, 3x3): csrc/conv24.hip
        for m_ in (mul, res):
            if m_ is not None:
                _nhwc(m_)
                assert tuple(m_.shape[:2]) == (h, w)
        out = torch.empty((h, w, cw.cout), dtype=torch.float16, device=src0.device)
        fn = _c24(cw, 'refvsr_' + entry)
        hip.check(fn(_ptr(src0), c0, _ptr(src1), c1, h, w, _ptr(cw.blob24), act, _ptr(mul), _ptr(res), post, _ptr(out), _stream()), entry)
        return out
    return _conv_mfma(cw, src0, src1, None, stride, pad, act, mul, res, post, planar_out, res_planar, add_const, clamp)


def _conv_batch(cw, src0, B, stride, pad, act, post, planar_out, res_planar, add_const, clamp, src1, mul, res):
    assert src1 is None and mul is None and res is None and not cw.shuffle, 'batched conv: single source, no mul / res'
    assert src0.dim() == 4 and src0.shape[0] == B and src0.is_contiguous() and B >= 1
    _nhwc(src0[0], cw.f32)
    c0 = src0.shape[3]
    assert [c0] == list(cw.cpads), 'conv input channels %s do not match packed weights %s' % ([c0], cw.cpads)
    return _conv_mfma(cw, src0, None, B, stride, cw.ksize // 2 if pad is None else pad, act, None, None, post, planar_out, res_planar,
                      add_const, clamp)


def _conv_mfma(cw, src0, src1, B, stride, pad, act, mul, res, post, planar_out, res_planar, add_const, clamp):
    """The refvsr_conv_mfma launch of conv() on checked sources: ONE fill of the shared descriptor for one image (B None) or for a
    contiguous batch (src0 [B,h,w,c], res_planar [B,cout,ho,wo], output [B,...]: RefvsrConv.batch and the bs_* byte strides)."""
    f32 = cw.f32
    lead = () if B is None else (B,)
    h, w, c0 = src0.shape[-3:]
    c1 = src1.shape[2] if src1 is not None else 0
    k = cw.ksize
    ho = (h + 2 * pad - k) // stride + 1
    wo = (w + 2 * pad - k) // stride + 1
    esz = 4 if f32 else 2
    d = cw.desc
    d.src0, d.c0, d.src1, d.c1 = src0.data_ptr(), c0, (src1.data_ptr() if src1 is not None else None), c1
    d.h_in, d.w_in, d.h_out, d.w_out = h, w, ho, wo
    d.stride, d.pad = stride, pad
    d.act_slope, d.post_slope = act, post
    for name, m_ in (('mul', mul), ('res', res)):
        if m_ is not None:
            _nhwc(m_, f32)
            assert tuple(m_.shape[:2]) == (ho, wo)
        setattr(d, name, m_.data_ptr() if m_ is not None else None)
        setattr(d, name + '_c', m_.shape[2] if m_ is not None else 0)
    d.res_planar, d.add_const, d.clamp_lo, d.clamp_hi = None, 0.0, 0.0, 0.0
    d.bs_src0, d.bs_src1, d.bs_res_planar = h * w * c0 * esz, 0, 0
    if planar_out:
        out = torch.empty(lead + (cw.cout, ho, wo), dtype=torch.float32, device=src0.device)
        d.out_mode, d.out_c = OUT_PLANAR32, 0
        if res_planar is not None:
            _planar(res_planar if B is None else res_planar[0], cw.cout)
            assert res_planar.is_contiguous() and tuple(res_planar.shape) == lead + (cw.cout, ho, wo)
            d.res_planar = res_planar.data_ptr()
            d.bs_res_planar = cw.cout * ho * wo * 4
        d.add_const = add_const
        if clamp is not None:
            d.clamp_lo, d.clamp_hi = clamp
        d.bs_out = cw.cout * ho * wo * 4
    else:
        up = 2 if cw.shuffle else 1                 # pixel-shuffle weights: [2ho, 2wo, cout / 4]
        co = _round_up(cw.cout // 4, 8) if cw.shuffle else _round_up(cw.cout, 4 if f32 else 8)    # channel stride of the map (padding channels are written as zeros)
        out = torch.empty(lead + (up * ho, up * wo, co), dtype=torch.float16 if cw.shuffle else cw.odtype, device=src0.device)
        d.out_mode, d.out_c = OUT_NHWC16_SHUFFLE2 if cw.shuffle else OUT_NHWC16, co
        d.bs_out = ho * wo * co * esz
    d.out = out.data_ptr()
    d.batch = B or 0
    try:
        hip.check(hip.lib().refvsr_conv_mfma(C.byref(d), _stream()), 'conv_mfma')
    finally:
        d.batch = 0                                  # the descriptor is shared between the batched and the single-image calls
    return out


_WAVES_SET = False


def resblock_fits(c):
    """Channel counts of the runtime-generic fused block (resblock_lean.hip: C in {8, 16, 24, 32})."""
    return bool(hip.lib().refvsr_resblock_lean_fits(int(c)))


def _apply_resblock_knobs():
    global _WAVES_SET
    if not _WAVES_SET:                     # A/B knob of the lean kernel's workgroup shape (default 8 waves)
        _WAVES_SET = True
        if os.environ.get('REFVSR_RESBLOCK_WAVES'):
            hip.check(hip.lib().refvsr_set_resblock_waves(int(os.environ['REFVSR_RESBLOCK_WAVES'])), 'set_resblock_waves')


def resblock(cw1, cw2, x, act, post=1.0):
    """refvsr_resblock_lean: post(x + conv2(act(conv1(x)))) in one launch (3x3, C->C)."""
    _nhwc(x)
    h, w, c = x.shape
    assert cw1.cpads == [c] and cw2.cpads == [c] and cw1.cout == c and cw2.cout == c and cw1.ksize == 3
    assert not cw1.f32 and not cw1.shuffle and cw1.wpack.shape[0] == 1
    out = torch.empty_like(x)
    _apply_resblock_knobs()
    hip.check(hip.lib().refvsr_resblock_lean(_ptr(x), c, h, w, _ptr(cw1.wpack), _ptr(cw1.bias), _ptr(cw2.wpack),
                                             _ptr(cw2.bias), cw1.ksteps, act, post, _ptr(out), _stream()), 'resblock_lean')
    return out


class ResblockChain(object):
    """Pointer tables of a run of fused blocks (built once per run of packed weights, reused by every call)."""

    def __init__(self, pairs):
        self.pairs = list(pairs)
        n = self.n = len(self.pairs)
        c1 = self.pairs[0][0]
        self.c, self.ksteps = c1.cout, c1.ksteps
        for a, b in self.pairs:
            assert a.cpads == [self.c] and b.cpads == [self.c] and a.cout == self.c and b.cout == self.c and a.ksize == 3
            assert not a.f32 and not a.shuffle and a.wpack.shape[0] == 1 and a.ksteps == self.ksteps
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        self.w1, self.b1 = arr([a.wpack for a, _ in self.pairs]), arr([a.bias for a, _ in self.pairs])
        self.w2, self.b2 = arr([b.wpack for _, b in self.pairs]), arr([b.bias for _, b in self.pairs])


def resblock_chain(chain, x, act, post=1.0):
    """refvsr_resblock_chain: chain.n fused blocks behind ONE library call (same launches and results as chain.n calls of
    resblock(); two scratch maps instead of n - 1 intermediates).  """
    _nhwc(x)
    h, w, c = x.shape
    assert c == chain.c
    out = torch.empty_like(x)
    s0 = torch.empty_like(x) if chain.n >= 2 else None
    s1 = torch.empty_like(x) if chain.n >= 3 else None
    hip.check(hip.lib().refvsr_resblock_chain(_ptr(x), c, h, w, chain.n, chain.w1, chain.b1, chain.w2, chain.b2, chain.ksteps,
                                              act, post, _ptr(s0), _ptr(s1), _ptr(out), _stream()), 'resblock_chain')
    return out


class BlobChain(object):
    """A run of fused c-channel blocks (c = 24 | 48) for refvsr_resblock<c>_chain as one device buffer [n, stride] of per-block blobs
    (packing.pack_resblock).  pairs: [(conv1, conv2)] ConvWeights whose packer kept the raw fp32 weights, or [((w1, b1), (w2, b2))]
    raw tensors.  wfmt (c = 24): 'hi_lo' | 'fp16' (the blobs of refvsr_resblock24_chain_f16w); None = the weight format of the
    ConvWeights (raw tensors: 'hi_lo').  The 48-channel block has no fp16-format twin: always 'hi_lo'."""

    def __init__(self, pairs, device, c, wfmt=None):
        pairs = list(pairs)
        if c != 24:
            assert wfmt is None
            wfmt = 'hi_lo'
        elif wfmt is None:
            fmts = set(x.wfmt if isinstance(x, ConvWeights) else 'hi_lo' for p in pairs for x in p)
            assert len(fmts) == 1, 'one weight format per chain: %s' % sorted(fmts)
            wfmt = fmts.pop()
        self.wfmt = wfmt
        self.n = len(pairs)
        raw = lambda x: x.raw if isinstance(x, ConvWeights) else x
        self.blobs = torch.stack([pack_resblock(c, wfmt, *raw(a), *raw(b)) for a, b in pairs], 0).to(device).contiguous()
        self.stride = self.blobs.shape[1]
        assert self.stride == _RB_BLOB_BYTES[c, wfmt] and self.blobs.data_ptr() % 16 == 0


_RB_BLOB_BYTES = {(24, 'hi_lo'): hip.RESBLOCK24_BLOB_BYTES, (24, 'fp16'): hip.RESBLOCK24_F16W_BLOB_BYTES, (48, 'hi_lo'): hip.RESBLOCK48_BLOB_BYTES}


def Resblock24Chain(pairs, device, wfmt=None):
    return BlobChain(pairs, device, 24, wfmt)


def Resblock48Chain(pairs, device):
    return BlobChain(pairs, device, 48)


_RB24_KNOBS_SET = False


def _rb_entry(c, chain, name):
    """Entry point `name` of the c-channel fused block ('resblock24_chain' ...): for c = 24 the A/B knobs of its workgroup shape
    (default 8 waves) and output store path (0 | 1, refvsr_set_resblock24_store) are applied before the first call, and a chain of
    fp16-format blobs goes to the _f16w twin (chain-like objects without a weight format -- torch_ops' blob tables -- are hi + lo)."""
    global _RB24_KNOBS_SET
    if c == 24 and not _RB24_KNOBS_SET:
        _RB24_KNOBS_SET = True
        if os.environ.get('REFVSR_RESBLOCK24_WAVES'):
            hip.check(hip.lib().refvsr_set_resblock24_waves(int(os.environ['REFVSR_RESBLOCK24_WAVES'])), 'set_resblock24_waves')
        if os.environ.get('REFVSR_RB24_STORE'):
            hip.check(hip.lib().refvsr_set_resblock24_store(int(os.environ['REFVSR_RB24_STORE'])), 'set_resblock24_store')
    return _entry('refvsr_' + name, c == 24 and getattr(chain, 'wfmt', 'hi_lo') == 'fp16')


def _rb_chain(c, chain, xs, act, B=None):
    """refvsr_resblock<c>_chain on the map xs (B None), or refvsr_resblock<c>_chain_batch on the list xs of B maps -> [B, h, w, c]."""
    maps = [xs] if B is None else xs
    for t_ in maps:
        _nhwc(t_)
        assert tuple(t_.shape) == tuple(maps[0].shape) and t_.shape[2] == c
    h, w, _ = maps[0].shape
    out = torch.empty(((B,) if B else ()) + (h, w, c), dtype=torch.float16, device=maps[0].device)
    s0 = torch.empty_like(out) if chain.n >= 2 else None
    s1 = torch.empty_like(out) if chain.n >= 3 else None
    name = 'resblock%d_chain' % c + ('_batch' if B else '')
    src = (_parr(xs), B) if B else (_ptr(xs),)
    hip.check(_rb_entry(c, chain, name)(*src, h, w, chain.n, _ptr(chain.blobs), chain.stride, act, _ptr(s0), _ptr(s1),
                                        _parr(list(out)) if B else _ptr(out), _stream()), name)
    return out


def resblock24_chain(chain, x, act):
    """refvsr_resblock24_chain: chain.n fused 24-channel blocks x <- x + conv2(act(conv1 x)) behind one library call."""
    return _rb_chain(24, chain, x, act)


def resblock48_chain(chain, x, act):
    """refvsr_resblock48_chain: chain.n fused 48-channel blocks x <- x + conv2(act(conv1 x)), one launch per block."""
    return _rb_chain(48, chain, x, act)


def resblock_chain_ok(c):
    _apply_resblock_knobs()
    return bool(hip.lib().refvsr_resblock_lean_fits(int(c)))


def conv_direct(x, w, b, stride=1, pad=None, act=1.0, nhwc16_out=False):
    """refvsr_conv_direct_f32 on a planar fp32 map; w fp32 [cout,cin,k,k] on the device."""
    _planar(x)
    cout, cin, k, _ = w.shape
    assert x.shape[0] == cin and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    if pad is None:
        pad = k // 2
    h, wd = x.shape[1:]
    ho = (h + 2 * pad - k) // stride + 1
    wo = (wd + 2 * pad - k) // stride + 1
    if nhwc16_out:
        assert cout % 8 == 0
        out = torch.empty((ho, wo, cout), dtype=torch.float16, device=x.device)
    else:
        out = torch.empty((cout, ho, wo), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().refvsr_conv_direct_f32(_ptr(x), cin, h, wd, _ptr(w), _ptr(b), cout, k, stride, pad, act,
                                               _ptr(out), int(nhwc16_out), cout if nhwc16_out else 0, _stream()),
              'conv_direct_f32')
    return out


def conf_alpha(conf_a, conf_b, up, w0, b0, cw, slope0=0.2, slope1=0.2, want_max=False):
    """refvsr_conf_alpha: conv_{16->C}(lrelu(conv_{2->16}(P))) with P = cat[conf_a, conf_b] (up = 1) or its clamped bicubic x2
    up-sampling (up = 2), one launch.  conf_a / conf_b planar fp32 [1,h,w]; w0 / b0 the 2 -> 16 conv (fp32, device); cw the packed
    16 -> C conv (ConvWeights with a conv24 / conv48 blob).  Returns alpha [up h, up w, C] (and max(conf_a, conf_b) [1,h,w])."""
    return _conf_alpha(conf_a, conf_b, up, w0, b0, cw, slope0, slope1, want_max)


def _conf_alpha(conf_as, conf_bs, up, w0, b0, cw, slope0, slope1, want_max, B=None):
    """refvsr_conf_alpha on one pair of maps (B None), or refvsr_conf_alpha_batch on the lists of B maps -> [B, ...] results."""
    a_s, b_s = ([conf_as], [conf_bs]) if B is None else (conf_as, conf_bs)
    for t_ in list(a_s) + list(b_s):
        _planar(t_, 1)
        assert t_.shape == a_s[0].shape
    assert conf_alpha_ok(cw, B)
    assert tuple(w0.shape) == (16, 2, 3, 3) and w0.is_cuda and w0.dtype == torch.float32 and w0.is_contiguous() and b0.numel() == 16
    lead = (B,) if B else ()
    h, w = a_s[0].shape[1:]
    dev = a_s[0].device
    alpha = torch.empty(lead + (up * h, up * w, cw.cout), dtype=torch.float16, device=dev)
    cmax = torch.empty(lead + (1, h, w), dtype=torch.float32, device=dev) if want_max else None
    tab = (lambda t: None if t is None else _parr(list(t))) if B else _ptr
    name = 'conf_alpha_batch' if B else 'conf_alpha'
    hip.check(_c24(cw, 'refvsr_' + name)(tab(conf_as), tab(conf_bs), *lead, h, w, up, _ptr(w0), _ptr(b0), slope0, _ptr(cw.blob24), cw.cout,
                                         slope1, tab(alpha), tab(cmax), _stream()), name)
    return (alpha, cmax) if want_max else alpha


RESULT_DTYPES = {'float32': (torch.float32, hip.RESULT_F32), 'float16': (torch.float16, hip.RESULT_F16), 'uint8': (torch.uint8, hip.RESULT_U8)}


def result_format(name):
    """(torch dtype, REFVSR_RESULT_*) of config.result_dtype ('float32' | 'float16' | 'uint8'; None = 'float32')."""
    key = str(name or 'float32').replace('torch.', '')
    if key not in RESULT_DTYPES:
        raise ValueError("result_dtype must be 'float32', 'float16' or 'uint8', got %r" % (name,))
    return RESULT_DTYPES[key]


RESULT_LAYOUTS = ('chw', 'hwc')


def check_result_layout(name):
    """config.result_layout resolved: 'chw' (planar [3, h, w] memory; None = 'chw') | 'hwc' (the channels-last view of dense [h, w, 3]
    memory, REFVSR_RESULT_HWC: what image writers and encoders consume; the logical shape and the values do not change)."""
    key = str(name or 'chw')
    if key not in RESULT_LAYOUTS:
        raise ValueError("result_layout must be 'chw' or 'hwc', got %r" % (name,))
    return key


def _result_empty(h, w, dt, device, layout):
    """An uninitialised [3, h, w] result of the layout (hwc: the view of a dense [h, w, 3] array) and the flag for its out_fmt."""
    if check_result_layout(layout) == 'hwc':
        return torch.empty((h, w, 3), dtype=dt, device=device).permute(2, 0, 1), hip.RESULT_HWC
    return torch.empty((3, h, w), dtype=dt, device=device), 0


def stack_results(frames, layout=None):
    """[3, h, w] results -> [n, 3, h, w]; with 'hwc' the dense [n, h, w, 3] array viewed channels-first (a plain torch.stack would
    re-planarise the frames)."""
    if check_result_layout(layout) == 'hwc':
        return torch.stack([f.permute(1, 2, 0) for f in frames]).permute(0, 3, 1, 2)
    return torch.stack(frames)


def result_layout_of(x):
    """'chw' | 'hwc' of a result [..., 3, h, w] by its strides (any dtype): contiguous, or the channels-last view of dense
    [..., h, w, 3] memory; None for any other strides.  (A frame both describe, e.g. h = w = 1, counts as 'chw'.)"""
    if x.dim() < 3 or x.shape[-3] != 3:
        return None
    if x.is_contiguous():
        return 'chw'
    if x.movedim(-3, -1).is_contiguous():
        return 'hwc'
    return None


def convert_result(x, result_dtype, result_layout=None):
    """fp32 planar result in [0, 1] -> fp16 | uint8 = rint(255 x) (refvsr_convert_result: what the fused heads store directly);
    result_layout = 'hwc': the same values as the channels-last view of dense [h, w, 3] memory (refvsr_convert_result_hwc; x [3, h, w])."""
    dt, fmt = result_format(result_dtype)
    if check_result_layout(result_layout) == 'hwc':
        _planar(x, 3)
        h, w = x.shape[1:]
        out, flag = _result_empty(h, w, dt, x.device, 'hwc')
        hip.check(hip.lib().refvsr_convert_result_hwc(_ptr(x), h, w, fmt | flag, _ptr(out), _stream()), 'convert_result_hwc')
        return out
    if fmt == hip.RESULT_F32:
        return x
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(x.shape, dtype=dt, device=x.device)
    hip.check(hip.lib().refvsr_convert_result(_ptr(x), x.numel(), fmt, _ptr(out), _stream()), 'convert_result')
    return out


def conv_last(blob, src, base_lr, result_dtype=None, result_layout=None):
    """refvsr_conv_last: clamp(conv3x3_{C->3}(src) + bias + clamp01(bicubic(base_lr)), 0, 1) -> planar [3, h, w] in one launch (fp32, or
    result_dtype = 'float16' | 'uint8': REFVSR_RESULT_*; result_layout = 'hwc': the same [3, h, w] tensor over dense [h, w, 3] memory).
    blob: packing.pack_conv_last on the device; src nhwc16 [h, w, C]; base_lr planar fp32 [3, h / s, w / s]."""
    _nhwc(src)
    _planar(base_lr, 3)
    h, w, c = src.shape
    bh, bw = base_lr.shape[1:]
    dt, fmt = result_format(result_dtype)
    out, flag = _result_empty(h, w, dt, src.device, result_layout)
    hip.check(hip.lib().refvsr_conv_last_fmt(_ptr(src), c, h, w, _ptr(blob), _ptr(base_lr), bh, bw, _ptr(out), fmt | flag, _stream()), 'conv_last')
    return out


def conv_hr_last(blob, src, base_lr, act=0.1, result_dtype=None, result_layout=None):
    """refvsr_conv_hr_last: clamp(conv_last(lrelu(conv_hr(src))) + clamp01(bicubic(base_lr)), 0, 1) -> planar [3, h, w], one launch
    (mid_channels = 24; fp32, or result_dtype = 'float16' | 'uint8'; result_layout as conv_last).  blob: packing.pack_conv_hr_last on the device."""
    _nhwc(src)
    _planar(base_lr, 3)
    h, w, c = src.shape
    assert c == 24 and blob.numel() == hip.RESBLOCK24_BLOB_BYTES
    bh, bw = base_lr.shape[1:]
    dt, fmt = result_format(result_dtype)
    out, flag = _result_empty(h, w, dt, src.device, result_layout)
    hip.check(hip.lib().refvsr_conv_hr_last_fmt(_ptr(src), h, w, _ptr(blob), act, _ptr(base_lr), bh, bw, _ptr(out), fmt | flag, _stream()), 'conv_hr_last')
    return out


def conv_last_ok(c, h, w):
    return bool(hip.lib().refvsr_conv_last_supported(int(c))) and h * w * c * 2 < 2 ** 31


def conf_alpha_ok(cw, B=None):
    """cw can be the 16 -> C conv of refvsr_conf_alpha (B None: C = 24 | 48) or of refvsr_conf_alpha_batch over B maps (C = 24)."""
    return cw.blob24 is not None and cw.cpads == [16] and cw.cout in ((24, 48) if B is None else (24,)) and not cw.shuffle


def _pack_nhwc(x, cs, name, align, dtype):
    _planar(x)
    c, h, w = x.shape
    cs = cs or _round_up(c, align)
    out = torch.empty((h, w, cs), dtype=dtype, device=x.device)
    hip.check(getattr(hip.lib(), 'refvsr_' + name)(_ptr(x), c, h, w, _ptr(out), cs, _stream()), name)
    return out


def pack_nhwc16(x, cs=None):
    return _pack_nhwc(x, cs, 'pack_nhwc16', 8, torch.float16)


def pack_nhwc32(x, cs=None):
    return _pack_nhwc(x, cs, 'pack_nhwc32', 4, torch.float32)


def conv1x1_f32(x, w, b, act=0.2):
    """refvsr_conv1x1_f32: fp32 HWC [h][w][cin] -> planar fp32 [16][h][w], 1x1 conv + LeakyReLU (the matching's map64 / map128 block)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    h, w_, cin = x.shape
    assert tuple(w.shape) == (16, cin) and w.dtype == torch.float32 and w.is_contiguous() and tuple(b.shape) == (16,)
    out = torch.empty((16, h, w_), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().refvsr_conv1x1_f32(_ptr(x), cin, h, w_, _ptr(w), _ptr(b), float(act), _ptr(out), _stream()), 'conv1x1_f32')
    return out


def unpack_nhwc16(x, c=None):
    _nhwc(x)
    h, w, cs = x.shape
    c = c or cs
    out = torch.empty((c, h, w), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().refvsr_unpack_nhwc16(_ptr(x), h, w, cs, c, _ptr(out), _stream()), 'unpack_nhwc16')
    return out


def resize(x, out_hw, mode, src_scale=None, mean=None, std=None, chan_mul=None, clamp01=False, nhwc16_out=False):
    """F.interpolate restatement.  src_scale: (sy, sx) source step per output sample; default in/out."""
    _planar(x)
    c, h, w = x.shape
    oh, ow = out_hw
    if src_scale is None:
        src_scale = (float(h) / float(oh), float(w) / float(ow))
    if nhwc16_out:
        out = torch.empty((oh, ow, 8), dtype=torch.float16, device=x.device)
    else:
        out = torch.empty((c, oh, ow), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().refvsr_resize(_ptr(x), c, h, w, _ptr(out), oh, ow, mode, src_scale[0], src_scale[1],
                                      _farr(mean), _farr(std), _farr(chan_mul), int(clamp01), int(nhwc16_out),
                                      8 if nhwc16_out else 0, _stream()), 'resize')
    return out


def bicubic_scale(x, factor, clamp01=True, nhwc16_out=False):
    """F.interpolate(x, scale_factor=factor, mode='bicubic', align_corners=False)[.clamp(0,1)]."""
    c, h, w = x.shape
    oh, ow = int(math.floor(h * factor)), int(math.floor(w * factor))
    s = 1.0 / factor
    return resize(x, (oh, ow), RS_BICUBIC, (s, s), clamp01=clamp01, nhwc16_out=nhwc16_out)


def flow_up2(flow):
    """F.interpolate(flow, scale_factor=2, 'bilinear', align_corners=True) * 2."""
    c, h, w = flow.shape
    return resize(flow, (2 * h, 2 * w), RS_BILINEAR_AC, (0.0, 0.0), chan_mul=[2.0] * c)


def _pool2(x, name):
    _planar(x)
    c, h, w = x.shape
    out = torch.empty((c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    hip.check(getattr(hip.lib(), 'refvsr_' + name)(_ptr(x), c, h, w, _ptr(out), _stream()), name)
    return out


def avgpool2(x):
    return _pool2(x, 'avgpool2')


def maxpool2(x):
    return _pool2(x, 'maxpool2')


def avgpool_pyramid(x):
    """Five avgpool2 calls in one launch (refvsr_avgpool_pyramid): x planar [c,h,w] with h, w multiples of 32 -> the list of the five
    coarser levels, finest first (views of one allocation).  The same bits as the five calls."""
    _planar(x)
    c, h, w = x.shape
    assert h % 32 == 0 and w % 32 == 0
    sizes = [c * (h >> k) * (w >> k) for k in range(1, 6)]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + (n + 63) // 64 * 64)
    buf = torch.empty((offs[-1],), dtype=torch.float32, device=x.device)
    lv = [buf[offs[k]:offs[k] + sizes[k]].view(c, h >> (k + 1), w >> (k + 1)) for k in range(5)]
    dst = (C.c_void_p * 5)(*[t_.data_ptr() for t_ in lv])
    hip.check(hip.lib().refvsr_avgpool_pyramid(_ptr(x), c, h, w, dst, _stream()), 'avgpool_pyramid')
    return lv


def frame_prep(lr, ref, w, b):
    """refvsr_frame_prep: what pack_nhwc16 x 2, the 1x1 MeanShift conv_direct x 2, avgpool2 of the reference map and pack_nhwc32 x 2
    make of the planar fp32 frames lr [3,h,w] / ref [3,hr,wr], in one launch and the same bits.  w [3,3,1,1] / b [3]: the MeanShift.
    Returns (lr8 [h,w,8] fp16, ref8 [hr,wr,8] fp16, lr_n [h,w,4] fp32, ref_n [hr//2,wr//2,4] fp32)."""
    _planar(lr, 3)
    _planar(ref, 3)
    assert tuple(w.shape) == (3, 3, 1, 1) and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    assert tuple(b.shape) == (3,) and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()
    h, wd = lr.shape[1:]
    hr, wr = ref.shape[1:]
    lr8 = torch.empty((h, wd, 8), dtype=torch.float16, device=lr.device)
    ref8 = torch.empty((hr, wr, 8), dtype=torch.float16, device=lr.device)
    lr_n = torch.empty((h, wd, 4), dtype=torch.float32, device=lr.device)
    ref_n = torch.empty((hr // 2, wr // 2, 4), dtype=torch.float32, device=lr.device)
    hip.check(hip.lib().refvsr_frame_prep(_ptr(lr), h, wd, _ptr(ref), hr, wr, _ptr(w), _ptr(b), _ptr(lr8), _ptr(ref8), _ptr(lr_n),
                                          _ptr(ref_n), _stream()), 'frame_prep')
    return lr8, ref8, lr_n, ref_n


def max2(a, b):
    assert a.shape == b.shape and a.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    out = torch.empty_like(a)
    hip.check(hip.lib().refvsr_max2(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), 'max2')
    return out


def _chunks(n, per):
    """(s0, count) of the library calls over n frames, at most `per` frames each: the frames [s0, s0 + count) of every frame op's tables."""
    for s0 in range(0, n, per):
        yield s0, min(per, n - s0)


class _Cache(dict):
    """The frame ops' caches (workspaces per device, stream and geometry; device tables per geometry): built on a miss, all dropped once
    more than 16 are held."""

    def get_or_build(self, key, build):
        v = self.get(key)
        if v is None:
            if len(self) > 16:
                self.clear()
            v = self[key] = build()
        return v


def _workspace(cache, dev, st, h, w, nbytes, what, too_small, esize=8):
    """The cached workspace of one full launch per (device, stream, h, w): nbytes() bytes as floats of esize = 8 | 4 bytes; nbytes() = 0
    is the library's refusal of the geometry: `too_small` says why."""
    def build():
        n = nbytes()
        if n == 0:
            raise RuntimeError('%s: %s (got %d x %d)' % (what, too_small, h, w))
        return torch.empty(n // esize, dtype={8: torch.float64, 4: torch.float32}[esize], device=dev)
    return cache.get_or_build((dev, st.value, h, w), build)


_RESULT_CODES = dict(RESULT_DTYPES.values())          # torch dtype -> REFVSR_RESULT_*


def _src_fmt(dtype, lay):
    """REFVSR_RESULT_* | REFVSR_RESULT_HWC of result frames of the dtype and layout ('chw' | 'hwc')."""
    return _RESULT_CODES[dtype] | (hip.RESULT_HWC if lay == 'hwc' else 0)


def _check_dense(name, noun, f, lay):
    """The frame f of a frame op's `noun` ('results' | 'frames') is dense and of the layout `lay` of the first (result_layout_of)."""
    if lay is None or result_layout_of(f) != lay:
        raise RuntimeError('%s: %s must be dense and of one layout, contiguous [3, h, w] or the channels-last view of [h, w, 3] '
                           '(config.result_layout), got strides %s' % (name, noun, tuple(f.stride())))


def _result_frames(name, frames, noun):
    """The result frames of a frame op as a list, at least one, the first a cuda float32 | float16 | uint8 [3,h,w]: (frames, h, w).  The
    caller's own checks of h and w come next, then _result_format."""
    frames = list(frames)
    if not frames:
        raise RuntimeError('%s: at least one frame' % name)
    f0 = frames[0]
    if not (f0.is_cuda and f0.dtype in _RESULT_CODES and f0.dim() == 3 and f0.shape[0] == 3):
        raise RuntimeError('%s: cuda float32 | float16 | uint8 %s [3,h,w] (got %s %s %s)' % (name, noun, f0.device.type, f0.dtype, tuple(f0.shape)))
    _, h, w = f0.shape
    return frames, h, w


def _result_format(name, frames, noun):
    """Every frame of _result_frames' list has the first's dtype and geometry, lies on a GPU and is dense in one layout: the source
    format of them all."""
    f0 = frames[0]
    lay = result_layout_of(f0)
    for f in frames:
        if f.shape != f0.shape or f.dtype != f0.dtype or not f.is_cuda:
            raise RuntimeError('%s: frames must all be %s [3, %d, %d] (got %s %s)' % (name, f0.dtype, f0.shape[1], f0.shape[2], f.dtype, tuple(f.shape)))
        _check_dense(name, noun, f, lay)
    return _src_fmt(f0.dtype, lay)


def _pairs_equal(pairs, name, ok):
    """refvsr_<name> over (a, b) pairs of one size in bytes, ok(a, b) asserted per pair: one launch per 32 pairs, one D2H sync."""
    if not pairs:
        return []
    nbytes = pairs[0][0].numel() * pairs[0][0].dtype.itemsize
    flags = torch.ones(len(pairs), dtype=torch.int32, device=pairs[0][0].device)
    for s0, n in _chunks(len(pairs), 32):
        chunk = pairs[s0:s0 + n]
        for a, b in chunk:
            assert ok(a, b) and a.dtype == b.dtype == pairs[0][0].dtype and a.numel() == b.numel() == pairs[0][0].numel()
        hip.check(getattr(hip.lib(), 'refvsr_' + name)(_parr([a for a, _ in chunk]), _parr([b for _, b in chunk]), n, nbytes,
                                                       C.c_void_p(flags.data_ptr() + 4 * s0), _stream()), name)
    return [bool(v) for v in flags.cpu().tolist()]


def buffers_equal(pairs):
    """pairs: list of (a, b) float32 tensors of one common shape.  Returns a python list of bools (one launch per 32 pairs, one D2H sync)."""
    return _pairs_equal(pairs, 'buffers_equal', lambda a, b: a.shape == b.shape and a.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous())


def bytes_equal(pairs):
    """pairs: list of (a, b) uint8 tensors of one size whose bytes are dense (contiguous, or a channels-last frame: u8_layout; a and b
    may differ in alignment), or contiguous uint16 tensors (4:2:0 frames of 10-bit samples), compared through their bytes.  Returns a
    python list of bools -- True where the raw bytes are equal (one launch per 32 pairs, one D2H sync).  The caller compares frames
    of one layout only."""
    return _pairs_equal(pairs, 'bytes_equal', lambda a, b: a.dtype in (torch.uint8, torch.uint16) and
                        all(x.is_contiguous() or u8_layout(x) is not None for x in (a, b)))


def u8_layout(x):
    """Layout code of a uint8 frame [3,h,w] or window [t,3,h,w] whose frames are dense: INGEST_PLANAR (contiguous) or INGEST_HWC
    (the channels-last view of [.., h, w, 3] bytes, e.g. x.permute(0, 3, 1, 2) of a decoded window); None for any other strides."""
    if x.dtype != torch.uint8 or x.shape[-3] != 3:
        return None
    if x.is_contiguous():
        return hip.INGEST_PLANAR
    if x.movedim(-3, -1).is_contiguous():
        return hip.INGEST_HWC
    return None


def ingest_table():
    """The library's byte -> float table (256 floats, host query, no device work): T[u] = (float)((double)u / 255.0)."""
    t = (C.c_float * 256)()
    hip.check(hip.lib().refvsr_ingest_table(t), 'ingest_table')
    return list(t)


def _decode_frames(pairs, name, what, ok, max_frames, launch):
    """ingest_u8 / yuv420_ingest over pairs [(src frame, dst float32 [3,h,w] contiguous)] of one h x w: ok(src, h, w) asserted per pair
    (`what`), then one launch(srcs, dsts, n, h, w) of refvsr_<name> per max_frames frames, on the current stream."""
    h, w = pairs[0][1].shape[1:]
    for src, dst in pairs:
        assert ok(src, h, w) and _planar(dst, 3).shape[1:] == (h, w), what
    for s0, n in _chunks(len(pairs), max_frames):
        chunk = pairs[s0:s0 + n]
        hip.check(launch(_parr([s_ for s_, _ in chunk]), _parr([d for _, d in chunk]), n, h, w), name)


def _frames_of(x, nd, dense, align, h, w, decode):
    """ingest_frames / yuv420_to_frames: x [..., <nd frame dimensions>] made dense (a copy otherwise) in storage aligned to `align` bytes
    (a copy otherwise: it keeps the strides of a dense tensor), a new contiguous float32 [..., 3, h, w] allocated, both viewed as
    frames and handed to decode([(src frame, dst frame)]).  Returns the new tensor."""
    if not dense(x):
        x = x.contiguous()
    if x.data_ptr() % align:
        x = x.clone()
    out = torch.empty(tuple(x.shape[:-nd]) + (3, h, w), dtype=torch.float32, device=x.device)
    if x.is_contiguous():
        frames = x.reshape((-1,) + tuple(x.shape[-nd:]))
    else:                                            # (channels-last uint8 RGB)
        frames = x.movedim(-3, -1).reshape(-1, h, w, 3).permute(0, 3, 1, 2)
    decode(list(zip(frames, out.view(-1, 3, h, w))))
    return out


def ingest_u8(pairs):
    """pairs: [(src uint8 [3,h,w] (u8_layout not None), dst float32 [3,h,w] contiguous)] of one h x w: dst = src / 255 exactly as the
    reference loader computes it (refvsr_ingest_u8).  One launch per layout and REFVSR_INGEST_MAX_FRAMES frames."""
    what = 'ingest_u8: uint8 [3,h,w] planar or channels-last frames of one size'
    lays = [u8_layout(src) for src, _ in pairs]
    assert None not in lays, what
    for lay in sorted(set(lays)):
        _decode_frames([p for p, l_ in zip(pairs, lays) if l_ == lay], 'ingest_u8', what, lambda src, h, w: src.shape == pairs[0][1].shape,
                       hip.INGEST_MAX_FRAMES, lambda ps, pd, n, h, w: hip.lib().refvsr_ingest_u8(ps, pd, n, h, w, lay, _stream()))


def ingest_frames(x):
    """uint8 [..., 3, h, w] (planar or channels-last; other strides and unaligned storage are copied first) -> a new contiguous
    float32 tensor of the same shape, x / 255 as the reference loader computes it, frame by frame through refvsr_ingest_u8."""
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() >= 3 and x.shape[-3] == 3, 'ingest_frames: cuda uint8 [..., 3, h, w]'
    return _frames_of(x, 3, lambda x_: u8_layout(x_) is not None, 4, x.shape[-2], x.shape[-1], ingest_u8)


_SCORE_WS = _Cache()  # (device, stream handle, h, w) -> workspace of one full refvsr_score_frames launch
_TOO_SMALL = 'frames must be at least 7 x 7'          # both scorers' refusal of a geometry (the SSIM window)


def _score_inputs(outs, gts, what, down=1):
    """The frame pairs of a scorer call, checked: (results, ground truths, h, w, result format, ground-truth format, layout); h, w are
    the ground truth's, the results are [3, down h, down w]."""
    outs, gts = list(outs), list(gts)
    assert outs and len(outs) == len(gts), '%s: as many results as ground truths' % what
    a0, g0 = outs[0], gts[0]
    _, h, w = a0.shape if down == 1 else g0.shape
    assert a0.dtype in _RESULT_CODES and g0.dtype in (torch.float32, torch.uint8), '%s: float32 | float16 | uint8 results, float32 | uint8 ground truth' % what
    lay = u8_layout(g0) if g0.dtype == torch.uint8 else hip.INGEST_PLANAR
    alay = result_layout_of(a0)
    for a, g in zip(outs, gts):
        if down == 1 and (a.shape != (3, h, w) or g.shape != (3, h, w)):
            raise RuntimeError('%s: result %s and ground truth %s must both be [3, %d, %d]' % (what, tuple(a.shape), tuple(g.shape), h, w))
        if down != 1 and (a.shape != (3, down * h, down * w) or g.shape != (3, h, w)):
            raise RuntimeError('%s: result %s and ground truth %s must both be [3, %d, %d] after the down-scale by %d (the result %d times that)'
                               % (what, tuple(a.shape), tuple(g.shape), h, w, down, down))
        assert a.is_cuda and g.is_cuda and a.dtype == a0.dtype and g.dtype == g0.dtype
        _check_dense(what, 'results', a, alay)
        assert (u8_layout(g) if g.dtype == torch.uint8 else (hip.INGEST_PLANAR if g.is_contiguous() else None)) == lay and lay is not None, \
            '%s: ground-truth frames must be dense and of one layout' % what
    return outs, gts, h, w, _src_fmt(a0.dtype, alay), _RESULT_CODES[g0.dtype], lay


def score_frames(outs, gts, win=7, down=1):
    """{mse, ssim} of B (result, ground truth) pairs of one 3 x h x w geometry, computed on the device (refvsr_score_frames): a
    torch.float64 [B, 2] tensor on the current stream, no synchronisation.  outs: [B,3,h,w] tensor or B tensors [3,h,w], contiguous
    or channels-last (config.result_layout = 'hwc': the same scores, bit for bit),
    float32 / float16 / uint8 (what the output head stores; a byte means byte / 255); gts: the same shapes, contiguous float32, or
    uint8 planar or channels-last (u8_layout).  win = 7: both numbers; win = 0: the mse alone (ssim field 0).  One launch per
    REFVSR_SCORE_MAX_FRAMES pairs.  PSNR = metrics.psnr_from_mse(mse) on the host.
    down = 2 | 4 (the flag_HD_in configs; refvsr_score_frames_down): outs are [3, down h, down w] against gts [3, h, w]; the kernel
    forms the bicubic down-scale D of the result while it stages its tiles (metrics.down_bicubic_model) and returns the mse of
    clamp(D, 0, 1) and the ssim of D."""
    if down not in (1, 2, 4):
        raise RuntimeError('score_frames: down must be 1, 2 or 4 (got %r)' % (down,))
    outs, gts, h, w, afmt, gfmt, lay = _score_inputs(outs, gts, 'score_frames', down)
    st = _stream()
    dev = outs[0].device
    ws = _workspace(_SCORE_WS, dev, st, h, w, lambda: hip.lib().refvsr_score_workspace_bytes(hip.SCORE_MAX_FRAMES, h, w), 'score_frames', _TOO_SMALL)
    scores = torch.empty((len(outs), 2), dtype=torch.float64, device=dev)
    for s0, n in _chunks(len(outs), hip.SCORE_MAX_FRAMES):
        pa, pg = _parr(outs[s0:s0 + n]), _parr(gts[s0:s0 + n])
        tail = (int(win), _ptr(ws), ws.numel() * 8, C.c_void_p(scores.data_ptr() + 16 * s0), st)
        if down == 1:
            hip.check(hip.lib().refvsr_score_frames(pa, afmt, pg, gfmt, lay, n, h, w, *tail), 'score_frames')
        else:
            hip.check(hip.lib().refvsr_score_frames_down(pa, afmt, pg, gfmt, lay, n, h, w, int(down), *tail), 'score_frames_down')
    return scores


_REGION_WS = _Cache()  # (device, stream handle, h, w) -> workspace of one full refvsr_score_regions launch


def score_regions(outs, gts, rects):
    """{sum (a - b)^2, sum S} of B (result, ground truth) pairs of one 3 x h x w geometry over R <= REFVSR_SCORE_MAX_RECTS rectangles
    (y0, y1, x0, x1), half-open, computed on the device (refvsr_score_regions; S = the full SSIM map with the symmetric border): a
    torch.float64 [B, R, 2] tensor of raw sums on the current stream, no synchronisation.  Inputs as score_frames takes them.  One
    launch per REFVSR_SCORE_MAX_FRAMES pairs.  The FOV table: metrics.fov_table(sums of metrics.fov_rects(h, w), h, w) on the host."""
    outs, gts, h, w, afmt, gfmt, lay = _score_inputs(outs, gts, 'score_regions')
    rects = [tuple(int(v) for v in r) for r in rects]
    assert all(len(r) == 4 for r in rects), 'score_regions: rectangles are (y0, y1, x0, x1)'
    nr = len(rects)
    crects = (C.c_int * max(4 * nr, 1))(*[v for r in rects for v in r])
    st = _stream()
    dev = outs[0].device
    ws = _workspace(_REGION_WS, dev, st, h, w, lambda: hip.lib().refvsr_score_regions_workspace_bytes(hip.SCORE_MAX_FRAMES, h, w, hip.SCORE_MAX_RECTS),
                    'score_regions', _TOO_SMALL)
    sums = torch.empty((len(outs), nr, 2), dtype=torch.float64, device=dev)
    for s0, n in _chunks(len(outs), hip.SCORE_MAX_FRAMES):
        hip.check(hip.lib().refvsr_score_regions(_parr(outs[s0:s0 + n]), afmt, _parr(gts[s0:s0 + n]), gfmt, lay, n, h, w, crects, nr, _ptr(ws), ws.numel() * 8,
                                                 C.c_void_p(sums.data_ptr() + 16 * nr * s0), st), 'score_regions')
    return sums


def result_to_yuv420(frames, fmt='nv12', matrix='bt709', range='limited'):
    """Result frames -> Y'CbCr 4:2:0 on the device (refvsr_result_to_yuv420; the bits of yuv.rgb_to_yuv420): a [B, 3 h / 2, w] tensor,
    torch.uint8 ('nv12' | 'i420') or torch.uint16 ('p010' | 'i420p10'), frame b one dense buffer (yuv.planes gives its views), on the
    current stream, no synchronisation.  frames: a [B,3,h,w] tensor or B tensors [3,h,w], float32 / float16 / uint8 (what the output
    head stores), contiguous or channels-last (config.result_layout = 'hwc'), h and w even.  matrix: 'bt709' | 'bt601'; range:
    'limited' | 'full'.  One launch per REFVSR_YUV420_MAX_FRAMES frames."""
    if fmt not in yuv.FORMATS:
        yuv.check_format(fmt)
        raise ValueError('result_to_yuv420: %r is not a 4:2:0 format: ops.result_to_yuv takes it' % (fmt,))
    return _result_to_yuv('result_to_yuv420', frames, fmt, matrix, range, lambda ps, sfmt, pd, n, h, w, coef, st: hip.lib().refvsr_result_to_yuv420(
        ps, sfmt, pd, n, h, w, yuv.FORMAT_IDS[fmt], coef, st))


def result_to_yuv(frames, fmt='i422', matrix='bt709', range='limited', siting='centre'):
    """result_to_yuv420 for every format and siting (refvsr_result_to_yuv; the bits of yuv.rgb_to_yuv): fmt also 'i422' | 'i444' |
    'i422p10' | 'i444p10', a [B, 2 h, w] or [B, 3 h, w] tensor; siting 'centre' | 'left' (checked and ignored for 4:4:4).  A 4:2:0
    format with siting 'centre' gives result_to_yuv420's bits (the same kernel instance)."""
    samp, sit = yuv.SAMPLINGS[yuv.sampling_of(fmt)], yuv.SITINGS[yuv.check_siting(siting)]
    return _result_to_yuv('result_to_yuv', frames, fmt, matrix, range, lambda ps, sfmt, pd, n, h, w, coef, st: hip.lib().refvsr_result_to_yuv(
        ps, sfmt, pd, n, h, w, yuv.FORMAT_IDS[yuv.twin_of(fmt)], samp, sit, coef, st))


def _result_to_yuv(name, frames, fmt, matrix, range_, launch):
    """The body of result_to_yuv420 / result_to_yuv: the frames checked, the output [B] + yuv.frame_shape(h, w, fmt) allocated, one
    launch(src table, src format, dst table, n, h, w, coef9, stream) per REFVSR_YUV420_MAX_FRAMES frames."""
    coef = (C.c_double * 9)(*yuv.coefficients(fmt, matrix, range_))
    frames, h, w = _result_frames(name, frames, 'results')
    if h % 2 or w % 2:
        raise RuntimeError('%s: %s needs even h and w (got %d x %d)' % (name, '4:2:0' if fmt in yuv.FORMATS else fmt, h, w))
    sfmt = _result_format(name, frames, 'results')
    out = torch.empty((len(frames),) + yuv.frame_shape(h, w, fmt), dtype=torch.uint8 if yuv.depth_of(fmt) == 8 else torch.uint16, device=frames[0].device)
    st = _stream()
    for s0, n in _chunks(len(frames), hip.YUV420_MAX_FRAMES):
        hip.check(launch(_parr(frames[s0:s0 + n]), sfmt, _parr([out[s0 + i] for i in range(n)]), n, h, w, coef, st), name)
    return out


_RESIZE_TAPS = _Cache()  # (device, h, w, oh, ow) -> the device tap tables of one geometry (resize.aa_taps of both axes) and their widths


def _resize_taps(dev, h, w, oh, ow):
    """The cached device tables of resize_aa for one geometry: (lo_x, cnt_x, wx, lo_y, cnt_y, wy, maxcnt_x, maxcnt_y); built on the
    host by resize.aa_taps and uploaded once (the first call of a geometry copies; later calls launch only)."""
    from . import resize
    def build():
        (lx, cx, wx), (ly, cy, wy) = resize.aa_taps(w, ow), resize.aa_taps(h, oh)
        return tuple(torch.from_numpy(np.ascontiguousarray(a_)).to(dev) for a_ in (lx, cx, wx, ly, cy, wy)) + (wx.shape[1], wy.shape[1])
    return _RESIZE_TAPS.get_or_build((dev, h, w, oh, ow), build)


def resize_aa(frames, oh, ow, out='float32', clamp=True):
    """Antialiased bicubic resize on the device (refvsr_resize_aa; the bits of resize.resize_aa_model): a new contiguous [B,3,oh,ow]
    tensor, torch.float32 (clamp True: clamped to [0, 1] before its one rounding) or torch.uint8 (out = 'uint8': rint of 255 x the
    clamped value, half to even), on the current stream, no synchronisation.  frames: a [B,3,h,w] tensor or B tensors [3,h,w], float32 /
    float16 / uint8 (a byte means the float32 ingest_u8 gives it), contiguous or channels-last (config.result_layout = 'hwc'), dense,
    of one geometry.  h <= 8 oh and w <= 8 ow; up-scaling has no limit.  The filter is Keys' cubic, a = -0.5, stretched by the
    down-scale ratio and normalised: the 'BI' degradation, what made the dataset's LRx4 folders -- not the engine's A = -0.75 bicubic.
    One launch per REFVSR_RESIZE_MAX_FRAMES frames; the tap tables are cached per (h, w, oh, ow)."""
    from . import resize
    if out not in ('float32', 'uint8'):
        raise RuntimeError("resize_aa: out must be 'float32' or 'uint8' (got %r)" % (out,))
    frames, h, w = _result_frames('resize_aa', frames, 'frames')
    try:
        resize.check_sizes(h, oh, 'resize_aa')
        resize.check_sizes(w, ow, 'resize_aa')
        oh, ow = int(oh), int(ow)
    except (TypeError, ValueError) as e:
        raise RuntimeError(str(e) if isinstance(e, ValueError) else 'resize_aa: oh, ow must be integers (got %r, %r)' % (oh, ow))
    sfmt = _result_format('resize_aa', frames, 'frames')
    dev = frames[0].device
    lx, cx, wx, ly, cy, wy, mx, my = _resize_taps(dev, h, w, oh, ow)
    res = torch.empty((len(frames), 3, oh, ow), dtype=torch.float32 if out == 'float32' else torch.uint8, device=dev)
    dfmt = hip.RESULT_F32 if out == 'float32' else hip.RESULT_U8
    st = _stream()
    for s0, n in _chunks(len(frames), hip.RESIZE_MAX_FRAMES):
        hip.check(hip.lib().refvsr_resize_aa(_parr(frames[s0:s0 + n]), sfmt, _parr([res[s0 + i] for i in range(n)]), dfmt, n, h, w, oh, ow,
                                             _ptr(lx), _ptr(cx), _ptr(wx), _ptr(ly), _ptr(cy), _ptr(wy), mx, my, 1 if clamp else 0, st), 'resize_aa')
    return res


def yuv_window_kind(x, fmt):
    """('yuv', fmt) for a tensor whose trailing [3 h / 2, w] frames are dense 4:2:0 buffers of format `fmt` -- the sample type of the
    format (torch.uint8 | torch.uint16), at least 2-D, contiguous, even h and w -- else None.  A 4:2:2 format: [2 h, w] frames, a
    4:4:4 one: [3 h, w]."""
    dt = torch.uint8 if yuv.depth_of(fmt) == 8 else torch.uint16
    if x.dtype != dt or x.dim() < 2 or not x.is_contiguous():
        return None
    r, w = x.shape[-2:]
    unit = _YUV_ROW_UNIT[yuv.sampling_of(fmt)]              # (3 h / 2 rows with even h: a multiple of 3; 2 h: of 4; 3 h: of 6)
    if r < unit or r % unit or w < 2 or w % 2:
        return None
    return ('yuv', fmt)


_YUV_ROW_UNIT = {'420': 3, '422': 4, '444': 6}               # the rows of a frame of two luma rows


def yuv_geometry(x, fmt=None):
    """(h, w) of a tensor of [3 h / 2, w] frames; with a format, of that format's frames ([2 h, w] for 4:2:2, [3 h, w] for 4:4:4)."""
    return 2 * x.shape[-2] // _YUV_ROW_UNIT[yuv.sampling_of(fmt) if fmt else '420'], x.shape[-1]


def yuv420_ingest(pairs, fmt='nv12', matrix='bt709', range='limited', chroma='bilinear'):
    """pairs: [(src [3 h / 2, w] uint8 | uint16 by `fmt`, one dense frame at any address that is a multiple of its sample size, dst
    float32 [3,h,w] contiguous)] of one h x w: dst = the bits of yuv.yuv420_to_rgb (refvsr_yuv420_to_rgb) -- the twin of ingest_u8.
    One launch per REFVSR_YUV420_IN_MAX_FRAMES frames, on the current stream."""
    _yuv_ingest('yuv420_to_rgb', 'yuv420_ingest: dense %s frames [3h/2, w] of one size' % fmt, pairs, fmt, matrix, range, chroma,
                lambda ps, pd, n, h, w, mode, coef, st: hip.lib().refvsr_yuv420_to_rgb(ps, pd, n, h, w, yuv.FORMAT_IDS[fmt], mode, coef, st))


def yuv_ingest(pairs, fmt='i422', matrix='bt709', range='limited', chroma='bilinear', siting='centre'):
    """yuv420_ingest for every format and siting (refvsr_yuv_to_rgb; the bits of yuv.yuv_to_rgb): src frames yuv.frame_shape(h, w, fmt),
    siting 'centre' | 'left' (checked and ignored for 4:4:4).  A 4:2:0 format with siting 'centre': yuv420_ingest's kernel and bits."""
    fid, samp, sit = yuv.FORMAT_IDS[yuv.twin_of(fmt)], yuv.SAMPLINGS[yuv.sampling_of(fmt)], yuv.SITINGS[yuv.check_siting(siting)]
    _yuv_ingest('yuv_to_rgb', 'yuv_ingest: dense %s frames of one size' % fmt, pairs, fmt, matrix, range, chroma,
                lambda ps, pd, n, h, w, mode, coef, st: hip.lib().refvsr_yuv_to_rgb(ps, pd, n, h, w, fid, samp, sit, mode, coef, st))


def _yuv_ingest(name, what, pairs, fmt, matrix, range, chroma, launch):
    """The body of yuv420_ingest / yuv_ingest: nothing for no pairs; else the coefficients and the chroma mode, the pairs checked
    (`what`), one launch(src table, dst table, n, h, w, mode, coef9, stream) of refvsr_<name> per REFVSR_YUV420_IN_MAX_FRAMES frames."""
    if not pairs:
        return
    coef = (C.c_double * 9)(*yuv.decode_coefficients(fmt, matrix, range))
    mode = yuv.CHROMA_MODES[yuv.check_chroma(chroma)]
    _decode_frames(pairs, name, what, lambda src, h, w: yuv_window_kind(src, fmt) is not None and tuple(src.shape) == yuv.frame_shape(h, w, fmt),
                   hip.YUV420_IN_MAX_FRAMES, lambda ps, pd, n, h, w: launch(ps, pd, n, h, w, mode, coef, _stream()))


def yuv_decode(pairs, params):
    """pairs decoded under config.input_yuv resolved (yuv.resolve_input): the four parameters of a centre-sited 4:2:0 format are
    yuv420_ingest's, everything else -- a 4:2:2 / 4:4:4 format, a fifth parameter 'left' -- yuv_ingest's."""
    (yuv420_ingest if params[0] in yuv.FORMATS and len(params) == 4 else yuv_ingest)(pairs, *params)


def result_yuv(frames, params, siting='centre'):
    """frames under config.result_yuv resolved (yuv.resolve) and the engine's siting: a centre-sited 4:2:0 format is
    result_to_yuv420's, everything else result_to_yuv's."""
    siting = yuv.effective_siting(params[0], siting)
    return result_to_yuv420(frames, *params) if params[0] in yuv.FORMATS and siting == 'centre' else result_to_yuv(frames, *(params + (siting,)))


def yuv_to_frames(x, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear', siting='centre'):
    """yuv420_to_frames for every format and siting: [..., rows, w] frames, rows = yuv.frame_shape(h, w, fmt)[0], -> a new contiguous
    float32 [..., 3, h, w] tensor, the bits of yuv.yuv_to_rgb, through refvsr_yuv_to_rgb."""
    yuv.check_siting(siting)
    return _yuv_to_frames('yuv_to_frames', x, h, w, fmt, lambda pairs: yuv_ingest(pairs, fmt, matrix, range, chroma, siting))


def yuv420_to_frames(x, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear'):
    """[..., 3 h / 2, w] 4:2:0 frames (uint8 'nv12' | 'i420', uint16 'p010' | 'i420p10'; other strides and storage that is unaligned
    for the sample size are copied first) -> a new contiguous float32 [..., 3, h, w] tensor, the bits of yuv.yuv420_to_rgb, frame by
    frame through refvsr_yuv420_to_rgb (as ingest_frames)."""
    return _yuv_to_frames('yuv420_to_frames', x, h, w, fmt, lambda pairs: yuv420_ingest(pairs, fmt, matrix, range, chroma))


def _yuv_to_frames(name, x, h, w, fmt, ingest):
    """The body of yuv420_to_frames / yuv_to_frames: x checked against the format's frames at h x w, then _frames_of with `ingest`."""
    dt, rows = torch.uint8 if yuv.depth_of(fmt) == 8 else torch.uint16, yuv.frame_shape(h, w, fmt)[0]
    if not (x.is_cuda and x.dtype == dt and x.dim() >= 2 and tuple(x.shape[-2:]) == (rows, w)):
        raise RuntimeError('%s: cuda %s [..., %d, %d] frames for %s at %d x %d (got %s %s %s)'
                           % (name, dt, rows, w, fmt, h, w, x.device.type, x.dtype, tuple(x.shape)))
    return _frames_of(x, 2, torch.Tensor.is_contiguous, dt.itemsize, h, w, ingest)


_JPEG_TABLES = _Cache()  # (device, quality, fmt) -> the device tables of refvsr_jpeg_encode: (qtables, dct, huffman LUT)


def _jpeg_tables(dev, quality, fmt):
    """The cached device tables of jpeg_encode for one (quality, fmt): the float64 quantisation tables [2, 64], the DCT matrix
    jpeg.dct_table() and jpeg.huffman_lut(), made on the host and uploaded once."""
    from . import jpeg
    def build():
        q = np.stack(jpeg.quant_tables(quality)).astype(np.float64)
        return tuple(torch.from_numpy(np.ascontiguousarray(a_)).to(dev) for a_ in (q, jpeg.dct_table(), jpeg.huffman_lut().view(np.int32)))
    return _JPEG_TABLES.get_or_build((dev, quality, fmt), build)


def _jpeg_frames(name, yuv_frames, h, w, fmt, quality, restart):
    """The arguments of jpeg_encode / jpeg_encode_device checked, in the order format, quality, restart, size, dtype, shape, device:
    (the frames as a list of dense [rows, w] tensors, quality, restart).  Names and numbers are ValueErrors, tensors RuntimeErrors, as
    in result_to_yuv."""
    from . import jpeg
    jpeg.check_format(fmt)
    quality, restart = jpeg.check_quality(quality), jpeg.check_restart(restart)
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, int) or not isinstance(w, int):
        raise ValueError('%s: h and w must be integers (got %r, %r)' % (name, h, w))
    jpeg.check_size(h, w)
    shape = yuv.frame_shape(h, w, fmt)
    if isinstance(yuv_frames, torch.Tensor):
        if yuv_frames.dim() < 2 or tuple(yuv_frames.shape[-2:]) != shape:
            raise RuntimeError('%s: %s frames at %d x %d are [.., %d, %d] (got %s)' % (name, fmt, h, w, shape[0], shape[1], tuple(yuv_frames.shape)))
        frames = [yuv_frames] if yuv_frames.dim() == 2 else list(yuv_frames.flatten(0, -3).unbind(0))
    else:
        frames = list(yuv_frames)
    if not frames:
        raise RuntimeError('%s: at least one frame' % name)
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8:
            raise RuntimeError('%s: frames are torch.uint8 (8-bit %s; got %s)' % (name, fmt, getattr(f, 'dtype', type(f).__name__)))
        if tuple(f.shape) != shape or not f.is_contiguous():
            raise RuntimeError('%s: every frame is one dense [%d, %d] buffer (%s at %d x %d; got %s, strides %s)'
                               % (name, shape[0], shape[1], fmt, h, w, tuple(f.shape), tuple(f.stride())))
    for f in frames:
        if not f.is_cuda or f.device != frames[0].device:
            raise RuntimeError('%s: frames must lie on one GPU (got %s)' % (name, f.device))
    return frames, quality, restart


def jpeg_encode_device(yuv_frames, h, w, fmt, quality=90, restart=None):
    """The entropy-coded data of B frames, made on the device (refvsr_jpeg_encode; the bytes of jpeg.entropy_data), for callers that
    issue the copies themselves: (dst, offsets, sizes) -- dst a torch.uint8 [B * bound] tensor, bound = refvsr_jpeg_capacity, offsets
    and sizes torch.int64 [B] device tensors: frame i's data is dst[offsets[i] : offsets[i] + sizes[i]]; jpeg.assemble(jpeg.header(..),
    data) makes the file.  On the current stream, no synchronisation.  yuv_frames: the 'yuv' frames of a call or of result_to_yuv(frames,
    'i420' | 'i444', 'bt601', 'full', 'centre'): a [.., 3 h / 2, w] | [.., 3 h, w] torch.uint8 tensor or a list of such frames, each one
    dense buffer at any address.  One launch set per REFVSR_JPEG_MAX_FRAMES frames (each set's frames lie back to back from the set's
    first slot on)."""
    frames, quality, restart = _jpeg_frames('jpeg_encode_device', yuv_frames, h, w, fmt, quality, restart)
    dev = frames[0].device
    lib = hip.lib()
    samp = yuv.SAMPLINGS[yuv.sampling_of(fmt)]
    bound = lib.refvsr_jpeg_capacity(h, w, samp, restart)
    if bound == 0:
        raise RuntimeError('jpeg_encode_device: frames of %d x %d hold too many blocks' % (h, w))
    qt, dct, lut = _jpeg_tables(dev, quality, fmt)
    n = len(frames)
    dst = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    meta = torch.empty((2, n), dtype=torch.int64, device=dev)
    st = _stream()
    for s0, k in _chunks(n, hip.JPEG_MAX_FRAMES):
        wsb = lib.refvsr_jpeg_workspace_bytes(k, h, w, samp, restart)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        hip.check(lib.refvsr_jpeg_encode(_parr(frames[s0:s0 + k]), k, h, w, samp, _ptr(qt), _ptr(dct), _ptr(lut), restart,
                                         C.c_void_p(dst.data_ptr() + s0 * bound), k * bound, C.c_void_p(meta.data_ptr() + 8 * (n + s0)),
                                         C.c_void_p(meta.data_ptr() + 8 * s0), _ptr(ws), wsb, st), 'jpeg_encode')
        if s0:
            meta[0, s0:s0 + k] += s0 * bound                            # (a set's offsets count from its own first slot)
    return dst, meta[0], meta[1]


def jpeg_encode(yuv_frames, h, w, fmt, quality=90, restart=None):
    """B frames -> B complete JFIF files (bytes; the bytes of jpeg.encode_model): jpeg_encode_device, then the sizes are read -- the one
    synchronisation -- and exactly the compressed bytes are copied to the host, where header and EOI are put around each frame's data.
    quality: 1..100; restart: MCUs per restart interval, None: jpeg.DEFAULT_RESTART."""
    from . import jpeg
    frames, quality, restart = _jpeg_frames('jpeg_encode', yuv_frames, h, w, fmt, quality, restart)
    dst, offsets, sizes = jpeg_encode_device(frames, h, w, fmt, quality, restart)
    off, size = offsets.cpu().tolist(), sizes.cpu().tolist()
    head = jpeg.header(h, w, fmt, quality, restart)
    out = []
    for s0 in range(0, len(frames), hip.JPEG_MAX_FRAMES):               # a launch set's frames lie back to back: one copy per set
        s1 = min(s0 + hip.JPEG_MAX_FRAMES, len(frames))
        data = dst[off[s0]:off[s1 - 1] + size[s1 - 1]].cpu().numpy().tobytes()
        out.extend(jpeg.assemble(head, data[off[i] - off[s0]:off[i] - off[s0] + size[i]]) for i in range(s0, s1))
    return out


_SAD_WS = _Cache()    # (device, stream handle, h, w) -> workspace of one full refvsr_luma_sad call


def luma_sad(frames_a, frames_b, h, w, fmt):
    """The sums of absolute luma differences of B pairs of 4:2:0 frames of one h x w, computed on the device (refvsr_luma_sad; the
    integers of yuv.luma_sad): a torch.int64 [B] tensor on the current stream, no synchronisation.  frames_a, frames_b: a
    [B, 3 h / 2, w] tensor or B tensors [3 h / 2, w] each, uint8 ('nv12' | 'i420') or uint16 ('p010' | 'i420p10'), dense frames at
    any multiple of their sample size (views into a [t, 3 h / 2, w] window included); the same frame on both sides gives 0.  One call
    (two launches) per REFVSR_SCENE_MAX_PAIRS pairs.  A 4:2:2 or 4:4:4 format: [2 h, w] or [3 h, w] frames, read under the format id
    of the 4:2:0 twin -- the luma plane is the first h w samples of every layout."""
    fa, fb = list(frames_a), list(frames_b)
    if not fa or len(fa) != len(fb):
        raise RuntimeError('luma_sad: as many frames on both sides, at least one (got %d and %d)' % (len(fa), len(fb)))
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise RuntimeError('luma_sad: 4:2:0 needs even h and w (got %d x %d)' % (h, w))
    dev = fa[0].device
    shape = yuv.frame_shape(h, w, fmt)
    for f in fa + fb:
        if not (f.is_cuda and f.device == dev and yuv_window_kind(f, fmt) is not None and tuple(f.shape) == shape):
            raise RuntimeError('luma_sad: dense cuda %s frames [%d, %d] of one GPU (got %s %s %s)'
                               % (fmt, shape[0], w, f.device.type, f.dtype, tuple(f.shape)))
    st = _stream()
    ws = _workspace(_SAD_WS, dev, st, h, w, lambda: hip.lib().refvsr_luma_sad_workspace_bytes(hip.SCENE_MAX_PAIRS, h, w), 'luma_sad',
                    'frames must hold at most 2^29 pixels', 4)
    sad = torch.empty(len(fa), dtype=torch.int64, device=dev)
    for s0, n in _chunks(len(fa), hip.SCENE_MAX_PAIRS):
        hip.check(hip.lib().refvsr_luma_sad(_parr(fa[s0:s0 + n]), _parr(fb[s0:s0 + n]), n, h, w, yuv.FORMAT_IDS[yuv.twin_of(fmt)], _ptr(ws), ws.numel() * 4,
                                            C.c_void_p(sad.data_ptr() + 8 * s0), st), 'luma_sad')
    return sad


_COLORMAP_WS = _Cache()  # (device, stream handle, h, w) -> workspace of one full refvsr_conf_colormap launch


def colormap_table():
    """The library's colour table (host query, no device work): 256 [r, g, b] byte triples, matplotlib's inferno as the reference's
    images hold it (csrc/colormap_table.h)."""
    t = (C.c_ubyte * 768)()
    hip.check(hip.lib().refvsr_colormap_table(t), 'colormap_table')
    return [list(t[3 * i:3 * i + 3]) for i in range(256)]


def conf_colormap(maps):
    """The confidence-map images of evaluation/eval_quan_conf_map.py:64-100,148-165, computed on the device (refvsr_conf_colormap):
    maps: cuda float32 tensors of one [.., h, w] geometry with numel == h * w (e.g. the [1, h, w] or [1, 1, h, w] maps of 'eval_vis'),
    contiguous.  Returns one uint8 [h, w, 3] tensor (RGB) per map -- the map min/max-normalised and coloured with matplotlib's
    inferno, bit for bit the reference's bytes (metrics.conf_colormap_model) -- on the current stream, no synchronisation.  One launch
    per REFVSR_COLORMAP_MAX_MAPS maps."""
    maps = list(maps)
    assert maps, 'conf_colormap: no maps'
    h, w = maps[0].shape[-2:]
    for m in maps:
        assert m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and m.dim() >= 2, \
            'conf_colormap: contiguous cuda float32 maps, got %s %s' % (m.dtype, tuple(m.shape))
        if tuple(m.shape[-2:]) != (h, w) or m.numel() != h * w:
            raise RuntimeError('conf_colormap: maps must be single [.., %d, %d] maps of one geometry (got %s)' % (h, w, tuple(m.shape)))
    st = _stream()
    dev = maps[0].device
    ws = _workspace(_COLORMAP_WS, dev, st, h, w, lambda: hip.lib().refvsr_conf_colormap_workspace_bytes(hip.COLORMAP_MAX_MAPS, h, w),
                    'conf_colormap', 'maps must hold 1 .. 2^31 - 1 samples', 4)
    outs = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for _ in maps]
    for s0, n in _chunks(len(maps), hip.COLORMAP_MAX_MAPS):
        pm, po = _parr(maps[s0:s0 + n]), _parr(outs[s0:s0 + n])
        hip.check(hip.lib().refvsr_conf_colormap(pm, n, h, w, po, _ptr(ws), ws.numel() * 4, st), 'conf_colormap')
    return outs


class FingerprintTable(object):
    """The device chunk table of refvsr_param_fingerprint for one list of tensors (fingerprint.chunk_entries), with one workspace per
    stream that used it.  Valid while the tensors keep their storage: `pointers` is what the owner compares (Network rebuilds the
    table when the tuple of data_ptr()s changes).  The tensors are referenced, so their storage cannot be reused under the table."""

    def __init__(self, tensors):
        tensors = list(tensors)
        if not tensors:
            raise ValueError('param_fingerprint: empty tensor list')
        dev = tensors[0].device
        for t in tensors:
            if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError('param_fingerprint: contiguous float32 tensors of one GPU (got %s, %s, contiguous=%s)'
                                   % (t.dtype, t.device, t.is_contiguous()))
        self.tensors = tensors
        self.pointers = tuple(t.data_ptr() for t in tensors)
        ent = fingerprint.chunk_entries(self.pointers, [t.numel() for t in tensors], hip.FINGERPRINT_CHUNK_WORDS)
        self.nchunks = len(ent)
        self.device = dev
        self.chunks = torch.from_numpy(ent.view(np.int64).reshape(-1, 2).copy()).to(dev)
        self._ws = _Cache()

    def workspace(self, st):
        return self._ws.get_or_build(st.value, lambda: torch.empty(hip.lib().refvsr_param_fingerprint_workspace_bytes(self.nchunks) // 8 + 1,
                                                                   dtype=torch.int64, device=self.device))


def param_fingerprint(tensors, out=None):
    """The 64-bit fingerprint of a table of contiguous cuda float32 tensors (refvsr_param_fingerprint; fingerprint.
    param_fingerprint_model restates it): F = sum of mix64((g << 32) | word) over all 32-bit words, g the word's index over the
    concatenated table -- one changed bit changes F.  tensors: a list of tensors (the chunk table is built and uploaded for the call)
    or an ops.FingerprintTable (built once).  Returns `out`, a device int64 [1] (the 64 bits, read as signed), written on the current
    stream with no synchronisation."""
    tab = tensors if isinstance(tensors, FingerprintTable) else FingerprintTable(tensors)
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=tab.device)
    assert out.is_cuda and out.device == tab.device and out.dtype == torch.int64 and out.numel() == 1
    st = _stream()
    ws = tab.workspace(st)
    hip.check(hip.lib().refvsr_param_fingerprint(_ptr(tab.chunks), tab.nchunks, _ptr(ws), ws.numel() * 8, _ptr(out), st), 'param_fingerprint')
    return out


def warp_nhwc16(x, flow):
    _nhwc(x)
    _planar(flow, 2)
    hin, win, cs = x.shape
    hf, wf = flow.shape[1:]
    out = torch.empty((hf, wf, cs), dtype=torch.float16, device=x.device)
    hip.check(hip.lib().refvsr_warp_nhwc16(_ptr(x), hin, win, cs, _ptr(flow), hf, wf, _ptr(out), _stream()), 'warp_nhwc16')
    return out


def warp_nhwc16_up2(x, flow_lr):
    """warp_nhwc16(x, flow_up2(flow_lr)) in one launch (the 2x flow map is evaluated per pixel, never written)."""
    _nhwc(x)
    _planar(flow_lr, 2)
    hin, win, cs = x.shape
    hl, wl = flow_lr.shape[1:]
    out = torch.empty((2 * hl, 2 * wl, cs), dtype=torch.float16, device=x.device)
    hip.check(hip.lib().refvsr_warp_nhwc16_up2(_ptr(x), hin, win, cs, _ptr(flow_lr), hl, wl, _ptr(out), _stream()), 'warp_nhwc16_up2')
    return out


def warp_planar(x, flow):
    _planar(x)
    _planar(flow, 2)
    c, hin, win = x.shape
    hf, wf = flow.shape[1:]
    out = torch.empty((c, hf, wf), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().refvsr_warp_planar(_ptr(x), c, hin, win, _ptr(flow), hf, wf, _ptr(out), _stream()), 'warp_planar')
    return out


def spynet_level_input(ref, supp, flow_prev):
    _planar(ref, 3)
    _planar(supp, 3)
    h, w = ref.shape[1:]
    if flow_prev is not None:
        _planar(flow_prev, 2)
        assert tuple(flow_prev.shape[1:]) == (h // 2, w // 2)
    out8 = torch.empty((h, w, 8), dtype=torch.float16, device=ref.device)
    fup = torch.empty((2, h, w), dtype=torch.float32, device=ref.device)
    hip.check(hip.lib().refvsr_spynet_level_input(_ptr(ref), _ptr(supp), _ptr(flow_prev), h, w, _ptr(out8), _ptr(fup),
                                                  _stream()), 'spynet_level_input')
    return out8, fup


def spynet_level_input_batch(refs, supps, flow_prev):
    """refvsr_spynet_level_input_batch: B independent (ref, supp) pairs of one pyramid level in one launch.  refs / supps:
    lists of B planar fp32 [3,h,w] tensors; flow_prev [B,2,h/2,w/2] or None.  Returns (x [B,h,w,8] fp16, flow_up [B,2,h,w])."""
    B = len(refs)
    assert 1 <= B <= 8 and len(supps) == B
    for t_ in list(refs) + list(supps):
        _planar(t_, 3)
    h, w = refs[0].shape[1:]
    if flow_prev is not None:
        assert flow_prev.is_cuda and flow_prev.dtype == torch.float32 and flow_prev.is_contiguous() and \
            tuple(flow_prev.shape) == (B, 2, h // 2, w // 2)
    out8 = torch.empty((B, h, w, 8), dtype=torch.float16, device=refs[0].device)
    fup = torch.empty((B, 2, h, w), dtype=torch.float32, device=refs[0].device)
    pr = (C.c_void_p * B)(*[t_.data_ptr() for t_ in refs])
    ps = (C.c_void_p * B)(*[t_.data_ptr() for t_ in supps])
    hip.check(hip.lib().refvsr_spynet_level_input_batch(pr, ps, B, _ptr(flow_prev), h, w, _ptr(out8), _ptr(fup), _stream()),
              'spynet_level_input_batch')
    return out8, fup


def set_match_patches_kernel(mode):
    """A/B knob of refvsr_match_patches (process-wide): 0 = one pixel per thread with global gathers, 1 = LDS tile (default)."""
    hip.check(hip.lib().refvsr_set_match_patches_kernel(int(mode)), 'set_match_patches_kernel')


def match_patches(feat, row_pad, want_lo=False):
    """feat planar [16,h,w] -> (rows fp16 [pad(h*w), KP] zero padded, inv_norm fp32 [h*w][, rows_lo fp16 like rows: the
    low halves of the hi + lo operand split, scaled by 2^11 -- the exact search's second operand])."""
    _planar(feat, 16)
    h, w = feat.shape[1:]
    n = h * w
    # the kernel writes every slot of the n valid rows (incl. the zero pad of each row); only the pad ROWS need clearing
    rows = torch.empty((_round_up(n, row_pad), hip.MATCH_KP), dtype=torch.float16, device=feat.device)
    inv = torch.empty((n,), dtype=torch.float32, device=feat.device)
    lo = torch.empty_like(rows) if want_lo else None
    if rows.shape[0] > n:
        rows[n:].zero_()
        if lo is not None:
            lo[n:].zero_()
    hip.check(hip.lib().refvsr_match_patches(_ptr(feat), h, w, _ptr(rows), _ptr(inv), _ptr(lo), _stream()), 'match_patches')
    return (rows, inv, lo) if want_lo else (rows, inv)


def match_top2(ref_rows, n_ref, lr_rows, n_lr, row_splits=1):
    assert ref_rows.shape[0] % hip.MATCH_ROWCHUNK == 0 and lr_rows.shape[0] % hip.MATCH_COLBLOCK == 0
    assert ref_rows.shape[0] >= n_ref and lr_rows.shape[0] >= n_lr
    ci = torch.empty((n_lr, 2 * row_splits), dtype=torch.int32, device=ref_rows.device)
    cv = torch.empty((n_lr, 2 * row_splits), dtype=torch.float32, device=ref_rows.device)
    hip.check(hip.lib().refvsr_match_top2(_ptr(ref_rows), n_ref, _ptr(lr_rows), n_lr, row_splits, _ptr(ci), _ptr(cv),
                                          _stream()), 'match_top2')
    return ci, cv


# fp16-GEMM scores of rows outside the candidate list are trusted to this margin; columns whose exact maximum does not
# clear the runner-up's fp16 score by it are searched exhaustively at fp32 accuracy (refvsr_match_exact).  The fp16 operand
# rounding perturbs a correlation by ~3e-5 (measured), bounded by 2^-10 = 9.8e-4 in the worst case.
MATCH_EXACT_MARGIN = 2.5e-4


def match_refine(lr_feat, ref_feat, inv_lr, inv_ref, cand, cand_val=None, margin=None, lr_split=None, ref_split=None):
    """Exact re-rank of the candidates; with cand_val / margin / lr_split = (lr_rows, lr_rows_lo) / ref_split = (ref_rows, ref_rows_lo) also the exhaustive
    search of the columns the fp16 GEMM cannot decide.  margin = inf searches EVERY column exhaustively (test aid).
    lr_rows_lo = None: the low halves of the flagged columns' rows -- the only ones the search reads -- are written here, after the
    flagging, by refvsr_match_lo_rows (the reference rows' low halves are streamed whole and must be complete).
    Returns (conf, idx) or (conf, idx, flagged int32 [1 + n], [0] = count) when flagging is on."""
    _planar(lr_feat, 16)
    _planar(ref_feat, 16)
    h, w = lr_feat.shape[1:]
    hr, wr = ref_feat.shape[1:]
    assert cand.dtype == torch.int32 and cand.shape[0] == h * w and cand.is_contiguous()
    conf = torch.empty((h * w,), dtype=torch.float32, device=lr_feat.device)
    idx = torch.empty((h * w,), dtype=torch.int32, device=lr_feat.device)
    if margin is None:
        hip.check(hip.lib().refvsr_match_refine(_ptr(lr_feat), h, w, _ptr(ref_feat), hr, wr, _ptr(inv_lr), _ptr(inv_ref),
                                                _ptr(cand), None, cand.shape[1], 0.0, None, _ptr(conf), _ptr(idx), _stream()),
                  'match_refine')
        return conf, idx
    assert cand_val is not None and ref_split is not None and lr_split is not None
    assert cand_val.shape == cand.shape and cand_val.is_contiguous()
    (lr_rows, lr_lo), (ref_rows, ref_lo) = lr_split, ref_split
    sparse_lo = lr_lo is None
    if sparse_lo:
        lr_lo = torch.empty_like(lr_rows)
    for r, n_, pad in ((lr_rows, h * w, 1), (lr_lo, h * w, 1), (ref_rows, hr * wr, hip.MATCH_ROWCHUNK), (ref_lo, hr * wr, hip.MATCH_ROWCHUNK)):
        assert r.dtype == torch.float16 and r.is_contiguous() and r.shape[1] == hip.MATCH_KP
        assert r.shape[0] >= n_ and r.shape[0] % pad == 0
    # one zeroed scratch allocation: [flag count + list (int32 1 + n, padded to 8 bytes)] [merge keys uint64 n]
    n = h * w
    fl_words = (n + 2) // 2 * 2
    scratch = torch.zeros(fl_words + 2 * n, dtype=torch.int32, device=lr_feat.device)
    flagged, keys = scratch[:n + 1], scratch[fl_words:]
    hip.check(hip.lib().refvsr_match_refine(_ptr(lr_feat), h, w, _ptr(ref_feat), hr, wr, _ptr(inv_lr), _ptr(inv_ref),
                                            _ptr(cand), _ptr(cand_val), cand.shape[1], float(margin), _ptr(flagged), _ptr(conf),
                                            _ptr(idx), _stream()), 'match_refine')
    if sparse_lo:
        hip.check(hip.lib().refvsr_match_lo_rows(_ptr(lr_feat), h, w, _ptr(inv_lr), _ptr(flagged), _ptr(lr_lo), _stream()), 'match_lo_rows')
    hip.check(hip.lib().refvsr_match_exact(_ptr(lr_feat), h, w, _ptr(ref_feat), hr, wr, _ptr(lr_rows), _ptr(lr_lo), _ptr(ref_rows), _ptr(ref_lo),
                                           _ptr(inv_lr), _ptr(inv_ref), _ptr(flagged), _ptr(keys), _ptr(conf), _ptr(idx),
                                           _stream()), 'match_exact')
    return conf, idx, flagged


def match_naive(lr_feat, ref_feat):
    _planar(lr_feat, 16)
    _planar(ref_feat, 16)
    h, w = lr_feat.shape[1:]
    hr, wr = ref_feat.shape[1:]
    conf = torch.empty((h * w,), dtype=torch.float32, device=lr_feat.device)
    idx = torch.empty((h * w,), dtype=torch.int32, device=lr_feat.device)
    hip.check(hip.lib().refvsr_match_naive(_ptr(lr_feat), h, w, _ptr(ref_feat), hr, wr, _ptr(conf), _ptr(idx),
                                           _stream()), 'match_naive')
    return conf, idx


def block_gather_nhwc16(value, idx, gh, gw, s):
    _nhwc(value)
    hv, wv, cs = value.shape
    assert idx.dtype == torch.int32 and idx.numel() == gh * gw and idx.is_contiguous()
    out = torch.empty((gh * s, gw * s, cs), dtype=torch.float16, device=value.device)
    hip.check(hip.lib().refvsr_block_gather_nhwc16(_ptr(value), hv, wv, cs, _ptr(idx), gh, gw, s, _ptr(out), _stream()),
              'block_gather_nhwc16')
    return out


def block_gather_rgb(value, idx, gh, gw, s, planar=False):
    """nhwc16 [gh*s, gw*s, 8] (3 valid channels), or with planar=True an exact planar fp32 copy [3, gh*s, gw*s]."""
    _planar(value, 3)
    hv, wv = value.shape[1:]
    assert idx.dtype == torch.int32 and idx.numel() == gh * gw and idx.is_contiguous()
    if planar:
        out = torch.empty((3, gh * s, gw * s), dtype=torch.float32, device=value.device)
        hip.check(hip.lib().refvsr_block_gather_rgb(_ptr(value), hv, wv, _ptr(idx), gh, gw, s, None, _ptr(out), _stream()),
                  'block_gather_rgb')
        return out
    out = torch.empty((gh * s, gw * s, 8), dtype=torch.float16, device=value.device)
    hip.check(hip.lib().refvsr_block_gather_rgb(_ptr(value), hv, wv, _ptr(idx), gh, gw, s, _ptr(out), None, _stream()),
              'block_gather_rgb')
    return out


def aligned_sample(x, affine, ks):
    _nhwc(x)
    _planar(affine, 3)
    h, w = affine.shape[1:]
    assert tuple(x.shape[:2]) == (h * ks, w * ks)
    out = torch.empty_like(x)
    hip.check(hip.lib().refvsr_aligned_sample(_ptr(x), h, w, ks, x.shape[2], _ptr(affine), _ptr(out), _stream()),
              'aligned_sample')
    return out


# ---- multi-map launches (ABI 11): B maps of one geometry behind one launch per layer ---------------------------------------
# Inputs are LISTS of B tensors (slices of a batched tensor or separately allocated per-frame maps); outputs are ONE tensor with a
# leading batch axis whose slices out[b] are the maps.  Map b of every call == the single-map op on map b, bit for bit.
def _parr(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def multimap_ok(B):
    return 2 <= B <= hip.MAX_MAPS


def _maps(ts, stack):
    """Result of a map-by-map fallback: one [B, ...] tensor like the multi-map launches return (stack: one more copy per map), or
    the list of the B maps as they are (the engine only ever indexes / iterates the result)."""
    return torch.stack(ts, 0) if stack else ts


def conv_b(cw, src0s, src1s=None, act=1.0, muls=None, ress=None, post=1.0, stack=True):
    """refvsr_conv24_batch / refvsr_conv_shuffle2_batch: conv() over B maps (24 output channels, 3x3, or the C = 24 pixel-shuffle
    conv).  Shapes without a multi-map kernel run map by map (same results; stack=False: returned as a list, no copy)."""
    B = len(src0s)
    if B == 1:                                       # the single-map op, before anything is spent on the list
        return _maps([conv(cw, src0s[0], None if src1s is None else src1s[0], act=act, mul=None if muls is None else muls[0],
                           res=None if ress is None else ress[0], post=post)], stack)
    h, w, c0 = src0s[0].shape
    c1 = src1s[0].shape[2] if src1s is not None else 0
    for l_ in (src0s, src1s, muls, ress):
        if l_ is not None:
            assert len(l_) == B
            for t_ in l_:
                _nhwc(t_)
                assert tuple(t_.shape[:2]) == (h, w)
    dev = src0s[0].device
    # (conv_b has no stride / pad / planar options: what conv() makes of their defaults)
    entry = _conv_route(cw, c0, None if src1s is None else c1, None if muls is None else muls[0], None if ress is None else ress[0], h, w,
                        1, cw.ksize // 2, False, act, post, B)
    if entry == 'conv_shuffle2_batch':
        out = torch.empty((B, 2 * h, 2 * w, c0), dtype=torch.float16, device=dev)
        hip.check(_c24(cw, 'refvsr_conv_shuffle2_batch')(_parr(src0s), B, c0, h, w, _ptr(cw.blob24), act, _parr(list(out)), _stream()),
                  'conv_shuffle2_batch')
        return out
    if entry == 'conv24_batch':
        out = torch.empty((B, h, w, 24), dtype=torch.float16, device=dev)
        hip.check(_c24(cw, 'refvsr_conv24_batch')(_parr(src0s), c0, _parr(src1s) if src1s is not None else None, c1, B, h, w, _ptr(cw.blob24),
                                                act, _parr(muls) if muls is not None else None, _parr(ress) if ress is not None else None,
                                                post, _parr(list(out)), _stream()), 'conv24_batch')
        return out
    return _maps([conv(cw, src0s[b], None if src1s is None else src1s[b], act=act, mul=None if muls is None else muls[b],
                       res=None if ress is None else ress[b], post=post) for b in range(B)], stack)


def _rb_chain_b(c, single, chain, xs, act, stack):
    B = len(xs)
    if not multimap_ok(B):
        return _maps([single(chain, x, act) for x in xs], stack)
    return _rb_chain(c, chain, xs, act, B)


def resblock24_chain_b(chain, xs, act, stack=True):
    """refvsr_resblock24_chain_batch: chain.n fused 24-channel blocks over B maps, one launch per block."""
    return _rb_chain_b(24, resblock24_chain, chain, xs, act, stack)


def resblock48_chain_b(chain, xs, act, stack=True):
    """refvsr_resblock48_chain_batch (ABI 12): chain.n fused 48-channel blocks over B maps, one launch per block."""
    return _rb_chain_b(48, resblock48_chain, chain, xs, act, stack)


def conf_alpha_b(conf_as, conf_bs, up, w0, b0, cw, slope0=0.2, slope1=0.2, want_max=False, stack=True):
    """refvsr_conf_alpha_batch: conf_alpha() over B pairs of confidence maps (24 output channels)."""
    B = len(conf_as)
    assert len(conf_bs) == B
    if not (multimap_ok(B) and cw.cout == 24):
        r = [conf_alpha(conf_as[b], conf_bs[b], up, w0, b0, cw, slope0, slope1, want_max) for b in range(B)]
        if want_max:
            return _maps([a for a, _ in r], stack), _maps([m for _, m in r], stack)
        return _maps(r, stack)
    return _conf_alpha(conf_as, conf_bs, up, w0, b0, cw, slope0, slope1, want_max, B)


def _warp_b(single, name, check, out_shape, xs, flows, stack):
    """refvsr_<name>_batch: the warp `single` over B maps.  check: the maps' layout check; out_shape(map shape, hf, wf): one result."""
    B = len(xs)
    if not multimap_ok(B):
        return _maps([single(x, f) for x, f in zip(xs, flows)], stack)
    for x, f in zip(xs, flows):
        check(x)
        _planar(f, 2)
        assert x.shape == xs[0].shape and f.shape == flows[0].shape
    hf, wf = flows[0].shape[1:]
    out = torch.empty((B,) + out_shape(xs[0].shape, hf, wf), dtype=xs[0].dtype, device=xs[0].device)
    # (the maps' three extents go as they lie: hin, win, cs of an nhwc16 map, c, hin, win of a planar one)
    hip.check(getattr(hip.lib(), 'refvsr_%s_batch' % name)(_parr(xs), B, *xs[0].shape, _parr(flows), hf, wf, _parr(list(out)), _stream()),
              name + '_batch')
    return out


def warp_nhwc16_b(xs, flows, stack=True):
    return _warp_b(warp_nhwc16, 'warp_nhwc16', _nhwc, lambda s, hf, wf: (hf, wf, s[2]), xs, flows, stack)


def warp_nhwc16_up2_b(xs, flows_lr, stack=True):
    return _warp_b(warp_nhwc16_up2, 'warp_nhwc16_up2', _nhwc, lambda s, hl, wl: (2 * hl, 2 * wl, s[2]), xs, flows_lr, stack)


def warp_planar_b(xs, flows, stack=True):
    return _warp_b(warp_planar, 'warp_planar', _planar, lambda s, hf, wf: (s[0], hf, wf), xs, flows, stack)


# ---- RefVSR_IR / EDVR-M pieces (csrc/edvr.hip) -------------------------------------------------------------------------
def dcn_sample(x, offset_mask, deform_groups=8):
    """Sampling half of the modulated deformable conv: x nhwc16 [h,w,c], offset_mask planar fp32 [3*dg*9,h,w] (raw
    conv_offset output) -> columns nhwc16 [h,w,9*c] in (tap, channel) order."""
    _nhwc(x)
    h, w, c = x.shape
    _planar(offset_mask, 3 * deform_groups * 9)
    assert tuple(offset_mask.shape[1:]) == (h, w)
    cols = torch.empty((h, w, 9 * c), dtype=torch.float16, device=x.device)
    hip.check(hip.lib().refvsr_dcn_sample(_ptr(x), h, w, c, _ptr(offset_mask), deform_groups, _ptr(cols), _stream()), 'dcn_sample')
    return cols


def tsa_weight(aligned, emb, emb_ref):
    """TSAFusion temporal attention: t aligned maps weighted by sigmoid(<emb_i, emb_ref>), side by side -> [h,w,t*c]."""
    t = len(aligned)
    h, w, c = aligned[0].shape
    for m in list(aligned) + list(emb) + [emb_ref]:
        _nhwc(m)
        assert tuple(m.shape) == (h, w, c)
    out = torch.empty((h, w, t * c), dtype=torch.float16, device=emb_ref.device)
    pa = (C.c_void_p * t)(*[m.data_ptr() for m in aligned])
    pe = (C.c_void_p * t)(*[m.data_ptr() for m in emb])
    hip.check(hip.lib().refvsr_tsa_weight(pa, pe, _ptr(emb_ref), t, c, h * w, _ptr(out), _stream()), 'tsa_weight')
    return out


def pool3s2_pair(x):
    """cat([MaxPool2d(3, 2, 1)(x), AvgPool2d(3, 2, 1)(x)], channel) on an nhwc16 map -> [ho, wo, 2c]."""
    _nhwc(x)
    h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty((ho, wo, 2 * c), dtype=torch.float16, device=x.device)
    for off, is_max in ((0, 1), (c, 0)):
        hip.check(hip.lib().refvsr_pool3s2_nhwc16(_ptr(x), h, w, c, _ptr(out), 2 * c, off, is_max, _stream()), 'pool3s2')
    return out


def up2_bilinear_nhwc16(x, mul=1.0):
    _nhwc(x)
    h, w, c = x.shape
    out = torch.empty((2 * h, 2 * w, c), dtype=torch.float16, device=x.device)
    hip.check(hip.lib().refvsr_up2_bilinear_nhwc16(_ptr(x), h, w, c, mul, _ptr(out), _stream()), 'up2_bilinear')
    return out


def tsa_blend(feat, attn, add):
    """feat * sigmoid(attn) * 2 + add."""
    for m in (feat, attn, add):
        _nhwc(m)
        assert m.shape == feat.shape
    out = torch.empty_like(feat)
    hip.check(hip.lib().refvsr_tsa_blend(_ptr(feat), _ptr(attn), _ptr(add), feat.numel(), _ptr(out), _stream()), 'tsa_blend')
    return out
