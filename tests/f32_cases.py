"""Inputs on which the exact-fp32 kernels compute EXACTLY, and a float64 reference of each: the fp32 twin of tests/exact_cases.py.

The fp32 path feeds the matching's arg-max: refvsr_conv_mfma in F32 mode (fp32 operands on v_mfma_f32_16x16x4_f32),
refvsr_conv_direct_f32 and refvsr_conv1x1_f32 (fmaf chains), refvsr_frame_prep (MeanShift + pool).  If the activations are multiples
of a granule g_x, the weights multiples of g_w, all of them fp32 numbers and none a subnormal, and for every output element

    sum |x| |w| + |bias| + |residual|  <  2^24 g_x g_w                                              (the exactness condition)

then every product and every partial sum, in ANY order, is a multiple of g_x g_w below 2^24 of them: an fp32 number.  Any MFMA
schedule and any fmaf chain then returns the bits of a float64 reference.  The bookkeeping (Val, granule, the bound) is that of
exact_cases; only the weight handling differs (no hi / lo split: an fp32 weight is one operand).

Case kinds and their controls, all computed from the reference alone:
  dense   dyadic weights of 12 to 14 significant bits (more than fp16 holds) on maps in {-1, 0, 1}, with bias and the epilogue
          operands.  Control: ONE 4-channel K-block of ONE tap dropped changes >= CTL_B_MIN and >= CTL_B_COUNT outputs.
  wfull   one-tap weights whose value uses all 24 bits (an odd integer in [2^23, 2^24) times 2^-24) on maps of +-2^k.  Controls:
          weights rounded to fp16, and to an exact hi + lo pair (22 bits), change >= CTL_A_MIN of the outputs.
  xfull   one-tap weights +-1 (or +-1/2) on maps whose values use all 24 bits.  Control: activations rounded to fp16.
The one-tap kinds are what separate exact fp32 operands from fp16, tf32-like or hi + lo operands.  They carry no bias and one
weight magnitude / one map exponent per case: a 24-bit operand leaves the condition room for nothing else (the map granule is
tracked per tensor).
"""
import functools
import math

import torch
import torch.nn.functional as F

import exact_cases as ec
from exact_cases import CTL_A_MIN, CTL_B_COUNT, CTL_B_MIN, F64, LIMIT, Val, granule, rng

TINY = 2.0 ** -126                # smallest normal fp32 number
S7, T8, L19 = ec.S7, ec.T8, ec.L19


def pad4(c):
    return (c + 3) // 4 * 4


def channel_groups4(src_channels):
    """Real input channels of each 4-channel group of the concatenated sources (each source padded to 4 in its own buffer)."""
    groups, base = [], 0
    for c in src_channels:
        for o in range(0, c, 4):
            groups.append(list(range(base + o, base + min(o + 4, c))))
        base += c
    return groups


def _r16(t):
    return t.float().half().double()


class Arith32(ec.Arith):
    """The arithmetic a reference runs in.
       'f64'   float64                                                  (the reference)
       'f32'   float32 F.conv2d                                         (the empirical side of the exactness argument)
       'drop'  float64, K-block `block` = (tap, 4-channel group) of every conv dropped          (control of the dense cases)
       'w16'   weights rounded to fp16, 'whl' to hi + lo = fp16(w) + fp16(w - fp16(w))            (controls of the wfull cases)
       'x16'   activations rounded to fp16                                                       (control of the xfull cases)"""

    def weights(self, w, src_channels):
        assert torch.equal(w.float().double(), w), 'weights must be fp32 numbers'
        if self.mode == 'drop':
            groups, ks = channel_groups4(src_channels), w.shape[2]
            tap, cg = self.block[0] % (ks * ks), self.block[1] % len(groups)
            w = w.clone()
            w[:, groups[cg], tap // ks, tap % ks] = 0
        elif self.mode == 'w16':
            w = _r16(w)
        elif self.mode == 'whl':
            hi = _r16(w)
            w = hi + _r16(w - hi)
        return w

    def conv(self, x, w, b, stride=1, pad=None, src_channels=None):
        x = x if isinstance(x, Val) else Val(self, x)
        ks = w.shape[2]
        pad = ks // 2 if pad is None else pad
        wv = self.weights(w, src_channels or [w.shape[1]])
        xv = _r16(x.v) if self.mode == 'x16' else x.v.double()
        for t in (x.v.double(), w, b):
            nz = t[t != 0].abs()
            assert nz.numel() == 0 or float(nz.min()) >= TINY, 'subnormal operand'
        if self.mode == 'f32':
            y = F.conv2d(xv.float()[None], wv.float(), b.float(), stride, pad)[0]
        else:
            y = F.conv2d(xv[None], wv, b, stride, pad)[0]
        m = F.conv2d(x.v.double().abs()[None], w.abs(), b.abs(), stride, pad)[0]
        g = min(x.g * granule(w), granule(b))
        assert g >= TINY, 'partial sums could be subnormal'
        return Val(self, y, m, g)


# ---- references ------------------------------------------------------------------------------------------------------------------
def ref_conv32(A, p):
    """refvsr_conv_mfma with RefvsrConv.f32 = 1 (conv_mfma.hip `epilogue`: bias after the K loop, rv_lrelu, mul, res, post, then the
    fp32 store, or the planar branch: + res_planar + add_const, clamp), refvsr_conv_direct_f32 (conv_direct.hip:85-100:
    rv_lrelu(acc + bias, slope), stored as fp32 or as `(f16)`: ONE rounding) and refvsr_conv1x1_f32 (conv_direct.hip:164-167)."""
    y = A.conv(torch.cat(p['srcs'], 0), p['w'], p['b'], p.get('stride', 1), p.get('pad'), [s.shape[0] for s in p['srcs']])
    y = y.lrelu(p.get('act', 1.0))
    if p.get('mul') is not None:
        y = y.mul(p['mul'])
    if p.get('res') is not None:
        y = y.add(p['res'])
    y = y.lrelu(p.get('post', 1.0))
    if p.get('out') == 'planar':
        if p.get('res_planar') is not None:
            y = y.add(p['res_planar'])
        y = y.add(p.get('add_const', 0.0))
        if p.get('clamp') is not None:
            y = y.clamp(*p['clamp'])
    if p.get('store') == 'f16':
        y = y.half()
    return {'out': y.v.double()}, y.g


def ref_prep(A, p):
    """refvsr_frame_prep (prep.hip): lr8 / ref8 = `(f16)x` of the three frame channels (lanes 3..7 zero); lr_n = MeanShift(lr) =
    W x + b per pixel (mean_shift3: an fmaf chain from 0, then + bias), lane 3 zero; ref_n = the mean of the MeanShift of each whole
    2 x 2 quad of the reference frame (pool4), lane 3 zero -- a row / column left over at an odd edge feeds ref8 only."""
    w, b = p['w'], p['b']
    lr_n = A.conv(p['lr'], w, b)
    rn = A.conv(p['ref'], w, b)
    hr, wr = p['ref'].shape[1:]
    q = rn.v[:, :hr // 2 * 2, :wr // 2 * 2]
    pooled = (q[:, 0::2, 0::2] + q[:, 0::2, 1::2] + q[:, 1::2, 0::2] + q[:, 1::2, 1::2]) * 0.25
    mq = rn.m[:, :hr // 2 * 2, :wr // 2 * 2]
    pm = mq[:, 0::2, 0::2] + mq[:, 0::2, 1::2] + mq[:, 1::2, 0::2] + mq[:, 1::2, 1::2]       # every partial sum of the four, before the scale
    A.check(pm, rn.g)
    ref_n = Val(A, pooled, pm * 0.25, rn.g * 0.25)
    return {'out': lr_n.v.double(), 'ref_n': ref_n.v.double(), 'lr8': _r16(p['lr']), 'ref8': _r16(p['ref'])}, ref_n.g


REFS = {'conv': ref_conv32, 'prep': ref_prep}
CONTROL_OF = {'dense': ('drop',), 'wfull': ('w16', 'whl'), 'xfull': ('x16',)}


class Case32(object):
    """name; kind (which reference); strength ('dense' | 'wfull' | 'xfull'); run (which entry point and how); p (inputs, float64)."""
    primary, lo0 = 'f64', None

    def __init__(self, name, kind, strength, run, p, seed=0):
        self.name, self.kind, self.strength, self.run, self.p = name, kind, strength, run, p
        g = rng(seed + 977)
        self.block = (int(torch.randint(0, 49, (1,), generator=g)), int(torch.randint(0, 64, (1,), generator=g)))

    def evaluate(self, mode):
        A = Arith32(mode, self.block)
        out, g = REFS[self.kind](A, self.p)
        return out, g, A.bound

    @functools.cached_property
    def full(self):
        return self.evaluate('f64')

    @property
    def want(self):
        return self.full[0]

    @property
    def g_out(self):
        return self.full[1]

    @property
    def bound(self):
        return self.full[2]

    @functools.cached_property
    def changed(self):
        """{control: (share, count)} of the outputs that the control changes."""
        res = {}
        for mode in CONTROL_OF[self.strength]:
            d = self.evaluate(mode)[0]['out'] != self.want['out']
            res[mode] = (float(d.double().mean()), int(d.sum()))
        return res

    @property
    def controls(self):
        """(a, b share, b count) in the shape exact_cases.matches reads: b = the weakest control of the case."""
        weakest = min(self.changed.values())
        return weakest[0], weakest[0], weakest[1]

    def assert_strong(self):
        assert self.bound < LIMIT, '%s: exactness condition violated: 2^%.2f granules' % (self.name, math.log2(self.bound))
        for mode, (share, n) in self.changed.items():
            if mode == 'drop':
                assert share >= CTL_B_MIN and n >= CTL_B_COUNT, '%s: control drop = %.4f (%d elements)' % (self.name, share, n)
            else:
                assert share >= CTL_A_MIN, '%s: control %s = %.3f' % (self.name, mode, share)

    def line(self):
        return 'bound=2^%.2f %s' % (math.log2(max(self.bound, 1.0)), ' '.join('ctl_%s=%.4f (%d)' % (k, v[0], v[1]) for k, v in self.changed.items()))


# ---- generators ------------------------------------------------------------------------------------------------------------------
def full24(g, shape):
    """Signed values that use all 24 bits of an fp32 significand: odd integers in [2^23, 2^24) times 2^-24, in (-1, -1/2] u [1/2, 1)."""
    n = torch.randint(2 ** 22, 2 ** 23, shape, generator=g).to(F64) * 2 + 1
    return n * 2.0 ** -24 * ec.pick(g, [1.0, -1.0], shape)


def out_hw(hw, ks, stride, pad=None):
    pad = ks // 2 if pad is None else pad
    return (hw[0] + 2 * pad - ks) // stride + 1, (hw[1] + 2 * pad - ks) // stride + 1


def conv_inputs(strength, seed, co, cins, ks, hw, stride=1, out='planar', act=1.0, post=1.0, mul=False, res=False, res_planar=False,
                add_const=0.0, clamp=None, mag_exp=-3, store='f32', wmag=1.0, xexp=0):
    """The inputs of one conv case.  dense: dyadic weights on the 2^-17 grid below 2^mag_exp; wfull / xfull: see the module text."""
    g = rng(seed)
    h, w = hw
    cin = sum(cins)
    if strength == 'dense':
        wt, b = ec.dyadic_weights(g, co, cin, ks, -17, mag_exp), ec.dyadic_vec(g, co)
        srcs = [ec.int_map(g, c, h, w) for c in cins]
    elif strength == 'wfull':
        wt = ec.onetap_weights(g, co, cin, ks, vals=(1.0,))
        wt, b = wt * full24(g, wt.shape), torch.zeros(co, dtype=F64)
        srcs = [ec.pick(g, [2.0 ** xexp, -2.0 ** xexp], (c, h, w)) for c in cins]
    else:
        assert strength == 'xfull'
        wt, b = ec.onetap_weights(g, co, cin, ks, vals=(wmag, -wmag)), torch.zeros(co, dtype=F64)
        srcs = [full24(g, (c, h, w)) * 2.0 ** xexp for c in cins]
    p = dict(w=wt, b=b, srcs=srcs, stride=stride, out=out, shuffle=False, act=act, post=post, add_const=add_const, clamp=clamp, store=store)
    ho, wo = out_hw(hw, ks, stride)
    if mul:
        p['mul'] = ec.pick(g, [1.0, -1.0], (co, ho, wo))
    if res:
        p['res'] = ec.int_map(g, co, ho, wo, -4, 4, 0.25)
    if res_planar:
        p['res_planar'] = ec.int_map(g, co, ho, wo, -4, 4, 0.25)
    return p


def conv_case(name, seed, strength, co, cins, ks, hw, run, **kw):
    """A conv case; a dense one takes the most significant bits (14, 13, 12) with which its exactness bound holds."""
    for mag_exp in ((-3, -4, -5) if strength == 'dense' else (None,)):
        if mag_exp is not None:
            kw['mag_exp'] = mag_exp
        c = Case32(name, 'conv', strength, run, conv_inputs(strength, seed, co, cins, ks, hw, **kw), seed)
        if c.bound < LIMIT:
            break
    return c


def _mfma(name, seed, strength, co, cins, ks, hw, mt=None, cap=0, **kw):
    return conv_case(name, seed, strength, co, cins, ks, hw, dict(entry='conv_mfma', mt=mt, hi_only=False, f32=True, cap=cap), **kw)


def _direct(name, seed, strength, co, ci, ks, hw, stride=1, out_c=0, act=0.25, **kw):
    """refvsr_conv_direct_f32: planar fp32 output, or fp16 HWC (`nhwc16_out`) in a channel stride of out_c."""
    return conv_case(name, seed, strength, co, [ci], ks, hw, dict(entry='conv_direct', out_c=out_c), stride=stride, act=act,
                     out='nhwc' if out_c else 'planar', store='f16' if out_c else 'f32', **kw)


def _c1x1(name, seed, strength, ci, hw, act, **kw):
    return conv_case(name, seed, strength, 16, [ci], 1, hw, dict(entry='conv1x1'), act=act, **kw)


def _prep(name, seed, sizes):
    """Frames on the 2^-12 grid in [0, 1) (their fp16 copies round), a dyadic MeanShift: |W| <= 2 on the 2^-6 grid, bias on 2^-8."""
    g = rng(seed)
    h, w, hr, wr = sizes
    p = dict(lr=torch.randint(0, 4096, (3, h, w), generator=g).to(F64) * 2.0 ** -12,
             ref=torch.randint(0, 4096, (3, hr, wr), generator=g).to(F64) * 2.0 ** -12,
             w=torch.randint(-128, 129, (3, 3, 1, 1), generator=g).to(F64) * 2.0 ** -6,
             b=torch.randint(-512, 513, (3,), generator=g).to(F64) * 2.0 ** -8)
    return Case32(name, 'prep', 'dense', dict(entry='frame_prep'), p, seed)


def _table():
    T = {}

    def add(fn, name, *a, **k):
        assert name not in T, name
        T[name] = functools.partial(fn, name, 5000 + len(T), *a, **k)
    # -- premise: does the fp32 MFMA return exactly representable sums exactly?  dense weights, planar fp32 output, no epilogue operand
    add(_mfma, 'premise conv_mfma f32 [24]->32 3x3 19x45', 'dense', 32, [24], 3, L19)
    # -- refvsr_conv_mfma, F32 mode: the engine's shapes (VGG head of the matching) at 19 x 45, both stores, below one tile
    add(_mfma, 'conv_mfma f32 [3]->64 3x3 19x45 hwc relu', 'dense', 64, [3], 3, L19, out='nhwc', act=0.0)
    add(_mfma, 'conv_mfma f32 [3]->64 3x3 7x5 planar', 'dense', 64, [3], 3, S7)
    add(_mfma, 'conv_mfma f32 [64]->64 3x3 19x45 hwc relu', 'dense', 64, [64], 3, L19, out='nhwc', act=0.0)
    add(_mfma, 'conv_mfma f32 [64]->64 3x3 19x45 planar', 'dense', 64, [64], 3, L19)
    add(_mfma, 'conv_mfma f32 [64]->128 3x3 19x45 hwc relu', 'dense', 128, [64], 3, L19, out='nhwc', act=0.0)
    add(_mfma, 'conv_mfma f32 [64]->128 3x3 7x5 hwc', 'dense', 128, [64], 3, S7, out='nhwc')
    add(_mfma, 'conv_mfma f32 [64]->16 1x1 19x45 planar act.25', 'dense', 16, [64], 1, L19, act=0.25)
    add(_mfma, 'conv_mfma f32 [128]->16 1x1 19x45 hwc act.25', 'dense', 16, [128], 1, L19, out='nhwc', act=0.25)
    add(_mfma, 'conv_mfma f32 [128]->16 1x1 7x5 planar', 'dense', 16, [128], 1, S7)
    add(_mfma, 'conv_mfma f32 [64]->64 3x3 19x45 hwc mul res post0', 'dense', 64, [64], 3, L19, out='nhwc', mul=True, res=True, post=0.0)
    add(_mfma, 'conv_mfma f32 [64]->64 3x3 19x45 planar everything', 'dense', 64, [64], 3, L19, act=0.0, mul=True, res=True, res_planar=True,
        add_const=0.25, clamp=(-1.0, 1.0))
    add(_mfma, 'conv_mfma f32 wfull [3]->64 3x3 19x45 hwc', 'wfull', 64, [3], 3, L19, out='nhwc', xexp=-2)
    add(_mfma, 'conv_mfma f32 wfull [64]->64 3x3 19x45 planar relu', 'wfull', 64, [64], 3, L19, act=0.0, xexp=3)
    add(_mfma, 'conv_mfma f32 wfull [128]->16 1x1 19x45 hwc', 'wfull', 16, [128], 1, L19, out='nhwc')
    add(_mfma, 'conv_mfma f32 xfull [64]->128 3x3 19x45 hwc', 'xfull', 128, [64], 3, L19, out='nhwc')
    add(_mfma, 'conv_mfma f32 xfull [64]->64 3x3 7x5 planar w.5', 'xfull', 64, [64], 3, S7, wmag=0.5, xexp=2)
    add(_mfma, 'conv_mfma f32 xfull [64]->16 1x1 19x45 planar relu', 'xfull', 16, [64], 1, L19, act=0.0)
    # -- refvsr_conv_direct_f32: 16 x 16 pixel tiles, channel chunks of 8 in and 16 out
    D17, D18 = (17, 19), (18, 22)
    add(_direct, 'conv_direct [2]->16 3x3 17x19 (confidence conv)', 'dense', 16, 2, 3, D17, act=0.25)
    add(_direct, 'conv_direct [2]->16 3x3 17x19 nhwc16', 'dense', 16, 2, 3, D17, act=0.25, out_c=16)
    add(_direct, 'conv_direct [2]->16 3x3 7x5 nhwc16', 'dense', 16, 2, 3, S7, act=0.0, out_c=16)
    add(_direct, 'conv_direct [3]->3 1x1 7x5 (MeanShift)', 'dense', 3, 3, 1, S7, act=1.0)
    add(_direct, 'conv_direct [3]->64 3x3 17x19', 'dense', 64, 3, 3, D17, act=0.0)
    add(_direct, 'conv_direct [2]->3 3x3 7x5', 'dense', 3, 2, 3, S7)
    add(_direct, 'conv_direct [9]->2 3x3 17x19', 'dense', 2, 9, 3, D17)
    add(_direct, 'conv_direct [5]->24 3x3 s2 18x22', 'dense', 24, 5, 3, D18, stride=2)
    add(_direct, 'conv_direct [5]->24 3x3 s2 18x22 nhwc16 in 24', 'dense', 24, 5, 3, D18, stride=2, out_c=24)
    add(_direct, 'conv_direct [5]->24 3x3 17x19 nhwc16 in 32', 'dense', 24, 5, 3, D17, out_c=32)
    add(_direct, 'conv_direct [9]->24 1x1 7x5 nhwc16 in 32', 'dense', 24, 9, 1, S7, out_c=32)
    add(_direct, 'conv_direct [64]->128 3x3 17x19', 'dense', 128, 64, 3, D17, act=0.0)
    add(_direct, 'conv_direct [64]->16 1x1 17x19', 'dense', 16, 64, 1, D17)
    add(_direct, 'conv_direct [64]->2 1x1 s2 18x22', 'dense', 2, 64, 1, D18, stride=2, act=1.0)
    add(_direct, 'conv_direct [9]->128 3x3 7x5', 'dense', 128, 9, 3, S7)
    add(_direct, 'conv_direct wfull [9]->24 3x3 17x19', 'wfull', 24, 9, 3, D17, act=0.0, xexp=-1)
    add(_direct, 'conv_direct wfull [64]->16 1x1 17x19', 'wfull', 16, 64, 1, D17, act=1.0, xexp=4)
    add(_direct, 'conv_direct xfull [5]->16 3x3 17x19', 'xfull', 16, 5, 3, D17, act=1.0)
    add(_direct, 'conv_direct xfull [3]->2 3x3 s2 18x22 w.5', 'xfull', 2, 3, 3, D18, stride=2, act=0.0, wmag=0.5)
    # -- refvsr_conv1x1_f32: 64 pixels per workgroup; 3 pixels, whole workgroups (256), a partial last one (855)
    slopes = (0.0, 0.25, 1.0)
    for i, ci in enumerate((4, 64, 128, 256)):
        for j, hw in enumerate(((1, 3), T8, L19)):
            add(_c1x1, 'conv1x1 [%d]->16 %dx%d act%g' % (ci, hw[0], hw[1], slopes[(i + j) % 3]), 'dense', ci, hw, slopes[(i + j) % 3])
    add(_c1x1, 'conv1x1 wfull [64]->16 19x45 act0', 'wfull', 64, L19, 0.0, xexp=-3)
    add(_c1x1, 'conv1x1 wfull [256]->16 8x32 act1', 'wfull', 256, T8, 1.0)
    add(_c1x1, 'conv1x1 xfull [128]->16 19x45 act1', 'xfull', 128, L19, 1.0)
    add(_c1x1, 'conv1x1 xfull [4]->16 1x3 act0 w.5', 'xfull', 4, (1, 3), 0.0, wmag=0.5)
    # -- refvsr_frame_prep (h, w, hr, wr): the smallest frames, odd edges of the reference frame, more than one workgroup
    for sizes in ((2, 2, 2, 2), (6, 10, 7, 11), (19, 45, 19, 45)):
        add(_prep, 'frame_prep %dx%d ref %dx%d' % sizes, sizes)
    return T


TABLE = _table()
NAMES = list(TABLE)
PREMISE = NAMES[0]
_CACHE = {}


def get_case(name):
    if name not in _CACHE:
        _CACHE[name] = TABLE[name]()
    return _CACHE[name]


# ---- decoder of the f32 packing (inverse of refvsr_amd.packing.pack_conv(f32=True)) -------------------------------------------------
def decode_pack_conv_f32(pk, kslot):
    """packing.pack_conv's fp32 fragments [nz, S, MT, 64, 4] -> (w, bias) in conv-channel order; asserts that every K-block is there
    once and that padding channels, padding rows and unused K-slots hold zeros."""
    wp = pk['wpack']
    assert wp.dtype == torch.float32 and wp.dim() == 5 and wp.shape[3:] == (64, 4)
    nz, S, MT = wp.shape[:3]
    full = wp.double().reshape(nz, S, MT, 4, 16, 4).permute(0, 2, 4, 1, 3, 5).reshape(nz * MT * 16, S * 4, 4)
    ks, cout, srcs = pk['ksize'], pk['cout'], pk['src_channels']
    cmap, base = [], 0
    for c in srcs:
        cmap += [base + i if i < c else -1 for i in range(pad4(c))]
        base += c
    ncg = len(cmap) // 4
    assert not full[cout:].any(), 'padding rows hold weights'
    w = torch.zeros(cout, sum(srcs), ks, ks, dtype=F64)
    seen = set()
    for tap in range(ks * ks):
        for cg in range(ncg):
            j = kslot(tap // ks, tap % ks, cg, ks, ncg)
            assert j not in seen and j < S * 4
            seen.add(j)
            for i in range(4):
                ch = cmap[cg * 4 + i]
                if ch < 0:
                    assert not full[:cout, j, i].any(), 'padding channel holds weights'
                else:
                    w[:, ch, tap // ks, tap % ks] = full[:cout, j, i]
    rest = [j for j in range(S * 4) if j not in seen]
    assert not full[:, rest].any(), 'unused K-slot holds weights'
    return w, pk['bias'].double()[:cout]

