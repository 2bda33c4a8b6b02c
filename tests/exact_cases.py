"""Inputs on which the hi + lo conv kernels compute EXACTLY, and a float64 reference of every operation they are fed to.

Every conv kernel of the library multiplies fp16 activations by fp16 weight halves (hi = fp16(w), lo = fp16(w - hi)) on MFMAs that
accumulate in fp32.  If the activations are multiples of a granule g_x, hi and lo multiples of g_w, and for every output element

    sum |x| (|hi| + |lo|) + |bias| + |residual|  <  2^24 g_x g_w                                    (the exactness condition)

then every product and every partial sum -- in ANY order, through any MFMA shape, any hi / lo fold -- is a multiple of g_x g_w below
2^24 of them: an fp32 number.  The fp32 accumulator is then the exact sum, an fp16 store is ONE round-to-nearest-even of an exact
number, and a float64 reference that rounds at the same points equals the kernel bit for bit.  A kernel that loses one lo fragment
of one K-block (a lo value is ~2^-12 of its weight) does not.

This module has
  * generators: dyadic full weights, one-tap weights, null weights, integer maps;
  * checks: the exact hi / lo split, the exactness condition (tracked in float64 through every stage: Arith / Val), the granule
    finder;
  * the float64 reference of each operation (ref_*), F.conv2d on float64 tensors, with the fp16 roundings where the kernel stores
    fp16 -- each ref_* names the kernel lines its rounding points come from.  Nothing of refvsr_amd goes into a reference;
  * the controls: (a) the share of outputs that changes when EVERY lo term is dropped, (b) the share / count that changes when the
    lo term of ONE 8-channel K-block of ONE tap is dropped -- both from the reference alone, so a weak input cannot pass for a
    strong test;
  * decoders of the packed weight formats (the inverse of refvsr_amd.packing, for tests/test_exact_cases.py);
  * the output heads with a NON-ZERO base frame: base maps on which the fp32 bicubic at steps 1/4 and 1/2 is itself exact (BASE_SETS,
    base_proof), so that clamp(conv + bias + clamp01(bicubic(base)), 0, 1) is one fp32 rounding of an exact real; their class counts,
    border condition and controls (head_classes, head_borders, base_control); and a general family with a base of bytes / 255 held
    to a bound derived from the chain of roundings (GeneralCase);
  * the case table shared by tests/test_exact_cases.py (CPU: condition, controls, fp32 emulation, packing) and
    tests/test_gpu_exact.py (the kernels).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
LIMIT = 2.0 ** 24                 # granules an fp32 significand counts exactly
CTL_A_MIN = 0.05                  # control (a): share of outputs
CTL_B_MIN, CTL_B_COUNT = 0.01, 8  # control (b): share and count of outputs
S7, T8, T16, L19 = (7, 5), (8, 32), (16, 32), (19, 45)      # below one tile, one exact tile (8 | 16 rows), partial tiles both ways


# ---- generators ------------------------------------------------------------------------------------------------------------------
def rng(seed):
    return torch.Generator().manual_seed(int(seed))


def dyadic_weights(g, cout, cin, ks, g_exp=-17, mag_exp=-3):
    """Random integer multiples of 2^g_exp with |w| < 2^mag_exp (float64)."""
    n = 2 ** (mag_exp - g_exp)
    return torch.randint(-n + 1, n, (cout, cin, ks, ks), generator=g).to(F64) * 2.0 ** g_exp


def onetap_weights(g, cout, cin, ks=3, vals=(1.0, -1.0, 0.5, -0.5)):
    """Output channel o takes ONE input channel (a random permutation, repeated when cout > cin) through ONE random tap with a
    weight of `vals`: fp16-representable (lo = 0), and any fp16 input map stays exact through it."""
    w = torch.zeros(cout, cin, ks, ks, dtype=F64)
    perm = torch.randperm(cin, generator=g)
    for o in range(cout):
        tap = int(torch.randint(0, ks * ks, (1,), generator=g))
        w[o, int(perm[o % cin]), tap // ks, tap % ks] = vals[int(torch.randint(0, len(vals), (1,), generator=g))]
    return w


def null_weights(c, cin=None, ks=3):
    return torch.zeros(c, cin or c, ks, ks, dtype=F64)


def int_map(g, c, h, w, lo=-1, hi=1, scale=1.0):
    return torch.randint(lo, hi + 1, (c, h, w), generator=g).to(F64) * scale


def dyadic_vec(g, n, lo=-4, hi=4, scale=0.25):
    return torch.randint(lo, hi + 1, (n,), generator=g).to(F64) * scale


def pick(g, vals, shape):
    return torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), shape, generator=g)]


# ---- checks ----------------------------------------------------------------------------------------------------------------------
def split_hi_lo(w):
    """hi = fp16(w), lo = fp16(w - hi) as float64 tensors, with the assert that the split is exact."""
    assert torch.equal(w.float().double(), w), 'weights must be fp32 numbers'
    hi = w.float().half().double()
    lo = (w - hi).float().half().double()
    assert torch.equal(hi + lo, w), 'hi + lo != w: the weights do not fit the 22-bit split'
    return hi, lo


def granule(t):
    """Largest power of two that divides every element of t (2^16 for an all-zero tensor)."""
    t = t.double().reshape(-1)
    t = t[t != 0]
    for e in range(16, -80, -1):
        s = t * 2.0 ** -e
        if torch.equal(s, s.round()):
            return 2.0 ** e
    raise AssertionError('no granule down to 2^-80')


def pad8(c):
    return (c + 7) // 8 * 8


def channel_groups(src_channels):
    """Real input channels of each 8-channel group of the concatenated sources (each source padded to 8 in its own buffer)."""
    groups, base = [], 0
    for c in src_channels:
        for o in range(0, c, 8):
            groups.append(list(range(base + o, base + min(o + 8, c))))
        base += c
    return groups


class Val(object):
    """A map under the exactness bookkeeping: v the values, m an upper bound of every partial magnitude, g the granule."""

    def __init__(self, A, v, m=None, g=None):
        self.A, self.v = A, v
        self.m = v.double().abs() if m is None else m
        self.g = granule(v) if g is None else g
        A.check(self.m, self.g)

    def _t(self, t):
        return t.to(self.v.dtype) if isinstance(t, torch.Tensor) else t

    def lrelu(self, s):
        """max(y, s y) (0 <= s <= 1) == y >= 0 ? y : s y; s is 0, 1 or a power of two."""
        if s == 1.0:
            return self
        assert s == 0.0 or math.log2(s) == round(math.log2(s)), s
        v = torch.where(self.v >= 0, self.v, self.v * s)
        return Val(self.A, v, self.m, self.g * s if s else self.g)

    def mul(self, t):
        return Val(self.A, self.v * self._t(t), self.m * t.double().abs(), self.g * granule(t))

    def add(self, t):
        if not isinstance(t, torch.Tensor):
            t = torch.tensor(float(t), dtype=F64)
        return Val(self.A, self.v + self._t(t), self.m + t.double().abs(), min(self.g, granule(t)))

    def clamp(self, lo, hi):
        return Val(self.A, self.v.clamp(lo, hi), self.m, min(self.g, granule(torch.tensor([lo, hi], dtype=F64))))

    def half(self):
        """ONE round-to-nearest-even to fp16 (the value is an fp32 number by the condition, so the float32 step is exact)."""
        return Val(self.A, self.v.float().half().to(self.v.dtype))


class Arith(object):
    """The arithmetic a reference runs in.
       'f64'     float64, w = hi + lo                                   (the reference)
       'f32'     float32 F.conv2d with hi and with lo, added            (the empirical side of the exactness argument)
       'hi'      float64, every lo term dropped: w = fp16(w)            (control (a); the reference of the fp16-weight kernels)
       'drop'    float64, the lo term of K-block `block` = (tap, group) dropped in every conv            (control (b))
       'drop_hi' the same K-block's hi term dropped, 'flush' fp16-subnormal hi terms zeroed (controls of the lo = 0 cases)
    bound = the largest count of granules any stage reached."""

    def __init__(self, mode='f64', block=(0, 0)):
        self.mode, self.block, self.bound = mode, block, 0.0

    def check(self, m, g):
        self.bound = max(self.bound, float(m.max()) / g)

    def weights(self, w, src_channels):
        hi, lo = split_hi_lo(w)
        if self.mode == 'hi':
            lo = torch.zeros_like(lo)
        elif self.mode in ('drop', 'drop_hi'):
            groups, ks = channel_groups(src_channels), w.shape[2]
            tap, cg = self.block[0] % (ks * ks), self.block[1] % len(groups)
            t = (lo if self.mode == 'drop' else hi).clone()
            t[:, groups[cg], tap // ks, tap % ks] = 0
            hi, lo = (hi, t) if self.mode == 'drop' else (t, lo)
        elif self.mode == 'flush':
            hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
        return hi, lo

    def conv(self, x, w, b, stride=1, pad=None, src_channels=None):
        """conv2d(x, w) + b of a [C, H, W] map (zero padding), under the bookkeeping."""
        x = x if isinstance(x, Val) else Val(self, x)
        ks = w.shape[2]
        pad = ks // 2 if pad is None else pad
        hi, lo = self.weights(w, src_channels or [w.shape[1]])
        if self.mode == 'f32':
            xf = x.v.float()[None]
            y = (F.conv2d(xf, hi.float(), None, stride, pad) + F.conv2d(xf, lo.float(), None, stride, pad))[0] + b.float()[:, None, None]
        else:
            y = F.conv2d(x.v.double()[None], hi + lo, b, stride, pad)[0]
        m = F.conv2d(x.v.double().abs()[None], hi.abs() + lo.abs(), b.abs(), stride, pad)[0]
        g = min(x.g * min(granule(hi), granule(lo)), granule(b))
        return Val(self, y, m, g)


# ---- references ------------------------------------------------------------------------------------------------------------------
def ref_conv(A, p):
    """refvsr_conv_mfma, refvsr_conv24 / 32 / 48, refvsr_conv_shuffle2:
         y = post(act(conv + bias) * mul + res)                          all in fp32
         planar fp32 output: y + res_planar + add_const, clamp, stored as fp32 -- no rounding at all
         fp16 HWC output:    ONE rounding at the store; the pixel shuffle only moves elements
    conv_mfma.hip `epilogue` (bias after the K loop, rv_lrelu, mul, res, post, then `(f16)y[i]` or the planar branch) and
    `epilogue_lean` (fmaxf(y, y * slope): the same function for slopes in [0, 1]); conv24.hip "epilogue: out = post(act(acc) * mul
    + res)" (bias is the accumulators' initial value, `(f16)y[i]` at the store) and its pixel-shuffle epilogue."""
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
        return {'out': y.v.double()}, y.g
    y = y.half()
    v = y.v.double()
    if p.get('shuffle'):
        v = F.pixel_shuffle(v[None], 2)[0]
    return {'out': v}, y.g


def _block(A, x, w1, b1, w2, b2, act, post=1.0):
    t = A.conv(x, w1, b1).lrelu(act).half()
    return A.conv(t, w2, b2).add(x.v if isinstance(x, Val) else x).lrelu(post).half()


def ref_blocks(A, p):
    """refvsr_resblock24_chain, refvsr_resblock48_chain, refvsr_resblock_lean, refvsr_resblock_chain: per block
         t   = fp16(act(conv1(x) + b1))          zero outside the frame (conv2's padding)
         out = fp16(post(x + conv2(t) + b2))     post only in the lean kernel; the next block reads this fp16 map
    resblock24.hip: rb_act_pack `(f16)fmaxf(y, y * slope)` (ReLU: `(f16)y` then max with 0 -- the same number), "phase 2: out =
    (b2 + x) + conv2(t)" and rb_pack `(f16)y`; resblock48.hip:123-124 and :365 `(f16)(y + x)`; resblock_lean.hip:286-287 and
    :324-328 (post, then `(f16)y`)."""
    x = p['x']
    for (w1, b1, w2, b2) in p['blocks']:
        x = _block(A, x, w1, b1, w2, b2, p['act'], p.get('post', 1.0))
    return {'out': x.v.double()}, x.g


def ref_conf_alpha(A, p):
    """refvsr_conf_alpha, up = 1:  t = fp16(lrelu(conv_{2->16}(cat[conf_a, conf_b]) + b0, slope0)) (conv24.hip:272, an fp32 FMA chain
    over fp32 weights: exact on one-tap weights), alpha = fp16(lrelu(conv_{16->C}(t) + b, slope1)) (the conv24 epilogue),
    conf_max = max(conf_a, conf_b) (conv24.hip:284).
    up = 2 (CONF = 2): P = clamp01(bicubic x2 of the pair) in fp32 (conv24.hip conf_stage: rv_bicubic_at with a source step of 0.5,
    fminf / fmaxf), the rest as above on the (2 h) x (2 w) grid; no conf_max.  The bicubic is sampling_cases.ref_resize, the float64
    restatement of the resize kernel that shares rv_bicubic_at (float32 under the 'f32' arithmetic); p['mut'] hands it a mutation."""
    P = torch.cat([p['conf_a'], p['conf_b']], 0)
    if p.get('up', 1) == 2:
        P = bicubic_up2(P, np.float32 if A.mode == 'f32' else np.float64, p.get('mut'))
    t = A.conv(P, p['w0'], p['b0']).lrelu(p['slope0']).half()
    y = A.conv(t, p['w'], p['b']).lrelu(p['slope1']).half()
    if p.get('up', 1) == 2:
        return {'out': y.v.double()}, y.g
    return {'out': y.v.double(), 'cmax': torch.maximum(p['conf_a'], p['conf_b'])}, y.g


def bicubic_up(P, s, T=np.float64, mut=None, clamp=True, transposed=False, step=None, mode=None):
    """clamp01(F.interpolate(P, x s, bicubic)) of a [C, h, w] float64 tensor by sampling_cases.ref_resize over the number type T
    (transposed: columns first -- the other summation order).  step: the source step per output sample (default 1 / s: the launchers'
    (float)bh / (float)h); mode: a sampling_cases.RS_* other than the bicubic -- both only for the controls."""
    import sampling_cases as sc                             # (imports this module)
    x = P.numpy().transpose(0, 2, 1) if transposed else P.numpy()
    c, h, w = x.shape
    step = 1.0 / s if step is None else step
    out = sc.ref_resize(T, dict(x=np.ascontiguousarray(x), mode=sc.RS_BICUBIC if mode is None else mode, out_hw=(s * h, s * w),
                                src_scale=(step, step), clamp01=clamp), mut)['out']
    out = out.transpose(0, 2, 1) if transposed else out
    return torch.from_numpy(np.ascontiguousarray(out.astype(np.float64)))


def bicubic_up2(P, T=np.float64, mut=None, clamp=True, transposed=False):
    """bicubic_up at a factor of 2: the staging of refvsr_conf_alpha, up = 2."""
    return bicubic_up(P, 2, T, mut, clamp, transposed)


BASE_SETS = {'u': (0.0, 0.5, 1.0), 's': (-1.0, 0.0, 1.0, 2.0)}     # base values on which the fp32 bicubic at steps 1/4 and 1/2 is exact
BASE_CONTROLS = ('a', 'c', 'd', 'reflect', 'noclamp', 'plane', 'nearest', 'step')


def head_base(p, T=np.float64, ctl=None, transposed=False):
    """The base term of the output heads, clamp01(bicubic x s of p['base']) as a float64 [3, s bh, s bw] tensor: rv_bicubic_at
    (common.h: rv_cubic_src's `((float)o + 0.5f) * scale - 0.5f`, floorf, the four index clamps, rv_cubic_taps; row chains of four
    fmaf, then the column chain) with the step (float)bh / (float)h of the launchers (conv24.hip refvsr_conv_last_fmt, resblock24.hip
    refvsr_conv_hr_last_fmt), channel q reading plane q (`p.base_lr + q * plane_b`), then `fminf(fmaxf(., 0.0f), 1.0f)`.
    ctl: None, or ONE deliberate defect for the controls (applied to the reference alone, never to a kernel):
      'a' trunc for floor | 'c' align-corners coordinates | 'd' two taps swapped      (sampling_cases.ref_resize's mutations)
      'reflect' taps past a border reflect (-1 -> 1) instead of clamping              'noclamp' the sample is not clamped to [0, 1]
      'plane' channel q reads plane (q + 1) % 3      'nearest' the nearest sample     'step' the other factor's step (1/2 for 1/4)"""
    import sampling_cases as sc
    base, s = p['base'], p['s']
    assert ctl is None or ctl in BASE_CONTROLS, ctl
    if ctl == 'plane':
        base = base[[1, 2, 0]]
    if ctl == 'reflect':                                    # x s of the map padded by two reflected samples, cropped: no tap clamps
        pad = torch.from_numpy(np.pad(base.numpy(), ((0, 0), (2, 2), (2, 2)), mode='reflect'))
        out = bicubic_up(pad, s, T, None, True, transposed)
        return out[:, 2 * s:-2 * s, 2 * s:-2 * s].contiguous()
    return bicubic_up(base, s, T, ctl if ctl in ('a', 'c', 'd') else None, ctl != 'noclamp', transposed,
                      step=1.0 / (6 - s) if ctl == 'step' else None, mode=sc.RS_NEAREST if ctl == 'nearest' else None)


def _head_out(A, y, p):
    """The heads' last line, `fminf(fmaxf(v + b, 0.0f), 1.0f)` (conv24.hip:461, resblock24.hip:386): v = conv + bias is exact by the
    exactness condition and the base term b lies on the 2^-24 grid (proved per case on the CPU), so v + b is ONE fp32 rounding of an
    exact real: formed here in float64 (exact: fewer than 53 bits) and rounded once (float32 arithmetic: the fp32 add itself).  With
    no base the sample of a zero map is exactly 0 and nothing is added."""
    if p.get('base') is None:
        y = y.clamp(0.0, 1.0)
        return {'out': y.v.double()}, y.g
    b = head_base(p, np.float32 if A.mode == 'f32' else np.float64, p.get('ctl'))
    assert b.shape == y.v.shape, (tuple(b.shape), tuple(y.v.shape))
    v = (y.v + b.to(y.v.dtype)).float().double()
    return {'out': v.clamp(0.0, 1.0)}, y.g


def ref_conv_last(A, p):
    """refvsr_conv_last: clamp(conv + bias + clamp01(bicubic(base_lr)), 0, 1) as fp32 (conv24.hip:460-461; head_base and _head_out
    name the rounding points; without p['base']: base_lr = 0, whose bicubic sample is exactly 0); result formats (common.h
    rv_store_result): fp16 = `(f16)v`, uint8 = rint(v * 255.0f) with the product rounded to fp32."""
    return _head_out(A, A.conv(p['x'], p['w'], p['b']), p)


def ref_hr_last(A, p):
    """refvsr_conv_hr_last: t = fp16(lrelu(conv_hr(x) + b1)) (resblock24.hip rb_act_pack), then
    clamp(conv_last(t) + b2 + clamp01(bicubic(base_lr)), 0, 1) as fp32 (resblock24.hip:385-386; without p['base']: base_lr = 0)."""
    t = A.conv(p['x'], p['w1'], p['b1']).lrelu(p['act']).half()
    return _head_out(A, A.conv(t, p['w2'], p['b2']), p)


def result_formats(v):
    """fp16 and uint8 results of an exact fp32 head output v (float64 tensor of fp32 numbers) as rv_store_result forms them."""
    v32 = v.float()
    return v32.half(), (v32 * 255.0).round().to(torch.uint8)         # torch.round: half to even, like __float2int_rn


REFS = {'conv': ref_conv, 'blocks': ref_blocks, 'conf_alpha': ref_conf_alpha, 'conv_last': ref_conv_last, 'hr_last': ref_hr_last}


# ---- a case: inputs + reference + controls -----------------------------------------------------------------------------------------
class Case(object):
    """name; kind (which reference); run (which entry point and how: see tests/test_gpu_exact.py); p (the inputs, float64);
    primary: 'f64' (hi + lo kernels) or 'hi' (kernels that are fed fp16(w)); lo0: the weights have no lo part (premise, subnormal)."""

    def __init__(self, name, kind, run, p, primary='f64', lo0=None, seed=0, b_count=CTL_B_COUNT):
        self.name, self.kind, self.run, self.p, self.primary, self.lo0, self.b_count = name, kind, run, p, primary, lo0, b_count
        g = rng(seed + 977)
        self.block = (int(torch.randint(0, 49, (1,), generator=g)), int(torch.randint(0, 12, (1,), generator=g)))

    def evaluate(self, mode):
        A = Arith(mode, self.block)
        out, g = REFS[self.kind](A, self.p)
        return out, g, A.bound

    @functools.cached_property
    def full(self):
        return self.evaluate('f64')

    @functools.cached_property
    def hi(self):
        return self.evaluate('hi')

    @property
    def want(self):
        """What the kernel must return, bit for bit (float64 tensors holding fp16 / fp32 numbers)."""
        return (self.hi if self.primary == 'hi' else self.full)[0]

    @property
    def g_out(self):
        return (self.hi if self.primary == 'hi' else self.full)[1]

    @property
    def bound(self):
        return max(self.full[2], self.hi[2])

    def _changed(self, a, b):
        d = a['out'] != b['out']
        return float(d.double().mean()), int(d.sum())

    @functools.cached_property
    def controls(self):
        """((a) share, (b) share, (b) count).  Weights with a lo part: (a) every lo term dropped, (b) one K-block's lo term dropped
        -- for the kernels fed fp16(w) (primary 'hi') the same two numbers say how far their reference is from the hi + lo one, and
        what one K-block's hi term is worth.  lo = 0 cases: (a) = `lo0` ('drop_hi' | 'flush') applied, (b) one K-block's hi term."""
        if self.lo0:
            a = self._changed(self.full[0], self.evaluate(self.lo0)[0])
            b = self._changed(self.full[0], self.evaluate('drop_hi')[0])
        elif self.primary == 'hi':
            a = self._changed(self.full[0], self.hi[0])
            b = self._changed(self.hi[0], Arith_hi_drop(self))
        else:
            a = self._changed(self.full[0], self.hi[0])
            b = self._changed(self.full[0], self.evaluate('drop')[0])
        return a[0], b[0], b[1]

    def assert_strong(self):
        a, b, nb = self.controls
        assert self.bound < LIMIT, '%s: exactness condition violated: 2^%.2f granules' % (self.name, math.log2(self.bound))
        assert a >= CTL_A_MIN, '%s: control (a) = %.3f' % (self.name, a)
        assert b >= CTL_B_MIN and nb >= self.b_count, '%s: control (b) = %.4f (%d elements)' % (self.name, b, nb)

    def line(self):
        a, b, nb = self.controls
        return 'bound=2^%.2f ctl_a=%.3f ctl_b=%.4f (%d)' % (math.log2(max(self.bound, 1.0)), a, b, nb)


def Arith_hi_drop(case):
    """Reference on fp16(w) with one K-block's hi term dropped (control (b) of the fp16-weight kernels)."""
    p = dict(case.p)
    for k in ('w', 'w1', 'w2'):
        if k in p:
            p[k] = p[k].float().half().double()
    if 'blocks' in p:
        p['blocks'] = [tuple(t.float().half().double() if t.dim() == 4 else t for t in blk) for blk in p['blocks']]
    return REFS[case.kind](Arith('drop_hi', case.block), p)[0]


# ---- mismatch report ---------------------------------------------------------------------------------------------------------------
def _ord16(t):
    i = t.half().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


def mismatch(got, want, g, fp16):
    """(count, text) of the elements where got != want (both float64 [C, H, W]): the first one's (channel, y, x), its deviation in
    fp16 ulps (fp16 outputs) and in granules."""
    d = got != want
    n = int(d.sum())
    if n == 0:
        return 0, 'bit-equal'
    c, y, x = [int(v) for v in d.nonzero()[0]]
    dev = (got - want).abs()
    txt = '%d of %d differ; first at (c=%d, y=%d, x=%d): got %r want %r = %.3g granules' % (
        n, d.numel(), c, y, x, float(got[c, y, x]), float(want[c, y, x]), float(dev[c, y, x]) / g)
    if fp16:
        u = (_ord16(got) - _ord16(want)).abs()
        txt += ', %d fp16 ulps (max %d ulps)' % (int(u[c, y, x]), int(u.max()))
    return n, txt + ', max %.3g granules' % (float(dev.max()) / g)


def matches(got, want, case, fp16, premise_ok):
    """The verdict of one output.  premise_ok (the matrix unit adds exactly representable sums exactly -- the premise case):
    bit equality.  Otherwise the fallback written down before any run: fp16 outputs within 1 fp16 ulp and a mismatch share of at
    most 1/8 of control (b) (the smallest defect the case is meant to see); fp32 outputs within 4 granules."""
    n, txt = mismatch(got, want, case.g_out, fp16)
    if premise_ok or n == 0:
        return n == 0, n, txt
    if fp16:
        ok = int((_ord16(got) - _ord16(want)).abs().max()) <= 1 and n / got.numel() <= case.controls[1] / 8.0
    else:
        ok = float((got - want).abs().max()) <= 4 * case.g_out
    return ok, n, txt


# ---- decoders of the packed formats (inverse of refvsr_amd.packing; the table functions are passed in) ----------------------------
def _padded_channels(src_channels):
    """padded-channel index -> real input channel or -1."""
    cmap, base = [], 0
    for c in src_channels:
        cmap += [base + i if i < c else -1 for i in range(pad8(c))]
        base += c
    return cmap


def _from_kblocks(rows_of, kblocks, cout, src_channels, ks=3):
    """w [cout, cin, ks, ks] (float64) from rows_of(i) -> [cout, 8] sums hi + lo of the i-th listed K-block (ty, tx, cg); asserts
    that every K-block of the conv is listed exactly once and that padding channels hold zeros."""
    cmap = _padded_channels(src_channels)
    w = torch.zeros(cout, sum(src_channels), ks, ks, dtype=F64)
    seen = set()
    for i, kb in enumerate(kblocks):
        if kb is None:
            assert not rows_of(i).any(), 'zero K-block holds weights'
            continue
        assert kb not in seen, kb
        seen.add(kb)
        ty, tx, cg = kb
        r = rows_of(i)
        for j in range(8):
            ch = cmap[cg * 8 + j]
            if ch < 0:
                assert not r[:, j].any(), 'padding channel holds weights'
            else:
                w[:, ch, ty, tx] = r[:, j]
    assert len(seen) == ks * ks * len(cmap) // 8, 'K-blocks missing from the packed order'
    return w


def decode_pack_conv(pk, kslot):
    """packing.pack_conv's hi + lo (or hi-only) fragments -> (w, bias) in conv-channel order."""
    wp = pk['wpack'].double()
    nz, S, MT, nh = wp.shape[:4]
    frag = wp.sum(3)                                                    # hi + lo
    full = frag.reshape(nz, S, MT, 4, 16, 8).permute(0, 2, 4, 1, 3, 5).reshape(nz * MT * 16, S * 4, 8)
    ks, cout = pk['ksize'], pk['cout']
    ncg = sum(pk['cpads']) // 8
    kbs = [None] * (S * 4)
    for tap in range(ks * ks):
        for cg in range(ncg):
            kbs[kslot(tap // ks, tap % ks, cg, ks, ncg)] = (tap // ks, tap % ks, cg)
    assert not full[cout:].any()
    w = _from_kblocks(lambda i: full[:cout, i], kbs, cout, pk['src_channels'], ks)
    b = pk['bias'].double()[:cout]
    if pk['shuffle']:                                                   # row r = sub * C + c holds conv channel 4 c + sub
        C = cout // 4
        rows = (torch.arange(cout) % C) * 4 + torch.arange(cout) // C
        w2, b2 = torch.zeros_like(w), torch.zeros_like(b)
        w2[rows], b2[rows] = w, b
        w, b = w2, b2
    return w, b


def _frag_rows(fr, cout, f16w=False):
    """[NF, 4, 16, 8] fragments of one K-step -> [4 quarters][cout, 8] hi + lo sums (the layouts of pack_conv24's docstring)."""
    fr = fr.double()
    if f16w:
        return fr.permute(1, 0, 2, 3).reshape(4, -1, 8)[:, :cout]
    if cout == 24:
        return torch.cat([fr[0] + fr[1], fr[2][:, 0:8] + fr[2][:, 8:16]], 1)
    if cout == 3:
        return fr[0][:, 0:3] + fr[0][:, 8:11]
    return torch.cat([fr[2 * m] + fr[2 * m + 1] for m in range(cout // 16)], 1)


def decode_frags(raw, S, nf, cout, kblock, src_channels, f16w=False):
    """S x nf x 64 x 8 fp16 fragments (uint8 tensor) of the conv24 / resblock24 family -> w; kblock(s, q) -> (ty, tx, cg) | None."""
    fr = torch.from_numpy(raw.numpy().view(np.float16).copy()).reshape(S, nf, 4, 16, 8)
    if cout == 3:                                                       # head: everything outside rows 0-2 / 8-10 of slot 0 is zero
        z = fr.clone()
        z[:, 0, :, 0:3] = 0
        z[:, 0, :, 8:11] = 0
        assert not z.any(), 'head blob holds weights outside rows 0-2 / 8-10 of fragment 0'
    rows = [_frag_rows(fr[s], cout, f16w) for s in range(S)]
    return _from_kblocks(lambda i: rows[i // 4][i % 4], [kblock(i // 4, i % 4) for i in range(4 * S)], cout, src_channels)


def blob_floats(raw):
    return torch.from_numpy(raw.numpy().view(np.float32).copy()).double()


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _conv_case(name, seed, co, cins, ks, hw, stride=1, out='planar', shuffle=False, g_exp=-17, mag_exp=-3, xr=1, run=None, primary='f64',
               lo0=None, act=1.0, post=1.0, mul=False, res=False, res_planar=False, add_const=0.0, clamp=None, xscale=1.0, bias=True):
    g = rng(seed)
    h, w = hw
    cin = sum(cins)
    p = dict(w=dyadic_weights(g, co, cin, ks, g_exp, mag_exp), b=dyadic_vec(g, co) if bias else torch.zeros(co, dtype=F64),
             srcs=[int_map(g, c, h, w, -xr, xr, xscale) for c in cins], stride=stride, out=out, shuffle=shuffle, act=act, post=post,
             add_const=add_const, clamp=clamp)
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
    if mul:
        p['mul'] = pick(g, [0.5, -0.5, 1.0, -1.0, 2.0, -2.0], (co, ho, wo))
    if res:
        p['res'] = int_map(g, co, ho, wo, -4, 4, 0.25)
    if res_planar:
        p['res_planar'] = int_map(g, co, ho, wo, -4, 4, 0.25)
    r = dict(entry='conv', mt=None, hi_only=False, cap=0, generic=True, wfmt='hi_lo')
    r.update(run or {})
    return Case(name, 'conv', r, p, primary, lo0, seed)


def _blocks_case(name, seed, kernel, C, hw, plan, act, post=1.0, g_exp=-17, mag_exp=-3, wfmt='hi_lo', lo0=None, xscale=1.0, xr=1):
    """plan: per block a pair of conv kinds -- 'full' (dyadic, with lo), 'tapA' (one tap, +-1 | +-1/2, dyadic bias), 'tapB' (one tap
    +-1, integer bias), 'null' (W = 0, b = 0)."""
    g = rng(seed)
    h, w = hw

    def make(kind):
        if kind == 'full':
            return dyadic_weights(g, C, C, 3, g_exp, mag_exp), (dyadic_vec(g, C) if xscale == 1.0 else torch.zeros(C, dtype=F64))
        if kind == 'tapA':
            return onetap_weights(g, C, C), (dyadic_vec(g, C) if xscale == 1.0 else torch.zeros(C, dtype=F64))
        if kind == 'tapB':
            return onetap_weights(g, C, C, vals=(1.0, -1.0)), dyadic_vec(g, C, -1, 1, 1.0)
        assert kind == 'null'
        return null_weights(C), torch.zeros(C, dtype=F64)
    blocks = []
    for k1, k2 in plan:
        (w1, b1), (w2, b2) = make(k1), make(k2)
        blocks.append((w1, b1, w2, b2))
    p = dict(x=int_map(g, C, h, w, -xr, xr, xscale), blocks=blocks, act=act, post=post)
    return Case(name, 'blocks', dict(entry=kernel, wfmt=wfmt), p, 'hi' if wfmt == 'fp16' else 'f64', lo0, seed)


CASE_A, CASE_B = [('full', 'tapA')], [('tapB', 'full')]


def _placement(j, c):
    """n = 3 chain with the full conv at block j, conv c: one-tap integer blocks before, identity blocks (W2 = 0, b2 = 0) after."""
    plan = []
    for i in range(3):
        if i < j:
            plan.append(('tapB', 'tapB'))
        elif i == j:
            plan.append(('full', 'tapA') if c == 0 else ('tapB', 'full'))
        else:
            plan.append(('tapB', 'null'))
    return plan


def _conf_case(name, seed, C, hw, want_max=False, wfmt='hi_lo', up=1, staging=False):
    """hw: the confidence maps.  up = 2 has two forms (the hi + lo budget does not fit behind a generic bicubic sample: 2^-16-granule
    samples rounded to fp16, times 2^-17-granule weights):
      K (staging False): the maps hold -64 | 65 in 2 x 2-pixel cells placed at random, so that every up-sampled sample lies outside
        (0, 1) and the clamp makes it exactly 0 or 1 (asserted below on the case's own data) -- from there the up = 1 construction.
      S (staging True): rich maps in {-1, 0, 1}; BOTH convs one-tap with weights +-1 | +-1/2 (lo = 0), the first conv's bias chosen per
        channel so that w P + b0 lies in [1, 2] -- exactly representable in fp32 and never an fp16 subnormal: each output is a
        relocated, rescaled copy of ONE sample rounded once to fp16, every tap, clamp and border of the bicubic shows."""
    g = rng(seed)
    h, w = hw
    run = dict(entry='conf_alpha', want_max=want_max, wfmt=wfmt, up=up)
    if up == 1:
        p = dict(conf_a=int_map(g, 1, h, w), conf_b=int_map(g, 1, h, w), w0=onetap_weights(g, 16, 2), b0=dyadic_vec(g, 16, -1, 1, 0.5),
                 slope0=0.5, w=dyadic_weights(g, C, 16, 3), b=dyadic_vec(g, C), slope1=0.25)
        return Case(name, 'conf_alpha', run, p, 'hi' if wfmt == 'fp16' else 'f64', None, seed)
    assert up == 2 and not want_max
    if not staging:
        cells = lambda: pick(g, [-64.0, 65.0], (1, (h + 1) // 2, (w + 1) // 2)).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w].contiguous()
        p = dict(conf_a=cells(), conf_b=cells(), w0=onetap_weights(g, 16, 2), b0=dyadic_vec(g, 16, -1, 1, 0.5), slope0=0.5,
                 w=dyadic_weights(g, C, 16, 3), b=dyadic_vec(g, C), slope1=0.25, up=2)
        raw = bicubic_up2(torch.cat([p['conf_a'], p['conf_b']], 0), clamp=False)
        assert not ((raw > 0) & (raw < 1)).any(), '%s: an up-sampled sample lies inside (0, 1)' % name
        assert (raw <= 0).any() and (raw >= 1).any()
        return Case(name, 'conf_alpha', run, p, 'hi' if wfmt == 'fp16' else 'f64', None, seed)
    w0 = onetap_weights(g, 16, 2)
    v0 = w0.sum((1, 2, 3))                                            # the one weight of each output channel
    b0 = torch.where(v0 == -1.0, 2.0, torch.where(v0 == -0.5, 1.5, 1.0)).to(F64)
    p = dict(conf_a=int_map(g, 1, h, w), conf_b=int_map(g, 1, h, w), w0=w0, b0=b0, slope0=0.5, w=onetap_weights(g, C, 16), b=dyadic_vec(g, C),
             slope1=0.25, up=2)
    return Case(name, 'conf_alpha', run, p, 'hi' if wfmt == 'fp16' else 'f64', 'drop_hi', seed)


def conf_up2_classes(p):
    """(samples clamped at 0, clamped at 1, strictly between) of an up = 2 case, with the proof that the fp32 bicubic is exact on its
    maps: float32 equals float64, rows first equals columns first."""
    P = torch.cat([p['conf_a'], p['conf_b']], 0)
    raw = bicubic_up2(P, clamp=False)
    for T in (np.float32, np.float64):
        for tr in (False, True):
            assert torch.equal(bicubic_up2(P, T, clamp=False, transposed=tr), raw), 'the bicubic is not exact on this case (%s, transposed %s)' % (T.__name__, tr)
    return int((raw <= 0).sum()), int((raw >= 1).sum()), int(((raw > 0) & (raw < 1)).sum())


def base_map(g, bhw, vals):
    """float64 [3, bh, bw] from `vals`, the three planes drawn separately (so that a wrong plane shows); a 1 x 1 map takes three
    different values."""
    bh, bw = bhw
    if bh * bw == 1:
        return torch.tensor(vals, dtype=F64)[torch.randperm(len(vals), generator=g)[:3]].reshape(3, 1, 1)
    return torch.stack([pick(g, vals, (bh, bw)) for _ in range(3)])


def byte_map(g, bhw):
    """float64 [3, bh, bw] holding the float32 numbers byte / 255 of random bytes: what ingest_u8 hands the head."""
    return (torch.randint(0, 256, (3,) + tuple(bhw), generator=g).float() / 255.0).double()


BASED_BIAS = (0.0, -0.0625, 0.0625)         # with a base in [0, 1] on top, a conv centred at 0 keeps all three output classes filled


def _with_base(g, p, hw, base):
    """base: None | (s, 'u' | 's' of BASE_SETS | 'bytes'); drawn AFTER everything else, so that the zero-base cases keep their data."""
    if base is not None:
        s, vals = base
        assert hw[0] % s == 0 and hw[1] % s == 0, (hw, s)
        bhw = (hw[0] // s, hw[1] // s)
        p.update(s=s, base=byte_map(g, bhw) if vals == 'bytes' else base_map(g, bhw, BASE_SETS[vals]))
    return p


def _last_case(name, seed, C, hw, lo0=None, g_exp=-17, mag_exp=-3, xr=1, base=None):
    g = rng(seed)
    h, w = hw
    b = torch.tensor([0.5, 0.4375, 0.5625], dtype=F64) if lo0 is None else torch.tensor([2.0 ** -9, 0.0, 2.0 ** -10], dtype=F64)
    if base is not None:
        b = torch.tensor(BASED_BIAS, dtype=F64)
    p = dict(x=int_map(g, C, h, w, -xr, xr), w=dyadic_weights(g, 3, C, 3, g_exp, mag_exp), b=b)
    return Case(name, 'conv_last', dict(entry='conv_last'), _with_base(g, p, hw, base), 'f64', lo0, seed)


def _hr_case(name, seed, hw, which, act, base=None, b_count=CTL_B_COUNT):
    g = rng(seed)
    h, w = hw
    if which == 'A':
        w1, b1 = dyadic_weights(g, 24, 24, 3), dyadic_vec(g, 24)
        w2, b2 = onetap_weights(g, 3, 24), torch.tensor([0.5, 0.25, 0.75], dtype=F64)
    else:
        w1, b1 = onetap_weights(g, 24, 24, vals=(1.0, -1.0)), dyadic_vec(g, 24, -1, 1, 1.0)
        w2, b2 = dyadic_weights(g, 3, 24, 3), torch.tensor([0.5, 0.4375, 0.5625], dtype=F64)
    if base is not None:
        b2 = torch.tensor(BASED_BIAS, dtype=F64)
    p = dict(x=int_map(g, 24, h, w), w1=w1, b1=b1, w2=w2, b2=b2, act=act)
    return Case(name, 'hr_last', dict(entry='hr_last'), _with_base(g, p, hw, base), 'f64', None, seed, b_count)


# ---- the based head cases: proofs and controls, from the reference alone -----------------------------------------------------------
def base_proof(p):
    """The unclamped bicubic sample of a based case's map, with the proof that the fp32 evaluation is exact on it: float32 equals
    float64, rows first equals columns first, and every sample lies on the 2^-24 grid."""
    proxy = dict(p, ctl='noclamp')
    raw = head_base(proxy, np.float64, 'noclamp')
    for T in (np.float32, np.float64):
        for tr in (False, True):
            assert torch.equal(head_base(proxy, T, 'noclamp', tr), raw), 'the bicubic is not exact on this map (%s, transposed %s)' % (T.__name__, tr)
    assert torch.equal((raw * 2.0 ** 24).round(), raw * 2.0 ** 24), 'a sample lies off the 2^-24 grid'
    return raw


def _count3(t):
    return int((t <= 0).sum()), int((t >= 1).sum()), int(((t > 0) & (t < 1)).sum())


def head_classes(c):
    """Class counts of a based case: samples (clamped at 0, clamped at 1, strictly inside), outputs (at 0, at 1, inside), and the
    outputs inside (0, 1) whose base sample was clamped -- the ones a missing first clamp changes."""
    raw, out = base_proof(c.p), c.want['out']
    inside = (out > 0) & (out < 1)
    return dict(samples=_count3(raw), outputs=_count3(out), inside_clamped=int((inside & ((raw < 0) | (raw > 1))).sum()))


def _clamped_taps(n_in, s):
    """(low, high): bool per output index -- a tap of its 4-tap window was clamped onto index 0 | n_in - 1."""
    o = np.arange(n_in * s)
    fl = np.floor((o + 0.5) / s - 0.5).astype(np.int64)
    return torch.from_numpy(fl - 1 < 0), torch.from_numpy(fl + 2 > n_in - 1)


BORDERS = ('top', 'bottom', 'left', 'right', 'top-left', 'top-right', 'bottom-left', 'bottom-right')


def head_borders(c):
    """{border | corner: outputs there (any channel) whose taps were index-clamped AND whose reference value lies strictly inside
    (0, 1)}: a stray value read there -- a fence's NaN included, which the clamps would turn into 0 -- changes such an output."""
    out, s = c.want['out'], c.p['s']
    inside = ((out > 0) & (out < 1)).any(0)
    (t, b), (le, r) = _clamped_taps(c.p['base'].shape[1], s), _clamped_taps(c.p['base'].shape[2], s)
    ones_y, ones_x = torch.ones_like(t), torch.ones_like(le)
    sets = dict(zip(BORDERS, ((t, ones_x), (b, ones_x), (ones_y, le), (ones_y, r), (t, le), (t, r), (b, le), (b, r))))
    return dict((k, int((inside & (ry[:, None] & rx[None, :])).sum())) for k, (ry, rx) in sets.items())


def base_control(c, ctl):
    """Outputs of the case that change when the reference's base term carries the defect `ctl` (head_base)."""
    mutated = REFS[c.kind](Arith('f64', c.block), dict(c.p, ctl=ctl))[0]['out']
    return int((mutated != c.want['out']).sum())


# ---- the general family: a base of bytes / 255 behind exact conv operands ---------------------------------------------------------
# rv_bicubic_at on data that is NOT exact: the cubic weights are still exact (dyadic t), each of the 16 row fmaf rounds a partial
# sum of magnitude <= sum |w| max |x| < 2 (half an ulp: 2^-24), their errors reach the sample through the column weights, sum |wy|
# = 1.375 at most: 4 x 1.375 = 5.5 x 2^-24; the 4 column fmaf round partial sums <= (sum |w|)^2 max |x| = 1.890625 < 2: 4 x 2^-24.
# The clamp widens nothing, v is exact, and the fp32 add rounds a result that is kept only inside [0, 1]: 2^-25.  Against the
# float64 reference (which rounds nothing): 5.5 + 4 + 0.5 = 10 x 2^-24.
GENERAL_BOUND = 10.0 * 2.0 ** -24
GENERAL_CAP = 0.01


class GeneralCase(object):
    """A head case whose base is bytes / 255.  want = clamp(v + clamp01(bicubic(base)), 0, 1) in float64 with NO rounding (v, the conv,
    is exact); a kernel's fp32 value lies within GENERAL_BOUND of it (derivation above; checked on the CPU against the reference's
    own float32 replay, never taken from a GPU result).  The stores are monotone, so a stored fp16 | uint8 value lies between the
    stores of want - bound and want + bound: allowed(fmt) -> (lo, hi); where lo != hi (255 want within 255 bound of a half-integer,
    for uint8) the result may differ by one step, nowhere else, and that set is capped at GENERAL_CAP of the elements."""

    def __init__(self, name, case):
        self.name, self.case, self.kind, self.p = name, case, case.kind, case.p
        self.v = self._conv()
        self.pre = self.v + head_base(self.p, np.float64)           # before the last clamp: the interval is clamped, not widened at 0 | 1
        self.want = self.pre.clamp(0.0, 1.0)

    def _conv(self):
        """conv + bias of the head (hr_last: of fp16(lrelu(conv_hr))), exact under the condition: float64 holding fp32 numbers."""
        A, p = Arith('f64'), self.p
        if self.kind == 'conv_last':
            y = A.conv(p['x'], p['w'], p['b'])
        else:
            y = A.conv(A.conv(p['x'], p['w1'], p['b1']).lrelu(p['act']).half(), p['w2'], p['b2'])
        assert A.bound < LIMIT and torch.equal(y.v.float().double(), y.v), self.name
        return y.v

    @staticmethod
    def store(v, fmt):
        """float64 values in [0, 1] -> the fp32 | fp16 | uint8 store of rv_store_result, as float64."""
        v32 = v.float()
        if fmt == 'float16':
            return v32.half().double()
        if fmt == 'uint8':
            return (v32 * 255.0).round().double()
        return v32.double()

    def allowed(self, fmt):
        lo, hi = (self.pre - GENERAL_BOUND).clamp(0.0, 1.0), (self.pre + GENERAL_BOUND).clamp(0.0, 1.0)
        if fmt in (None, 'float32'):
            return lo, hi
        return self.store(lo, fmt), self.store(hi, fmt)

    def loose(self, fmt):
        """Share of the elements at which the stored format leaves a choice."""
        lo, hi = self.allowed(fmt)
        return float((lo != hi).double().mean())

    def replay32(self, transposed=False):
        """The reference's own float32 replay: fp32 bicubic (either summation order), fp32 clamp, ONE fp32 add, clamp."""
        b = head_base(self.p, np.float32, None, transposed)
        return (self.v.float() + b.float()).clamp(0.0, 1.0).double()


def _hw(s):
    return '%dx%d' % s


def _table():
    T = {}

    def add(fn, name, *a, **k):
        assert name not in T, name
        T[name] = functools.partial(fn, name, 1000 + len(T) + 7919 * k.pop('reseed', 0), *a, **k)
    spec = dict(generic=False)
    # -- premise: fp16-representable weights (lo = 0) on the generic kernel, fp32 planar output
    add(_conv_case, 'premise conv_mfma 24->24 3x3 19x45 lo=0', 24, [24], 3, L19, g_exp=-13, lo0='drop_hi')
    # -- generic refvsr_conv_mfma, hi + lo weights, fp32 planar output: the kernel-selecting shapes
    add(_conv_case, 'conv_mfma [24]->24 3x3 19x45', 24, [24], 3, L19)
    add(_conv_case, 'conv_mfma [24]->24 3x3 7x5', 24, [24], 3, S7)
    add(_conv_case, 'conv_mfma [3,24]->24 3x3 8x32', 24, [3, 24], 3, T8)
    add(_conv_case, 'conv_mfma [24,24]->24 3x3 19x45', 24, [24, 24], 3, L19)
    add(_conv_case, 'conv_mfma [48]->48 3x3 19x45', 48, [48], 3, L19)
    add(_conv_case, 'conv_mfma [24]->24 3x3 s2 19x45', 24, [24], 3, L19, stride=2)
    add(_conv_case, 'conv_mfma [3]->32 5x5 19x45', 32, [3], 5, L19, xr=2)
    add(_conv_case, 'conv_mfma [32,32]->32 5x5 s2 19x45', 32, [32, 32], 5, L19, stride=2, mag_exp=-4)
    add(_conv_case, 'conv_mfma [24,24]->24 1x1 8x32', 24, [24, 24], 1, T8, xr=2)
    add(_conv_case, 'conv_mfma [8]->32 7x7 19x45', 32, [8], 7, L19)
    for co, ci, hw in ((64, 32, (9, 15)), (32, 64, (18, 30))):
        for mt in (1, 2):
            for hi_only in (False, True):
                add(_conv_case, 'conv_mfma streamed [%d]->%d 7x7 %s mt%d%s' % (ci, co, _hw(hw), mt, ' fp16 weights' if hi_only else ''), co, [ci], 7, hw,
                    mag_exp=-4 if ci == 32 else -5, run=dict(mt=mt, hi_only=hi_only), primary='hi' if hi_only else 'f64')
    add(_conv_case, 'conv_mfma gather [32,32]->32 5x5 s4 37x50', 32, [32, 32], 5, (37, 50), stride=4, mag_exp=-4)
    add(_conv_case, 'conv_mfma walk cap=8 [24]->24 3x3 33x70', 24, [24], 3, (33, 70), run=dict(cap=8))
    # -- stores of the generic kernel: fp16 HWC (C = 36 in a stride of 40), pixel shuffle
    add(_conv_case, 'conv_mfma nhwc16 [24]->24 3x3 7x5', 24, [24], 3, S7, out='nhwc')
    add(_conv_case, 'conv_mfma nhwc16 [24]->36 3x3 19x45', 36, [24], 3, L19, out='nhwc')
    add(_conv_case, 'conv_mfma shuffle [24]->96 3x3 19x45', 96, [24], 3, L19, out='nhwc', shuffle=True)
    add(_conv_case, 'conv_mfma shuffle [36]->144 3x3 7x5', 144, [36], 3, S7, out='nhwc', shuffle=True)
    add(_conv_case, 'conv_mfma shuffle [36]->144 3x3 19x45', 144, [36], 3, L19, out='nhwc', shuffle=True)
    # -- epilogue of the generic kernel: lean (fp16 HWC, slopes in [0, 1]) and full (planar)
    add(_conv_case, 'conv_mfma epi act0', 24, [24], 3, L19, out='nhwc', act=0.0)
    add(_conv_case, 'conv_mfma epi act1 post0', 24, [24], 3, L19, out='nhwc', act=1.0, post=0.0)
    add(_conv_case, 'conv_mfma epi act.5 mul', 24, [24], 3, L19, out='nhwc', act=0.5, mul=True)
    add(_conv_case, 'conv_mfma epi res post.25', 24, [24], 3, L19, out='nhwc', res=True, post=0.25)
    add(_conv_case, 'conv_mfma epi act.25 mul res post.5', 24, [24], 3, L19, out='nhwc', act=0.25, mul=True, res=True, post=0.5, g_exp=-15)
    add(_conv_case, 'conv_mfma epi planar act0 res_planar', 24, [24], 3, L19, act=0.0, res_planar=True)
    add(_conv_case, 'conv_mfma epi planar add_const clamp', 24, [24], 3, L19, add_const=1.0, clamp=(0.5, 1.5))
    add(_conv_case, 'conv_mfma epi planar everything', 24, [24], 3, L19, act=0.25, mul=True, res=True, post=0.5, res_planar=True,
        add_const=0.25, clamp=(-1.0, 1.0), g_exp=-15)
    # -- refvsr_conv24: every input combination of test_conv24_specialised, every epilogue term
    add(_conv_case, 'conv24 [24] 19x45 act.25', 24, [24], 3, L19, out='nhwc', act=0.25, run=spec)
    add(_conv_case, 'conv24 [24] 8x32 act0', 24, [24], 3, T8, out='nhwc', act=0.0, run=spec)
    add(_conv_case, 'conv24 [24] 7x5 act1 mul', 24, [24], 3, S7, out='nhwc', mul=True, run=spec)
    add(_conv_case, 'conv24 [24] 19x45 act.5 mul res', 24, [24], 3, L19, out='nhwc', act=0.5, mul=True, res=True, run=spec)
    add(_conv_case, 'conv24 [16] 19x45 act.25', 24, [16], 3, L19, out='nhwc', act=0.25, run=spec)
    add(_conv_case, 'conv24 [3,24] 8x32 act.5', 24, [3, 24], 3, T8, out='nhwc', act=0.5, run=spec)
    add(_conv_case, 'conv24 [3,24] 19x45 act.25', 24, [3, 24], 3, L19, out='nhwc', act=0.25, run=spec)
    add(_conv_case, 'conv24 [24,24] 7x5 res post.25', 24, [24, 24], 3, S7, out='nhwc', res=True, post=0.25, run=spec)
    add(_conv_case, 'conv24 [24,24] 19x45 act.25', 24, [24, 24], 3, L19, out='nhwc', act=0.25, run=spec)
    # -- refvsr_conv32
    add(_conv_case, 'conv32 [32] 19x45 act.25', 32, [32], 3, L19, out='nhwc', act=0.25, run=spec)
    add(_conv_case, 'conv32 [32] 7x5 res post.25', 32, [32], 3, S7, out='nhwc', res=True, post=0.25, run=spec)
    add(_conv_case, 'conv32 [3] 19x45 act.25', 32, [3], 3, L19, out='nhwc', act=0.25, xr=2, run=spec)
    # -- refvsr_conv48: one source, the 48 + 48 channel-half form, the 8 + 48 input conv, 16 -> 48
    add(_conv_case, 'conv48 [48] 16x32 res', 48, [48], 3, T16, out='nhwc', res=True, run=spec)
    add(_conv_case, 'conv48 [48] 19x45 act0', 48, [48], 3, L19, out='nhwc', act=0.0, run=spec)
    add(_conv_case, 'conv48 [48] 7x5 act.25 res', 48, [48], 3, S7, out='nhwc', act=0.25, res=True, run=spec)
    add(_conv_case, 'conv48 [16] 19x45 act.25', 48, [16], 3, L19, out='nhwc', act=0.25, run=spec)
    add(_conv_case, 'conv48 [48,48] 19x45 act.25', 48, [48, 48], 3, L19, out='nhwc', act=0.25, mag_exp=-4, run=spec)
    add(_conv_case, 'conv48 [3,48] 19x45 act.25', 48, [3, 48], 3, L19, out='nhwc', act=0.25, run=spec)
    # -- refvsr_conv_shuffle2
    add(_conv_case, 'conv_shuffle2 C24 7x5 act1', 96, [24], 3, S7, out='nhwc', shuffle=True, run=spec)
    add(_conv_case, 'conv_shuffle2 C24 19x45 act.25', 96, [24], 3, L19, out='nhwc', shuffle=True, act=0.25, run=spec)
    add(_conv_case, 'conv_shuffle2 C48 8x32 act.25', 192, [48], 3, T8, out='nhwc', shuffle=True, act=0.25, run=spec)
    add(_conv_case, 'conv_shuffle2 C48 19x45 act1', 192, [48], 3, L19, out='nhwc', shuffle=True, run=spec)
    # -- refvsr_conf_alpha, up = 1
    add(_conf_case, 'conf_alpha C24 19x45 max', 24, L19, want_max=True)
    add(_conf_case, 'conf_alpha C24 7x5', 24, S7)
    add(_conf_case, 'conf_alpha C48 8x32 max', 48, T8, want_max=True)
    add(_conf_case, 'conf_alpha C48 19x45', 48, L19)
    # -- the output head
    add(_last_case, 'conv_last C24 19x45', 24, L19)
    add(_last_case, 'conv_last C24 7x5', 24, S7)
    add(_last_case, 'conv_last C48 8x32', 48, T8)
    add(_last_case, 'conv_last C48 19x45', 48, L19)
    for which in 'AB':
        for hw, act in ((S7, 0.5), (T8, 1.0), (L19, 0.25)):
            add(_hr_case, 'conv_hr_last %s %s act%g' % (which, _hw(hw), act), hw, which, act, reseed=9 * int(which == 'A' and hw == S7))       # (3 x 7 x 5 outputs: a seed whose control (b) reaches 8 elements)
    # -- fused blocks: cases A and B, slopes 0.0 and 0.25
    for nm, plan in (('A', CASE_A), ('B', CASE_B)):
        for act in (0.0, 0.25):
            for hw in (S7, T8, L19):
                add(_blocks_case, 'resblock24 %s %s act%g' % (nm, _hw(hw), act), 'rb24', 24, hw, plan, act)
            for hw in (T8, L19):
                add(_blocks_case, 'resblock48 %s %s act%g' % (nm, _hw(hw), act), 'rb48', 48, hw, plan, act, mag_exp=-4)
            add(_blocks_case, 'resblock_chain %s 19x45 act%g' % (nm, act), 'chain', 24, L19, plan, act)
        for C in (8, 16, 24, 32):
            for post in (1.0, 0.5):
                add(_blocks_case, 'resblock_lean C%d %s post%g act%g' % (C, nm, post, 0.25 if post == 1.0 else 0.0), 'lean', C, L19, plan,
                    0.25 if post == 1.0 else 0.0, post, mag_exp=-2 if C == 8 else -3)
    # -- n = 3 chains: the full conv at block j, conv c
    for kern, C, hw, me in (('rb24', 24, L19, -3), ('rb48', 48, T8, -4), ('chain', 24, L19, -3)):
        for j in range(3):
            for c in range(2):
                add(_blocks_case, '%s n3 full at block %d conv %d' % ({'rb24': 'resblock24', 'rb48': 'resblock48', 'chain': 'resblock_chain'}[kern], j, c + 1),
                    kern, C, hw, _placement(j, c), 0.0, mag_exp=me)
    # -- _f16w twins: the same kind of weights (with a lo part); the twin computes with fp16(w), the hi + lo entry point with w
    tw = dict(generic=False, wfmt='fp16')
    add(_conv_case, 'f16w conv24 [24] 19x45 act.25', 24, [24], 3, L19, out='nhwc', act=0.25, run=tw, primary='hi')
    add(_conv_case, 'f16w conv24 [3,24] 8x32 act.5 res', 24, [3, 24], 3, T8, out='nhwc', act=0.5, res=True, run=tw, primary='hi')
    add(_conv_case, 'f16w conv32 [32] 19x45 act.25', 32, [32], 3, L19, out='nhwc', act=0.25, run=tw, primary='hi')
    add(_conv_case, 'f16w conv_shuffle2 C24 19x45 act.25', 96, [24], 3, L19, out='nhwc', shuffle=True, act=0.25, run=tw, primary='hi')
    add(_blocks_case, 'f16w resblock24 A 19x45 act0', 'rb24', 24, L19, CASE_A, 0.0, wfmt='fp16')
    add(_blocks_case, 'f16w resblock24 B 19x45 act.25', 'rb24', 24, L19, CASE_B, 0.25, wfmt='fp16')
    add(_conf_case, 'f16w conf_alpha C24 19x45', 24, L19, wfmt='fp16')
    # -- fp16-subnormal hi operands: |w| < 2^-14 on the 2^-24 granule (every weight an fp16 subnormal, lo = 0), integer maps up to +-8
    add(_conv_case, 'subnormal conv_mfma [24]->24 3x3 19x45', 24, [24], 3, L19, g_exp=-24, mag_exp=-14, xr=8, lo0='flush', bias=False)
    add(_conv_case, 'subnormal conv24 [24] 19x45', 24, [24], 3, L19, out='nhwc', g_exp=-24, mag_exp=-14, xr=8, lo0='flush', bias=False, run=spec)
    add(_blocks_case, 'subnormal resblock24 19x45', 'rb24', 24, L19, CASE_A, 0.0, g_exp=-24, mag_exp=-14, lo0='flush', xscale=2.0 ** -10, xr=8)
    add(_last_case, 'subnormal conv_last C24 19x45', 24, L19, lo0='flush', g_exp=-24, mag_exp=-14, xr=8)
    # -- the output head with a NON-ZERO base frame (appended: the seeds above follow the table's order)
    for s, hw, vals in BASED_SHAPES:
        for C in (24, 48):
            add(_last_case, 'based conv_last C%d x%d %s' % (C, s, _hw(hw)), C, hw, base=(s, vals))
        for which in 'AB':
            # (form A at 4 x 4: one K-block's lo term moves the fp16 map between the convs at too few of 48 outputs for control (b)'s
            # count of 8 -- the best of 120 seeds reaches 7, taken here with a count of 6; the case is there for the base, and form
            # A's convs are held to the full count at the four other shapes)
            tiny_a = which == 'A' and hw == (4, 4)
            add(_hr_case, 'based conv_hr_last %s x%d %s' % (which, s, _hw(hw)), hw, which, 0.25, base=(s, vals), reseed=54 * int(tiny_a),
                b_count=6 if tiny_a else CTL_B_COUNT)
    return T


# (factor, output shape, value set): partial 8x32 and 16x32 tiles | exactly one 8x32 tile | every tap clamps onto the one sample |
# partial tiles | below one tile
BASED_SHAPES = ((4, (20, 44), 'u'), (4, (8, 32), 's'), (4, (4, 4), 'u'), (2, (18, 46), 's'), (2, (14, 6), 'u'))
TABLE = _table()
NAMES = list(TABLE)
PREMISE = NAMES[0]
BASED = [n for n in NAMES if n.startswith('based')]
_CACHE = {}


def _general_table():
    G = {}
    for k, (kind, a, s, hw) in enumerate((('conv_last', 24, 4, (20, 44)), ('conv_last', 48, 2, (18, 46)), ('hr_last', 'B', 4, (20, 44)),
                                          ('hr_last', 'A', 2, (18, 46)))):
        name = 'general %s %s x%d %s' % ('conv_last C%d' % a if kind == 'conv_last' else 'conv_hr_last %s' % a, 'bytes', s, _hw(hw))
        if kind == 'conv_last':
            G[name] = functools.partial(_last_case, name, 5000 + k, a, hw, base=(s, 'bytes'))
        else:
            G[name] = functools.partial(_hr_case, name, 5000 + k, hw, a, 0.25, base=(s, 'bytes'))
    return G


GENERAL = _general_table()
GENERAL_NAMES = list(GENERAL)


def get_general(name):
    if name not in _CACHE:
        _CACHE[name] = GeneralCase(name, GENERAL[name]())
    return _CACHE[name]


def get_case(name):
    """The case of that name, built once per process (inputs, reference and controls are shared by every test that asks)."""
    if name not in _CACHE:
        _CACHE[name] = TABLE[name]()
    return _CACHE[name]
