"""Exact-arithmetic parity of the hi + lo conv kernels on a real MI355X: every case of tests/exact_cases.py is fed to its kernel and
the result must equal the float64 reference BIT FOR BIT (torch.equal on the fp16 or fp32 values).

The inputs are chosen (and checked on the CPU, tests/test_exact_cases.py) so that every product and every partial sum a kernel can
form is an fp32 number: summation order, MFMA shape and hi / lo fold order cannot change the accumulator, an fp16 store is one
round-to-nearest-even of an exact number, and a kernel that loses the lo term of ONE 8-channel K-block of ONE tap changes at least
1 % (and at least 8) of the outputs -- control (b) of each case, printed in its report line next to control (a) (every lo term
dropped) and the exactness bound in log2 granules.  Almost every lo value of these weights is an fp16 SUBNORMAL, as in real
checkpoints (packing.py stores lo = fp16(w - hi) unscaled): the whole weight path depends on the MFMA taking fp16 subnormal
operands unflushed, which the `subnormal` cases pin for the hi operand too.

The output heads run with a zero base frame (the conv and the stores alone) and, in the `based` cases, with a non-zero base at x4
and x2 whose bicubic sample is exact: those go through all three routes of engine.compute_up in every result format and layout,
each launch twice (plain and fenced), and the `general` cases (base = bytes / 255) are held to a derived bound
(profiles/gpu_head_base_report.txt).

Multi-map, batched, workgroup-shape and store-mode variants are pinned bit-identical to the single launches by test_gpu_ops.py;
each family is anchored here once.

If the premise case fails (the matrix unit does not add exactly representable sums exactly), that is a finding about the hardware,
not a kernel bug: the other cases then follow the fallback rule of exact_cases.matches (fp16 outputs within one ulp on at most 1/8
of control (b)'s share, fp32 outputs within 4 granules).  On the MI355X the premise holds and every case is bit-equal
(profiles/gpu_exact_parity_report.txt, which also records a packing mutation that these tests catch)."""
import os

import pytest
import torch

import exact_cases as ec
from exact_cases import get_case
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(OPS_REPORT), 'gpu_exact_report.txt')       # next to test_gpu_ops.py's report, in its git-ignored folder


def report(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, 'a') as f:
            f.write(line + '\n')
    except OSError:
        pass


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


# ---- feeding the kernels ---------------------------------------------------------------------------------------------------------
def nhwc16(x, dev, cs=None):
    """float64 [C, H, W] of fp16 numbers -> device fp16 [H, W, Cs] (channel padding zero), built with torch alone."""
    c, h, w = x.shape
    t = torch.zeros(h, w, cs or ec.pad8(c), dtype=torch.float16)
    t[:, :, :c] = x.permute(1, 2, 0).to(torch.float16)
    assert torch.equal(t[:, :, :c].double(), x.permute(1, 2, 0)), 'input map is not fp16-representable'
    return t.to(dev)


def planar64(t, c):
    """device fp16 [H, W, Cs] -> float64 [c, H, W]; the channel padding must hold zeros."""
    t = t.cpu()
    assert not t[:, :, c:].any(), 'channel padding of the output map is not zero'
    return t[:, :, :c].permute(2, 0, 1).double().contiguous()


def f32(t, dev=None):
    t = t.float().contiguous()
    return t.to(dev) if dev is not None else t


def conv_weights(w, b, cins, dev, shuffle=False, mt=None, hi_only=False, wfmt='hi_lo', generic=False):
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv
    cw = ops.ConvWeights(pack_conv(f32(w), f32(b), cins, shuffle, mt=mt, hi_only=hi_only), dev, wfmt)
    if generic:
        cw.blob24 = None                                   # refvsr_conv_mfma for the shapes the specialised kernels serve as well
    else:
        assert cw.blob24 is not None, 'no specialised kernel for this shape'
        if wfmt == 'fp16' and (cw.cout in (24, 32) or (shuffle and cins == [24])):
            assert cw.blob_wfmt == 'fp16'
    return cw


def run_conv(c, dev, wfmt=None):
    from refvsr_amd import hip, ops
    p, r = c.p, c.run
    cins = [s.shape[0] for s in p['srcs']]
    co = p['w'].shape[0]
    cw = conv_weights(p['w'], p['b'], cins, dev, p['shuffle'], r['mt'], r['hi_only'], wfmt or r['wfmt'], r['generic'])
    srcs = [nhwc16(s, dev) for s in p['srcs']]
    kw = dict(stride=p['stride'], act=p['act'], post=p['post'])
    if p.get('mul') is not None:
        kw['mul'] = nhwc16(p['mul'], dev)
    if p.get('res') is not None:
        kw['res'] = nhwc16(p['res'], dev)
    if p['out'] == 'planar':
        kw.update(planar_out=True, add_const=p['add_const'], clamp=p['clamp'])
        if p.get('res_planar') is not None:
            kw['res_planar'] = f32(p['res_planar'], dev)
    if r['cap']:
        hip.lib().refvsr_set_conv_workgroup_cap(r['cap'])  # persistent walk: every workgroup takes several tiles
    try:
        got = ops.conv(cw, srcs[0], srcs[1] if len(srcs) > 1 else None, **kw)
        torch.cuda.synchronize()
    finally:
        if r['cap']:
            hip.lib().refvsr_set_conv_workgroup_cap(0)
    if p['out'] == 'planar':
        assert got.dtype == torch.float32
        return {'out': got.cpu().double()}
    assert got.dtype == torch.float16
    if p['shuffle']:
        assert got.shape[2] == ec.pad8(co // 4)
        return {'out': planar64(got, co // 4)}
    assert got.shape[2] == ec.pad8(co)
    return {'out': planar64(got, co)}


def run_blocks(c, dev, wfmt=None):
    from refvsr_amd import ops
    p, kern = c.p, c.run['entry']
    wfmt = wfmt or c.run['wfmt']
    C = p['x'].shape[0]
    x = nhwc16(p['x'], dev)
    x0 = x.clone()
    raw = [((f32(w1), f32(b1)), (f32(w2), f32(b2))) for (w1, b1, w2, b2) in p['blocks']]
    if kern == 'rb24':
        got = ops.resblock24_chain(ops.Resblock24Chain(raw, dev, wfmt), x, p['act'])
    elif kern == 'rb48':
        got = ops.resblock48_chain(ops.Resblock48Chain(raw, dev), x, p['act'])
    else:
        pairs = [tuple(conv_weights(w, b, [C], dev, generic=True) for (w, b) in blk) for blk in raw]
        if kern == 'lean':
            assert len(pairs) == 1 and ops.resblock_fits(C)
            got = ops.resblock(pairs[0][0], pairs[0][1], x, p['act'], p['post'])
        else:
            assert ops.resblock_chain_ok(C)
            got = ops.resblock_chain(ops.ResblockChain(pairs), x, p['act'], p['post'])
    assert torch.equal(x, x0), 'the input map was written to'
    return {'out': planar64(got, C)}


def run_conf_alpha(c, dev, wfmt=None):
    from refvsr_amd import ops
    p = c.p
    cw = conv_weights(p['w'], p['b'], [16], dev, wfmt=wfmt or c.run['wfmt'])
    out = ops.conf_alpha(f32(p['conf_a'], dev), f32(p['conf_b'], dev), 1, f32(p['w0'], dev), f32(p['b0'], dev), cw, p['slope0'], p['slope1'],
                         want_max=c.run['want_max'])
    if c.run['want_max']:
        return {'out': planar64(out[0], cw.cout), 'cmax': out[1].cpu().double()}
    return {'out': planar64(out, cw.cout)}


ROUTES = ('conv_last', 'hr_last', 'fallback')
FORMATS = (None, 'float16', 'uint8')


def routes_of(c):
    """The routes of engine.compute_up a head case can take: the fused tail only where the case has a conv_hr."""
    return ROUTES if c.kind == 'hr_last' else (ROUTES[0], ROUTES[2])


def run_head(c, dev, result_dtype=None, result_layout=None, route=None, fenced=False):
    """One head case through one of the three routes by which engine.compute_up returns a frame:
      'conv_last'  ops.conv_last (an hr_last case: behind ops.conv(conv_hr, act), engine.py:929)
      'hr_last'    ops.conv_hr_last, the fused tail
      'fallback'   ops.bicubic_scale + the planar ops.conv with res_planar and clamp + ops.convert_result (engine.py:934-935)
    route None: the case's own entry point.  The base is the case's (a zero map of the output's size for the zero-base cases: its
    bicubic sample is exactly 0).  fenced: every input (the base included) between the NaN fences of tests/footprint.py, every
    allocation of ops between 0xA5 fences -> (result, footprint.judge's verdict without the comparison to a plain run)."""
    import footprint as fp
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv, pack_conv_hr_last, pack_conv_last
    p = c.p
    route = route or c.run['entry']
    assert route in routes_of(c), (c.name, route)
    put = (lambda t: fp.fenced_input(t.cpu(), dev, 'nan')) if fenced else (lambda t: t.to(dev))
    weights = (lambda cw: fp.fence_weights(cw)) if fenced else (lambda cw: cw)
    if fenced:
        fp.reset_inputs()
    x = put(nhwc16(p['x'], 'cpu'))
    base = put(f32(p['base']) if p.get('base') is not None else torch.zeros(3, x.shape[0], x.shape[1]))
    if route == 'hr_last':
        blob = put(pack_conv_hr_last(f32(p['w1']), f32(p['b1']), f32(p['w2']), f32(p['b2'])))
        launch = lambda: ops.conv_hr_last(blob, x, base, p['act'], result_dtype, result_layout)
    else:
        w, b = (p['w2'], p['b2']) if c.kind == 'hr_last' else (p['w'], p['b'])
        cw_hr = weights(conv_weights(p['w1'], p['b1'], [24], dev)) if c.kind == 'hr_last' else None
        src = lambda: ops.conv(cw_hr, x, act=p['act']) if cw_hr is not None else x
        if route == 'conv_last':
            blob = put(pack_conv_last(f32(w), f32(b)))
            launch = lambda: ops.conv_last(blob, src(), base, result_dtype, result_layout)
        else:
            cw = weights(ops.ConvWeights(pack_conv(f32(w), f32(b), [w.shape[1]]), dev))
            s = x.shape[0] // base.shape[1]
            launch = lambda: ops.convert_result(ops.conv(cw, src(), planar_out=True, res_planar=ops.bicubic_scale(base, s, clamp01=True),
                                                         clamp=(0.0, 1.0)), result_dtype, result_layout)
    if not fenced:
        return launch().cpu()
    try:
        with fp.fenced_outputs(ops) as fo:
            got = launch()
            verdict = fp.judge(fo, [got])
    finally:
        fp.reset_inputs()
    return got.cpu(), verdict


def run_case(c, dev, wfmt=None):
    if c.kind == 'conv':
        return run_conv(c, dev, wfmt)
    if c.kind == 'blocks':
        return run_blocks(c, dev, wfmt)
    if c.kind == 'conf_alpha':
        return run_conf_alpha(c, dev, wfmt)
    return {'out': run_head(c, dev).double()}


def is_fp16(c):
    return not (c.kind in ('conv_last', 'hr_last') or c.p.get('out') == 'planar')


def check(c, got, want, premise_ok, tag=''):
    ok, lines = True, []
    assert 'out' in got and set(got) <= set(want)
    for k in got:                                           # (conf_max only where the case asked for it)
        v = want[k]
        assert got[k].shape == v.shape, (k, tuple(got[k].shape), tuple(v.shape))
        o, n, txt = ec.matches(got[k], v, c, is_fp16(c) and k == 'out', premise_ok)
        ok = ok and o
        lines.append('%s: %s' % (k, txt))
    report('%-58s %s mismatches=%s' % (c.name + tag, c.line(), '; '.join(lines)))
    assert ok, '%s%s: %s' % (c.name, tag, '; '.join(lines))


# ---- the premise: a dependency of every other case --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def premise(dev):
    """(holds, text): does refvsr_conv_mfma return the exact sums on fp16-representable dyadic weights (lo = 0)?"""
    c = get_case(ec.PREMISE)
    c.assert_strong()
    n, txt = ec.mismatch(run_case(c, dev)['out'], c.want['out'], c.g_out, False)
    return n == 0, txt


def test_premise_matrix_unit_adds_exact_sums_exactly(dev, premise):
    """Generic refvsr_conv_mfma, 24 -> 24 3x3 at 19 x 45, fp32 planar output, dyadic weights that ARE fp16 numbers (lo = 0), inputs
    in {-1, 0, 1}: every partial sum is an fp32 number, so this checks one thing only -- that the MFMA's fp32 accumulation returns
    exactly representable sums exactly (no truncated alignment, no flushed operand).  Every other case of this file rests on it.
    On the MI355X: holds, 0 of 20520 outputs differ."""
    c = get_case(ec.PREMISE)
    report('%-58s %s mismatches=%s' % (c.name, c.line(), premise[1]))
    assert premise[0], premise[1]


PLAIN = [n for n in ec.NAMES[1:] if not n.startswith(('f16w', 'subnormal'))]


@pytest.mark.parametrize('name', PLAIN)
def test_kernel_equals_reference_bit_for_bit(dev, premise, name):
    c = get_case(name)
    c.assert_strong()
    check(c, run_case(c, dev), c.want, premise[0])


@pytest.mark.parametrize('name', [n for n in ec.NAMES if n.startswith('conv_last') or n.startswith('conv_hr_last')][::2])
def test_head_result_formats(dev, premise, name):
    """The fused heads store fp16 and uint8 results directly: fp16(v) and rint(255 v) of the exact fp32 value v."""
    c = get_case(name)
    want16, want8 = ec.result_formats(c.want['out'])
    got16, got8 = run_head(c, dev, 'float16'), run_head(c, dev, 'uint8')
    assert got16.dtype == torch.float16 and got8.dtype == torch.uint8
    n16, n8 = int((got16 != want16).sum()), int((got8 != want8).sum())
    report('%-58s float16 mismatches=%d uint8 mismatches=%d (outputs at 0: %d, at 255: %d)' % (
        c.name + ' formats', n16, n8, int((want8 == 0).sum()), int((want8 == 255).sum())))
    assert int((want8 == 0).sum()) > 0 and int((want8 == 255).sum()) > 0, 'both clamps must be hit'
    if premise[0]:
        assert n16 == 0 and n8 == 0
    else:
        assert float((got16.double() - want16.double()).abs().max()) <= 2.0 ** -10 and int((got8.int() - want8.int()).abs().max()) <= 1


def _want_of(v, fmt):
    """The stored value of an exact fp32 head output v (float64 tensor) in a result format, as rv_store_result forms it."""
    w16, w8 = ec.result_formats(v)
    return {None: v.float(), 'float16': w16, 'uint8': w8}[fmt]


@pytest.mark.parametrize('name', ec.BASED)
def test_head_with_base_equals_reference_on_every_route(dev, premise, name):
    """A NON-ZERO base frame at x4 and x2 through each route by which a frame leaves the network (run_head: ops.conv_last,
    ops.conv_hr_last where the case has a conv_hr, and the unfused fallback), in float32, float16 and uint8, each planar and
    channels-last: every stored value must be the reference's, bit for bit -- the bicubic term (coordinates at steps 1/4 and 1/2,
    the 4 x 4 window and its index clamps on all borders, the plane of each channel, the first clamp) is exact on these maps
    (tests/test_exact_cases.py).  Each launch runs a second time between fences (tests/footprint.py), the base NaN-fenced: the
    fenced result must equal the plain one and no fence may change.  A read past the base is detected by EQUALITY WITH THE
    REFERENCE (every border and corner has outputs strictly inside (0, 1) whose taps were index-clamped), not by no_nan: a NaN that
    reaches `fminf(fmaxf(x, 0), 1)` comes out as 0."""
    from refvsr_amd import ops
    c = get_case(name)
    c.assert_strong()
    want = c.want['out']
    bad = []
    for route in routes_of(c):
        for fmt in FORMATS:
            for layout in ('chw', 'hwc'):
                got = run_head(c, dev, fmt, layout, route)
                got2, verdict = run_head(c, dev, fmt, layout, route, fenced=True)
                w = _want_of(want, fmt)
                assert got.dtype == w.dtype and got.shape == w.shape
                assert ops.result_layout_of(got) == layout and ops.result_layout_of(got2) == layout
                n, n2 = int((got != w).sum()), int((got2 != w).sum())
                report('%-58s %-9s %-7s %s mismatches=%d fenced=%d fence=%s' % (c.name, route, fmt or 'float32', layout, n, n2, verdict or 'intact'))
                if n or n2 or verdict or not torch.equal(got, got2):
                    bad.append('%s %s %s: %d | fenced %d of %d differ; %s' % (route, fmt or 'float32', layout, n, n2, w.numel(), verdict))
    assert premise[0], premise[1]
    assert not bad, '%s: %s' % (c.name, '\n'.join(bad))


@pytest.mark.parametrize('name', ec.GENERAL_NAMES)
def test_head_with_byte_base_stays_within_the_derived_bound(dev, premise, name):
    """Base = random bytes / 255 (what ingest_u8 hands the head) behind conv operands that are still exact, through every route,
    format and layout: the float32 result within exact_cases.GENERAL_BOUND (10 x 2^-24: derived from the chain of roundings in
    exact_cases.py, checked on the CPU against the reference's float32 replay) of the float64 reference; a float16 | uint8 result
    between the stores of reference - bound and reference + bound, which differ at fewer than 1 % of the elements (for uint8: by
    one code, only where 255 x reference lies within 255 x bound of a half-integer)."""
    g = ec.get_general(name)
    bad = []
    for route in routes_of(g.case):
        for fmt in FORMATS:
            lo, hi = g.allowed(fmt or 'float32')
            assert fmt is None or g.loose(fmt) <= ec.GENERAL_CAP
            for layout in ('chw', 'hwc'):
                got = run_head(g.case, dev, fmt, layout, route).double()
                if fmt == 'float16':
                    assert got.dtype == torch.float64
                out = int(((got < lo) | (got > hi)).sum())
                err = float((got / (255.0 if fmt == 'uint8' else 1.0) - g.want).abs().max())
                report('%-58s %-9s %-7s %s outside=%d max |got - reference|=%.3g differs from the stored reference at %d' % (
                    name, route, fmt or 'float32', layout, out, err, int((got != g.store(g.want, fmt or 'float32')).sum())))
                if out:
                    bad.append('%s %s %s: %d of %d outside the allowed interval (max error %.3g)' % (route, fmt or 'float32', layout, out, got.numel(), err))
    assert not bad, '%s: %s' % (name, '\n'.join(bad))


@pytest.mark.parametrize('name', [n for n in ec.NAMES if n.startswith('f16w')])
def test_f16w_twin_drops_lo_and_default_path_keeps_it(dev, premise, name):
    """Weights WITH a lo part through both entry points: the _f16w twin must equal the reference on fp16(w), the hi + lo entry point
    the reference on w, and the two references differ on control (a)'s share of the outputs -- the default path uses lo and the
    opt-in path does not, pinned in both directions."""
    c = get_case(name)
    c.assert_strong()
    assert c.primary == 'hi' and c.controls[0] >= ec.CTL_A_MIN
    check(c, run_case(c, dev, 'fp16'), c.hi[0], premise[0], ' [twin, fp16(w)]')
    check(c, run_case(c, dev, 'hi_lo'), c.full[0], premise[0], ' [hi + lo entry, w]')


@pytest.mark.parametrize('name', [n for n in ec.NAMES if n.startswith('subnormal')])
def test_subnormal_hi_operands_reach_the_mfma_unflushed(dev, premise, name):
    """Every weight of these cases is an fp16 SUBNORMAL (|w| < 2^-14 on the 2^-24 granule, lo = 0) on integer maps up to +-8 (the
    fused block: the same integers scaled by 2^-10, so that its residual fits the exactness condition; its intermediate map is then
    made of fp16 subnormals too -- the B operand).  This pins that fp16 subnormal A operands reach the MFMA unflushed: the lo halves
    of real weights (|w| < 2^-3) are all subnormals, and a flushed operand would silently turn the 22-bit weights into 11-bit
    ones.  Control (a) of these cases is the share of outputs that changes when subnormal weights are flushed to zero."""
    c = get_case(name)
    c.assert_strong()
    check(c, run_case(c, dev), c.want, premise[0])
