"""Parity of the sampling, gather and EDVR helper kernels on a real MI355X (csrc/resample.hip, gather.hip, edvr.hip) against the
float64 references of tests/sampling_cases.py.

  * Every EXACT case goes through its ops.* entry point and must return the reference's BITS: its inputs are proved on the CPU
    (tests/test_sampling_cases.py) to make every step of the kernel's fp32 chain exact, so neither operation order nor FMA contraction
    can change the result and the store is one round-to-nearest-even of an exact number.  A failure prints the number of mismatches,
    the first mismatching coordinates and their tap class: a kernel bug or a reference error, never a tolerance.
  * Every GENERAL case must lie inside  |got - want64| <= ulp16(want64) / 2 + delta  (fp16 stores; fp32 stores: delta), elementwise and
    with no element excluded; delta = 4 x the float32-vs-float64 error of the reference itself on that case's inputs, + 2^-20 |want|
    for the kernels that use __expf (derivation: sampling_cases.py).
  * fp16 maps are built with torch alone (nhwc16 / planar64 of test_gpu_exact.py), not through the pack kernels; those are pinned
    once here against the same helpers.  Inputs must be unchanged after every call and the channel padding a kernel is specified
    to write must be zero.

Report lines (per case: mismatches or delta and the observed maximum, the controls) are appended next to the other GPU reports;
profiles/gpu_sampling_parity_report.txt has the MI355X run."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import footprint as fp
import sampling_cases as sc
from sampling_cases import get_case
from test_gpu_exact import nhwc16, planar64
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(OPS_REPORT), 'gpu_sampling_report.txt')


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
    t0 = time.time()
    yield torch.device('cuda:0')
    report('%-58s %.1f s' % ('wall time of tests/test_gpu_sampling.py', time.time() - t0))


# ---- feeding the kernels -------------------------------------------------------------------------------------------------------------
class Inputs(object):
    """Device copies of a case's inputs; unchanged() proves that no kernel wrote to one of them.  fenced: every copy is a view
    between the fences of footprint.fenced_input, of the poison kind its call names: 'nan' for data that enters arithmetic, 'benign'
    (zeros) for what a kernel turns into a coordinate or an address -- flows, offsets and masks, affine parameters, indices."""

    def __init__(self, dev, fenced=False):
        self.dev, self.kept, self.fenced = dev, [], fenced
        if fenced:
            fp.reset_inputs()

    def _keep(self, t):
        self.kept.append((t, t.clone()))
        return t

    def _put(self, t, poison):
        return fp.fenced_input(t, self.dev, poison) if self.fenced else t.to(self.dev)

    def f16(self, a, cs=None, poison='nan'):
        return self._keep(self._put(nhwc16(torch.from_numpy(np.ascontiguousarray(a)), 'cpu', cs), poison))

    def f32(self, a, poison='nan'):
        t = torch.from_numpy(np.ascontiguousarray(a))
        assert torch.equal(t.float().double(), t), 'input is not fp32-representable'
        return self._keep(self._put(t.float(), poison))

    def i32(self, a, poison='benign'):
        return self._keep(self._put(torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32), poison))

    def unchanged(self):
        torch.cuda.synchronize()
        for t, t0 in self.kept:
            assert torch.equal(t, t0), 'an input was written to'
        if self.fenced:
            assert fp.inputs_unchanged() is None, fp.inputs_unchanged()
            fp.reset_inputs()


def np16(t, c):
    return planar64(t, c).numpy()


def np32(t):
    assert t.dtype == torch.float32
    return t.cpu().double().numpy()


BENIGN = 'benign'


def run_case(c, dev, fenced=False):
    """({output: float64 numpy array in the reference's layout}, [the raw result tensors on the cpu], fence) of case c through its
    ops.* entry point.  fenced: the inputs between fences (Inputs), every allocation of ops between 0xA5 fences; fence is
    footprint.judge's verdict on fences, results, NaN and inputs ('' = all is well; always '' for a plain run)."""
    from refvsr_amd import ops
    if not fenced:
        out, raw = _run_case(c, dev, Inputs(dev))
        return out, raw, ''
    I = Inputs(dev, True)
    with fp.fenced_outputs(ops) as fo:
        raw = []
        out = _run_case(c, dev, I, raw)[0]
        fence = fp.judge(fo, raw)
    return out, [t.cpu() for t in raw], fence


def _run_case(c, dev, I, raw=None):
    from refvsr_amd import hip, ops
    p = c.p
    raw = [] if raw is None else raw

    def K(t):                                                # keeps the raw result tensors as the entry point returned them
        raw.extend(t if isinstance(t, (tuple, list)) else [t])
        return t
    if c.op == 'warp':
        entry = c.run['entry']
        if entry == 'warp_planar':
            out = {'out': np32(K(ops.warp_planar(I.f32(p['x']), I.f32(p['flow'], BENIGN))))}
        else:
            fn = ops.warp_nhwc16_up2 if entry == 'warp_nhwc16_up2' else ops.warp_nhwc16
            out = {'out': np16(K(fn(I.f16(p['x']), I.f32(p['flow'], BENIGN))), p['x'].shape[0])}
    elif c.op == 'resize':
        got = K(ops.resize(I.f32(p['x']), p['out_hw'], p['mode'], p.get('src_scale'), p.get('mean'), p.get('std'), p.get('chan_mul'),
                           bool(p.get('clamp01')), c.run['nhwc16']))
        out = {'out': np16(got, p['x'].shape[0]) if c.run['nhwc16'] else np32(got)}     # (np16: the channels 3 .. 7 must be zero)
    elif c.op == 'spynet':
        B = len(p['ref'])
        refs, supps = [I.f32(a) for a in p['ref']], [I.f32(a) for a in p['supp']]
        prev = I.f32(np.stack(p['flow_prev']), BENIGN) if p['flow_prev'] is not None else None
        if B == 1:
            o8, up = K(ops.spynet_level_input(refs[0], supps[0], prev[0] if prev is not None else None))
            o8, up = o8[None], up[None]
        else:
            o8, up = K(ops.spynet_level_input_batch(refs, supps, prev))
        out = {'out': np.stack([np16(o8[b], 8) for b in range(B)]), 'flow_up': np32(up)}
    elif c.op == 'aligned':
        out = {'out': np16(K(ops.aligned_sample(I.f16(p['x']), I.f32(p['affine'], BENIGN), p['ks'])), p['x'].shape[0])}
    elif c.op == 'gather':
        gh, gw = p['idx'].shape
        idx = I.i32(p['idx'].reshape(-1))
        if c.run['kind'] == 'nhwc16':
            out = {'out': np16(K(ops.block_gather_nhwc16(I.f16(p['value']), idx, gh, gw, p['s'])), p['value'].shape[0])}
        elif c.run['kind'] == 'rgb16':
            out = {'out': np16(K(ops.block_gather_rgb(I.f32(p['value']), idx, gh, gw, p['s'])), 3)}
        else:
            out = {'out': np32(K(ops.block_gather_rgb(I.f32(p['value']), idx, gh, gw, p['s'], planar=True)))}
    elif c.op == 'dcn':
        out = {'out': np16(K(ops.dcn_sample(I.f16(p['x']), I.f32(p['om'], BENIGN), p['dg'])), 9 * p['x'].shape[0])}
    elif c.op == 'pool3s2':                                 # into channels [8, 8 + c) of a wider map: the others keep a sentinel
        x = I.f16(p['x'])
        h, w, ch = x.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        wide = K(ops.torch.empty((ho, wo, ch + 16), dtype=torch.float16, device=dev).fill_(-77.0))  # (ops.torch: fenced in a fenced run)
        hip.check(hip.lib().refvsr_pool3s2_nhwc16(C.c_void_p(x.data_ptr()), h, w, ch, C.c_void_p(wide.data_ptr()), ch + 16, 8, int(p['is_max']),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'pool3s2')
        torch.cuda.synchronize()
        assert bool((wide[:, :, :8] == -77.0).all()) and bool((wide[:, :, 8 + ch:] == -77.0).all()), 'pool3s2 wrote outside its channels'
        out = {'out': np16(wide[:, :, 8:8 + ch].contiguous(), ch)}
    elif c.op == 'up2':
        out = {'out': np16(K(ops.up2_bilinear_nhwc16(I.f16(p['x']), p['mul'])), p['x'].shape[0])}
    elif c.op == 'tsa_weight':
        got = K(ops.tsa_weight([I.f16(a) for a in p['aligned']], [I.f16(a) for a in p['emb']], I.f16(p['emb_ref'])))
        out = {'out': np16(got, got.shape[2])}
    elif c.op == 'tsa_blend':
        out = {'out': np16(K(ops.tsa_blend(I.f16(p['feat']), I.f16(p['attn']), I.f16(p['add']))), p['feat'].shape[0])}
    else:
        assert c.op == 'pool2'
        x = I.f32(p['x'])
        got = K(ops.max2(x, I.f32(p['y'])) if p['kind'] == 'max2' else (ops.maxpool2(x) if p['kind'] == 'max' else ops.avgpool2(x)))
        out = {'out': np32(got)}
    I.unchanged()
    return out, [t.cpu() for t in raw]


def fenced_twin(c, dev, raw, judge):
    """The fenced second run of a case whose plain run returned the raw tensors `raw`: fences intact and every result fenced, raw
    results equal to the plain run's, no NaN, inputs and their fences unchanged -- and the same judgement against the reference."""
    got2, raw2, fence = run_case(c, dev, fenced=True)
    equal = len(raw) == len(raw2) and all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) for a, b in zip(raw, raw2))
    report('%-58s fenced run: fences=%s equal=%s' % (c.name, 'BROKEN' if fence else 'ok', 'ok' if equal else 'NO'))
    assert not fence, '%s, fenced run: %s' % (c.name, fence)
    assert equal, '%s: the fenced run does not equal the plain run' % c.name
    judge(c, got2, ' [fenced]')


def check_exact(c, got, tag=''):
    lines, bad = [], 0
    assert set(got) == set(c.want)
    for k in got:
        assert got[k].shape == c.want[k].shape, (k, got[k].shape, c.want[k].shape)
        n, txt = sc.mismatch_report(c, got[k], k)
        bad += n
        lines.append('%s: %s' % (k, txt))
    report('%-58s %s mismatches=%s' % (c.name + tag, c.line(), '; '.join(lines)))
    assert bad == 0, '%s%s: %s' % (c.name, tag, '; '.join(lines))


def check_general(c, got, tag=''):
    lines, good = [], True
    assert set(got) == set(c.want64)
    for k in got:
        assert got[k].shape == c.want64[k].shape, (k, got[k].shape, c.want64[k].shape)
        ok, txt = sc.within_report(c, got[k], k)
        good = good and ok
        lines.append(txt)
    report('%-58s general %s' % (c.name + tag, '; '.join(lines)))
    assert good, '%s%s: %s' % (c.name, tag, '; '.join(lines))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sc.EXACT)
def test_kernel_equals_reference_bit_for_bit(dev, name):
    c = get_case(name)
    c.assert_strong()
    got, raw, _ = run_case(c, dev)
    check_exact(c, got)
    fenced_twin(c, dev, raw, check_exact)


@pytest.mark.parametrize('name', sc.GENERAL)
def test_kernel_within_the_reference_bracket(dev, name):
    c = get_case(name)
    got, raw, _ = run_case(c, dev)
    check_general(c, got)
    fenced_twin(c, dev, raw, check_general)


def test_pool3s2_pair_is_max_then_avg(dev):
    from refvsr_amd import ops
    c = get_case('pool3s2 x max 5x7')
    got = np16(ops.pool3s2_pair(nhwc16(torch.from_numpy(c.p['x']), dev)), 32)
    avg = sc.f16_store(sc.ref_pool3s2(sc.F64, {'x': c.p['x'], 'is_max': 0})['out'])
    assert np.array_equal(got[:16], c.want['out']) and np.array_equal(got[16:], avg)


# ---- multi-map launches: every output against ITS OWN map's reference -------------------------------------------------------------------
def test_multimap_warp_nhwc16_each_output_equals_its_own_reference(dev):
    from refvsr_amd import ops
    cases = [sc.warp_exact('warp_nhwc16 x 9x17<-9x17 cs24 #%d' % b, 7100 + b, (9, 17, 9, 17), 24, False)() for b in range(4)]
    I = Inputs(dev)
    out = ops.warp_nhwc16_b([I.f16(c.p['x']) for c in cases], [I.f32(c.p['flow']) for c in cases])
    I.unchanged()
    assert len({c.want['out'].tobytes() for c in cases}) == 4
    for b, c in enumerate(cases):
        c.assert_exact()
        check_exact(c, {'out': np16(out[b], 24)}, ' [batch of 4]')


def test_multimap_warp_planar_each_output_equals_its_own_reference(dev):
    from refvsr_amd import ops
    cases = [sc.warp_exact('warp_planar x 9x17<-9x17 c3 #%d' % b, 7200 + b, (9, 17, 9, 17), 3, True)() for b in range(4)]
    I = Inputs(dev)
    out = ops.warp_planar_b([I.f32(c.p['x']) for c in cases], [I.f32(c.p['flow']) for c in cases])
    I.unchanged()
    assert len({c.want['out'].tobytes() for c in cases}) == 4
    for b, c in enumerate(cases):
        c.assert_exact()
        check_exact(c, {'out': np32(out[b])}, ' [batch of 4]')


def test_multimap_warp_nhwc16_up2_each_output_within_its_own_bracket(dev):
    from refvsr_amd import ops
    cases = [sc.warp_general('warp_nhwc16_up2 g 18x34<-9x17 cs24 #%d' % b, 7300 + b, (18, 34, 9, 17), 24, 'warp_nhwc16_up2')() for b in range(4)]
    I = Inputs(dev)
    out = ops.warp_nhwc16_up2_b([I.f16(c.p['x']) for c in cases], [I.f32(c.p['flow']) for c in cases])
    I.unchanged()
    for b, c in enumerate(cases):
        check_general(c, {'out': np16(out[b], 24)}, ' [batch of 4]')
        other = cases[(b + 1) % 4]
        assert not sc.within_report(other, np16(out[b], 24))[0], 'two maps of the batch cannot be told apart'


# ---- the pack kernels, pinned against the torch-only helpers ---------------------------------------------------------------------------
@pytest.mark.parametrize('c,cs', [(3, 8), (5, 8), (5, 16), (24, 32)])
def test_pack_and_unpack_against_torch(dev, c, cs):
    from refvsr_amd import ops
    g = sc.rng(7400 + c)
    x = torch.from_numpy((g.standard_normal((c, 7, 13)) * 3).astype(np.float32))
    x[0, 0, :4] = torch.tensor([65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25 * 1.5])      # fp16 max, the smallest denormal, a tie-free rounding below it
    want16 = torch.zeros(7, 13, cs, dtype=torch.float16)
    want16[:, :, :c] = x.permute(1, 2, 0).to(torch.float16)
    xd = x.to(dev)
    got16 = ops.pack_nhwc16(xd, cs)
    assert got16.dtype == torch.float16 and torch.equal(got16.cpu(), want16), 'pack_nhwc16 (padding must be zero)'
    want32 = torch.zeros(7, 13, cs, dtype=torch.float32)
    want32[:, :, :c] = x.permute(1, 2, 0)
    got32 = ops.pack_nhwc32(xd, cs)
    assert got32.dtype == torch.float32 and torch.equal(got32.cpu(), want32), 'pack_nhwc32 (padding must be zero)'
    filled = torch.full((7, 13, cs), 5.0, dtype=torch.float16)
    filled[:, :, :c] = want16[:, :, :c]
    back = ops.unpack_nhwc16(filled.to(dev), c)
    assert torch.equal(back.cpu(), want16[:, :, :c].permute(2, 0, 1).float()), 'unpack_nhwc16'
    assert torch.equal(xd.cpu(), x)
    report('%-58s bit-equal (c=%d cs=%d)' % ('pack_nhwc16 / pack_nhwc32 / unpack_nhwc16', c, cs))
