"""Exact-arithmetic parity of the fp32 path that feeds the matching's arg-max, on a real MI355X: every case of tests/f32_cases.py is
fed to its kernel -- refvsr_conv_mfma in F32 mode, refvsr_conv_direct_f32, refvsr_conv1x1_f32, refvsr_frame_prep -- and the result
must equal the float64 reference BIT FOR BIT.

The inputs are chosen (and checked on the CPU, tests/test_f32_cases.py) so that every product and every partial sum is an fp32
number: no MFMA schedule and no fmaf order can change the result.  The wfull / xfull cases carry 24-bit weights / activations: a
kernel that rounds an operand to fp16, tf32 or a hi + lo pair differs on their controls' share of the outputs.

The fmaf-chain kernels have no premise: IEEE fmaf returns an exactly representable result exactly.  For the fp32 MFMA the premise
case asks the hardware; if it fails, that is a finding about the matrix unit and the conv_mfma cases follow the fallback written
down in exact_cases.matches (within 4 granules).  On the MI355X it holds."""
import ctypes
import os

import pytest
import torch

import conv_variant_child as child
import exact_cases as ec
import f32_cases as fc
import footprint as fp
from f32_cases import get_case
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(OPS_REPORT), 'gpu_f32_exact_report.txt')
MARK = 7.0                          # what the fences around a directly allocated output and its channel padding hold before the launch


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


def f32(t, dev):
    return t.float().contiguous().to(dev)


def f32_fenced(t, dev):
    """The same values as a view between NaN fences (tests/footprint.py)."""
    return fp.fenced_input(t.float().contiguous(), dev, 'nan')


def marked(shape, dtype, dev):
    """((flat buffer, lead), its view of that shape): the buffer is all MARK, and a lead and a tail of footprint.fence_bytes(bytes of
    the shape) each lie before and behind the view."""
    n = 1
    for s in shape:
        n *= s
    esz = torch.empty((), dtype=dtype).element_size()
    lead = fp.fence_bytes(n * esz) // esz
    buf = torch.full((2 * lead + n,), MARK, dtype=dtype, device=dev)
    view = buf[lead:lead + n].view(*shape)
    assert view.data_ptr() % 16 == 0
    return (buf, lead), view


def guard_ok(marked_buf):
    buf, lead = marked_buf
    return bool((buf[:lead] == MARK).all()) and bool((buf[-lead:] == MARK).all())


def run_mfma(c, dev):
    out, key, same = child.run_conv(c, dev)
    assert same, 'an input was written to'
    fence, equal = child.fenced_twin(c, dev, out, key)
    report('%-62s key=%-5d fenced run: fences=%s equal=%s' % (c.name, key, 'BROKEN' if fence else 'ok', 'ok' if equal else 'NO'))
    assert not fence, '%s, fenced run: %s' % (c.name, fence)
    assert equal, '%s: the fenced run does not equal the plain run' % c.name
    p = c.p
    co = p['w'].shape[0]
    if p['out'] == 'planar':
        return {'out': out.double()}
    assert out.dtype == torch.float32 and out.shape[2] == fc.pad4(co)
    return {'out': child.planar64(out, co)}


def run_direct(c, dev):
    """refvsr_conv_direct_f32 from NaN-fenced inputs into a marked buffer: the fences before and behind the output and, for the fp16
    HWC store, channels cout .. out_c stay as they were."""
    from refvsr_amd import hip
    from refvsr_amd.ops import _ptr, _stream
    p, r = c.p, c.run
    fp.reset_inputs()
    x, w, b = f32_fenced(p['srcs'][0], dev), f32_fenced(p['w'], dev), f32_fenced(p['b'], dev)
    keep = [t.clone() for t in (x, w, b)]
    co, ci, ks, _ = p['w'].shape
    h, wd = x.shape[1:]
    ho, wo = fc.out_hw((h, wd), ks, p['stride'])
    oc = r['out_c']
    buf, out = marked((ho, wo, oc), torch.float16, dev) if oc else marked((co, ho, wo), torch.float32, dev)
    hip.check(hip.lib().refvsr_conv_direct_f32(_ptr(x), ci, h, wd, _ptr(w), _ptr(b), co, ks, p['stride'], ks // 2, p['act'], _ptr(out), int(bool(oc)), oc,
                                               _stream()), 'conv_direct_f32')
    torch.cuda.synchronize()
    assert guard_ok(buf), 'written before or behind the output'
    assert all(torch.equal(a, k) for a, k in zip((x, w, b), keep)), 'an input was written to'
    assert fp.inputs_unchanged() is None, fp.inputs_unchanged()
    fp.reset_inputs()
    out = out.cpu()
    assert not torch.isnan(out).any(), 'a NaN from an input fence reached the output'
    report('%-62s fenced run: fences=ok' % c.name)
    if not oc:
        return {'out': out.double()}
    assert bool((out[:, :, co:] == MARK).all()), 'the channel padding of the fp16 HWC output was written to'
    return {'out': out[:, :, :co].permute(2, 0, 1).double().contiguous()}


def run_c1x1(c, dev):
    from refvsr_amd import ops
    p = c.p
    x = f32(p['srcs'][0].permute(1, 2, 0), dev)              # fp32 HWC, exactly cin channels
    w, b = f32(p['w'][:, :, 0, 0], dev), f32(p['b'], dev)
    keep = [t.clone() for t in (x, w, b)]
    out = ops.conv1x1_f32(x, w, b, p['act'])
    torch.cuda.synchronize()
    assert all(torch.equal(a, k) for a, k in zip((x, w, b), keep)), 'an input was written to'
    # the fenced second run: NaN around the map, the weights and the bias, 0xA5 around the output
    fp.reset_inputs()
    xf, wf, bf = f32_fenced(p['srcs'][0].permute(1, 2, 0), dev), f32_fenced(p['w'][:, :, 0, 0], dev), f32_fenced(p['b'], dev)
    with fp.fenced_outputs(ops) as fo:
        out2 = ops.conv1x1_f32(xf, wf, bf, p['act'])
        bad = fp.judge(fo, [out2], [out])
    fp.reset_inputs()
    report('%-62s fenced run: fences=%s equal=%s' % (c.name, 'BROKEN' if bad else 'ok', 'NO' if 'differs' in bad else 'ok'))
    assert not bad, '%s, fenced run: %s' % (c.name, bad)
    return {'out': out.cpu().double()}


def run_prep(c, dev):
    """refvsr_frame_prep from NaN-fenced inputs into marked buffers -> lr_n as 'out', ref_n, lr8, ref8 as [3, h, w]; the zero lanes
    are checked here."""
    from refvsr_amd import hip
    from refvsr_amd.ops import _ptr, _stream
    p = c.p
    fp.reset_inputs()
    lr, ref, w, b = f32_fenced(p['lr'], dev), f32_fenced(p['ref'], dev), f32_fenced(p['w'], dev), f32_fenced(p['b'], dev)
    keep = [t.clone() for t in (lr, ref, w, b)]
    h, wd = lr.shape[1:]
    hr, wr = ref.shape[1:]
    bufs = [marked((h, wd, 8), torch.float16, dev), marked((hr, wr, 8), torch.float16, dev), marked((h, wd, 4), torch.float32, dev),
            marked((hr // 2, wr // 2, 4), torch.float32, dev)]
    (lr8, ref8, lr_n, ref_n) = [v for _, v in bufs]
    hip.check(hip.lib().refvsr_frame_prep(_ptr(lr), h, wd, _ptr(ref), hr, wr, _ptr(w), _ptr(b), _ptr(lr8), _ptr(ref8), _ptr(lr_n), _ptr(ref_n), _stream()),
              'frame_prep')
    torch.cuda.synchronize()
    assert all(guard_ok(bf) for bf, _ in bufs), 'written before or behind an output (ref_n ends at the last whole 2 x 2 quad)'
    assert all(torch.equal(a, k) for a, k in zip((lr, ref, w, b), keep)), 'an input was written to'
    assert fp.inputs_unchanged() is None, fp.inputs_unchanged()
    fp.reset_inputs()
    report('%-62s fenced run: fences=ok' % c.name)
    res = {}
    for name, t in (('lr8', lr8), ('ref8', ref8), ('out', lr_n), ('ref_n', ref_n)):
        t = t.cpu()
        assert not torch.isnan(t).any(), '%s: a NaN from an input fence reached the output' % name
        assert not t[:, :, 3:].any(), '%s: the zero lanes are not zero' % name
        res[name] = t[:, :, :3].permute(2, 0, 1).double().contiguous()
    return res


RUN = {'conv_mfma': run_mfma, 'conv_direct': run_direct, 'conv1x1': run_c1x1, 'frame_prep': run_prep}


def check(c, got, premise_ok):
    ok, lines = True, []
    assert set(got) == set(c.want)
    for k, v in c.want.items():
        assert got[k].shape == v.shape, (k, tuple(got[k].shape), tuple(v.shape))
        fp16 = k in ('lr8', 'ref8') or (k == 'out' and c.p.get('store') == 'f16')
        o, n, txt = ec.matches(got[k], v, c, fp16, premise_ok)
        ok = ok and o
        lines.append('%s: %s' % (k, txt))
    report('%-62s %s mismatches=%s' % (c.name, c.line(), '; '.join(lines)))
    assert ok, '%s: %s' % (c.name, '; '.join(lines))


@pytest.fixture(scope='module')
def premise(dev):
    c = get_case(fc.PREMISE)
    n, txt = ec.mismatch(run_mfma(c, dev)['out'], c.want['out'], c.g_out, False)
    return n == 0, txt


def test_premise_fp32_matrix_unit_adds_exact_sums_exactly(dev, premise):
    """refvsr_conv_mfma in F32 mode, 24 -> 32 3x3 at 19 x 45, fp32 planar output, dyadic 14-bit weights on inputs in {-1, 0, 1}:
    every partial sum is an fp32 number, so this asks one thing -- does v_mfma_f32_16x16x4_f32 return exactly representable sums
    exactly.  Every conv_mfma case of this file and every F32 row of tests/test_gpu_conv_variants.py rests on it."""
    c = get_case(fc.PREMISE)
    c.assert_strong()
    report('%-62s %s mismatches=%s' % (c.name, c.line(), premise[1]))
    assert premise[0], premise[1]


@pytest.mark.parametrize('name', fc.NAMES[1:])
def test_kernel_equals_reference_bit_for_bit(dev, premise, name):
    c = get_case(name)
    c.assert_strong()
    entry = c.run['entry']
    check(c, RUN[entry](c, dev), premise[0] if entry == 'conv_mfma' else True)
