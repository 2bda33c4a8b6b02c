"""Runs rows of tests/conv_variant_cases.py on the GPU: imported by tests/test_gpu_conv_variants.py for the rows without a knob, and
started by it as a fresh process for each other knob set (the library reads the REFVSR_CONV_* knobs once per process):

    python conv_variant_child.py KNOB_SET OUT.npz

runs every row of KNOB_SET (and the walk twin of the resident ones) under the environment it was given and writes, per run `t`:
out_t (the raw output map), key_t (what refvsr_conv_variant reports for the descriptor that was launched), same_t (1: the
inputs came back unchanged), and of the fenced second run (fenced_twin()) fence_t ('' = fences intact, every result fenced, no
NaN, inputs and their fences unchanged, same key; else what was found) and equal_t (1: its raw output equals out_t).  It judges
nothing else: the parent compares."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_variant_cases as cv  # noqa: E402
import footprint as fp  # noqa: E402


def hwc(x, dtype, dev, poison=None):
    """float64 [C, H, W] -> device [H, W, Cs] of dtype (channel padding zero: 8 fp16 or 4 fp32 channels per group), with torch alone.
    poison: None = an allocation of its own, 'nan' | 'benign' = a view between the fences of footprint.fenced_input."""
    grp = 4 if dtype == torch.float32 else 8
    c, h, w = x.shape
    t = torch.zeros(h, w, (c + grp - 1) // grp * grp, dtype=dtype)
    t[:, :, :c] = x.permute(1, 2, 0).to(dtype)
    assert torch.equal(t[:, :, :c].double(), x.permute(1, 2, 0)), 'input map is not representable in %s' % dtype
    return t.to(dev) if poison is None else fp.fenced_input(t, dev, poison)


def planar64(t, c):
    """[H, W, Cs] (cpu) -> float64 [c, H, W]; the channel padding must hold zeros."""
    assert not t[:, :, c:].any(), 'channel padding of the output map is not zero'
    return t[:, :, :c].permute(2, 0, 1).double().contiguous()


def run_conv(c, dev, fenced=False):
    """One refvsr_conv_mfma launch of a conv case (exact_cases.Case or f32_cases.Case32) through ops.conv -> (raw output on the
    cpu, the planned variant's key, inputs unchanged).  fenced: the same launch with every map, the weights and the bias between NaN
    fences and the output between 0xA5 fences (tests/footprint.py) -> one more element, '' or what footprint.judge found."""
    from refvsr_amd import hip, ops
    from refvsr_amd.packing import pack_conv
    p, r = c.p, c.run
    f32 = bool(r.get('f32'))
    dt = torch.float32 if f32 else torch.float16
    cins = [s.shape[0] for s in p['srcs']]
    cw = ops.ConvWeights(pack_conv(p['w'].float(), p['b'].float(), cins, False, mt=r['mt'], f32=f32, hi_only=r['hi_only']), dev)
    cw.blob24 = None                                        # refvsr_conv_mfma for the shapes the specialised kernels serve as well
    poison = 'nan' if fenced else None
    if fenced:
        fp.reset_inputs()
        fp.fence_weights(cw)
    ins = dict(('src%d' % i, hwc(s, dt, dev, poison)) for i, s in enumerate(p['srcs']))
    kw = dict(stride=p['stride'], act=p['act'], post=p['post'])
    for k in ('mul', 'res'):
        if p.get(k) is not None:
            kw[k] = ins[k] = hwc(p[k], dt, dev, poison)
    if p['out'] == 'planar':
        kw.update(planar_out=True, add_const=p['add_const'], clamp=p['clamp'])
        if p.get('res_planar') is not None:
            rp = p['res_planar'].float().contiguous()
            kw['res_planar'] = ins['res_planar'] = fp.fenced_input(rp, dev, 'nan') if fenced else rp.to(dev)
    ins['wpack'], ins['bias'] = cw.wpack, cw.bias
    before = dict((k, v.clone()) for k, v in ins.items())
    if r['cap']:
        hip.lib().refvsr_set_conv_workgroup_cap(r['cap'])  # persistent walk: every workgroup takes several tiles
    msg = None
    try:
        if fenced:
            with fp.fenced_outputs(ops) as fo:
                got = ops.conv(cw, ins['src0'], ins.get('src1'), **kw)
                msg = fp.judge(fo, [got])
        else:
            got = ops.conv(cw, ins['src0'], ins.get('src1'), **kw)
        torch.cuda.synchronize()
    finally:
        if r['cap']:
            hip.lib().refvsr_set_conv_workgroup_cap(0)
    key = ctypes.c_int(-1)
    hip.check(hip.lib().refvsr_conv_variant(ctypes.byref(cw.desc), ctypes.byref(key)), 'conv_variant')      # the descriptor that was launched
    assert got.dtype == (torch.float32 if f32 or p['out'] == 'planar' else torch.float16)
    same = all(torch.equal(v, before[k]) for k, v in ins.items())
    if fenced:
        fp.reset_inputs()
        return got.cpu(), key.value, same, msg
    return got.cpu(), key.value, same


def fenced_twin(c, dev, out, key):
    """The fenced second run of a case whose plain run gave (out, key) -> (fence, equal): fence = '' or why it fails (a damaged
    fence, an unfenced result, a NaN, a changed input or input fence: footprint.judge; a planned variant that moved with the
    pointers), equal = the raw output, channel padding included, equals the plain run's."""
    out2, key2, same2, msg = run_conv(c, dev, fenced=True)
    bad = [msg] if msg else []
    equal = out2.dtype == out.dtype and torch.equal(out2, out)
    if key2 != key:
        bad.append('the fenced run was planned as key %d, the plain run as %d' % (key2, key))
    if not same2:
        bad.append('an input of the fenced run was written to')
    return '\n'.join(bad), equal


def runs_of(knob):
    """[(tag, row index, walk)] of a knob set."""
    out = []
    for i, r in enumerate(cv.ROWS):
        if r.knob == knob:
            out.append(('%02d' % i, i, False))
            if cv.is_resident(r):
                out.append(('%02dw' % i, i, True))
    return out


def main(knob, path):
    t0 = time.time()
    for k, v in cv.KNOBS[knob].items():
        assert os.environ.get(k) == v, 'knob %s did not arrive' % k
    assert torch.cuda.is_available(), 'the child needs a GPU'
    dev = torch.device('cuda:0')
    res = {}
    for tag, i, walk in runs_of(knob):
        out, key, same = run_conv(cv.get_case(i, walk), dev)
        res['out_' + tag], res['key_' + tag], res['same_' + tag] = out.numpy(), np.int64(key), np.int64(same)
        fence, equal = fenced_twin(cv.get_case(i, walk), dev, out, key)
        res['fence_' + tag], res['equal_' + tag] = np.array(fence), np.int64(equal)
    res['seconds'] = np.float64(time.time() - t0)
    np.savez(path, **res)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
