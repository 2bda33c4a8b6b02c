"""Runs rows of tests/fixed_variant_cases.py on the GPU: imported by tests/test_gpu_fixed_variants.py for the rows without a knob, and
started by it as ONE fresh process for the row that needs REFVSR_CONV48_WAVES=8 (the library reads the knob once per process):

    python fixed_variant_child.py KNOB_SET OUT.npz

runs every run of every row of KNOB_SET under the environment it was given and writes, per run `t` (tag()): t.key / t.n_tiles / t.lds
(what the library's query reports for the arguments that were launched), t.same (1: the inputs came back unchanged), the raw
results t.<map>.<output>, and of the fenced second run (tests/footprint.py) t.fence ('' = every fence intact, every result fenced,
no NaN, inputs and their fences unchanged, the same key / n_tiles / lds; else what was found) and t.equal (1: every raw result
tensor equals the plain run's).  It judges nothing else: the parent compares.

One run = one launch through the entry point of refvsr_amd.ops that the engine uses: the maps of a multi-map row are separately
allocated tensors; a `walk` run goes to a plain side stream whose CU budget is 8 (refvsr_stream_set_cu_budget), set back to 0 in a
`finally`; the resblock24 setters (waves, store, probe buffer) are set for the run and restored in a `finally`."""
import contextlib
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

import exact_cases as ec  # noqa: E402
import fixed_variant_cases as fv  # noqa: E402
import footprint as fp  # noqa: E402

PROBE_WORDS, PROBE_TAIL, PROBE_MARK = 12, 64, 0x5a5a5a5a5a5a5a5a
SETTER_ENV = ('REFVSR_RESBLOCK24_WAVES', 'REFVSR_RB24_STORE')


def nhwc16(x, dev, poison=None):
    """float64 [C, H, W] of fp16 numbers -> device fp16 [H, W, Cs] (channel padding zero), with torch alone.  poison: None = an
    allocation of its own, 'nan' | 'benign' = a view between the fences of footprint.fenced_input."""
    c, h, w = x.shape
    t = torch.zeros(h, w, ec.pad8(c), dtype=torch.float16)
    t[:, :, :c] = x.permute(1, 2, 0).to(torch.float16)
    assert torch.equal(t[:, :, :c].double(), x.permute(1, 2, 0)), 'input map is not fp16-representable'
    return t.to(dev) if poison is None else fp.fenced_input(t, dev, poison)


def f32(t, dev=None, poison=None):
    t = t.float().contiguous()
    if poison is not None:
        return fp.fenced_input(t, dev, poison)
    return t.to(dev) if dev is not None else t


def planar64(t, c):
    """[H, W, Cs] (cpu) -> float64 [c, H, W]; the channel padding must hold zeros."""
    assert not t[:, :, c:].any(), 'channel padding of the output map is not zero'
    return t[:, :, :c].permute(2, 0, 1).double().contiguous()


def tag(i, run, form=None):
    return '%02d_%s%s' % (i, run, form or '')


def runs_of(knob):
    """[(row index, run, form)] of a knob set."""
    return [(i, run, form) for i, r in enumerate(fv.ROWS) if r.knob == knob for run in fv.runs_of(r) for form in fv.forms(r)]


@contextlib.contextmanager
def walk_stream(run):
    """The stream of a run: the current one, or for a walk run a side stream whose CU budget is 8 while the run lasts."""
    from refvsr_amd import hip, ops
    if fv.kind(run) != 'walk':
        yield ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    ptr = ctypes.c_void_p(s.cuda_stream)
    hip.check(hip.lib().refvsr_stream_set_cu_budget(ptr, fv.WALK_CUS), 'stream_set_cu_budget')
    try:
        with ops.on_stream(s):
            yield ptr
        s.synchronize()
    finally:
        hip.lib().refvsr_stream_set_cu_budget(ptr, 0)
        torch.cuda.synchronize()


@contextlib.contextmanager
def setters(row, hw, dev):
    """The resblock24 setters of a row; yields the probe buffer (or None).  The probe kernels write 12 words per workgroup at
    buf[12 * blockIdx.x + i], i < 12 (resblock24.hip: RB_STAMP), and the grid is min(n_tiles, cap) (launch_rb24): 12 x n_tiles words
    hold every stamp; a marked tail behind them must come back untouched."""
    from refvsr_amd import hip
    if row.kernel != 'rb24':
        yield None
        return
    h = hip.lib()
    buf = None
    try:
        hip.check(h.refvsr_set_resblock24_waves(row.setters['waves']), 'set_resblock24_waves')
        hip.check(h.refvsr_set_resblock24_store(row.setters['store']), 'set_resblock24_store')
        if row.setters['probe']:
            n = fv.n_tiles(row, hw)
            buf = torch.zeros(PROBE_WORDS * n + PROBE_TAIL, dtype=torch.int64)
            buf[PROBE_WORDS * n:] = PROBE_MARK
            buf = buf.to(dev)
            hip.check(h.refvsr_set_probe(ctypes.c_void_p(buf.data_ptr()), 0), 'set_probe')
        yield buf
    finally:
        h.refvsr_set_probe(None, 0)
        h.refvsr_set_resblock24_waves(0)
        h.refvsr_set_resblock24_store(1)


def query(row, hw, stream):
    """(key, n_tiles, lds) by the library's own query on the launched arguments, under the process's knobs and setters."""
    from refvsr_amd import hip
    n, lds = ctypes.c_int(-1), ctypes.c_int(-1)
    a = fv.query_args(row, hw)
    if row.kernel == 'rb24':
        key = ctypes.c_int(-1)
        hip.check(hip.lib().refvsr_resblock24_variant(*a, stream, ctypes.byref(key), ctypes.byref(n), ctypes.byref(lds)), 'resblock24_variant')
    else:
        key = ctypes.c_longlong(-1)
        hip.check(hip.lib().refvsr_conv24_variant(*a, ctypes.byref(key), ctypes.byref(n), ctypes.byref(lds)), 'conv24_variant')
    return key.value, n.value, lds.value


def _conv(row, cases, dev, pz):
    """-> (inputs, launch) of a conv24 / conv32 / conv48 / conv_shuffle2 row; launch() -> (the raw result tensors, fetch).  pz: None,
    or 'nan' = every map (each of a multi-map row on its own) and the weights between NaN fences"""
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv
    p0 = cases[0].p
    shuffle = row.entry == 'shuffle2'
    cw = ops.ConvWeights(pack_conv(f32(p0['w']), f32(p0['b']), list(row.cins), shuffle), dev, 'fp16' if row.wf else 'hi_lo')
    assert cw.blob24 is not None and cw.blob_wfmt == ('fp16' if row.wf else 'hi_lo'), 'no specialised kernel in this weight format'
    if pz:
        fp.fence_weights(cw)
    ins = {'blob': cw.blob24}
    for b, c in enumerate(cases):
        for k, s in enumerate(c.p['srcs']):
            ins['src%d.%d' % (k, b)] = nhwc16(s, dev, pz)
        for k in ('mul', 'res'):
            if c.p.get(k) is not None:
                ins['%s.%d' % (k, b)] = nhwc16(c.p[k], dev, pz)
    lst = lambda k: [ins['%s.%d' % (k, b)] for b in range(len(cases))] if k + '.0' in ins else None
    kw = dict(act=p0['act'], post=p0['post'])
    co = row.cout // 4 if shuffle else row.cout
    want = {'shuffle2': 'conv_shuffle2'}.get(row.entry, row.entry) + ('_batch' if row.mm else '')
    h, w = p0['srcs'][0].shape[1:]
    s0 = ins['src0.0']
    assert ops._conv_route(cw, s0.shape[2], ins['src1.0'].shape[2] if 'src1.0' in ins else None, ins.get('mul.0'), ins.get('res.0'), h, w, 1, 1, False,
                           kw['act'], kw['post'], len(cases) if row.mm else None) == want, 'the call does not reach refvsr_' + want

    def launch():
        if row.mm:
            out = ops.conv_b(cw, lst('src0'), lst('src1'), muls=lst('mul'), ress=lst('res'), **kw)
        else:
            out = [ops.conv(cw, s0, ins.get('src1.0'), mul=ins.get('mul.0'), res=ins.get('res.0'), **kw)]
        return list(out), lambda: [{'out': planar64(o.cpu(), co)} for o in out]
    return ins, launch


def _conf(row, cases, dev, pz):
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv
    p0 = cases[0].p
    cw = ops.ConvWeights(pack_conv(f32(p0['w']), f32(p0['b']), [16], False), dev, 'fp16' if row.wf else 'hi_lo')
    assert ops.conf_alpha_ok(cw, len(cases) if row.mm else None) and cw.blob_wfmt == ('fp16' if row.wf else 'hi_lo')
    if pz:
        fp.fence_weights(cw)
    ins = {'blob': cw.blob24, 'w0': f32(p0['w0'], dev, pz), 'b0': f32(p0['b0'], dev, pz)}
    for b, c in enumerate(cases):
        ins['a.%d' % b], ins['b.%d' % b] = f32(c.p['conf_a'], dev, pz), f32(c.p['conf_b'], dev, pz)
    lst = lambda k: [ins['%s.%d' % (k, b)] for b in range(len(cases))]
    wm = row.up == 1

    def launch():
        if row.mm:
            out = ops.conf_alpha_b(lst('a'), lst('b'), row.up, ins['w0'], ins['b0'], cw, p0['slope0'], p0['slope1'], want_max=wm)
            out = list(zip(out[0], out[1])) if wm else [(o,) for o in out]
        else:
            out = ops.conf_alpha(ins['a.0'], ins['b.0'], row.up, ins['w0'], ins['b0'], cw, p0['slope0'], p0['slope1'], want_max=wm)
            out = [out if wm else (out,)]
        return [t for o in out for t in o], lambda: [dict([('out', planar64(o[0].cpu(), row.cout))] + ([('cmax', o[1].cpu().double())] if wm else [])) for o in out]
    return ins, launch


def _head(row, cases, dev, formats, pz):
    """refvsr_conv_last | refvsr_conv_hr_last in every result format asked, with the base frame of the case: the exact non-zero map of a
    based run ([3, h / s, w / s]: base_step = 1 / s), or a zero frame of the output's own size (its bicubic sample is exactly 0).  The
    fenced twin puts the base between NaN fences like every other input; what detects a read past it is the bit equality with the
    reference (a NaN that reaches the head's clamps comes out as 0, which footprint.no_nan cannot see)."""
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv_hr_last, pack_conv_last
    p = cases[0].p
    x = nhwc16(p['x'], dev, pz)
    base = p['base'] if p.get('base') is not None else torch.zeros(3, x.shape[0], x.shape[1])
    ins = {'x': x, 'base': f32(base, dev, pz)}
    if row.entry == 'conv_last':
        ins['blob'] = pack_conv_last(f32(p['w']), f32(p['b'])).to(dev)
        ins['blob'] = fp.fence_weights(ins['blob']) if pz else ins['blob']
        run = lambda dt: ops.conv_last(ins['blob'], x, ins['base'], dt)
    else:
        ins['blob'] = pack_conv_hr_last(f32(p['w1']), f32(p['b1']), f32(p['w2']), f32(p['b2'])).to(dev)
        ins['blob'] = fp.fence_weights(ins['blob']) if pz else ins['blob']
        run = lambda dt: ops.conv_hr_last(ins['blob'], x, ins['base'], p['act'], dt)

    def launch():
        out = [(k, run(dt)) for k, dt in formats]
        return [o for _, o in out], lambda: [dict((k, o.cpu()) for k, o in out)]
    return ins, launch


def _blocks(row, cases, dev, pz):
    from refvsr_amd import ops
    p0 = cases[0].p
    raw = [((f32(w1), f32(b1)), (f32(w2), f32(b2))) for (w1, b1, w2, b2) in p0['blocks']]
    chain = ops.Resblock24Chain(raw, dev, 'fp16' if row.wf else 'hi_lo')
    if pz:
        fp.fence_weights(chain)
    ins = {'blobs': chain.blobs}
    for b, c in enumerate(cases):
        ins['x.%d' % b] = nhwc16(c.p['x'], dev, pz)

    def launch():
        if row.batch:
            out = ops.resblock24_chain_b(chain, [ins['x.%d' % b] for b in range(len(cases))], p0['act'])
        else:
            out = [ops.resblock24_chain(chain, ins['x.0'], p0['act'])]
        return list(out), lambda: [{'out': planar64(o.cpu(), 24)} for o in out]
    return ins, launch


FORMATS = (('out', None), ('f16', 'float16'), ('u8', 'uint8'))


def formats_of(run):
    """The result formats a head row is asked for: all three at the small shapes; fp32 alone at the zero-base walk and tiny shapes,
    fp32 and uint8 at the based ones."""
    if fv.kind(run) == 'small':
        return FORMATS
    return FORMATS[:1] if fv.factor(run) is None else (FORMATS[0], FORMATS[2])


def run_row(i, run, form, dev):
    """One run of row i and its fenced twin -> {'key', 'n_tiles', 'lds', 'same', 'tail' (probe rows), '<map>.<output>': raw result on
    the cpu, 'fence': '' or what the fenced run found, 'equal': the fenced run's raw result tensors equal the plain run's}."""
    res, raw = _run_row(i, run, form, dev, False)
    res2, raw2 = _run_row(i, run, form, dev, True)
    bad = [res2['fence']] if res2['fence'] else []
    for k in ('key', 'n_tiles', 'lds'):
        if res2[k] != res[k]:
            bad.append('the fenced run reports %s %d, the plain run %d' % (k, res2[k], res[k]))
    if not res2['same']:
        bad.append('an input of the fenced run was written to')
    if res2.get('tail', 1) != 1:
        bad.append('the probe kernel of the fenced run wrote behind 12 x n_tiles words')
    res['fence'] = '\n'.join(bad)
    res['equal'] = int(len(raw) == len(raw2) and all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) for a, b in zip(raw, raw2)))
    return res


def _run_row(i, run, form, dev, fenced):
    """One launch of row i -> (the results as run_row describes them, [raw result tensors on the cpu]).  fenced: every input between
    the fences of footprint.fenced_input, every allocation of ops between 0xA5 fences, entered inside the run's stream so that the
    fence fills are ordered on it; 'fence' holds footprint.judge's verdict."""
    from refvsr_amd import ops
    row = fv.ROWS[i]
    pz = 'nan' if fenced else None
    fp.reset_inputs()
    cases = fv.get_cases(i, run, form)
    hw = fv.shape(row, run)
    for k in SETTER_ENV:
        assert not os.environ.get(k), 'the rows set the resblock24 setters themselves: %s must not be set' % k
    if row.entry in ('conv_last', 'hr_last'):
        ins, launch = _head(row, cases, dev, formats_of(run), pz)
    elif row.entry == 'conf_alpha':
        ins, launch = _conf(row, cases, dev, pz)
    elif row.entry == 'rb24':
        ins, launch = _blocks(row, cases, dev, pz)
    else:
        ins, launch = _conv(row, cases, dev, pz)
    before = dict((k, v.clone()) for k, v in ins.items())
    res = {}
    with setters(row, hw, dev) as probe:
        with walk_stream(run) as stream:
            res['key'], res['n_tiles'], res['lds'] = query(row, hw, stream)
            if probe is not None:
                assert probe.numel() == PROBE_WORDS * res['n_tiles'] + PROBE_TAIL, 'probe buffer sized for another tile count'
            if fenced:
                with fp.fenced_outputs(ops) as fo:
                    raw, fetch = launch()
                    res['fence'] = fp.judge(fo, raw)
            else:
                raw, fetch = launch()
        if probe is not None:
            res['tail'] = int((probe[-PROBE_TAIL:].cpu() == PROBE_MARK).all())
    res['same'] = int(all(torch.equal(v, before[k]) for k, v in ins.items()))
    for b, outs in enumerate(fetch()):
        for k, v in outs.items():
            res['%d.%s' % (b, k)] = v
    fp.reset_inputs()
    return res, [t.cpu() for t in raw]


def main(knob, path):
    t0 = time.time()
    for k, v in fv.KNOBS[knob].items():
        assert os.environ.get(k) == v, 'knob %s did not arrive' % k
    assert torch.cuda.is_available(), 'the child needs a GPU'
    dev = torch.device('cuda:0')
    out = {}
    for i, run, form in runs_of(knob):
        for k, v in run_row(i, run, form, dev).items():
            out['%s.%s' % (tag(i, run, form), k)] = v.numpy() if isinstance(v, torch.Tensor) else np.array(v) if isinstance(v, str) else np.int64(v)
    out['seconds'] = np.float64(time.time() - t0)
    np.savez(path, **out)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
