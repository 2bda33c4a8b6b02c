"""Every one of the 3 resblock48_kernel and 6 resblock_lean_kernel instantiations on a real MI355X, bit for bit, the persistent tile
walk included: each run of each row of tests/block_variant_cases.py is ONE launch through the entry point of refvsr_amd.ops that the
engine uses and must (1) be the row's variant by the library's own word (refvsr_resblock48_variant / refvsr_resblock_lean_variant on
the arguments that were launched, on the stream they were launched on, under the process's probe buffer and wave setter), with the
row's LDS bytes and tile count, and on a walk run with a grid of less than half the tiles -- the restated rv_tile_range is then
asked again, for THAT grid, whether every workgroup walks, through an interior and an edge tile, across a map boundary in the
three-map rows; (2) equal the float64 reference bit for bit -- one round-to-nearest-even into fp16 -- on EVERY map of a multi-map
launch; (3) leave its inputs, the other maps' included, unchanged.

The probe row runs with a zeroed buffer of 12 x n_tiles words and a marked tail: stamp 0 of a workgroup is non-zero exactly for the
workgroups below the grid, the words from 12 x grid on are zero and the tail is untouched.

A walk run goes to a side stream whose CU budget is 8 (fixed_variant_child.walk_stream).  The wave setter, the probe pointer and the CU
budget are restored in `finally` blocks.  No tolerance appears in this file: if the fp16 premise case fails (the matrix unit does not
add exactly representable sums exactly: tests/test_gpu_exact.py), the rows follow the fallback rule of exact_cases.matches.  On the
MI355X it holds and every run is bit-equal.  Every run appends its lines, and the file its wall time, to
gpu_block_variants_report.txt next to the other GPU reports of a run; profiles/gpu_block_variants_report.txt is that file from the
MI355X, with three kernel mutations that this file catches and the older exact suite does not."""
import contextlib
import ctypes
import os
import time

import pytest
import torch

import block_variant_cases as bv
import conv_variant_child as generic
import exact_cases as ec
import fixed_variant_child as child
import footprint as fp
from test_gpu_fixed_variants import REPORT as FIXED_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(FIXED_REPORT), 'gpu_block_variants_report.txt')
RUNS = [(i, run) for i, r in enumerate(bv.ROWS) for run in bv.runs_of(r)]
T0 = [None]


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
    assert not os.environ.get('REFVSR_RESBLOCK_WAVES'), 'the rows set the wave count themselves: REFVSR_RESBLOCK_WAVES must not be set'
    T0[0] = time.time()
    yield torch.device('cuda:0')
    report('file wall time %.1f s' % (time.time() - T0[0]))


@pytest.fixture(scope='module')
def premise(dev):
    c = ec.get_case(ec.PREMISE)
    out, _, _ = generic.run_conv(c, dev)
    n, txt = ec.mismatch(out.double(), c.want['out'], c.g_out, False)
    report('%-72s %s' % ('premise fp16', txt))
    return n == 0


@contextlib.contextmanager
def setters(row, hw, run, dev):
    """The wave setter and the probe buffer of a row; yields the buffer (or None).  The probe kernel writes 12 words per workgroup at
    buf[12 * blockIdx.x + i] (resblock48.hip: R48_STAMP) and the grid is at most n_tiles: 12 x n_tiles words hold every stamp; a
    marked tail behind them must come back untouched.  Walk runs stamp the workgroup's SECOND tile (the stamps under has_next)."""
    from refvsr_amd import hip
    h = hip.lib()
    buf = None
    try:
        if row.waves:
            hip.check(h.refvsr_set_resblock_waves(row.waves), 'set_resblock_waves')
        if row.probe:
            n = bv.n_tiles(row, hw)
            buf = torch.zeros(child.PROBE_WORDS * n + child.PROBE_TAIL, dtype=torch.int64)
            buf[child.PROBE_WORDS * n:] = child.PROBE_MARK
            buf = buf.to(dev)
            hip.check(h.refvsr_set_probe(ctypes.c_void_p(buf.data_ptr()), 1 if run == 'walk' else 0), 'set_probe')
        yield buf
    finally:
        h.refvsr_set_probe(None, 0)
        h.refvsr_set_resblock_waves(8)


def query(row, hw, stream):
    """(key, n_tiles, grid, lds) by the library's own query on the launched arguments and stream."""
    from refvsr_amd import hip
    key, n, grid, lds = [ctypes.c_int(-1) for _ in range(4)]
    out = [ctypes.byref(v) for v in (key, n, grid, lds)]
    if row.kernel == 'rb48':
        hip.check(hip.lib().refvsr_resblock48_variant(row.act, bv.maps(row), hw[0], hw[1], stream, *out), 'resblock48_variant')
    else:
        hip.check(hip.lib().refvsr_resblock_lean_variant(row.c, hw[0], hw[1], stream, *out), 'resblock_lean_variant')
    return key.value, n.value, grid.value, lds.value


def prepare(row, cases, dev, pz=None):
    """-> (inputs, launch): the device tensors of the launch and the call through refvsr_amd.ops.  pz: None, or 'nan' = every map
    (each map of a multi-map row on its own), the blobs, the weight packs and the biases between the NaN fences of tests/footprint.py"""
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv
    p0 = cases[0].p
    raw = [((child.f32(w1), child.f32(b1)), (child.f32(w2), child.f32(b2))) for (w1, b1, w2, b2) in p0['blocks']]
    ins = dict(('x.%d' % b, child.nhwc16(c.p['x'], dev, pz)) for b, c in enumerate(cases))
    xs = [ins['x.%d' % b] for b in range(len(cases))]
    if row.kernel == 'rb48':
        chain = ops.Resblock48Chain(raw, dev)
        if pz:
            fp.fence_weights(chain)
        ins['blobs'] = chain.blobs
        if row.batch:
            return ins, lambda: list(ops.resblock48_chain_b(chain, xs, p0['act']))
        return ins, lambda: [ops.resblock48_chain(chain, xs[0], p0['act'])]
    assert ops.resblock_fits(row.c)
    pairs = [tuple(ops.ConvWeights(pack_conv(w, b, [row.c], False), dev, 'hi_lo') for (w, b) in blk) for blk in raw]
    for k, (a, b) in enumerate(pairs):
        if pz:                                               # before ResblockChain takes the pointers
            fp.fence_weights(a)
            fp.fence_weights(b)
        ins.update({'w1.%d' % k: a.wpack, 'b1.%d' % k: a.bias, 'w2.%d' % k: b.wpack, 'b2.%d' % k: b.bias})
    if row.entry == 'chain':
        chain = ops.ResblockChain(pairs)
        return ins, lambda: [ops.resblock_chain(chain, xs[0], p0['act'], p0['post'])]
    assert len(pairs) == 1
    return ins, lambda: [ops.resblock(pairs[0][0], pairs[0][1], xs[0], p0['act'], p0['post'])]


def run_row(i, run, dev, fenced=False):
    """One run of row i -> {'key', 'n_tiles', 'grid', 'lds', 'same', 'probe' (probe rows: the buffer on the cpu), 'out': [map], 'raw':
    [the raw result tensors on the cpu]}.  fenced: every input between NaN fences and every allocation of ops (outputs and the
    chain's scratch maps) between 0xA5 fences, entered inside the run's stream so that the fence fills are ordered on it; 'fence' holds
    footprint.judge's verdict ('' = all is well)."""
    from refvsr_amd import ops
    row = bv.ROWS[i]
    cases = bv.get_cases(i, run)
    hw = bv.shape(row, run)
    fp.reset_inputs()
    ins, launch = prepare(row, cases, dev, 'nan' if fenced else None)
    before = dict((k, v.clone()) for k, v in ins.items())
    res = {}
    with setters(row, hw, run, dev) as probe:
        with child.walk_stream(run) as stream:
            res['key'], res['n_tiles'], res['grid'], res['lds'] = query(row, hw, stream)
            assert probe is None or probe.numel() == child.PROBE_WORDS * res['n_tiles'] + child.PROBE_TAIL, 'probe buffer sized for another tile count'
            if fenced:
                with fp.fenced_outputs(ops) as fo:
                    outs = launch()
                    res['fence'] = fp.judge(fo, outs)
            else:
                outs = launch()
        if probe is not None:
            res['probe'] = probe.cpu()
    res['same'] = all(torch.equal(v, before[k]) for k, v in ins.items())
    res['raw'] = [o.cpu() for o in outs]
    res['out'] = [child.planar64(o, row.c) for o in res['raw']]
    fp.reset_inputs()
    return res


def judge(i, run, res, premise_ok):
    """The assertions of one run on what the runner returned."""
    r = bv.ROWS[i]
    cases = bv.get_cases(i, run)
    hw = bv.shape(r, run)
    n = bv.n_tiles(r, hw)
    assert res['key'] == bv.key(r), 'planned variant key %d, the row is for %d %s' % (res['key'], bv.key(r), r.variant)
    assert res['lds'] == r.lds and res['n_tiles'] == n and 1 <= res['grid'] <= n
    if run == 'walk':
        g = res['grid']
        assert 2 * g < n and g in bv.grids(r), 'every workgroup must walk at least two tiles (grid %d, %d tiles)' % (g, n)
        rng = bv.tile_ranges(n, g)
        later = [bv.is_interior(hw, y, x) for _, y, x in (bv.tile_origin(hw, t) for t in bv.later_tiles(n, g))]
        assert min(hi - lo for lo, hi in rng) >= 2 and max(hi - lo for lo, hi in rng) >= 3 and any(later) and not all(later)
        assert not r.batch or any(lo // (n // r.batch) != (hi - 1) // (n // r.batch) for lo, hi in rng), 'no range spans two maps'
    elif run == 'tiny':
        assert n == 1 == res['grid']
    assert res['same'], 'an input was written to'
    if r.probe:
        words = res['probe'][:-child.PROBE_TAIL].view(-1, child.PROBE_WORDS)
        assert bool((res['probe'][-child.PROBE_TAIL:] == child.PROBE_MARK).all()), 'the probe kernel wrote behind 12 x n_tiles words'
        assert not words[res['grid']:].any(), 'stamps of workgroups that were not launched'
        assert bool((words[:res['grid'], 0] != 0).all()), 'a launched workgroup left no entry stamp'
    assert len(res['out']) == len(cases)
    ok, lines = True, []
    for b, (c, got) in enumerate(zip(cases, res['out'])):
        assert got.shape == c.want['out'].shape
        o, _, txt = ec.matches(got, c.want['out'], c, True, premise_ok)
        ok = ok and o
        lines.append('%s%s' % ('map %d: ' % b if r.batch else '', txt))
        report('%-72s key=%-2d tiles=%-3d grid=%-3d lds=%-6d %s mismatches=%s' % (c.name, res['key'], res['n_tiles'], res['grid'], res['lds'], c.line(), txt))
    assert ok, '%s: %s' % (cases[0].name, '; '.join(lines))


@pytest.mark.parametrize('i,run', RUNS, ids=['%02d-%s' % t for t in RUNS])
def test_block_variant_run_is_planned_and_bit_equal(i, run, dev, premise):
    res = run_row(i, run, dev)
    judge(i, run, res, premise)
    # the fenced second run (tests/footprint.py) must pass the same judgement, with the same plan and the same raw maps
    res2 = run_row(i, run, dev, fenced=True)
    name = bv.get_cases(i, run)[0].name
    equal = len(res['raw']) == len(res2['raw']) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(res['raw'], res2['raw']))
    report('%-72s key=%-2d fenced run: fences=%s equal=%s' % (name, res2['key'], 'BROKEN' if res2['fence'] else 'ok', 'ok' if equal else 'NO'))
    assert not res2['fence'], '%s, fenced run: %s' % (name, res2['fence'])
    assert equal, '%s: the fenced run does not equal the plain run' % name
    assert [res2[k] for k in ('key', 'n_tiles', 'grid', 'lds')] == [res[k] for k in ('key', 'n_tiles', 'grid', 'lds')], 'the plan moved with the pointers'
    judge(i, run, res2, premise)
