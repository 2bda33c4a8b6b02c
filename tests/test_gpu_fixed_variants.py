"""Every one of the 42 conv24_kernel and 24 resblock24_kernel instantiations on a real MI355X, bit for bit, the persistent tile walk
included: each row of tests/fixed_variant_cases.py is launched through its entry point and must (1) be planned as the row's variant,
by the library's own word (refvsr_conv24_variant / refvsr_resblock24_variant on the arguments that were launched, under the process's
knob and setters), with the row's LDS bytes and the tile count its walk shape rests on, (2) equal the float64 reference bit for bit --
one round-to-nearest-even for fp16 maps, no rounding for the fp32, fp16 and uint8 results of the heads, the conf_max by-product
included where up = 1 -- on EVERY map of a multi-map launch, and (3) leave its inputs unchanged.  Every row runs at its small shape
and at its walk shape (a side stream with a CU budget of 8: every workgroup takes two tiles or more), the marked rows at 7 x 5 too.
The four head rows run these with a zero base frame and once more per factor (x4, x2) with an exact non-zero base
(fixed_variant_cases: `small_x4`, `walk_x2`, ...): all three result formats at the small shapes, fp32 and uint8 at the walk and
tiny ones, the fenced twin and the key / tile count / LDS equality unchanged (profiles/gpu_head_base_report.txt).

Rows without a knob run in this process.  REFVSR_CONV48_WAVES is read once per process, so the 8-wave 48 -> 48 conv gets ONE fresh
child (tests/fixed_variant_child.py), which writes its results to an .npz that this file judges.  A child that ends by a signal, a
non-zero exit or its timeout fails the row with that reason; nothing further is started on the GPU by that fixture.  CHILD_SECONDS
is the child's measured wall time on the MI355X (torch import + library load dominate); the timeout is three times that, at least
60 s.  Setter state (waves, store, probe buffer, CU budget) is restored in `finally` blocks by the runner.

The two probe rows run with a zeroed buffer of 12 x n_tiles words and a marked tail: the map must be bit-equal and the tail untouched;
nothing is asserted about the stamps.

If the fp16 premise case fails (the matrix unit does not add exactly representable sums exactly: tests/test_gpu_exact.py), the rows
follow the fallback rule of exact_cases.matches.  On the MI355X it holds and every run is bit-equal
(profiles/gpu_fixed_variants_report.txt, which also records two kernel mutations that this file catches)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import conv_variant_child as generic
import exact_cases as ec
import fixed_variant_cases as fv
import fixed_variant_child as child
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(OPS_REPORT), 'gpu_fixed_variants_report.txt')
CHILD_SECONDS = 2.4                 # measured with the fenced runs (2.2 and 2.4 s over two runs): profiles/gpu_footprint_report.txt; re-measured with
#                                     the based head runs in the file (they run in this process, not in the child): 2.1 s, profiles/gpu_head_base_report.txt
CHILD_TIMEOUT = max(60.0, 3 * CHILD_SECONDS)
IDS = ['%02d' % i for i in range(len(fv.ROWS))]
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
    assert not os.environ.get('REFVSR_CONV48_WAVES'), 'the rows without a knob need a process without one'
    T0[0] = time.time()
    yield torch.device('cuda:0')
    report('file wall time %.1f s' % (time.time() - T0[0]))


@pytest.fixture(scope='module')
def premise(dev):
    c = ec.get_case(ec.PREMISE)
    out, _, _ = generic.run_conv(c, dev)
    n, txt = ec.mismatch(out.double(), c.want['out'], c.g_out, False)
    report('%-104s %s' % ('premise fp16', txt))
    return n == 0


@pytest.fixture(scope='module')
def w8_child(dev, tmp_path_factory):
    """(the child's .npz as a dict | None, reason)"""
    path = str(tmp_path_factory.mktemp('fixed_variant_child') / 'W8.npz')
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fixed_variant_child.py'), 'W8', path],
                           env=dict(os.environ, **fv.KNOBS['W8']), timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        why = None if r.returncode == 0 else ('ended by signal %d' % -r.returncode if r.returncode < 0 else 'exit status %d' % r.returncode)
        tail = r.stdout.decode(errors='replace')[-2000:]
    except subprocess.TimeoutExpired as e:
        why, tail = 'timeout after %.0f s' % CHILD_TIMEOUT, (e.stdout or b'').decode(errors='replace')[-2000:]
    wall = time.time() - t0
    if why:
        report('child W8 %s after %.1f s' % (why, wall))
        return None, 'child W8: %s\n%s' % (why, tail)
    with np.load(path) as z:
        data = dict((k, z[k]) for k in z.files)
    report('child W8 %d runs, wall %.1f s (of which %.1f s after the imports)' % (len(child.runs_of('W8')), wall, float(data['seconds'])))
    return data, ''


def _from_child(data, t):
    res = {}
    for k, v in data.items():
        if k.startswith(t + '.'):
            res[k[len(t) + 1:]] = torch.from_numpy(v) if v.ndim else str(v) if v.dtype.kind == 'U' else int(v)
    return res


def judge(i, run, form, res, premise_ok):
    """The assertions of one run on what the runner returned."""
    r = fv.ROWS[i]
    cases = fv.get_cases(i, run, form)
    hw = fv.shape(r, run)
    assert res['key'] == fv.key(r), 'planned variant key %d, the row is for %d %s' % (res['key'], fv.key(r), r.variant)
    assert res['lds'] == r.lds and res['n_tiles'] == fv.n_tiles(r, hw)
    if fv.kind(run) == 'walk':
        assert res['n_tiles'] >= 2 * fv.walk_bound(r) + 1, 'every workgroup must walk at least two tiles'
    assert res['same'], 'an input was written to'
    if r.setters.get('probe'):
        assert res['tail'] == 1, 'the probe kernel wrote behind 12 x n_tiles words'
    ok, lines = True, []
    for b, c in enumerate(cases):
        want = dict(c.want)
        if r.entry in ('conv_last', 'hr_last'):
            assert ('base' in c.p) == (fv.factor(run) is not None) and sorted(k for k, _ in child.formats_of(run)) == sorted(
                k[len('%d.' % b):] for k in res if k.startswith('%d.' % b))
            stored = dict(zip(('f16', 'u8'), (t.double() for t in ec.result_formats(c.want['out']))))
            want.update((k, stored[k]) for k, _ in child.formats_of(run) if k in stored)
        got = dict((k[len('%d.' % b):], v.double()) for k, v in res.items() if k.startswith('%d.' % b))
        assert set(got) == set(want), (sorted(got), sorted(want))
        for k in sorted(got):
            assert got[k].shape == want[k].shape, (k, tuple(got[k].shape), tuple(want[k].shape))
            if k in ('f16', 'u8'):
                n = int((got[k] != want[k]).sum())
                o, txt = (n == 0 if premise_ok else float((got[k] - want[k]).abs().max()) <= (2.0 ** -10 if k == 'f16' else 1)), '%d differ' % n
            else:
                o, n, txt = ec.matches(got[k], want[k], c, fv.is_fp16(r) and k == 'out', premise_ok)
            ok = ok and o
            lines.append('%s%s: %s' % ('map %d ' % b if r.batch else '', k, txt))
        report('%-104s knob=%-4s key=%-13d tiles=%-3d %s mismatches=%s' % (c.name, r.knob or 'none', res['key'], res['n_tiles'], c.line(),
                                                                         '; '.join(l for l in lines if l.startswith('map %d ' % b) or not r.batch)))
    assert ok, '%s: %s' % (cases[0].name, '; '.join(lines))
    # the fenced second run (tests/footprint.py): NaN around every map (each map of a multi-map row on its own), the blob and the
    # fp32 operands, 0xA5 around every allocation of ops -- outputs in every result format and the chain's scratch maps
    report('%-104s knob=%-4s key=%-13d fenced run: fences=%s equal=%s' % (cases[0].name, r.knob or 'none', res['key'], 'BROKEN' if res['fence'] else 'ok',
                                                                         'ok' if res['equal'] else 'NO'))
    assert not res['fence'], '%s, fenced run: %s' % (cases[0].name, res['fence'])
    assert res['equal'], '%s: the fenced run does not equal the plain run' % cases[0].name


@pytest.mark.parametrize('i', range(len(fv.ROWS)), ids=IDS)
def test_variant_row_is_planned_and_bit_equal(i, dev, premise, request):
    r = fv.ROWS[i]
    data = None
    if r.knob:
        data, reason = request.getfixturevalue('w8_child')
        assert data is not None, reason
    for run in fv.runs_of(r):
        for form in fv.forms(r):
            res = _from_child(data, child.tag(i, run, form)) if r.knob else child.run_row(i, run, form, dev)
            judge(i, run, form, res, premise)
