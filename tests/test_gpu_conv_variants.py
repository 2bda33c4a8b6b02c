"""Every one of the 56 conv_mfma_kernel instantiations on a real MI355X, bit for bit: each row of tests/conv_variant_cases.py is run
through refvsr_conv_mfma and must (1) be planned as the row's variant, by the library's own word (refvsr_conv_variant on the
descriptor that was launched, under the process's knobs), (2) equal the float64 reference bit for bit -- one round-to-nearest-even
for fp16 HWC outputs, no rounding for planar and fp32 outputs -- and (3) leave its inputs unchanged and the channel padding of HWC
outputs zero.  Resident variants run twice: 19 x 45, and 33 x 70 with the workgroup cap at 2 (the persistent walk and its prefetch).

Rows without a knob run in this process.  The REFVSR_CONV_* knobs are read once per process, so each other knob set gets ONE fresh
child (tests/conv_variant_child.py), one after the other; a child writes outputs and keys to an .npz and this file judges them.  If
a child ends by a signal, a non-zero exit or its timeout, no further child is started and the rows waiting for one fail with that
reason.  CHILD_SECONDS is a child's measured wall time on the MI355X (torch import + library load dominate); the timeout is three
times that, at least 60 s.

If a premise case fails (the matrix unit does not add exactly representable sums exactly: tests/test_gpu_exact.py for the fp16
MFMA, tests/test_gpu_f32_exact.py for the fp32 one), the rows follow the fallback rule of exact_cases.matches.  On the MI355X both
hold and every row is bit-equal (profiles/gpu_conv_variants_report.txt, which also records two kernel mutations that this file
catches)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import conv_variant_cases as cv
import conv_variant_child as child
import exact_cases as ec
import f32_cases as fc
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(OPS_REPORT), 'gpu_conv_variants_report.txt')
CHILD_SECONDS = 2.9                 # measured with the fenced runs (2.1 to 2.9 s over two runs of both children): profiles/gpu_footprint_report.txt
CHILD_TIMEOUT = max(60.0, 3 * CHILD_SECONDS)
IDS = ['%02d' % i for i in range(len(cv.ROWS))]


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
    assert not [k for k in os.environ if k.startswith('REFVSR_CONV_')], 'the rows without a knob need a process without one'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def premises(dev):
    """{'fp16' | 'f32': holds}: the two premise cases on the generic kernel."""
    res = {}
    for kind, c in (('fp16', ec.get_case(ec.PREMISE)), ('f32', fc.get_case(fc.PREMISE))):
        out, _, _ = child.run_conv(c, dev)
        n, txt = ec.mismatch(out.double(), c.want['out'], c.g_out, False)
        report('%-96s %s' % ('premise ' + kind, txt))
        res[kind] = n == 0
    return res


@pytest.fixture(scope='module')
def children(dev, tmp_path_factory):
    """{knob set: (the child's .npz as a dict | None, reason)}; the children run one after the other, none after a failed one."""
    tmp = tmp_path_factory.mktemp('conv_variant_children')
    res, failed = {}, None
    for knob, env in cv.KNOBS.items():
        if not knob:
            continue
        if failed:
            res[knob] = (None, 'child not started: ' + failed)
            continue
        path = str(tmp / (knob + '.npz'))
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_variant_child.py'), knob, path],
                               env=dict(os.environ, **env), timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            why = None if r.returncode == 0 else ('ended by signal %d' % -r.returncode if r.returncode < 0 else 'exit status %d' % r.returncode)
            tail = r.stdout.decode(errors='replace')[-2000:]
        except subprocess.TimeoutExpired as e:
            why, tail = 'timeout after %.0f s' % CHILD_TIMEOUT, (e.stdout or b'').decode(errors='replace')[-2000:]
        wall = time.time() - t0
        if why:
            failed = 'child %s: %s' % (knob, why)
            res[knob] = (None, failed + '\n' + tail)
            report('child %-8s %s after %.1f s' % (knob, why, wall))
            continue
        with np.load(path) as z:
            res[knob] = (dict((k, z[k]) for k in z.files), '')
        report('child %-8s %d runs, wall %.1f s (of which %.1f s after the imports)' % (knob, len(child.runs_of(knob)), wall, float(res[knob][0]['seconds'])))
    return res


@pytest.mark.parametrize('i', range(len(cv.ROWS)), ids=IDS)
def test_variant_row_is_planned_and_bit_equal(i, dev, premises, request):
    r = cv.ROWS[i]
    f32 = cv.mode(r) == 'f32'
    for tag, _, walk in [t for t in child.runs_of(r.knob) if t[1] == i]:
        c = cv.get_case(i, walk)
        if r.knob:
            data, reason = request.getfixturevalue('children')[r.knob]
            assert data is not None, reason
            out, key, same = torch.from_numpy(data['out_' + tag]), int(data['key_' + tag]), bool(data['same_' + tag])
            fence, equal = str(data['fence_' + tag]), bool(data['equal_' + tag])
        else:
            out, key, same = child.run_conv(c, dev)
            fence, equal = child.fenced_twin(c, dev, out, key)
        assert key == cv.variant_key(r.variant), 'planned variant key %d, the row is for %d %s' % (key, cv.variant_key(r.variant), r.variant)
        assert same, 'an input was written to'
        if r.out == 'planar':
            assert out.dtype == torch.float32
            got = out.double()
        else:
            assert out.dtype == (torch.float32 if f32 else torch.float16) and out.shape[2] == (fc.pad4 if f32 else ec.pad8)(r.cout)
            got = child.planar64(out, r.cout)
        fp16 = not f32 and r.out != 'planar'
        ok, n, txt = ec.matches(got, c.want['out'], c, fp16, premises['f32' if f32 else 'fp16'])
        report('%-96s knob=%-6s key=%-5d %s mismatches=%s' % (c.name, r.knob or 'none', key, c.line(), txt))
        assert ok, '%s: %s' % (c.name, txt)
        # the fenced second run (tests/footprint.py): NaN around every map, the weights and the bias, 0xA5 around the output
        report('%-96s knob=%-6s key=%-5d fenced run: fences=%s equal=%s' % (c.name, r.knob or 'none', key, 'BROKEN' if fence else 'ok', 'ok' if equal else 'NO'))
        assert not fence, '%s, fenced run: %s' % (c.name, fence)
        assert equal, '%s: the fenced run does not equal the plain run' % c.name
