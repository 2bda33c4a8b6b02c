"""The launch plan of the generic MFMA convolution (refvsr_amd/csrc/conv_plan.h), pinned on the CPU.

Which conv_mfma_kernel instantiation a descriptor runs, and with which LDS carve, decides speed and nothing else: every variant
computes the same numbers (tests/test_gpu_conv_variants.py runs all 56 bit for bit against one float64 reference), so no parity test
sees a slipped threshold.  tools/conv_plan_dump (plain C++, no HIP) prints the plan of
every descriptor row of tests/golden/conv_plan_cases.txt; tests/golden/conv_plan_expected.txt holds the plans the launcher chose
before the plan was a function of its own (recorded from that launcher's code, not from conv_plan.h)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
VARIANT = ('MT', 'TILES', 'F32', 'GATHER', 'RESIDENT', 'EPI', 'NW', 'HI1')


def _rows(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return [l.rstrip('\n') for l in f]


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    """The built program as a function: arguments -> output lines."""
    exe = str(tmp_path_factory.mktemp('conv_plan') / 'conv_plan_dump')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'refvsr_amd', 'csrc'), 'plan_dump', 'PLAN_DUMP=' + exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith('REFVSR_CONV_')}     # (the program reads no knob from the environment)
    return lambda *args: subprocess.check_output([exe] + list(args), env=env).decode().splitlines()


@pytest.fixture(scope='module')
def plans(dump):
    """[(case row, plan as {field: text} or the `rejected: ...` line)]"""
    cases = [l for l in _rows('conv_plan_cases.txt') if l.split('#')[0].strip()]
    out = dump(os.path.join(GOLDEN, 'conv_plan_cases.txt'))
    assert len(out) == len(cases)
    return [(c, o if o.startswith('rejected:') else dict(t.split('=') for t in o.split())) for c, o in zip(cases, out)]


@pytest.fixture(scope='module')
def variants(dump):
    out = [dict(t.split('=') for t in l.split()) for l in dump('--variants')]
    return [tuple(int(v[k]) for k in VARIANT) for v in out], [int(v['key']) for v in out]


def test_plans_equal_the_recorded_ones(plans):
    want = _rows('conv_plan_expected.txt')
    cols = want[0].lstrip('# ').split()
    want = want[1:]
    assert len(want) == len(plans) and len(plans) > 1900
    wrong = []
    for (case, got), w in zip(plans, want):
        w = w if w.startswith('rejected:') else dict(zip(cols, w.split()))
        if isinstance(got, dict) and isinstance(w, dict):
            assert list(got) == cols
            diff = ['%s: %s, recorded %s' % (k, got[k], w[k]) for k in cols if got[k] != w[k]]
        else:
            diff = [] if got == w else ['%s, recorded %s' % (got, w)]
        if diff:
            wrong.append('%s\n    %s' % (case, '; '.join(diff)))
    assert not wrong, '%d of %d plans differ from the recorded ones:\n%s' % (len(wrong), len(want), '\n'.join(wrong[:20]))


def test_every_plan_names_a_listed_variant(plans, variants):
    listed, keys = variants
    assert len(listed) == 56 and len(set(listed)) == 56 and len(set(keys)) == 56      # one table entry, one key per instantiation
    stray = [case for case, p in plans if isinstance(p, dict) and tuple(int(p[k]) for k in VARIANT) not in listed]
    assert not stray, 'plans outside RV_CONV_VARIANTS:\n' + '\n'.join(stray[:20])


def test_reached_variants(plans, variants):
    listed, _ = variants
    reached = set(tuple(int(p[k]) for k in VARIANT) for _, p in plans if isinstance(p, dict))
    recorded = [tuple(int(x) for x in l.split()) for l in _rows('conv_plan_reached.txt') if not l.startswith('#')]
    print('variants of RV_CONV_VARIANTS that no row reaches:', [v for v in listed if v not in reached] or 'none')
    assert sorted(reached) == sorted(recorded)
