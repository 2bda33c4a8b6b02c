"""The launch plans of the fixed-channel kernels (refvsr_amd/csrc/fixed_plan.h), pinned on the CPU.

Which conv24_kernel / resblock24_kernel instantiation an entry point runs depends on the op, its channel counts, single- or multi-map,
the weight format, REFVSR_CONV48_WAVES, the resblock24 knobs and a tile-count threshold against the stream's CU budget.  Where two
variants compute the same numbers a slipped choice costs speed only and no parity test sees it.  tools/conv_plan_dump (plain C++, no
HIP) prints the plan of every row of tests/golden/fixed_plan_cases.txt; tests/golden/fixed_plan_expected.txt holds what the launchers
chose before the plans were functions of their own (recorded from those launchers' code, not from fixed_plan.h: see the cases file)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
C24 = ('COUT', 'NCG0', 'NCG1', 'NWV', 'TH', 'WPS', 'SHUF', 'CONF', 'HALF', 'MM', 'WF')
RB24 = ('RELU', 'NWV', 'PROBE', 'TH', 'STORE', 'HEAD', 'WF')


def _rows(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return [l.rstrip('\n') for l in f]


def _is_rb24(case):
    return 'op=rb24' in case.split() or 'op=hr_last' in case.split()


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    """The built program as a function: arguments -> output lines."""
    exe = str(tmp_path_factory.mktemp('fixed_plan') / 'conv_plan_dump')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'refvsr_amd', 'csrc'), 'plan_dump', 'PLAN_DUMP=' + exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith('REFVSR_CONV')}      # (the program reads no knob from the environment)
    return lambda *args: subprocess.check_output([exe] + list(args), env=env).decode().splitlines()


@pytest.fixture(scope='module')
def plans(dump):
    """[(case row, plan as {field: text} or the `rejected: ...` line)]"""
    cases = [l for l in _rows('fixed_plan_cases.txt') if l.split('#')[0].strip()]
    out = dump('--fixed', os.path.join(GOLDEN, 'fixed_plan_cases.txt'))
    assert len(out) == len(cases)
    return [(c, o if o.startswith('rejected:') else dict(t.split('=') for t in o.split())) for c, o in zip(cases, out)]


@pytest.fixture(scope='module')
def variants(dump):
    """{'c24' | 'rb24': ([template arguments], [key])} of the two lists"""
    out = [dict(t.split('=') for t in l.split()) for l in dump('--fixed-variants')]
    got = {}
    for name, cols in (('c24', C24), ('rb24', RB24)):
        mine = [v for v in out if ('COUT' in v) == (name == 'c24')]
        got[name] = ([tuple(int(v[k]) for k in cols) for v in mine], [int(v['key']) for v in mine])
    return got


def test_plans_equal_the_recorded_ones(plans):
    want = _rows('fixed_plan_expected.txt')
    cols = {False: want[0].split(':')[1].split(), True: want[1].split(':')[1].split()}      # conv rows | rb24 and hr_last rows
    assert tuple(cols[False][:11]) == C24 and tuple(cols[True][:7]) == RB24
    want = want[2:]
    assert len(want) == len(plans) and len(plans) > 1800
    wrong = []
    for (case, got), w in zip(plans, want):
        names = cols[_is_rb24(case)]
        w = w if w.startswith('rejected:') else dict(zip(names, w.split()))
        if isinstance(got, dict) and isinstance(w, dict):
            assert list(got) == names and len(w) == len(names)
            diff = ['%s: %s, recorded %s' % (k, got[k], w[k]) for k in names if got[k] != w[k]]
        else:
            diff = [] if got == w else ['%s, recorded %s' % (got, w)]
        if diff:
            wrong.append('%s\n    %s' % (case, '; '.join(diff)))
    assert not wrong, '%d of %d plans differ from the recorded ones:\n%s' % (len(wrong), len(want), '\n'.join(wrong[:20]))


def test_every_plan_names_a_listed_variant(plans, variants):
    for name, n in (('c24', 42), ('rb24', 24)):
        listed, keys = variants[name]
        assert len(listed) == n and len(set(listed)) == n and len(set(keys)) == n       # one list entry, one key per instantiation
    stray = [case for case, p in plans if isinstance(p, dict) and
             (tuple(int(p[k]) for k in RB24) not in variants['rb24'][0] if _is_rb24(case) else
              tuple(int(p[k]) for k in C24) not in variants['c24'][0])]
    assert not stray, 'plans outside RV_C24_VARIANTS / RV_RB24_VARIANTS:\n' + '\n'.join(stray[:20])


def test_every_listed_variant_is_reached(plans, variants):
    """Nothing is unreachable at plan level: each of the 42 + 24 entries is the plan of at least one row."""
    reached_rb = set(tuple(int(p[k]) for k in RB24) for case, p in plans if isinstance(p, dict) and _is_rb24(case))
    reached_c = set(tuple(int(p[k]) for k in C24) for case, p in plans if isinstance(p, dict) and not _is_rb24(case))
    missing = [v for v in variants['c24'][0] if v not in reached_c] + [v for v in variants['rb24'][0] if v not in reached_rb]
    assert not missing, 'listed variants that no row reaches: %s' % missing
