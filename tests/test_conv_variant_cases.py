"""The variant matrix of the generic MFMA convolution (tests/conv_variant_cases.py), proven on the CPU: through tools/conv_plan_dump,
row i of the table reaches exactly entry i of RV_CONV_VARIANTS under its knob set -- 56 of 56 -- at 19 x 45 and, for the resident
variants, at the 33 x 70 of their walk twin; every row obeys the rules by which its descriptor was chosen; every case is exact and
strong.  tests/test_gpu_conv_variants.py then runs each row and asks the library which variant it planned."""
import os
import subprocess

import pytest

import conv_variant_cases as cv
import exact_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ['%02d' % i for i in range(len(cv.ROWS))]


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    """The built program as a function: rows -> plans as {field: text} (a rejection raises)."""
    tmp = tmp_path_factory.mktemp('conv_variants')
    exe = str(tmp / 'conv_plan_dump')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'refvsr_amd', 'csrc'), 'plan_dump', 'PLAN_DUMP=' + exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith('REFVSR_CONV_')}

    def run(lines=None):
        if lines is None:
            return subprocess.check_output([exe, '--variants'], env=env).decode().splitlines()
        path = str(tmp / 'rows.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        out = subprocess.check_output([exe, path], env=env).decode().splitlines()
        assert len(out) == len(lines)
        bad = [(l, o) for l, o in zip(lines, out) if o.startswith('rejected:')]
        assert not bad, bad[:3]
        return [dict(t.split('=') for t in o.split()) for o in out]
    return run


@pytest.fixture(scope='module')
def listed(dump):
    out = [dict(t.split('=') for t in l.split()) for l in dump()]
    return [tuple(int(v[k]) for k in cv.FIELDS) for v in out], [int(v['key']) for v in out]


@pytest.fixture(scope='module')
def plans(dump):
    return dump([cv.dump_line(r, ec.L19) for r in cv.ROWS])


def test_rows_are_the_listed_variants(listed):
    variants, keys = listed
    assert len(variants) == 56 and len(set(variants)) == 56
    assert [r.variant for r in cv.ROWS] == variants, 'row i of the table is entry i of RV_CONV_VARIANTS'
    assert [cv.variant_key(v) for v in variants] == keys, 'variant_key is conv_variant_key'
    assert set(r.knob for r in cv.ROWS) <= set(cv.KNOBS) and list(cv.KNOBS)[0] == ''


def test_row_reaches_exactly_its_variant(plans, dump):
    got = [tuple(int(p[k]) for k in cv.FIELDS) for p in plans]
    wrong = ['row %d (%s): planned %s' % (i, r.variant, g) for i, (r, g) in enumerate(zip(cv.ROWS, got)) if g != r.variant]
    assert not wrong, '\n'.join(wrong)
    assert len(set(got)) == 56                                                  # 56 of 56 variants covered
    res = [r for r in cv.ROWS if cv.is_resident(r)]
    walk = dump([cv.dump_line(r, cv.WALK_HW) for r in res])
    assert [tuple(int(p[k]) for k in cv.FIELDS) for p in walk] == [r.variant for r in res], 'the walk twin runs the same variant'
    assert all(int(p['n_xy']) >= 3 * cv.WALK_CAP for p in walk), 'with the cap, every workgroup walks several tiles'
    assert all(int(p['prefetch']) == 1 for p in walk)


def test_rows_obey_the_rules(plans):
    from refvsr_amd import packing as pk
    for i, (r, p) in enumerate(zip(cv.ROWS, plans)):
        S, ring = int(p['S']), int(p['ring'])
        assert r.ks >= 3 and S >= 5, (i, r)
        assert S == cv.geometry(r, ec.L19)[2]
        if not cv.is_resident(r):
            assert (S + 7) // 8 > ring >= 1, 'row %d: %d chunks of 8 K-steps on %d ring slots: the ring does not wrap' % (i, (S + 7) // 8, ring)
        ho, wo = cv.geometry(r, ec.L19)[1]
        assert wo % 32 and ho % 4 and ho % 8 and ho % 16, 'row %d: partial tiles in both directions' % i
        c = cv.get_case(i)
        packed = pk.pack_conv(c.p['w'].float(), c.p['b'].float(), list(r.cins), mt=r.mt, f32=cv.mode(r) == 'f32', hi_only=cv.mode(r) == 'hi_only')
        assert packed['ksteps'] == S and packed['mt'] == r.mt and packed['wpack'].shape[0] == int(p['nz'])
        if r.out != 'planar':
            assert r.epi not in cv.PLANAR_ONLY and r.cout % 4 == 0
        if r.variant[5]:
            assert r.out == 'nhwc'


LIBRARY_QUERY = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from refvsr_amd import hip
h = hip.lib()
buf = (ctypes.c_char * 64)()
p = ctypes.cast(buf, ctypes.c_void_p).value                     # stands in for device memory: a plan reads none
keys = []
for f in json.loads(sys.stdin.read()):
    d = hip.RefvsrConv()
    d.src0, d.wpack, d.bias, d.out = p, p, p, p
    d.src1 = p if f['c1'] else None
    for k in ('mul', 'res', 'res_planar'):
        setattr(d, k, p if f[k] else None)
    d.mt_per_block, d.act_slope, d.post_slope = f['mt'], f['act'], f['post']
    for k in ('c0', 'c1', 'h_in', 'w_in', 'h_out', 'w_out', 'ksize', 'stride', 'pad', 'cout', 'ksteps', 'mul_c', 'res_c', 'out_mode', 'out_c', 'f32'):
        setattr(d, k, f[k])
    key = ctypes.c_int(-1)
    hip.check(h.refvsr_conv_variant(ctypes.byref(d), ctypes.byref(key)), 'conv_variant')
    keys.append(key.value)
print(json.dumps(keys))
"""


@pytest.mark.parametrize('knob', list(cv.KNOBS))
def test_library_plans_each_row_under_its_knob_set(knob):
    """The library itself, not the dump program: refvsr_conv_variant is host only, so a fresh process with the knob set in its
    environment -- the way the GPU test starts its children -- answers here, without a device, with each row's key."""
    import json
    import sys
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    rows = [(r, hw) for r in cv.ROWS if r.knob == knob for hw in ((ec.L19, cv.WALK_HW) if cv.is_resident(r) else (ec.L19,))]
    assert rows
    env = {k: v for k, v in os.environ.items() if not k.startswith('REFVSR_CONV_')}
    env.update(cv.KNOBS[knob])
    out = subprocess.run([sys.executable, '-c', LIBRARY_QUERY, ROOT], input=json.dumps([cv.descriptor(r, hw) for r, hw in rows]).encode(), env=env,
                         stdout=subprocess.PIPE, check=True).stdout
    assert json.loads(out.decode()) == [cv.variant_key(r.variant) for r, _ in rows]


FAMILIES = {'gather': lambda v: v[3], 'single-fp16': lambda v: v[7], 'resident': lambda v: v[4] and not v[2],
            'streamed': lambda v: not (v[2] or v[3] or v[4] or v[7]), 'fp32': lambda v: v[2]}


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_family_coverage(family, plans):
    rows = [(r, p) for r, p in zip(cv.ROWS, plans) if FAMILIES[family](r.variant)]
    assert rows
    assert any(len(r.cins) == 2 for r, _ in rows), 'two sources'
    assert set(r.mt for r, _ in rows) == ({1, 2} if family == 'single-fp16' else {1, 2, 3})
    assert any(int(p['nz']) > 1 for _, p in rows), 'nz > 1'
    assert set(r.out for r, _ in rows) == {'nhwc', 'planar'}
    for operand in ('mul', 'res'):
        assert any(cv.EPILOGUES[r.epi].get(operand) for r, _ in rows), operand
    assert any(cv.EPILOGUES[r.epi].get('post', 1.0) != 1.0 for r, _ in rows), 'post'
    if family == 'resident':
        for epi in (0, 1):
            e = [cv.EPILOGUES[r.epi] for r, _ in rows if r.variant[5] == epi]
            assert any(x.get('mul') and x.get('res') and x.get('post', 1.0) != 1.0 for x in e), 'lean and general epilogue with mul / res / post'


@pytest.mark.parametrize('i', range(len(cv.ROWS)), ids=IDS)
def test_case_is_exact_and_strong(i):
    r = cv.ROWS[i]
    for walk in ((False, True) if cv.is_resident(r) else (False,)):
        c = cv.get_case(i, walk)
        print('%-90s %s' % (c.name, c.line()))
        c.assert_strong()
        assert c.run['mt'] == r.mt and c.run['cap'] == (cv.WALK_CAP if walk else 0)
        assert (c.primary == 'hi') == (cv.mode(r) == 'hi_only') and bool(c.run.get('f32')) == (cv.mode(r) == 'f32')
        p32 = c.evaluate('f32')[0] if c.primary != 'hi' else None
        if p32 is not None:
            assert (p32['out'].double() == c.want['out']).all(), 'float32 arithmetic is not exact on this case'
