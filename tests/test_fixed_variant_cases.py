"""The variant matrix of the fixed-channel kernels (tests/fixed_variant_cases.py), proven on the CPU: the rows ARE the two lists of
refvsr_amd/csrc/fixed_plan.h -- 66 entries, in order; through tools/conv_plan_dump row i reaches exactly entry i under its knob set and
its setters, with a CU budget of 8, at the shape of every run, with the LDS bytes the row states and the tile count the walk rests on;
the conv24 rows get the same key from the loaded library, in a fresh process per knob set; every case is exact and strong; the up = 2
cases saturate (K) or show every class of sample (S); every walk shape gives every workgroup two tiles or more; and a handful of wrong
models each fail the case built for them.  tests/test_gpu_fixed_variants.py then runs each row and asks the library which variant it
planned."""
import json
import os
import subprocess
import sys

import pytest
import torch

import exact_cases as ec
import fixed_variant_cases as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ['%02d' % i for i in range(len(fv.ROWS))]
CLASS_MIN = 4


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    """The built program as a function: rows -> plans as {field: text} (a rejection raises)."""
    tmp = tmp_path_factory.mktemp('fixed_variants')
    exe = str(tmp / 'conv_plan_dump')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'refvsr_amd', 'csrc'), 'plan_dump', 'PLAN_DUMP=' + exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith('REFVSR_CONV')}      # (the program reads no knob from the environment)

    def run(lines=None):
        if lines is None:
            return [dict(t.split('=') for t in l.split()) for l in subprocess.check_output([exe, '--fixed-variants'], env=env).decode().splitlines()]
        path = str(tmp / 'rows.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        out = subprocess.check_output([exe, '--fixed', path], env=env).decode().splitlines()
        assert len(out) == len(lines)
        bad = [(l, o) for l, o in zip(lines, out) if o.startswith('rejected:')]
        assert not bad, bad[:3]
        return [dict(t.split('=') for t in o.split()) for o in out]
    return run


def _variant(row, d):
    return tuple(int(d[k]) for k in (fv.C24_FIELDS if row.kernel == 'c24' else fv.RB24_FIELDS))


def test_rows_are_the_two_lists(dump):
    listed = dump()
    assert len(listed) == 66 == len(fv.ROWS) and [('COUT' in d) for d in listed] == [True] * 42 + [False] * 24
    assert [r.kernel for r in fv.ROWS] == ['c24'] * 42 + ['rb24'] * 24
    assert [_variant(r, d) for r, d in zip(fv.ROWS, listed)] == [r.variant for r in fv.ROWS], 'row i is entry i of the lists'
    assert [int(d['key']) for d in listed] == [fv.key(r) for r in fv.ROWS], 'c24_key / rb24_key are the header functions'
    assert len(set((r.kernel, r.variant) for r in fv.ROWS)) == 66
    assert [r.knob for r in fv.ROWS].count('') == 65 and fv.ROWS[22].knob == 'W8' and set(r.knob for r in fv.ROWS) == set(fv.KNOBS)
    for r in fv.ROWS:
        if r.kernel == 'rb24':
            assert r.setters['waves'] in (4, 8, 16) and r.setters['store'] in (0, 1)
            assert r.variant[2] == r.setters['probe'] and r.variant[4] == (r.setters['store'] if r.variant[1] != 4 and not r.variant[5] and not r.variant[2] else 0)
        assert bool(r.batch) == bool(r.mm) and r.batch in (0, fv.B)
    # at least one three-map block per weight format and tile height
    assert set((r.wf, fv.tile_h(r)) for r in fv.ROWS if r.entry == 'rb24' and r.batch == fv.B) == {(0, 8), (0, 16), (1, 8), (1, 16)}


def test_every_run_is_planned_as_its_row(dump):
    """Key, LDS bytes and tile count of every run's plan, with the row's arguments, cus = 8, its knob and its setters."""
    runs = [(i, r, run) for i, r in enumerate(fv.ROWS) for run in fv.runs_of(r)]
    plans = dump([fv.dump_line(r, fv.shape(r, run)) for _, r, run in runs])
    wrong = []
    for (i, r, run), p in zip(runs, plans):
        hw = fv.shape(r, run)
        if _variant(r, p) != r.variant or int(p['lds']) != r.lds or int(p['n_tiles']) != fv.n_tiles(r, hw) or int(p.get('nz', 1)) != fv.nz(r):
            wrong.append('row %d %s %s: %s' % (i, run, hw, p))
    assert not wrong, '\n'.join(wrong)
    assert len(set((r.kernel, _variant(r, p)) for (_, r, _), p in zip(runs, plans))) == 66          # 66 of 66 variants planned


LIBRARY_QUERY = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from refvsr_amd import hip
h = hip.lib()
out = []
for a in json.loads(sys.stdin.read()):
    key, n, lds = ctypes.c_longlong(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    hip.check(h.refvsr_conv24_variant(*a, ctypes.byref(key), ctypes.byref(n), ctypes.byref(lds)), 'conv24_variant')
    out.append([key.value, n.value, lds.value])
print(json.dumps(out))
"""


@pytest.mark.parametrize('knob', list(fv.KNOBS))
def test_library_plans_each_conv_row_under_its_knob_set(knob):
    """The library itself, not the dump program: refvsr_conv24_variant is host only, so a fresh process with the knob in its environment
    -- the way the GPU test starts its child -- answers here, without a device, with each row's key, tile count and LDS bytes."""
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    runs = [(r, fv.shape(r, run)) for r in fv.ROWS if r.kernel == 'c24' and r.knob == knob for run in fv.runs_of(r)]
    assert runs
    env = {k: v for k, v in os.environ.items() if not k.startswith('REFVSR_CONV')}
    env.update(fv.KNOBS[knob])
    out = subprocess.run([sys.executable, '-c', LIBRARY_QUERY, ROOT], input=json.dumps([fv.query_args(r, hw) for r, hw in runs]).encode(), env=env,
                         stdout=subprocess.PIPE, check=True).stdout
    assert json.loads(out.decode()) == [[fv.key(r), fv.n_tiles(r, hw), r.lds] for r, hw in runs]


def test_library_plans_each_block_row_under_its_setters():
    """refvsr_resblock24_variant under the setters of each row (this process; restored): key, tile count, LDS bytes.  The probe rows are
    planned with a buffer SET -- the address is never used here: no launch."""
    import ctypes
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = hip.lib()
    buf = (ctypes.c_char * 64)()
    stream = ctypes.c_void_p(0x1000)                        # a stream no budget is registered for ...
    hip.check(h.refvsr_stream_set_cu_budget(stream, fv.WALK_CUS), 'stream_set_cu_budget')      # ... until now
    try:
        for i, r in enumerate(fv.ROWS):
            if r.kernel != 'rb24':
                continue
            hip.check(h.refvsr_set_resblock24_waves(r.setters['waves']), 'waves')
            hip.check(h.refvsr_set_resblock24_store(r.setters['store']), 'store')
            h.refvsr_set_probe(ctypes.cast(buf, ctypes.c_void_p) if r.setters['probe'] else None, 0)
            for run in fv.runs_of(r):
                hw = fv.shape(r, run)
                key, n, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
                hip.check(h.refvsr_resblock24_variant(*fv.query_args(r, hw), stream, ctypes.byref(key), ctypes.byref(n), ctypes.byref(lds)), 'resblock24_variant')
                assert (key.value, n.value, lds.value) == (fv.key(r), fv.n_tiles(r, hw), r.lds), (i, run)
    finally:
        h.refvsr_set_probe(None, 0)
        h.refvsr_set_resblock24_waves(0)
        h.refvsr_set_resblock24_store(1)
        h.refvsr_stream_set_cu_budget(stream, 0)


def test_shapes_of_the_runs():
    for i, r in enumerate(fv.ROWS):
        th = fv.tile_h(r)
        assert fv.runs_of(r)[:2] == ('small', 'walk')
        h, w = fv.small_shape(r)
        assert (h, w) == ((33, 70) if th == 16 else (19, 45)) and (h * r.up) % th and (w * r.up) % 32 and h * r.up > th and w * r.up > 32, 'partial tiles on both axes'
        h, w = fv.walk_shape(r)
        n, bound = fv.n_tiles(r, (h, w)), fv.walk_bound(r)
        assert bound == max(8, (8 * (160 * 1024 // r.lds) // fv.nz(r)) & ~7)
        assert n >= 2 * bound + 1, 'row %d: %d tiles on at most %d workgroups' % (i, n, bound)
        assert (h * r.up) % th and (w * r.up) % 32 and h * r.up <= 120 and w * r.up <= 480
    assert fv.walk_shape(fv.ROWS[40]) == (75, 301)                       # the 24-channel head: 97 tiles needed, 10 x 10
    # the based runs of the four head rows: multiples of both factors, partial tiles on both axes, the zero-base runs' tile counts
    heads = [r for r in fv.ROWS if fv.is_head(r)]
    assert [fv.ROWS.index(r) for r in heads] == [40, 41, 64, 65] and fv.BASED_RUNS == ('small_x4', 'small_x2', 'walk_x4', 'walk_x2', 'tiny_x4', 'tiny_x2')
    for r in fv.ROWS:
        based = [run for run in fv.runs_of(r) if fv.factor(run)]
        assert based == ([k + '_x%d' % s for k in fv.runs_of(r) if not fv.factor(k) for s in (4, 2)] if fv.is_head(r) else [])
        th = fv.tile_h(r)
        for run in based:
            h, w = fv.shape(r, run)
            assert fv.factor(run) in (4, 2) and h % fv.factor(run) == 0 and w % fv.factor(run) == 0
            if fv.kind(run) == 'tiny':
                assert h < 8 and w < 32 and (h, w) == {4: (4, 4), 2: (6, 8)}[fv.factor(run)]
                continue
            assert h % 4 == 0 and w % 4 == 0 and h % th and w % 32 and h > th and w > 32, 'both factors divide, partial tiles on both axes'
            zero = fv.shape(r, fv.kind(run))
            assert fv.n_tiles(r, (h, w)) == fv.n_tiles(r, zero) and (h, w) == (zero[0] + 1, zero[1] - 1) if fv.kind(run) == 'walk' else (h, w) == ((36, 76) if th == 16 else (20, 44))
    assert fv.shape(fv.ROWS[40], 'walk_x4') == (76, 300) and max(fv.shape(r, run)[0] * fv.shape(r, run)[1] for r in heads for run in fv.runs_of(r)) == 76 * 300
    # Multi-map rows: rank r of g workgroups walks tiles [r n / g, (r + 1) n / g) (rv_tile_range), map b starts at tile b n / 3: with
    # a grid that 3 divides the two coincide, otherwise one workgroup walks from one map into the next.  The grid is the cap when
    # the LDS bound is the occupancy; for every entry point at least one row has a bound that 3 does not divide
    crossing = set()
    for r in fv.ROWS:
        if r.batch:
            n, g = fv.n_tiles(r, fv.walk_shape(r)), fv.walk_bound(r)
            if any(rk * n // g < b * n // 3 < (rk + 1) * n // g for rk in range(g) for b in (1, 2)):
                crossing.add(r.entry)
    assert crossing == {'conv24', 'shuffle2', 'conf_alpha', 'rb24'}
    tiny = [r for r in fv.ROWS if r.tiny]
    fam = lambda r: (r.entry, r.up, bool(r.mm or r.batch), r.knob)
    assert {('conv24', 1, True, ''), ('shuffle2', 1, True, ''), ('conf_alpha', 1, True, ''), ('conf_alpha', 2, False, ''), ('conf_alpha', 2, True, ''),
            ('conv48', 1, False, 'W8'), ('rb24', 1, False, ''), ('rb24', 1, True, ''), ('hr_last', 1, False, '')} <= set(fam(r) for r in tiny)
    blocks = set(r.variant for r in tiny if r.entry == 'rb24')
    assert any(v[1] == 4 for v in blocks) and any(v[1] == 16 and v[4] == 1 for v in blocks) and any(v[1] == 8 and v[4] == 0 and not v[2] for v in blocks)
    assert any(v[2] for v in blocks) and any(r.variant[1] == 16 for r in tiny if r.entry == 'hr_last')


@pytest.mark.parametrize('i', range(len(fv.ROWS)), ids=IDS)
def test_cases_are_exact_and_strong(i):
    r = fv.ROWS[i]
    for run in fv.runs_of(r):
        for form in fv.forms(r):
            cases = fv.get_cases(i, run, form)
            assert len(cases) == fv.maps(r)
            for b, c in enumerate(cases):
                print('%-100s %s' % (c.name, c.line()))
                c.assert_strong()
                assert (c.primary == 'hi') == bool(r.wf) and (c.lo0 is None) == (form != 'S')
                shape = c.want['out'].shape
                hw = fv.shape(r, run)
                assert tuple(shape[1:]) == (hw[0] * r.up * (2 if r.entry == 'shuffle2' else 1), hw[1] * r.up * (2 if r.entry == 'shuffle2' else 1))
                if b:
                    for k in fv.WEIGHTS:
                        if k in c.p:
                            assert c.p[k] is cases[0].p[k], 'the maps of a launch share the weights'
                    assert not torch.equal(c.want['out'], cases[0].want['out'])
                if fv.factor(run):
                    assert c.p['s'] == fv.factor(run) and tuple(c.p['base'].shape) == (3, hw[0] // c.p['s'], hw[1] // c.p['s'])
                    cl, one = ec.head_classes(c), c.p['base'].shape[1] * c.p['base'].shape[2] == 1     # (head_classes proves the base exact)
                    assert min(cl['samples']) >= 1 and min(cl['outputs']) >= 1 and (one or cl['inside_clamped'] >= CLASS_MIN), cl
                    assert min(ec.head_borders(c).values()) >= 1, 'a border without a live output'
                    assert ec.base_control(c, 'plane') >= 1 and (one or all(ec.base_control(c, k) >= 1 for k in ('a', 'reflect', 'noclamp', 'step')))
                else:
                    assert 'base' not in c.p
                if fv.kind(run) == 'small' and c.primary != 'hi':
                    assert (c.evaluate('f32')[0]['out'].double() == c.want['out']).all(), 'float32 arithmetic is not exact on this case'
                if r.up == 2:
                    z, o, m = ec.conf_up2_classes(c.p)
                    if form == 'K':
                        assert m == 0 and z >= CLASS_MIN and o >= CLASS_MIN, 'K: every sample saturates'
                    else:
                        assert min(z, o, m) >= CLASS_MIN, 'S: samples clamped at 0, at 1 and strictly between (%d, %d, %d)' % (z, o, m)


# ---- wrong models: each must FAIL the case that was built for it ------------------------------------------------------------------------
def _fails(c, got, fp16=True):
    return not ec.matches(got, c.want['out'], c, fp16, True)[0]


def _row(pred):
    return next(i for i, r in enumerate(fv.ROWS) if pred(r))


@pytest.mark.parametrize('entry', ['conv24', 'shuffle2', 'conf_alpha', 'rb24'])
def test_wrong_model_map_b_read_as_map_0(entry):
    """A multi-map kernel that takes map 0's operands for every map returns map 0's result B times."""
    i = _row(lambda r: r.entry == entry and r.batch)
    for run in ('small', 'walk'):
        cases = fv.get_cases(i, run)
        assert all(_fails(c, cases[0].want['out']) for c in cases[1:])
    if entry == 'conv24':                                   # ... or only the residual of map 0: the table of one operand
        i = _row(lambda r: r.entry == entry and r.batch and fv.EPILOGUES[r.epi].get('res'))
        cases = fv.get_cases(i, 'small')
        for c in cases[1:]:
            p = dict(c.p, res=cases[0].p['res'])
            assert _fails(c, ec.ref_conv(ec.Arith('f64'), p)[0]['out'])


def test_wrong_model_staging_tap_moved_by_one_pixel():
    """The in-kernel bicubic with the weights of two neighbouring taps exchanged (sampling_cases' mutation 'd'): the S cases see it."""
    for i in [i for i, r in enumerate(fv.ROWS) if r.up == 2]:
        for run in fv.runs_of(fv.ROWS[i]):
            for c in fv.get_cases(i, run, 'S'):
                got = ec.ref_conf_alpha(ec.Arith('hi' if c.primary == 'hi' else 'f64'), dict(c.p, mut='d'))[0]['out']
                assert _fails(c, got), c.name


def test_wrong_model_lo_fragment_of_channels_16_to_23_dropped():
    """COUT = 24 keeps the lo halves of output channels 16-23 in the shared third fragment: a kernel that never adds it."""
    for i in [i for i, r in enumerate(fv.ROWS) if r.kernel == 'c24' and r.variant[0] == 24 and r.wf == 0 and r.up == 1]:
        c = fv.get_cases(i, 'small')[0]
        p = dict(c.p)
        w = p['w'].clone()
        w[16:24] = w[16:24].float().half().double()
        p['w'] = w
        assert _fails(c, ec.REFS[c.kind](ec.Arith('f64'), p)[0]['out']), c.name
    i = _row(lambda r: r.entry == 'rb24' and r.wf == 0 and not r.variant[2])
    c = fv.get_cases(i, 'small')[0]
    blocks = []
    for blk in c.p['blocks']:
        blk = [t.clone() for t in blk]
        for k in (0, 2):
            blk[k][16:24] = blk[k][16:24].float().half().double()
        blocks.append(tuple(blk))
    assert _fails(c, ec.ref_blocks(ec.Arith('f64'), dict(c.p, blocks=blocks))[0]['out'])


def test_wrong_model_last_tile_row_skipped():
    """A walk that ends one tile row early leaves the rows of the last tile row unwritten (here: zero)."""
    for i, r in enumerate(fv.ROWS):
        for c in fv.get_cases(i, 'walk', fv.forms(r)[0]):
            got = c.want['out'].clone()
            th = fv.tile_h(r) * (2 if r.entry == 'shuffle2' else 1)
            got[:, (got.shape[1] - 1) // th * th:] = 0
            assert _fails(c, got, fv.is_fp16(r)), c.name
