"""The variant matrix of resblock48_kernel and resblock_lean_kernel (tests/block_variant_cases.py), proven on the CPU: the rows cover
the two lists of the sources, entry by entry, by the keys the library's own host-only queries give; no channel count reaches a lean
instantiation outside its list; every run is planned as its row, with the row's LDS bytes and the tile count its walk rests on; on
every grid a walk run can get, every workgroup takes two tiles or more and some three, a tile that is second or later in its range is
interior and another an edge tile, and in the three-map rows a workgroup's range spans two maps; every case is exact and strong; and
the wrong kernels a walk can produce -- a weight set not swapped, a parked tile that never arrived, an intermediate map not zeroed --
each fail the case built for them, also when only the tiles after a workgroup's first are wrong.  tests/test_gpu_block_variants.py
then runs each row and asks the library which variant and grid it planned."""
import ctypes
import os
import re

import pytest
import torch

import block_variant_cases as bv
import exact_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ['%02d' % i for i in range(len(bv.ROWS))]


@pytest.fixture(scope='module')
def lib():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def _listed(name, source):
    """The X(...) entries of the variant list `name` in a kernel source, as tuples of ints."""
    src = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', source)).read()
    body = re.search(r'#define %s\(X\)((?:.*\\\n)*.*)\n' % name, src).group(1)
    val = {'true': 1, 'false': 0}
    return [tuple(val[t] if t in val else int(t) for t in re.split(r'\s*,\s*', e.strip())) for e in re.findall(r'X\(([^)]*)\)', body)]


def lean_query(h, c, hw, stream=None):
    key, n, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert h.refvsr_resblock_lean_variant(c, hw[0], hw[1], stream, ctypes.byref(key), ctypes.byref(n), None, ctypes.byref(lds)) == 0, h.refvsr_last_error()
    return key.value, n.value, lds.value


def test_rows_are_the_two_lists():
    r48, rl = _listed('R48_VARIANTS', 'resblock48.hip'), _listed('RL_VARIANTS', 'resblock_lean.hip')
    assert r48 == [(0, 0), (1, 0), (1, 1)] and len(rl) == 6 == len(set(rl))
    assert [r.variant for r in bv.ROWS[:3]] == r48 and [r.variant for r in bv.ROWS[6:12]] == rl, 'the first rows of a family are its list, in order'
    assert set(r.variant for r in bv.ROWS if r.kernel == 'rb48') == set(r48) and set(r.variant for r in bv.ROWS if r.kernel == 'lean') == set(rl)
    assert [r.kernel for r in bv.ROWS] == ['rb48'] * 6 + ['lean'] * 8
    # both plain 48-channel kernels in the three-map form; one n = 3 chain per family; CASE_A and CASE_B on half of the one-block rows each
    assert sorted(r.variant for r in bv.ROWS if r.batch == bv.B) == [(0, 0), (1, 0)] and all(r.batch in (0, bv.B) for r in bv.ROWS)
    assert [(r.kernel, r.entry) for r in bv.ROWS if len(r.plan) == 3] == [('rb48', 'rb48'), ('lean', 'chain')]
    assert all(r.plan == ec._placement(1, 1) for r in bv.ROWS if len(r.plan) == 3)
    for kern in ('rb48', 'lean'):
        plans = [r.plan for r in bv.ROWS if r.kernel == kern and len(r.plan) == 1]
        assert abs(plans.count(ec.CASE_A) - plans.count(ec.CASE_B)) <= 1 and set(map(str, plans)) == {str(ec.CASE_A), str(ec.CASE_B)}
    assert all(r.mag_exp == -4 for r in bv.ROWS if r.kernel == 'rb48')
    # lean: c in {8 | 16, 24, 32} x waves in {4, 8}; c = 8 and c = 16 both on 8 waves; both slope pairs on each wave count
    lean = [r for r in bv.ROWS if r.kernel == 'lean']
    assert all(r.waves == r.variant[2] and r.waves in (4, 8) for r in lean)
    assert {(r.c, r.waves) for r in lean} >= {(8, 8), (16, 8), (24, 8), (32, 8), (8, 4), (24, 4), (32, 4)}
    for waves in (4, 8):
        assert {(r.act, r.post) for r in lean if r.waves == waves and r.entry == 'lean'} == {(0.25, 1.0), (0.0, 0.5)}
    # resblock48: the slope picks the kernel; the probe row has a buffer set
    assert all(r.act == (0.0 if r.variant[0] else 0.25) and r.probe == r.variant[1] for r in bv.ROWS if r.kernel == 'rb48')
    assert sorted(r.kernel for r in bv.ROWS if r.tiny) == ['lean', 'rb48'], '7 x 5 once per kernel family'


def test_no_channel_count_reaches_a_lean_kernel_outside_the_list(lib):
    """Every c that refvsr_resblock_lean_fits, under both wave counts, is planned as one of the six listed instantiations, and every
    one of the six is reached: MT = 1 (c <= 16: two channel groups, 72 chunk slots) is never WIDE -- the two entries the list had for
    it could not be launched."""
    listed = set(v[0] | v[1] << 2 | v[2] << 3 for v in _listed('RL_VARIANTS', 'resblock_lean.hip'))
    fits = [c for c in range(-8, 513) if lib.refvsr_resblock_lean_fits(c)]
    assert fits == [8, 16, 24, 32]
    seen = set()
    try:
        for waves in (4, 8):
            assert lib.refvsr_set_resblock_waves(waves) == 0
            for c in fits:
                k = lean_query(lib, c, bv.SMALL)[0]
                mt, wide, nwv = k & 3, k >> 2 & 1, k >> 3
                assert (mt, nwv) == ((c + 15) // 16, waves) and wide == int(36 * (c // 8) > 128) and not (mt == 1 and wide)
                seen.add(k)
    finally:
        lib.refvsr_set_resblock_waves(8)
    assert seen == listed and len(listed) == 6


def test_library_plans_each_run_as_its_row(lib):
    """refvsr_resblock48_variant / refvsr_resblock_lean_variant with a null grid pointer (host only) under the setters of each row
    (restored): key, tile count, LDS bytes.  The probe row is planned with a buffer SET -- never written: nothing is launched."""
    buf = (ctypes.c_char * 64)()
    try:
        for i, r in enumerate(bv.ROWS):
            lib.refvsr_set_probe(ctypes.cast(buf, ctypes.c_void_p) if r.probe else None, 0)
            if r.waves:
                assert lib.refvsr_set_resblock_waves(r.waves) == 0
            for run in bv.runs_of(r):
                hw = bv.shape(r, run)
                if r.kernel == 'rb48':
                    key, n, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
                    assert lib.refvsr_resblock48_variant(r.act, bv.maps(r), hw[0], hw[1], None, ctypes.byref(key), ctypes.byref(n), None, ctypes.byref(lds)) == 0
                    got = (key.value, n.value, lds.value)
                else:
                    got = lean_query(lib, r.c, hw)
                assert got == (bv.key(r), bv.n_tiles(r, hw), r.lds), (i, run, got)
    finally:
        lib.refvsr_set_probe(None, 0)
        lib.refvsr_set_resblock_waves(8)


def test_shapes_of_the_runs():
    ty, tx = bv.tiles_xy(bv.SMALL)
    assert (ty, tx) == (6, 3) and bv.SMALL[0] % bv.TH and bv.SMALL[1] % bv.TW
    assert sum(bv.is_interior(bv.SMALL, y * bv.TH, x * bv.TW) for y in range(ty) for x in range(tx)) == 4
    assert bv.TINY == (7, 5)
    for i, r in enumerate(bv.ROWS):
        assert bv.runs_of(r)[:2] == ('small', 'walk') and bv.shape(r, 'small') == bv.SMALL
        h, w = bv.walk_shape(r)
        if r.kernel == 'rb48':
            assert (h, w) == bv.SMALL and bv.walk_bound(r) == 8 and bv.grids(r) == [8]
        else:
            bound = bv.walk_bound(r)
            assert bound == max(8, (8 * (160 * 1024 // r.lds)) & ~7) and bv.grids(r)[-1] == bound
            assert (h - 3) % 8 == 0 and (w - 13) % 32 == 0 and h >= 27 and w >= 109 and h <= 120 and w <= 480
            assert bv.n_tiles(r, (h, w)) >= 2 * bound + 1, 'row %d: %d tiles on at most %d workgroups' % (i, bv.n_tiles(r, (h, w)), bound)
    assert [bv.walk_shape(r) for r in bv.ROWS[6:10]] == [(51, 205), (43, 173), (27, 141), (83, 365)]


@pytest.mark.parametrize('i', range(len(bv.ROWS)), ids=IDS)
def test_every_workgroup_of_a_walk_run_walks(i):
    """rv_tile_range restated (bv.tile_ranges), for every grid the launcher can choose on a stream with a CU budget of 8."""
    r = bv.ROWS[i]
    hw = bv.walk_shape(r)
    n = bv.n_tiles(r, hw)
    tpm = n // bv.maps(r)
    for g in bv.grids(r):
        rng = bv.tile_ranges(n, g)
        assert sorted(t for lo, hi in rng for t in range(lo, hi)) == list(range(n)), 'the ranges partition the tiles'
        sizes = [hi - lo for lo, hi in rng]
        assert min(sizes) >= 2 and max(sizes) >= 3, (g, sizes)
        later = [bv.tile_origin(hw, t) for t in bv.later_tiles(n, g)]
        kinds = [bv.is_interior(hw, y, x) for _, y, x in later]
        assert any(kinds) and not all(kinds), 'grid %d: a later tile on the fast path and one on the masked path' % g
        if r.batch:
            assert sum(lo // tpm != (hi - 1) // tpm for lo, hi in rng) >= 1, 'a range that spans two maps'
    if r.kernel == 'rb48':
        sizes = [hi - lo for lo, hi in bv.tile_ranges(n, 8)]
        if r.batch:
            assert sorted(set(sizes)) == [6, 7] and sum(lo // tpm != (hi - 1) // tpm for lo, hi in bv.tile_ranges(n, 8)) == 2
        else:
            assert sorted(set(sizes)) == [2, 3]


@pytest.mark.parametrize('i', range(len(bv.ROWS)), ids=IDS)
def test_cases_are_exact_and_strong(i):
    r = bv.ROWS[i]
    for run in bv.runs_of(r):
        cases = bv.get_cases(i, run)
        hw = bv.shape(r, run)
        assert len(cases) == bv.maps(r)
        print('%-72s %s' % (cases[0].name, bv.control_line(cases, r, run)))
        assert bv.weak(cases, r, run) is None
        for b, c in enumerate(cases):
            print('%-72s %s' % (c.name, c.line()))
            c.assert_strong()
            assert c.bound < ec.LIMIT and c.primary == 'f64' and c.lo0 is None
            assert tuple(c.want['out'].shape) == (r.c, hw[0], hw[1]) and len(c.p['blocks']) == len(r.plan)
            assert c.p['act'] == r.act and c.p['post'] == r.post
            if b:
                assert c.p['blocks'] is cases[0].p['blocks'], 'the maps of a launch share the weights'
                assert not torch.equal(c.p['x'], cases[0].p['x']) and not torch.equal(c.want['out'], cases[0].want['out'])
            if run != 'walk' or r.kernel == 'rb48':
                assert (c.evaluate('f32')[0]['out'].double() == c.want['out']).all(), 'float32 arithmetic is not exact on this case'


# ---- wrong models: each must FAIL the case that was built for it ------------------------------------------------------------------------
def _fails(c, got):
    return not ec.matches(got, c.want['out'], c, True, True)[0]


@pytest.mark.parametrize('i', range(len(bv.ROWS)), ids=IDS)
def test_wrong_kernels_fail_on_the_later_tiles_alone(i):
    """A workgroup's first tile is right in each of the walk's defects (W1 and the first window arrive before the loop): the output is
    the reference on the first tiles and the wrong kernel's on the later ones.  Every launch must see that, at every grid."""
    r = bv.ROWS[i]
    cases = bv.get_cases(i, 'walk')
    hw = bv.shape(r, 'walk')
    n = bv.n_tiles(r, hw)
    for g in bv.grids(r)[-1:] + bv.grids(r)[:1]:
        later = bv.later_tiles(n, g)
        mask = bv.tile_mask(hw, len(cases), later)
        wk = bv.wrong_kernels(cases, later)
        assert torch.equal(torch.stack(wk.pop('plain')), torch.stack([c.want['out'] for c in cases]))
        assert sorted(wk) == ['a', 'b', 'c', 'd']
        for k, outs in wk.items():
            got = [torch.where(mask[b][None], o, c.want['out']) for b, (o, c) in enumerate(zip(outs, cases))]
            assert any(_fails(c, o) for c, o in zip(cases, got)), (k, g)
            if k in 'abc':
                assert all(_fails(c, o) for c, o in zip(cases, got)), (k, g)


def test_wrong_model_map_b_read_as_map_0():
    """A multi-map kernel that takes map 0's input for every map returns map 0's result B times."""
    rows = [i for i, r in enumerate(bv.ROWS) if r.batch]
    assert len(rows) == 2
    for i in rows:
        for run in ('small', 'walk'):
            cases = bv.get_cases(i, run)
            assert all(_fails(c, cases[0].want['out']) for c in cases[1:])


def test_wrong_model_last_tile_row_skipped():
    """A walk that ends one tile row early leaves the rows of the last tile row unwritten (here: zero)."""
    for i, r in enumerate(bv.ROWS):
        for c in bv.get_cases(i, 'walk'):
            got = c.want['out'].clone()
            got[:, (got.shape[1] - 1) // bv.TH * bv.TH:] = 0
            assert _fails(c, got), c.name
