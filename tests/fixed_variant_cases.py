"""Exact cases for EVERY instantiation of conv24_kernel and resblock24_kernel: the table behind tests/test_fixed_variant_cases.py
(CPU) and tests/test_gpu_fixed_variants.py (the kernels), the counterpart of tests/conv_variant_cases.py for the fixed-channel kernels.

refvsr_amd/csrc/fixed_plan.h lists 42 conv24_kernel and 24 resblock24_kernel instantiations (RV_C24_VARIANTS, RV_RB24_VARIANTS).  Row i
of ROWS is entry i of the two lists, one after the other: the template arguments, the entry point and arguments that reach the entry
(op, channels, `_f16w` twin, `_batch` form), for resblock24 the state of its setters (waves ALWAYS forced to 4 | 8 | 16, so that no row
depends on the CU count of the machine; store; a probe buffer), the knob set (one row: REFVSR_CONV48_WAVES=8, read once per process:
that row runs in a child, tests/fixed_variant_child.py) and the dynamic LDS bytes of the plan.

Each row has a SMALL run -- 19 x 45, or 33 x 70 for the 16-row tiles: partial tiles on both axes -- and a WALK run: the launch goes to
a side stream whose CU budget is 8, so the launcher caps the grid at max(8, (8 x occupancy / nz) & ~7) workgroups (rv_launch_cap);
occupancy <= floor(160 KiB / lds), and walk_shape() picks the smallest h = TH a + 3, w = 32 b + 13 whose tile count (maps included)
is at least twice that bound plus one: every workgroup walks at least two tiles and some three -- has_next, the next-tile fetch under
the K loop, its barrier, and in the multi-map rows the step from one map to the next inside a workgroup.  Rows marked `tiny` run a
third time at 7 x 5, below one tile: one row of every family that had no float64 comparison before.

The four head rows (refvsr_conv_last at C = 24 | 48, the two HEAD rows of resblock24_kernel) run their small, walk and tiny shapes with
a ZERO base frame of the output's own size (base_step = 1) and, besides, BASED runs with an exact non-zero base at x4 and at x2
(exact_cases.head_base; `small_x4`, `walk_x2`, ...): shapes that are multiples of the factor and still leave partial tiles on both axes --
small 20 x 44 | 36 x 76, walk h = TH a + 4, w = 32 b + 12 under the same tile-count rule, tiny 4 x 4 (x4: a 1 x 1 base) | 6 x 8 (x2).

Multi-map rows carry B = 3 maps with separately built data (weights shared, as in the launch); every map has its own case and its own
reference.  Cases come from exact_cases' builders; a case that is not strong at its first seed moves to the next one (the choice is
made on the reference alone).  up = 2 rows have two cases per run, K and S (exact_cases._conf_case).
"""
import collections

import exact_cases as ec

C24_FIELDS = ('COUT', 'NCG0', 'NCG1', 'NWV', 'TH', 'WPS', 'SHUF', 'CONF', 'HALF', 'MM', 'WF')
RB24_FIELDS = ('RELU', 'NWV', 'PROBE', 'TH', 'STORE', 'HEAD', 'WF')
KNOBS = collections.OrderedDict((('', {}), ('W8', {'REFVSR_CONV48_WAVES': '8'})))
OPS = dict(conv24=0, conv32=1, conv48=2, shuffle2=3, conf_alpha=4, conv_last=5)          # REFVSR_C24_* of include/refvsr_hip.h
B = 3
WALK_CUS = 8
LDS_BYTES = 160 * 1024
SMALL8, SMALL16, TINY = ec.L19, (33, 70), ec.S7

# epilogues of the conv rows (fp16 HWC stores, slopes in [0, 1])
EPILOGUES = {
    'plain': dict(),
    'relu': dict(act=0.0),
    'lrelu': dict(act=0.25),
    'res_relu': dict(res=True, post=0.0),
    'lrelu_mul': dict(act=0.25, mul=True),
    'res_post': dict(res=True, post=0.25),
    'all': dict(act=0.5, mul=True, res=True),
}

Row = collections.namedtuple('Row', 'kernel variant entry cins cout up wf mm batch setters knob lds epi tiny')


def c24_key(v):
    """c24_variant_key of fixed_plan.h."""
    COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF = v
    return COUT | NCG0 << 6 | NCG1 << 10 | NWV << 14 | TH << 19 | WPS << 24 | SHUF << 27 | CONF << 33 | HALF << 35 | MM << 36 | WF << 37


def rb24_key(v):
    """rb24_variant_key of fixed_plan.h."""
    RELU, NWV, PROBE, TH, STORE, HEAD, WF = v
    return RELU | NWV << 1 | PROBE << 6 | TH << 7 | STORE << 12 | HEAD << 13 | WF << 14


def key(row):
    return c24_key(row.variant) if row.kernel == 'c24' else rb24_key(row.variant)


def tile_h(row):
    return row.variant[4] if row.kernel == 'c24' else row.variant[3]


def nz(row):
    """gridDim.y of the launch (c24_nz of fixed_plan.h): the channel halves and the row groups of the pixel shuffle."""
    if row.kernel != 'c24':
        return 1
    shuf, half = row.variant[6], row.variant[8]
    return 2 if half else {0: 1, 24: 2, 48: 4}[shuf]


def maps(row):
    return row.batch if row.batch else 1


def C(variant, entry, cins=(), cout=24, up=1, knob='', lds=0, epi='plain', tiny=False):
    mm, wf = variant[9], variant[10]
    return Row('c24', tuple(variant), entry, tuple(cins), cout, up, wf, mm, B if mm else 0, {}, knob, lds, epi, tiny)


def R(variant, batch=0, lds=0, tiny=False):
    relu, nwv, probe, th, store, head, wf = variant
    return Row('rb24', tuple(variant), 'hr_last' if head else 'rb24', (24,), 3 if head else 24, 1, wf, int(bool(batch)), batch,
               dict(waves=nwv, store=store if nwv != 4 and not head and not probe else 1, probe=probe), '', lds, 'relu' if relu else 'lrelu', tiny)


def _c24_rows24(mm, wf, epis, tiny):
    lds = {0: (37952, 31808, 54976, 81216), 1: (30784, 26688, 45760, 66880)}[wf]
    return [C((24, 3, 0, 8, 8, 4, 0, 0, 0, mm, wf), 'conv24', [24], lds=lds[0], epi=epis[0], tiny=tiny),
            C((24, 2, 0, 8, 8, 4, 0, 0, 0, mm, wf), 'conv24', [16], lds=lds[1], epi=epis[1]),
            C((24, 1, 3, 8, 8, 4, 0, 0, 0, mm, wf), 'conv24', [3, 24], lds=lds[2], epi=epis[2]),
            C((24, 3, 3, 8, 8, 4, 0, 0, 0, mm, wf), 'conv24', [24, 24], lds=lds[3], epi=epis[3])]


# in the order of RV_C24_VARIANTS, then of RV_RB24_VARIANTS.  lds: what the plan states (asserted against tools/conv_plan_dump and,
# on the GPU, against the library's query); the tile counts follow from the shapes
ROWS = (
    _c24_rows24(0, 0, ('lrelu', 'res_post', 'all', 'res_relu'), False) +
    _c24_rows24(0, 1, ('res_relu', 'lrelu', 'all', 'lrelu_mul'), False) +
    _c24_rows24(1, 0, ('all', 'lrelu_mul', 'res_post', 'relu'), True) +
    _c24_rows24(1, 1, ('lrelu_mul', 'all', 'res_relu', 'res_post'), True) + [
        C((32, 4, 0, 8, 8, 4, 0, 0, 0, 0, 0), 'conv32', [32], 32, lds=64192, epi='lrelu'),
        C((32, 1, 0, 8, 8, 4, 0, 0, 0, 0, 0), 'conv32', [3], 32, lds=17856, epi='res_post'),
        C((32, 4, 0, 8, 8, 4, 0, 0, 0, 0, 1), 'conv32', [32], 32, lds=45760, epi='all'),
        C((32, 1, 0, 8, 8, 4, 0, 0, 0, 0, 1), 'conv32', [3], 32, lds=11712, epi='lrelu_mul'),
        C((24, 6, 6, 16, 8, 4, 0, 0, 1, 0, 0), 'conv48', [48, 48], 48, lds=153792, epi='lrelu'),
        C((48, 1, 6, 16, 8, 4, 0, 0, 0, 0, 0), 'conv48', [3, 48], 48, lds=148928, epi='res_relu'),
        C((48, 6, 0, 8, 16, 2, 0, 0, 0, 0, 0), 'conv48', [48], 48, knob='W8', lds=154816, epi='res_relu', tiny=True),
        C((48, 6, 0, 16, 16, 4, 0, 0, 0, 0, 0), 'conv48', [48], 48, lds=154816, epi='lrelu_mul'),
        C((48, 2, 0, 8, 8, 4, 0, 0, 0, 0, 0), 'conv48', [16], 48, lds=47296, epi='res_post'),
        C((48, 3, 0, 8, 8, 4, 24, 0, 0, 0, 0), 'shuffle2', [24], 96, lds=59584, epi='lrelu'),
        C((48, 6, 0, 16, 16, 4, 48, 0, 0, 0, 0), 'shuffle2', [48], 192, lds=154816, epi='plain'),
        C((48, 3, 0, 8, 8, 4, 24, 0, 0, 0, 1), 'shuffle2', [24], 96, lds=38080, epi='relu'),
        C((48, 3, 0, 8, 8, 4, 24, 0, 0, 1, 0), 'shuffle2', [24], 96, lds=59584, epi='lrelu', tiny=True),
        C((48, 3, 0, 8, 8, 4, 24, 0, 0, 1, 1), 'shuffle2', [24], 96, lds=38080, epi='plain'),
        C((24, 2, 0, 8, 8, 4, 0, 1, 0, 0, 0), 'conf_alpha', [16], 24, 1, lds=36480),
        C((24, 2, 0, 8, 8, 4, 0, 2, 0, 0, 0), 'conf_alpha', [16], 24, 2, lds=36480, tiny=True),
        C((48, 2, 0, 8, 8, 4, 0, 1, 0, 0, 0), 'conf_alpha', [16], 48, 1, lds=51968),
        C((48, 2, 0, 8, 8, 4, 0, 2, 0, 0, 0), 'conf_alpha', [16], 48, 2, lds=51968),
        C((24, 2, 0, 8, 8, 4, 0, 1, 0, 0, 1), 'conf_alpha', [16], 24, 1, lds=31360),
        C((24, 2, 0, 8, 8, 4, 0, 2, 0, 0, 1), 'conf_alpha', [16], 24, 2, lds=31360),
        C((24, 2, 0, 8, 8, 4, 0, 1, 0, 1, 0), 'conf_alpha', [16], 24, 1, lds=36480, tiny=True),
        C((24, 2, 0, 8, 8, 4, 0, 2, 0, 1, 0), 'conf_alpha', [16], 24, 2, lds=36480, tiny=True),
        C((24, 2, 0, 8, 8, 4, 0, 1, 0, 1, 1), 'conf_alpha', [16], 24, 1, lds=31360),
        C((24, 2, 0, 8, 8, 4, 0, 2, 0, 1, 1), 'conf_alpha', [16], 24, 2, lds=31360),
        C((3, 3, 0, 8, 8, 4, 0, 0, 0, 0, 0), 'conv_last', [24], 3, lds=23616),
        C((3, 6, 0, 8, 8, 4, 0, 0, 0, 0, 0), 'conv_last', [48], 3, lds=52544),
        R((1, 8, 1, 8, 0, 0, 0), lds=64000, tiny=True),
        R((1, 16, 1, 16, 0, 0, 0), lds=77824)] +
    [r for wf, l8, l16 in ((0, 64000, 77824), (1, 49664, 63488)) for r in (
        R((1, 4, 0, 8, 0, 0, wf), lds=l8, tiny=not wf),
        R((0, 4, 0, 8, 0, 0, wf), B, lds=l8),
        R((1, 16, 0, 16, 1, 0, wf), B, lds=l16, tiny=True),
        R((1, 16, 0, 16, 0, 0, wf), lds=l16),
        R((1, 8, 0, 8, 1, 0, wf), B, lds=l8),
        R((1, 8, 0, 8, 0, 0, wf), lds=l8, tiny=True),
        R((0, 16, 0, 16, 1, 0, wf), lds=l16),
        R((0, 16, 0, 16, 0, 0, wf), lds=l16),
        R((0, 8, 0, 8, 1, 0, wf), lds=l8),
        R((0, 8, 0, 8, 0, 0, wf), lds=l8))] + [
        R((0, 16, 0, 16, 0, 1, 0), lds=77824, tiny=True),
        R((0, 8, 0, 8, 0, 1, 0), lds=64000)])


# ---- what reaches a row: the dump program's line, the library query's arguments -------------------------------------------------------
def pads(row):
    return [ec.pad8(c) for c in row.cins]


def slope(row):
    """act_slope of a resblock24 row's launch (the chain: 0 = ReLU; the head is always leaky)."""
    return 0.0 if row.variant[0] else 0.25


def dump_line(row, hw, cus=WALK_CUS):
    """The row as a --fixed line of tools/conv_plan_dump, knob and setters included (hw: the maps the entry point is given)."""
    t = 'op=%s wf=%d mm=%d batch=%d h=%d w=%d cus=%d' % (row.entry, row.wf, row.mm, maps(row), hw[0], hw[1], cus)
    if row.kernel == 'rb24':
        return t + ' slope=%g waves=%d store=%d probe=%d' % (slope(row), row.setters['waves'], row.setters['store'], row.setters['probe'])
    if row.knob:
        t += ' CONV48_WAVES=8'
    if row.entry == 'conf_alpha':
        return t + ' cout=%d up=%d' % (row.cout, row.up)
    if row.entry in ('shuffle2', 'conv_last'):
        return t + ' c=%d' % row.cins[0]
    p = pads(row)
    return t + ' c0=%d c1=%d' % (p[0], p[1] if len(p) > 1 else 0)


def query_args(row, hw):
    """(op, x0, x1, mm, wf, batch, h, w) of refvsr_conv24_variant | (head, wf, relu, batch, h, w) of refvsr_resblock24_variant."""
    if row.kernel == 'rb24':
        return (int(row.entry == 'hr_last'), row.wf, int(slope(row) == 0.0), maps(row), hw[0], hw[1])
    p = pads(row)
    x0, x1 = (row.cout, row.up) if row.entry == 'conf_alpha' else (p[0], p[1] if len(p) > 1 else 0)
    return (OPS[row.entry], x0, x1, row.mm, row.wf, maps(row), hw[0], hw[1])


# ---- the shapes of the runs -----------------------------------------------------------------------------------------------------------
def walk_bound(row):
    """Upper bound of the grid of a launch on a stream with a CU budget of 8: rv_launch_cap with occupancy <= floor(160 KiB / lds)."""
    return max(8, (WALK_CUS * (LDS_BYTES // row.lds) // nz(row)) & ~7)


def n_tiles(row, hw):
    """Tiles of the launch on maps of hw (up = 2: the conv runs on the doubled grid)."""
    th = tile_h(row)
    h, w = hw[0] * row.up, hw[1] * row.up
    return -(-h // th) * -(-w // 32) * maps(row)


def walk_shape(row, dh=3, dw=13):
    """The smallest h = TH a + dh, w = 32 b + dw (3 and 13; the based runs of the heads: 4 and 12, multiples of both factors) (a, b >= 1; by the longer side in tiles, then by area: as many tile rows as tile
    columns, or one fewer) with n_tiles >= 2 walk_bound + 1.  up = 2: the
    conv's grid is twice the confidence maps, so the MAPS are (TH a + 6) / 2 x (32 b + 14) / 2: partial tiles again."""
    th, need, best = tile_h(row), 2 * walk_bound(row) + 1, None
    for a in range(1, 200):
        for b in range(1, 200):
            if (a + 1) * (b + 1) * maps(row) >= need:
                hw = (th * a + dh, 32 * b + dw) if row.up == 1 else ((th * a + 6) // 2, (32 * b + 14) // 2)
                if best is None or (max(a, b), hw[0] * hw[1]) < best[0]:
                    best = ((max(a, b), hw[0] * hw[1]), hw)
                break
    assert n_tiles(row, best[1]) >= need
    return best[1]


def small_shape(row):
    return SMALL16 if tile_h(row) == 16 else SMALL8


RUNS = ('small', 'walk', 'tiny')
FACTORS = (4, 2)
BASED_RUNS = tuple('%s_x%d' % (run, s) for run in RUNS for s in FACTORS)
BASED_SMALL8, BASED_SMALL16 = (20, 44), (36, 76)
BASED_TINY = {4: (4, 4), 2: (6, 8)}
BASE_VALUES = {4: 'u', 2: 's'}              # exact_cases.BASE_SETS of the based runs


def is_head(row):
    return row.entry in ('conv_last', 'hr_last')


def runs_of(row):
    """The zero-base runs of every row, then the based runs of the head rows."""
    runs = RUNS if row.tiny else RUNS[:2]
    return runs + tuple('%s_x%d' % (run, s) for run in runs for s in FACTORS) if is_head(row) else runs


def kind(run):
    """'small' | 'walk' | 'tiny' of a run, based or not."""
    return run.split('_x')[0]


def factor(run):
    """The base's factor of a based run, None for a zero-base run."""
    return int(run.split('_x')[1]) if '_x' in run else None


def shape(row, run):
    if factor(run) is None:
        return {'small': small_shape, 'walk': walk_shape, 'tiny': lambda r: TINY}[run](row)
    if kind(run) == 'small':
        return BASED_SMALL16 if tile_h(row) == 16 else BASED_SMALL8
    return walk_shape(row, 4, 12) if kind(run) == 'walk' else BASED_TINY[factor(run)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
WEIGHTS = ('w', 'b', 'w0', 'b0', 'blocks', 'w1', 'b1', 'w2', 'b2')       # shared by the maps of a launch; everything else is per map


def row_name(i, row):
    v = '.'.join(str(int(x)) for x in row.variant)
    return 'variant %02d %s %s %s' % (i, row.kernel, v, row.entry) + (' up2' if row.up == 2 else '') + (' f16w' if row.wf else '') + (' B%d' % row.batch if row.batch else '')


def _build(i, row, hw, seed, form, name, base=None):
    wfmt, primary = ('fp16', 'hi') if row.wf else ('hi_lo', 'f64')
    if row.entry in ('conv24', 'conv32', 'conv48', 'shuffle2'):
        c = None
        for g_exp, mag_exp in ((-17, -3), (-17, -4), (-17, -5)):          # the most weight bits (14, 13, 12: a lo part) with which the bound holds
            c = ec._conv_case(name, seed, row.cout, list(row.cins), 3, hw, out='nhwc', shuffle=row.entry == 'shuffle2', g_exp=g_exp, mag_exp=mag_exp,
                              xr=2 if row.cins == (3,) else 1, run=dict(generic=False, wfmt=wfmt), primary=primary, **EPILOGUES[row.epi])
            if c.bound < ec.LIMIT:
                break
        return c
    if row.entry == 'conf_alpha':
        return ec._conf_case(name, seed, row.cout, hw, want_max=row.up == 1, wfmt=wfmt, up=row.up, staging=form == 'S')
    if row.entry == 'conv_last':
        return ec._last_case(name, seed, row.cins[0], hw, base=base)
    if row.entry == 'hr_last':
        return ec._hr_case(name, seed, hw, 'AB'[i % 2], 0.25, base=base, b_count=6 if base and hw == BASED_TINY[4] and i % 2 == 0 else ec.CTL_B_COUNT)
    return ec._blocks_case(name, seed, 'rb24', 24, hw, (ec.CASE_A, ec.CASE_B)[i % 2], slope(row), wfmt=wfmt)


def _strong(c):
    try:
        c.assert_strong()
        return True
    except AssertionError:
        return False


def forms(row):
    """The cases of one run: 'K' and 'S' for the up = 2 rows, one (None) for every other."""
    return ('K', 'S') if row.up == 2 else (None,)


def build_cases(i, run, form=None):
    """[the case of map b] of row i's run (one map for the single-map rows): the first seed of the row's sequence at which map 0 is
    strong, then per further map the first seed at which the map -- its own data, map 0's weights -- is strong."""
    row = ROWS[i]
    hw = shape(row, run)
    base = 9000 + 64 * i + 16 * RUNS.index(kind(run)) + (8 if form == 'S' else 0) + (100000 * factor(run) if factor(run) else 0)
    based = (factor(run), BASE_VALUES[factor(run)]) if factor(run) else None
    name = '%s %s%s %dx%d' % (row_name(i, row), run, ' ' + form if form else '', hw[0], hw[1])
    cases = []
    for b in range(maps(row)):
        for k in range(24):
            c = _build(i, row, hw, base + b + 7919 * k, form, name + (' map %d' % b if row.batch else ''), based)
            if b:
                c.p.update((key_, cases[0].p[key_]) for key_ in WEIGHTS if key_ in c.p)
                for key_ in ('full', 'hi', 'controls'):     # (the builder looked at the bound of its own weights)
                    c.__dict__.pop(key_, None)
            if _strong(c):
                break
        cases.append(c)
    return cases


_CACHE = {}


def get_cases(i, run, form=None):
    if (i, run, form) not in _CACHE:
        _CACHE[(i, run, form)] = build_cases(i, run, form)
    return _CACHE[(i, run, form)]


def is_fp16(row):
    return row.entry not in ('conv_last', 'hr_last')
