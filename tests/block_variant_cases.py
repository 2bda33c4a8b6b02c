"""Exact cases for EVERY instantiation of resblock48_kernel and resblock_lean_kernel, tile walk included: the table behind
tests/test_block_variant_cases.py (CPU) and tests/test_gpu_block_variants.py (the kernels), the counterpart of
tests/fixed_variant_cases.py for the two other fused blocks.

refvsr_amd/csrc/resblock48.hip lists 3 instantiations (R48_VARIANTS: RELU, PROBE), refvsr_amd/csrc/resblock_lean.hip 6 (RL_VARIANTS: MT,
WIDE, NWV).  ROWS has every one of them through the entry points the engine uses: the 48-channel block through refvsr_resblock48_chain
(the probe kernel with a probe buffer set) and, the two plain kernels, through refvsr_resblock48_chain_batch with B = 3 separately
built maps; the lean block through refvsr_resblock_lean for c in {8, 16, 24, 32} x waves in {4, 8} (refvsr_set_resblock_waves, set per
run); one n = 3 chain per family.

Each row has a SMALL run -- 43 x 77 on the current stream: 6 x 3 tiles, partial on both axes, 4 of them interior (the fast path of
resblock48's x_fetch), one tile per workgroup on a part with 18 CUs or more -- and a WALK run on a side stream whose CU budget is 8, so
the launcher caps the grid at max(8, (8 x occupancy) & ~7) workgroups (rv_launch_cap).  resblock48 runs one workgroup per CU: 8
workgroups over the 18 (B = 3: 54) tiles of 43 x 77 again.  The lean block's occupancy is at most floor(160 KiB / lds); walk_shape()
picks the smallest h = 8 a + 3, w = 32 b + 13 (a, b >= 3: interior tiles) whose tile count is at least twice that bound plus one.
Every workgroup then walks two tiles or more and some three: has_next, the weight-set swap back to W1, the park of the prefetched
tile, barriers C and D, and in the B = 3 rows the step from one map to the next inside a workgroup.  Rows marked `tiny` run a third
time at 7 x 5, below one tile.

Cases come from exact_cases._blocks_case.  Besides exact_cases' controls (every lo term / the lo term of one K-block dropped) a case
must see four wrong kernels that a walk can produce, each computed from the reference alone (controls()): W1 used for both convs, W2
used for both, conv1 fed the window of the workgroup's PREVIOUS tile, the intermediate map not zeroed outside the frame.  A case that
is weak at its first seed moves to the next one."""
import collections

import torch
import torch.nn.functional as F

import exact_cases as ec
import fixed_variant_cases as fv

B = fv.B
TH, TW = 8, 32
SMALL, TINY = (43, 77), ec.S7
R48_LDS = 134912
RUNS = fv.RUNS

# kernel 'rb48' | 'lean'; variant (RELU, PROBE) | (MT, WIDE, NWV); entry: 'rb48' (refvsr_resblock48_chain), 'rb48_batch', 'lean'
# (refvsr_resblock_lean), 'chain' (refvsr_resblock_chain); plan: exact_cases' conv kinds per block
Row = collections.namedtuple('Row', 'kernel variant entry c batch plan act post waves probe lds mag_exp tiny')


def R48(relu, probe, plan, batch=0, tiny=False):
    return Row('rb48', (relu, probe), 'rb48_batch' if batch else 'rb48', 48, batch, plan, 0.0 if relu else 0.25, 1.0, 0, probe, R48_LDS, -4, tiny)


def RL(mt, wide, nwv, c, plan, act, post, lds, entry='lean', tiny=False):
    return Row('lean', (mt, wide, nwv), entry, c, 0, plan, act, post, nwv, 0, lds, -2 if c == 8 else -3, tiny)


A, Bc, N3 = ec.CASE_A, ec.CASE_B, ec._placement(1, 1)
# resblock48: in the order of R48_VARIANTS, then the multi-map and n = 3 forms; lean: in the order of RL_VARIANTS, then c = 8 on the
# wave count that already has c = 16, and the n = 3 chain.  lds: what the library's query states (asserted on the CPU and on the GPU)
ROWS = (
    R48(0, 0, A),
    R48(1, 0, Bc, tiny=True),
    R48(1, 1, A),
    R48(0, 0, Bc, batch=B),
    R48(1, 0, A, batch=B),
    R48(1, 0, N3),
    RL(1, 0, 8, 16, A, 0.25, 1.0, 41632),
    RL(2, 0, 8, 24, Bc, 0.0, 0.5, 78560, tiny=True),
    RL(2, 1, 8, 32, Bc, 0.25, 1.0, 108832),
    RL(1, 0, 4, 8, Bc, 0.0, 0.5, 19552),
    RL(2, 0, 4, 24, A, 0.25, 1.0, 78560),
    RL(2, 1, 4, 32, A, 0.0, 0.5, 108832),
    RL(1, 0, 8, 8, A, 0.25, 1.0, 19552),
    RL(2, 0, 8, 24, N3, 0.0, 1.0, 78560, entry='chain'),
)


def key(row):
    """r48_variant_key of resblock48.hip | rl_variant_key of resblock_lean.hip."""
    if row.kernel == 'rb48':
        return row.variant[0] | row.variant[1] << 1
    return row.variant[0] | row.variant[1] << 2 | row.variant[2] << 3


def maps(row):
    return row.batch if row.batch else 1


def row_name(i, row):
    return 'block %02d %s %s %s c%d n%d' % (i, row.kernel, '.'.join(str(int(v)) for v in row.variant), row.entry, row.c, len(row.plan)) + (' B%d' % row.batch if row.batch else '')


# ---- the shapes of the runs, the walk ------------------------------------------------------------------------------------------------
def walk_bound(row):
    """Upper bound of the grid on a stream with a CU budget of 8 (fixed_variant_cases.walk_bound; resblock48: one workgroup per CU)."""
    return 8 if row.kernel == 'rb48' else max(8, (fv.WALK_CUS * (fv.LDS_BYTES // row.lds)) & ~7)


def grids(row):
    """Every grid the launcher can choose on that stream: the multiples of 8 up to the bound (the occupancy is the runtime's word)."""
    return list(range(8, walk_bound(row) + 1, 8))


def tiles_xy(hw):
    return -(-hw[0] // TH), -(-hw[1] // TW)


def n_tiles(row, hw):
    ty, tx = tiles_xy(hw)
    return ty * tx * maps(row)


def walk_shape(row):
    """resblock48: SMALL again.  lean: the smallest h = 8 a + 3, w = 32 b + 13 with a, b >= 3 (by the longer side in tiles, then by
    area) whose tile count is at least 2 walk_bound + 1 -- the rule of fixed_variant_cases.walk_shape with room for interior tiles."""
    if row.kernel == 'rb48':
        return SMALL
    need, best = 2 * walk_bound(row) + 1, None
    for a in range(3, 64):
        for b in range(3, 64):
            if (a + 1) * (b + 1) >= need:
                hw = (TH * a + 3, TW * b + 13)
                if best is None or (max(a, b), hw[0] * hw[1]) < best[0]:
                    best = ((max(a, b), hw[0] * hw[1]), hw)
                break
    assert n_tiles(row, best[1]) >= need
    return best[1]


def runs_of(row):
    return RUNS if row.tiny else RUNS[:2]


def shape(row, run):
    return {'small': SMALL, 'walk': walk_shape(row), 'tiny': TINY}[run]


def tile_ranges(n, g):
    """rv_tile_range of common.h for every workgroup b < g: [(first tile, one past the last)]."""
    out = []
    for b in range(g):
        rank = b
        if g >= 8:
            xcd, rank = b & 7, b >> 3
            for y in range(xcd):
                rank += (g - y + 7) >> 3
        out.append((rank * n // g, (rank + 1) * n // g))
    return out


def later_tiles(n, g):
    """Flat indices of the tiles that come second or later in their workgroup's range."""
    return [t for lo, hi in tile_ranges(n, g) for t in range(lo + 1, hi)]


def tile_origin(hw, t):
    """(map, ty0, tx0) of flat tile t: t = map * tiles per map + tile of the map, row-major (resblock48.hip x_fetch)."""
    ty, tx = tiles_xy(hw)
    b, t = divmod(t, ty * tx)
    return b, t // tx * TH, t % tx * TW


def is_interior(hw, ty0, tx0):
    """The fast path of resblock48's x_fetch / epilogues: the 12 x 36 window lies inside the frame."""
    return ty0 >= 2 and ty0 + TH + 2 <= hw[0] and tx0 >= 2 and tx0 + TW + 2 <= hw[1]


def tile_mask(hw, nmaps, tiles):
    """bool [nmaps, h, w]: the pixels of the listed flat tiles."""
    m = torch.zeros(nmaps, hw[0], hw[1], dtype=torch.bool)
    for t in tiles:
        b, y, x = tile_origin(hw, t)
        m[b, y:y + TH, x:x + TW] = True
    return m


# ---- wrong kernels, from the reference's own pieces ------------------------------------------------------------------------------------
def _lrelu(v, s):
    return v if s == 1.0 else torch.where(v >= 0, v, v * s)


def _half(v):
    return v.float().half().double()


def _block(x, blk, act, post, zero_t=True):
    """One block on a whole map, the intermediate map as the kernels hold it: on the frame and one ring around it.  zero_t: the ring
    is zeroed (conv2's padding: exact_cases.ref_blocks); False: it keeps act(conv1 of the zero-padded x + b1) -- control (d)."""
    w1, b1, w2, b2 = blk
    t = _half(_lrelu(F.conv2d(F.pad(x, (2, 2, 2, 2))[None], w1, b1)[0], act))
    if zero_t:
        t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = 0, 0, 0, 0
    return _half(_lrelu(F.conv2d(t[None], w2, b2)[0] + x, post))


def _block_stale(xs, blk, act, post, stale):
    """One block on the maps of a launch, tile by tile where a tile is in `stale`: that tile computes from the 12 x 36 window of the
    flat tile before it (the previous map's last tile where it is a map's first), residual included -- a parked tile that never
    arrived.  The intermediate map is still zeroed by the tile's own frame coordinates, the stores are still clipped."""
    w1, b1, w2, b2 = blk
    h, w = xs[0].shape[1:]
    ty, tx = tiles_xy((h, w))
    pad = [F.pad(x, (2, tx * TW - w + 2, 2, ty * TH - h + 2)) for x in xs]
    outs = [_block(x, blk, act, post) for x in xs]
    for t in stale:
        b, y0, x0 = tile_origin((h, w), t)
        pb, py, px = tile_origin((h, w), t - 1)
        win = pad[pb][:, py:py + TH + 4, px:px + TW + 4]
        tt = _half(_lrelu(F.conv2d(win[None], w1, b1)[0], act))
        iy, ix = torch.arange(y0 - 1, y0 + TH + 1), torch.arange(x0 - 1, x0 + TW + 1)
        tt = tt * (((iy >= 0) & (iy < h))[:, None] & ((ix >= 0) & (ix < w))[None, :])
        o = _half(_lrelu(F.conv2d(tt[None], w2, b2)[0] + win[:, 2:TH + 2, 2:TW + 2], post))
        hh, ww = min(TH, h - y0), min(TW, w - x0)
        outs[b][:, y0:y0 + hh, x0:x0 + ww] = o[:, :hh, :ww]
    return outs


def wrong_kernels(cases, stale=()):
    """{control: [output of map b]} for the maps of one launch (weights shared).  In every block of the chain:
       a  W1 used for both convs (the swap to W2 dropped; the biases have their own LDS words and stay)
       b  W2 used for both (the swap back to W1 dropped)
       c  conv1 fed the previous tile's window, on the tiles `stale` (none: no entry)
       d  the intermediate map not zeroed outside the frame
    and `plain`, the same code with nothing wrong: it must equal the reference."""
    p = cases[0].p
    act, post = p['act'], p.get('post', 1.0)
    xs0 = [c.p['x'] for c in cases]

    def chain(fn, blocks=p['blocks']):
        xs = xs0
        for blk in blocks:
            xs = fn(xs, blk)
        return xs
    out = {'plain': chain(lambda xs, blk: [_block(x, blk, act, post) for x in xs]),
           'a': chain(lambda xs, blk: [_block(x, blk, act, post) for x in xs], [(w1, b1, w1, b2) for (w1, b1, w2, b2) in p['blocks']]),
           'b': chain(lambda xs, blk: [_block(x, blk, act, post) for x in xs], [(w2, b1, w2, b2) for (w1, b1, w2, b2) in p['blocks']]),
           'd': chain(lambda xs, blk: [_block(x, blk, act, post, zero_t=False) for x in xs])}
    if len(stale):
        out['c'] = chain(lambda xs, blk: _block_stale(xs, blk, act, post, stale))
    return out


def controls(cases, row, run):
    """{control: bool [maps, C, h, w]}: the outputs of the launch that each wrong kernel changes; 'e' is exact_cases' control (b),
    the lo term of one K-block dropped.  Control (c) is taken at the largest grid the walk run can get."""
    hw = tuple(cases[0].p['x'].shape[1:])
    stale = later_tiles(n_tiles(row, hw), walk_bound(row)) if run == 'walk' else ()
    want = torch.stack([c.want['out'] for c in cases])
    wk = wrong_kernels(cases, stale)
    assert torch.equal(torch.stack(wk.pop('plain')), want), 'the tile-wise restatement is not the reference'
    out = dict((k, torch.stack(v) != want) for k, v in wk.items())
    out['e'] = torch.stack([c.evaluate('drop')[0]['out'] for c in cases]) != want
    return out


def weak(cases, row, run):
    """None, or why the launch is not a strong test: exact_cases.assert_strong per map; every control must change CTL_B_MIN of the
    launch's outputs and CTL_B_COUNT of them; on a walk run, for EVERY grid the launcher can choose, CTL_B_COUNT outputs inside the
    tiles that come second or later in a workgroup's range."""
    for c in cases:
        try:
            c.assert_strong()
        except AssertionError as e:
            return str(e)
    hw = tuple(cases[0].p['x'].shape[1:])
    ctl = controls(cases, row, run)
    if run == 'walk' and 'c' not in ctl:
        return 'no control (c)'
    masks = [tile_mask(hw, len(cases), later_tiles(n_tiles(row, hw), g))[:, None] for g in grids(row)] if run == 'walk' else []
    for k in sorted(ctl):
        d = ctl[k]
        if float(d.double().mean()) < ec.CTL_B_MIN or int(d.sum()) < ec.CTL_B_COUNT:
            return 'control (%s) = %.4f (%d elements)' % (k, float(d.double().mean()), int(d.sum()))
        for g, m in zip(grids(row), masks):
            if int((d & m).sum()) < ec.CTL_B_COUNT:
                return 'control (%s): %d elements in the later tiles of grid %d' % (k, int((d & m).sum()), g)
    return None


def control_line(cases, row, run):
    ctl = controls(cases, row, run)
    return ' '.join('%s=%.3f' % (k, float(ctl[k].double().mean())) for k in sorted(ctl))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def build_cases(i, run):
    """[the case of map b] of row i's run: the first seed of the row's sequence at which the launch is strong (weak(): on the
    reference alone); the maps of a multi-map row have their own data and map 0's weights."""
    row = ROWS[i]
    hw = shape(row, run)
    base = 12000 + 64 * i + 16 * RUNS.index(run)
    name = '%s %s %dx%d' % (row_name(i, row), run, hw[0], hw[1])
    why = None
    for k in range(24):
        cases = []
        for b in range(maps(row)):
            c = ec._blocks_case(name + (' map %d' % b if row.batch else ''), base + b + 7919 * k, row.kernel, row.c, hw, row.plan, row.act, row.post,
                                mag_exp=row.mag_exp)
            if b:
                c.p.update((k_, cases[0].p[k_]) for k_ in fv.WEIGHTS if k_ in c.p)
            cases.append(c)
        why = weak(cases, row, run)
        if why is None:
            return cases
    raise AssertionError('%s: no strong case in 24 seeds (%s)' % (name, why))


_CACHE = {}


def get_cases(i, run):
    if (i, run) not in _CACHE:
        _CACHE[(i, run)] = build_cases(i, run)
    return _CACHE[(i, run)]
