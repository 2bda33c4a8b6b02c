"""Exact-arithmetic cases of the matching kernels (refvsr_match_patches, _lo_rows, _top2, _refine, _exact): inputs, float64 references,
column classes and controls.  numpy only -- the kernels run in tests/test_gpu_match_exact.py, the cases are proved in
tests/test_match_cases.py.

EXACTNESS CONDITION (Case.exactness, checked for every case on the CPU).  Every operand is a dyadic rational its storage type holds
(rows fp16, features and inv fp32), and for every (row, column) pair  sum |a b| over the 144 terms / g < 2^24,  g = the common
granularity of the products (per K slot: granule of the slot's row operands x granule of its column operands; the smallest over the
slots).  Every partial sum, in any order, with or without FMA contraction, is then an integer multiple of g below 2^24 g: an fp32
number.  Summation order, MFMA shape, K slot order inside a step and the hi + lo fold cannot change a score; the kernels must return
the reference's BITS and, with the first of equal values winning like torch.max, the reference's indices.

REFERENCES.  Plain on purpose: the score table is R.astype(f8) @ L.astype(f8).T, the top-2 of a row range the first two rows under
np.lexsort((index, -score)), the arg-max the first maximal index.  No model of a kernel's streaming order.

FAMILIES
  T  match_top2 on prescribed score tables: LR column p is the one-hot row e_(p mod 144), so score[r][p] = ref_rows[r][p mod 144] --
     the reference row matrix IS the score table and every pattern (ties, placements in the 32-row tile / 256-row stage, staircases,
     all-negative columns next to zero pad rows) is written down directly, one pattern per column type, repeated at every column
     position (wave, ct, l31) of the 512-column blocks.
  G  match_top2 on integers in [-3, 3] in all 144 slots of both operands: every K step and both K halves of a lane contribute.
  R  match_refine on crafted candidate lists over small-integer feature maps (duplicates, out-of-range entries, equal values in both
     orders, fp16-score perturbations inside the kernel's premise, the flag condition at equality).
  E  match_exact: every column searched (margin = inf) and crafted flagged lists with pre-filled conf / idx; the lo-term cases
     (entries a + b 2^-13, b only in the K slots of even channels on the LR side and of odd channels on the reference side: every
     b b' product is zero, the three-MFMA sum IS the dot product, and the hi-only score misranks).
  P  match_patches end to end: every 3x3 window's sum of squares is a power of 4, so sqrtf, the reciprocal and v * inv are exact.

CONTROLS.  Wrong models applied to the REFERENCE (never run on a GPU): each must change the expected output of at least one case, and
where it names a term or an edge, of a case built for it (test_match_cases.py prints "changes N columns in case X").  A kernel that
behaves like a control therefore fails at least that case in tests/test_gpu_match_exact.py."""
import functools

import numpy as np

F64, F32, F16 = np.float64, np.float32, np.float16
K, KP, ROWCHUNK, COLBLOCK = 144, 152, 256, 512        # = refvsr_amd.hip.MATCH_KP / MATCH_ROWCHUNK / MATCH_COLBLOCK (test_match_cases.py)
TILE, EX_STAGE, EX_TILE = 32, 64, 16                  # match_top2: rows per MFMA tile; match_exact: rows per stage / per MFMA tile
LO_SCALE = 2048.0
NEG_INF = -np.inf

CONTROLS = ('last of equals', 'pad rows not masked', 'one lane half only', 'merge prefers partner lane', 'skip rule 1 x margin',
            'flag with >', 'ah.bl dropped', 'al.bh dropped', 'last real row masked', 'first pad row admitted')


# ---- host side of the ABI --------------------------------------------------------------------------------------------------------
def round_up(a, b):
    return (a + b - 1) // b * b


def reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def unfold(feat):
    """[C, h, w] -> [h*w, C*9]: reflect-pad 3x3 unfold, element e = c*9 + ky*3 + kx."""
    C, h, w = feat.shape
    fp = feat[:, reflect(np.arange(-1, h + 1), h)][:, :, reflect(np.arange(-1, w + 1), w)]
    taps = [fp[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)]
    return np.stack(taps, 1).reshape(C * 9, h * w).T.copy()


def rows16(m, mult):
    """float64 [n, 144] of fp16 numbers -> fp16 [round_up(n, mult), KP]; pad slots and pad rows zero."""
    m = np.asarray(m, F64)
    assert np.array_equal(m.astype(F16).astype(F64), m), 'row operand is not an fp16 number'
    out = np.zeros((round_up(m.shape[0], mult), KP), F16)
    out[:m.shape[0], :K] = m
    return out


def split_rows(v):
    """v = normalised rows (float64 of fp32 numbers) -> (hi, lo) as match_patches stores them: hi = fp16(v), lo = fp16((v - hi) 2^11)."""
    hi = v.astype(F32).astype(F16).astype(F64)
    lo = ((v - hi) * LO_SCALE).astype(F32).astype(F16).astype(F64)
    return hi, lo


# ---- exactness ----------------------------------------------------------------------------------------------------------------------
def granule_exp(a):
    """Smallest e such that a * 2^e is all integers (a: finite dyadic rationals); None for an all-zero array."""
    a = np.abs(np.asarray(a, F64).ravel())
    a = a[a != 0]
    if a.size == 0:
        return None
    m, ex = np.frexp(a)
    M = (m * 2.0 ** 53).astype(np.int64)
    low = np.log2((M & -M).astype(F64)).astype(np.int64)
    return int(-(ex - 53 + low).min())


def exactness(A, B):
    """log2 of max over pairs of  sum_k |A[r][k] B[p][k]| / g  (the condition: < 24), g = the products' common granularity."""
    e = 0
    for k in range(A.shape[1]):
        ea, eb = granule_exp(A[:, k]), granule_exp(B[:, k])
        if ea is not None and eb is not None:
            e = max(e, ea + eb)
    worst = float((np.abs(A) @ np.abs(B).T).max())
    return float(np.log2(max(worst, 2.0 ** -300))) + e


def scores64(R, L):
    return R.astype(F64) @ L.astype(F64).T


def scores32(R, L, order):
    """float32 evaluation in two different summation orders: 0 = one product and one add per K slot, ascending; 1 = sgemm over the
    slots in descending order (blocked, fused multiply-adds)."""
    a, b = R.astype(F32), L.astype(F32)
    if order == 1:
        return np.ascontiguousarray(a[:, ::-1]) @ np.ascontiguousarray(b[:, ::-1]).T
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, :, k]
    return acc


# ---- references ---------------------------------------------------------------------------------------------------------------------
def split_ranges(n_ref, splits):
    """Row range of every split, from refvsr_match_top2's launch arithmetic; None where its two checks reject the combination."""
    n_chunks = round_up(n_ref, ROWCHUNK) // ROWCHUNK
    if n_ref < 2 or splits < 1 or splits > n_chunks:
        return None
    cps = (n_chunks + splits - 1) // splits
    if (splits - 1) * cps >= n_chunks:
        return None
    return [(s * cps * ROWCHUNK, min((s + 1) * cps, n_chunks) * ROWCHUNK) for s in range(splits)]


def top2_range(sc, n_ref, lo, hi, model=None):
    """Top-2 of rows [lo, min(hi, n_ref)) of the score table sc [n_ref, n]: (idx [n, 2], val [n, 2]).  A range with one row has
    (-inf, any index) as its second entry."""
    n = sc.shape[1]
    end = min(hi, n_ref)
    if model == 'last real row masked':
        end = min(hi, n_ref - 1)
    if model in ('pad rows not masked', 'first pad row admitted'):
        end = hi if model == 'pad rows not masked' else min(hi, n_ref + 1)
        end = min(end, round_up(n_ref, ROWCHUNK))
        sc = np.concatenate([sc, np.zeros((max(end - n_ref, 0), n), F64)])
    rows = np.arange(lo, end)
    if model == 'one lane half only':
        rows = rows[rows % 8 < 4]
    blk = sc[rows].T                                             # [n, rows]
    ix = np.broadcast_to(rows, blk.shape)
    if model == 'last of equals':
        order = np.lexsort((-ix, -blk), axis=-1)
    elif model == 'merge prefers partner lane':
        order = np.lexsort((ix, -(ix % 8 >= 4).astype(np.int64), -blk), axis=-1)
    else:
        order = np.lexsort((ix, -blk), axis=-1)
    idx = np.zeros((n, 2), np.int64)
    val = np.full((n, 2), NEG_INF)
    for j in range(min(2, len(rows))):
        idx[:, j] = rows[order[:, j]]
        val[:, j] = np.take_along_axis(blk, order[:, j:j + 1], 1)[:, 0]
    return idx, val


def top2_ref(sc, n_ref, splits, model=None):
    """(cand_idx [n, 2 splits], cand_val [n, 2 splits]) in the kernel's layout: split s at entries 2 s, 2 s + 1."""
    parts = [top2_range(sc, n_ref, lo, hi, model) for lo, hi in split_ranges(n_ref, splits)]
    return np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1)


def argmax_ref(sc, model=None):
    """(first maximal index, maximum) of every column."""
    if model == 'last real row masked':
        sc = sc[:-1]
    elif model == 'first pad row admitted':
        sc = np.concatenate([sc, np.zeros((1, sc.shape[1]), F64)])
    if model == 'last of equals':
        idx = sc.shape[0] - 1 - np.argmax(sc[::-1], 0)
    else:
        idx = np.argmax(sc, 0)
    return idx.astype(np.int64), sc[idx, np.arange(sc.shape[1])]


def refine_ref(sc, cand, cand_val=None, margin=None, model=None):
    """match_refine on the exact score table sc [n_ref, n]: the exact best of ALL listed candidates (clamped to [0, n_ref); the smaller
    index of equal values), and with cand_val / margin the flagged columns {p : not (best - max(second entries) >= margin)}.
    Returns (idx, val, flagged bool [n] or None)."""
    n_ref, n = sc.shape
    c = np.clip(cand.astype(np.int64), 0, n_ref - 1)
    ex = sc[c, np.arange(n)[:, None]]
    if cand_val is not None and model == 'skip rule 1 x margin':    # the kernel's skip rule with half its slack
        top16 = cand_val.max(1, keepdims=True)
        keep = (cand_val > top16 - 1.0 * margin) | (cand_val == top16)
        ex = np.where(keep, ex, NEG_INF)
        c = np.where(keep, c, np.iinfo(np.int32).max)
    order = np.lexsort((c, -ex), axis=-1)[:, 0]
    idx, val = c[np.arange(n), order], ex[np.arange(n), order]
    if cand_val is None:
        return idx, val, None
    m2 = cand_val[:, 1::2].max(1)
    with np.errstate(invalid='ignore'):
        ok = (val - m2 > margin) if model == 'flag with >' else (val - m2 >= margin)
    return idx, val, ~ok


def exact_ref(sc, flagged, conf0, idx0, model=None):
    """match_exact + finish: the flagged columns take the first arg-max where it beats the pre-filled (conf, idx); the others keep
    their bits."""
    ai, av = argmax_ref(sc, model)
    conf, idx = conf0.copy(), idx0.copy()
    f = np.zeros(sc.shape[1], bool)
    f[flagged] = True
    take = f & ((av > conf0) | ((av == conf0) & (ai < idx0)))
    conf[take], idx[take] = av[take], ai[take]
    return idx, conf


# ---- column classes of family T ----------------------------------------------------------------------------------------------------
def geo(r):
    j = r % TILE
    return dict(tile=r // TILE, stage=r // ROWCHUNK, half=(j % 8) // 4, quad=j // 8)


def placement(r1, r2):
    """Where two rows sit relative to each other in match_top2's walk (r1 = the first-place row)."""
    a, b = geo(r1), geo(r2)
    if a['stage'] != b['stage']:
        return 'different stages'
    if a['tile'] != b['tile']:
        return 'different tiles'
    if a['half'] != b['half']:
        return 'partner lanes, %s half first' % ('low' if a['half'] == 0 else 'high')
    if a['quad'] != b['quad']:
        return 'different quads of one lane'
    return 'same quad'


PLACEMENTS = ('same quad', 'different quads of one lane', 'partner lanes, low half first', 'partner lanes, high half first',
              'different tiles', 'different stages')
BUILT = ('ascending staircase', 'descending staircase', "late value equal to the partner lane's runner-up")
T_CLASSES = (('all distinct', 'all equal, positive', 'all equal, zero', 'all equal, negative', 'pad rows, negative scores')
             + tuple('max at tile row %d' % j for j in range(TILE))
             + ('max in an even tile', 'max in an odd tile', 'max in the first half of a stage', 'max in the second half of a stage',
                'max at the first row of a stage', 'max at the last row of a stage', 'max at row n_ref - 1')
             + tuple('winner and runner-up: ' + p for p in PLACEMENTS) + tuple('two-way tie: ' + p for p in PLACEMENTS)
             + ('three-way tie', 'tie between second and third') + BUILT)


def column_classes(col):
    """Class labels of one score column (all rows real)."""
    n = len(col)
    order = np.lexsort((np.arange(n), -col))
    i1, i2 = int(order[0]), int(order[1])
    v1, v2 = col[i1], col[i2]
    v3 = col[order[2]] if n > 2 else None
    out = ['max at tile row %d' % (i1 % TILE), 'max in an %s tile' % ('even' if (i1 // TILE) % 2 == 0 else 'odd'),
           'max in the %s half of a stage' % ('first' if i1 % ROWCHUNK < ROWCHUNK // 2 else 'second')]
    if i1 % ROWCHUNK == 0 and i1 > 0:
        out.append('max at the first row of a stage')
    if i1 % ROWCHUNK == ROWCHUNK - 1:
        out.append('max at the last row of a stage')
    if i1 == n - 1:
        out.append('max at row n_ref - 1')
    if v1 != v2:
        out.append('winner and runner-up: ' + placement(i1, i2))
        if v3 is not None and v2 == v3:
            out.append('tie between second and third')
    elif v3 is not None and v3 == v1:
        out.append('three-way tie')
    else:
        out.append('two-way tie: ' + placement(i1, i2))
    if len(np.unique(col)) == n:
        out.append('all distinct')
    if col.min() == col.max():
        out.append('all equal, %s' % ('positive' if v1 > 0 else 'zero' if v1 == 0 else 'negative'))
    if v1 < 0 and n % ROWCHUNK:
        out.append('pad rows, negative scores')
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
class Top2Case(object):
    """match_top2 on host-built rows: ref [n_ref, 144] and lr [n_lr, 144] float64 of fp16 numbers; inv = 1 (no normalisation)."""

    def __init__(self, name, family, ref, lr, tags=None):
        self.name, self.family, self.ref, self.lr = name, family, ref, lr
        self.n_ref, self.n_lr = ref.shape[0], lr.shape[0]
        self.tags = tags or {}                                   # column type -> builder tag (family T)
        self._sc = None

    def operands(self):
        return [(self.ref, self.lr_types())]

    def lr_types(self):
        return self.lr[:K] if self.family == 'T' else self.lr   # T: columns p and p + 144 k are one type

    def rows(self):
        return rows16(self.ref, ROWCHUNK), rows16(self.lr, COLBLOCK)

    def scores(self):
        if self._sc is None:
            self._sc = scores64(self.ref, self.lr)
        return self._sc

    def splits(self):
        return [s for s in (1, 2, 3) if split_ranges(self.n_ref, s) is not None]

    def want(self, splits, model=None):
        return top2_ref(self.scores(), self.n_ref, splits, model)

    def single_row_ranges(self, splits):
        return [min(hi, self.n_ref) - lo == 1 for lo, hi in split_ranges(self.n_ref, splits)]

    @functools.lru_cache(maxsize=None)
    def type_classes(self, t):
        if self.family != 'T':
            return ('general integers',)
        return tuple(column_classes(self.ref[:, t])) + ((self.tags[t],) if t in self.tags else ())

    def classes(self, p):
        return self.type_classes(p % K)


def _tile_rows(n_ref, rng, want, ordered=False):
    """Rows realising a placement (first-place row first; ordered: r1 < r2), or None where n_ref has no room for it."""
    for _ in range(64):
        t = int(rng.integers(0, (n_ref + TILE - 1) // TILE))
        g, h, j = (int(v) for v in rng.integers(0, [4, 2, 4]))
        r1 = t * TILE + 8 * g + 4 * h + j
        if want == 'same quad':
            r2 = t * TILE + 8 * g + 4 * h + (j + 1 + int(rng.integers(0, 3))) % 4
        elif want == 'different quads of one lane':
            r2 = t * TILE + 8 * ((g + 1 + int(rng.integers(0, 3))) % 4) + 4 * h + int(rng.integers(0, 4))
        elif want.startswith('partner lanes'):
            h = 0 if 'low' in want else 1
            r1 = t * TILE + 8 * g + 4 * h + j
            r2 = t * TILE + 8 * int(rng.integers(0, 4)) + 4 * (1 - h) + int(rng.integers(0, 4))
        elif want == 'different tiles':
            r2 = r1 % ROWCHUNK // TILE
            r2 = (r1 // ROWCHUNK) * ROWCHUNK + ((r2 + 1 + int(rng.integers(0, 7))) % 8) * TILE + int(rng.integers(0, TILE))
        else:
            r2 = int(rng.integers(0, n_ref))
        if max(r1, r2) < n_ref and r1 != r2 and placement(r1, r2) == want and (r1 < r2 or not ordered):
            return r1, r2
    return None


def build_T(n_ref, n_lr, seed):
    rng = np.random.default_rng(seed)
    S = np.zeros((n_ref, K), F64)
    tags = {}
    cols = []                                                     # (values, tag)

    def bg():
        return rng.integers(-60, -19, n_ref).astype(F64)

    def put(rows_vals, tag=None):
        c = bg()
        for r, v in rows_vals:
            c[r] = v
        cols.append((c, tag))

    def any_row(avoid=()):
        while True:
            r = int(rng.integers(0, n_ref))
            if r not in avoid:
                return r

    cols.append((rng.permutation(n_ref).astype(F64) - n_ref // 2, None))                  # all distinct
    for v in (2.0, 0.0, -2.0):
        cols.append((np.full(n_ref, v), None))
    cols.append((rng.integers(-50, 0, n_ref).astype(F64), None))                           # all negative, ties likely
    cols.append((np.arange(n_ref, dtype=F64) - n_ref // 2, 'ascending staircase'))
    cols.append((n_ref // 2 - np.arange(n_ref, dtype=F64), 'descending staircase'))
    for j in range(TILE):                                                                  # the maximum at every row of a tile
        tiles = [t for t in range((n_ref + TILE - 1) // TILE) if t * TILE + j < n_ref]
        r1 = (tiles[(5 * j + 1) % len(tiles)] * TILE + j) if tiles else j % n_ref
        put([(any_row((r1,)), 10.0), (r1, 20.0)])
    for pl in PLACEMENTS:
        for kind in ('wr', 'rw', 'tie'):                                                   # (of a tie, the FIRST row is the one the placement names)
            r1, r2 = _tile_rows(n_ref, rng, pl, ordered=kind == 'tie') or (0, 1)
            put([(r1, 20.0), (r2, 20.0 if kind == 'tie' else 10.0)] if kind != 'rw' else [(r2, 20.0), (r1, 10.0)])
    if n_ref > 2:
        a = any_row(); b = any_row((a,)); c = any_row((a, b))
        put([(a, 20.0), (b, 20.0), (c, 20.0)])                                             # three-way tie
        put([(a, 20.0), (b, 10.0), (c, 10.0)])                                             # second = third
        put([(0, 20.0), (n_ref - 1, 20.0), (n_ref // 2, 20.0)])
    put([(n_ref - 1, 20.0), (0, 10.0)])                                                    # the last real row
    put([(n_ref - 1, 20.0), (n_ref - 2, 20.0)])
    for st in range(1, (n_ref + ROWCHUNK - 1) // ROWCHUNK):
        put([(st * ROWCHUNK, 20.0), (any_row((st * ROWCHUNK,)), 10.0)])                    # first / last row of a stage
        put([(st * ROWCHUNK - 1, 20.0), (st * ROWCHUNK, 20.0)])
        put([(st * ROWCHUNK - 1, 20.0), (any_row((st * ROWCHUNK - 1,)), 10.0)])
        if st * ROWCHUNK + 4 < n_ref:                                                      # rows 0, 1: low lane half; row 4 of a later stage: high
            put([(0, 20.0), (1, 10.0), (st * ROWCHUNK + 4, 10.0)], BUILT[2])
        if st * ROWCHUNK + 9 < n_ref:                                                      # the other way round
            put([(4, 20.0), (5, 10.0), (st * ROWCHUNK + 9, 10.0)], BUILT[2])
    if n_ref >= 200:                                                                       # second half of a stage, after the mid-stage park
        r1 = (n_ref - 1) // ROWCHUNK * ROWCHUNK + 128 + int(rng.integers(0, 64))
        r1 = r1 if r1 < n_ref else 128 + int(rng.integers(0, 64))
        put([(r1, 20.0), (any_row((r1,)), 10.0)])
    while len(cols) < K:                                                                   # random pairs and ties
        a = any_row(); b = any_row((a,))
        put([(a, 20.0), (b, 20.0 if rng.integers(0, 3) == 0 else 10.0)])
    for t, (c, tag) in enumerate(cols[:K]):
        neg = t >= 7 and t % 2 == 1 and tag is None                                        # every second pattern: all scores negative
        S[:, t] = c - 100.0 if neg else c
        if tag:
            tags[t] = tag
    lr = np.zeros((n_lr, K), F64)
    lr[np.arange(n_lr), np.arange(n_lr) % K] = 1.0
    return Top2Case('T n_ref=%d n_lr=%d' % (n_ref, n_lr), 'T', S, lr, tags)


def build_G(n_ref, n_lr, seed):
    rng = np.random.default_rng(seed)
    return Top2Case('G n_ref=%d n_lr=%d' % (n_ref, n_lr), 'G', rng.integers(-3, 4, (n_ref, K)).astype(F64),
                    rng.integers(-3, 4, (n_lr, K)).astype(F64))


# a covering set of the cross {2, 3, 255, 256, 257, 512, 513, 777} x {1, 31, 33, 64, 511, 512, 513, 1100}: every n_ref and every n_lr at
# least twice, the large n_lr (several column blocks) with every stage count
SIZES = ((2, 1), (2, 513), (3, 31), (3, 1100), (255, 33), (255, 512), (256, 64), (256, 511), (257, 1), (257, 513), (257, 1100),
         (512, 31), (512, 512), (513, 33), (513, 64), (513, 1100), (777, 64), (777, 511), (777, 513), (777, 1100))
TOP2_NAMES = tuple('%s %d x %d' % (f, a, b) for f in 'TG' for a, b in SIZES)
REJECTED = ((777, 3), (256, 2), (513, 4), (2, 2))                 # (n_ref, row_splits) that refvsr_match_top2 must refuse


@functools.lru_cache(maxsize=None)
def top2_case(name):
    f, a, _, b = name.split()
    a, b = int(a), int(b)
    return (build_T if f == 'T' else build_G)(a, b, 1000 * SIZES.index((a, b)) + (0 if f == 'T' else 500))


class FeatCase(object):
    """Feature maps lf [16, h, w] / rf [16, hr, wr] (float64 of fp32 numbers) with inv vectors that are powers of two; the rows the
    kernels take are built here on the host: unfold * inv, split into fp16 hi + lo."""

    def __init__(self, name, lf, rf, il, ir):
        self.name, self.lf, self.rf, self.il, self.ir = name, lf, rf, il, ir
        self.h, self.w = lf.shape[1:]
        self.hr, self.wr = rf.shape[1:]
        self.n, self.n_ref = self.h * self.w, self.hr * self.wr
        self.L, self.R = unfold(lf), unfold(rf)
        self.lr_hi, self.lr_lo = split_rows(self.L * il[:, None])
        self.ref_hi, self.ref_lo = split_rows(self.R * ir[:, None])
        assert np.array_equal(self.lr_hi + self.lr_lo / LO_SCALE, self.L * il[:, None])
        assert np.array_equal(self.ref_hi + self.ref_lo / LO_SCALE, self.R * ir[:, None])
        for v in (lf, rf, il, ir):
            assert np.array_equal(v.astype(F32).astype(F64), v)
        self._sc = {}

    def operands(self):
        """Operand pairs the kernels multiply: raw patches (patch_dot) and the split rows (MFMA: hh, and hl + lh in one accumulator)."""
        return [(self.R, self.L), (self.ref_hi, self.lr_hi),
                (np.concatenate([self.ref_hi, self.ref_lo], 1), np.concatenate([self.lr_lo, self.lr_hi], 1))]

    def scores(self, model=None):
        """score[r][p] = <R_r, L_p> inv_ref[r] inv_lr[p]; the two term-dropping controls act on the three-term sum of the split rows."""
        if model not in self._sc:
            if model in ('ah.bl dropped', 'al.bh dropped'):
                sc = scores64(self.ref_hi, self.lr_hi)
                sc += (scores64(self.ref_lo, self.lr_hi) if model == 'ah.bl dropped' else scores64(self.ref_hi, self.lr_lo)) / LO_SCALE
            else:
                sc = scores64(self.R, self.L) * self.ir[:, None] * self.il[None, :]
            self._sc[model] = sc
        return self._sc[model]

    def classes(self, p):
        return ('feature maps',)

    def rows(self):
        """(lr_hi, lr_lo, ref_hi, ref_lo) fp16: LR rows unpadded, reference rows padded to the 256-row multiple."""
        return rows16(self.lr_hi, 1), rows16(self.lr_lo, 1), rows16(self.ref_hi, ROWCHUNK), rows16(self.ref_lo, ROWCHUNK)


def int_maps(rng, h, w, hr, wr, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, (16, h, w)).astype(F64), rng.integers(lo, hi + 1, (16, hr, wr)).astype(F64)


def pow2(rng, n, exps):
    return 2.0 ** rng.choice(np.asarray(exps, F64), n)


# ---- family R ------------------------------------------------------------------------------------------------------------------------
R_SHAPES = ((2, 2, 2, 2), (3, 5, 2, 3), (9, 15, 5, 7), (13, 11, 13, 11))
R_MARGINS = (0.0, 2.0 ** -12, np.inf)
R_KINDS = ('random', 'with the arg-max', 'duplicates', 'out of range', 'equal values, small index first', 'equal values, large index first',
           'best - m2 == margin', 'close pair, opposite perturbations')
R_NAMES = (tuple('R %dx%d/%dx%d ncand=%d plain' % (s + (k,)) for s in R_SHAPES for k in (1, 2, 4, 6))
           + tuple('R %dx%d/%dx%d ncand=%d margin=%s' % (s + (k, 'inf' if np.isinf(m) else '0' if m == 0 else '2^-12'))
                   for s in R_SHAPES for k in (2, 4, 6) for m in R_MARGINS))


class RefineCase(object):
    def __init__(self, name, fc, cand, cand_val, margin, kinds):
        self.name, self.fc, self.cand, self.cand_val, self.margin, self.kinds = name, fc, cand, cand_val, margin, kinds

    def want(self, model=None):
        """(idx, conf, flagged set or None): with flagging, ops.match_refine also runs the exhaustive search of the flagged columns, which
        take the first arg-max of all rows."""
        sc = self.fc.scores()
        idx, val, fl = refine_ref(sc, self.cand, self.cand_val, self.margin, model)
        if fl is None:
            return idx, val, None
        ai, av = argmax_ref(sc)
        return np.where(fl, ai, idx), np.where(fl, av, val), np.flatnonzero(fl)

    def classes(self, p):
        return (self.kinds[p],)


@functools.lru_cache(maxsize=None)
def feat_case_R(shape):
    rng = np.random.default_rng(77 + sum(shape))
    lf, rf = int_maps(rng, *shape)
    n, n_ref = shape[0] * shape[1], shape[2] * shape[3]
    return FeatCase('R features %dx%d/%dx%d' % shape, lf, rf, pow2(rng, n, (-6, -7)), pow2(rng, n_ref, (-6, -7)))


@functools.lru_cache(maxsize=None)
def refine_case(name):
    i = R_NAMES.index(name)
    shape = tuple(int(v) for v in name.split()[1].replace('/', 'x').split('x'))
    ncand = int(name.split('ncand=')[1].split()[0])
    mtxt = name.split()[-1]
    margin = None if mtxt == 'plain' else {'margin=0': 0.0, 'margin=2^-12': 2.0 ** -12, 'margin=inf': np.inf}[mtxt]
    fc = feat_case_R(shape)
    sc = fc.scores()
    n, n_ref = fc.n, fc.n_ref
    rng = np.random.default_rng(9000 + i)
    cand = rng.integers(0, n_ref, (n, ncand)).astype(np.int64)
    pert = np.zeros((n, ncand), F64)
    finite = margin is not None and 0 < margin < np.inf
    if margin is not None and margin > 0:
        step = (margin if finite else 2.0 ** -10) / 16
        pert = rng.integers(-14, 15, (n, ncand)).astype(F64) * step          # |perturbation| <= 0.875 margin
    kinds = []
    for p in range(n):
        kind = R_KINDS[(p + i) % len(R_KINDS)]
        col = sc[:, p]
        order = np.lexsort((np.arange(n_ref), -col))
        if kind == 'with the arg-max':
            cand[p, rng.integers(0, ncand)] = order[0]
        elif kind == 'duplicates':
            cand[p, :] = cand[p, 0]
            pert[p, :] = pert[p, 0]
        elif kind == 'out of range':
            cand[p, :] = rng.choice([-1, -7, -2 ** 30, n_ref, n_ref + 5, 2 ** 30, 0, n_ref - 1], ncand)
        elif kind.startswith('equal values') and ncand >= 2:
            vals, first, counts = np.unique(col, return_index=True, return_counts=True)
            if (counts > 1).any():
                v = vals[counts > 1].max()
                a, b = np.flatnonzero(col == v)[:2]
                cand[p, :2] = (a, b) if 'small' in kind else (b, a)
                pert[p, :2] = 0
            else:
                kind = 'random'
        elif kind == 'best - m2 == margin' and ncand >= 2 and margin is not None and np.isfinite(margin):
            # first entry: the best listed row, second entry (m2) a row whose exact score is exactly `margin` below it
            hit = None
            for a in order[:8]:
                b = np.flatnonzero(col == col[a] - margin)
                if margin == 0:
                    b = b[b != a]
                if len(b):
                    hit = (int(a), int(b[0]))
                    break
            if hit:
                cand[p, :] = hit[1]
                cand[p, 0] = hit[0]
                pert[p, :] = 0
            else:
                kind = 'random'
        elif kind == 'close pair, opposite perturbations' and ncand >= 4 and finite:
            # exact scores a > b no further apart than 0.75 margin, fp16 scores a - 0.875 margin and b + 0.875 margin: the better row's
            # fp16 score is >= margin below the top one and still inside the kernel's 2 x margin.  Both sit at even entries; the odd
            # entries (the runner-ups the flag looks at) hold a row far below, so the column is final after the re-rank
            hit = None
            low = int(order[-1])
            for a in order[:16]:
                b = np.flatnonzero((col < col[a]) & (col >= col[a] - 0.75 * margin))
                if len(b) and col[low] <= col[a] - 4 * margin:
                    hit = (int(a), int(b[0]))
                    break
            if hit:
                cand[p, :] = low
                cand[p, 0], cand[p, 2] = hit[1], hit[0]
                pert[p, :] = 0
                pert[p, 0], pert[p, 2] = 14 * margin / 16, -14 * margin / 16
            else:
                kind = 'random'
        elif kind not in ('random',):
            kind = 'random'
        kinds.append(kind)
    cand_val = None
    if margin is not None:
        c = np.clip(cand, 0, n_ref - 1)
        cand_val = sc[c, np.arange(n)[:, None]] + pert
        assert np.array_equal(cand_val.astype(F32).astype(F64), cand_val)
        # the kernel's own arithmetic on these numbers is exact: top16 - 2 margin and best - m2 are fp32 numbers
        if finite:
            t = cand_val.max(1) - 2 * margin
            assert np.array_equal(t.astype(F32).astype(F64), t)
    return RefineCase(name, fc, cand, cand_val, margin, kinds)


# ---- family E ------------------------------------------------------------------------------------------------------------------------
E_REF_SHAPES = {4: (2, 2), 63: (7, 9), 64: (8, 8), 65: (5, 13), 129: (3, 43), 777: (21, 37)}
E_FEATS = (tuple('int n_ref=%d' % n for n in E_REF_SHAPES) + ('negative n_ref=129', 'negative n_ref=777', 'ties n_ref=777',
           'lo const-a n_ref=129', 'lo const-a n_ref=777', 'lo random-a n_ref=65', 'lo random-a n_ref=777'))
E_COUNTS = (0, 1, 255, 256, 257, 'all')
E_LIST_FEATS = ('int n_ref=129', 'int n_ref=777', 'negative n_ref=777', 'ties n_ref=777', 'lo const-a n_ref=777', 'int n_ref=4')
E_ALL_NAMES = tuple('E all ' + f for f in E_FEATS)
E_LIST_NAMES = (tuple('E list %s count=%s' % (f, c) for f in E_LIST_FEATS[:2] for c in E_COUNTS)
                + tuple('E list %s count=%s' % (f, c) for f in E_LIST_FEATS[2:] for c in (1, 257)))
E_CLASSES = (tuple('max at stage row %d' % j for j in range(EX_STAGE))
             + ('tie inside a 16-row tile', 'tie across 16-row tiles', 'tie across stages (row parts)', 'all-negative column',
                'mixed-sign column', 'hi-only score misranks'))
E_LR = (16, 25)                                                   # 400 columns: flagged counts up to 257 and two column groups


@functools.lru_cache(maxsize=None)
def feat_case_E(feat):
    kind, n_ref = feat.rsplit(' n_ref=', 1)
    n_ref = int(n_ref)
    hr, wr = E_REF_SHAPES[n_ref]
    h, w = E_LR
    rng = np.random.default_rng(4000 + n_ref + 17 * len(kind))
    il, ir = pow2(rng, h * w, (-4, -5)), pow2(rng, n_ref, (-4, -5))
    if kind == 'int':
        lf, rf = int_maps(rng, h, w, hr, wr)
    elif kind == 'negative':                                      # every score negative: the zero pad rows must lose
        lf = rng.integers(1, 4, (16, h, w)).astype(F64)
        rf = -rng.integers(1, 4, (16, hr, wr)).astype(F64)
    elif kind == 'ties':                                          # few distinct reference patches: the maximum repeats across tiles and stages
        lf = rng.integers(-3, 4, (16, h, w)).astype(F64)
        rf = np.repeat(rng.integers(-3, 4, (16, hr, 1)), wr, 2).astype(F64)
        rf[:, :, ::5] = rng.integers(-1, 2, (16, hr, len(range(0, wr, 5))))
        ir = np.full(n_ref, 2.0 ** -4)
    else:
        lf, rf = lo_maps(rng, h, w, hr, wr, const_a=kind == 'lo const-a')
        il, ir = np.full(h * w, 2.0 ** -4), np.full(n_ref, 2.0 ** -4)
    return FeatCase('E features ' + feat, lf, rf, il, ir)


def lo_maps(rng, h, w, hr, wr, const_a):
    """Maps with entries a + b 2^-13 (a a nonzero small integer, b a small integer) such that every b b' product of an LR row with a
    reference row is zero.  The rows are unfolds of the maps (match_exact_finish re-evaluates the winner from the MAPS, and
    refvsr_match_lo_rows derives lr_lo from them), and a pixel is read at K slots of both parities by its nine patches, so "b in even
    slots on one side, odd slots on the other" is realised on the slot's CHANNEL: K slot e = 9 c + tap carries b on the LR side for
    even c and on the reference side for odd c.  Every K step of the search's MFMAs (slots 32 s .. 32 s + 31 and the
    16-slot tail) spans at least two channels, i.e. holds both an al.bh and an ah.bl contribution.  const_a: the a part of the reference map is one
    value per channel, so every hi-only score of a column is the same number and the lo terms alone decide the winner."""
    ch = np.arange(16)[:, None, None]
    la = rng.choice([-2.0, -1.0, 1.0, 2.0], (16, h, w))
    ra = rng.choice([-2.0, -1.0, 1.0, 2.0], (16, 1, 1) if const_a else (16, hr, wr)) + np.zeros((16, hr, wr))
    lb = np.where(ch % 2 == 0, rng.integers(-3, 4, (16, h, w)), 0).astype(F64)
    rb = np.where(ch % 2 == 1, rng.integers(-3, 4, (16, hr, wr)), 0).astype(F64)
    return la + lb * 2.0 ** -13, ra + rb * 2.0 ** -13


def exact_classes(sc, hh=None):
    """Class labels of every column of a score table searched by match_exact (64-row stages, 16-row tiles; with few column groups the
    kernel gives every stage to another workgroup, so a tie across stages is a tie across row parts, decided by the atomicMax keys)."""
    out = []
    ai, av = argmax_ref(sc)
    for p in range(sc.shape[1]):
        lab = ['max at stage row %d' % (ai[p] % EX_STAGE)]
        rows = np.flatnonzero(sc[:, p] == av[p])
        if len(rows) > 1:
            st, tl = rows // EX_STAGE, rows // EX_TILE
            if len(np.unique(st)) > 1:
                lab.append('tie across stages (row parts)')
            if len(np.unique(tl)) < len(tl):
                lab.append('tie inside a 16-row tile')
            if any(len(np.unique(tl[st == s])) > 1 for s in np.unique(st)):
                lab.append('tie across 16-row tiles')
        if av[p] < 0:
            lab.append('all-negative column')
        elif sc[:, p].min() < 0:
            lab.append('mixed-sign column')
        if hh is not None and np.argmax(hh[:, p]) != ai[p]:
            lab.append('hi-only score misranks')
        out.append(tuple(lab))
    return out


class ExactCase(object):
    """E all: through ops.match_refine(margin = inf) -- every column flagged; E list: refvsr_match_exact on a crafted flagged list
    (unsorted, `count` distinct columns) with pre-filled conf / idx."""

    def __init__(self, name, fc, count=None):
        self.name, self.fc, self.count = name, fc, count
        n, n_ref = fc.n, fc.n_ref
        rng = np.random.default_rng(31 + n_ref + (0 if count is None else 7 * count))
        sc = fc.scores()
        self.cand = rng.integers(0, n_ref, (n, 2)).astype(np.int64)
        self.cand_val = sc[self.cand, np.arange(n)[:, None]]
        if count is not None:
            self.flagged = rng.permutation(n)[:count].astype(np.int64)
            ai, av = argmax_ref(sc)
            k = np.arange(n) % 4                                  # pre-filled (conf, idx): below the maximum; equal with a larger index;
            self.conf0 = np.where(k == 0, -2.0 ** 100, np.where(k == 3, av + 1.0, av))              # equal with a smaller index; above
            self.idx0 = np.where(k == 0, -5, np.where(k == 1, ai + 3, np.where(k == 2, -1, 12345))).astype(np.int64)

    @functools.lru_cache(maxsize=None)
    def _classes(self):
        hh = scores64(self.fc.ref_hi, self.fc.lr_hi) if self.fc.name.split()[2] == 'lo' else None
        return exact_classes(self.fc.scores(), hh)

    def classes(self, p):
        return self._classes()[p]

    def want(self, model=None):
        """(idx, conf, flagged set)."""
        sc = self.fc.scores(model if model in ('ah.bl dropped', 'al.bh dropped') else None)
        if self.count is None:
            ai, av = argmax_ref(sc, model)
            return ai, av, np.arange(self.fc.n)
        idx, conf = exact_ref(sc, self.flagged, self.conf0, self.idx0, model)
        return idx, conf, np.sort(self.flagged)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    if name.startswith('E all '):
        return ExactCase(name, feat_case_E(name[6:]))
    feat, count = name[7:].rsplit(' count=', 1)
    fc = feat_case_E(feat)
    return ExactCase(name, fc, fc.n if count == 'all' else int(count))


# ---- family P ------------------------------------------------------------------------------------------------------------------------
P_SIZES = (((4, 7), (7, 4)), ((10, 13), (7, 10)), ((16, 25), (10, 13)))
P_NAMES = tuple('P %dx%d/%dx%d kernel=%d' % (a + b + (m,)) for a, b in P_SIZES for m in (0, 1))
P_VECTORS = ((1,) * 4 + (0,) * 12, (2,) + (0,) * 15, (1,) * 16, (3, 2, 1, 1, 1) + (0,) * 11, (2,) * 16, (6, 4, 2, 2, 2) + (0,) * 11,
             (4,) * 4 + (0,) * 12)                                # squared sums 4, 4, 16, 16, 64, 64, 64


def lattice_map(rng, h, w):
    """Energy only on the pixels with y % 3 == 0 and x % 3 == 0 of an h = w = 1 (mod 3) map: with reflect padding every 3x3 window holds
    exactly one of them, so its sum of squares is that pixel's -- 4, 16 or 64."""
    assert h % 3 == 1 and w % 3 == 1
    f = np.zeros((16, h, w), F64)
    for y in range(0, h, 3):
        for x in range(0, w, 3):
            v = np.asarray(P_VECTORS[rng.integers(0, len(P_VECTORS))], F64)
            f[:, y, x] = rng.permutation(v) * rng.choice([-1.0, 1.0], 16)
    return f + 0.0                                                # (no -0)


def window_sums(feat):
    return (unfold(feat) ** 2).sum(1)


@functools.lru_cache(maxsize=None)
def patch_case(name):
    shape = tuple(int(v) for v in name.split()[1].replace('/', 'x').split('x'))
    rng = np.random.default_rng(600 + sum(shape))
    lf, rf = lattice_map(rng, shape[0], shape[1]), lattice_map(rng, shape[2], shape[3])
    fc = FeatCase(name, lf, rf, 1.0 / np.sqrt(window_sums(lf)), 1.0 / np.sqrt(window_sums(rf)))
    fc.mode = int(name[-1])
    return fc


def patch_want(fc, margin):
    """Chain top-2 (one split) -> refine -> exact at `margin` (the float32 default): (cand_idx, cand_val, idx, conf, flagged set).  The
    scores are multiples of 2^-6, the margin is far below that: best - m2 >= margin decides as in float64."""
    sc = fc.scores()
    ci, cv = top2_ref(sc, fc.n_ref, 1)
    idx, val, fl = refine_ref(sc, ci, cv, margin)
    ai, av = argmax_ref(sc)
    return ci, cv, np.where(fl, ai, idx), np.where(fl, av, val), np.flatnonzero(fl)
