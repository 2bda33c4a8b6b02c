"""CPU side of the matching kernels' exact-arithmetic suite (tests/match_cases.py; the kernels run in tests/test_gpu_match_exact.py):

  * every case meets the exactness condition, and its float32 evaluation in two summation orders equals the float64 one bit for bit;
  * every listed column class is populated;
  * every control (a wrong model applied to the reference) changes the expected output of at least one case -- of a case built for
    the term or edge the control names;
  * the P construction's window sums are powers of 4; the host unfold is the oracle's patches3x3.

Run with -s for the tables.  Cases: T and G 20 size pairs each (35 launches each with their row splits); R 52; E 13 exhaustive + 20
crafted flagged lists; P 6.  Populations:
  T  every class of match_cases.T_CLASSES over the 20 x 144 column types; the rarest: all equal, zero 20; ascending / descending
     staircase 20 each; two-way tie in partner lanes, high half first 28; late value equal to the partner lane's runner-up 30;
     max at the first row of a stage 39; each of the 32 tile rows > 40.
  R  every candidate-list kind of match_cases.R_KINDS in the plain and in the flagged cases (>= 100 columns each); "best - m2 ==
     margin" at margin 0 and 2^-12 (121 columns), "close pair, opposite perturbations" at 2^-12 (87).
  E  every class of match_cases.E_CLASSES: each of the 64 stage rows (>= 26 columns), ties inside a 16-row tile 117, across tiles
     153, across stages 124, all-negative columns 1137, mixed-sign 3598, columns the hi-only score misranks 762.
Controls (test_every_control_changes_a_case_built_for_it prints "control: changes N columns in case X" with N >= 1 for each): since
the GPU suite compares every column with the unmodified reference, a kernel behaving like any control fails that case there."""
from collections import Counter

import numpy as np
import pytest
import torch

import match_cases as mc


def all_cases():
    for n in mc.TOP2_NAMES:
        yield mc.top2_case(n)
    for shape in mc.R_SHAPES:
        yield mc.feat_case_R(shape)
    for f in mc.E_FEATS:
        yield mc.feat_case_E(f)
    for n in mc.P_NAMES[::2]:
        yield mc.patch_case(n)


CASE_NAMES = [c.name for c in all_cases()]


def case_by_name(name):
    return next(c for c in all_cases() if c.name == name)


def test_constants_are_the_library_s():
    from refvsr_amd import hip
    assert (mc.KP, mc.ROWCHUNK, mc.COLBLOCK) == (hip.MATCH_KP, hip.MATCH_ROWCHUNK, hip.MATCH_COLBLOCK)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_case_is_exact_in_float32(name):
    """The exactness condition, and what it promises: two float32 evaluations in different orders return the float64 scores."""
    c = case_by_name(name)
    for A, B in c.operands():
        bound = mc.exactness(A, B)
        assert bound < 24, '%s: sum |a b| / g = 2^%.2f' % (name, bound)
        for v in (A, B):
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
        want = mc.scores64(A, B)
        for order in (0, 1):
            got = mc.scores32(A, B, order)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (name, order)
    if isinstance(c, mc.FeatCase):                                # the scaled scores and the three-term sum of the split rows
        sc = c.scores()
        assert np.array_equal(sc.astype(np.float32).astype(np.float64), sc)
        three = (mc.scores64(c.ref_hi, c.lr_hi) + (mc.scores64(c.ref_hi, c.lr_lo) + mc.scores64(c.ref_lo, c.lr_hi)) / mc.LO_SCALE)
        assert np.array_equal(three, sc), 'hi + lo rows do not reproduce the dot product'
        assert not (mc.scores64(np.abs(c.ref_lo), np.abs(c.lr_lo))).any(), 'a b b\' product is not zero'
        for r in c.rows():
            assert r.dtype == np.float16 and r.shape[1] == mc.KP and not r[:, mc.K:].any()
    else:
        ref_rows, lr_rows = c.rows()
        assert ref_rows.shape[0] % mc.ROWCHUNK == 0 and lr_rows.shape[0] % mc.COLBLOCK == 0
        assert not ref_rows[c.n_ref:].any() and not lr_rows[c.n_lr:].any() and not ref_rows[:, mc.K:].any()


def test_top2_classes_are_populated():
    cnt, per_family = Counter(), Counter()
    for n in mc.TOP2_NAMES:
        c = mc.top2_case(n)
        per_family[c.family] += len(c.splits())
        if c.family == 'T':
            assert np.array_equal(c.scores(), c.ref[:, np.arange(c.n_lr) % mc.K])       # the row matrix IS the score table
            for t in range(mc.K):
                cnt.update(c.type_classes(t))
    print('\nfamily T: %d launches, family G: %d launches over %d size pairs' % (per_family['T'], per_family['G'], len(mc.SIZES)))
    for k in mc.T_CLASSES:
        print('  T %-55s %5d column types' % (k, cnt[k]))
        assert cnt[k] > 0, k
    g = mc.top2_case('G 777 x 1100')
    assert set(np.unique(g.ref)) == set(range(-3, 4)) and (g.ref != 0).all(0).sum() == 0 and (g.lr != 0).any(0).all()


def test_top2_sizes_cover_the_cross_and_the_split_rule():
    assert {a for a, _ in mc.SIZES} == {2, 3, 255, 256, 257, 512, 513, 777}
    assert {b for _, b in mc.SIZES} == {1, 31, 33, 64, 511, 512, 513, 1100}
    assert len(mc.SIZES) == 20
    used = {(a, s) for a, _ in mc.SIZES for s in (1, 2, 3) if mc.split_ranges(a, s)}
    assert {s for _, s in used} == {1, 2, 3} and (513, 3) in used and (777, 2) in used and (257, 2) in used
    for n_ref, s in mc.REJECTED:
        assert mc.split_ranges(n_ref, s) is None
    # a split range with one real row exists exactly where the issue says: one row past a stage boundary
    single = {a for a, _ in mc.SIZES for s in (1, 2, 3) if mc.split_ranges(a, s) and any(mc.top2_case('T %d x %d' % (a, [b for x, b in mc.SIZES if x == a][0])).single_row_ranges(s))}
    assert single == {257, 513}


def test_refine_kinds_are_populated():
    plain, flagged = Counter(), Counter()
    for n in mc.R_NAMES:
        c = mc.refine_case(n)
        assert c.fc.n % 128 != 0
        (plain if c.margin is None else flagged).update(c.kinds)
        if c.margin is not None:
            flagged.update('%s @ %s' % (k, n.split()[-1]) for k in c.kinds)
            idx, val, fl = c.want()
            assert fl is not None
        plain.update(['below 0'] * int((c.cand < 0).sum()) + ['at or beyond n_ref'] * int((c.cand >= c.fc.n_ref).sum()))
    print('\nfamily R: %d cases' % len(mc.R_NAMES))
    for k in mc.R_KINDS:
        print('  R %-45s plain %4d  flagged %4d columns' % (k, plain[k], flagged[k]))
    assert plain['below 0'] > 0 and plain['at or beyond n_ref'] > 0
    for k in mc.R_KINDS[:4]:
        assert plain[k] > 0 and flagged[k] > 0
    for k in mc.R_KINDS[4:6]:
        assert plain[k] > 0 and flagged[k] > 0, k
    assert flagged['best - m2 == margin @ margin=0'] > 0 and flagged['best - m2 == margin @ margin=2^-12'] > 0
    assert flagged['close pair, opposite perturbations @ margin=2^-12'] > 0
    # columns where best - m2 == margin exactly are NOT flagged; at margin = inf every column is
    for n in mc.R_NAMES:
        c = mc.refine_case(n)
        if c.margin is None:
            continue
        _, val, fl = mc.refine_ref(c.fc.scores(), c.cand, c.cand_val, c.margin)
        eq = np.array([k == 'best - m2 == margin' for k in c.kinds])
        if eq.any():
            assert np.array_equal(val[eq] - c.cand_val[eq, 1::2].max(1), np.full(int(eq.sum()), c.margin)) and not fl[eq].any()
        if np.isinf(c.margin):
            assert fl.all()
    # every pixel of the edge and corner of both maps takes part: the maps are smaller than or equal to 13 x 15, every pixel is a column
    assert all(min(s) >= 2 for s in mc.R_SHAPES)


def test_exact_classes_and_counts_are_populated():
    cnt = Counter()
    for n in mc.E_ALL_NAMES:
        c = mc.exact_case(n)
        for p in range(c.fc.n):
            cnt.update(c.classes(p))
    print('\nfamily E: %d exhaustive cases, %d crafted flagged lists' % (len(mc.E_ALL_NAMES), len(mc.E_LIST_NAMES)))
    for k in mc.E_CLASSES:
        print('  E %-40s %5d columns' % (k, cnt[k]))
        assert cnt[k] > 0, k
    counts = {mc.exact_case(n).count for n in mc.E_LIST_NAMES}
    assert counts == {0, 1, 255, 256, 257, mc.E_LR[0] * mc.E_LR[1]}
    assert {mc.exact_case(n).fc.n_ref for n in mc.E_ALL_NAMES} == {4, 63, 64, 65, 129, 777}
    for n in mc.E_LIST_NAMES:
        c = mc.exact_case(n)
        if c.count > 1:
            assert len(set(c.flagged)) == c.count and (np.diff(c.flagged) < 0).any()            # distinct, unsorted
        idx, conf, _ = c.want()
        un = np.ones(c.fc.n, bool)
        un[c.flagged] = False
        assert np.array_equal(idx[un], c.idx0[un]) and np.array_equal(conf[un], c.conf0[un])
        if c.count >= 255:                                        # all four pre-fill outcomes occur: replaced (lower, larger index), kept (smaller index, higher)
            ch = (idx != c.idx0)[c.flagged]
            k = (c.flagged % 4)
            assert ch[k == 0].all() and ch[k == 1].all() and not ch[k == 2].any() and not ch[k == 3].any()


def test_lo_cases_are_decided_by_the_lo_terms():
    for f in mc.E_FEATS:
        if ' lo ' not in ' ' + f:
            continue
        fc = mc.feat_case_E(f)
        assert fc.lr_lo.any() and fc.ref_lo.any()
        b_l = (fc.L - np.round(fc.L)) * 2.0 ** 13
        b_r = (fc.R - np.round(fc.R)) * 2.0 ** 13
        assert np.array_equal(b_l, np.round(b_l)) and np.abs(b_l).max() == 3 and (np.round(fc.L) != 0).all()
        assert not (np.abs(b_r) @ np.abs(b_l).T).any()            # every b b' product is zero
        slots = np.arange(mc.K) // 9 % 2
        assert not b_l[:, slots == 1].any() and not b_r[:, slots == 0].any()
        for a, b in ((0, 32), (32, 64), (64, 96), (96, 128), (128, 144)):          # every K step of the search's MFMAs holds slots of both sides
            assert len(set(slots[a:b])) == 2


def test_patch_windows_are_powers_of_four():
    for n in mc.P_NAMES:
        fc = mc.patch_case(n)
        for f, inv in ((fc.lf, fc.il), (fc.rf, fc.ir)):
            ss = mc.window_sums(f)
            assert set(np.unique(ss)) <= {4.0, 16.0, 64.0} and len(np.unique(ss)) >= 2
            assert set(np.unique(inv)) <= {0.5, 0.25, 0.125}
            assert np.array_equal(np.sqrt(ss.astype(np.float32)).astype(np.float64) ** 2, ss)
        assert not fc.lr_lo.any() and not fc.ref_lo.any()
        assert fc.n % 128 != 0 and fc.n % 256 != 0
        ci, cv, idx, conf, fl = mc.patch_want(fc, float(np.float32(2.5e-4)))
        assert 0 < len(fl) < fc.n                                 # the default margin sends some columns to the search and keeps others


def test_host_unfold_is_the_oracle_s():
    from oracle import refvsr_oracle as orc
    rng = np.random.default_rng(3)
    for h, w in ((2, 2), (3, 5), (9, 15)):
        f = rng.integers(-3, 4, (16, h, w)).astype(np.float64)
        want = orc.patches3x3(torch.from_numpy(f)[None])[0].t().numpy()
        assert np.array_equal(mc.unfold(f), want)


# ---- controls -------------------------------------------------------------------------------------------------------------------------
def changed_top2(c, model):
    n = 0
    for s in c.splits():
        (i0, v0), (i1, v1) = c.want(s), c.want(s, model)
        n += int(((i0 != i1) | (v0 != v1)).any(1).sum())
    return n


def changed_tuple(a, b):
    (i0, v0, f0), (i1, v1, f1) = a, b
    n = int(((i0 != i1) | (v0 != v1)).sum())
    if f0 is not None and not np.array_equal(f0, f1):
        n += len(set(f0) ^ set(f1))
    return n


def built_for(control, c, p):
    """Is column p of case c one the control's term or edge was built into?"""
    cl = ' | '.join(c.classes(p))
    return {'last of equals': 'tie' in cl or 'all equal' in cl, 'pad rows not masked': 'pad rows, negative scores' in cl,
            'merge prefers partner lane': 'partner lanes' in cl and 'tie' in cl, 'last real row masked': 'max at row n_ref - 1' in cl,
            'first pad row admitted': 'pad rows, negative scores' in cl or 'all-negative' in cl}.get(control, True)


TOP2_CONTROLS = ('last of equals', 'pad rows not masked', 'one lane half only', 'merge prefers partner lane', 'last real row masked',
                 'first pad row admitted')


@pytest.mark.parametrize('control', mc.CONTROLS)
def test_every_control_changes_a_case_built_for_it(control):
    lines, built = [], 1
    if control in TOP2_CONTROLS:
        for name in ('T 257 x 1100', 'T 513 x 1100', 'T 777 x 1100', 'T 255 x 512', 'G 777 x 513'):
            c = mc.top2_case(name)
            n = changed_top2(c, control)
            lines.append((n, name))
            if c.family == 'T' and n:                             # ... and in a column built for it
                s = c.splits()[-1]
                (i0, v0), (i1, v1) = c.want(s), c.want(s, control)
                cols = np.flatnonzero(((i0 != i1) | (v0 != v1)).any(1))
                assert any(built_for(control, c, p) for p in cols), (control, name)
        if control in ('last of equals', 'last real row masked', 'first pad row admitted'):
            for name in ('E all ties n_ref=777', 'E all negative n_ref=129', 'E all int n_ref=65'):
                c = mc.exact_case(name)
                lines.append((changed_tuple(c.want(), c.want(control)), name))
    elif control in ('skip rule 1 x margin', 'flag with >'):
        built = 0
        for name in mc.R_NAMES:
            c = mc.refine_case(name)
            if c.margin is not None:
                n = changed_tuple(c.want(), c.want(control))
                if n:
                    lines.append((n, name))
                    ch = np.flatnonzero((c.want()[0] != c.want(control)[0]) | np.isin(np.arange(c.fc.n), np.setxor1d(c.want()[2], c.want(control)[2])))
                    want_kind = 'close pair, opposite perturbations' if control.startswith('skip') else 'best - m2 == margin'
                    built += sum(c.kinds[p] == want_kind for p in ch)
    else:
        for name in mc.E_ALL_NAMES + mc.E_LIST_NAMES:
            if ' lo ' in name:
                c = mc.exact_case(name)
                lines.append((changed_tuple(c.want(), c.want(control)), name))
    print()
    for n, name in lines:
        print('%s: changes %d columns in case %s' % (control, n, name))
    assert lines and max(n for n, _ in lines) >= 1
    assert built >= 1, 'no changed column is of the kind built for this control'
    if control in TOP2_CONTROLS:
        assert lines[2][0] >= 1                                   # the full-size T case catches every top-2 control
    if control in ('ah.bl dropped', 'al.bh dropped'):
        assert all(n >= 1 for n, name in lines if 'count=1' not in name and 'count=0' not in name)
