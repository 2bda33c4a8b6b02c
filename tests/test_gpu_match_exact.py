"""Exact-arithmetic contract of the matching kernels on a real MI355X: every case of tests/match_cases.py is fed to its kernel(s) and
the result must equal the float64 reference BIT FOR BIT -- cand_val of every column and every row split, cand_idx wherever the value
is finite, conf, idx and the flagged set -- with the first of equal values winning, like torch.max.  Every input tensor must be
unchanged after the call.  No tolerance, no excluded column.

The inputs are chosen (and proved on the CPU, tests/test_match_cases.py) so that every partial sum a kernel can form is an fp32
number: the streaming order of match_top2, the MFMA shapes, the three-term hi + lo sum of match_exact and patch_dot's fmaf chain
cannot change a score.  What can: a masked or admitted row at a stage boundary, a prune gate that drops a value it must keep, a merge
that prefers the wrong lane on equality, a dropped al.bh / ah.bl fragment, a skip or flag rule off by a factor or a `=`.  Each of
these is a control of match_cases.py that changes the reference on at least one case here, so a kernel behaving like it fails.

A failing case reports the class of its first mismatching column (e.g. "two-way tie: partner lanes, high half first").
On the MI355X: 0 mismatches in every case (profiles/gpu_match_exact_report.txt)."""
import os
import time

import numpy as np
import pytest
import torch

import footprint as fp
import match_cases as mc
from test_gpu_ops import REPORT as OPS_REPORT

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(OPS_REPORT), 'gpu_match_exact_report.txt')     # next to the other GPU reports
T0 = []


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
    T0.append(time.perf_counter())
    return torch.device('cuda:0')


class Inputs(object):
    """Device copies of a case's inputs; unchanged() proves that no kernel wrote to one of them.  fenced: every copy is a view
    between the fences of footprint.fenced_input: NaN around rows, low rows, features and inverse norms, zeros ('benign') around what
    a kernel turns into an address -- candidate tables, their values, flag lists."""

    def __init__(self, dev, fenced=False):
        self.dev, self.kept, self.fenced = dev, [], fenced
        if fenced:
            fp.reset_inputs()

    def _keep(self, t):
        self.kept.append((t, t.clone()))
        return t

    def _put(self, t, poison):
        return fp.fenced_input(t, self.dev, poison) if self.fenced else t.to(self.dev)

    def f16(self, a, poison='nan'):
        assert a.dtype == np.float16
        return self._keep(self._put(torch.from_numpy(np.ascontiguousarray(a)), poison))

    def f32(self, a, poison='nan'):
        t = torch.from_numpy(np.ascontiguousarray(a))
        assert torch.equal(t.float().double(), t), 'input is not fp32-representable'
        return self._keep(self._put(t.float(), poison))

    def i32(self, a, poison='benign'):
        assert np.abs(a).max() < 2 ** 31
        return self._keep(self._put(torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32), poison))

    def unchanged(self):
        torch.cuda.synchronize()
        for t, t0 in self.kept:
            assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8)), 'an input tensor was written to'
        if self.fenced:
            assert fp.inputs_unchanged() is None, fp.inputs_unchanged()
            fp.reset_inputs()


def fenced_verdict(label, fo, results, plain, flagged=None):
    """The fenced second run's assertions: every fence intact and every result fenced, the raw results equal to the plain run's, no
    NaN (footprint.judge); one report line.  flagged = (fenced run's, plain run's) flag list: fenced like the others, compared as
    the set it is (its order is the order the columns were flagged in)."""
    bad = fp.judge(fo, results, plain)
    if flagged is not None:
        bad = '\n'.join(b for b in (bad, '\n'.join(fo.problems([flagged[0]])),
                                    '' if np.array_equal(flagged_set(flagged[0]), flagged_set(flagged[1])) else 'the flagged set differs from the plain run') if b)
    report('%-52s fenced run: fences=%s equal=%s' % (label, 'BROKEN' if bad else 'ok', 'NO' if 'differs' in bad else 'ok'))
    assert not bad, '%s, fenced run: %s' % (label, bad)


def bits32(a):
    """float values -> their fp32 bit patterns (the reference's float64 numbers are fp32 numbers; -0 is not among them)."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        a32 = (a + 0.0).astype(np.float32)
        assert np.array_equal(a32.astype(np.float64), a)
        a = a32
    return np.ascontiguousarray(a).view(np.int32)


def check(c, items, label=None):
    """items: (what, bad [n] or [n, k] bool, got, want).  One report line per case: mismatch count and the first mismatching
    (what, column, entry, got, want) with the column's class; asserts that there is none."""
    total, first = 0, ''
    for what, bad, got, want in items:
        bad = np.asarray(bad)
        bad = bad.reshape(bad.shape[0], -1)
        total += int(bad.sum())
        if bad.any() and not first:
            p, k = (int(v) for v in np.argwhere(bad)[0])
            g, w = np.asarray(got).reshape(bad.shape[0], -1), np.asarray(want).reshape(bad.shape[0], -1)
            first = ' first: %s column %d split %d entry %d got %r want %r class [%s]' % (what, p, k // 2, k % 2, g[p, k].item(), w[p, k].item(),
                                                                                      ' | '.join(c.classes(p)))
    label = label or c.name
    report('%-52s mismatches=%d%s  (file wall time %.1f s)' % (label, total, first, time.perf_counter() - T0[0]))
    assert total == 0, '%s:%s' % (label, first)


def flagged_set(fl):
    fl = fl.cpu().numpy().astype(np.int64)
    got = np.sort(fl[1:1 + fl[0]])
    assert len(np.unique(got)) == len(got), 'a column is flagged twice'
    return got


def set_items(n, got, want):
    g, w = np.zeros(n, bool), np.zeros(n, bool)
    g[got], w[want] = True, True
    return ('flagged', g != w, g, w)


# ---- T, G: match_top2 ---------------------------------------------------------------------------------------------------------------
TOP2 = [(n, s) for n in mc.TOP2_NAMES for s in (1, 2, 3) if mc.split_ranges(int(n.split()[1]), s)]


@pytest.mark.parametrize('name,splits', TOP2)
def test_top2_returns_the_reference_candidates(dev, name, splits):
    from refvsr_amd import ops
    c = mc.top2_case(name)
    inp = Inputs(dev)
    ref_rows, lr_rows = (inp.f16(r) for r in c.rows())
    ci, cv = ops.match_top2(ref_rows, c.n_ref, lr_rows, c.n_lr, splits)
    inp.unchanged()
    inp2 = Inputs(dev, True)
    ref_rows2, lr_rows2 = (inp2.f16(r) for r in c.rows())
    with fp.fenced_outputs(ops) as fo:
        got2 = ops.match_top2(ref_rows2, c.n_ref, lr_rows2, c.n_lr, splits)
        fenced_verdict('%s splits=%d' % (name, splits), fo, got2, (ci, cv))
    inp2.unchanged()
    ci, cv = ci.cpu().numpy().astype(np.int64), cv.cpu().numpy()
    wi, wv = c.want(splits)
    assert ci.shape == wi.shape == (c.n_lr, 2 * splits)
    finite = np.isfinite(wv)
    # a -inf entry exists only as the second entry of a split range that holds a single real row (n_ref = 257, 513)
    allowed = np.zeros(2 * splits, bool)
    allowed[1::2] = c.single_row_ranges(splits)
    assert not (~finite & ~allowed[None, :]).any()
    bad_i = np.where(finite, ci != wi, (ci < 0) | (ci >= c.n_ref))
    check(c, [('cand_val', bits32(cv) != bits32(wv), cv, wv), ('cand_idx', bad_i, ci, wi)], '%s splits=%d' % (name, splits))


@pytest.mark.parametrize('n_ref,splits', mc.REJECTED)
def test_top2_refuses_an_empty_row_split(dev, n_ref, splits):
    from refvsr_amd import ops
    ref_rows = torch.zeros(mc.round_up(n_ref, mc.ROWCHUNK), mc.KP, dtype=torch.float16, device=dev)
    lr_rows = torch.zeros(mc.COLBLOCK, mc.KP, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match='match_top2'):
        ops.match_top2(ref_rows, n_ref, lr_rows, 64, splits)


# ---- R, E: match_refine and match_exact -----------------------------------------------------------------------------------------------
def feat_inputs(inp, fc):
    lr_hi, lr_lo, ref_hi, ref_lo = (inp.f16(r) for r in fc.rows())
    return dict(lf=inp.f32(fc.lf), rf=inp.f32(fc.rf), il=inp.f32(fc.il), ir=inp.f32(fc.ir), lr_hi=lr_hi, lr_lo=lr_lo, ref_hi=ref_hi,
                ref_lo=ref_lo)


def _refine(dev, fc, cand, cand_val, margin, sparse_lo, fenced):
    """One ops.match_refine call on host-built rows -> (conf, idx[, flagged]) as returned; the inputs must come back unchanged."""
    from refvsr_amd import ops
    inp = Inputs(dev, fenced)
    t = feat_inputs(inp, fc)
    cand = inp.i32(cand)
    if margin is None:
        got = ops.match_refine(t['lf'], t['rf'], t['il'], t['ir'], cand)
    else:
        got = ops.match_refine(t['lf'], t['rf'], t['il'], t['ir'], cand, inp.f32(cand_val, 'benign'), float(margin),
                               (t['lr_hi'], None if sparse_lo else t['lr_lo']), (t['ref_hi'], t['ref_lo']))
    inp.unchanged()
    return got


def run_refine(dev, c, fc, cand, cand_val, margin, sparse_lo=False):
    """ops.match_refine on host-built rows -> (idx, conf, flagged set or None) as numpy; the inputs must come back unchanged.  Then
    the fenced second run of the same call (its zeroed scratch and, with sparse_lo, the low rows it writes are fenced allocations)."""
    from refvsr_amd import ops
    got = _refine(dev, fc, cand, cand_val, margin, sparse_lo, False)
    with fp.fenced_outputs(ops) as fo:
        got2 = _refine(dev, fc, cand, cand_val, margin, sparse_lo, True)
        fenced_verdict('%s margin=%s lr_lo=%s' % (c.name, margin, 'None' if sparse_lo else 'dense'), fo, got2[:2], got[:2],
                       (got2[2], got[2]) if len(got) == 3 else None)
    conf, idx, fl = got if len(got) == 3 else (got[0], got[1], None)
    return idx.cpu().numpy().astype(np.int64), conf.cpu().numpy(), None if fl is None else flagged_set(fl)


def result_items(n, got, want):
    (gi, gc, gf), (wi, wc, wf) = got, want
    items = [('conf', bits32(gc) != bits32(wc), gc, wc), ('idx', gi != wi, gi, wi)]
    if wf is not None:
        items.append(set_items(n, gf, wf))
    return items


@pytest.mark.parametrize('name', mc.R_NAMES)
def test_refine_returns_the_best_listed_candidate_and_the_flagged_set(dev, name):
    c = mc.refine_case(name)
    got = run_refine(dev, c, c.fc, c.cand, c.cand_val, c.margin)
    check(c, result_items(c.fc.n, got, c.want()))


@pytest.mark.parametrize('name', mc.E_ALL_NAMES)
def test_exact_search_of_every_column(dev, name):
    """margin = inf: every column goes to refvsr_match_exact; with a dense lr_lo and with lr_lo = None (refvsr_match_lo_rows writes the
    flagged columns' low halves) -- both must return the reference, hence equal bits."""
    c = mc.exact_case(name)
    want = c.want()
    for sparse in (False, True):
        got = run_refine(dev, c, c.fc, c.cand, c.cand_val, np.inf, sparse)
        check(c, result_items(c.fc.n, got, want), '%s lr_lo=%s' % (name, 'None' if sparse else 'dense'))


@pytest.mark.parametrize('name', mc.E_LIST_NAMES)
def test_exact_search_of_a_crafted_flagged_list(dev, name):
    """refvsr_match_exact through the library: an unsorted flagged list, pre-filled conf / idx.  Flagged columns take the first arg-max
    where it beats the pre-filled pair, every other column keeps its bits."""
    from refvsr_amd import hip, ops
    c = mc.exact_case(name)
    fc = c.fc
    fl0 = np.zeros(fc.n + 1, np.int64)
    fl0[0] = c.count
    fl0[1:1 + c.count] = c.flagged
    assert fl0[1:].max() < fc.n and fl0.min() >= 0
    conf0 = torch.from_numpy(c.conf0)
    assert torch.equal(conf0.float().double(), conf0)

    def go(fenced):
        """the call on plain tensors, or on fenced inputs and hand-marked keys / conf / idx (the buffers the kernel reads and writes)"""
        inp = Inputs(dev, fenced)
        t = feat_inputs(inp, fc)
        fl = inp.i32(fl0)
        bufs = [torch.zeros(fc.n, dtype=torch.int64), conf0.float(), torch.from_numpy(c.idx0).to(torch.int32)]
        recs = [fp.marked_buffer(b, dev) for b in bufs] if fenced else []
        keys, conf, idx = [r.view for r in recs] if fenced else [b.to(dev) for b in bufs]
        p = ops._ptr
        hip.check(hip.lib().refvsr_match_exact(p(t['lf']), fc.h, fc.w, p(t['rf']), fc.hr, fc.wr, p(t['lr_hi']), p(t['lr_lo']), p(t['ref_hi']),
                                               p(t['ref_lo']), p(t['il']), p(t['ir']), p(fl), p(keys), p(conf), p(idx), ops._stream()),
                  'match_exact')
        inp.unchanged()
        for r in recs:
            assert not r.damage(), 'written outside %s %s: %s' % (tuple(r.view.shape), r.view.dtype, r.damage())
        return conf, idx

    conf, idx = go(False)
    conf2, idx2 = go(True)
    assert torch.equal(conf2, conf) and torch.equal(idx2, idx) and not torch.isnan(conf2).any(), 'the fenced run does not equal the plain run'
    report('%-52s fenced run: fences=ok equal=ok' % name)
    wi, wc, _ = c.want()
    check(c, [('conf', bits32(conf.cpu().numpy()) != bits32(wc), conf.cpu().numpy(), wc),
              ('idx', idx.cpu().numpy().astype(np.int64) != wi, idx.cpu().numpy(), wi)])


# ---- P: match_patches end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mc.P_NAMES)
def test_patches_rows_norms_and_the_whole_chain(dev, name):
    from refvsr_amd import ops
    fc = mc.patch_case(name)
    inp = Inputs(dev)
    lf, rf = inp.f32(fc.lf), inp.f32(fc.rf)
    ops.set_match_patches_kernel(fc.mode)
    try:
        lr_rows, inv_lr, lr_lo = ops.match_patches(lf, mc.COLBLOCK, want_lo=True)
        ref_rows, inv_ref, ref_lo = ops.match_patches(rf, mc.ROWCHUNK, want_lo=True)
        torch.cuda.synchronize()
    finally:
        ops.set_match_patches_kernel(1)
    items = []
    for what, got, want in (('lr rows', lr_rows, mc.rows16(fc.lr_hi, mc.COLBLOCK)), ('lr rows_lo', lr_lo, mc.rows16(fc.lr_lo, mc.COLBLOCK)),
                            ('ref rows', ref_rows, mc.rows16(fc.ref_hi, mc.ROWCHUNK)), ('ref rows_lo', ref_lo, mc.rows16(fc.ref_lo, mc.ROWCHUNK))):
        got = got.cpu().numpy()
        assert got.shape == want.shape
        items.append((what, got.view(np.int16) != want.view(np.int16), got, want))              # pad rows and pad slots: zero bits
    for what, got, want in (('inv_lr', inv_lr, fc.il), ('inv_ref', inv_ref, fc.ir)):
        items.append((what, bits32(got.cpu().numpy()) != bits32(want), got.cpu().numpy(), want))
    kept = Inputs(dev)
    for t in (lr_rows, lr_lo, ref_rows, ref_lo, inv_lr, inv_ref):
        kept._keep(t)
    cand, cval = ops.match_top2(ref_rows, fc.n_ref, lr_rows, fc.n, 1)
    conf, idx, fl = ops.match_refine(lf, rf, inv_lr, inv_ref, cand, cval, ops.MATCH_EXACT_MARGIN, (lr_rows, lr_lo), (ref_rows, ref_lo))
    inp.unchanged()
    kept.unchanged()
    # the fenced second run of the whole chain: NaN around the feature maps; rows, low rows and norms are fenced allocations of ops
    # whose fences begin behind the last pad row; want_lo on and off
    inp2 = Inputs(dev, True)
    lf2, rf2 = inp2.f32(fc.lf), inp2.f32(fc.rf)
    with fp.fenced_outputs(ops) as fo:
        ops.set_match_patches_kernel(fc.mode)
        try:
            pl = ops.match_patches(lf2, mc.COLBLOCK, want_lo=True)
            pr = ops.match_patches(rf2, mc.ROWCHUNK, want_lo=True)
            pl0 = ops.match_patches(lf2, mc.COLBLOCK)
            pr0 = ops.match_patches(rf2, mc.ROWCHUNK)
            torch.cuda.synchronize()
        finally:
            ops.set_match_patches_kernel(1)
        assert len(pl0) == len(pr0) == 2
        t2 = ops.match_top2(pr[0], fc.n_ref, pl[0], fc.n, 1)
        r2 = ops.match_refine(lf2, rf2, pl[1], pr[1], t2[0], t2[1], ops.MATCH_EXACT_MARGIN, (pl[0], pl[2]), (pr[0], pr[2]))
        fenced_verdict(name, fo, [pl, pr, pl0, pr0, t2, r2[:2]],
                       [(lr_rows, inv_lr, lr_lo), (ref_rows, inv_ref, ref_lo), (lr_rows, inv_lr), (ref_rows, inv_ref), (cand, cval), (conf, idx)], (r2[2], fl))
    inp2.unchanged()
    wci, wcv, wi, wc, wf = mc.patch_want(fc, float(np.float32(ops.MATCH_EXACT_MARGIN)))
    cand, cval = cand.cpu().numpy().astype(np.int64), cval.cpu().numpy()
    items += [('cand_val', bits32(cval) != bits32(wcv), cval, wcv), ('cand_idx', cand != wci, cand, wci)]
    items += result_items(fc.n, (idx.cpu().numpy().astype(np.int64), conf.cpu().numpy(), flagged_set(fl)), (wi, wc, wf))
    check(fc, items)
