"""CPU side of the exact-arithmetic parity tests (tests/exact_cases.py, tests/test_gpu_exact.py): for every case the GPU file runs,
  * the exactness condition holds (fewer than 2^24 granules at every stage of every conv) and the controls show that the case
    would see a missing lo term: (a) all lo terms dropped >= 5 % of the outputs, (b) one K-block's lo term >= 1 % and >= 8 outputs;
  * a float32 evaluation -- F.conv2d with hi and with lo, added -- equals the float64 reference exactly (the empirical side of the
    exactness argument: float32 sums in MKL-DNN's order lose nothing either);
  * for the head cases with a non-zero base frame: the base's bicubic sample is exact (float32 = float64, either summation order, on
    the 2^-24 grid), every class of sample and output occurs, every border and corner has a live output behind index-clamped taps,
    every deliberate defect of the base term changes the reference ("control X changes N outputs in case Y"), and the general
    family (bytes / 255) keeps its derived bound and its 1 % cap on the reference's own float32 replay;
  * the packers accept the weights and their fragments decode back to w exactly (hi + lo == w element by element, every K-block
    present once, padding zero) -- a packer that drops or misplaces one lo fragment fails here before any GPU is involved."""
import math

import pytest
import torch

import exact_cases as ec
from exact_cases import get_case


def test_table_is_sound():
    assert ec.PREMISE.startswith('premise') and len(set(ec.NAMES)) == len(ec.NAMES) > 100
    w = ec.dyadic_weights(ec.rng(1), 24, 24, 3)
    hi, lo = ec.split_hi_lo(w)
    sub = (lo != 0) & (lo.abs() < 2.0 ** -14)
    assert float(sub.double().sum() / (lo != 0).double().sum()) > 0.9, 'almost every lo value is an fp16 subnormal at |w| < 2^-3'
    assert ec.granule(w) == 2.0 ** -17 and ec.granule(torch.tensor([0.75, -2.0])) == 0.25
    with pytest.raises(AssertionError):
        ec.split_hi_lo(torch.tensor([0.1]).double())                            # fp32(0.1): 24 bits do not fit hi + lo


@pytest.mark.parametrize('name', ec.NAMES)
def test_case_is_exact_and_strong(name):
    c = get_case(name)
    print('%-52s %s' % (name, c.line()))
    c.assert_strong()
    if c.lo0:
        for k, v in c.p.items():
            if k in ('w', 'w1', 'w2'):
                assert not ec.split_hi_lo(v)[1].any()
        if c.lo0 == 'flush':
            full = [v for k, v in c.p.items() if k == 'w'] + [b[0] for b in c.p.get('blocks', [])]
            assert full and all(float(v.abs().max()) < 2.0 ** -14 for v in full), 'every hi value must be an fp16 subnormal'


@pytest.mark.parametrize('name', ec.NAMES)
def test_float32_emulation_equals_reference(name):
    c = get_case(name)
    if c.primary == 'hi':
        p32 = ec.REFS[c.kind](ec.Arith('f32'), _rounded(c))[0]
    else:
        p32 = c.evaluate('f32')[0]
    for k, v in c.want.items():
        assert p32[k].dtype in (torch.float32, torch.float64)
        assert torch.equal(p32[k].double(), v), '%s: float32 arithmetic is not exact on this case (%s)' % (name, k)


# ---- the output head with a non-zero base frame --------------------------------------------------------------------------------------
def _one_sample(c):
    return c.p['base'].shape[1] * c.p['base'].shape[2] == 1


@pytest.mark.parametrize('name', ec.BASED)
def test_based_case_base_is_exact_and_every_class_is_filled(name):
    """On the case's own data: the bicubic sample is the same number in float32 and float64, rows first and columns first, and lies
    on the 2^-24 grid (base_proof); samples below 0, above 1 and inside, outputs at 0, at 1 and inside, and outputs inside (0, 1)
    whose sample was clamped all occur (a 1 x 1 map returns its one sample: no overshoot there); v + b is exact in float64."""
    c = get_case(name)
    p = c.p
    assert p['base'].shape == (3, p['x'].shape[1] // p['s'], p['x'].shape[2] // p['s']) and p['s'] in (2, 4)
    assert all(float(v) in ec.BASE_SETS['u'] for v in p['base'].unique()) or all(float(v) in ec.BASE_SETS['s'] for v in p['base'].unique())
    assert not torch.equal(p['base'][0], p['base'][1]) and not torch.equal(p['base'][1], p['base'][2]) and not torch.equal(p['base'][0], p['base'][2])
    cl = ec.head_classes(c)
    print('%-40s samples <=0 / >=1 / inside %s  outputs 0 / 1 / inside %s  inside with a clamped sample %d' % (
        name, cl['samples'], cl['outputs'], cl['inside_clamped']))
    least = 1 if _one_sample(c) else 4
    assert min(cl['samples']) >= least and min(cl['outputs']) >= least, cl
    assert _one_sample(c) or cl['inside_clamped'] >= least, cl
    pre = c.evaluate('f64')[0]['out']
    assert torch.equal(pre.float().double(), pre) and torch.equal(c.evaluate('f32')[0]['out'].double(), pre)
    raw = ec.base_proof(p)
    assert float(raw.abs().max()) < 4.0 and c.bound < ec.LIMIT       # |v| < 2^24 g_v, |b| < 4 on the 2^-24 grid: v + b fits float64


@pytest.mark.parametrize('name', ec.BASED)
def test_based_case_borders_have_live_outputs(name):
    """On each of the four borders and four corners at least one output whose taps were index-clamped has a reference value strictly
    inside (0, 1): a wrong value read there changes it, and so does a fence's NaN that the clamps turn into 0."""
    c = get_case(name)
    n = ec.head_borders(c)
    print('%-40s %s' % (name, '  '.join('%s %d' % (k, n[k]) for k in ec.BORDERS)))
    assert set(n) == set(ec.BORDERS) and min(n.values()) >= 1, n


@pytest.mark.parametrize('name', ec.BASED)
def test_based_case_controls_change_the_reference(name):
    """Every deliberate defect of the base term (exact_cases.head_base), applied to the REFERENCE: a map with more than one sample
    must change under each of them, the 1 x 1 map (every tap on the one sample, weights summing to 1) under the wrong plane."""
    c = get_case(name)
    for ctl in ec.BASE_CONTROLS:
        n = ec.base_control(c, ctl)
        print('control %-8s changes %4d of %4d outputs in case %s' % (ctl, n, c.want['out'].numel(), name))
        if ctl == 'plane' or not _one_sample(c):
            assert n >= 1, (name, ctl)
        else:
            assert n == 0, (name, ctl)


def test_based_table_covers_the_shapes_and_the_proof_has_teeth():
    assert len(ec.BASED) == 20 and all(n in ec.NAMES for n in ec.BASED)
    assert sorted(set((c.p['s'],) + tuple(c.p['base'].shape[1:]) for c in map(get_case, ec.BASED))) == [(2, 7, 3), (2, 9, 23), (4, 1, 1), (4, 2, 8), (4, 5, 11)]
    p = dict(s=4, base=ec.base_map(ec.rng(3), (5, 11), (0.0, 0.25, 0.5, 0.75, 1.0)))
    with pytest.raises(AssertionError):
        ec.base_proof(p)                                                        # five levels: the fp32 bicubic at a step of 1/4 rounds
    zero = get_case('conv_last C24 19x45')
    assert 'base' not in zero.p and float(zero.p['b'][0]) == 0.5                # the zero-base cases keep their data


@pytest.mark.parametrize('name', ec.GENERAL_NAMES)
def test_general_family_bound_and_cap(name):
    """Base = bytes / 255: the reference's own float32 replay (either summation order) stays within GENERAL_BOUND of the float64
    reference, its stored formats inside the allowed intervals, and the elements at which a stored format leaves a choice stay
    under the 1 % cap."""
    g = ec.get_general(name)
    b = g.p['base']
    assert torch.equal((b.float() * 255.0).round() / 255.0, b.float()) and b.unique().numel() > 100
    for tr in (False, True):
        r = g.replay32(tr)
        err = float((r - g.want).abs().max())
        print('%-48s float32 replay (%s first): max error %.3f x 2^-24, bound %.1f x 2^-24' % (name, 'columns' if tr else 'rows', err * 2.0 ** 24, ec.GENERAL_BOUND * 2.0 ** 24))
        assert err <= ec.GENERAL_BOUND
        for fmt in ('float32', 'float16', 'uint8'):
            lo, hi = g.allowed(fmt)
            s = g.store(r, fmt)
            assert bool(((s >= lo) & (s <= hi)).all()), fmt
    for fmt in ('float16', 'uint8'):
        lo, hi = g.allowed(fmt)
        step = float((hi - lo).max())
        print('%-48s %s: %.4f of the elements leave a choice' % (name, fmt, g.loose(fmt)))
        assert g.loose(fmt) <= ec.GENERAL_CAP and (fmt != 'uint8' or step <= 1.0)
    assert min(ec._count3(g.want)) >= 4


def _rounded(c):
    p = dict(c.p)
    for k in ('w', 'w1', 'w2'):
        if k in p:
            p[k] = p[k].float().half().double()
    if 'blocks' in p:
        p['blocks'] = [tuple(t.float().half().double() if t.dim() == 4 else t for t in blk) for blk in p['blocks']]
    return p


# ---- packing -----------------------------------------------------------------------------------------------------------------------
def _conv24_blob(blob, cout, cins, f16w=False):
    from refvsr_amd import packing as pk
    ncg = sum(ec.pad8(c) for c in cins) // 8
    S = pk.c24_steps(ncg)
    nf = (cout + 15) // 16 if f16w else 3 if cout == 24 else cout // 8
    n = S * nf * 1024
    w = ec.decode_frags(blob[:n], S, nf, cout, lambda s, q: pk.c24_kblock(ncg, s, q), cins, f16w)
    return w, ec.blob_floats(blob[n:])[:cout]


def _check_conv24(w, b, cins, f16w=False):
    from refvsr_amd import packing as pk
    cout = w.shape[0]
    blob = pk.pack_conv24(w.float(), b.float(), cins, wfmt='fp16' if f16w else 'hi_lo')
    want = w.float().half().double() if f16w else w
    if cout == 48 and len(cins) == 2 and sum(cins) == 96:                       # two channel halves of the 24-output layout
        half = blob.numel() // 2
        got = [_conv24_blob(blob[i * half:(i + 1) * half], 24, cins, f16w) for i in range(2)]
        gw, gb = torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])
    else:
        gw, gb = _conv24_blob(blob, cout, cins, f16w)
    assert torch.equal(gw, want) and torch.equal(gb, b), 'pack_conv24 fragments do not decode to w'


def _check_pack_conv(w, b, cins, shuffle=False, mt=None, hi_only=False):
    from refvsr_amd import packing as pk
    p = pk.pack_conv(w.float(), b.float(), cins, shuffle, mt=mt, hi_only=hi_only)
    gw, gb = ec.decode_pack_conv(p, pk.kslot)
    assert torch.equal(gw, w.float().half().double() if hi_only else w) and torch.equal(gb, b), 'pack_conv fragments do not decode to w'


def _check_rb24(blob, convs, f16w=False):
    from refvsr_amd import packing as pk
    nf = 2 if f16w else 3
    wb = 7 * nf * 1024
    for i, (w, b) in enumerate(convs):
        want = w.float().half().double() if f16w else w
        got = ec.decode_frags(blob[i * wb:(i + 1) * wb], 7, nf, w.shape[0], pk.rb24_kblock, [24], f16w)
        assert torch.equal(got, want), 'resblock24 blob: conv %d does not decode to w' % (i + 1)
        bias = ec.blob_floats(blob[2 * wb + 128 * i:2 * wb + 128 * (i + 1)])
        assert torch.equal(bias[:w.shape[0]], b) and not bias[w.shape[0]:].any()


@pytest.mark.parametrize('name', ec.NAMES)
def test_packers_decode_to_the_weights(name):
    from refvsr_amd import packing as pk
    c = get_case(name)
    p, r = c.p, c.run
    f16w = r.get('wfmt') == 'fp16'
    if c.kind == 'conv':
        cins = [s.shape[0] for s in p['srcs']]
        _check_pack_conv(p['w'], p['b'], cins, p['shuffle'], r['mt'], r['hi_only'])
        if not r['generic'] and not p['shuffle']:
            _check_conv24(p['w'], p['b'], cins, f16w and p['w'].shape[0] in (24, 32))
        elif not r['generic']:
            C = cins[0]
            f = f16w and C == 24
            blobs = pk.pack_conv_shuffle2(p['w'].float(), p['b'].float(), wfmt='fp16' if f else 'hi_lo')
            nz = 2 if C == 24 else 4
            n = blobs.numel() // nz
            R = torch.arange(48)
            for z in range(nz):
                rows = 4 * (R % 24) + 2 * z + R // 24 if C == 24 else 4 * R + z
                gw, gb = _conv24_blob(blobs[z * n:(z + 1) * n], 48, [C], f)
                assert torch.equal(gw, (p['w'].float().half().double() if f else p['w'])[rows]) and torch.equal(gb, p['b'][rows])
    elif c.kind == 'blocks':
        for (w1, b1, w2, b2) in p['blocks']:
            if r['entry'] == 'rb24':
                blob = (pk.pack_resblock24_f16w if f16w else pk.pack_resblock24)(w1.float(), b1.float(), w2.float(), b2.float())
                _check_rb24(blob, [(w1, b1), (w2, b2)], f16w)
            elif r['entry'] == 'rb48':
                blob = pk.pack_resblock48(w1.float(), b1.float(), w2.float(), b2.float())
                assert blob.numel() == pk.RB48_BLOB
                for i, (w, b) in enumerate(((w1, b1), (w2, b2))):
                    got = ec.decode_frags(blob[i * pk.RB48_WB:(i + 1) * pk.RB48_WB], 14, 6, 48, lambda s, q: pk.c24_kblock(6, s, q), [48])
                    bias = ec.blob_floats(blob[2 * pk.RB48_WB + 256 * i:2 * pk.RB48_WB + 256 * (i + 1)])
                    assert torch.equal(got, w) and torch.equal(bias[:48], b) and not bias[48:].any()
            else:
                _check_pack_conv(w1, b1, [w1.shape[1]])
                _check_pack_conv(w2, b2, [w2.shape[1]])
    elif c.kind == 'conf_alpha':
        _check_conv24(p['w'], p['b'], [16], f16w and p['w'].shape[0] == 24)
    elif c.kind == 'conv_last':
        C = p['w'].shape[1]
        blob = pk.pack_conv_last(p['w'].float(), p['b'].float())
        S = pk.c24_steps(C // 8)
        got = ec.decode_frags(blob[:S * 1024], S, 1, 3, lambda s, q: pk.c24_kblock(C // 8, s, q), [C])
        bias = ec.blob_floats(blob[S * 1024:])
        assert torch.equal(got, p['w']) and torch.equal(bias[:3], p['b']) and not bias[3:].any()
    else:
        assert c.kind == 'hr_last'
        blob = pk.pack_conv_hr_last(p['w1'].float(), p['b1'].float(), p['w2'].float(), p['b2'].float())
        _check_rb24(blob, [(p['w1'], p['b1']), (p['w2'], p['b2'])])


def test_mismatch_report_and_fallback_rule():
    """The failure report names the first differing element in fp16 ulps and granules; the fallback rule (used only if the premise
    case fails on the device) accepts one-ulp noise on a small share of outputs and nothing else."""
    c = get_case('conv24 [24] 19x45 act.25')
    want = c.want['out']
    got = want.clone()
    assert ec.matches(got, want, c, True, True)[0]
    nz = (want != 0).nonzero()[0]
    i = tuple(int(v) for v in nz)
    got[i] = torch.nextafter(want[i].float().half(), torch.tensor(float('inf'), dtype=torch.float16)).double()
    ok, n, txt = ec.matches(got, want, c, True, True)
    assert not ok and n == 1 and '1 fp16 ulps' in txt and 'granules' in txt and 'c=%d, y=%d, x=%d' % i in txt
    assert ec.matches(got, want, c, True, False)[0]                             # fallback: one ulp, one element
    got[i] = want[i] * 2 + 1
    assert not ec.matches(got, want, c, True, False)[0]                         # more than one ulp
    share = c.controls[1] / 8.0
    many = want.clone().reshape(-1)
    k = int(math.ceil(share * many.numel())) + 1
    idx = (many != 0).nonzero()[:k, 0]
    many[idx] = torch.nextafter(many[idx].float().half(), torch.tensor(float('inf'), dtype=torch.float16)).double()
    assert not ec.matches(many.reshape(want.shape), want, c, True, False)[0]    # one ulp, but as many outputs as a lost K-block
