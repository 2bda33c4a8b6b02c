"""CPU side of the exact-arithmetic parity tests (tests/exact_cases.py, tests/test_gpu_exact.py): for every case the GPU file runs,
  * the exactness condition holds (fewer than 2^24 granules at every stage of every conv) and the controls show that the case
    would see a missing lo term: (a) all lo terms dropped >= 5 % of the outputs, (b) one K-block's lo term >= 1 % and >= 8 outputs;
  * a float32 evaluation -- F.conv2d with hi and with lo, added -- equals the float64 reference exactly (the empirical side of the
    exactness argument: float32 sums in MKL-DNN's order lose nothing either);
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
