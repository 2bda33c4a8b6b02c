"""CPU side of the sampling / gather parity suite (tests/sampling_cases.py; the kernels run in tests/test_gpu_sampling.py):

  * every exact case proves its condition -- each traced step of the float32 chain equals the float64 chain -- its controls and its
    populated tap classes;
  * every general case's E_ref (float32 evaluation vs float64 evaluation of the same reference) stays under the project's
    fp32-interpolation bar, so the GPU bracket delta = 4 max E_ref cannot grow unnoticed;
  * anchoring: each float64 reference agrees with the reference-pinned oracle on seeded random inputs, and reproduces the
    fixtures the reference itself produced (op_warp, op_sampler, op_resize to 2e-5 max|x|; op_aa bit for bit)."""
import numpy as np
import pytest
import torch

import sampling_cases as sc
from conftest import load_golden
from sampling_cases import F64, get_case

BAR = sc.E_REF_BAR


def t32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def close(got, want, scale, what=''):
    err = float(np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64)).max())
    assert err <= BAR * scale, '%s: %.3e > %.3e' % (what, err, BAR * scale)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_kernel_family():
    ops = {get_case(n).op for n in sc.NAMES}
    assert ops == set(sc.REFS)
    assert len(sc.EXACT) + len(sc.GENERAL) == len(sc.NAMES)


@pytest.mark.parametrize('name', sc.EXACT)
def test_exact_case_is_exact_and_strong(name):
    c = get_case(name)
    steps = c.assert_exact()
    c.assert_strong()
    for k, v in c.want.items():                              # the inputs and results are numbers the kernel's formats hold
        assert np.array_equal(v, c.store({k: v})[k])
    assert steps > 0 or c.bits_only or c.op == 'gather' or c.p.get('is_max') or c.p.get('kind') in ('max', 'max2')


@pytest.mark.parametrize('name', sc.GENERAL)
def test_general_case_reference_error_is_under_the_bar(name):
    c = get_case(name)
    worst = max(c.e_ref().values())
    assert worst <= BAR * c.max_input(), (name, worst, c.max_input())
    for k in c.want64:
        assert np.isfinite(c.want64[k]).all() and np.isfinite(c.bound(k)).all()
        assert (c.bound(k) >= c.delta(k)).all()


def test_wild_flows_take_the_clamp_and_give_zero():
    c = get_case(sc.EXACT[0])
    assert int(c.untraced.sum()) == 8 and float(np.abs(c.p['flow']).max()) == 2.0 ** 30
    for T in (sc.F32, F64):
        x0, y0, _, _, _, _ = sc.warp_coords(T, c.p['flow'], 5, 9)
        bad = c.untraced
        assert (((x0[bad] == -2) | (x0[bad] == 10)) | ((y0[bad] == -2) | (y0[bad] == 6))).all()
    assert not c.want['out'][:, c.untraced].any()


def test_clamp_cases_hit_both_clamps_and_saturated_cases_all_three_values():
    for n in sc.EXACT:
        c = get_case(n)
        if c.op == 'resize' and c.p.get('clamp01'):
            o = c.want['out']
            assert (o == 0).sum() >= 4 and (o == 1).sum() >= 4 and ((o > 0) & (o < 1)).sum() >= 4, n
    c = get_case('tsa_blend x saturated')
    assert {0.0, 100.0, -100.0} == set(np.unique(c.p['attn']))


def test_block_gather_indices_cover_the_corners():
    for n in sc.EXACT:
        c = get_case(n)
        if c.op == 'gather':
            assert list(c.p['idx'].flat[:4]) == [0, 6 * 9 - 1, 9 - 1, 9]


def test_ulp16():
    assert sc.ulp16(1.0) == 2.0 ** -10 and sc.ulp16(0.999) == 2.0 ** -11 and sc.ulp16(0.0) == 2.0 ** -24 and sc.ulp16(-3e-5) == 2.0 ** -24
    assert sc.ulp16(2048.0) == 2.0


# ---- anchoring against the oracle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def orc():
    from oracle import refvsr_oracle
    return refvsr_oracle


@pytest.fixture(scope='module')
def iro():
    from oracle import refvsr_ir_oracle
    return refvsr_ir_oracle


@pytest.mark.parametrize('geo', [(18, 26, 18, 26), (36, 52, 18, 26), (7, 13, 7, 13)])
def test_ref_warp_vs_oracle(orc, geo):
    g = sc.rng(11)
    hf, wf, hin, win = geo
    x, fl = sc.f32_map(g, 5, hin, win), sc.f32_map(g, 2, hf, wf, 4.0)
    close(sc.ref_warp(F64, {'x': x, 'flow': fl})['out'], orc.warp(t32(x)[None], t32(fl)[None])[0], np.abs(x).max(), 'warp')


def test_ref_flow_warp_border_flow_up2_and_level_input_vs_oracle(orc):
    g = sc.rng(12)
    a, b, fp = sc.f32_map(g, 3, 18, 30), sc.f32_map(g, 3, 18, 30), sc.f32_map(g, 2, 9, 15, 6.0)
    up = sc.ref_flow_up2(F64, fp)
    want_up = orc.flow_up2(t32(fp)[None])
    close(up, want_up[0], np.abs(fp).max(), 'flow_up2')
    wrp, clamped = sc.ref_flow_warp_border(F64, b, up)
    assert all(int(v.sum()) >= 4 for v in clamped.values()), 'the border clamp must bind on all four sides'
    close(wrp, orc.flow_warp_border(t32(b)[None], want_up)[0], np.abs(b).max(), 'flow_warp_border')
    out = sc.ref_spynet_level_input(F64, {'ref': [a], 'supp': [b], 'flow_prev': [fp]})
    want = torch.cat([t32(a), orc.flow_warp_border(t32(b)[None], want_up)[0], want_up[0]], 0)
    close(out['out'][0], want, float(want.abs().max()), 'spynet_level_input')
    close(out['flow_up'][0], want_up[0], np.abs(fp).max())
    none = sc.ref_spynet_level_input(F64, {'ref': [a], 'supp': [b], 'flow_prev': None})
    assert not none['flow_up'].any()
    close(none['out'][0][3:6], orc.flow_warp_border(t32(b)[None], torch.zeros(1, 2, 18, 30))[0], np.abs(b).max())


def test_spynet_general_cases_clamp_on_all_four_sides():
    for n in sc.GENERAL:
        c = get_case(n)
        if c.op == 'spynet' and c.p['flow_prev'] is not None:
            up = c.want64['flow_up'][0]
            _, clamped = sc.ref_flow_warp_border(F64, c.p['supp'][0], up)
            assert all(int(v.sum()) >= 4 for v in clamped.values()), (n, {k: int(v.sum()) for k, v in clamped.items()})


@pytest.mark.parametrize('mode,name,hw,out_hw,scale', [
    (sc.RS_BICUBIC, 'bicubic', (18, 26), (36, 52), 0.5), (sc.RS_BICUBIC, 'bicubic', (18, 26), (9, 13), 2.0),
    (sc.RS_BICUBIC, 'bicubic', (7, 13), (10, 19), None), (sc.RS_BILINEAR, 'bilinear', (18, 26), (32, 32), None),
    (sc.RS_BILINEAR, 'bilinear', (32, 32), (18, 26), None), (sc.RS_BILINEAR_AC, 'bilinear_ac', (9, 15), (18, 30), None),
    (sc.RS_BILINEAR_AC, 'bilinear_ac', (5, 5), (9, 9), None), (sc.RS_NEAREST, 'nearest', (18, 26), (9, 13), 2.0),
    (sc.RS_NEAREST, 'nearest', (7, 13), (10, 19), None)])
def test_ref_resize_vs_oracle(orc, mode, name, hw, out_hw, scale):
    x = sc.f32_map(sc.rng(13), 3, hw[0], hw[1])
    got = sc.ref_resize(F64, {'x': x, 'out_hw': out_hw, 'mode': mode, 'src_scale': (scale, scale) if scale else None})['out']
    close(got, orc.resize(t32(x)[None], out_hw, name, scale)[0], np.abs(x).max(), name)


def test_ref_resize_epilogues_and_bicubic_scale_vs_oracle(orc):
    x = np.abs(sc.f32_map(sc.rng(14), 3, 13, 19))
    mean, std, mul = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], [0.5, 2.0, 0.25]
    base = orc.resize(t32(x)[None], (16, 32), 'bilinear')[0]
    got = sc.ref_resize(F64, {'x': x, 'out_hw': (16, 32), 'mode': sc.RS_BILINEAR, 'mean': mean, 'std': std, 'chan_mul': mul, 'clamp01': True})['out']
    want = (((base - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)) * torch.tensor(mul).view(3, 1, 1)).clamp(0, 1)
    close(got, want, 20.0)
    for f in (2, 4, 0.5):
        oh, ow = int(13 * f), int(19 * f)
        got = sc.ref_resize(F64, {'x': x, 'out_hw': (oh, ow), 'mode': sc.RS_BICUBIC, 'src_scale': (1.0 / f, 1.0 / f), 'clamp01': True})['out']
        close(got, orc.bicubic_scale(t32(x)[None], f)[0], np.abs(x).max(), 'bicubic_scale %g' % f)


@pytest.mark.parametrize('s', [1, 2, 4])
def test_ref_block_gather_vs_oracle(orc, s):
    c = get_case('block_gather x planar s%d' % s)
    v, idx = c.p['value'], c.p['idx']
    want = orc.block_gather(t32(v)[None], torch.from_numpy(idx.reshape(1, -1)), s, (idx.shape[0] * s, idx.shape[1] * s))[0]
    assert np.array_equal(c.want['out'], want.double().numpy())


@pytest.mark.parametrize('ks', [2, 4])
def test_ref_aligned_sample_vs_oracle(orc, ks):
    g = sc.rng(15)
    x = sc.f32_map(g, 6, 7 * ks, 9 * ks)
    for aff in (g.uniform(-3, 3, size=(3, 7, 9)), sc.placed_affine(g, 7, 9, ks)):
        aff = aff.astype(np.float32).astype(F64)
        got = sc.ref_aligned_sample(F64, {'x': x, 'affine': aff, 'ks': ks})['out']
        close(got, orc.aligned_sample(t32(x)[None], t32(aff)[None], ks)[0], np.abs(x).max(), 'aligned_sample')


def test_ref_pools_vs_oracle(orc, iro):
    x = sc.f32_map(sc.rng(16), 5, 7, 11)
    close(sc.ref_pool2(F64, {'x': x, 'kind': 'avg'})['out'], orc.avg_pool2(t32(x)[None])[0], np.abs(x).max())
    assert np.array_equal(sc.ref_pool2(F64, {'x': x, 'kind': 'max'})['out'], orc.max_pool2(t32(x)[None])[0].double().numpy())
    for hw in ((5, 7), (6, 8)):
        y = sc.f16_map(sc.rng(17), 8, hw[0], hw[1])
        assert np.array_equal(sc.ref_pool3s2(F64, {'x': y, 'is_max': 1})['out'], iro.pool3s2(t32(y)[None], 'max')[0].double().numpy())
        close(sc.ref_pool3s2(F64, {'x': y, 'is_max': 0})['out'], iro.pool3s2(t32(y)[None], 'avg')[0], np.abs(y).max())
        close(sc.ref_up2_bilinear(F64, {'x': y, 'mul': 2.0})['out'], iro.up2_bilinear(t32(y)[None])[0] * 2, 2 * np.abs(y).max())


def test_ref_dcn_sample_vs_oracle_dcn_pack(iro):
    """The oracle's ModulatedDCNPack with an identity conv_offset (its output IS the offset / mask map) against a float64 1 x 1
    contraction of the reference's sampled columns."""
    g = sc.rng(18)
    M, h, w = 64, 9, 13
    x = sc.f32_map(g, M, h, w)
    om = sc.f32_map(g, 216, h, w, 2.5)
    om[:, :2] += 3.0                                         # rows pushed off the map: zero outside, partial corners
    wt = sc.f32_map(g, M, M * 9, 1).reshape(M, M, 3, 3) / 24.0
    eye = np.zeros((216, 216, 3, 3), dtype=np.float32)
    eye[np.arange(216), np.arange(216), 1, 1] = 1.0
    W = {'d.weight': t32(wt), 'd.bias': torch.zeros(M), 'd.conv_offset.weight': torch.from_numpy(eye), 'd.conv_offset.bias': torch.zeros(216)}
    want = iro.dcn_pack(t32(x)[None], t32(om)[None], W, 'd')[0]
    cols = sc.ref_dcn_sample(F64, {'x': x, 'om': om, 'dg': 8})['out'].reshape(9, M, h, w)
    got = np.einsum('kchw,ock->ohw', cols, wt.reshape(M, M, 9))
    close(got, want, float(want.abs().max()), 'dcn_pack')


def test_ref_tsa_vs_torch_float64():
    c = get_case('tsa_weight g t5')
    em, er, al = [torch.from_numpy(np.stack(c.p[k])) for k in ('emb', 'emb_ref', 'aligned')]
    corr = torch.sigmoid((em * er[None]).sum(1))
    assert float(corr.logit().abs().max()) <= 8.0
    close(c.want64['out'], (al * corr[:, None]).reshape(-1, 5, 7), 8.0)
    c = get_case('tsa_blend g random')
    f, a, d = [torch.from_numpy(c.p[k]) for k in ('feat', 'attn', 'add')]
    assert float(a.abs().max()) <= 8.0
    close(c.want64['out'], f * torch.sigmoid(a) * 2 + d, 8.0)


# ---- the fixtures the reference produced ----------------------------------------------------------------------------------------------
def n64(t):
    return t.double().numpy()


def test_fixture_op_warp():
    g = load_golden('op_warp')
    x = n64(g['x'][0])
    close(sc.ref_warp(F64, {'x': x, 'flow': n64(g['flow'][0])})['out'], g['warp'][0], np.abs(x).max(), 'warp')
    close(sc.ref_warp(F64, {'x': x, 'flow': n64(g['flow2'][0])})['out'], g['warp2'][0], np.abs(x).max(), 'warp2')
    close(sc.ref_flow_warp_border(F64, x, n64(g['flow'][0]))[0], g['flow_warp'][0], np.abs(x).max(), 'flow_warp')


def test_fixture_op_sampler():
    g = load_golden('op_sampler')
    x = n64(g['x'][0])
    close(sc.ref_aligned_sample(F64, {'x': x, 'affine': n64(g['affine'][0]), 'ks': 2})['out'], g['out'][0], np.abs(x).max())


def test_fixture_op_resize():
    g = load_golden('op_resize')
    img, fl = n64(g['img'][0]), n64(g['flow'][0])

    def rs(x, out_hw, mode, scale=None):
        return sc.ref_resize(F64, {'x': x, 'out_hw': out_hw, 'mode': mode, 'src_scale': (scale, scale) if scale else None})['out']
    m = np.abs(img).max()
    close(rs(img, (9, 13), sc.RS_BICUBIC, 2.0), g['bicubic_half'][0], m, 'bicubic_half')
    close(rs(img, (36, 52), sc.RS_BICUBIC, 0.5), g['bicubic_x2'][0], m, 'bicubic_x2')
    close(rs(img, (72, 104), sc.RS_BICUBIC, 0.25), g['bicubic_x4'][0], m, 'bicubic_x4')
    close(sc.ref_flow_up2(F64, fl), g['flow_up2'][0], np.abs(fl).max(), 'flow_up2')
    close(rs(img, (32, 32), sc.RS_BILINEAR), g['bilinear_32x32'][0], m, 'bilinear_32x32')
    close(rs(n64(g['bilinear_32x32'][0]), (18, 26), sc.RS_BILINEAR), g['bilinear_back'][0], m, 'bilinear_back')
    assert np.array_equal(rs(img, (9, 13), sc.RS_NEAREST, 2.0), n64(g['nearest_half'][0]))


def test_fixture_op_aa_bit_for_bit():
    g = load_golden('op_aa')
    idx = g['idx'][0].numpy().reshape(20, 28)
    for value, s, want in (('value_down', 1, 'aa1'), ('value', 2, 'aa2_fm'), ('ref', 2, 'aa2_rgb')):
        got = sc.ref_block_gather(F64, {'value': n64(g[value][0]), 'idx': idx, 's': s})['out']
        assert np.array_equal(got, n64(g[want][0])), want
