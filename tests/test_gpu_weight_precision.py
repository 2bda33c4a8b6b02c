"""config.weight_precision = 'fp16' on a real MI355X: the refvsr_*_f16w twins against the hi + lo entry points on round16 weights,
and the engine in fp16 mode against the default engine on round16(sd) -- bit for bit (torch.equal) everywhere.

The contract: with weight_precision = 'fp16' and state dict sd, the engine's output equals the default engine's
output on weights.round16(sd).  The hi + lo kernels fed fp16-representable weights compute lo = 0 and add exact zeros; the twins skip
those MFMAs and keep the K order, the accumulators' initial values and the fold order, so any mismatch here is a kernel bug."""
import pytest
import torch

from conftest import maxdiff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def _r16(t):
    return t.half().float()


def _weights(co, ci, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'random':
        w = torch.randn(co, ci, 3, 3, generator=g) * 0.2
    else:                                        # 'plausible': fan-in scaled, like a trained net (a contractive residual branch)
        w = torch.randn(co, ci, 3, 3, generator=g) * (0.5 / (9 * ci) ** 0.5)
    return w, torch.randn(co, generator=g) * 0.1


def _map(h, w, c, seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(h, w, c, generator=g) * scale).half().to(dev)


SIZES = [(8, 32), (13, 37), (64, 96), (270, 480)]


# ---------------------------------------------------------------------------------------------------------- kernel twins
@pytest.mark.parametrize('kind', ['random', 'plausible'])
def test_resblock24_chain_twins(dev, kind):
    """refvsr_resblock24_chain[_batch]_f16w(pack_resblock24_f16w(w)) == refvsr_resblock24_chain[_batch](pack_resblock24(round16(w))):
    every workgroup shape (waves 4 / 8 / 16 and the by-size default), both store modes, ReLU and LeakyReLU, border / odd / full-size
    maps, batch 1 .. REFVSR_MAX_MAPS."""
    from refvsr_amd import hip, ops
    L = hip.lib()
    pairs = [(_weights(24, 24, kind, 10 + i), _weights(24, 24, kind, 20 + i)) for i in range(3)]
    pairs16 = [((_r16(w1), b1), (_r16(w2), b2)) for (w1, b1), (w2, b2) in pairs]
    ch16 = ops.Resblock24Chain(pairs, dev, wfmt='fp16')
    ch = ops.Resblock24Chain(pairs16, dev, wfmt='hi_lo')
    assert ch16.stride == hip.RESBLOCK24_F16W_BLOB_BYTES == L.refvsr_resblock24_f16w_blob_bytes()
    n_cmp = 0
    try:
        for waves in (0, 4, 8, 16):
            for store in (0, 1):
                hip.check(L.refvsr_set_resblock24_waves(waves), 'set_resblock24_waves')
                hip.check(L.refvsr_set_resblock24_store(store), 'set_resblock24_store')
                for h, w in SIZES:
                    if (waves, store) not in ((0, 1), (8, 0)) and h * w > 64 * 96:
                        continue                     # the full-size map on the default shape and one other
                    for act in (0.0, 0.2):
                        x = _map(h, w, 24, h * w + int(act * 10), dev)
                        assert torch.equal(ops.resblock24_chain(ch16, x, act), ops.resblock24_chain(ch, x, act)), (waves, store, h, w, act)
                        n_cmp += 1
                    for B in range(2, hip.MAX_MAPS + 1):
                        xs = [_map(h, w, 24, 100 * b + h, dev) for b in range(B)]
                        got = ops.resblock24_chain_b(ch16, xs, 0.0)
                        want = ops.resblock24_chain_b(ch, xs, 0.0)
                        assert torch.equal(got, want), (waves, store, h, w, B)
                        n_cmp += 1
        torch.cuda.synchronize()
    finally:
        L.refvsr_set_resblock24_waves(0)
        L.refvsr_set_resblock24_store(1)
    assert n_cmp > 50


def _cw_pair(w, b, srcs, dev, shuffle=False):
    from refvsr_amd import ops
    from refvsr_amd.packing import pack_conv
    a = ops.ConvWeights(pack_conv(_r16(w), b, srcs, shuffle), dev, wfmt='fp16')
    h = ops.ConvWeights(pack_conv(_r16(w), b, srcs, shuffle), dev, wfmt='hi_lo')
    assert a.blob24 is not None and a.blob_wfmt == 'fp16' and h.blob_wfmt == 'hi_lo'
    return a, h


@pytest.mark.parametrize('kind', ['random', 'plausible'])
def test_conv24_family_twins(dev, kind):
    """refvsr_conv24 / conv32 / conv_shuffle2 (+ their batch forms) _f16w on fp16-format blobs == the hi + lo entry points on round16
    weights: every input shape of the C = 24 family, with / without mul, res, activations, and batch 2 .. REFVSR_MAX_MAPS."""
    from refvsr_amd import hip, ops
    L = hip.lib()
    n_cmp = 0
    for (c0, c1) in ((24, 0), (16, 0), (8, 24), (24, 24)):
        srcs = [c0] if c1 == 0 else [3 if c0 == 8 else c0, c1]
        w, b = _weights(24, sum(srcs), kind, c0 + c1)
        cf, ch = _cw_pair(w, b, srcs, dev)
        assert cf.blob24.numel() == L.refvsr_conv24_f16w_blob_bytes(c0, c1)
        for h, wd in SIZES:
            s0 = _map(h, wd, c0, 1, dev)
            s1 = _map(h, wd, c1, 2, dev) if c1 else None
            m = _map(h, wd, 24, 3, dev)
            r = _map(h, wd, 24, 4, dev)
            for kw in (dict(), dict(act=0.2), dict(act=0.1, mul=m, res=r), dict(res=r, post=0.2)):
                assert torch.equal(ops.conv(cf, s0, s1, **kw), ops.conv(ch, s0, s1, **kw)), (c0, c1, h, wd, sorted(kw))
                n_cmp += 1
            if h * wd <= 64 * 96:
                for B in range(2, hip.MAX_MAPS + 1):
                    s0s = [_map(h, wd, c0, 10 + i, dev) for i in range(B)]
                    s1s = [_map(h, wd, c1, 20 + i, dev) for i in range(B)] if c1 else None
                    rs = [_map(h, wd, 24, 30 + i, dev) for i in range(B)]
                    assert torch.equal(ops.conv_b(cf, s0s, s1s, act=0.2, ress=rs), ops.conv_b(ch, s0s, s1s, act=0.2, ress=rs)), (c0, c1, B)
                    n_cmp += 1
    for srcs in ([32], [3]):                         # conv32: AlignedConv2d's 32 -> 32 convs and its RGB stem
        c0 = 32 if srcs == [32] else 8
        w, b = _weights(32, srcs[0], kind, 40 + c0)
        cf, ch = _cw_pair(w, b, srcs, dev)
        assert cf.blob24.numel() == L.refvsr_conv32_f16w_blob_bytes(c0, 0)
        for h, wd in SIZES:
            s0 = _map(h, wd, c0, 5, dev)
            r = _map(h, wd, 32, 6, dev)
            for kw in (dict(act=0.1), dict(res=r)):
                assert torch.equal(ops.conv(cf, s0, **kw), ops.conv(ch, s0, **kw)), (c0, h, wd)
                n_cmp += 1
    w, b = _weights(96, 24, kind, 77)                # PixelShufflePack 24 -> 96 + pixel shuffle (upsample1 / upsample2)
    cf, ch = _cw_pair(w, b, [24], dev, shuffle=True)
    assert cf.blob24.numel() == L.refvsr_conv_shuffle2_f16w_blob_bytes(24)
    for h, wd in SIZES:
        s0 = _map(h, wd, 24, 7, dev)
        for act in (1.0, 0.1):
            assert torch.equal(ops.conv(cf, s0, act=act), ops.conv(ch, s0, act=act)), ('shuffle', h, wd, act)
            n_cmp += 1
        if h * wd <= 64 * 96:
            for B in range(2, hip.MAX_MAPS + 1):
                s0s = [_map(h, wd, 24, 50 + i, dev) for i in range(B)]
                assert torch.equal(ops.conv_b(cf, s0s, act=0.1), ops.conv_b(ch, s0s, act=0.1)), ('shuffle', B)
                n_cmp += 1
    torch.cuda.synchronize()
    assert n_cmp > 60


@pytest.mark.parametrize('kind', ['random', 'plausible'])
def test_conf_alpha_twins(dev, kind):
    """refvsr_conf_alpha[_batch]_f16w == refvsr_conf_alpha[_batch] on round16 weights of the 16 -> 24 conv (the 2 -> 16 conv stays
    fp32 in both): up = 1 with the max by-product, up = 2, batch 2 .. REFVSR_MAX_MAPS."""
    from refvsr_amd import hip, ops
    w, b = _weights(24, 16, kind, 91)
    cf, ch = _cw_pair(w, b, [16], dev)
    g = torch.Generator().manual_seed(5)
    w0 = (torch.randn(16, 2, 3, 3, generator=g) * 0.3).to(dev).contiguous()
    b0 = (torch.randn(16, generator=g) * 0.1).to(dev).contiguous()
    for h, wd in SIZES[:3] + [(135, 240)]:
        ca = torch.rand(1, h, wd, generator=g).to(dev)
        cb = torch.rand(1, h, wd, generator=g).to(dev)
        a1, m1 = ops.conf_alpha(ca, cb, 1, w0, b0, cf, want_max=True)
        a2, m2 = ops.conf_alpha(ca, cb, 1, w0, b0, ch, want_max=True)
        assert torch.equal(a1, a2) and torch.equal(m1, m2), (h, wd)
        assert torch.equal(ops.conf_alpha(ca, cb, 2, w0, b0, cf), ops.conf_alpha(ca, cb, 2, w0, b0, ch)), (h, wd)
        for B in range(2, hip.MAX_MAPS + 1):
            cas = [torch.rand(1, h, wd, generator=g).to(dev) for _ in range(B)]
            cbs = [torch.rand(1, h, wd, generator=g).to(dev) for _ in range(B)]
            for up in (1, 2):
                assert torch.equal(ops.conf_alpha_b(cas, cbs, up, w0, b0, cf), ops.conf_alpha_b(cas, cbs, up, w0, b0, ch)), (h, wd, B, up)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- engine
def _nets(name, t, dev, scale=4, precision='fp16', sd_variant=None, seed=1234, result_dtype=None):
    """(fp16-mode net on sd, default net on round16(sd), cfg, sd)"""
    from refvsr_amd import SRNet, get_config, make_state_dict, set_scale
    from refvsr_amd.weights import round16
    nets = []
    for mode in (precision, 'hi_lo'):
        cfg = get_config('p', 'm', name)
        if scale != 4:
            set_scale(cfg, scale)
        cfg.frame_num, cfg.save_sample = t, False
        cfg.weight_precision = mode
        if result_dtype:
            cfg.result_dtype = result_dtype
        sd = make_state_dict(cfg, seed, variant=sd_variant)
        n_ = SRNet(cfg).to(dev).eval()
        n_.load_state_dict(sd if mode != 'hi_lo' else round16(sd))
        nets.append(n_)
    return nets[0], nets[1], cfg, sd


def _per_frame(net, lr, rf, nfr, t, dev, frame_ids=False):
    from refvsr_amd.synth import window_indices
    outs = []
    for f in range(nfr):
        w = window_indices(f, nfr, t)
        kw = dict(frame_ids=w) if frame_ids else {}
        outs.append(net(lr[w][None].to(dev), rf[w][None].to(dev), f == 0, **kw)['result'].clone())
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('name,h,w,nfr,scale,t', [
    ('config_RefVSR_small_L1', 64, 96, 6, 4, 5),
    ('config_RefVSR_small_MFID_8K', 64, 96, 3, 4, 3),
    ('config_RefVSR_small_L1', 64, 96, 4, 2, 5),
    ('config_RefVSR_small_L1', 270, 480, 3, 4, 5),
])
def test_engine_fp16_equals_default_on_round16(dev, name, h, w, nfr, scale, t):
    """SRNet with weight_precision = 'fp16' on sd == the default SRNet on round16(sd), every frame (t = 5, reset_branch = 4 so that
    six frames cross a branch restart).  Fails when the engine ignores the field: round16 moves the result by far more than a bit."""
    from refvsr_amd.synth import make_clip
    lr, rf, _ = make_clip(nfr, h, w, seed=7, want_gt=False)
    a, b, cfg, sd = _nets(name, t, dev, scale=scale)
    for n_ in (a, b):
        n_.config.reset_branch = 4
    assert a.Network._weights(dev).wfmt == 'fp16' and b.Network._weights(dev).wfmt == 'hi_lo'
    ga = _per_frame(a, lr, rf, nfr, t, dev)
    gb = _per_frame(b, lr, rf, nfr, t, dev)
    for f in range(nfr):
        assert torch.equal(ga[f], gb[f]), '%s %dx%d x%d frame %d: max diff %.3e' % (name, h, w, scale, f, maxdiff(ga[f], gb[f]))


def test_engine_fp16_group_pipelined_multi_uint8_and_reload(dev):
    """The schedules of the C = 24 engine in fp16 mode against the default engine on round16(sd): forward_group (B = 4) after a
    pipelined first call with frame_ids, n = 2 samples, result_dtype = 'uint8', and a second state dict loaded mid-stream."""
    from refvsr_amd.synth import make_clip, window_indices
    from refvsr_amd import make_state_dict
    from refvsr_amd.weights import round16
    nfr, t = 5, 5
    lr, rf, _ = make_clip(nfr, 64, 96, seed=9)
    lr, rf = lr.to(dev), rf.to(dev)
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    a, b, cfg, sd = _nets('config_RefVSR_small_L1', t, dev)
    outs = []
    for n_ in (a, b):
        n_.Network.set_pipelined(True)
        got = [n_(lr[wins[0]][None], rf[wins[0]][None], True, frame_ids=wins[0])['result']]
        got += list(n_.forward_group(torch.stack([lr[w] for w in wins[1:]], 0), torch.stack([rf[w] for w in wins[1:]], 0), wins[1:])['result'])
        torch.cuda.synchronize()
        outs.append([g.clone() for g in got])
    for f in range(nfr):
        assert torch.equal(outs[0][f].reshape(-1), outs[1][f].reshape(-1)), 'forward_group frame %d' % f
    # a second state dict mid-stream: the packed weights follow load_state_dict in both modes
    sd2 = make_state_dict(cfg, 4321, variant='plausible')
    a.load_state_dict(sd2)
    b.load_state_dict(round16(sd2))
    for n_ in (a, b):
        n_.Network.set_pipelined(False)
        n_.Network.reset()
    x2 = torch.stack([lr[wins[0]], lr[wins[1]]], 0)
    r2 = torch.stack([rf[wins[0]], rf[wins[1]]], 0)
    oa = a(x2, r2, True)['result']
    ob = b(x2, r2, True)['result']
    torch.cuda.synchronize()
    assert torch.equal(oa, ob), 'n = 2 after load_state_dict'
    # uint8 results
    a8, b8, _, _ = _nets('config_RefVSR_small_L1', t, dev, result_dtype='uint8', sd_variant='plausible')
    ga = _per_frame(a8, lr.cpu(), rf.cpu(), 3, t, dev, frame_ids=True)
    gb = _per_frame(b8, lr.cpu(), rf.cpu(), 3, t, dev, frame_ids=True)
    for f in range(3):
        assert ga[f].dtype == torch.uint8 and torch.equal(ga[f], gb[f]), 'uint8 frame %d' % f


def test_two_modes_in_one_process(dev):
    """Two engines of different weight formats side by side, interleaved call by call: each equals its own single-mode run."""
    from refvsr_amd.synth import make_clip
    nfr, t = 3, 5
    lr, rf, _ = make_clip(nfr, 32, 48, seed=3)
    a, b, cfg, sd = _nets('config_RefVSR_small_L1', t, dev)
    from refvsr_amd import SRNet
    ref_a = _per_frame(a, lr, rf, nfr, t, dev)
    c = SRNet(a.config).to(dev).eval()            # fp16 mode again, fresh
    c.load_state_dict(sd)
    d = SRNet(cfg).to(dev).eval()                 # cfg.weight_precision was left at 'hi_lo' by _nets: the default on sd
    d.load_state_dict(sd)
    from refvsr_amd.synth import window_indices
    for f in range(nfr):
        w = window_indices(f, nfr, t)
        oc = c(lr[w][None].to(dev), rf[w][None].to(dev), f == 0)['result']
        od = d(lr[w][None].to(dev), rf[w][None].to(dev), f == 0)['result']
        torch.cuda.synchronize()
        assert torch.equal(oc, ref_a[f]), 'fp16 engine next to a default one, frame %d' % f
        assert not torch.equal(od, oc), 'the default engine on sd must differ from fp16 mode (frame %d)' % f


@pytest.mark.parametrize('precision', ['hi_lo', 'amp'])
def test_c48_hi_lo_and_amp_equal_default(dev, precision):
    """On a mid_channels = 48 config (is_amp = False) 'hi_lo' and 'amp' resolve to the default: bit-identical to an engine whose
    config never mentions the field."""
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    lr, rf, _ = make_clip(2, 32, 48, seed=4)
    outs = []
    for mode in (precision, None):
        cfg = get_config('p', 'm', 'config_RefVSR_MFID')
        cfg.frame_num, cfg.save_sample = 3, False
        if mode is None:
            del cfg['weight_precision']
        else:
            cfg.weight_precision = mode
        n_ = SRNet(cfg).to(dev).eval()
        n_.load_state_dict(make_state_dict(cfg, 1234))
        outs.append(_per_frame(n_, lr, rf, 2, 3, dev))
        assert n_.Network._weights(dev).wfmt == 'hi_lo'
    for f in range(2):
        assert torch.equal(outs[0][f], outs[1][f])


def test_fp16_mode_against_live_oracle_on_round16(dev):
    """weight_precision = 'fp16' against OracleNetwork(cfg, round16(sd)) at 64x96, t = 5, under the bars of
    test_gpu_e2e.py:test_midsize_against_live_oracle_and_cache_equivalence."""
    import numpy as np
    from oracle import refvsr_oracle as orc
    from refvsr_amd.synth import make_clip, window_indices
    from refvsr_amd.weights import round16

    def psnr(x, y):
        mse = float(((x.double() - y.double()) ** 2).mean())
        return 10.0 * np.log10(1.0 / max(mse, 1e-30))
    lr, rf, gt = make_clip(4, 64, 96, seed=5)
    a, _, cfg, sd = _nets('config_RefVSR_small_L1', 5, dev)
    o = orc.OracleNetwork(cfg, round16(sd))
    for f in range(4):
        w = window_indices(f, 4, 5)
        got = a(lr[w][None].to(dev), rf[w][None].to(dev), f == 0)['result'].cpu()
        want = o.forward(lr[w][None], rf[w][None], f == 0)['result']
        d_psnr = abs(psnr(got, gt[f][None]) - psnr(want, gt[f][None]))
        assert maxdiff(got, want) < 2e-2 and psnr(got, want) > 55.0 and d_psnr < 1e-3, (f, maxdiff(got, want), d_psnr)
