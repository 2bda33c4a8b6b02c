"""Channels-last result frames on a real MI355X (config.result_layout = 'hwc', REFVSR_RESULT_HWC): the two fused output heads and the
generic conversion store the interleaved [h][w][3] array with the planar result's values bit for bit and touch nothing around it; the
device scorers read such frames and return the planar frame's float64 bits; the engine keeps the layout on every call surface and
head route; evalrun writes the same image bytes and score lines.  Every comparison is torch.equal / byte equality: the layout moves
addresses, never values."""
import ctypes
import os
import re
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

DTYPES = ['float32', 'float16', 'uint8']
CANARY = 0xA5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def channels_last(x):
    return x.movedim(-3, -1).contiguous().movedim(-1, -3)


# ------------------------------------------------------------------------------------------------ heads, kernel level
# (bh, bw, scale): one partial tile | 10 x 14 output, uint8 rows of 42 bytes: every row but the first starts off dword alignment |
# several tiles with partial right and bottom edges | x2 | interior tiles
GEOMS = [(2, 8, 4), (5, 7, 2), (19, 45, 4), (33, 50, 2), (64, 96, 4)]


def guarded(h, w, dtype, dev):
    """(buffer, byte offset, byte count): a canary-filled allocation around an [h][w][3] frame of `dtype`.  The pad keeps the natural
    alignment of the samples and nothing more (uint8: an odd address), so a store wider than an element would fault or spill."""
    size = torch.empty((), dtype=dtype).element_size()
    pad = {4: 252, 2: 254, 1: 253}[size]
    n = h * w * 3 * size
    buf = torch.full((pad + n + 256,), CANARY, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    shift = (-(base + pad)) % size                                 # (torch allocations are 256-byte aligned: 0)
    return buf, pad + shift, n


def head_case(kind, c, bh, bw, scale, dev):
    """(call(fmt, out pointer) -> rc, planar call(result_dtype, result_layout) -> tensor, h, w) of one head with inputs that hit both
    clamps (the recipe of test_gpu_ops.py:test_conv_last_fused_head / test_conv_hr_last_fused_tail)."""
    from refvsr_amd import hip, ops
    from refvsr_amd.packing import pack_conv_hr_last, pack_conv_last
    g = torch.Generator().manual_seed(c + bh * bw + scale)
    h, w = bh * scale, bw * scale
    x = ops.pack_nhwc16(torch.randn(c, h, w, generator=g).to(dev))
    base = (torch.rand(3, bh, bw, generator=g) * 1.2 - 0.1).to(dev)
    P = ctypes.c_void_p
    if kind == 'conv_last':
        blob = pack_conv_last(torch.randn(3, c, 3, 3, generator=g) * 0.03, torch.randn(3, generator=g) * 0.1).to(dev)
        raw = lambda fmt, out: hip.lib().refvsr_conv_last_fmt(P(x.data_ptr()), c, h, w, P(blob.data_ptr()), P(base.data_ptr()), bh, bw,
                                                              P(out), fmt, ops._stream())
        op = lambda dt, lay: ops.conv_last(blob, x, base, result_dtype=dt, result_layout=lay)
    else:
        w1 = torch.randn(24, 24, 3, 3, generator=g) / (24 * 9) ** 0.5
        blob = pack_conv_hr_last(w1, torch.randn(24, generator=g) * 0.1, torch.randn(3, 24, 3, 3, generator=g) * 0.04,
                                 torch.randn(3, generator=g) * 0.1).to(dev)
        raw = lambda fmt, out: hip.lib().refvsr_conv_hr_last_fmt(P(x.data_ptr()), h, w, P(blob.data_ptr()), 0.1, P(base.data_ptr()), bh, bw,
                                                                 P(out), fmt, ops._stream())
        op = lambda dt, lay: ops.conv_hr_last(blob, x, base, act=0.1, result_dtype=dt, result_layout=lay)
    return raw, op, h, w, (blob, x, base)


@pytest.mark.parametrize('bh,bw,scale', GEOMS)
@pytest.mark.parametrize('kind,c', [('conv_last', 24), ('conv_last', 48), ('conv_hr_last', 24)])
def test_heads_store_the_planar_values_interleaved(dev, kind, c, bh, bw, scale):
    from refvsr_amd import hip, ops
    raw, op, h, w, keep = head_case(kind, c, bh, bw, scale, dev)
    for dt in DTYPES:
        tdt, fmt = ops.result_format(dt)
        chw = op(dt, None)
        assert chw.is_contiguous() and chw.shape == (3, h, w) and torch.equal(chw, op(dt, 'chw'))
        if dt == 'float32':                                        # both clamps are hit (so a moved clamp or rounding would show)
            assert float((chw == 0).float().mean()) > 0.01 and float((chw == 1).float().mean()) > 0.01
        # through the binding: the logical shape stays, the memory is [h][w][3]
        hwc = op(dt, 'hwc')
        assert hwc.shape == (3, h, w) and hwc.dtype == tdt
        assert hwc.permute(1, 2, 0).is_contiguous()
        assert torch.equal(hwc, chw), '%s C=%d %s: %d elements differ' % (kind, c, dt, int((hwc != chw).sum()))
        # through the C entry point into a guarded allocation at the samples' natural alignment only
        buf, off, n = guarded(h, w, tdt, dev)
        assert raw(fmt | hip.RESULT_HWC, buf.data_ptr() + off) == 0, hip.lib().refvsr_last_error()
        torch.cuda.synchronize()
        body = buf[off:off + n].clone().view(tdt).view(h, w, 3).permute(2, 0, 1)
        assert torch.equal(body, chw), '%s C=%d %s (guarded): %d elements differ' % (kind, c, dt, int((body != chw).sum()))
        assert bool((buf[:off] == CANARY).all()) and bool((buf[off + n:] == CANARY).all()), 'a store left the frame'
        # the planar form into the same kind of allocation: the flag bit alone selects the layout
        buf, off, n = guarded(h, w, tdt, dev)
        assert raw(fmt, buf.data_ptr() + off) == 0
        torch.cuda.synchronize()
        assert torch.equal(buf[off:off + n].clone().view(tdt).view(3, h, w), chw)
        assert bool((buf[:off] == CANARY).all()) and bool((buf[off + n:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ generic head
@pytest.mark.parametrize('h,w', [(10, 14), (76, 180), (256, 384)])
def test_generic_head_conversion(dev, h, w):
    from refvsr_amd import hip, ops
    g = torch.Generator().manual_seed(h + w)
    x = (torch.rand(3, h, w, generator=g) * 1.2 - 0.1).to(dev)   # past both ends: the conversion clamps as convert_result_kernel does
    x[:, 0, :5] = torch.tensor([0.0, 1.0, 0.5 / 255, 1.5 / 255, 2.5 / 255], device=dev)      # ties: round to nearest even
    P = ctypes.c_void_p
    for dt in DTYPES:
        tdt, fmt = ops.result_format(dt)
        want = ops.convert_result(x.clamp(0, 1), dt)
        if dt != 'float32':
            assert torch.equal(want, ops.convert_result(x, dt))  # (the planar kernel clamps too)
        got = ops.convert_result(x, dt, result_layout='hwc')
        assert got.shape == (3, h, w) and got.dtype == tdt and got.permute(1, 2, 0).is_contiguous()
        assert torch.equal(got, want) and torch.equal(got.permute(1, 2, 0).contiguous(), want.permute(1, 2, 0).contiguous())
        assert torch.equal(ops.convert_result(x, dt, result_layout='chw'), ops.convert_result(x, dt))
        buf, off, n = guarded(h, w, tdt, dev)
        for flag in (0, hip.RESULT_HWC):                           # (the entry point's layout is its name: the bit is accepted, not needed)
            buf.fill_(CANARY)
            assert hip.lib().refvsr_convert_result_hwc(P(x.data_ptr()), h, w, fmt | flag, P(buf.data_ptr() + off), ops._stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(buf[off:off + n].clone().view(tdt).view(h, w, 3).permute(2, 0, 1), want)
            assert bool((buf[:off] == CANARY).all()) and bool((buf[off + n:] == CANARY).all())
    with pytest.raises(ValueError):
        ops.convert_result(x, 'uint8', result_layout='nhwc')


# ------------------------------------------------------------------------------------------------ scorers
def make_result(fmt, b, h, w, g):
    if fmt == 'uint8':
        return torch.randint(0, 256, (b, 3, h, w), dtype=torch.uint8, generator=g)
    x = torch.rand(b, 3, h, w, generator=g)
    return x.half() if fmt == 'float16' else x


def make_gt(fmt, b, h, w, g):
    if fmt == 'f32':
        return torch.rand(b, 3, h, w, generator=g)
    x = torch.randint(0, 256, (b, 3, h, w), dtype=torch.uint8, generator=g)
    return channels_last(x) if fmt == 'u8_hwc' else x


@pytest.mark.parametrize('gfmt', ['f32', 'u8', 'u8_hwc'])
@pytest.mark.parametrize('afmt', DTYPES)
def test_scorers_take_channels_last_results(dev, afmt, gfmt):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects
    g = torch.Generator().manual_seed(len(afmt) * 31 + len(gfmt))
    for b in (1, 3):
        for h, w in ((7, 7), (39, 71), (45, 130)):                 # (the 32 x 64 tile edges are crossed)
            a, t = make_result(afmt, b, h, w, g).to(dev), make_gt(gfmt, b, h, w, g).to(dev)
            ah = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert (h * w == 1 or not ah.is_contiguous()) and torch.equal(ah, a)
            want = ops.score_frames(a, t)
            assert want.dtype == torch.float64 and torch.equal(ops.score_frames(ah, t), want), (b, h, w)
            assert torch.equal(ops.score_frames(list(ah), list(t)), want)
            assert torch.equal(ops.score_frames(ah, t, win=0), ops.score_frames(a, t, win=0))
        for down in (2, 4):
            for h, w in ((9, 11), (39, 71)):
                a, t = make_result(afmt, b, down * h, down * w, g).to(dev), make_gt(gfmt, b, h, w, g).to(dev)
                ah = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                want = ops.score_frames(a, t, down=down)
                assert torch.equal(ops.score_frames(ah, t, down=down), want), (b, h, w, down)
        for h, w in ((24, 40), (45, 130)):
            a, t = make_result(afmt, b, h, w, g).to(dev), make_gt(gfmt, b, h, w, g).to(dev)
            ah = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            rects = fov_rects(h, w)
            want = ops.score_regions(a, t, rects)
            assert want.dtype == torch.float64 and torch.equal(ops.score_regions(ah, t, rects), want), (b, h, w)


def test_scorers_refuse_other_strides(dev):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects
    g = torch.Generator().manual_seed(9)
    t = torch.rand(2, 3, 24, 40, generator=g).to(dev)
    wide = torch.rand(2, 3, 24, 80, generator=g).to(dev)
    for a in (wide[:, :, :, ::2], wide[:, :, :, :40], torch.rand(2, 24, 3, 40, generator=g).to(dev).permute(0, 2, 1, 3)):
        assert a.shape == t.shape
        with pytest.raises(RuntimeError, match='one layout'):
            ops.score_frames(a, t)
        with pytest.raises(RuntimeError, match='one layout'):
            ops.score_regions(a, t, fov_rects(24, 40))
    mixed = [t[0].clone(), channels_last(t[1])]                    # two dense frames of two layouts: one launch reads one layout
    with pytest.raises(RuntimeError, match='one layout'):
        ops.score_frames(mixed, list(t))


# ------------------------------------------------------------------------------------------------ engine
def make_net(name, t, dev, layout, dtype='float32', scale=4, route=None, pipelined=False):
    from refvsr_amd import SRNet, get_config, make_state_dict, set_scale
    cfg = get_config('p', 'm', name)
    if scale != 4:
        set_scale(cfg, scale)
    cfg.frame_num, cfg.save_sample = t, False
    cfg.result_dtype, cfg.result_layout = dtype, layout
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234))
    for e in net.Network.ensure_engines(2, dev):                   # routes through the engine's attributes, not the environment
        assert e.result_layout == layout
        if route == 'tail':
            e.fuse_head = e.fuse_tail = True
        elif route == 'generic':
            e.fuse_head = e.fuse_tail = False
        elif route == 'head':
            e.fuse_head, e.fuse_tail = True, False
    if pipelined:
        net.Network.set_pipelined(True)
    return net


def clip(nfr, h, w, t, dev, seed=21, n=1):
    from refvsr_amd.synth import make_clip, window_indices
    cl = [make_clip(nfr, h, w, seed=seed + b) for b in range(n)]
    lr = torch.stack([c[0] for c in cl], 0).to(dev)                # [n, nfr, 3, h, w]
    rf = torch.stack([c[1] for c in cl], 0).to(dev)
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    return lr, rf, wins


def same_frames(got, want, what):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and b.is_contiguous(), '%s frame %d' % (what, f)
        assert a.permute(0, 2, 3, 1).is_contiguous(), '%s frame %d: the result is not dense [n, sh, sw, 3] memory' % (what, f)
        assert a.shape[-1] * a.shape[-2] > 1 and not a.is_contiguous()
        assert torch.equal(a, b), '%s frame %d: %d elements differ' % (what, f, int((a != b).sum()))
        c = a.cpu()                                                # the copy to the host keeps the layout: the writer's array is dense
        assert c.permute(0, 2, 3, 1).is_contiguous() and c[0].numpy().transpose(1, 2, 0).flags['C_CONTIGUOUS']


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
@pytest.mark.parametrize('route', ['head', 'tail', 'generic'])
def test_engine_per_frame_calls(dev, route, dtype):
    nfr, t = 4, 5
    lr, rf, wins = clip(nfr, 32, 48, t, dev)
    outs = {}
    for layout in ('chw', 'hwc'):
        net = make_net('config_RefVSR_small_L1', t, dev, layout, dtype, route=route)
        outs[layout] = [net(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0)['result'].clone() for f, w in enumerate(wins)]
    assert outs['chw'][0].shape == (1, 3, 128, 192)
    same_frames(outs['hwc'], outs['chw'], '%s %s' % (route, dtype))


@pytest.mark.parametrize('dtype,route', [('uint8', 'head'), ('float32', 'tail'), ('uint8', 'generic')])
def test_engine_forward_group_pipelined(dev, dtype, route):
    nfr, t = 4, 5
    lr, rf, wins = clip(nfr, 32, 48, t, dev)
    wl = torch.stack([lr[0, w] for w in wins], 0).contiguous()     # [nfr, t, 3, h, w]
    wr = torch.stack([rf[0, w] for w in wins], 0).contiguous()
    outs = {}
    for layout in ('chw', 'hwc'):
        net = make_net('config_RefVSR_small_L1', t, dev, layout, dtype, route=route, pipelined=True)
        first = net.forward_group(wl[:1], wr[:1], [wins[0]], is_first_frame=True)['result']
        rest = net.forward_group(wl[1:], wr[1:], wins[1:], is_first_frame=False)['result']       # three windows, steady state
        torch.cuda.synchronize()
        assert isinstance(rest, tuple) and len(rest) == 3
        outs[layout] = list(first) + list(rest)
    same_frames(outs['hwc'], outs['chw'], 'forward_group %s %s' % (route, dtype))


@pytest.mark.parametrize('pipelined', [True, False])
def test_engine_two_samples_in_one_call(dev, pipelined):
    """n = 2: Engine.forward_multi's stacking (pipelined, with frame ids, steady state included) and the per-sample loop's."""
    nfr, t = 4, 5
    lr, rf, wins = clip(nfr, 32, 48, t, dev, n=2)
    outs = {}
    for layout in ('chw', 'hwc'):
        net = make_net('config_RefVSR_small_L1', t, dev, layout, 'uint8', pipelined=pipelined)
        kw = (lambda w: {'frame_ids': w}) if pipelined else (lambda w: {})
        outs[layout] = [net(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0, **kw(w))['result'] for f, w in enumerate(wins)]
        torch.cuda.synchronize()
    assert outs['chw'][0].shape == (2, 3, 128, 192)
    same_frames(outs['hwc'], outs['chw'], 'n = 2 pipelined=%s' % pipelined)


@pytest.mark.parametrize('name,t,size,scale,dtype', [('config_RefVSR_MFID', 3, (32, 48), 4, 'float16'),          # C = 48 head
                                                     ('config_RefVSR_small_L1', 5, (32, 48), 2, 'uint8'),        # x2
                                                     ('config_RefVSR_IR_L1', 5, (64, 64), 4, 'uint8'),           # generic head
                                                     ('config_RefVSR_IR_L1', 5, (64, 64), 4, 'float32')])
def test_engine_other_configurations(dev, name, t, size, scale, dtype):
    nfr = 3
    lr, rf, wins = clip(nfr, size[0], size[1], t, dev)
    outs = {}
    for layout in ('chw', 'hwc'):
        net = make_net(name, t, dev, layout, dtype, scale=scale)
        outs[layout] = [net(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0)['result'].clone() for f, w in enumerate(wins)]
    assert outs['chw'][0].shape == (1, 3, size[0] * scale, size[1] * scale)
    same_frames(outs['hwc'], outs['chw'], '%s x%d %s' % (name, scale, dtype))


@pytest.mark.parametrize('n', [1, 2])
def test_engine_two_phase_round_trip(dev, n):
    nfr, t = 3, 5
    lr, rf, wins = clip(nfr, 32, 48, t, dev, n=n)
    outs = {}
    for layout in ('chw', 'hwc'):
        net = make_net('config_RefVSR_small_L1', t, dev, layout, 'uint8')
        hs = [net.Network.phase_a(lr[:, w].contiguous(), rf[:, w].contiguous(), frame_ids=w, first_hint=f == 0) for f, w in enumerate(wins)]
        got = [net.Network.phase_b(hs[0], True)['result'], net.Network.phase_b(hs[1], False)['result']]
        net.Network.phase_b1(hs[2], False)
        got.append(net.Network.phase_b2(hs[2])['result'])
        outs[layout] = got
    same_frames(outs['hwc'], outs['chw'], 'two-phase n = %d' % n)


def test_engine_refuses_an_unknown_layout(dev):
    with pytest.raises(ValueError, match="'chw' or 'hwc'"):
        make_net('config_RefVSR_small_L1', 3, dev, 'nhwc')


# ------------------------------------------------------------------------------------------------ evalrun
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    import make_synth_dataset
    root = str(tmp_path_factory.mktemp('ds_layout'))
    make_synth_dataset.make(root, clips=2, frames=5, h=32, w=48)
    return root


def test_evalrun_writes_the_same_images_and_score_lines(dev, dataset, tmp_path):
    from refvsr_amd import evalrun, get_config, make_state_dict
    ck = str(tmp_path / 'RefVSR_small_L1.pytorch')
    torch.save(make_state_dict(get_config('p', 'm', 'config_RefVSR_small_L1'), 1234), ck)
    res = {}
    for layout in ('chw', 'hwc'):
        cfg = evalrun.build_config(['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', dataset, '--output_offset',
                                    str(tmp_path / layout), '--frame_num', '3', '--ckpt_abs_name', ck, '--result_dtype', 'uint8',
                                    '--metrics', 'device', '--frame_group', '4', '--result_layout', layout])
        assert cfg.result_layout == layout
        res[layout] = evalrun.evaluate(cfg, log=lambda *_: None)
    a, b = res['chw'], res['hwc']
    assert a['frames'] == b['frames'] == 10
    assert a['psnr'] == b['psnr'] and a['ssim'] == b['ssim']       # float64 bits from the device, not just the printed digits
    strip = lambda text: re.sub(r'\([0-9.]+sec\)', '', text)
    la, lb = (strip(open(r['score_file']).read()) for r in (a, b))
    assert la == lb and la.count('PSNR:') >= 10
    n = 0
    for fmt in ('png', 'jpg'):
        top = os.path.join(a['output_root'], fmt, 'output')
        for d, _, files in sorted(os.walk(top)):
            for fn in sorted(files):
                pa = os.path.join(d, fn)
                pb = os.path.join(b['output_root'], fmt, 'output', os.path.relpath(pa, top))
                assert open(pa, 'rb').read() == open(pb, 'rb').read(), pb
                n += 1
    assert n == 20
