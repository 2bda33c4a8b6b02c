"""8-bit input frames on a real MI355X: refvsr_ingest_u8 and refvsr_bytes_equal against the CPU, and every engine schedule fed
uint8 windows (planar and channels-last) against the float32 engine fed the CPU-converted frames -- torch.equal, frame by frame.

The contract: a uint8 input means byte / 255 as the reference loader computes it (float64 quotient rounded to float32); the engine
converts the bytes on the device into the fp32 frames it owns, and everything after that is the float path, so the results are
bit-identical to the float32 engine on float32(bytes / 255)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def _cpu_conv(b):
    """The reference loader's conversion of bytes (data_loader/utils.py:28) on the CPU."""
    return torch.from_numpy((b.cpu().contiguous().numpy() / 255.).astype(np.float32))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('layout', ['planar', 'hwc'])
@pytest.mark.parametrize('h,w', [(2, 2), (18, 26), (270, 480), (1080, 1920)])
def test_ingest_kernel_bit_exact_with_guards(dev, layout, h, w):
    """Frames at the offsets of frames 0..t-1 of a window (4-byte aligned only) behind a base offset of 0 / 4 / 8 / 12 bytes, 1..16
    frames per launch: every output equals the CPU conversion bit for bit, the guard floats around every destination stay untouched."""
    from refvsr_amd import ops
    fb = 3 * h * w
    counts = list(range(1, 17)) if fb <= 3 * 18 * 26 else ([1, 5, 16] if h < 1080 else [1, 7])
    G = 64
    g = torch.Generator().manual_seed(h * w)
    n_cmp = 0
    for nf in counts:
        for off in ((0, 4, 8, 12) if nf <= 5 or h < 270 else (4,)):
            raw = torch.randint(0, 256, (off + nf * fb,), dtype=torch.uint8, generator=g)
            k = min(raw.numel(), 4 * 256)
            raw[:k] = (torch.arange(k) * 37 + off) % 256          # every byte value where the frames hold 256 bytes or more
            raw_d = raw.to(dev)
            srcs = []
            for i in range(nf):
                x = raw_d[off + i * fb: off + (i + 1) * fb]
                srcs.append(x.view(3, h, w) if layout == 'planar' else x.view(h, w, 3).permute(2, 0, 1))
            stride = fb + G
            dst = torch.full((G + nf * stride,), -3.25, dtype=torch.float32, device=dev)
            dsts = [dst[G + i * stride: G + i * stride + fb].view(3, h, w) for i in range(nf)]
            ops.ingest_u8(list(zip(srcs, dsts)))
            out = dst.cpu()
            for i in range(nf):
                fr = raw[off + i * fb: off + (i + 1) * fb]
                want = _cpu_conv(fr.view(3, h, w) if layout == 'planar' else fr.view(h, w, 3).permute(2, 0, 1))
                assert _same_bits(out[G + i * stride: G + i * stride + fb].view(3, h, w), want), (nf, off, i)
                n_cmp += 1
            guard = torch.cat([out[:G]] + [out[G + i * stride + fb: G + (i + 1) * stride] for i in range(nf)])
            assert bool((guard == -3.25).all()), 'guard bytes written (nf %d, off %d)' % (nf, off)
    assert n_cmp >= len(counts)


def test_ingest_torch_op_and_every_byte_value(dev):
    """torch.ops.refvsr.ingest_u8 on a [n, t, h, w, 3] view, a planar window and an unaligned slice == the CPU conversion; all 256
    byte values go through the table."""
    import refvsr_amd.torch_ops  # noqa: F401
    b = torch.arange(2 * 5 * 18 * 26 * 3, dtype=torch.int64).remainder(256).to(torch.uint8).view(2, 5, 18, 26, 3)
    y = torch.ops.refvsr.ingest_u8(b.to(dev).permute(0, 1, 4, 2, 3))
    assert y.dtype == torch.float32 and y.is_contiguous() and _same_bits(y.cpu(), _cpu_conv(b.permute(0, 1, 4, 2, 3)))
    p = b.view(2, 5, 3, 18, 26)
    assert _same_bits(torch.ops.refvsr.ingest_u8(p.to(dev)).cpu(), _cpu_conv(p))
    flat = torch.arange(3 * 8 * 10 + 1, dtype=torch.int64).remainder(256).to(torch.uint8).to(dev)
    x = flat[1:].view(3, 8, 10)                                       # 1-byte offset: copied to aligned storage first
    assert _same_bits(torch.ops.refvsr.ingest_u8(x).cpu(), _cpu_conv(x.cpu()))
    u = torch.arange(256, dtype=torch.int64).to(torch.uint8).repeat(3 * 16 * 16 // 256 * 1).view(3, 16, 16)
    t = torch.ops.refvsr.ingest_u8(u.to(dev)).cpu()
    assert _same_bits(t, _cpu_conv(u)) and sorted(set(t.view(-1).tolist())) == sorted(set((np.arange(256) / 255.).astype(np.float32).tolist()))


def test_bytes_equal_finds_one_changed_byte(dev):
    """refvsr_bytes_equal at many lengths and both buffers' offsets: equal buffers give True, a single changed byte at the head, the
    middle or the tail gives False."""
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(5)
    lengths = (1, 3, 4, 15, 16, 17, 31, 64, 1001, 4097, 3 * 270 * 480 + 4)
    offs = ((0, 0), (1, 0), (0, 5), (4, 12), (7, 3), (12, 4), (15, 15))
    for n in lengths:
        pairs, want = [], []
        base = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
        for oa, ob in offs:
            A = torch.zeros(oa + n + 16, dtype=torch.uint8)
            B = torch.zeros(ob + n + 16, dtype=torch.uint8)
            A[oa:oa + n] = base
            B[ob:ob + n] = base
            B[:ob] = 255 - (torch.arange(ob) % 256).to(torch.uint8)     # (bytes outside the range differ and must not count)
            B[ob + n:] = 7
            for pos in (None, 0, n // 2, n - 1):
                Bx = B.clone()
                if pos is not None:
                    Bx[ob + pos] ^= 1
                Ad, Bd = A.to(dev), Bx.to(dev)
                pairs.append((Ad[oa:oa + n], Bd[ob:ob + n]))
                want.append(pos is None)
        got = ops.bytes_equal(pairs)                                    # (one size per call)
        assert got == want, (n, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:10])


# ------------------------------------------------------------------------------------------------------------ the engine
def _net(name, t, dev, scale=4, reset='keep', save_sample=False, **cfg_kw):
    from refvsr_amd import SRNet, get_config, make_state_dict, set_scale
    cfg = get_config('p', 'm', name)
    if scale != 4:
        set_scale(cfg, scale)
    cfg.frame_num, cfg.save_sample = t, save_sample
    if reset != 'keep':
        cfg.reset_branch = reset
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234, variant='plausible'))
    return net


def _clip(nfr, h, w, seed=3):
    from refvsr_amd.synth import make_clip
    lr, rf, _ = make_clip(nfr, h, w, seed=seed, want_gt=False)
    q = lambda x: torch.round(x * 255.0).to(torch.uint8)
    return q(lr), q(rf)


def _win(x, idx, lay, dev):
    """Window `idx` of the byte clip x [N,3,h,w] as a [1,t,3,h,w] cuda input: 'f32' = the CPU-converted float32 frames, 'planar' =
    contiguous bytes, 'hwc' = the channels-last view of [1,t,h,w,3] bytes."""
    y = x[idx]
    if lay == 'f32':
        return _cpu_conv(y)[None].to(dev)
    if lay == 'hwc':
        return y.permute(0, 2, 3, 1).contiguous()[None].to(dev).permute(0, 1, 4, 2, 3)
    return y.contiguous()[None].to(dev)


def _stream(net, lr, rf, t, dev, lays, ids=False, ready=None, is_log=False):
    """One forward() per output frame; lays: the input kind of each frame's call (a list: a dtype switch mid-stream)."""
    from refvsr_amd.synth import window_indices
    nfr = lr.shape[0]
    outs = []
    for f in range(nfr):
        w = window_indices(f, nfr, t)
        kw = {'frame_ids': w} if ids else {}
        a, b = _win(lr, w, lays[f], dev), _win(rf, w, lays[f], dev)
        if ready is not None:
            r = ready
            if ready == 'event':
                r = torch.cuda.Event()
                r.record()
            kw['input_ready'] = r
        o = net(a, b, f == 0, is_log=is_log, **kw)
        outs.append((o['result'].clone(), {k: v.clone() for k, v in o.get('eval_vis', {}).items()}))
    torch.cuda.synchronize()
    return outs


def _check(want, got, what):
    for f, ((a, va), (b, vb)) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and torch.equal(a, b), '%s: frame %d differs' % (what, f)
        assert sorted(va) == sorted(vb) and all(torch.equal(va[k], vb[k]) for k in va), '%s: vis of frame %d' % (what, f)


@pytest.mark.parametrize('name,h,w,t,nfr,scale,kw', [
    ('config_RefVSR_small_L1', 32, 48, 5, 6, 4, {}),                                    # RefVSR_small, C = 24, restart at frame 3
    ('config_RefVSR_MFID', 32, 48, 3, 4, 4, {}),                                        # C = 48
    ('config_RefVSR_small_MFID_8K', 32, 48, 3, 4, 4, {}),                               # HD input
    ('config_RefVSR_small_L1', 32, 48, 5, 4, 2, {}),                                    # x2
    ('config_RefVSR_small_L1', 32, 48, 5, 4, 4, {'result_dtype': 'uint8'}),
    ('config_RefVSR_small_L1', 32, 48, 5, 4, 4, {'weight_precision': 'fp16'}),
    ('config_RefVSR_IR_MFID', 64, 64, 5, 6, 4, {}),                                     # RefVSR_IR
])
def test_engine_u8_equals_float32_dropin_and_pipelined(dev, name, h, w, t, nfr, scale, kw):
    """Sequential drop-in calls (window cache keyed by the byte content) and frame_ids + pipelined calls with input_ready =
    'materialised' and an Event, planar and channels-last bytes: equal to the float32 engine, every frame."""
    lr, rf = _clip(nfr, h, w)
    reset = 3 if nfr >= 6 else 'keep'
    ref_net = _net(name, t, dev, scale, reset, **kw)
    want = _stream(ref_net, lr, rf, t, dev, ['f32'] * nfr)
    for lay in ('planar', 'hwc'):
        got = _stream(_net(name, t, dev, scale, reset, **kw), lr, rf, t, dev, [lay] * nfr)
        _check(want, got, '%s drop-in %s' % (name, lay))
    for ready in ('materialised', 'event'):
        net = _net(name, t, dev, scale, reset, **kw)
        net.Network.set_pipelined(True)
        lay = 'hwc' if ready == 'event' else 'planar'
        got = _stream(net, lr, rf, t, dev, [lay] * nfr, ids=True, ready=ready)
        assert net.Network.engine(0).takes_pipelined_path(list(range(t)))
        _check(want, got, '%s pipelined %s %s' % (name, ready, lay))


def test_engine_u8_with_vis_restart_and_dtype_switch(dev):
    """is_log with save_sample (the vis dict), a reset_branch restart, and a stream whose inputs switch dtype and layout mid-stream
    (contexts of the other kind are cache misses) -- drop-in and frame_ids."""
    name, h, w, t, nfr = 'config_RefVSR_small_L1', 32, 48, 5, 7
    lr, rf = _clip(nfr, h, w, seed=11)
    want = _stream(_net(name, t, dev, reset=3, save_sample=True), lr, rf, t, dev, ['f32'] * nfr, is_log=True)
    got = _stream(_net(name, t, dev, reset=3, save_sample=True), lr, rf, t, dev, ['hwc'] * nfr, is_log=True)
    _check(want, got, 'is_log')
    want = _stream(_net(name, t, dev, reset=3), lr, rf, t, dev, ['f32'] * nfr)
    switch = ['planar', 'planar', 'f32', 'hwc', 'hwc', 'f32', 'planar']
    for ids in (False, True):
        got = _stream(_net(name, t, dev, reset=3), lr, rf, t, dev, switch, ids=ids)
        _check(want, got, 'dtype switch ids=%s' % ids)
    net = _net(name, t, dev, reset=3)
    net.Network.set_pipelined(True)
    _check(want, _stream(net, lr, rf, t, dev, switch, ids=True, ready='materialised'), 'dtype switch pipelined')


def test_forward_group_multimap_and_phases_u8(dev):
    """forward_group (B = 4 after a pipelined first call), n = 2 samples as multi-map launches, phase_a + phase_b and phase_a_group:
    byte windows equal the float32 engine."""
    from refvsr_amd.synth import window_indices
    name, h, w, t, nfr = 'config_RefVSR_small_L1', 32, 48, 5, 5
    lr, rf = _clip(nfr, h, w, seed=21)
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    res = {}
    for lay in ('f32', 'planar', 'hwc'):
        net = _net(name, t, dev)
        net.Network.set_pipelined(True)
        got = [net(_win(lr, wins[0], lay, dev), _win(rf, wins[0], lay, dev), True, frame_ids=wins[0])['result']]
        gl = torch.cat([_win(lr, x, lay, dev) for x in wins[1:]]) if lay != 'hwc' else \
            torch.stack([lr[x].permute(0, 2, 3, 1) for x in wins[1:]]).to(dev).permute(0, 1, 4, 2, 3)
        gr = torch.cat([_win(rf, x, lay, dev) for x in wins[1:]]) if lay != 'hwc' else \
            torch.stack([rf[x].permute(0, 2, 3, 1) for x in wins[1:]]).to(dev).permute(0, 1, 4, 2, 3)
        got += list(net.forward_group(gl, gr, wins[1:])['result'])
        torch.cuda.synchronize()
        res[lay] = [g.clone() for g in got]
    for lay in ('planar', 'hwc'):
        for f in range(nfr):
            assert torch.equal(res['f32'][f], res[lay][f]), 'forward_group %s frame %d' % (lay, f)
    # n = 2: two clips side by side; steady calls run Engine.forward_multi
    lr2, rf2 = _clip(nfr, h, w, seed=22)
    res = {}
    for lay in ('f32', 'hwc', 'planar'):
        net = _net(name, t, dev)
        net.Network.set_pipelined(True)
        outs = []
        for f in range(nfr):
            a = torch.cat([_win(lr, wins[f], lay, dev), _win(lr2, wins[f], lay, dev)])
            b = torch.cat([_win(rf, wins[f], lay, dev), _win(rf2, wins[f], lay, dev)])
            if lay == 'hwc':
                a = torch.stack([x[wins[f]].permute(0, 2, 3, 1) for x in (lr, lr2)]).to(dev).permute(0, 1, 4, 2, 3)
                b = torch.stack([x[wins[f]].permute(0, 2, 3, 1) for x in (rf, rf2)]).to(dev).permute(0, 1, 4, 2, 3)
            outs.append(net(a, b, f == 0, frame_ids=wins[f], input_ready='materialised')['result'].clone())
        torch.cuda.synchronize()
        res[lay] = outs
    for lay in ('planar', 'hwc'):
        for f in range(nfr):
            assert torch.equal(res['f32'][f], res[lay][f]), 'n = 2 %s frame %d' % (lay, f)
    # phase_a + phase_b, and phase_a_group for the steady windows
    res = {}
    for lay in ('f32', 'planar', 'hwc'):
        net = _net(name, t, dev)
        N = net.Network
        outs = []
        for f in range(nfr):
            hs = N.phase_a(_win(lr, wins[f], lay, dev), _win(rf, wins[f], lay, dev), frame_ids=wins[f], first_hint=f == 0)
            outs.append(N.phase_b(hs, f == 0)['result'].clone())
        net2 = _net(name, t, dev)
        N2 = net2.Network
        hs0 = N2.phase_a(_win(lr, wins[0], lay, dev), _win(rf, wins[0], lay, dev), frame_ids=wins[0], first_hint=True)
        outs.append(N2.phase_b(hs0, True)['result'].clone())
        hg = N2.phase_a_group([_win(lr, x, lay, dev)[0] for x in wins[1:]], [_win(rf, x, lay, dev)[0] for x in wins[1:]], wins[1:])
        for k, hh in enumerate(hg):
            outs.append(N2.phase_b(hh, False)['result'].clone())
        torch.cuda.synchronize()
        res[lay] = outs
    for lay in ('planar', 'hwc'):
        for f in range(2 * nfr):
            assert torch.equal(res['f32'][f], res[lay][f]), 'phases %s output %d' % (lay, f)


def test_static_byte_buffer_refilled_in_place(dev):
    """One static uint8 input buffer refilled in place between calls (drop-in: the contexts own byte copies, so the content compare
    is not fooled by the refill; pipelined with frame_ids after a host synchronisation) == fresh buffers."""
    from refvsr_amd.synth import window_indices
    name, h, w, t, nfr = 'config_RefVSR_small_L1', 32, 48, 5, 6
    lr, rf = _clip(nfr, h, w, seed=31)
    want = _stream(_net(name, t, dev, reset=3), lr, rf, t, dev, ['planar'] * nfr)
    for pipelined in (False, True):
        net = _net(name, t, dev, reset=3)
        net.Network.set_pipelined(pipelined)
        A = torch.empty((1, t, h, w, 3), dtype=torch.uint8, device=dev)
        B = torch.empty_like(A)
        got = []
        for f in range(nfr):
            x = window_indices(f, nfr, t)
            A.copy_(lr[x].permute(0, 2, 3, 1)[None])
            B.copy_(rf[x].permute(0, 2, 3, 1)[None])
            kw = {'frame_ids': x} if pipelined else {}
            got.append((net(A.permute(0, 1, 4, 2, 3), B.permute(0, 1, 4, 2, 3), f == 0, **kw)['result'].clone(), {}))
            torch.cuda.synchronize()
        _check(want, got, 'static buffer pipelined=%s' % pipelined)


def test_input_contract_errors(dev):
    """A byte / float mix raises; under input_ready= on the pipelined path unsupported byte strides are refused; forward_group
    accepts bytes and still refuses float16."""
    name, h, w, t = 'config_RefVSR_small_L1', 16, 24, 3
    lr, rf = _clip(3, h, w)
    net = _net(name, t, dev)
    a8, b8 = _win(lr, [0, 1, 2], 'planar', dev), _win(rf, [0, 1, 2], 'planar', dev)
    with pytest.raises(RuntimeError, match='both be uint8 or both float'):
        net(a8, b8.float() / 255, True)
    net.Network.set_pipelined(True)
    odd = torch.empty((1, t, 3, w, h), dtype=torch.uint8, device=dev).transpose(-1, -2)
    odd.copy_(a8)
    with pytest.raises(RuntimeError, match='input_ready'):
        net(odd, odd, True, frame_ids=[0, 1, 2], input_ready='materialised')
    out = net(odd, b8, True, frame_ids=[0, 1, 2])['result']          # input_ready=None: made contiguous on the caller's stream
    assert out.shape == (1, 3, 4 * h, 4 * w)
    with pytest.raises(RuntimeError, match='forward_group'):
        net.forward_group(a8.half(), b8.half(), [[0, 1, 2]])
    with pytest.raises(RuntimeError, match='forward_group'):
        net.forward_group(a8, b8.float(), [[0, 1, 2]])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ evalrun
def test_evalrun_input_dtype_uint8_same_pngs_and_scores(tmp_path):
    """`--input_dtype uint8` on a synthetic dataset (frame_group 1 and 4): the same PNG bytes and the same scores as the float32 run."""
    import make_synth_dataset
    from refvsr_amd import evalrun, get_config, make_state_dict
    root = str(tmp_path / 'ds')
    make_synth_dataset.make(root, clips=2, frames=6, h=32, w=48)
    sd = make_state_dict(get_config('p', 'm', 'config_RefVSR_small_L1'), 1234)
    ck = str(tmp_path / 'ck.pytorch')
    torch.save(sd, ck)
    for group in ('1', '4'):
        res = {}
        for dt in ('float32', 'uint8'):
            cfg = evalrun.build_config(['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', root, '--output_offset',
                                        str(tmp_path / ('o_%s_%s' % (dt, group))), '--frame_num', '5', '--ckpt_abs_name', ck,
                                        '--input_dtype', dt, '--frame_group', group])
            res[dt] = evalrun.evaluate(cfg, log=lambda *_: None)
        assert res['float32']['frames'] == res['uint8']['frames'] == 12
        assert res['float32']['psnr'] == res['uint8']['psnr'] and res['float32']['ssim'] == res['uint8']['ssim']
        for clip in ('0001', '0002'):
            for fr in range(6):
                for kind in ('output', 'input'):
                    p = os.path.join('png', kind, clip, '%04d.png' % fr)
                    a = open(os.path.join(res['float32']['output_root'], p), 'rb').read()
                    b = open(os.path.join(res['uint8']['output_root'], p), 'rb').read()
                    assert a == b, 'PNG %s differs (frame_group %s)' % (p, group)
