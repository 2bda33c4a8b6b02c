"""Y'CbCr 4:2:0 input frames on the device: refvsr_yuv420_to_rgb returns the bits of refvsr_amd/yuv.py:yuv420_to_rgb -- every format,
matrix / range, chroma mode, size class and frame count, frames as they lie in a window (odd address phases), canaries around every
destination -- and every call surface of the engine under config.input_yuv equals the same call on the float32 windows the model makes
from the same buffers, bit for bit.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import yuv_in_cases as yc
from refvsr_amd import yuv

pytestmark = pytest.mark.gpu

FORMATS = yc.FORMATS
MODES = (('bt709', 'limited'), ('bt709', 'full'), ('bt601', 'limited'))
CHROMA = ('bilinear', 'nearest')
# one block | a single block row | a single block column | two row pairs | ragged groups of 2 | rows of 26: a ragged group of 2 behind
# three whole ones, 8-bit row phases 26 y (mod 16) | whole and ragged groups, w % 4 == 2: float2 stores | 270 x 480: w % 8 == 0, float4
# stores, more than one workgroup along y, a last workgroup with two idle waves (135 row pairs)
SIZES = ((2, 2), (2, 4), (4, 2), (4, 4), (6, 10), (18, 26), (34, 70), (270, 480))
PAD = 64                       # canary floats before and after every destination
builtins_range = range


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


_FRAMES = {}


def frames_of(fmt, n, h, w):
    """n seeded frames [n, 3h/2, w] of random codes, with the bits the model ignores set at random (p010: low six, i420p10: high six);
    built once per key and left unchanged."""
    key = (fmt, n, h, w)
    if key not in _FRAMES:
        rs = np.random.RandomState(17 * h + w + 1000 * n + yuv.FORMAT_IDS[fmt])
        x = np.stack([yc.random_codes(rs, h, w, fmt) for _ in builtins_range(n)])
        if fmt == 'p010':
            x = x | rs.randint(0, 64, x.shape).astype(np.uint16)
        if fmt == 'i420p10':
            x = x | (rs.randint(0, 64, x.shape) << 10).astype(np.uint16)
        x.setflags(write=False)
        _FRAMES[key] = x
    return _FRAMES[key]


def convert(srcs, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear'):
    """ops.yuv420_ingest of the cuda frames `srcs` into destinations carved out of one NaN-filled buffer, PAD canary floats before
    and after each; returns the frames [n,3,h,w] (numpy) after checking every canary."""
    from refvsr_amd import ops
    n, fl = len(srcs), 3 * h * w
    buf = torch.full((n, 2 * PAD + fl), float('nan'), dtype=torch.float32, device=srcs[0].device)
    dsts = [buf[i, PAD:PAD + fl].view(3, h, w) for i in builtins_range(n)]
    assert all(d.data_ptr() % 16 == 0 for d in dsts)
    ops.yuv420_ingest(list(zip(srcs, dsts)), fmt, matrix, range, chroma)
    out = buf.cpu().numpy()
    assert np.isnan(out[:, :PAD]).all() and np.isnan(out[:, PAD + fl:]).all(), 'a canary was overwritten'
    return out[:, PAD:PAD + fl].reshape(n, 3, h, w)


def exact(x, dev):
    """One cuda tensor per frame, each allocated exactly (no slack behind the frame inside its own tensor)."""
    return [torch.from_numpy(np.array(f)).to(dev) for f in x]


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), '%s: %d of %d samples differ, first at %s' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# ------------------------------------------------------------------------------------------------ the kernel against the model
@pytest.mark.parametrize('chroma', CHROMA)
@pytest.mark.parametrize('matrix, range', MODES)
@pytest.mark.parametrize('fmt', FORMATS)
def test_kernel_returns_the_models_bits(dev, fmt, matrix, range, chroma):
    for h, w in SIZES:
        n = 3 if h * w < 10000 else 1
        x = frames_of(fmt, n, h, w)
        got = convert(exact(x, dev), h, w, fmt, matrix, range, chroma)
        same_bits(got, yuv.yuv420_to_rgb(x, h, w, fmt, matrix, range, chroma), '%s %s %s %s %d x %d' % (fmt, matrix, range, chroma, h, w))


@pytest.mark.parametrize('fmt', FORMATS)
def test_crafted_cases(dev, fmt):
    """The case sets of tests/yuv_in_cases.py (every code of every plane, in-gamut frames, dirty bits) and the anchors."""
    for name, _, h, w, buf in yc.cases(fmt):
        got = convert(exact(buf[None], dev), h, w, fmt)
        same_bits(got[0], yuv.yuv420_to_rgb(buf, h, w, fmt), '%s %s' % (fmt, name))
    s = 2 ** (yuv.depth_of(fmt) - 8)
    x = np.stack([yc.constant_frame([c * s for c in code], fmt) for code, _ in yc.ANCHORS])
    got = convert(exact(x, dev), 4, 4, fmt)
    same_bits(got, yuv.yuv420_to_rgb(x, 4, 4, fmt), '%s anchors' % fmt)
    assert got[0].max() == 0.0 and got[1].min() == 1.0


@pytest.mark.parametrize('n', [1, 3, 16, 17])
@pytest.mark.parametrize('fmt', FORMATS)
def test_frame_counts(dev, fmt, n):
    """1, 3, 16 frames in one launch, 17 in two: every frame its own content."""
    from refvsr_amd import hip, ops
    calls = []
    lib = hip.lib()
    real = lib.refvsr_yuv420_to_rgb

    class Counting(object):
        def __getattr__(self, k):
            if k == 'refvsr_yuv420_to_rgb':
                return lambda *a: (calls.append(a[2]), real(*a))[1]
            return getattr(lib, k)
    h, w = 18, 26
    x = frames_of(fmt, n, h, w)
    mp = pytest.MonkeyPatch()
    mp.setattr(hip, 'lib', lambda: Counting())
    try:
        got = convert(exact(x, dev), h, w, fmt)
    finally:
        mp.undo()
    assert calls == ([n] if n <= 16 else [16, n - 16])
    same_bits(got, yuv.yuv420_to_rgb(x, h, w, fmt), '%s %d frames' % (fmt, n))


@pytest.mark.parametrize('fmt', FORMATS)
def test_full_hd_frame(dev, fmt):
    """One 1080 x 1920 frame (the 8K configs' input size): 540 x 240 work items, offsets beyond 2^21 samples."""
    h, w = 1080, 1920
    x = frames_of(fmt, 1, h, w)
    got = convert(exact(x, dev), h, w, fmt)
    same_bits(got, yuv.yuv420_to_rgb(x, h, w, fmt), '%s 1080 x 1920' % fmt)


# ------------------------------------------------------------------------------------------------ frames as they lie in a window
@pytest.mark.parametrize('fmt', ['nv12', 'i420'])
def test_frames_of_a_window_have_odd_phases(dev, fmt):
    """A [5, 27, 26] 8-bit window: frames 702 bytes apart, so their address phases (mod 16) are 0, 14, 12, 10, 8."""
    x = frames_of(fmt, 5, 18, 26)
    win = torch.from_numpy(np.array(x)).to(dev)
    assert win.stride(0) == 702 and sorted(set(win[i].data_ptr() % 16 for i in builtins_range(5))) == [0, 8, 10, 12, 14]
    got = convert([win[i] for i in builtins_range(5)], 18, 26, fmt)
    same_bits(got, yuv.yuv420_to_rgb(x, 18, 26, fmt), '%s window' % fmt)


@pytest.mark.parametrize('fmt, offsets', [('nv12', (1, 2, 3, 5, 15)), ('i420', (1, 2, 3, 5, 15)), ('p010', (2, 6, 14)), ('i420p10', (2, 6, 14))])
def test_sources_at_byte_offsets(dev, fmt, offsets):
    """Sources sliced from a byte buffer at the given offsets; the buffer ends with the frame (no slack behind it)."""
    for h, w in ((6, 10), (18, 26), (34, 80)):
        x = frames_of(fmt, len(offsets), h, w)
        nb = yuv.frame_bytes(h, w, fmt)
        srcs = []
        for f, off in zip(x, offsets):
            raw = torch.zeros(off + nb, dtype=torch.uint8, device=dev)
            assert raw.data_ptr() % 16 == 0
            raw[off:].copy_(torch.from_numpy(np.array(f).view(np.uint8).reshape(-1)).to(dev))
            s = raw[off:]
            srcs.append((s if f.dtype == np.uint8 else s.view(torch.uint16)).view(3 * h // 2, w))
            assert srcs[-1].data_ptr() % 16 == off
        got = convert(srcs, h, w, fmt)
        same_bits(got, yuv.yuv420_to_rgb(x, h, w, fmt), '%s offsets %s at %d x %d' % (fmt, offsets, h, w))


# ------------------------------------------------------------------------------------------------ ops
def test_ops_and_torch_op_return_the_same_tensors(dev):
    from refvsr_amd import ops
    import refvsr_amd.torch_ops  # noqa: F401
    for fmt in FORMATS:
        x = frames_of(fmt, 5, 18, 26)
        t = torch.from_numpy(np.array(np.stack([x, x[::-1]]))).to(dev)                  # [2, 5, 27, 26]
        a = ops.yuv420_to_frames(t, 18, 26, fmt, 'bt601', 'full', 'nearest')
        b = torch.ops.refvsr.yuv420_to_rgb(t, 18, 26, fmt, 'bt601', 'full', 'nearest')
        assert a.shape == (2, 5, 3, 18, 26) and a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, b)
        same_bits(a[0].cpu().numpy(), yuv.yuv420_to_rgb(x, 18, 26, fmt, 'bt601', 'full', 'nearest'), 'ops %s' % fmt)
        one = ops.yuv420_to_frames(t[1, 2], 18, 26, fmt)
        same_bits(one.cpu().numpy(), yuv.yuv420_to_rgb(x[::-1][2], 18, 26, fmt), 'ops %s one frame' % fmt)
        # other strides are copied first
        wide = np.zeros((5, 27, 52), dtype=x.dtype)
        wide[..., ::2] = x
        strided = torch.from_numpy(wide).to(dev)[..., ::2]
        assert not strided.is_contiguous()
        same_bits(ops.yuv420_to_frames(strided, 18, 26, fmt).cpu().numpy(), yuv.yuv420_to_rgb(x, 18, 26, fmt), 'ops %s strided' % fmt)
    with pytest.raises(RuntimeError, match='yuv420_to_frames'):
        ops.yuv420_to_frames(t, 18, 26, 'nv12')
    with pytest.raises(RuntimeError, match='yuv420_to_frames'):
        ops.yuv420_to_frames(t, 18, 24, 'i420p10')
    u8 = torch.from_numpy(np.array(frames_of('nv12', 5, 18, 26))).to(dev)
    torch.library.opcheck(torch.ops.refvsr.yuv420_to_rgb, (u8, 18, 26, 'nv12', 'bt709', 'limited', 'bilinear'), test_utils=('test_schema', 'test_faketensor'))
    # the content compare takes 16-bit frames through their bytes
    x = frames_of('p010', 3, 18, 26)
    y = x.copy()
    y[1, 26, 25] ^= 0x100
    a, b = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(y).to(dev)
    assert ops.bytes_equal([(a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[1], a[1].clone())]) == [True, False, True, True]


# ------------------------------------------------------------------------------------------------ through the engine
def make_net(name, t, dev, input_yuv=None, pipelined=False, n_engines=1, **cfg_kw):
    from refvsr_amd import SRNet, get_config, make_state_dict
    cfg = get_config('p', 'm', name)
    cfg.frame_num, cfg.save_sample = t, False
    if input_yuv is not None:
        cfg.input_yuv, cfg.input_yuv_matrix, cfg.input_yuv_range, cfg.input_yuv_chroma = input_yuv
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234))
    if pipelined:
        net.Network.ensure_engines(n_engines, dev)
        net.Network.set_pipelined(True)
    return net


_CLIPS = {}


def clip(nfr, h, w, t, kind, seed=21):
    """A synthetic clip as 4:2:0 frames of `kind` = (fmt, matrix, range, chroma) and as the float32 frames the model decodes from
    them: (lr yuv [nfr, 3h/2, w], ref yuv, lr float32 [nfr,3,h,w], ref float32, windows); numpy, built once, left unchanged."""
    from refvsr_amd.synth import make_clip, window_indices
    key = (nfr, h, w, t, kind, seed)
    if key not in _CLIPS:
        fmt, matrix, range, chroma = kind
        lr, rf, _ = make_clip(nfr, h, w, seed=seed, want_gt=False)
        ys = [yuv.rgb_to_yuv420(x.numpy(), fmt, matrix, range) for x in (lr, rf)]
        fs = [yuv.yuv420_to_rgb(y, h, w, fmt, matrix, range, chroma) for y in ys]
        for a in ys + fs:
            a.setflags(write=False)
        _CLIPS[key] = (ys[0], ys[1], fs[0], fs[1], [window_indices(f, nfr, t) for f in builtins_range(nfr)])
    return _CLIPS[key]


def win(x, idx, dev):
    """Window(s) `idx` of the clip x as a cuda tensor: a list of indices -> [1, t, ...], a list of lists -> [B, t, ...]."""
    return torch.from_numpy(np.array(x[np.array(idx)])).to(dev) if isinstance(idx[0], list) else \
        torch.from_numpy(np.array(x[np.array(idx)][None])).to(dev)


K709 = ('nv12', 'bt709', 'limited', 'bilinear')


def both(name, t, dev, kind, **kw):
    return make_net(name, t, dev, kind, **kw), make_net(name, t, dev, None, **kw)


def equal_results(a, b, what):
    ra, rb = a['result'], b['result']
    if isinstance(ra, tuple):
        assert len(ra) == len(rb)
        ra, rb = torch.cat(list(ra)), torch.cat(list(rb))
    assert ra.shape == rb.shape and ra.dtype == rb.dtype and torch.equal(ra, rb), '%s: the results differ' % what
    assert sorted(a.keys()) == sorted(b.keys())
    if 'eval_vis' in a:
        for va, vb in zip(a['eval_vis'], b['eval_vis']):
            assert sorted(va) == sorted(vb) and all(torch.equal(va[k], vb[k]) for k in va), '%s: the confidence maps differ' % what


@pytest.mark.parametrize('kind', [K709, ('i420', 'bt601', 'full', 'nearest'), ('p010', 'bt709', 'full', 'bilinear'),
                                  ('i420p10', 'bt601', 'limited', 'bilinear')])
def test_engine_forward(dev, kind):
    nfr, t, h, w = 3, 3, 16, 24
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind)
    for f, wi in enumerate(wins):
        a = ynet(win(ly, wi, dev), win(ry, wi, dev), f == 0)
        b = fnet(win(lf, wi, dev), win(rf, wi, dev), f == 0)
        assert a['result'].shape == (1, 3, 4 * h, 4 * w)
        equal_results(a, b, 'forward %s frame %d' % (kind[0], f))


def test_engine_forward_at_18_x_26_with_five_frames(dev):
    nfr, t, h, w = 3, 5, 18, 26
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, K709)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, K709)
    for f, wi in enumerate(wins):
        a = ynet(win(ly, wi, dev), win(ry, wi, dev), f == 0)
        b = fnet(win(lf, wi, dev), win(rf, wi, dev), f == 0)
        equal_results(a, b, 'forward 18 x 26 frame %d' % f)


@pytest.mark.parametrize('pipelined', [False, True])
def test_engine_two_samples_in_one_call(dev, pipelined):
    nfr, t, h, w = 3, 3, 16, 24
    kind = ('p010', 'bt709', 'limited', 'bilinear')
    c0, c1 = clip(nfr, h, w, t, kind), clip(nfr, h, w, t, kind, seed=22)
    kw = dict(pipelined=True, n_engines=2) if pipelined else {}
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind, **kw)
    for f, wi in enumerate(c0[4]):
        ids = {'frame_ids': wi, 'input_ready': 'materialised'} if pipelined else {}
        ya, yb, fa, fb = (torch.from_numpy(np.stack([c0[k][np.array(wi)], c1[k][np.array(wi)]])).to(dev) for k in (0, 1, 2, 3))
        torch.cuda.synchronize()
        a, b = ynet(ya, yb, f == 0, **ids), fnet(fa, fb, f == 0, **ids)
        assert a['result'].shape == (2, 3, 4 * h, 4 * w)
        equal_results(a, b, 'n = 2 pipelined=%s frame %d' % (pipelined, f))
    torch.cuda.synchronize()


@pytest.mark.parametrize('ids', [False, True])
def test_engine_stream_of_seven_frames(dev, ids):
    """Sequential mode: the window cache keyed by the content of the source bytes (ids=False) or by frame ids."""
    nfr, t, h, w = 7, 3, 16, 24
    kind = ('i420', 'bt709', 'limited', 'bilinear')
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind, reset_branch=3)
    for f, wi in enumerate(wins):
        kw = {'frame_ids': wi} if ids else {}
        a = ynet(win(ly, wi, dev), win(ry, wi, dev), f == 0, **kw)
        b = fnet(win(lf, wi, dev), win(rf, wi, dev), f == 0, **kw)
        equal_results(a, b, 'stream ids=%s frame %d' % (ids, f))


def test_engine_pipelined_materialised(dev):
    nfr, t, h, w = 7, 3, 16, 24
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, K709)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, K709, pipelined=True)
    assert ynet.Network.engine(0).takes_pipelined_path(list(builtins_range(t)))
    outs = {}
    for tag, net, l, r in (('yuv', ynet, ly, ry), ('f32', fnet, lf, rf)):
        clipl, clipr = torch.from_numpy(np.array(l)).to(dev), torch.from_numpy(np.array(r)).to(dev)
        ws = [(clipl[wi][None].contiguous(), clipr[wi][None].contiguous()) for wi in wins]
        torch.cuda.synchronize()
        outs[tag] = [net(a, b, f == 0, frame_ids=wins[f], input_ready='materialised')['result'].clone() for f, (a, b) in enumerate(ws)]
        torch.cuda.synchronize()
    for f in builtins_range(nfr):
        assert torch.equal(outs['yuv'][f], outs['f32'][f]), 'pipelined frame %d' % f


@pytest.mark.parametrize('want_conf', [False, True])
def test_engine_forward_group(dev, want_conf):
    nfr, t, h, w = 5, 3, 16, 24
    kind = ('i420p10', 'bt709', 'limited', 'bilinear')
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind, pipelined=True)
    kw = {'want_conf': True} if want_conf else {}
    for tag, net, l, r in (('yuv', ynet, ly, ry), ('f32', fnet, lf, rf)):
        first = net.forward_group(win(l, wins[:1], dev), win(r, wins[:1], dev), wins[:1], is_first_frame=True, **kw)
        rest = net.forward_group(win(l, wins[1:], dev), win(r, wins[1:], dev), wins[1:], **kw)          # B = 4, steady state
        torch.cuda.synchronize()
        if tag == 'yuv':
            got = (first, rest)
    assert len(got[1]['result']) == 4 and ('eval_vis' in got[1]) == want_conf
    equal_results(got[0], first, 'forward_group first')
    equal_results(got[1], rest, 'forward_group B = 4 want_conf=%s' % want_conf)


def test_engine_phases(dev):
    """phase_a + phase_b frame by frame, and phase_a_group for the steady windows."""
    nfr, t, h, w = 4, 3, 16, 24
    kind = ('nv12', 'bt601', 'limited', 'nearest')
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    res = {}
    for tag, k, l, r in (('yuv', kind, ly, ry), ('f32', None, lf, rf)):
        N = make_net('config_RefVSR_small_L1', t, dev, k).Network
        outs = []
        for f in builtins_range(nfr):
            hs = N.phase_a(win(l, wins[f], dev), win(r, wins[f], dev), frame_ids=wins[f], first_hint=f == 0)
            outs.append(N.phase_b(hs, f == 0)['result'].clone())
        N2 = make_net('config_RefVSR_small_L1', t, dev, k).Network
        hs0 = N2.phase_a(win(l, wins[0], dev), win(r, wins[0], dev), frame_ids=wins[0], first_hint=True)
        outs.append(N2.phase_b(hs0, True)['result'].clone())
        hg = N2.phase_a_group(list(win(l, wins[1:], dev)), list(win(r, wins[1:], dev)), wins[1:])
        for hh in hg:
            outs.append(N2.phase_b(hh, False)['result'].clone())
        torch.cuda.synchronize()
        res[tag] = outs
    assert len(res['yuv']) == 2 * nfr
    for i, (a, b) in enumerate(zip(res['yuv'], res['f32'])):
        assert torch.equal(a, b), 'phases output %d' % i


def test_engine_ir_configuration(dev):
    nfr, t, h, w = 2, 5, 64, 64
    kind = ('p010', 'bt709', 'limited', 'bilinear')
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    ynet, fnet = both('config_RefVSR_IR_L1', t, dev, kind)
    for f, wi in enumerate(wins):
        a = ynet(win(ly, wi, dev), win(ry, wi, dev), f == 0)
        b = fnet(win(lf, wi, dev), win(rf, wi, dev), f == 0)
        equal_results(a, b, 'RefVSR_IR frame %d' % f)


def counted(mp):
    """ops.yuv420_ingest wrapped: the list of the frame counts of its calls (one call = one launch up to 16 frames)."""
    from refvsr_amd import ops
    calls = []
    real = ops.yuv420_ingest
    mp.setattr(ops, 'yuv420_ingest', lambda pairs, *a, **k: (calls.append(len(pairs)), real(pairs, *a, **k))[1])
    return calls


def test_launch_counts(dev, monkeypatch):
    """One launch per call over the call's new frames only: 2 t frames for a first frame, 2 (one lr, one ref) for a steady call of the
    id-keyed stream, 8 for a steady group of four."""
    nfr, t, h, w = 9, 3, 16, 24
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, K709)
    calls = counted(monkeypatch)
    net = make_net('config_RefVSR_small_L1', t, dev, K709)
    for f in builtins_range(4):
        net(win(ly, wins[f], dev), win(ry, wins[f], dev), f == 0, frame_ids=wins[f])
    # window 0 is [0, 0, 1]: two distinct frames, lr and ref each
    assert calls == [4, 2, 2, 2], calls
    del calls[:]
    net = make_net('config_RefVSR_small_L1', t, dev, K709)
    net(win(ly, [0, 1, 2], dev), win(ry, [0, 1, 2], dev), True, frame_ids=[0, 1, 2])
    assert calls == [2 * t], calls
    del calls[:]
    net = make_net('config_RefVSR_small_L1', t, dev, K709, pipelined=True)
    net.forward_group(win(ly, wins[:1], dev), win(ry, wins[:1], dev), wins[:1], is_first_frame=True)
    net.forward_group(win(ly, wins[1:5], dev), win(ry, wins[1:5], dev), wins[1:5])
    net.forward_group(win(ly, wins[5:9], dev), win(ry, wins[5:9], dev), wins[5:9])
    torch.cuda.synchronize()
    # the first group brings frames 2 .. 5 (window 0 held 0 and 1), the second frames 6 .. 8 (window 8 repeats the clip's last frame)
    assert calls == [4, 8, 6], calls


def test_off_means_no_new_code_runs(dev, monkeypatch):
    nfr, t, h, w = 3, 3, 16, 24
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, K709)
    calls = counted(monkeypatch)
    net = make_net('config_RefVSR_small_L1', t, dev, None)
    for f, wi in enumerate(wins):
        net(win(lf, wi, dev), win(rf, wi, dev), f == 0, frame_ids=wi)
    u8 = lambda x, wi: (win(x, wi, dev) * 255).round().to(torch.uint8)
    net(u8(lf, wins[0]), u8(rf, wins[0]), True)
    assert calls == []


def test_engine_refusals(dev):
    t, h, w = 3, 16, 24
    ly, ry, lf, rf, wins = clip(3, h, w, t, K709)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, K709)
    a, b = win(ly, wins[0], dev), win(ry, wins[0], dev)
    expect = r"input_yuv = 'nv12'.*torch.uint8 \[n, t, 3h/2, w\]"
    with pytest.raises(RuntimeError, match=expect):
        ynet(win(lf, wins[0], dev), win(rf, wins[0], dev), True)                       # a 5-D RGB window
    with pytest.raises(RuntimeError, match=expect):
        ynet(win(ly.astype(np.uint16), wins[0], dev), win(ry.astype(np.uint16), wins[0], dev), True)      # a wrong dtype
    with pytest.raises(RuntimeError, match=expect):
        ynet(a[:, :, :23].contiguous(), b[:, :, :23].contiguous(), True)             # 23 rows: not 3h/2
    wide = torch.zeros(1, t, 24, 2 * w, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='not contiguous'):
        ynet(wide[..., ::2], wide[..., ::2], True)
    with pytest.raises(RuntimeError, match=r"input_yuv = 'nv12'.*\[B, t, 3h/2, w\]"):
        ynet.forward_group(win(lf, wins[:2], dev), win(rf, wins[:2], dev), wins[:2])
    with pytest.raises(RuntimeError, match='need config.input_yuv'):
        fnet(a, b, True)                                                              # a YUV-shaped window without input_yuv
    eng = fnet.Network.ensure_engines(1, dev)[0]
    with pytest.raises(RuntimeError, match='need config.input_yuv'):
        eng.forward(a[0], b[0], True)
    for field, bad in (('input_yuv', 'yv12'), ('input_yuv_matrix', 'bt2020'), ('input_yuv_range', 'pc'), ('input_yuv_chroma', 'bicubic')):
        kw = {'input_yuv': (bad, 'bt709', 'limited', 'bilinear')} if field == 'input_yuv' else {field: bad}      # (the other fields: while off)
        net = make_net('config_RefVSR_small_L1', t, dev, **kw)
        with pytest.raises(ValueError):
            net.Network.ensure_engines(1, dev)


# ------------------------------------------------------------------------------------------------ videorun
@pytest.mark.parametrize('depth', [8, 10])
def test_videorun_writes_the_models_bytes(dev, tmp_path, depth):
    """8-frame 16 x 24 .y4m pairs: the output file holds rgb_to_yuv420 of the float32 engine's results on the modelled inputs."""
    from refvsr_amd import get_config, videorun
    fmt = 'i420' if depth == 8 else 'i420p10'
    nfr, t, h, w, G = 8, 3, 16, 24, 4
    kind = (fmt, 'bt709', 'limited', 'bilinear')
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    paths = []
    for name, x in (('uw', ly), ('w', ry)):
        paths.append(str(tmp_path / ('%s.y4m' % name)))
        with yuv.Y4MWriter(paths[-1], h, w, fmt, (24, 1), 'limited') as wr:
            for f in x:
                wr.write(f)
    out = str(tmp_path / 'sr.y4m')
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.save_sample = t, False
    cfg.EVAL.frame_group = G
    net = make_net('config_RefVSR_small_L1', t, dev, kind, result_yuv=fmt)
    n, seconds = videorun.run(cfg, paths[0], paths[1], out, net=net)
    assert n == nfr and seconds > 0 and (cfg.input_yuv, cfg.result_yuv) == (fmt, fmt)
    fnet = make_net('config_RefVSR_small_L1', t, dev, None, pipelined=True)
    want = []
    for f0 in builtins_range(0, nfr, G):
        r = fnet.forward_group(win(lf, wins[f0:f0 + G], dev), win(rf, wins[f0:f0 + G], dev), wins[f0:f0 + G], is_first_frame=f0 == 0)['result']
        want += [yuv.rgb_to_yuv420(x[0].cpu().numpy(), fmt) for x in r]
    got = yuv.read_y4m(out)
    assert (got['h'], got['w'], got['fps'], got['fmt'], got['range']) == (4 * h, 4 * w, (24, 1), fmt, 'limited') and len(got['frames']) == nfr
    for f in builtins_range(nfr):
        assert np.array_equal(got['frames'][f], want[f]), 'frame %d of the output file' % f
    # mismatching files are refused
    short = str(tmp_path / 'short.y4m')
    with yuv.Y4MWriter(short, h, w, fmt, (24, 1)) as wr:
        for f in ry[:5]:
            wr.write(f)
    with pytest.raises(ValueError, match='frame count differs'):
        videorun.run(cfg, paths[0], short, out, net=net)
    other = str(tmp_path / 'other.y4m')
    with yuv.Y4MWriter(other, h, w + 2, fmt, (24, 1)) as wr:
        for _ in builtins_range(nfr):
            wr.write(np.zeros((3 * h // 2, w + 2), dtype=ly.dtype))
    with pytest.raises(ValueError, match='geometry differs'):
        videorun.run(cfg, paths[0], other, out, net=net)
