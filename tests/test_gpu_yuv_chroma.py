"""4:2:2, 4:4:4 and left-sited 4:2:0 frames on the device: refvsr_yuv_to_rgb and refvsr_result_to_yuv return the bits of the numpy models
refvsr_amd/yuv.py:yuv_to_rgb and rgb_to_yuv for every valid (format, siting), matrix / range, chroma mode, source form, size class and
frame count; canaries surround every destination; with 4:2:0 / centre both equal the 4:2:0 entry points bit for bit; the engine's call
surfaces under the new input formats equal the same calls on the float32 windows the model decodes, and 'yuv' in the new forms is the
model applied to 'result'.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import yuv_chroma_cases as cc
from refvsr_amd import yuv

pytestmark = pytest.mark.gpu

MODES = cc.MODES
CHROMA = ('bilinear', 'nearest')
# single sample | one row | one column | a ragged group | odd address phases inside a window | whole and ragged groups, w % 4 == 2 |
# more than one workgroup along y | 4 x 1040.  The way in: a workgroup spans 64 groups of 8 = 512 pixels of a row, so 1040 columns
# cross two workgroup edges and end in a ragged workgroup: the right neighbour of left siting (cxr) is read across both.  The way out:
# a workgroup is 256 consecutive groups of 8 (float sources) or 16 (byte sources) pixels in raster order, so its edges fall inside
# rows: at 4 x 1040 after group 256 of 260 (float, 130 groups a row) and, for the one-row samplings, of 260 byte groups; 4:2:0 byte
# sources have 130 groups there (one workgroup) and meet their workgroup edges at 270 x 480 (30 groups a row pair, 4050 in all).
SIZES = cc.SIZES
PAD = 64                       # canary floats (the way in) / bytes x 4 (the way out) before and after every destination
CANARY = 0xA5
SRC_FORMS = tuple((dt, lay) for dt in ('float32', 'float16', 'uint8') for lay in ('chw', 'hwc'))
builtins_range = range


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


_FRAMES, _RGB = {}, {}


def frames_of(fmt, n, h, w):
    """n seeded frames of random codes, the ignored bits of 10-bit samples set at random; built once per key, left unchanged."""
    key = (fmt, n, h, w)
    if key not in _FRAMES:
        rs = np.random.RandomState(17 * h + w + 1000 * n + len(fmt))
        x = np.stack([cc.random_codes(rs, h, w, fmt) for _ in builtins_range(n)])
        x.setflags(write=False)
        _FRAMES[key] = x
    return _FRAMES[key]


def rgb_of(n, h, w, dt):
    """n seeded results [n,3,h,w] of numpy type dt, one set per geometry."""
    key = (n, h, w, dt)
    if key not in _RGB:
        x64 = np.random.RandomState(1000 * h + w + n).rand(n, 3, h, w)
        _RGB[key] = np.rint(255.0 * x64).astype(np.uint8) if dt == 'uint8' else x64.astype(dt)
        _RGB[key].setflags(write=False)
    return _RGB[key]


def exact(x, dev):
    """One cuda tensor per frame, each allocated exactly (no slack behind the frame inside its own tensor)."""
    return [torch.from_numpy(np.array(f)).to(dev) for f in x]


def channels_last(x):
    return x.movedim(-3, -1).contiguous().movedim(-1, -3)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), '%s: %d of %d samples differ, first at %s' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def same_codes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got != want
    assert not bad.any(), '%s: %d of %d samples differ, first at %s' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def convert_in(srcs, h, w, fmt, siting, matrix='bt709', range='limited', chroma='bilinear'):
    """ops.yuv_ingest of the cuda frames `srcs` into destinations carved out of one NaN-filled buffer, PAD canary floats before and after
    each; returns the frames [n,3,h,w] (numpy) after checking every canary."""
    from refvsr_amd import ops
    n, fl = len(srcs), 3 * h * w
    buf = torch.full((n, 2 * PAD + fl), float('nan'), dtype=torch.float32, device=srcs[0].device)
    dsts = [buf[i, PAD:PAD + fl].view(3, h, w) for i in builtins_range(n)]
    assert all(d.data_ptr() % 16 == 0 for d in dsts)
    ops.yuv_ingest(list(zip(srcs, dsts)), fmt, matrix, range, chroma, siting)
    out = buf.cpu().numpy()
    assert np.isnan(out[:, :PAD]).all() and np.isnan(out[:, PAD + fl:]).all(), 'a canary was overwritten'
    return out[:, PAD:PAD + fl].reshape(n, 3, h, w)


def convert_out(frames, fmt, siting, matrix='bt709', range='limited', offset=0):
    """refvsr_result_to_yuv of the cuda results `frames` ([3,h,w] each, one dtype and layout) into destinations carved out of one
    canary-filled byte buffer at `offset` samples past a 256-byte boundary (sample-aligned only for offset != 0); returns the frames
    (numpy, the model's shape and type) after checking every canary byte."""
    from refvsr_amd import hip, ops
    P = ctypes.c_void_p
    f0 = frames[0]
    _, h, w = f0.shape
    n = len(frames)
    es = 1 if yuv.depth_of(fmt) == 8 else 2
    nbytes = hip.lib().refvsr_yuv_frame_bytes(h, w, yuv.FORMAT_IDS[yuv.twin_of(fmt)], yuv.SAMPLINGS[yuv.sampling_of(fmt)])
    assert nbytes == yuv.frame_bytes(h, w, fmt)
    lead = 256 + offset * es
    pitch = (lead + nbytes + 256 + 255) // 256 * 256
    buf = torch.full((n, pitch), CANARY, dtype=torch.uint8, device=f0.device)
    assert buf.data_ptr() % 256 == 0
    sfmt = {torch.float32: hip.RESULT_F32, torch.float16: hip.RESULT_F16, torch.uint8: hip.RESULT_U8}[f0.dtype]
    if not f0.is_contiguous():
        sfmt |= hip.RESULT_HWC
    coef = (ctypes.c_double * 9)(*yuv.coefficients(fmt, matrix, range))
    rc = hip.lib().refvsr_result_to_yuv((P * n)(*[f.data_ptr() for f in frames]), sfmt, (P * n)(*[buf[i].data_ptr() + lead for i in builtins_range(n)]),
                                        n, h, w, yuv.FORMAT_IDS[yuv.twin_of(fmt)], yuv.SAMPLINGS[yuv.sampling_of(fmt)], yuv.SITINGS[siting], coef,
                                        ops._stream())
    assert rc == 0, hip.lib().refvsr_last_error()
    out = buf.cpu().numpy()
    assert (out[:, :lead] == CANARY).all() and (out[:, lead + nbytes:] == CANARY).all(), 'a canary byte was overwritten'
    return np.stack([out[i, lead:lead + nbytes].copy().view(yuv.dtype_of(fmt)).reshape(yuv.frame_shape(h, w, fmt)) for i in builtins_range(n)])


def results_on(dev, n, h, w, dt, lay):
    """(numpy results [n,3,h,w], one separately allocated cuda tensor per frame in layout lay)."""
    src = rgb_of(n, h, w, dt)
    ts = [torch.from_numpy(np.array(f)).to(dev) for f in src]
    return src, ts if lay == 'chw' else [channels_last(t) for t in ts]


# ------------------------------------------------------------------------------------------------ the way in
@pytest.mark.parametrize('chroma', CHROMA)
@pytest.mark.parametrize('matrix, range', MODES)
@pytest.mark.parametrize('fmt, siting', cc.PAIRS)
def test_yuv_to_rgb_returns_the_models_bits(dev, fmt, siting, matrix, range, chroma):
    for h, w in SIZES:
        n = 3 if h * w < 10000 else 1
        x = frames_of(fmt, n, h, w)
        got = convert_in(exact(x, dev), h, w, fmt, siting, matrix, range, chroma)
        same_bits(got, yuv.yuv_to_rgb(x, h, w, fmt, matrix, range, chroma, siting), '%s %s %s %s %s %d x %d' % (fmt, siting, matrix, range, chroma, h, w))


@pytest.mark.parametrize('fmt', ['i422', 'i444', 'nv12'])
def test_frames_of_a_window_have_odd_phases(dev, fmt):
    """A [5, rows, 26] 8-bit window at 18 x 26: frames 702 (4:2:0), 936 (4:2:2) or 1404 (4:4:4) bytes apart."""
    x = frames_of(fmt, 5, 18, 26)
    win = torch.from_numpy(np.array(x)).to(dev)
    assert len(set(win[i].data_ptr() % 16 for i in builtins_range(5))) > 1
    got = convert_in([win[i] for i in builtins_range(5)], 18, 26, fmt, 'left')
    same_bits(got, yuv.yuv_to_rgb(x, 18, 26, fmt, siting='left'), '%s window' % fmt)


def test_in_controls_are_visible_on_the_device(dev):
    rs = np.random.RandomState(3)
    for control, fmt, siting in cc.IN_CONTROLS:
        h, w = 6, 10
        buf = cc.random_codes(rs, h, w, fmt)
        got = convert_in(exact(buf[None], dev), h, w, fmt, siting)[0]
        same_bits(got, yuv.yuv_to_rgb(buf, h, w, fmt, siting=siting), control)
        same_bits(got, cc.in_control(None, buf, h, w, fmt, siting), control)
        assert not np.array_equal(got, cc.in_control(control, buf, h, w, fmt, siting)), control


# ------------------------------------------------------------------------------------------------ the way out
@pytest.mark.parametrize('dt, lay', SRC_FORMS)
@pytest.mark.parametrize('fmt, siting', cc.PAIRS)
def test_result_to_yuv_returns_the_models_bits(dev, fmt, siting, dt, lay):
    """Every size under each of the three matrix / range pairs, destinations 256-byte aligned; the small sizes also at 1 and 3 samples
    past that (the pair changing with the size: the coefficients move no address)."""
    for k, (h, w) in enumerate(SIZES):
        n = 3 if h * w < 10000 else 1
        src, ts = results_on(dev, n, h, w, dt, lay)
        for m, (matrix, range) in enumerate(MODES):
            want = yuv.rgb_to_yuv(src, fmt, matrix, range, siting)
            for offset in (0, 1, 3) if h * w < 10000 and m == k % 3 else (0,):
                got = convert_out(ts, fmt, siting, matrix, range, offset)
                same_codes(got, want, '%s %s %s %s %s %s %d x %d +%d' % (fmt, siting, dt, lay, matrix, range, h, w, offset))


def test_ties_and_controls(dev):
    """The crafted ties of tests/yuv_chroma_cases.py (bt709, full range; at least two round down) and the wrong-model controls."""
    down = 0
    for fmt, siting, frame, plane, rounds_down in cc.tie_cases():
        assert cc.tie_mask(frame, fmt, siting, plane)[:, -1].any()
        for t in (torch.from_numpy(frame).to(dev), channels_last(torch.from_numpy(frame).to(dev))):
            same_codes(convert_out([t], fmt, siting, 'bt709', 'full')[0], yuv.rgb_to_yuv(frame, fmt, 'bt709', 'full', siting), 'tie %s %s' % (fmt, siting))
        down += bool(rounds_down)
    assert down >= 2
    for control, frame, fmt, siting in cc.out_controls():
        got = convert_out([torch.from_numpy(frame).to(dev)], fmt, siting, 'bt709', 'full')[0]
        same_codes(got, yuv.rgb_to_yuv(frame, fmt, 'bt709', 'full', siting), control)
        assert not np.array_equal(got, cc.out_control(control, frame, fmt, siting)), control


# ------------------------------------------------------------------------------------------------ bit-identity and launch counts
@pytest.mark.parametrize('fmt', ['nv12', 'i420', 'p010', 'i420p10'])
def test_420_centre_is_the_old_entry_points(dev, fmt):
    from refvsr_amd import ops
    for h, w in ((6, 10), (34, 70)):
        x = frames_of(fmt, 3, h, w)
        t = torch.from_numpy(np.array(x)).to(dev)
        for chroma in CHROMA:
            assert torch.equal(ops.yuv_to_frames(t, h, w, fmt, 'bt601', 'full', chroma, 'centre'), ops.yuv420_to_frames(t, h, w, fmt, 'bt601', 'full', chroma))
        for dt, lay in SRC_FORMS:
            _, ts = results_on(dev, 3, h, w, dt, lay)
            assert torch.equal(ops.result_to_yuv(ts, fmt, 'bt601', 'full', 'centre').view(torch.uint8), ops.result_to_yuv420(ts, fmt, 'bt601', 'full').view(torch.uint8))


def counting_lib(mp, names):
    """hip.lib() wrapped: the frame counts of the calls of the entry points `names` = {name: index of nframes}."""
    from refvsr_amd import hip
    lib, calls = hip.lib(), []

    class Counting(object):
        def __getattr__(self, k):
            if k in names:
                return lambda *a: (calls.append((k, a[names[k]])), getattr(lib, k)(*a))[1]
            return getattr(lib, k)
    mp.setattr(hip, 'lib', lambda: Counting())
    return calls


@pytest.mark.parametrize('n', [1, 3, 16, 17])
@pytest.mark.parametrize('fmt, siting', [('i422', 'left'), ('i444p10', 'centre'), ('nv12', 'left')])
def test_frame_counts(dev, monkeypatch, fmt, siting, n):
    """1, 3, 16 frames in one launch, 17 in two, each way: every frame its own content."""
    from refvsr_amd import ops
    h, w = 18, 26
    calls = counting_lib(monkeypatch, {'refvsr_yuv_to_rgb': 2, 'refvsr_result_to_yuv': 3})
    x = frames_of(fmt, n, h, w)
    got = convert_in(exact(x, dev), h, w, fmt, siting)
    src, ts = results_on(dev, n, h, w, 'float32', 'chw')
    out = ops.result_to_yuv(ts, fmt, 'bt709', 'limited', siting)
    monkeypatch.undo()
    counts = [n] if n <= 16 else [16, n - 16]
    assert calls == [('refvsr_yuv_to_rgb', c) for c in counts] + [('refvsr_result_to_yuv', c) for c in counts]
    same_bits(got, yuv.yuv_to_rgb(x, h, w, fmt, siting=siting), '%s %d frames in' % (fmt, n))
    same_codes(out.cpu().numpy(), yuv.rgb_to_yuv(src, fmt, siting=siting), '%s %d frames out' % (fmt, n))


@pytest.mark.parametrize('fmt, siting', [('i422p10', 'left'), ('i444', 'centre')])
def test_full_hd_frame_each_way(dev, fmt, siting):
    h, w = 1080, 1920
    x = frames_of(fmt, 1, h, w)
    same_bits(convert_in(exact(x, dev), h, w, fmt, siting), yuv.yuv_to_rgb(x, h, w, fmt, siting=siting), '%s 1080 x 1920 in' % fmt)
    src, ts = results_on(dev, 1, h, w, 'float16', 'hwc')
    same_codes(convert_out(ts, fmt, siting), yuv.rgb_to_yuv(src, fmt, siting=siting), '%s 1080 x 1920 out' % fmt)


def test_ops_and_torch_ops(dev):
    from refvsr_amd import ops
    import refvsr_amd.torch_ops  # noqa: F401
    h, w = 18, 26
    for fmt, siting in (('i422', 'left'), ('i444p10', 'left'), ('p010', 'left')):
        x = frames_of(fmt, 5, h, w)
        t = torch.from_numpy(np.array(np.stack([x, x[::-1]]))).to(dev)
        a = ops.yuv_to_frames(t, h, w, fmt, 'bt601', 'full', 'bilinear', siting)
        b = torch.ops.refvsr.yuv_to_rgb(t, h, w, fmt, 'bt601', 'full', 'bilinear', siting)
        assert a.shape == (2, 5, 3, h, w) and a.is_contiguous() and torch.equal(a, b)
        same_bits(a[0].cpu().numpy(), yuv.yuv_to_rgb(x, h, w, fmt, 'bt601', 'full', 'bilinear', siting), 'ops %s' % fmt)
        r = torch.from_numpy(np.array(rgb_of(3, h, w, 'float32'))).to(dev)
        y = torch.ops.refvsr.result_to_yuv(r, fmt, 'bt601', 'full', siting)
        assert torch.equal(y.view(torch.uint8), ops.result_to_yuv(r, fmt, 'bt601', 'full', siting).view(torch.uint8))
        same_codes(y.cpu().numpy(), yuv.rgb_to_yuv(rgb_of(3, h, w, 'float32'), fmt, 'bt601', 'full', siting), 'torch op %s' % fmt)
        torch.library.opcheck(torch.ops.refvsr.yuv_to_rgb, (t, h, w, fmt, 'bt709', 'limited', 'bilinear', siting), test_utils=('test_schema', 'test_faketensor'))
        torch.library.opcheck(torch.ops.refvsr.result_to_yuv, (r, fmt, 'bt709', 'limited', siting), test_utils=('test_schema', 'test_faketensor'))
    with pytest.raises(RuntimeError, match='yuv_to_frames'):
        ops.yuv_to_frames(torch.zeros(2, 27, 26, dtype=torch.uint8, device=dev), h, w, 'i422')
    with pytest.raises(ValueError, match="'centre' or 'left'"):
        ops.result_to_yuv(r, 'i422', 'bt709', 'limited', 'top')
    with pytest.raises(ValueError, match='not a 4:2:0 format'):
        ops.result_to_yuv420(r, 'i444')


@pytest.mark.parametrize('fmt', ['i422', 'i444p10'])
def test_luma_sad(dev, fmt):
    from refvsr_amd import ops
    h, w = 18, 26
    x = frames_of(fmt, 5, h, w)
    t = torch.from_numpy(np.array(x)).to(dev)
    got = ops.luma_sad(t[1:], t[:-1], h, w, fmt).cpu().tolist()
    assert got == [yuv.luma_sad(x[i + 1], x[i], h, w, fmt) for i in builtins_range(4)] and min(got) > 0


# ------------------------------------------------------------------------------------------------ through the engine
def make_net(name, t, dev, input_yuv=None, pipelined=False, n_engines=1, **cfg_kw):
    from refvsr_amd import SRNet, get_config, make_state_dict
    cfg = get_config('p', 'm', name)
    cfg.frame_num, cfg.save_sample = t, False
    if input_yuv is not None:
        cfg.input_yuv, cfg.input_yuv_matrix, cfg.input_yuv_range, cfg.input_yuv_chroma, cfg.input_yuv_siting = input_yuv
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
    """A synthetic clip as frames of `kind` = (fmt, matrix, range, chroma, siting) and as the float32 frames the model decodes from
    them: (lr yuv, ref yuv, lr float32 [nfr,3,h,w], ref float32, windows); numpy, built once, left unchanged."""
    from refvsr_amd.synth import make_clip, window_indices
    key = (nfr, h, w, t, kind, seed)
    if key not in _CLIPS:
        fmt, matrix, range, chroma, siting = kind
        lr, rf, _ = make_clip(nfr, h, w, seed=seed, want_gt=False)
        ys = [yuv.rgb_to_yuv(x.numpy(), fmt, matrix, range, siting) for x in (lr, rf)]
        fs = [yuv.yuv_to_rgb(y, h, w, fmt, matrix, range, chroma, siting) for y in ys]
        for a in ys + fs:
            a.setflags(write=False)
        _CLIPS[key] = (ys[0], ys[1], fs[0], fs[1], [window_indices(f, nfr, t) for f in builtins_range(nfr)])
    return _CLIPS[key]


def win(x, idx, dev):
    return torch.from_numpy(np.array(x[np.array(idx)])).to(dev) if isinstance(idx[0], list) else \
        torch.from_numpy(np.array(x[np.array(idx)][None])).to(dev)


KINDS = [('i422', 'bt709', 'limited', 'bilinear', 'left'), ('i444p10', 'bt601', 'full', 'bilinear', 'centre')]
H, W = 16, 24                  # (the size tests/test_gpu_yuv_in.py runs its surfaces at)


def both(name, t, dev, kind, **kw):
    return make_net(name, t, dev, kind, **kw), make_net(name, t, dev, None, **kw)


def equal_results(a, b, what):
    ra, rb = a['result'], b['result']
    if isinstance(ra, tuple):
        assert len(ra) == len(rb)
        ra, rb = torch.cat(list(ra)), torch.cat(list(rb))
    assert ra.shape == rb.shape and ra.dtype == rb.dtype and torch.equal(ra, rb), '%s: the results differ' % what
    assert sorted(a.keys()) == sorted(b.keys())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('ids', [False, True])
def test_engine_forward(dev, kind, ids):
    """forward, n = 1, a stream of five frames: the window cache keyed by content (ids False) or by frame ids."""
    nfr, t = 5, 3
    ly, ry, lf, rf, wins = clip(nfr, H, W, t, kind)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind)
    for f, wi in enumerate(wins):
        kw = {'frame_ids': wi} if ids else {}
        a = ynet(win(ly, wi, dev), win(ry, wi, dev), f == 0, **kw)
        b = fnet(win(lf, wi, dev), win(rf, wi, dev), f == 0, **kw)
        assert a['result'].shape == (1, 3, 4 * H, 4 * W)
        equal_results(a, b, 'forward %s ids=%s frame %d' % (kind[0], ids, f))


@pytest.mark.parametrize('kind', KINDS)
def test_engine_two_samples_with_input_ready(dev, kind):
    nfr, t = 3, 3
    c0, c1 = clip(nfr, H, W, t, kind), clip(nfr, H, W, t, kind, seed=22)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind, pipelined=True, n_engines=2)
    for f, wi in enumerate(c0[4]):
        ya, yb, fa, fb = (torch.from_numpy(np.stack([c0[k][np.array(wi)], c1[k][np.array(wi)]])).to(dev) for k in (0, 1, 2, 3))
        torch.cuda.synchronize()
        ids = {'frame_ids': wi, 'input_ready': 'materialised'}
        a, b = ynet(ya, yb, f == 0, **ids), fnet(fa, fb, f == 0, **ids)
        assert a['result'].shape == (2, 3, 4 * H, 4 * W)
        equal_results(a, b, 'n = 2 %s frame %d' % (kind[0], f))
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', KINDS)
def test_engine_forward_group(dev, kind):
    nfr, t = 5, 3
    ly, ry, lf, rf, wins = clip(nfr, H, W, t, kind)
    ynet, fnet = both('config_RefVSR_small_L1', t, dev, kind, pipelined=True)
    for tag, net, l, r in (('yuv', ynet, ly, ry), ('f32', fnet, lf, rf)):
        first = net.forward_group(win(l, wins[:1], dev), win(r, wins[:1], dev), wins[:1], is_first_frame=True)
        rest = net.forward_group(win(l, wins[1:], dev), win(r, wins[1:], dev), wins[1:])
        torch.cuda.synchronize()
        if tag == 'yuv':
            got = (first, rest)
    assert len(got[1]['result']) == 4
    equal_results(got[0], first, 'forward_group first %s' % kind[0])
    equal_results(got[1], rest, 'forward_group B = 4 %s' % kind[0])


@pytest.mark.parametrize('kind', KINDS)
def test_engine_phases(dev, kind):
    """phase_a + phase_b frame by frame, and phase_a_group for the steady windows."""
    nfr, t = 4, 3
    ly, ry, lf, rf, wins = clip(nfr, H, W, t, kind)
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
        for hh in N2.phase_a_group(list(win(l, wins[1:], dev)), list(win(r, wins[1:], dev)), wins[1:]):
            outs.append(N2.phase_b(hh, False)['result'].clone())
        torch.cuda.synchronize()
        res[tag] = outs
    assert len(res['yuv']) == 2 * nfr
    for i, (a, b) in enumerate(zip(res['yuv'], res['f32'])):
        assert torch.equal(a, b), 'phases output %d (%s)' % (i, kind[0])


@pytest.mark.parametrize('kind', KINDS)
def test_engine_ir_configuration(dev, kind):
    nfr, t, h, w = 2, 5, 64, 64
    ly, ry, lf, rf, wins = clip(nfr, h, w, t, kind)
    ynet, fnet = both('config_RefVSR_IR_L1', t, dev, kind)
    for f, wi in enumerate(wins):
        equal_results(ynet(win(ly, wi, dev), win(ry, wi, dev), f == 0), fnet(win(lf, wi, dev), win(rf, wi, dev), f == 0), 'RefVSR_IR %s frame %d' % (kind[0], f))


@pytest.mark.parametrize('result_yuv, siting', [('i444p10', 'centre'), ('i422', 'left')])
def test_engine_returns_yuv_in_the_new_forms(dev, result_yuv, siting):
    """'yuv' of forward and of forward_group is the model applied to 'result', which is returned as it was."""
    nfr, t = 5, 3
    kind = ('nv12', 'bt709', 'limited', 'bilinear', 'centre')
    ly, ry, lf, rf, wins = clip(nfr, H, W, t, kind)
    net = make_net('config_RefVSR_small_L1', t, dev, None, result_yuv=result_yuv, yuv_matrix='bt601', yuv_range='full', yuv_siting=siting)
    plain = make_net('config_RefVSR_small_L1', t, dev, None)
    rows = yuv.frame_shape(4 * H, 4 * W, result_yuv)[0]
    for f, wi in enumerate(wins[:2]):
        a, b = net(win(lf, wi, dev), win(rf, wi, dev), f == 0), plain(win(lf, wi, dev), win(rf, wi, dev), f == 0)
        assert torch.equal(a['result'], b['result']) and a['yuv'].shape == (1, rows, 4 * W)
        same_codes(a['yuv'].cpu().numpy(), yuv.rgb_to_yuv(a['result'].cpu().numpy(), result_yuv, 'bt601', 'full', siting), 'forward yuv %s' % result_yuv)
    gnet = make_net('config_RefVSR_small_L1', t, dev, None, pipelined=True, result_yuv=result_yuv, yuv_siting=siting)
    g0 = gnet.forward_group(win(lf, wins[:1], dev), win(rf, wins[:1], dev), wins[:1], is_first_frame=True)
    g1 = gnet.forward_group(win(lf, wins[1:], dev), win(rf, wins[1:], dev), wins[1:])
    torch.cuda.synchronize()
    for g in (g0, g1):
        assert len(g['yuv']) == len(g['result'])
        for y, r in zip(g['yuv'], g['result']):
            assert y.shape == (1, rows, 4 * W)
            same_codes(y.cpu().numpy(), yuv.rgb_to_yuv(r.cpu().numpy(), result_yuv, 'bt709', 'limited', siting), 'forward_group yuv %s' % result_yuv)


def test_window_cache_keys_the_siting(dev, monkeypatch):
    """The content-keyed window cache: the same bytes under the same declaration hit (nothing is decoded) -- with is_first_frame too,
    which restarts the recurrence and leaves the cached window alone -- and under another siting they do not: the lookup runs against
    the populated left-sited window and declines it by its key, so every frame is decoded again, by the other entry point.  Nothing
    empties the cache between the calls."""
    from refvsr_amd import ops
    t = 3
    left = ('i420', 'bt709', 'limited', 'bilinear', 'left')
    ly, ry, lf, rf, wins = clip(3, H, W, t, left)
    calls = []
    for name in ('yuv_ingest', 'yuv420_ingest'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda pairs, *a, _r=real, _n=name, **k: (calls.append((_n, len(pairs))), _r(pairs, *a, **k))[1])
    net = make_net('config_RefVSR_small_L1', t, dev, left)
    a, b = win(ly, wins[1], dev), win(ry, wins[1], dev)
    r0 = net(a, b, True)['result'].clone()
    assert calls == [('yuv_ingest', 2 * t)], calls
    net(a.clone(), b.clone(), False)
    assert calls == [('yuv_ingest', 2 * t)], calls                # the same bytes, the same siting: a hit
    assert torch.equal(net(a.clone(), b.clone(), True)['result'], r0)
    assert calls == [('yuv_ingest', 2 * t)], calls                # is_first_frame does not empty the cache: still a hit
    eng = net.Network.ensure_engines(1, dev)[0]
    assert len(eng.prev_window) == t and all(c.kind == ('yuv',) + left for c in eng.prev_window)
    eng.input_yuv = eng.input_yuv[:4]                             # the same bytes declared centre-sited; the cache stays populated
    r1 = net(a.clone(), b.clone(), True)['result']
    assert calls == [('yuv_ingest', 2 * t), ('yuv420_ingest', 2 * t)], calls
    assert all(c.kind == ('yuv',) + left[:4] for c in eng.prev_window)
    centre = make_net('config_RefVSR_small_L1', t, dev, left[:4] + ('centre',))
    assert torch.equal(r1, centre(a, b, True)['result']) and not torch.equal(r1, r0)


# ------------------------------------------------------------------------------------------------ videorun
def write_y4m(path, frames, h, w, fmt, siting):
    with yuv.Y4MWriter(path, h, w, fmt, (24, 1), 'limited', siting) as wr:
        for f in frames:
            wr.write(f)


def run_video(dev, tmp_path, kind, nfr, t, G, lr, ref, name='sr.y4m', **eval_kw):
    from refvsr_amd import get_config, videorun
    paths = [str(tmp_path / ('uw_%s' % name)), str(tmp_path / ('w_%s' % name))]
    write_y4m(paths[0], lr, H, W, kind[0], kind[4])
    write_y4m(paths[1], ref, H, W, kind[0], kind[4])
    out = str(tmp_path / name)
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.save_sample = t, False
    cfg.EVAL.frame_group = G
    for k, v in eval_kw.items():
        setattr(cfg.EVAL, k, v)
    net = make_net('config_RefVSR_small_L1', t, dev, None)
    n, _ = videorun.run(cfg, paths[0], paths[1], out, net=net)
    assert n == nfr
    return out, cfg


def test_videorun_420mpeg2_to_444p10(dev, tmp_path):
    """A C420mpeg2 pair written as C444p10: the file holds rgb_to_yuv('i444p10') of the float32 engine's results on the frames the
    left-sited model decodes; without the options the output keeps the input's tag and siting."""
    nfr, t, G = 6, 3, 4
    kind = ('i420', 'bt709', 'limited', 'bilinear', 'left')
    ly, ry, lf, rf, wins = clip(nfr, H, W, t, kind)
    out, cfg = run_video(dev, tmp_path, kind, nfr, t, G, ly, ry, video_depth=10, out_chroma='444')
    assert (cfg.input_yuv, cfg.input_yuv_siting, cfg.result_yuv) == ('i420', 'left', 'i444p10')
    fnet = make_net('config_RefVSR_small_L1', t, dev, None, pipelined=True)
    rgb = []
    for f0 in builtins_range(0, nfr, G):
        r = fnet.forward_group(win(lf, wins[f0:f0 + G], dev), win(rf, wins[f0:f0 + G], dev), wins[f0:f0 + G], is_first_frame=f0 == 0)['result']
        rgb += [x[0].cpu().numpy() for x in r]
    got = yuv.read_y4m(out)
    assert open(out, 'rb').readline().split()[6] == b'C444p10'
    assert (got['h'], got['w'], got['fmt'], len(got['frames'])) == (4 * H, 4 * W, 'i444p10', nfr)
    for f in builtins_range(nfr):
        same_codes(got['frames'][f], yuv.rgb_to_yuv(rgb[f], 'i444p10'), 'frame %d of the C444p10 file' % f)
    same, cfg = run_video(dev, tmp_path, kind, nfr, t, G, ly, ry, name='same.y4m')
    got = yuv.read_y4m(same)
    assert open(same, 'rb').readline().split()[6] == b'C420mpeg2' and (got['fmt'], got['siting'], cfg.yuv_siting) == ('i420', 'left', 'left')
    for f in builtins_range(nfr):
        same_codes(got['frames'][f], yuv.rgb_to_yuv(rgb[f], 'i420', siting='left'), 'frame %d of the default output' % f)


def test_videorun_422_with_scene_cut(dev, tmp_path):
    """A C422 pair of two scenes under --scene_cut equals its scenes run alone, byte for byte, and keeps its tag.  The scenes are
    those of tests/test_gpu_scene.py (synth clips of two seeds, the motion scaled to a tenth so that only the cut scores high; the
    luma plane, which is all the detector reads, is the same in every sampling)."""
    from refvsr_amd.synth import make_clip
    t, G, na, nb = 3, 4, 5, 6
    kind = ('i422', 'bt709', 'limited', 'bilinear', 'left')
    sc = []
    for n, seed in ((na, 21), (nb, 22)):
        lr, rf, _ = make_clip(n, H, W, seed=seed, want_gt=False)
        sc.append([yuv.rgb_to_yuv((0.9 * x[:1] + 0.1 * x).numpy(), 'i422', 'bt709', 'limited', 'left') for x in (lr, rf)])
    lr, ref = np.concatenate([sc[0][0], sc[1][0]]), np.concatenate([sc[0][1], sc[1][1]])
    out, cfg = run_video(dev, tmp_path, kind, na + nb, t, G, lr, ref, name='cut.y4m', scene_cut=0.1)
    assert cfg.EVAL.scene_cuts == (na,) and cfg.result_yuv == 'i422' and open(out, 'rb').readline().split()[6] == b'C422'
    got = yuv.read_y4m(out)['frames']
    alone = []
    for name, (l, r) in (('s0.y4m', sc[0]), ('s1.y4m', sc[1])):
        o, _ = run_video(dev, tmp_path, kind, len(l), t, G, l, r, name=name)
        alone += yuv.read_y4m(o)['frames']
    assert len(got) == len(alone) == na + nb
    for f in builtins_range(na + nb):
        same_codes(got[f], alone[f], 'frame %d' % f)
