"""Scene cuts on the device: refvsr_luma_sad returns the integers of refvsr_amd/yuv.py:luma_sad -- every format, size class, pair count
and address phase, sums beyond 32 bits, canaries around its outputs, two streams -- and videorun runs a file with a cut as its two
scenes run alone, byte for byte, detected (--scene_cut) or given (--cuts); with neither option nothing new runs.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import yuv_in_cases as yc
from refvsr_amd import scene, yuv

pytestmark = pytest.mark.gpu

FORMATS = yc.FORMATS
# one 16-byte group at most (head / tail only) | ragged, less than one chunk | several groups, phases 3366 i (mod 16) | 270 x 480: 16
# chunks of 8-bit, 32 chunks of 10-bit samples -- every chunk boundary of the kernel, frames 16-byte aligned inside a window
SIZES = ((2, 2), (6, 10), (34, 66), (270, 480))
PAIRS = (1, 3, 16, 17)         # 17: two calls
builtins_range = range


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


_WINDOWS = {}


def window_of(fmt, n, h, w, salt=0):
    """A seeded window [n, 3h/2, w] of random codes over the full range, with the bits the model ignores set at random (p010: low six,
    i420p10: high six); built once per key and left unchanged."""
    key = (fmt, n, h, w, salt)
    if key not in _WINDOWS:
        rs = np.random.RandomState(31 * h + w + 1000 * n + yuv.FORMAT_IDS[fmt] + 7919 * salt)
        x = np.stack([yc.random_codes(rs, h, w, fmt) for _ in builtins_range(n)])
        if fmt == 'p010':
            x = x | rs.randint(0, 64, x.shape).astype(np.uint16)
        if fmt == 'i420p10':
            x = x | (rs.randint(0, 64, x.shape) << 10).astype(np.uint16)
        x.setflags(write=False)
        _WINDOWS[key] = x
    return _WINDOWS[key]


def on_device(x, dev, offset=0):
    """The window x as a cuda tensor whose first frame lies `offset` samples behind a 256-byte boundary."""
    flat = torch.empty(x.size + offset + 64, dtype=torch.uint8 if x.dtype == np.uint8 else torch.uint16, device=dev)
    assert flat.data_ptr() % 256 == 0
    out = flat[offset:offset + x.size].view(x.shape)
    out.copy_(torch.from_numpy(np.array(x)))
    return out


def model(a, b, h, w, fmt):
    return [yuv.luma_sad(p, q, h, w, fmt) for p, q in zip(a, b)]


# ------------------------------------------------------------------------------------------------ the kernel against the model
@pytest.mark.parametrize('h, w', SIZES)
@pytest.mark.parametrize('fmt', FORMATS)
def test_kernel_returns_the_models_integers(dev, fmt, h, w):
    from refvsr_amd import ops
    x, z = window_of(fmt, 18, h, w), window_of(fmt, 17, h, w, salt=1)
    want_seq = model(x[1:], x[:-1], h, w, fmt)                   # consecutive frames of one window
    want_cross = model(x[:17], z, h, w, fmt)                     # frames of two windows
    assert min(want_seq + want_cross) > 0
    ss = x.dtype.itemsize
    for oa, ob in ((0, 0), (1, 3), (5, 8), (8 // ss, 16 // ss)):
        dx, dz = on_device(x, dev, oa), on_device(z, dev, ob)
        phases = {(f.data_ptr() % 16) for f in dx}
        assert oa == 0 or phases != {0}                          # frames that are not 16-byte aligned
        for n in PAIRS:
            got = ops.luma_sad(dx[1:n + 1], dx[:n], h, w, fmt)
            assert got.dtype == torch.int64 and tuple(got.shape) == (n,) and got.device == dx.device
            assert got.cpu().tolist() == want_seq[:n], '%s %d x %d, %d consecutive pairs, offset %d' % (fmt, h, w, n, oa)
            got = ops.luma_sad([f for f in dx[:n]], [f for f in dz[:n]], h, w, fmt)              # lists of views, two phases per pair
            assert got.cpu().tolist() == want_cross[:n], '%s %d x %d, %d cross pairs, offsets %d, %d' % (fmt, h, w, n, oa, ob)
        # a pair of the same pointer, alone and among others
        assert ops.luma_sad([dx[2]], [dx[2]], h, w, fmt).cpu().tolist() == [0]
        assert ops.luma_sad([dx[1], dx[2], dx[3]], [dx[0], dx[2], dz[3]], h, w, fmt).cpu().tolist() == [want_seq[0], 0, want_cross[3]]


@pytest.mark.parametrize('fmt, h, w', [('p010', 2048, 2064), ('i420p10', 2048, 2064), ('nv12', 4096, 4128), ('i420', 4096, 4128)])
def test_sums_beyond_32_bits(dev, fmt, h, w):
    """All-zero against all-maximum, sums past 2^32 = 4 294 967 296: 10-bit at 2048 x 2064 gives 2048 * 2064 * 1023 = 4 324 294 656,
    8-bit at 4096 x 4128 gives 4096 * 4128 * 255 = 4 311 613 440."""
    from refvsr_amd import ops
    depth = yuv.depth_of(fmt)
    top = (2 ** depth - 1) << (6 if fmt == 'p010' else 0)
    a = torch.from_numpy(np.zeros(yuv.frame_shape(h, w), dtype=yuv.dtype_of(fmt))).to(dev)
    b = torch.from_numpy(np.full(yuv.frame_shape(h, w), top, dtype=yuv.dtype_of(fmt))).to(dev)
    want = h * w * (2 ** depth - 1)
    assert want > 2 ** 32 and want == (4324294656 if depth == 10 else 4311613440)
    assert ops.luma_sad([a], [b], h, w, fmt).cpu().tolist() == [want]
    assert ops.luma_sad([b], [a], h, w, fmt).cpu().tolist() == [want]
    if depth == 10:                                              # (the model on 4 M samples; the 8-bit frames are four times that)
        assert yuv.luma_sad(a.cpu().numpy(), b.cpu().numpy(), h, w, fmt) == want


@pytest.mark.parametrize('fmt', FORMATS)
def test_canaries_around_sad_and_workspace(dev, fmt):
    from refvsr_amd import hip, ops
    L = hip.lib()
    PAD = 64
    for (h, w), n in (((34, 66), 3), ((270, 480), 16), ((2, 2), 1)):
        x = window_of(fmt, 18, h, w)
        dx = on_device(x, dev, 1)
        nb = L.refvsr_luma_sad_workspace_bytes(n, h, w)
        assert nb > 0 and nb % 16 == 0
        ws = torch.full((2 * PAD + nb // 4,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        sad = torch.full((2 * PAD + n,), -0x0123456789abcdef, dtype=torch.int64, device=dev)
        wsp, sadp = ws.data_ptr() + 4 * PAD, sad.data_ptr() + 8 * PAD
        assert wsp % 16 == 0 and sadp % 8 == 0
        rc = L.refvsr_luma_sad(ops._parr([f for f in dx[1:n + 1]]), ops._parr([f for f in dx[:n]]), n, h, w, yuv.FORMAT_IDS[fmt],
                               C.c_void_p(wsp), nb, C.c_void_p(sadp), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        hip.check(rc, 'luma_sad')
        got, wsh = sad.cpu().tolist(), ws.cpu().numpy()
        assert got[PAD:PAD + n] == model(x[1:n + 1], x[:n], h, w, fmt)
        assert set(got[:PAD] + got[PAD + n:]) == {-0x0123456789abcdef}, 'a canary beside sad was overwritten'
        assert (wsh[:PAD] == 0x5a5a5a5a).all() and (wsh[PAD + nb // 4:] == 0x5a5a5a5a).all(), 'a canary beside the workspace was overwritten'


def test_two_streams_give_the_same_integers(dev):
    from refvsr_amd import ops
    h, w, fmt = 270, 480, 'p010'
    x = window_of(fmt, 18, h, w)
    dx = on_device(x, dev, 3)
    want = model(x[1:6], x[:5], h, w, fmt)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    got = []
    for st in (s1, s2, s1):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            got.append(ops.luma_sad(dx[1:6], dx[:5], h, w, fmt))
    torch.cuda.synchronize()
    assert [g.cpu().tolist() for g in got] == [want] * 3
    with pytest.raises(RuntimeError, match='luma_sad'):
        ops.luma_sad(dx[1:3], dx[:1], h, w, fmt)                 # 2 frames against 1
    with pytest.raises(RuntimeError, match='luma_sad'):
        ops.luma_sad(dx[1:3], dx[:2], h, w, 'nv12')              # uint16 frames are not nv12


# ------------------------------------------------------------------------------------------------ videorun
T_CUT = 0.1                    # the customary threshold
NA, NB, FRAME_T, GROUP, H, W = 5, 6, 3, 4, 16, 24


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


_SCENES = {}


def scenes(fmt):
    """Clip A (5 frames) and clip B (6 frames) from synth with different seeds, as 4:2:0 frames: ((lr A, ref A), (lr B, ref B)).
    synth's texture moves half an LR pixel per frame, which at 16 x 24 is a mean luma difference of about 20 codes between neighbours
    -- half of what the cut itself gives, so frame 1 and the frame behind the cut score nearly as high as the cut and NO pair of seeds
    meets the condition test_inputs_are_not_borderline sets (the best of 3 540 pairs reaches a ratio of 2, it asks for 4).  The
    motion is therefore scaled to a tenth: frame k is frame 0 + (frame k - frame 0) / 10 of synth's clip, all frames still distinct."""
    from refvsr_amd.synth import make_clip
    if fmt not in _SCENES:
        out = []
        for n, seed in ((NA, 21), (NB, 22)):
            lr, rf, _ = make_clip(n, H, W, seed=seed, want_gt=False)
            ys = [yuv.rgb_to_yuv420((0.9 * x[:1] + 0.1 * x).numpy(), fmt, 'bt709', 'limited') for x in (lr, rf)]
            for y in ys:
                y.setflags(write=False)
            out.append(tuple(ys))
        _SCENES[fmt] = tuple(out)
    return _SCENES[fmt]


def write_pair(tmp_path, name, fmt, lr, rf):
    paths = []
    for tag, x in (('uw', lr), ('w', rf)):
        paths.append(str(tmp_path / ('%s_%s.y4m' % (name, tag))))
        with yuv.Y4MWriter(paths[-1], H, W, fmt, (24, 1), 'limited') as wr:
            for f in x:
                wr.write(f)
    return paths


_NETS = {}


def run_file(dev, tmp_path, fmt, name, lr, rf, **eval_kw):
    """videorun.run on the frames (lr, rf) written as a .y4m pair: (the frames of the output file, the run's config).  One seeded
    network per format serves every run: run() starts each with Network.reset()."""
    from refvsr_amd import get_config, videorun
    paths = write_pair(tmp_path, name, fmt, lr, rf)
    out = str(tmp_path / ('%s_sr.y4m' % name))
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.save_sample = FRAME_T, False
    cfg.EVAL.frame_group = GROUP
    for k, v in eval_kw.items():
        setattr(cfg.EVAL, k, v)
    if fmt not in _NETS:
        _NETS[fmt] = make_net('config_RefVSR_small_L1', FRAME_T, dev, (fmt, 'bt709', 'limited', 'bilinear'), result_yuv=fmt)
    n, seconds = videorun.run(cfg, paths[0], paths[1], out, net=_NETS[fmt])
    got = yuv.read_y4m(out)
    assert n == len(lr) == len(got['frames']) and (got['h'], got['w'], got['fmt']) == (4 * H, 4 * W, fmt)
    return got['frames'], cfg


def same_frames(got, want, what):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), '%s: frame %d differs' % (what, f)


@pytest.mark.parametrize('depth', [8, 10])
def test_inputs_are_not_borderline(depth):
    """A condition on the inputs (numpy model, no device): the score at frame 5 is at least twice the threshold, every other at most
    half of it -- the detector tests below cannot hinge on a borderline case."""
    fmt = 'i420' if depth == 8 else 'i420p10'
    (la, _), (lb, _) = scenes(fmt)
    for x, cut in ((np.concatenate([la, lb]), NA), (la, None), (lb, None)):
        s = scene.scene_scores([yuv.luma_sad(x[k], x[k - 1], H, W, fmt) for k in builtins_range(1, len(x))], H, W, depth)
        assert len({f.tobytes() for f in x}) == len(x)
        assert all(v <= T_CUT / 2 for k, v in enumerate(s) if k != cut), s
        assert cut is None or s[cut] >= 2 * T_CUT, s
        assert scene.cuts_from_scores(s, T_CUT) == (() if cut is None else (cut,))


@pytest.mark.parametrize('depth', [8, 10])
def test_a_file_with_a_cut_runs_as_its_scenes_alone(dev, tmp_path, depth):
    fmt = 'i420' if depth == 8 else 'i420p10'
    test_inputs_are_not_borderline(depth)                        # before any GPU work
    (la, ra), (lb, rb) = scenes(fmt)
    lj, rj = np.concatenate([la, lb]), np.concatenate([ra, rb])
    alone_a, cfg = run_file(dev, tmp_path, fmt, 'a', la, ra)
    assert cfg.EVAL.scene_cuts == ()
    alone_b, _ = run_file(dev, tmp_path, fmt, 'b', lb, rb)
    want = alone_a + alone_b
    got, cfg = run_file(dev, tmp_path, fmt, 'detected', lj, rj, scene_cut=T_CUT)
    assert cfg.EVAL.scene_cuts == (NA,)
    same_frames(got, want, '--scene_cut %g' % T_CUT)
    got, cfg = run_file(dev, tmp_path, fmt, 'given', lj, rj, cuts=(NA,))
    assert cfg.EVAL.scene_cuts == (NA,)
    same_frames(got, want, '--cuts %d' % NA)
    # the comparison can tell: the file run as one clip differs in the frames around and behind the cut
    plain, cfg = run_file(dev, tmp_path, fmt, 'plain', lj, rj)
    assert cfg.EVAL.scene_cuts == ()
    same_frames(plain[:NA - 1], want[:NA - 1], 'ahead of the cut')
    assert any(not np.array_equal(plain[f], want[f]) for f in builtins_range(NA - 1, NA + NB)), 'one clip and two scenes give the same file'
    # a file without a cut: the detector changes nothing
    got, cfg = run_file(dev, tmp_path, fmt, 'nocut', lb, rb, scene_cut=T_CUT)
    assert cfg.EVAL.scene_cuts == ()
    same_frames(got, alone_b, 'a file without a cut under --scene_cut')


def clip(nfr, h, w, t, kind, seed=21):
    """A synthetic clip as 4:2:0 frames of `kind` = (fmt, matrix, range, chroma) and as the float32 frames the model decodes from
    them: (lr yuv [nfr, 3h/2, w], ref yuv, lr float32 [nfr,3,h,w], ref float32, windows); numpy."""
    from refvsr_amd.synth import make_clip, window_indices
    fmt, matrix, range, chroma = kind
    lr, rf, _ = make_clip(nfr, h, w, seed=seed, want_gt=False)
    ys = [yuv.rgb_to_yuv420(x.numpy(), fmt, matrix, range) for x in (lr, rf)]
    fs = [yuv.yuv420_to_rgb(y, h, w, fmt, matrix, range, chroma) for y in ys]
    return ys[0], ys[1], fs[0], fs[1], [window_indices(f, nfr, t) for f in builtins_range(nfr)]


def win(x, idx, dev):
    """Window(s) `idx` of the clip x as a cuda tensor: a list of indices -> [1, t, ...], a list of lists -> [B, t, ...]."""
    return torch.from_numpy(np.array(x[np.array(idx)])).to(dev) if isinstance(idx[0], list) else \
        torch.from_numpy(np.array(x[np.array(idx)][None])).to(dev)


@pytest.mark.parametrize('depth', [8, 10])
def test_off_means_no_new_code_runs(dev, tmp_path, depth, monkeypatch):
    """With neither option: ops.luma_sad is never called and the output file is the one-clip plan's -- the construction of
    tests/test_gpu_yuv_in.py:test_videorun_writes_the_models_bytes: 8-frame 16 x 24 .y4m pairs, the output file holds rgb_to_yuv420 of
    the float32 engine's results on the modelled inputs."""
    from refvsr_amd import get_config, ops, videorun
    calls = []
    real = ops.luma_sad
    monkeypatch.setattr(ops, 'luma_sad', lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
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
    resets = []
    real_reset = net.Network.reset
    monkeypatch.setattr(net.Network, 'reset', lambda: (resets.append(1), real_reset())[1])
    n, seconds = videorun.run(cfg, paths[0], paths[1], out, net=net)
    assert n == nfr and seconds > 0 and (cfg.input_yuv, cfg.result_yuv) == (fmt, fmt)
    assert calls == [] and resets == [1] and cfg.EVAL.scene_cuts == ()
    fnet = make_net('config_RefVSR_small_L1', t, dev, None, pipelined=True)
    want = []
    for f0 in builtins_range(0, nfr, G):
        r = fnet.forward_group(win(lf, wins[f0:f0 + G], dev), win(rf, wins[f0:f0 + G], dev), wins[f0:f0 + G], is_first_frame=f0 == 0)['result']
        want += [yuv.rgb_to_yuv420(x[0].cpu().numpy(), fmt) for x in r]
    got = yuv.read_y4m(out)
    assert (got['h'], got['w'], got['fps'], got['fmt'], got['range']) == (4 * h, 4 * w, (24, 1), fmt, 'limited') and len(got['frames']) == nfr
    for f in builtins_range(nfr):
        assert np.array_equal(got['frames'][f], want[f]), 'frame %d of the output file' % f
    # and with the option the detector runs once per group: the new frames of each against their predecessors
    cfg.EVAL.scene_cut = 1.0
    videorun.run(cfg, paths[0], paths[1], out, net=net)
    assert calls == [4, 3] and cfg.EVAL.scene_cuts == ()
    same_frames(yuv.read_y4m(out)['frames'], got['frames'], 'scene_cut = 1 on a clip without a cut')
