"""The antialiased resize on the device: refvsr_resize_aa returns the bits of refvsr_amd/resize.py:resize_aa_model -- every shape of
tests/resize_cases.py and a several-tile one, the six source forms at misaligned addresses, both destinations between canaries, clamp
on and off, 1, 3 and REFVSR_RESIZE_MAX_FRAMES + 1 frames, two streams -- and videorun's --in_down / --score / --out_size write the
bytes and the numbers of the same pipeline made on the host.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_cases as rc
from refvsr_amd import metrics, resize, scene, yuv

pytestmark = pytest.mark.gpu

CANARY = 0xA5
builtins_range = range


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def on_device(x, dev, hwc, offset):
    """The frames x [n,3,h,w] as cuda frames [3,h,w] (hwc: channels-last views) that start `offset` samples behind a 256-byte boundary
    and follow each other without a gap."""
    src = np.array(np.moveaxis(x, 1, -1) if hwc else x, order='C')                  # (a writable copy)
    t = torch.from_numpy(src)
    flat = torch.empty(src.size + offset + 64, dtype=t.dtype, device=dev)
    assert flat.data_ptr() % 256 == 0
    out = flat[offset:offset + src.size].view(src.shape)
    out.copy_(t)
    return [f.permute(2, 0, 1) for f in out] if hwc else [f for f in out]


def launch(frames, oh, ow, out, clamp, offset=1):
    """refvsr_resize_aa of the cuda frames into destinations carved out of one canary-filled byte buffer, `offset` samples behind a
    256-byte boundary each; returns [n,3,oh,ow] (numpy) after checking every canary byte."""
    from refvsr_amd import hip, ops
    f0 = frames[0]
    _, h, w = f0.shape
    n = len(frames)
    ds = 4 if out == 'float32' else 1
    nbytes = 3 * oh * ow * ds
    lead = 256 + offset * ds
    pitch = (lead + nbytes + 256 + 255) // 256 * 256
    buf = torch.full((n, pitch), CANARY, dtype=torch.uint8, device=f0.device)
    sfmt = {torch.float32: hip.RESULT_F32, torch.float16: hip.RESULT_F16, torch.uint8: hip.RESULT_U8}[f0.dtype]
    if not f0.is_contiguous():
        sfmt |= hip.RESULT_HWC
    lx, cx, wx, ly, cy, wy, mx, my = ops._resize_taps(f0.device, h, w, oh, ow)
    got = []
    for s0 in builtins_range(0, n, hip.RESIZE_MAX_FRAMES):
        k = min(hip.RESIZE_MAX_FRAMES, n - s0)
        hip.check(hip.lib().refvsr_resize_aa(ops._parr(frames[s0:s0 + k]), sfmt, (C.c_void_p * k)(*[buf[s0 + i].data_ptr() + lead for i in builtins_range(k)]),
                                             hip.RESULT_F32 if out == 'float32' else hip.RESULT_U8, k, h, w, oh, ow, ops._ptr(lx), ops._ptr(cx),
                                             ops._ptr(wx), ops._ptr(ly), ops._ptr(cy), ops._ptr(wy), mx, my, int(clamp),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'resize_aa')
        got.append(k)
    raw = buf.cpu().numpy()
    assert (raw[:, :lead] == CANARY).all() and (raw[:, lead + nbytes:] == CANARY).all(), 'a canary was overwritten'
    body = np.ascontiguousarray(raw[:, lead:lead + nbytes])
    return body.view(np.float32 if out == 'float32' else np.uint8).reshape(n, 3, oh, ow)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = a != b
    assert not bad.any(), '%s: %d of %d samples differ, first at %s' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# ------------------------------------------------------------------------------------------------ the kernel against the model
@pytest.mark.parametrize('shape', rc.SHAPES + (rc.TILED,))
def test_kernel_returns_the_models_bits(dev, shape):
    from refvsr_amd import hip
    h, w, oh, ow = shape
    nmax = hip.RESIZE_MAX_FRAMES + 1
    for dt in rc.DTYPES:
        x = rc.sources(shape, dt, nmax)
        d = resize.resize_aa_float64(x, oh, ow)
        want = {('float32', True): np.clip(d, 0.0, 1.0).astype(np.float32), ('float32', False): d.astype(np.float32),
                ('uint8', True): np.rint(255.0 * np.clip(d, 0.0, 1.0)).astype(np.uint8)}
        want[('uint8', False)] = want[('uint8', True)]                              # a byte destination is always clamped
        assert np.array_equal(want[('float32', True)][:2], resize.resize_aa_model(x[:2], oh, ow))
        for hwc in (False, True):
            for n in (1, 3, nmax):
                frames = on_device(x[:n], dev, hwc, offset=1)
                assert any(f.data_ptr() % 16 for f in frames)                       # addresses that are not 16-byte aligned
                for (out, clamp), wnt in want.items():
                    if n == 3 or (out, clamp) != ('uint8', False):
                        same(launch(frames, oh, ow, out, clamp, offset=1 if n != 3 else 3), wnt[:n],
                             '%s %s %s -> %s clamp %d, %d frames' % (shape, dt, 'hwc' if hwc else 'chw', out, clamp, n))


def test_two_streams_give_the_same_bits(dev):
    from refvsr_amd import ops
    shape = rc.TILED
    x = rc.sources(shape, 'float16', 3)
    frames = on_device(x, dev, True, 1)
    want = resize.resize_aa_model(x, shape[2], shape[3])
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    got = []
    for st in (s1, s2, s1):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            got.append(ops.resize_aa(frames, shape[2], shape[3]))
    torch.cuda.synchronize()
    for g in got:
        same(g.cpu().numpy(), want, 'two streams')


def test_ops_and_torch_op(dev):
    from refvsr_amd import ops
    import refvsr_amd.torch_ops  # noqa: F401
    shape = (37, 53, 12, 31)
    x = rc.sources(shape, 'uint8', 3)
    t = torch.from_numpy(np.array(x)).to(dev)
    for out in ('float32', 'uint8'):
        a = ops.resize_aa(t, 12, 31, out)
        b = torch.ops.refvsr.resize_aa(t, 12, 31, out, True)
        assert a.shape == (3, 3, 12, 31) and a.is_contiguous() and torch.equal(a, b)
        same(a.cpu().numpy(), resize.resize_aa_model(x, 12, 31, out), 'ops %s' % out)
        same(ops.resize_aa([f for f in t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)], 12, 31, out).cpu().numpy(),
             resize.resize_aa_model(x, 12, 31, out), 'ops, channels-last list, %s' % out)
    same(ops.resize_aa(t, 37, 53).cpu().numpy(), np.asarray(resize.source_values(x), np.float32), 'equal sizes: a copy')
    torch.library.opcheck(torch.ops.refvsr.resize_aa, (t, 12, 31, 'float32', True), test_utils=('test_schema', 'test_faketensor'))
    for bad, text in ((lambda: ops.resize_aa(t, 4, 31), 'ratio'), (lambda: ops.resize_aa(t, 0, 31), 'positive'),
                      (lambda: ops.resize_aa(t, 12, 31, 'float16'), "'float32' or 'uint8'"), (lambda: ops.resize_aa(t[:, :, ::2], 12, 31), 'dense'),
                      (lambda: ops.resize_aa(t.double(), 12, 31), 'float32 | float16 | uint8'), (lambda: ops.resize_aa([], 12, 31), 'at least one')):
        with pytest.raises(RuntimeError, match=text) as e:
            bad()
        assert '\n' not in str(e.value)


# ------------------------------------------------------------------------------------------------ videorun
def make_net(name, t, dev, pipelined=False, **cfg_kw):
    from refvsr_amd import SRNet, get_config, make_state_dict
    cfg = get_config('p', 'm', name)
    cfg.frame_num, cfg.save_sample = t, False
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234))
    if pipelined:
        net.Network.ensure_engines(1, dev)
        net.Network.set_pipelined(True)
    return net


_CLIPS = {}


def clip(nfr, h, w, fmt, seed=21):
    """A synthetic clip as 4:2:0 frames of `fmt` (bt709, limited, centre) and as the float32 frames the model decodes from them:
    (lr yuv, ref yuv, lr float32 [nfr,3,h,w], ref float32); numpy, built once, left unchanged."""
    from refvsr_amd.synth import make_clip
    key = (nfr, h, w, fmt, seed)
    if key not in _CLIPS:
        lr, rf, _ = make_clip(nfr, h, w, seed=seed, want_gt=False)
        ys = [yuv.rgb_to_yuv420(x.numpy(), fmt, 'bt709', 'limited') for x in (lr, rf)]
        fs = [yuv.yuv420_to_rgb(y, h, w, fmt, 'bt709', 'limited', 'bilinear') for y in ys]
        for a in ys + fs:
            a.setflags(write=False)
        _CLIPS[key] = (ys[0], ys[1], fs[0], fs[1])
    return _CLIPS[key]


def write_pair(tmp_path, h, w, fmt, lr, rf):
    paths = []
    for tag, x in (('uw', lr), ('w', rf)):
        paths.append(str(tmp_path / ('%s.y4m' % tag)))
        with yuv.Y4MWriter(paths[-1], h, w, fmt, (24, 1), 'limited') as wr:
            for f in x:
                wr.write(f)
    return paths


def run_config(t, G, **eval_kw):
    from refvsr_amd import get_config
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.save_sample = t, False
    cfg.EVAL.frame_group = G
    for k, v in eval_kw.items():
        setattr(cfg.EVAL, k, v)
    return cfg


def host_results(dev, lf, rf, t, G):
    """forward_group of a fresh float32 / uint8 network over the windows of the clip (lf, rf) [n,3,h,w], the plan of videorun: the
    results [n,3,4h,4w] as numpy."""
    fnet = make_net('config_RefVSR_small_L1', t, dev, pipelined=True)
    res = []
    for fs, wins, first in scene.plan_groups(len(lf), t, G, ()):
        lrs, rfs = (torch.from_numpy(np.stack([np.stack([x[i] for i in w_]) for w_ in wins])).to(dev) for x in (lf, rf))
        res += [r[0].cpu().numpy() for r in fnet.Network.forward_group(lrs, rfs, wins, is_first_frame=first)['result']]
    return res


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


@pytest.mark.parametrize('depth', [8, 10])
def test_in_down_and_score(dev, tmp_path, monkeypatch, depth):
    from refvsr_amd import videorun
    fmt = 'i420' if depth == 8 else 'i420p10'
    nfr, t, G, h, w, K = 6, 5, 4, 128, 192, 4
    ly, ry, lf, rf = clip(nfr, h, w, fmt)
    paths = write_pair(tmp_path, h, w, fmt, ly, ry)
    out, score = str(tmp_path / 'sr.y4m'), str(tmp_path / 'scores.txt')
    cfg = run_config(t, G, in_down=K, score_file=score)
    net = make_net('config_RefVSR_small_L1', t, dev)
    calls = counting_lib(monkeypatch, {'refvsr_yuv_to_rgb': 2, 'refvsr_resize_aa': 4})
    n, seconds = videorun.run(cfg, paths[0], paths[1], out, net=net)
    monkeypatch.undo()
    assert n == nfr and (cfg.input_yuv, cfg.result_yuv) == (None, fmt)
    for name in ('refvsr_yuv_to_rgb', 'refvsr_resize_aa'):                          # every file frame decoded once and resized once
        assert sum(c for k, c in calls if k == name) == 2 * nfr, calls
    # the same pipeline on the host: the model's decode, the model's down-scale, the network on those windows, the model's 4:2:0
    kind = 'uint8' if depth == 8 else 'float32'
    small = [resize.resize_aa_model(x, h // K, w // K, kind) for x in (lf, rf)]
    assert small[0].dtype == (np.uint8 if depth == 8 else np.float32)
    res = host_results(dev, small[0], small[1], t, G)
    got = yuv.read_y4m(out)
    assert (got['h'], got['w'], got['fmt']) == (h, w, fmt) and len(got['frames']) == nfr
    for f in builtins_range(nfr):
        assert np.array_equal(got['frames'][f], yuv.rgb_to_yuv420(res[f], fmt)), 'frame %d of the output file' % f
    lines = open(score).read().split('\n')
    assert len(lines) == nfr + 2 and lines[-1] == '' and lines[nfr].startswith('mean ')
    want = []
    for f in builtins_range(nfr):
        mse, ssim = metrics.score_frames_model(res[f], lf[f])
        want.append((f, metrics.psnr_from_mse(mse), float(ssim)))
        fr, p, s_ = lines[f].split()
        assert (int(fr), float(p), float(s_)) == want[-1], 'score line %d' % f
    assert cfg.EVAL.scores == want
    _, mp_, ms_ = lines[nfr].split()
    assert (float(mp_), float(ms_)) == (sum(p for _, p, _ in want) / nfr, sum(s_ for _, _, s_ in want) / nfr)


@pytest.mark.parametrize('size', [(72, 48), (160, 100)])          # W x H: three quarters of the 96 x 64 result | an up-scale
def test_out_size(dev, tmp_path, size):
    from refvsr_amd import videorun
    fmt, nfr, t, G, h, w = 'i420', 5, 3, 4, 16, 24
    ly, ry, lf, rf = clip(nfr, h, w, fmt)
    paths = write_pair(tmp_path, h, w, fmt, ly, ry)
    out = str(tmp_path / 'sr.y4m')
    cfg = run_config(t, G, out_size='%dx%d' % size)
    n, _ = videorun.run(cfg, paths[0], paths[1], out, net=make_net('config_RefVSR_small_L1', t, dev))
    assert n == nfr and (cfg.input_yuv, cfg.result_yuv, cfg.EVAL.out_yuv, cfg.EVAL.out_size) == (fmt, None, fmt, size)
    res = host_results(dev, lf, rf, t, G)
    got = yuv.read_y4m(out)
    assert (got['h'], got['w'], got['fmt']) == (size[1], size[0], fmt) and len(got['frames']) == nfr
    for f in builtins_range(nfr):
        want = yuv.rgb_to_yuv420(resize.resize_aa_model(res[f], size[1], size[0], 'float32', True), fmt)
        assert np.array_equal(got['frames'][f], want), 'frame %d of the output file' % f


def test_off_means_off(dev, tmp_path, monkeypatch):
    """With none of the options refvsr_resize_aa is never called, and the file is the one a run writes whose new code paths raise."""
    from refvsr_amd import ops, videorun
    fmt, nfr, t, G, h, w = 'i420', 5, 3, 4, 16, 24
    ly, ry, _, _ = clip(nfr, h, w, fmt)
    paths = write_pair(tmp_path, h, w, fmt, ly, ry)
    outs = [str(tmp_path / ('sr%d.y4m' % i)) for i in (0, 1)]
    calls = counting_lib(monkeypatch, {'refvsr_resize_aa': 4})
    cfg = run_config(t, G)
    assert videorun.run(cfg, paths[0], paths[1], outs[0], net=make_net('config_RefVSR_small_L1', t, dev))[0] == nfr
    assert calls == [] and (cfg.EVAL.in_down, cfg.EVAL.score_file, cfg.EVAL.out_size) == (None, None, None) and (cfg.input_yuv, cfg.result_yuv) == (fmt, fmt)

    def boom(*a, **k):
        raise AssertionError('an option that is off ran')
    for mod, name in ((ops, 'resize_aa'), (ops, 'score_frames'), (videorun, 'resized_yuv'), (videorun, 'write_scores')):
        monkeypatch.setattr(mod, name, boom)
    assert videorun.run(run_config(t, G), paths[0], paths[1], outs[1], net=make_net('config_RefVSR_small_L1', t, dev))[0] == nfr
    assert open(outs[0], 'rb').read() == open(outs[1], 'rb').read()
