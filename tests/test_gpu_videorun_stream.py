"""videorun --io stream on the device: the stream loop writes the bytes of the sync loop -- header included -- for both depths, with
detected and given cuts, under --in_down / --score / --out_size, for clips shorter than a window and a group, at every depth of the
pipeline; every file frame is uploaded once; a run that ends in an error leaves no thread, no pending device work and a network that
still runs.  All sources and sinks are in-process: regular files, and file objects that know neither seek nor fileno -- the length
really is unknown.  No tolerance anywhere."""
import io
import threading
import time

import numpy as np
import pytest
import torch

import test_gpu_resize as tgr
import test_gpu_scene as tgs
from refvsr_amd import scene, yuv

pytestmark = pytest.mark.gpu

H, W, T, G = tgs.H, tgs.W, tgs.FRAME_T, tgs.GROUP        # 16 x 24, t = 3, groups of 4
NAME = 'config_RefVSR_small_L1'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


class Source(object):
    """A stream's bytes as a file object that can only be read front to back, 4093 bytes at a time at most."""

    def __init__(self, data, name):
        self.data, self.pos, self.name = data, 0, name

    def read(self, n=-1):
        k = 4093 if n is None or n < 0 else min(n, 4093)
        out = self.data[self.pos:self.pos + k]
        self.pos += len(out)
        return out

    def seek(self, *a):
        raise io.UnsupportedOperation('seek')

    tell = fileno = seek


class Sink(object):
    """What a run writes, collected; no seek, no fileno."""

    def __init__(self):
        self.parts, self.flushed, self.name = [], 0, 'sink'

    def write(self, b):
        self.parts.append(bytes(b))
        return len(b)

    def flush(self):
        self.flushed += 1

    def seek(self, *a):
        raise io.UnsupportedOperation('seek')

    tell = fileno = seek

    def bytes(self):
        return b''.join(self.parts)


def y4m_bytes(frames, h, w, fmt):
    out = io.BytesIO()
    with yuv.Y4MWriter(out, h, w, fmt, (24, 1), 'limited') as wr:
        for f in frames:
            wr.write(f)
    return out.getvalue()


def config(t, **eval_kw):
    from refvsr_amd import get_config
    cfg = get_config('p', 'm', NAME)
    cfg.frame_num, cfg.save_sample = t, False
    cfg.EVAL.frame_group = G
    for k, v in eval_kw.items():
        setattr(cfg.EVAL, k, v)
    return cfg


def run_sync(net, t, tmp_path, tag, lr, rf, h, w, fmt, **eval_kw):
    """The sync loop on a pair of regular files: (the output file's bytes, the run's config)."""
    from refvsr_amd import videorun
    paths = []
    for name, x in (('uw', lr), ('w', rf)):
        paths.append(str(tmp_path / ('%s_%s.y4m' % (tag, name))))
        with open(paths[-1], 'wb') as f:
            f.write(y4m_bytes(x, h, w, fmt))
    out = str(tmp_path / ('%s_sr.y4m' % tag))
    cfg = config(t, io='sync', **eval_kw)
    n, _ = videorun.run(cfg, paths[0], paths[1], out, net=net)
    assert n == len(lr) and not hasattr(cfg.EVAL, 'io_stats')
    return open(out, 'rb').read(), cfg, paths


def run_stream(net, t, lr_src, ref_src, n, depth=2, **eval_kw):
    """The stream loop on two sources into a Sink: (the bytes written, the run's config); the counters every run has to meet."""
    from refvsr_amd import videorun
    sink = Sink()
    cfg = config(t, io='stream', io_depth=depth, io_timeout=10, **eval_kw)
    start = threading.active_count()
    got, seconds = videorun.run(cfg, lr_src, ref_src, sink, net=net)
    st = cfg.EVAL.io_stats
    assert got == n == st['frames'] and seconds > 0 and sink.flushed >= 1
    assert st['uploads'] == 2 * n, st                              # every file frame of both streams went to the device once
    assert 1 <= st['max_in_flight'] <= depth, st
    assert st['max_held'] <= videorun.held_bound(t, G, depth) == t + (depth + 1) * G + 2, st
    assert st['groups'] == len(scene.plan_groups(n, t, G, cfg.EVAL.scene_cuts))
    assert min(st[k] for k in ('read_wait', 'device_wait', 'write_wait')) >= 0.0 and st['wall'] >= seconds > 0
    assert threading.active_count() == start, [th.name for th in threading.enumerate()]
    return sink.bytes(), cfg


_NETS = {}


def net_of(dev, fmt, t):
    if (fmt, t) not in _NETS:
        _NETS[(fmt, t)] = tgs.make_net(NAME, t, dev, (fmt, 'bt709', 'limited', 'bilinear'), result_yuv=fmt)
    return _NETS[(fmt, t)]


def joined(fmt):
    (la, ra), (lb, rb) = tgs.scenes(fmt)
    return np.concatenate([la, lb]), np.concatenate([ra, rb])


@pytest.mark.parametrize('depth', [8, 10])
def test_stream_writes_the_bytes_of_sync(dev, tmp_path, depth):
    """11 frames with a cut at 5: one clip, --scene_cut and --cuts.  The sources: a file object and a regular file, both ways round."""
    fmt = 'i420' if depth == 8 else 'i420p10'
    tgs.test_inputs_are_not_borderline(depth)
    lj, rj = joined(fmt)
    n = len(lj)
    net = net_of(dev, fmt, T)
    datas = y4m_bytes(lj, H, W, fmt), y4m_bytes(rj, H, W, fmt)
    outs = {}
    for tag, kw, cuts in (('plain', {}, ()), ('detected', dict(scene_cut=tgs.T_CUT), (tgs.NA,)), ('given', dict(cuts=(tgs.NA,)), (tgs.NA,))):
        want, cfg, paths = run_sync(net, T, tmp_path, tag, lj, rj, H, W, fmt, **kw)
        assert cfg.EVAL.scene_cuts == cuts
        srcs = (Source(datas[0], 'lr'), paths[1]) if tag != 'given' else (paths[0], Source(datas[1], 'ref'))
        got, cfg = run_stream(net, T, srcs[0], srcs[1], n, **kw)
        assert cfg.EVAL.scene_cuts == cuts
        assert got == want, '%s %s: the stream loop and the sync loop write different files' % (fmt, tag)
        assert got.startswith(b'YUV4MPEG2 W%d H%d F24:1 ' % (4 * W, 4 * H)) and len(got) > n * yuv.frame_bytes(4 * H, 4 * W, fmt)
        outs[tag] = got
    assert outs['detected'] == outs['given'] != outs['plain']          # (the comparison can tell)
    # regular files on both sides, the mode asked for by name
    from refvsr_amd import videorun
    out = str(tmp_path / 'files_sr.y4m')
    cfg = config(T, io='stream', io_timeout=10)
    assert videorun.run(cfg, paths[0], paths[1], out, net=net)[0] == n and cfg.EVAL.io_stats['uploads'] == 2 * n
    assert open(out, 'rb').read() == outs['plain']


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_every_depth_of_the_pipeline(dev, tmp_path, depth):
    fmt = 'i420'
    lj, rj = joined(fmt)
    net = net_of(dev, fmt, T)
    want, _, _ = run_sync(net, T, tmp_path, 'd', lj, rj, H, W, fmt)
    got, cfg = run_stream(net, T, Source(y4m_bytes(lj, H, W, fmt), 'lr'), Source(y4m_bytes(rj, H, W, fmt), 'ref'), len(lj), depth=depth)
    assert got == want
    assert cfg.EVAL.io_stats['max_in_flight'] == min(depth, 3)         # (11 frames are three groups)


@pytest.mark.parametrize('n', [1, 2, 4, 5, 11])
def test_short_clips_with_five_frame_windows(dev, tmp_path, n):
    """t = 5: windows clamped at both ends of the clip, a last group that is short, clips shorter than a window and than a group."""
    fmt, t = 'i420', 5
    ly, ry, _, _ = tgr.clip(11, H, W, fmt)
    net = net_of(dev, fmt, t)
    want, _, _ = run_sync(net, t, tmp_path, 'n%d' % n, ly[:n], ry[:n], H, W, fmt)
    got, _ = run_stream(net, t, Source(y4m_bytes(ly[:n], H, W, fmt), 'lr'), Source(y4m_bytes(ry[:n], H, W, fmt), 'ref'), n)
    assert got == want


def test_in_down_score_and_out_size(dev, tmp_path):
    fmt, h, w, n = 'i420', 64, 96, 6
    ly, ry, _, _ = tgr.clip(n, h, w, fmt)
    net = tgr.make_net(NAME, T, dev)
    scores = [str(tmp_path / ('scores%d.txt' % i)) for i in (0, 1)]
    kw = dict(in_down=4, out_size='48x32')
    want, cfg, _ = run_sync(net, T, tmp_path, 'down', ly, ry, h, w, fmt, score_file=scores[0], **kw)
    assert (cfg.input_yuv, cfg.result_yuv, cfg.EVAL.out_size) == (None, None, (48, 32)) and want.startswith(b'YUV4MPEG2 W48 H32 ')
    got, cfg2 = run_stream(net, T, Source(y4m_bytes(ly, h, w, fmt), 'lr'), Source(y4m_bytes(ry, h, w, fmt), 'ref'), n, score_file=scores[1], **kw)
    assert got == want
    a, b = open(scores[0], 'rb').read(), open(scores[1], 'rb').read()
    assert a == b and a.count(b'\n') == n + 1 and cfg2.EVAL.scores == cfg.EVAL.scores


def test_errors_leave_nothing_behind(dev, tmp_path):
    from refvsr_amd import videorun
    fmt = 'i420'
    lj, rj = joined(fmt)
    n = len(lj)
    net = net_of(dev, fmt, T)
    want, _, _ = run_sync(net, T, tmp_path, 'before', lj, rj, H, W, fmt)
    dl, dr = y4m_bytes(lj, H, W, fmt), y4m_bytes(rj, H, W, fmt)
    for lr_data, ref_data, text in ((dl, y4m_bytes(rj[:n - 1], H, W, fmt), r'^videorun: lr and ref: frame count differs \(more than 10 and 10\)$'),
                                    (dl[:-5], dr, r'^lr: truncated frame 10$')):
        start = threading.active_count()
        cfg = config(T, io='stream', io_timeout=10)
        with pytest.raises(ValueError, match=text):
            videorun.run(cfg, Source(lr_data, 'lr'), Source(ref_data, 'ref'), Sink(), net=net)
        torch.cuda.synchronize()
        t0 = time.time()
        while threading.active_count() > start and time.time() - t0 < 5:
            time.sleep(0.02)
        assert threading.active_count() == start, [th.name for th in threading.enumerate()]
        assert cfg.EVAL.io_stats['frames'] <= 8 and net.Network.config.pipelined is False
        again, _, _ = run_sync(net, T, tmp_path, 'after', lj, rj, H, W, fmt)
        assert again == want, 'the network runs a correct sync run behind %s' % text


def test_pipelined_state_is_restored(dev):
    fmt = 'i420'
    lj, rj = joined(fmt)
    net = net_of(dev, fmt, T)
    for state in (False, True):
        net.Network.set_pipelined(state)
        run_stream(net, T, Source(y4m_bytes(lj[:5], H, W, fmt), 'lr'), Source(y4m_bytes(rj[:5], H, W, fmt), 'ref'), 5)
        assert net.Network.config.pipelined is state
    net.Network.set_pipelined(False)
