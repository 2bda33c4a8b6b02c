"""Whole runs of refvsr_amd.videorun.run() on the CPU (tests/test_videorun_runs.py), sync loop and stream loop: every set_pipelined /
reset / synchronize, every upload with the file frames it carries, every ops.* call with its shapes, every forward_group call with its
windows, is_first_frame and a digest of both window tensors, every event, every staging buffer given back and every sink take / put --
then the frame count, the bytes written, the score file and the fields a run leaves in its config; for a refused run the exception.

run() is driven through its public signature only, so the same file records the runs from one tree and checks another.  The net is a
stub (StubNet: the result of a window is a weighted sum over the t frames of BOTH windows, nearest-neighbour x scale -- a swapped
stream or a wrong window shows in the bytes); torch.Tensor.pin_memory is the identity, torch.Tensor.to logs a move to a device,
torch.cuda.Event / Stream / stream / synchronize are fakes that log; the seven ops entry points of the loops answer from the host
models (yuv.luma_sad, yuv.yuv_to_rgb, resize.resize_aa_model, metrics.score_frames_model, yuv.rgb_to_yuv, jpeg.encode_model /
jpeg.entropy_data); streamio.FrameSource.give, FrameSink.take / put and the two writers' constructors are wrapped on their classes.
Only calls made on the caller's thread are logged: the reader and writer threads leave no line, so the sequence is deterministic.
Wall times are not recorded.

Recording (from the repository root, with the videorun.py to be pinned in the tree):
    python tests/videorun_trace.py tests/golden/videorun_runs.json
"""
import collections
import contextlib
import hashlib
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'config_RefVSR_small_L1'
H, W, T, G, NA, NB = 16, 24, 3, 4, 5, 6          # file frames, window, group; 11 frames with a cut at 5
T_CUT = 0.1
REL = 1e-9               # floats of the score file and of EVAL.scores: the host models' float64 sums through another libm
FLOAT = re.compile(r'-?\d+\.\d+(?:e[-+]?\d+)?|inf|nan')
FIELDS = ('input_yuv', 'input_yuv_siting', 'input_yuv_range', 'result_yuv', 'yuv_siting', 'yuv_matrix', 'yuv_range')
EVAL_FIELDS = ('in_down', 'out_size', 'score_file', 'out_yuv', 'out_format', 'jpeg_quality', 'scene_cuts')
COUNTERS = ('frames', 'uploads', 'groups', 'max_in_flight', 'max_held')
# the one refusal run() and build_config worded differently; the fold keeps build_config's words, which end before this clause
SCORE_CLAUSE = ': the result is scored against the file frame'


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def _np(x):
    """A tensor or an array, or a list of them of one shape, as one numpy array."""
    one = lambda f: f.detach().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)          # noqa: E731
    return one(x) if isinstance(x, (torch.Tensor, np.ndarray)) else np.stack([one(f) for f in x])


def _what(x):
    a = _np(x)
    return '%s%s' % (a.dtype.name, list(a.shape))


class Trace(object):
    """The log of one run and what it needs to name things: the file frames by their bytes, the events by their order."""

    def __init__(self):
        self.lines, self.frames, self.events, self.sources, self.sinks, self.nets, self.memo = [], {}, 0, [], [], [], {}

    def start(self, frames):
        del self.lines[:], self.sources[:], self.sinks[:], self.nets[:]
        self.frames, self.events = frames, 0

    def log(self, line):
        self.lines.append(line)

    def names(self, x):
        """The file frames of [.., rows, w] buffers: L3 the LR stream's frame 3, R3 the reference's; '?' what is neither."""
        a = _np(x)
        a = a.reshape((-1,) + a.shape[-2:])
        return ','.join(self.frames.get(digest(f), '?') for f in a)

    def cached(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]


# ---------------------------------------------------------------------------------------------------------------- the stub net
class StubNetwork(object):
    def __init__(self, tr, config, engines, raise_at):
        self.tr, self.config, self._engines, self.raise_at, self.n = tr, config, engines, raise_at, 0

    def reset(self):
        self.tr.log('reset')

    def set_pipelined(self, on=True):
        self.tr.log('set_pipelined(%s)' % on)
        self.config.pipelined = bool(on)

    def forward_group(self, lrs, rfs, wins, is_first_frame=False, **kw):
        from refvsr_amd import yuv
        self.tr.log('forward_group wins=%s first=%s kw=%s lrs=%s:%s rfs=%s:%s' % (
            json.dumps(wins, separators=(',', ':')), is_first_frame, json.dumps(kw, sort_keys=True), _what(lrs), digest(_np(lrs)), _what(rfs), digest(_np(rfs))))
        assert lrs.shape == rfs.shape and lrs.dtype == rfs.dtype and lrs.shape[0] == len(wins) and all(len(w_) == lrs.shape[1] for w_ in wins)
        self.n += 1
        if self.n == self.raise_at:
            raise RuntimeError('stub: forward_group call %d fails' % self.n)
        nc = self.config
        a, b = _np(lrs), _np(rfs)
        if nc.get('input_yuv'):
            p = yuv.resolve_input(nc.input_yuv, nc.get('input_yuv_matrix'), nc.get('input_yuv_range'), nc.get('input_yuv_chroma'), nc.get('input_yuv_siting'))
            assert a.ndim == 4
            rows, w = a.shape[-2:]
            h = rows * {'420': 2, '422': 1, '444': 1}[yuv.sampling_of(p[0])] // {'420': 3, '422': 2, '444': 3}[yuv.sampling_of(p[0])]
            a, b = (np.stack([yuv.yuv_to_rgb(x, h, w, *p) for x in v]) for v in (a, b))
        else:
            assert a.ndim == 5 and a.shape[2] == 3
            a, b = ((v.astype(np.float32) / np.float32(255.0)) if v.dtype == np.uint8 else v.astype(np.float32) for v in (a, b))
        t, s = a.shape[1], int(nc.scale)
        wl = np.arange(1, t + 1, dtype=np.float64).reshape(1, t, 1, 1, 1)
        y = ((a.astype(np.float64) * wl).sum(1) + (b.astype(np.float64) * (wl + t)).sum(1)) / float(t * (2 * t + 1))
        y = np.clip(y, 0.0, 1.0).astype(np.float32).repeat(s, axis=-2).repeat(s, axis=-1)
        out = collections.OrderedDict(result=tuple(torch.from_numpy(f.copy())[None] for f in y))
        if nc.get('result_yuv'):
            out['yuv'] = tuple(torch.from_numpy(yuv.rgb_to_yuv(f, nc.result_yuv, nc.get('yuv_matrix') or 'bt709', nc.get('yuv_range') or 'limited',
                                                               nc.get('yuv_siting') or 'centre'))[None] for f in y)
        return out


class StubNet(object):
    """What videorun uses of an SRNet.  engines: what Network._engines holds; raise_at: the n-th forward_group call fails."""

    def __init__(self, tr, config, engines=(), raise_at=None):
        self.Network = StubNetwork(tr, config, list(engines), raise_at)
        self._p = torch.zeros(1)

    def parameters(self):
        return iter([self._p])

    def to(self, *a, **k):
        return self

    def eval(self):
        return self


# ---------------------------------------------------------------------------------------------------------------- the patches
def patch_all(setattr_, tr):
    """Install the fakes (setattr_(obj, name, value): monkeypatch.setattr or the recorder's own); they log to tr."""
    import refvsr_amd
    from refvsr_amd import jpeg, metrics, ops, resize, streamio, yuv

    real_to = torch.Tensor.to

    def to(self, *a, **k):
        if (a and isinstance(a[0], (str, torch.device))) or 'device' in k:
            tr.log('upload %s %s' % (_what(self), tr.names(self) if self.dim() >= 2 else '-'))
        return real_to(self, *a, **k)

    class Event(object):
        def __init__(self, *a, **k):
            self.k = tr.events
            tr.events += 1

        def record(self, *a):
            tr.log('event %d record' % self.k)

        def synchronize(self):
            tr.log('event %d synchronize' % self.k)

    class Stream(object):
        def __init__(self, *a, **k):
            tr.log('cuda.Stream')

        def synchronize(self):
            tr.log('stream synchronize')

    def luma_sad(fa, fb, h, w, fmt):
        tr.log('ops.luma_sad B=%d %s %dx%d %s a=%s b=%s' % (len(fa), _what(fa), h, w, fmt, tr.names(fa), tr.names(fb)))
        return torch.tensor([yuv.luma_sad(a, b, h, w, fmt) for a, b in zip(_np(fa), _np(fb))], dtype=torch.int64)

    def yuv_to_frames(x, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear', siting='centre'):
        tr.log('ops.yuv_to_frames %s %dx%d %s %s %s %s %s frames=%s' % (_what(x), h, w, fmt, matrix, range, chroma, siting, tr.names(x)))
        a = _np(x)
        return torch.from_numpy(np.stack([tr.cached(('dec', digest(f), h, w, fmt, matrix, range, chroma, siting),
                                                    lambda: yuv.yuv_to_rgb(f, h, w, fmt, matrix, range, chroma, siting)) for f in a]))

    def resize_aa(frames, oh, ow, out='float32', clamp=True):
        a = _np(frames)
        tr.log('ops.resize_aa B=%d %s -> %dx%d %s clamp=%s' % (len(a), _what(frames), oh, ow, out, clamp))
        return torch.from_numpy(np.stack([tr.cached(('aa', digest(f), f.shape, oh, ow, out, clamp), lambda: resize.resize_aa_model(f, oh, ow, out, clamp))
                                          for f in a]))

    def score_frames(outs, gts, win=7, down=1):
        a, b = _np(outs), _np(gts)
        tr.log('ops.score_frames B=%d win=%d down=%d out=%s gt=%s:%s' % (len(a), win, down, _what(outs), _what(gts), ','.join(digest(g) for g in b)))
        assert a.dtype == b.dtype == np.float32 and down == 1
        return torch.tensor([tr.cached(('sc', digest(x), digest(g), win), lambda: metrics.score_frames_model(x, g, win=win)) for x, g in zip(a, b)],
                            dtype=torch.float64)

    def result_to_yuv(frames, fmt='i422', matrix='bt709', range='limited', siting='centre'):
        tr.log('ops.result_to_yuv B=%d %s %s %s %s %s' % (len(frames), _what(frames), fmt, matrix, range, siting))
        return torch.from_numpy(yuv.rgb_to_yuv(_np(frames), fmt, matrix, range, siting))

    def entropy(f, h, w, fmt, quality, restart):
        return tr.cached(('jpg', digest(f), h, w, fmt, quality, restart), lambda: jpeg.entropy_data(f, h, w, fmt, quality, restart))

    def jpeg_encode(ys, h, w, fmt, quality=90, restart=None):
        tr.log('ops.jpeg_encode B=%d %s %dx%d %s q=%s' % (len(ys), _what(ys), h, w, fmt, quality))
        head = jpeg.header(h, w, fmt, quality, restart)
        return [jpeg.assemble(head, entropy(f, h, w, fmt, quality, restart)) for f in _np(ys)]

    def jpeg_encode_device(ys, h, w, fmt, quality=90, restart=None):
        tr.log('ops.jpeg_encode_device B=%d %s %dx%d %s q=%s' % (len(ys), _what(ys), h, w, fmt, quality))
        datas = [entropy(f, h, w, fmt, quality, restart) for f in _np(ys)]
        bound = jpeg.capacity(h, w, fmt, restart)
        dst = np.zeros(len(datas) * bound, np.uint8)
        for i, d in enumerate(datas):
            dst[i * bound:i * bound + len(d)] = np.frombuffer(d, np.uint8)
        return (torch.from_numpy(dst), torch.tensor([i * bound for i in range(len(datas))], dtype=torch.int64),
                torch.tensor([len(d) for d in datas], dtype=torch.int64))

    def wrap(cls, name, line, keep=None):
        real = getattr(cls, name)

        def method(self, *a, **k):
            if keep is not None:
                keep.append(self)
            text = line(self, *a, **k)
            if text:
                tr.log(text)
            return real(self, *a, **k)
        setattr_(cls, name, method)

    setattr_(torch.Tensor, 'pin_memory', lambda self, *a, **k: self)
    setattr_(torch.Tensor, 'to', to)
    setattr_(torch.cuda, 'Event', Event)
    setattr_(torch.cuda, 'Stream', Stream)
    setattr_(torch.cuda, 'stream', lambda s: contextlib.nullcontext())
    setattr_(torch.cuda, 'synchronize', lambda *a, **k: tr.log('cuda.synchronize'))
    for name, fake in (('luma_sad', luma_sad), ('yuv_to_frames', yuv_to_frames), ('resize_aa', resize_aa), ('score_frames', score_frames),
                       ('result_to_yuv', result_to_yuv), ('jpeg_encode', jpeg_encode), ('jpeg_encode_device', jpeg_encode_device)):
        setattr_(ops, name, fake)
    setattr_(refvsr_amd, 'SRNet', lambda config: tr.nets.append(StubNet(tr, config)) or tr.nets[-1])
    wrap(streamio.FrameSource, '__init__', lambda self, *a, **k: None, tr.sources)
    wrap(streamio.FrameSource, 'give', lambda self, buf: 'give %s' % tr.names(buf))
    wrap(streamio.FrameSink, '__init__', lambda self, *a, **k: None, tr.sinks)
    wrap(streamio.FrameSink, 'take', lambda self: 'sink.take')
    wrap(streamio.FrameSink, 'put', lambda self, buf, length=None, data=None: 'sink.put%s%s' % (
        '' if length is None else ' length=%d' % length, '' if data is None else ' data=%d' % len(data)))
    wrap(yuv.Y4MWriter, '__init__', lambda self, path, h, w, fmt='i420', fps=(30, 1), range='limited', siting=None:
         'Y4MWriter %dx%d %s fps=%d:%d %s siting=%s' % (h, w, fmt, fps[0], fps[1], range, siting))
    wrap(jpeg.MJPEGWriter, '__init__', lambda self, path: 'MJPEGWriter')


# ---------------------------------------------------------------------------------------------------------------- the data
def clip_frames(fmt, h, w):
    """11 frames of each stream with a cut at 5: two synth clips of different seeds, their motion scaled to a tenth (the detector then
    fires at the cut alone), as frames of `fmt`, BT.709 limited."""
    from refvsr_amd import yuv
    from refvsr_amd.synth import make_clip
    out = [[], []]
    for n, seed in ((NA, 21), (NB, 22)):
        for j, x in enumerate(make_clip(n, h, w, seed=seed, want_gt=False)[:2]):
            out[j].extend(yuv.rgb_to_yuv(f, fmt, 'bt709', 'limited', 'centre') for f in (0.9 * x[:1] + 0.1 * x).numpy())
    return out


class Data(object):
    """The input files of the scenarios, written once: pair(fmt, h, w, n, ..) -> (lr path, ref path, {digest: 'L3' | 'R3'})."""

    def __init__(self, tmp):
        self.tmp, self.clips, self.made = tmp, {}, {}

    def pair(self, fmt='i420', h=H, w=W, n=NA + NB, ref_n=None, cut_bytes=0, range='limited'):
        from refvsr_amd import yuv
        key = (fmt, h, w, n, ref_n, cut_bytes, range)
        if key not in self.made:
            if (fmt, h, w) not in self.clips:
                self.clips[(fmt, h, w)] = clip_frames(fmt, h, w)
            lr, rf = self.clips[(fmt, h, w)]
            paths, names = [], {}
            for tag, x, k in (('uw', lr, n), ('w', rf, n if ref_n is None else ref_n)):
                paths.append(os.path.join(self.tmp, '%s_%s.y4m' % (tag, '_'.join(str(v) for v in key))))
                with yuv.Y4MWriter(paths[-1], h, w, fmt, (24, 1), range) as wr:
                    for i, f in enumerate(x[:k]):
                        wr.write(f)
                        names[digest(f)] = '%s%d' % ('L' if tag == 'uw' else 'R', i)
            if cut_bytes:
                with open(paths[0], 'r+b') as fh:
                    fh.truncate(os.path.getsize(paths[0]) - cut_bytes)
            self.made[key] = (paths[0], paths[1], names)
        return self.made[key]


# ---------------------------------------------------------------------------------------------------------------- scenarios
def scenarios():
    """name -> dict(io, eval: EVAL fields, data: Data.pair arguments, t, net: StubNet options, own_config: the net's config is a copy,
    pipelined: the state on entry, ext: the output's extension, main: argv of videorun.main instead of run(), raises, racy: the error
    comes from a reader thread, at a moment that is the scheduler's -- the sequence is not kept).  Every case that both loops
    run is there twice, '<case> [sync]' and '<case> [stream]'."""
    sc = collections.OrderedDict()

    def add(name, modes=('sync', 'stream'), **k):
        for io_ in modes:
            sc['%s [%s]' % (name, io_)] = dict(dict(io=io_, eval={}, data={}, t=T, net={}, own_config=False, pipelined=False, ext='y4m',
                                                    main=None, raises=False, racy=False), **k)
    big = dict(h=4 * H, w=4 * W)
    for fmt in ('i420', 'i420p10'):
        add('plain %s' % fmt, data=dict(fmt=fmt))
        add('cuts %s' % fmt, data=dict(fmt=fmt), eval=dict(cuts=(NA,)))
        add('scene_cut %s' % fmt, data=dict(fmt=fmt), eval=dict(scene_cut=T_CUT))
    add('out_chroma 422', eval=dict(out_chroma='422'))
    add('out_chroma 444 depth 10', eval=dict(out_chroma='444', video_depth=10))
    add('in_siting left', eval=dict(in_siting='left'))
    add('out_siting left cuts', eval=dict(out_siting='left', cuts=(NA,)))
    add('in_down', data=big, eval=dict(in_down=4))
    add('in_down i420p10', data=dict(big, fmt='i420p10', n=6), eval=dict(in_down=4))
    add('in_down score', data=big, eval=dict(in_down=4, score_file=True))
    add('out_size', eval=dict(out_size='48x32'))
    add('in_down score out_size', data=big, eval=dict(in_down=4, score_file=True, out_size=(48, 32)))
    add('in_down score out_size scene_cut', data=big, eval=dict(in_down=4, score_file=True, out_size=(48, 32), scene_cut=T_CUT))
    add('mjpeg', eval=dict(out_format='mjpeg', cuts=(NA,)))
    add('mjpeg by extension out_size 444', eval=dict(out_size='48x32', out_chroma='444', jpeg_quality=75), ext='mjpeg')
    for n in (1, 2, 5):
        add('t 5 n %d' % n, t=5, data=dict(n=n))
    add('io_depth 1', ('stream',), eval=dict(io_depth=1))
    add('io_depth 3 scene_cut', ('stream',), eval=dict(io_depth=3, scene_cut=T_CUT))
    add('own config', own_config=True, eval=dict(in_siting='left', video_depth=10))
    add('own config mjpeg', own_config=True, eval=dict(out_format='mjpeg'), data=dict(n=5))
    add('pipelined on entry', pipelined=True, data=dict(n=5))
    # refusals
    add('length mismatch', data=dict(ref_n=NA + NB - 1), raises=True)
    add('truncated input', ('sync',), data=dict(cut_bytes=5), raises=True)
    add('truncated input', ('stream',), data=dict(cut_bytes=5), raises=True, racy=True)
    add('cuts beyond the end', eval=dict(cuts=(NA, NA + NB)), raises=True)
    add('scene_cut with cuts', eval=dict(scene_cut=T_CUT, cuts=(NA,)), raises=True)
    add('score_file without in_down', eval=dict(score_file=True), raises=True)
    add('mjpeg out_chroma 422', ('sync',), eval=dict(out_format='mjpeg', out_chroma='422'), raises=True)
    add('mjpeg video_depth 10', ('stream',), eval=dict(out_format='mjpeg', video_depth=10), raises=True)
    add('mjpeg out_siting left', ('sync',), eval=dict(out_format='mjpeg', out_siting='left'), raises=True)
    add('engines of the other kind', data=big, eval=dict(in_down=4), net=dict(engines=('i420', 'i420')), raises=True)
    add('engines with result_yuv under out_size', ('sync',), eval=dict(out_size='48x32'), net=dict(engines=('i420', 'i420')), raises=True)
    add('net raises in call 2', net=dict(raise_at=2), raises=True)
    # build_config + main(): the output keeps the input's range unless --yuv_range is given; the files say full range
    add('main range of the file', data=dict(range='full', n=5), main=[])
    add('main yuv_range limited', data=dict(range='full', n=5), main=['--yuv_range', 'limited'])
    return sc


def pairs():
    """The cases both loops run: [(case, sync name, stream name)]."""
    names = list(scenarios())
    return [(n[:-7], n, n[:-7] + ' [stream]') for n in names if n.endswith(' [sync]') and n[:-7] + ' [stream]' in names]


def run_scenario(sc, tr, data, out_dir):
    """One run() (or main()) call -> what the golden file keeps of it."""
    import copy

    from refvsr_amd import get_config, videorun
    os.makedirs(out_dir)
    lr, ref, names = data.pair(**sc['data'])
    tr.start(names)
    out = os.path.join(out_dir, 'sr.' + sc['ext'])
    score = os.path.join(out_dir, 'scores.txt')
    mask = lambda s: s.replace(data.tmp + os.sep, '')                                  # noqa: E731
    rec = collections.OrderedDict()
    raised, frames, printed = None, None, None
    if sc['main'] is not None:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            code = videorun.main(['--config', NAME, '--lr', lr, '--ref', ref, '--out', out, '--frame_num', str(sc['t']), '--frame_group', str(G),
                                  '--io', sc['io']] + sc['main'])
        net, = tr.nets                                          # (built by run() itself: the fake refvsr_amd.SRNet)
        cfg = net.Network.config
        printed = [re.sub(r'\d+\.\d{5} sec', '<sec> sec', re.sub(r'\d+\.\d{3} s ', '<s> s ', mask(ln))) for ln in buf.getvalue().split('\n') if ln]
        rec['exit'], frames = code, int(re.search(r'\] (\d+) frames', printed[0]).group(1))
    else:
        cfg = get_config('p', 'm', NAME)
        cfg.frame_num, cfg.save_sample = sc['t'], False
        cfg.EVAL.frame_group, cfg.EVAL.io = G, sc['io']
        if sc['io'] == 'stream':
            cfg.EVAL.io_timeout = 20
        for k, v in sc['eval'].items():
            setattr(cfg.EVAL, k, score if k == 'score_file' else v)
        nc = copy.deepcopy(cfg) if sc['own_config'] else cfg
        nc.pipelined = sc['pipelined']
        opts = dict(sc['net'])
        if 'engines' in opts:
            opts['engines'] = [type('Eng', (), dict(input_yuv=opts['engines'][0], result_yuv=opts['engines'][1]))()]
        net = StubNet(tr, nc, **opts)
        try:
            frames, _ = videorun.run(cfg, lr, ref, out, net=net)
        except (ValueError, RuntimeError) as e:
            raised = '%s: %s' % (type(e).__name__, mask(str(e)).replace(SCORE_CLAUSE, ''))
    assert (raised is not None) == sc['raises'], raised
    rec['raised'], rec['frames'], rec['seq'] = raised, frames, [] if sc['racy'] else list(tr.lines)
    if printed is not None:
        rec['printed'] = printed
    # (a stream run that ends in an error stops its writer thread wherever it is: what is on the disk then is not pinned)
    written = open(out, 'rb').read() if os.path.exists(out) and not (raised and sc['io'] == 'stream') else None
    rec['bytes'] = None if written is None else [len(written), hashlib.sha256(written).hexdigest()]
    if written is not None and sc['ext'] == 'y4m' and cfg.EVAL.get('out_format') != 'mjpeg':
        rec['header'] = written[:written.index(b'\n')].decode('ascii') if b'\n' in written else None
    rec['score'] = open(score).read().split('\n') if os.path.exists(score) else None
    E = cfg.EVAL
    left = collections.OrderedDict((k, cfg.get(k, '<unset>')) for k in FIELDS)
    left.update(('EVAL.' + k, mask(E[k]) if isinstance(E.get(k), str) else E.get(k, '<unset>')) for k in EVAL_FIELDS)
    left['EVAL.scores'] = [list(s) for s in E.scores] if 'scores' in E else '<unset>'
    left['EVAL.io_stats'] = [E.io_stats[k] for k in COUNTERS] if 'io_stats' in E else '<unset>'
    left['net.pipelined'] = net.Network.config.get('pipelined', '<unset>')
    if sc['own_config']:
        left['net.config'] = [net.Network.config.get(k, '<unset>') for k in FIELDS]
    left['outstanding'] = [x.outstanding for x in tr.sources + tr.sinks]
    if raised is not None and not raised.startswith('RuntimeError: stub:'):
        # a refused run is pinned by its exception and by the calls before it: how far it got with EVAL on the way is the module's own
        left = collections.OrderedDict([('net.pipelined', left['net.pipelined'])])
    rec['left'] = json.loads(json.dumps(left), object_pairs_hook=collections.OrderedDict)          # (tuples as the lists the file holds)
    return rec


def record(setattr_, only=None):
    """{scenario: what run_scenario keeps}, every scenario on a fresh output folder; the input files are written once."""
    tr = Trace()
    patch_all(setattr_, tr)
    tmp = tempfile.mkdtemp(prefix='videorun_trace_')
    try:
        data = Data(tmp)
        out = collections.OrderedDict()
        for i, (name, sc) in enumerate(scenarios().items()):
            if only is None or name in only:
                out[name] = run_scenario(sc, tr, data, os.path.join(tmp, 'out%02d' % i))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- comparison
def same(got, want, where=''):
    """Everything exact, except floats and the floats printed in the score file: within REL of their size."""
    if isinstance(want, str):
        assert isinstance(got, str) and FLOAT.sub('#', got) == FLOAT.sub('#', want), '%s: %r, recorded %r' % (where, got, want)
        for a, b in zip(FLOAT.findall(got), FLOAT.findall(want)):
            same(float(a), float(b), where)
    elif isinstance(want, float):
        assert isinstance(got, float) and (got == want or abs(got - want) <= REL * abs(want)), '%s: %r, recorded %r' % (where, got, want)
    elif isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), '%s: keys %s, recorded %s' % (where, list(got), list(want))
        for k in want:
            same(got[k], want[k], '%s.%s' % (where, k))
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)), where
        for i, (a, b) in enumerate(zip(got, want)):
            same(a, b, '%s[%d]' % (where, i))
        assert len(got) == len(want), '%s: %d entries, recorded %d' % (where, len(got), len(want))
    else:
        assert got == want and type(got) is type(want), '%s: %r, recorded %r' % (where, got, want)


def load(path):
    """The golden file with every run's `seq` as its lines again (the file holds each distinct line once, in `_lines`)."""
    with open(path) as fh:
        g = json.load(fh, object_pairs_hook=collections.OrderedDict)
    lines = g.pop('_lines')
    for name, sc in g.items():
        if name != '_recorded_from':
            sc['seq'] = [lines[i] for i in sc['seq']]
    return g


def main(argv):
    sys.path.insert(0, ROOT)
    undo = []

    def setattr_(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        rec = record(setattr_)
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
    commit = argv[2] if len(argv) > 2 else subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT).decode().strip()
    lines = collections.OrderedDict()
    for sc in rec.values():
        sc['seq'] = [lines.setdefault(ln, len(lines)) for ln in sc['seq']]
    parts = ['"_recorded_from": %s' % json.dumps(dict(commit=commit, file='refvsr_amd/videorun.py'), sort_keys=True),
             '"_lines": [\n%s]' % ',\n'.join(json.dumps(ln) for ln in lines)]
    for name, sc in rec.items():                                # a line per key of a scenario
        parts.append('%s: {%s}' % (json.dumps(name), ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':') if k == 'seq' else None))
                                                                 for k, v in sc.items())))
    with open(argv[1], 'w') as fh:
        fh.write('{\n' + ',\n'.join(parts) + '\n}\n')
    print('%d scenarios, %d distinct lines recorded from %s -> %s' % (len(rec), len(lines), commit[:12], argv[1]))


if __name__ == '__main__':
    main(sys.argv)
