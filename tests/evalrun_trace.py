"""Whole runs of refvsr_amd.evalrun.evaluate() on the CPU (tests/test_evalrun_runs.py): which network entry every frame takes and with
which arguments, when the state is reset and pipelining switched, which scorer / colour launch follows which call, the score file, the
log lines, the output tree and the returned dict -- for every mode and option of the loop.

evaluate() is driven through its public signature only, so the same file records the runs from one tree and checks another.  The net
is a stub (StubNet: the result of a window is its centre LR frame, bilinear x scale); torch.cuda.synchronize and the three device entry
points of the loop (ops.score_frames, ops.score_regions, ops.conf_colormap) are replaced by fakes that log and answer from the host
models of refvsr_amd/metrics.py; yuv.Y4MWriter is a subclass that remembers its instances.  The data set is
tools/make_synth_dataset.make(root, clips=2, frames=5, h=16, w=24).

Recording (from the repository root, with the evalrun.py to be pinned in the tree):
    python tests/evalrun_trace.py tests/golden/evalrun_runs.json
"""
import collections
import hashlib
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
CLIPS, FRAMES, H, W = 2, 5, 16, 24
TOL = 1.5e-5             # one unit of the fifth printed decimal for a rounding flip + half a unit (the host PSNR is a float32 mean)
SEC = re.compile(r'\(\d+\.\d{5}sec\)')
NUM = re.compile(r'-?\d+\.\d{5}(?!\d)')


# ---------------------------------------------------------------------------------------------------------------- the stub net
def upsample(x, s):
    """Bilinear x s of [3,h,w] (align_corners=False, edges clamped) from separately rounded float32 products: the same bits everywhere."""
    for axis in (-1, -2):
        n = x.shape[axis]
        src = ((torch.arange(n * s, dtype=torch.float32) + 0.5) / s - 0.5).clamp(min=0)
        i0 = src.floor().long()
        i1 = (i0 + 1).clamp(max=n - 1)
        f = (src - i0.float()).reshape([-1] + [1] * (-1 - axis))
        x = x.index_select(axis, i0) * (1 - f) + x.index_select(axis, i1) * f
    return x


class StubNetwork(object):
    def __init__(self, calls, config, pipelined):
        self.calls, self.config = calls, config
        self._engines = [type('Eng', (), dict(pipelined=pipelined))()]

    def reset(self):
        self.calls.append('reset')

    def set_pipelined(self, on=True):
        self.calls.append('set_pipelined(%s)' % on)
        self._engines[0].pipelined = bool(on)


class StubNet(object):
    """What evaluate() uses of an SRNet.  u8: the results are bytes (config.result_dtype = 'uint8'); raise_at: the n-th network call fails."""

    def __init__(self, calls, scale, result_yuv=None, u8=False, pipelined=False, raise_at=None):
        from refvsr_amd.config import AttrDict
        self.calls, self.scale, self.u8, self.raise_at, self.n = calls, int(scale), u8, raise_at, 0
        self.Network = StubNetwork(calls, AttrDict(save_sample=False, result_yuv=result_yuv), pipelined)
        self._p = torch.zeros(1)

    def parameters(self):
        return iter([self._p])

    def _count(self):
        self.n += 1
        if self.n == self.raise_at:
            raise RuntimeError('stub: network call %d fails' % self.n)

    def _window(self, lr_c):
        """(result [1,3,sh,sw], the four maps of 'eval_vis' [1,1,h,w], 'yuv' [1,3sh/2,sw] bytes) of one window's centre frame."""
        x = (lr_c.float() / 255.0 if lr_c.dtype == torch.uint8 else lr_c.float()).contiguous()
        y = upsample(x, self.scale).clamp(0, 1)
        b = torch.round(y * 255.0).to(torch.uint8)
        vis = collections.OrderedDict((k, m[None, None].contiguous()) for k, m in (
            ('conf_map', x[0]), ('conf_map_prop', x[1] * 0.5), ('conf_map_prop_backward', x[2] - x[0]), ('conf_map_prop_forward', x[1] * x[2])))
        yuv = torch.cat([b[1].reshape(-1), b[2][::2, ::2].reshape(-1), b[0][::2, ::2].reshape(-1)]).reshape(1, 3 * b.shape[1] // 2, b.shape[2])
        return (b if self.u8 else y)[None], vis, yuv

    def __call__(self, lr, rf, is_first, is_log=False, is_train=False, frame_ids=None):
        self.calls.append('net(is_first=%s, is_log=%s, frame_ids=%s) lr=%s' % (is_first, is_log, _ids(frame_ids), _what(lr)))
        assert lr.shape == rf.shape and lr.dim() == 5 and lr.shape[0] == 1 and is_train is False
        self._count()
        res, vis, yuv = self._window(lr[0, lr.shape[1] // 2])
        out = collections.OrderedDict(result=res)
        if is_log and self.Network.config.save_sample:
            out['eval_vis'] = vis
        if self.Network.config.result_yuv:
            out['yuv'] = yuv
        return out

    def forward_group(self, lrs, rfs, ids, is_first_frame=False, **kw):
        self.calls.append('forward_group(ids=%s, is_first_frame=%s, kwargs=%s) lrs=%s' % (
            '[%s]' % ' '.join(_ids(i) for i in ids), is_first_frame, json.dumps(kw, sort_keys=True), _what(lrs)))
        assert lrs.shape == rfs.shape and lrs.dim() == 5 and lrs.shape[0] == len(ids)
        self._count()
        wins = [self._window(lrs[b, lrs.shape[1] // 2]) for b in range(lrs.shape[0])]
        out = collections.OrderedDict(result=tuple(w[0] for w in wins))
        if kw.get('want_conf'):
            out['eval_vis'] = tuple(w[1] for w in wins)
        if self.Network.config.result_yuv:
            out['yuv'] = tuple(w[2] for w in wins)
        return out


def _ids(fid):
    return '-' if fid is None else '(%s)' % ','.join('%d:%d' % (v, i) for v, i in fid)


def _what(t):
    return '%s%s' % (str(t.dtype).split('.')[1], list(t.shape))


def _vals(t):
    """The float32 values a scorer sees: a byte means byte / 255."""
    t = t.detach().cpu()
    return (t.float() / 255.0 if t.dtype == torch.uint8 else t.float()).contiguous().numpy()


# ---------------------------------------------------------------------------------------------------------------- the patches
def patch_all(setattr_, calls, writers):
    """Install the fakes (setattr_(obj, name, value): monkeypatch.setattr or the recorder's own); they log to `calls` / `writers`."""
    from refvsr_amd import metrics, ops, yuv

    def score_frames(outs, gts, win=7, down=1):
        calls.append('score_frames B=%d down=%d win=%d out=%s gt=%s' % (len(outs), down, win, _what(outs[0]), _what(gts[0])))
        sc = [metrics.score_frames_model(_vals(o), _vals(g), win=win) if down == 1 else metrics.score_frames_down_model(_vals(o), _vals(g), down, win=win)
              for o, g in zip(outs, gts)]
        return torch.tensor(sc, dtype=torch.float64)

    def score_regions(outs, gts, rects):
        calls.append('score_regions B=%d down=1 rects=%d out=%s gt=%s' % (len(outs), len(rects), _what(outs[0]), _what(gts[0])))
        return torch.from_numpy(np.stack([metrics.host_region_sums(_vals(o), _vals(g), rects) for o, g in zip(outs, gts)]))

    def conf_colormap(maps):
        """A fixed stand-in for the inferno colouring (the GPU tests pin the colours): grey levels of the min/max-normalised map."""
        maps = list(maps)
        calls.append('conf_colormap B=%d down=1 map=%s' % (len(maps), _what(maps[0])))
        out = []
        for m in maps:
            a = m.reshape(m.shape[-2:]) - m.min()
            span = a.max()
            g = torch.round(a / span * 255.0).to(torch.uint8) if float(span) > 0 else torch.zeros(a.shape, dtype=torch.uint8)
            out.append(torch.stack([g, 255 - g, g // 2], dim=-1))
        return out

    real_writer = yuv.Y4MWriter

    class Writer(real_writer):
        def __init__(self, path, *a, **k):
            real_writer.__init__(self, path, *a, **k)
            self.path = path
            writers.append(self)

    setattr_(torch.cuda, 'synchronize', lambda *a, **k: calls.append('sync'))
    setattr_(ops, 'score_frames', score_frames)
    setattr_(ops, 'score_regions', score_regions)
    setattr_(ops, 'conf_colormap', conf_colormap)
    setattr_(yuv, 'Y4MWriter', Writer)


# ---------------------------------------------------------------------------------------------------------------- scenarios
def scenarios():
    """name -> dict(args: CLI flags, hd: a flag_HD_in config and data set, net: StubNet options, eval: EVAL fields set after the parse,
    frames: frames the run scores, raises: the run ends in the stub's exception).  2 clips x 5 frames, windows of 3."""
    sc = collections.OrderedDict()

    def add(name, args=(), frames=CLIPS * FRAMES, **k):
        sc[name] = dict(dict(args=list(args), hd=False, net={}, eval={}, frames=frames, raises=False), **k)
    add('qual_quan host group 1')
    add('qual_quan host group 3', ['--frame_group', '3'])                  # per clip: the first frame alone, a full group, a remainder of one
    add('quantitative_only', ['-quantitative_only'])
    add('qualitative_only', ['-qualitative_only'])
    add('uint8 results', net=dict(u8=True))
    add('use_frame_ids off group 3', ['--frame_group', '3'], eval=dict(use_frame_ids=False))
    add('vid_name 0002', ['--vid_name', '0002'], frames=FRAMES)
    add('metrics device group 1', ['--metrics', 'device'])
    add('metrics device group 3 quantitative_only', ['--metrics', 'device', '--frame_group', '3', '-quantitative_only'])
    add('HD host', hd=True)
    add('HD device', ['--metrics', 'device'], hd=True)
    add('FOV host group 1', ['--eval_mode', 'quan_FOV'])
    add('FOV device group 2', ['--eval_mode', 'quan_FOV', '--metrics', 'device', '--frame_group', '2'])
    add('conf_map group 1', ['--eval_mode', 'quan_conf_map'])
    add('conf_map group 2', ['--eval_mode', 'quan_conf_map', '--frame_group', '2'])
    add('y4m group 1', ['--video_out', 'y4m'])
    add('y4m group 4 uint8 input', ['--video_out', 'y4m', '--frame_group', '4', '--input_dtype', 'uint8'])
    add('net already pipelined group 2', ['--frame_group', '2'], net=dict(pipelined=True))
    add('net raises on call 4 y4m group 2', ['--video_out', 'y4m', '--frame_group', '2'], net=dict(raise_at=4), frames=FRAMES, raises=True)
    return sc


def mask(text):
    return SEC.sub('(<sec>)', text)


def tree_of(root):
    """Sorted [relative path, what it holds]: .png the digest of the decoded pixels (zlib versions differ, pixels do not), .jpg the
    decoded shape, .y4m the digest of the file."""
    from refvsr_amd import evalrun
    out = []
    for d, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(d, fn)
            if fn.endswith('.png') or fn.endswith('.jpg'):
                px = evalrun.read_frame(p, 'uint8').contiguous()
                what = 'x'.join(str(n) for n in px.shape)
                if fn.endswith('.png'):
                    what += ' ' + hashlib.sha1(px.numpy().tobytes()).hexdigest()[:16]
            else:
                with open(p, 'rb') as fh:
                    what = hashlib.sha1(fh.read()).hexdigest()[:16]
            out.append([os.path.relpath(p, root).replace(os.sep, '/'), what])
    return sorted(out)


def run_scenario(sc, data, out, calls, writers):
    """One evaluate() call -> what the golden file keeps of it."""
    from refvsr_amd import evalrun, yuv
    del calls[:], writers[:]
    name = 'config_RefVSR_small_MFID_8K' if sc['hd'] else 'config_RefVSR_small_L1'
    cfg = evalrun.build_config(['--config', name, '--mode', 'unit', '--data_offset', data['hd' if sc['hd'] else 'plain'], '--output_offset', out,
                                '--frame_num', '3'] + sc['args'])
    for k, v in sc['eval'].items():
        setattr(cfg.EVAL, k, v)
    net = StubNet(calls, cfg.scale, result_yuv=cfg.get('result_yuv'), **sc['net'])
    logged, res, raised = [], None, None
    try:
        res = evalrun.evaluate(cfg, net=net, log=lambda *a: logged.append(' '.join(str(x) for x in a)))
    except RuntimeError as e:
        if not str(e).startswith('stub:'):
            raise
        raised = '%s: %s' % (type(e).__name__, e)
    top = os.path.join(out, cfg.EVAL.eval_mode, 'seeded')
    run_root = os.path.join(top, 'RealMCVSR')                   # holds the one <date> folder of the run
    out_root = res['output_root'] if res else os.path.join(run_root, sorted(os.listdir(run_root))[0])
    score_file = res['score_file'] if res else os.path.join(top, 'score_RealMCVSR_%s.txt' % cfg.EVAL.eval_mode)
    with open(score_file) as fh:
        score = mask(fh.read())
    rec = collections.OrderedDict(raised=raised, frames=sum(ln.startswith('[EVAL ') for ln in score.split('\n')), calls=list(calls),
                                  score=score.split('\n'), log=[mask(ln) for ln in logged], tree=tree_of(out_root))
    rec['videos_closed'] = [[os.path.relpath(w.path, out_root).replace(os.sep, '/'), w.frames, w.fh is None,
                             (os.path.getsize(w.path) - len(w.header)) == w.frames * (6 + yuv.frame_bytes(w.h, w.w, w.fmt))] for w in writers]
    rec['net_after'] = dict(pipelined=net.Network._engines[0].pipelined, save_sample=[bool(cfg.save_sample), bool(net.Network.config.save_sample)])
    if res is not None:
        assert os.path.dirname(res['score_file']) == top and os.path.dirname(res['output_root']) == run_root
        r = collections.OrderedDict(keys=sorted(res), frames=res['frames'], n_seconds=len(res['seconds']), psnr=res['psnr'], ssim=res['ssim'])
        if 'fov' in res:
            r['fov'] = [np.asarray(t).tolist() for t in res['fov']]
        if 'videos' in res:
            r['videos'] = [os.path.relpath(p, out_root).replace(os.sep, '/') for p in res['videos']]
        r['score_file'] = os.path.basename(res['score_file'])
        rec['res'] = r
    return rec


def record(setattr_):
    """{scenario: what run_scenario keeps}, every scenario on a fresh output folder; the data sets are written once."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synth_dataset
    calls, writers = [], []
    patch_all(setattr_, calls, writers)
    tmp = tempfile.mkdtemp(prefix='evalrun_trace_')
    try:
        data = {'plain': os.path.join(tmp, 'ds'), 'hd': os.path.join(tmp, 'ds_hd')}
        make_synth_dataset.make(data['plain'], clips=CLIPS, frames=FRAMES, h=H, w=W)
        make_synth_dataset.make(data['hd'], clips=CLIPS, frames=FRAMES, h=H, w=W, hd=True)
        out = collections.OrderedDict()
        for i, (name, sc) in enumerate(scenarios().items()):
            out[name] = run_scenario(sc, data, os.path.join(tmp, 'out%02d' % i), calls, writers)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- comparison
def same(got, want, where=''):
    """Everything exact, except numbers printed with five decimals and floats: within TOL."""
    if isinstance(want, str):
        assert isinstance(got, str) and NUM.sub('#', got) == NUM.sub('#', want), '%s: %r, recorded %r' % (where, got, want)
        for a, b in zip(NUM.findall(got), NUM.findall(want)):
            assert abs(float(a) - float(b)) <= TOL, '%s: %s, recorded %s (in %r)' % (where, a, b, want)
    elif isinstance(want, float):
        assert isinstance(got, float) and abs(got - want) <= TOL, '%s: %r, recorded %r' % (where, got, want)
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), '%s: keys %s, recorded %s' % (where, sorted(got), sorted(want))
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
    with open(path) as fh:
        return json.load(fh, object_pairs_hook=collections.OrderedDict)


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
    head = collections.OrderedDict([('_recorded_from', dict(commit=commit, file='refvsr_amd/evalrun.py'))])

    def one(name, sc):                                          # a line per call, score line, log entry and file; the rest of a scenario a line per key
        parts = []
        for k, v in sc.items():
            if k in ('calls', 'score', 'log', 'tree') and v:
                parts.append('%s: [\n%s]' % (json.dumps(k), ',\n'.join(json.dumps(x) for x in v)))
            else:
                parts.append('%s: %s' % (json.dumps(k), json.dumps(v)))
        return '%s: {%s}' % (json.dumps(name), ',\n'.join(parts))
    with open(argv[1], 'w') as fh:
        fh.write('{\n' + ',\n'.join(one(n, s) for n, s in list(head.items()) + list(rec.items())) + '\n}\n')
    print('%d scenarios recorded from %s -> %s' % (len(rec), commit[:12], argv[1]))


if __name__ == '__main__':
    main(sys.argv)
