"""Schedule traces of refvsr_amd.engine.Engine on the CPU (tests/test_engine_schedule.py): which launch runs on which stream, behind
which waits, and which tensor is recorded on which stream -- for every call form of the engine.

An Engine is built with Engine.__new__ and driven through its public methods only (forward, forward_group, forward_multi, phase_a,
phase_a_group, phase_b1 / phase_b2 / phase_b), so the same file records the traces from one tree and checks another.
torch.cuda.Stream / Event / current_stream / device and ops.on_stream are named fakes that log; windows, frames and maps are
stand-ins whose record_stream logs; the leaves below the schedule (pyramid, prepare_frame, the backward head, _prop_step,
compute_up, _conf_vis, ops.ingest_u8, ops.yuv420_ingest, the SPyNet body) log one token each.  The window cache, the flow cache and its events are
the engine's own.  A trace line is '<current stream>| <what>'; runs of record_stream calls and of wait_event calls share a line (State.run).

Recording (from the repository root):  python tests/engine_schedule_trace.py tests/golden/engine_schedule.json
"""
import collections
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'dev'
T_FRAMES, H, W = 3, 4, 6


class State(object):
    """What the fakes write to: one per scenario."""

    def __init__(self):
        self.log, self.n_ev, self.n_st, self.n_tok = [], 0, 0, 0
        self.stack = [Stream(name='C')]
        self.spynet = self.open = None

    def cur(self):
        return self.stack[-1]

    def add(self, what):
        self.log.append('%s| %s' % (self.cur().name, what))

    def run(self, kind, who, what):
        """Consecutive record_stream calls (kind 'rs': tensor `who` on stream `what`) and consecutive wait_event calls (kind 'we': stream
        `who` for event `what`) under one current stream share a line, in order: 'rs a b > X Y; c > X' (a and b on X then Y each, then
        c on X), 'X.wait_event(e1 e2)'."""
        if self.open is None or self.open[:3] != (kind, self.cur().name, len(self.log)) or (kind == 'we' and self.open[3][0][0] != who):
            self.open = (kind, self.cur().name, len(self.log) + 1, [])
            self.log.append(None)
        items = self.open[3]
        if items and items[-1][0] == who:
            items[-1][1].append(what)
        else:
            items.append((who, [what]))
        if kind == 'we':
            self.log[-1] = '%s| %s.wait_event(%s)' % (self.cur().name, who, ' '.join(items[0][1]))
            return
        groups = []                                            # consecutive tensors with one list of streams: named once
        for name, sts in items:
            if groups and groups[-1][1] == sts:
                groups[-1][0].append(name)
            else:
                groups.append(([name], sts))
        self.log[-1] = '%s| rs %s' % (self.cur().name, '; '.join('%s > %s' % (' '.join(_ctx_names(ns)), ' '.join(sts)) for ns, sts in groups))

    def tok(self):
        self.n_tok += 1
        return self.n_tok


S = None                    # the current scenario's State
CTX = ["%slr%s'", "%sref%s'"] + [k + '(%slr%s)' for k in ['lr8', 'conf', 'idx', 'aligned', 'aligned_up'] + ['pyr%d' % l_ for l_ in range(6)]]


def _ctx_names(ns):
    """The names ns with every run that is exactly the published set of one frame (Engine._publish: CTX, in that order) as 'ctx(<frame>)'."""
    out, i = [], 0
    while i < len(ns):
        m = re.match(r"^(.*)lr(\d+)'$", ns[i])
        if m and ns[i:i + len(CTX)] == [c % m.groups() for c in CTX]:
            out.append('ctx(%slr%s)' % m.groups())
            i += len(CTX)
        else:
            out.append(ns[i])
            i += 1
    return out


class Stream(object):
    device = DEV

    def __init__(self, device=None, priority=0, name=None):
        if name is None:
            name = 'S%d' % S.n_st
            S.n_st += 1
        self.name = name

    def wait_event(self, ev):
        S.run('we', self.name, ev.name)

    def wait_stream(self, st):
        S.add('%s.wait_stream(%s)' % (self.name, st.name))

    def synchronize(self):
        S.add('%s.synchronize()' % self.name)


class Event(object):
    def __init__(self, enable_timing=False):
        self.name = 'e%d%s' % (S.n_ev, 't' if enable_timing else '')
        S.n_ev += 1
        self.stream = None

    def record(self, stream=None):
        self.stream = (stream or S.cur()).name
        S.add('%s.record(%s)' % (self.name, self.stream))

    def synchronize(self):
        S.add('%s.synchronize()' % self.name)


class OnStream(object):
    def __init__(self, st):
        self.st = st

    def __enter__(self):
        S.add('enter %s' % self.st.name)
        S.stack.append(self.st)
        return self

    def __exit__(self, *exc):
        S.stack.pop()
        S.add('exit %s' % self.st.name)
        return False


class NullCtx(object):
    def __init__(self, *a):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


class T(object):
    """A stand-in tensor: a name, a shape, a dtype and a content token (what the content compare of the window cache sees)."""
    device, is_cuda = DEV, True

    def __init__(self, name, shape, dtype=torch.float32, content=None, layout=0):
        self.name, self.shape, self.dtype, self.content, self.layout = name, tuple(shape), dtype, content, layout

    def record_stream(self, st):
        S.run('rs', self.name, st.name)

    def clone(self):
        return T(self.name + "'", self.shape, self.dtype, self.content, self.layout)

    def contiguous(self):
        return self

    def is_contiguous(self):
        return True

    def dim(self):
        return len(self.shape)

    def numel(self):
        return _numel(self.shape)

    def __getitem__(self, k):
        if isinstance(k, slice):
            n = len(range(*k.indices(self.shape[0])))
            return T('%s[%s:%s]' % (self.name, k.start, k.stop), (n,) + self.shape[1:], self.dtype)
        return T('%s[%d]' % (self.name, k), self.shape[1:], self.dtype)

    def reshape(self, *shape):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        if -1 in shape:
            rest = _numel([d for d in shape if d != -1])
            shape = tuple(self.numel() // rest if d == -1 else d for d in shape)
        return T(self.name, shape, self.dtype)

    view = reshape


YUV_DTYPES = {'nv12': torch.uint8, 'p010': torch.uint16}


def frame_shape(yuv):
    """One frame of a window: [3,h,w] RGB, or the dense 4:2:0 buffer [3h/2, w] of config.input_yuv."""
    return (3 * H // 2, W) if yuv else (3, H, W)


class Window(T):
    """A window [t,3,h,w] of the frames `nums` of a clip: lrs[i] is the frame itself ('lr5'), whatever window it is asked from.
    yuv (a format): a 4:2:0 window [t, 3h/2, w] of the format's sample type; layout: what ops.u8_layout says of a uint8 window."""

    def __init__(self, kind, nums, dtype, yuv=None, layout=0):
        T.__init__(self, '%ss[%s]' % (kind, ','.join(str(n) for n in nums)), (len(nums),) + frame_shape(yuv),
                   YUV_DTYPES[yuv] if yuv else dtype, layout=layout)
        self.kind, self.nums = kind, list(nums)

    def __getitem__(self, i):
        name = '%s%d' % (self.kind, self.nums[i])
        return T(name, self.shape[1:], self.dtype, content=name, layout=self.layout)


class Samples(T):
    """The n windows of a forward_multi call, [n,t,3,h,w]; sample b's frames are named 'b.lr5'."""

    def __init__(self, kind, nums, n, dtype, yuv=None):
        T.__init__(self, '%ss%d[%s]' % (kind, n, ','.join(str(x) for x in nums)), (n, len(nums)) + frame_shape(yuv), YUV_DTYPES[yuv] if yuv else dtype)
        self.wins = [Window('%d.%s' % (b, kind), nums, dtype, yuv) for b in range(n)]

    def __getitem__(self, b):
        return self.wins[b]


def fname(f):
    """A frame context's name: its input frame's."""
    return (f.src[0] if f.src is not None else f.lr).name.rstrip("'")


def names(xs):
    return '-' if xs is None else '[%s]' % ' '.join('-' if x is None else x.name for x in xs)


class Named(dict):
    def __init__(self, make):
        dict.__init__(self)
        self.make = make

    def __missing__(self, name):
        return self.make(name)

    def get(self, name, default=None):
        return self.make(name)


CW = collections.namedtuple('CW', 'name raw')


def patch_all(setattr_):
    """Install the fakes (setattr_(obj, name, value): monkeypatch.setattr or the recorder's own)."""
    from refvsr_amd import engine, ops
    setattr_(torch.cuda, 'Stream', Stream)
    setattr_(torch.cuda, 'Event', Event)
    setattr_(torch.cuda, 'current_stream', lambda dev=None: S.cur())
    setattr_(torch.cuda, 'device', NullCtx)
    setattr_(ops, 'on_stream', OnStream)
    empty, zeros, cat = torch.empty, torch.zeros, torch.cat

    def fake_alloc(real, tag):
        def alloc(shape, *a, **k):
            if k.get('device') == DEV:
                return T('%s%d' % (tag, S.tok()), shape, k.get('dtype', torch.float32))
            return real(shape, *a, **k)
        return alloc
    setattr_(torch, 'empty', fake_alloc(empty, 'buf'))
    setattr_(torch, 'zeros', fake_alloc(zeros, 'zero'))
    setattr_(torch, 'cat', lambda ts, dim=0: T('cat(%s)' % ','.join(t.name for t in ts), (sum(t.shape[0] for t in ts),) + ts[0].shape[1:])
             if isinstance(ts[0], T) else cat(ts, dim))

    def ingest_u8(pairs):
        if pairs:
            S.add('ingest_u8 %s' % names([src for src, _ in pairs]))
    setattr_(ops, 'ingest_u8', ingest_u8)
    setattr_(ops, 'u8_layout', lambda x: x.layout)

    def yuv420_ingest(pairs, *params):
        if pairs:
            S.add('yuv420_ingest %s %s' % (' '.join(params), names([src for src, _ in pairs])))
    setattr_(ops, 'yuv420_ingest', yuv420_ingest)
    setattr_(ops, 'yuv_window_kind', lambda x, fmt: ('yuv', fmt) if x.dtype == YUV_DTYPES[fmt] and x.shape[-2] % 3 == 0 else None)
    setattr_(ops, 'yuv_geometry', lambda x: (2 * x.shape[-2] // 3, x.shape[-1]))
    setattr_(ops, 'conf_alpha_ok', lambda cw, B=None: True)

    def equal(what):
        def same(pairs):
            if pairs:
                S.add('compare %s%d' % (what, len(pairs)))
            return [a.content == b.content for a, b in pairs]
        return same
    setattr_(ops, 'buffers_equal', equal(''))
    setattr_(ops, 'bytes_equal', equal('bytes '))
    setattr_(ops, 'warp_planar', lambda x, fl: S.add('warp_planar %s %s' % (x.name, fl.name)) or T('warp%d' % S.tok(), x.shape))

    # ---- the SPyNet body under Engine.flow / Engine._flow_batch: one token when a pass starts, one per resize that ends it
    def level_input(pr, ps, flow):
        if flow is None:
            S.spynet = '%s>%s' % (pr.name, ps.name)
            S.add('spynet %s' % S.spynet)
        return T('x', (H, W, 8)), T('fup', (2, H, W))

    def level_input_batch(prs, pss, flow):
        if flow is None:
            S.spynet = '|'.join('%s>%s' % (a.name, b.name) for a, b in zip(prs, pss))
            S.add('spynet %s' % S.spynet)
        return T('x', (len(prs), H, W, 8)), T('fup', (len(prs), 2, H, W))

    def conv(cw, x, *a, **k):
        if not k.get('planar_out'):
            return x
        return T('flow32', (2, H, W) if len(x.shape) == 3 else (x.shape[0], 2, H, W))

    def resize(x, size, mode, *a, **k):
        out = T('fl%d' % S.tok(), (x.shape[0],) + tuple(size))
        S.add('flow_resize -> %s' % out.name)
        return out
    setattr_(ops, 'spynet_level_input', level_input)
    setattr_(ops, 'spynet_level_input_batch', level_input_batch)
    setattr_(ops, 'conv', conv)
    setattr_(ops, 'resize', resize)

    def conf_vis(f, conf_bw, conf_fw):
        S.add('conf_vis %s %s %s' % (fname(f), conf_bw.name, conf_fw.name))
        k = S.tok()
        return collections.OrderedDict((key, T('vis%d.%s' % (k, key), (1, H, W))) for key in ('conf_map', 'conf_map_prop'))
    setattr_(engine.Engine, '_conf_vis', staticmethod(conf_vis))


def make_engine(C=24, layout=None, pipelined=False, overlap=True, gradio=False, reset=None, weights=None, group=True, input_yuv=None):
    from refvsr_amd import engine, yuv
    e = engine.Engine.__new__(engine.Engine)
    e.input_yuv = yuv.resolve_input(input_yuv)
    e.cfg = type('Cfg', (), dict(reset_branch=reset, pipe_layout=layout, cu_split=None, scale=4,
                                 EVAL=type('Eval', (), dict(is_gradio=gradio))()))()
    e.W = weights if weights is not None else type('Wts', (), dict(chains={}, conv=Named(lambda n: CW(n, ('w', 'b'))),
                                                                  raw=Named(lambda n: (n, n + '.bias'))))()
    e.C, e.nb, e.ks, e.hd, e.vgg7, e.cache, e.overlap, e.pipelined = C, 2, 2, False, False, True, overlap, pipelined
    e.fuse_resblocks, e.rb24, e.rb48, e.rb48_max_pixels, e.rb48_multimap, e.chain_calls = True, True, True, 1 << 30, True, False
    e.fuse_conf, e.warp_up2 = group, True            # (group False: an engine without the group schedule, group_ok())
    e.spynet_batch, e.spynet_mt1_pixels, e.legacy_prep, e.bw_head_blocks = True, 0, False, 1
    e._side, e._pipe, e._layout_default, e.pipe_depth, e._inflight = None, None, None, 3, collections.deque()
    e._zero_maps, e.stream_events, e.kernel_events, e.chain_events = {}, None, None, None
    e.result_dtype, e.result_layout = 'float32', 'chw'
    e.reset_state()
    e._zeros = lambda shape, dtype, dev: T('zeros%s' % 'x'.join(str(d) for d in shape), shape, dtype)

    def pyramid(fr):
        if fr.pyr is None:
            S.add('pyramid %s' % fname(fr))
            fr.pyr = [T('pyr%d(%s)' % (lvl, fname(fr)), (3, H, W)) for lvl in range(6)]
        return fr.pyr

    def prepare_frame(fr):
        if fr.conf is None:
            S.add('prepare_frame %s' % fname(fr))
            n = fname(fr)
            fr.lr8, fr.conf, fr.idx = T('lr8(%s)' % n, (H, W, 8)), T('conf(%s)' % n, (1, H, W)), T('idx(%s)' % n, (H * W,))
            fr.aligned, fr.aligned_up = T('aligned(%s)' % n, (H, W, C)), T('aligned_up(%s)' % n, (2 * H, 2 * W, C))

    def resblocks(lr8, feat, name, stop=None):
        S.add('resblocks %s %s %s stop=%s' % (name, lr8.name, feat.name, stop))
        return T('head(%s)' % lr8.name, (H, W, e._state_cs()))

    def prop_step(fs, branch, feats, feat_ups, confs, fls, up_from_lr=False):
        k = S.tok()
        heads = [f.bw_head[1].name if f.bw_head is not None else '-' for f in fs] if fls is None and branch == 'backward_resblocks' else None
        B_ = len(fs)
        src = [m.name.split('#')[1].split('.')[0] for m in feats if '#' in m.name]
        if len(src) == B_ and (names(feats), names(feat_ups), names(confs)) == tuple(
                '[%s]' % ' '.join('%s#%s.%d' % (kind, src[0], b) for b in range(B_)) for kind in ('feat', 'up', 'conf')):
            ins = 'in=#%s' % src[0]                            # (all three carried lists are step #n's outputs, in order)
        else:
            ins = 'feats=%s ups=%s confs=%s' % (names(feats), names(feat_ups), names(confs))
        S.add('prop_step#%d %s %s %s fls=%s%s%s' % (k, branch, '[%s]' % ' '.join(fname(f) for f in fs), ins, names(fls),
                                                                       ' up_from_lr' if up_from_lr else '',
                                                                       ' heads=[%s]' % ' '.join(heads) if heads else ''))
        B, cs = len(fs), e._state_cs()
        return ([T('feat#%d.%d' % (k, b), (H, W, cs)) for b in range(B)], [T('up#%d.%d' % (k, b), (2 * H, 2 * W, cs)) for b in range(B)],
                [T('conf#%d.%d' % (k, b), (1, H, W)) for b in range(B)])

    def compute_up(bw_up, fw_up, conf_bw, conf_fw, lr_center):
        S.add('compute_up %s %s %s %s %s' % (bw_up.name, fw_up.name, conf_bw.name, conf_fw.name, lr_center.name))
        return T('out%d' % S.tok(), (3, 4 * H, 4 * W))
    e.pyramid, e.prepare_frame, e.resblocks, e._prop_step, e.compute_up = pyramid, prepare_frame, resblocks, prop_step, compute_up
    return e


def name_pipe(e):
    """Build the engine's internal streams now and name them after their roles (a stream with several roles carries them all)."""
    pipe = e._pipe_streams(DEV)
    for st in pipe:
        st.name = ''
    for role, st in zip(('M0', 'M1', 'F', 'P'), pipe):
        st.name += role
    return pipe


def window(f, dtype=torch.float32, last=None, yuv=None, ref_layout=0):
    """The window of centre frame f of a clip of frames 0 .. last (edges replicate, datasets.py:233-234) + its frame ids."""
    nums = [min(max(f + d, 0), last if last is not None else f + 1) for d in range(-(T_FRAMES // 2), T_FRAMES // 2 + 1)]
    return Window('lr', nums, dtype, yuv), Window('ref', nums, dtype, yuv, ref_layout), list(nums)


def samples(f, n, dtype=torch.float32, yuv=None):
    nums = [max(f + d, 0) for d in range(-(T_FRAMES // 2), T_FRAMES // 2 + 1)]
    return Samples('lr', nums, n, dtype, yuv), Samples('ref', nums, n, dtype, yuv), [['%d.%d' % (b, x) for x in nums] for b in range(n)]


def final_state(engines):
    out = []
    for e in engines:
        uid = {}
        for f in list(e.id_cache.values()) + list(e.prev_window):
            uid[f.uid] = fname(f)
        out.append(dict(frame_itr_num=e.frame_itr_num, id_cache=sorted(str(k) for k in e.id_cache),
                        flow_cache=sorted('%s>%s' % (uid.get(a, '?'), uid.get(b, '?')) for a, b in e.flow_cache)))
    return out


def call(label, keep=True):
    """A call of a scenario begins.  keep False: the call runs (objects keep their running numbers) but only this marker stays in the
    trace -- its form is recorded by the scenario that is about it."""
    S.log.append(('# ' if keep else '#- ') + label)


def kept(log):
    out, on = [], True
    for ln in log:
        if ln.startswith('#'):
            on = not ln.startswith('#-')
            out.append(ln)
        elif on:
            out.append(ln)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenarios
def _ready(kind):
    """input_ready of a call: None | 'materialised' | an event | a stream (of a producer)."""
    if kind == 'event':
        ev = Event()
        ev.record(Stream(name='COPY'))
        return ev
    return Stream(name='COPY') if kind == 'stream' else kind


def sc_forward_seq(overlap=True, ids=False, want_log=False, want_vis=False, gradio=False, ready=None, reset=None, calls=2, keep=None,
                   pipelined=False, dtype=torch.float32, yuv=None, cache=True, ref_layouts=None):
    """dtype: one for every call, or one per call; ref_layouts: per call, what ops.u8_layout says of the call's refs."""
    e = make_engine(overlap=overlap, gradio=gradio, reset=reset, pipelined=pipelined, input_yuv=yuv)
    e.cache = cache
    for f in range(calls):
        lrs, refs, fid = window(f, dtype[f] if isinstance(dtype, tuple) else dtype, yuv=yuv, ref_layout=ref_layouts[f] if ref_layouts else 0)
        call('forward %d' % f, keep is None or f in keep)
        e.forward(lrs, refs, f == 0, want_vis=want_vis, frame_ids=fid if ids else None, want_log=want_log, input_ready=_ready(ready))
    return [e]


def sc_forward_pipe(C=24, layout=None, gradio=False, ready=None, reset=2, want_vis=False, depth=3, prebuilt=True, calls=3, keep=(1, 2),
                    dtype=torch.float32, yuv=None):
    e = make_engine(C=C, layout=layout, pipelined=True, gradio=gradio, reset=reset, input_yuv=yuv)
    e.pipe_depth = depth
    if prebuilt:
        name_pipe(e)
    for f in range(calls):                                    # first frame, steady, a reset_branch roll-over (reset = 2), steady
        lrs, refs, fid = window(f, dtype, yuv=yuv)
        call('forward %d' % f, f in keep)
        e.forward(lrs, refs, f == 0, want_vis=want_vis, frame_ids=fid, input_ready=_ready(ready))
    return [e]


def sc_group(B=2, C=24, layout=None, first_inside=False, reset=None, want_vis=False, events=False, ready=None, pipelined=True, group=True,
             gradio=False, prior_clip=False, groups=1, dtype=torch.float32, yuv=None):
    e = make_engine(C=C, layout=layout, pipelined=pipelined, reset=reset, group=group, gradio=gradio, input_yuv=yuv)
    if pipelined:
        name_pipe(e)
    f0 = 0
    for f in range(2 if prior_clip else 0):                   # a clip before this one: the counter and the caches are not fresh
        lrs, refs, fid = window(f, yuv=yuv)
        call('prior clip: forward %d' % f, False)
        e.forward(lrs, refs, f == 0, frame_ids=fid)
    if not first_inside:
        lrs, refs, fid = window(0, dtype, yuv=yuv)
        call('forward 0', False)
        e.forward(lrs, refs, True, frame_ids=fid)
        f0 = 1
    extra = {}
    for g in range(groups):
        if events:
            e.stream_events = []
        call('forward_group %d..%d' % (f0, f0 + B - 1))
        e.forward_group([window(f, dtype, yuv=yuv) for f in range(f0, f0 + B)], is_first_frame=first_inside and g == 0, input_ready=_ready(ready),
                        want_vis=want_vis)
        if events:
            extra['stream_events.%d' % g] = [dict((k, v if k == 'n' else '%s@%s' % (v.name, v.stream)) for k, v in sorted(ev.items()))
                                             for ev in e.stream_events]
        f0 += B
    return [e], extra


def sc_multi(n=2, C=24, dtype=torch.float32, ready=None, reset=None, layout=None, prebuilt=False, calls=2, keep=(1,), yuv=None):
    lead = make_engine(C=C, pipelined=True, reset=reset, layout=layout, input_yuv=yuv)
    engines = [lead] + [make_engine(C=C, pipelined=True, reset=reset, layout=layout, weights=lead.W, input_yuv=yuv) for _ in range(n - 1)]
    if prebuilt:
        name_pipe(lead)
    for f in range(calls):                                    # the first call falls back through one forward() per sample
        lrs, refs, fids = samples(f, n, dtype, yuv)
        call('forward_multi %d' % f, f in keep)
        type(lead).forward_multi(engines, lrs, refs, f == 0, fids, input_ready=_ready(ready))
    return engines


def sc_phase(ids=True, hint=True, gradio=False, reset=None, want_vis=False, yuv=None):
    e = make_engine(gradio=gradio, reset=reset, input_yuv=yuv)
    for f in range(3):
        lrs, refs, fid = window(f, yuv=yuv)
        call('phase_a %d' % f)
        pa = e.phase_a(lrs, refs, fid if ids else None, first_hint=hint and f == 0)
        if f < 2:
            call('phase_b %d' % f)
            e.phase_b(pa, f == 0, want_vis=want_vis, after_state=lambda: S.add('after_state'))
        else:
            call('phase_b1 %d' % f)
            e.phase_b1(pa, False)
            call('phase_b2 %d' % f)
            e.phase_b2(pa, want_vis=True)
    return [e]


def sc_phase_group(B=3, streams=False, hints=True, group=True, C=24, groups=2, keep=None, yuv=None):
    e = make_engine(C=C, group=group, input_yuv=yuv)
    lane_a, lane_m, lane_b = Stream(name='A'), Stream(name='GM'), Stream(name='B1')
    f0 = 0
    for g in range(groups):
        wins = [window(f, yuv=yuv) for f in range(f0, f0 + B)]
        on = keep is None or g in keep
        call('phase_a_group %d..%d' % (f0, f0 + B - 1), on)
        with OnStream(lane_a):
            pas = e.phase_a_group(wins, [hints and f0 + b == 0 for b in range(B)] if hints else None,
                                  streams=(lane_m, [lane_b]) if streams else None)
        with OnStream(lane_b if streams else lane_a):
            for b, pa in enumerate(pas):
                if pa.get('ready') is not None:
                    lane_b.wait_event(pa['ready'])
                call('phase_b %d' % (f0 + b), on)
                e.phase_b(pa, f0 + b == 0)
        f0 += B
    return [e]


def sc_context_ahead(dtype=torch.float32, yuv=None):
    """A context prepared ahead of its window (prepare_context) is taken out of ctx_pinned by the id-keyed lookup; the decode of its
    8-bit / 4:2:0 frames runs at once (no call collects it)."""
    e = make_engine(pipelined=True, input_yuv=yuv)
    name_pipe(e)
    lrs, refs, fid = window(0, dtype, yuv=yuv)
    call('forward 0', False)
    e.forward(lrs, refs, True, frame_ids=fid)
    lrs, refs, fid = window(1, dtype, yuv=yuv)
    call('prepare_context 2')
    e.prepare_context(lrs[2], refs[2], 2)
    call('forward 1')
    e.forward(lrs, refs, False, frame_ids=fid)
    return [e]


def scenarios():
    """Every call form once in full; a variant keeps the calls that it is about (call(..., keep))."""
    sc = collections.OrderedDict()
    sc['forward seq overlap=1'] = lambda: sc_forward_seq(calls=3)
    sc['forward seq overlap=0'] = lambda: sc_forward_seq(overlap=False)
    sc['forward seq ids reset=2'] = lambda: sc_forward_seq(ids=True, reset=2, calls=3)            # (roll-over at the third call)
    sc['forward seq want_vis'] = lambda: sc_forward_seq(want_vis=True, keep=(1,))
    sc['forward seq want_log'] = lambda: sc_forward_seq(want_log=True)
    sc['forward seq want_log pipelined engine'] = lambda: sc_forward_seq(want_log=True, ids=True, pipelined=True, keep=(1,))
    sc['forward seq gradio'] = lambda: sc_forward_seq(gradio=True)
    for rd in ('materialised', 'event', 'stream'):
        sc['forward seq input_ready=%s' % rd] = lambda rd=rd: sc_forward_seq(ready=rd, keep=(1,))
    sc['forward pipelined C=24 layout=pfm'] = lambda: sc_forward_pipe(layout='pfm', calls=4, keep=(0, 1, 2, 3))
    for C, layout in ((24, 'pf_m'), (24, 'one'), (48, 'pf_m'), (48, 'pfm')):
        sc['forward pipelined C=%d layout=%s' % (C, layout)] = lambda C=C, layout=layout: sc_forward_pipe(C=C, layout=layout)
    sc['forward pipelined gradio C=24'] = lambda: sc_forward_pipe(gradio=True, calls=2, keep=(0, 1))
    sc['forward pipelined gradio C=48'] = lambda: sc_forward_pipe(C=48, gradio=True)
    sc['forward pipelined want_vis'] = lambda: sc_forward_pipe(want_vis=True, calls=2, keep=(1,))
    sc['forward pipelined depth=1'] = lambda: sc_forward_pipe(depth=1, calls=2, keep=(1,))
    for rd in ('materialised', 'event', 'stream'):
        sc['forward pipelined input_ready=%s' % rd] = lambda rd=rd: sc_forward_pipe(ready=rd, calls=2, keep=(1,))
    sc['forward_group B=2'] = lambda: sc_group(B=2, groups=2)
    sc['forward_group B=5'] = lambda: sc_group(B=5)                                   # (a steady group of four, then one forward())
    sc['forward_group B=2 C=48'] = lambda: sc_group(B=2, C=48)
    sc['forward_group B=2 layout=pf_m'] = lambda: sc_group(B=2, layout='pf_m')
    sc['forward_group roll-over inside B=3 reset=2'] = lambda: sc_group(B=3, reset=2)
    sc['forward_group first and roll-over inside B=4 reset=3 after a clip'] = lambda: sc_group(B=4, reset=3, first_inside=True, prior_clip=True)
    sc['forward_group want_vis'] = lambda: sc_group(B=2, want_vis=True)
    sc['forward_group stream_events'] = lambda: sc_group(B=2, events=True)
    sc['forward_group stream_events first inside'] = lambda: sc_group(B=2, events=True, first_inside=True)
    sc['forward_group uint8'] = lambda: sc_group(B=2, dtype=torch.uint8)
    sc['forward_group input_ready=stream'] = lambda: sc_group(B=2, ready='stream')
    sc['forward_group no group schedule'] = lambda: sc_group(B=2, group=False)
    sc['forward_group gradio'] = lambda: sc_group(B=2, gradio=True)
    sc['forward_multi n=2'] = lambda: sc_multi(calls=3, keep=(0, 1, 2))              # (the first call: one forward() per sample)
    sc['forward_multi n=3 C=48'] = lambda: sc_multi(n=3, C=48)
    sc['forward_multi n=2 uint8'] = lambda: sc_multi(dtype=torch.uint8)
    sc['forward_multi n=2 reset=2'] = lambda: sc_multi(reset=2, calls=3, keep=(2,))  # (a roll-over: one forward() per sample)
    sc['forward_multi input_ready=event'] = lambda: sc_multi(ready='event')
    for ids, hint in ((True, True), (True, False), (False, True)):
        sc['phase_a ids=%d first_hint=%d' % (ids, hint)] = lambda ids=ids, hint=hint: sc_phase(ids=ids, hint=hint)
    sc['phase_a gradio'] = lambda: sc_phase(gradio=True)
    sc['phase_a reset=2 want_vis'] = lambda: sc_phase(reset=2, want_vis=True)
    for B in (1, 3):
        sc['phase_a_group B=%d' % B] = lambda B=B: sc_phase_group(B=B)
        sc['phase_a_group B=%d streams' % B] = lambda B=B: sc_phase_group(B=B, streams=True)
    sc['phase_a_group B=3 no hints'] = lambda: sc_phase_group(B=3, hints=False, groups=1)
    sc['phase_a_group B=2 streams C=48'] = lambda: sc_phase_group(B=2, streams=True, C=48, keep=(1,))
    sc['phase_a_group B=2 streams no group schedule'] = lambda: sc_phase_group(B=2, streams=True, group=False, groups=1)
    sc['contexts prepared ahead'] = sc_context_ahead
    # ---- the input kinds (float above): the content compare against the contexts' source copies, the decode of a call's new frames
    #      in one launch, the repeated edge frame of the first window
    sc['forward seq uint8'] = lambda: sc_forward_seq(calls=3, dtype=torch.uint8)
    sc['forward seq yuv nv12'] = lambda: sc_forward_seq(calls=3, yuv='nv12', keep=(0, 1))
    sc['forward seq float then uint8'] = lambda: sc_forward_seq(calls=3, dtype=(torch.float32, torch.uint8, torch.uint8), keep=(1,))
    sc['forward seq uint8 ref layout changes'] = lambda: sc_forward_seq(calls=3, dtype=torch.uint8, ref_layouts=(0, 1, 1), keep=(1,))
    sc['forward seq uint8 cache off'] = lambda: sc_forward_seq(dtype=torch.uint8, cache=False, keep=(0,))
    sc['forward pipelined yuv nv12'] = lambda: sc_forward_pipe(yuv='nv12', calls=2, keep=(1,))
    sc['forward_group yuv nv12 B=2'] = lambda: sc_group(B=2, yuv='nv12')
    sc['forward_multi n=2 yuv p010'] = lambda: sc_multi(yuv='p010')
    for ids in (1, 0):
        sc['phase_a yuv ids=%d' % ids] = lambda ids=ids: sc_phase(ids=bool(ids), yuv='nv12')
    sc['phase_a_group B=3 yuv'] = lambda: sc_phase_group(B=3, yuv='nv12', groups=1)
    sc['contexts prepared ahead uint8'] = lambda: sc_context_ahead(dtype=torch.uint8)
    sc['contexts prepared ahead yuv'] = lambda: sc_context_ahead(yuv='nv12')
    return sc


def record(setattr_):
    """{scenario: {'trace': [lines], 'final': [per engine: frame_itr_num, id_cache keys, flow_cache pairs], ...}}"""
    global S
    S = State()
    patch_all(setattr_)
    out = collections.OrderedDict()
    for name, run in scenarios().items():
        S = State()
        res = run()
        engines, extra = res if isinstance(res, tuple) else (res, {})
        out[name] = dict(trace=kept(S.log), final=final_state(engines), **extra)
    return out


def load(path):
    with open(path) as fh:
        return json.load(fh, object_pairs_hook=collections.OrderedDict)


def main(argv):
    sys.path.insert(0, ROOT)
    undo = []

    def setattr_(obj, name, value):
        undo.append((obj, name, obj.__dict__[name] if isinstance(obj, type) else getattr(obj, name)))
        setattr(obj, name, value)
    try:
        rec = record(setattr_)
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
    with open(argv[1], 'w') as fh:                              # one trace line per line of the file, everything else of a scenario on one
        fh.write('{\n' + ',\n'.join('%s: {"trace": [\n%s],\n%s}' % (
            json.dumps(name), ',\n'.join(json.dumps(ln) for ln in sc['trace']),
            ', '.join('%s: %s' % (json.dumps(k), json.dumps(v)) for k, v in sc.items() if k != 'trace')) for name, sc in rec.items()) + '\n}\n')
    print('%d scenarios, %d trace lines -> %s' % (len(rec), sum(len(v['trace']) for v in rec.values()), argv[1]))


if __name__ == '__main__':
    main(sys.argv)
