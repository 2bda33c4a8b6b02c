"""Every public entry of refvsr_amd.model.Network on the CPU (tests/test_network_entries.py): what the entry check makes of each kind of
input, what the engine is handed, and the dict that comes back -- or the refusal, type and full message.

A real Network(config) is built on the CPU and driven through its public methods only, so the same file records the entries from one tree
and checks another.  Its engine class is a recording stub (StubEngine: small named CPU tensors), `_weights` returns a token, hip.lib,
ops.stack_results and ops.result_to_yuv420 are fakes that log; device inputs are CPU tensors of a subclass whose is_cuda is True (the
entry check asks nothing else of a device).  n = 2, t = 3, h = 4, w = 6.

Recording (from the repository root, with the model.py to be pinned in the tree):
    python tests/network_entry_trace.py tests/golden/network_entries.json
"""
import collections
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T_FRAMES, H, W, SCALE = 2, 3, 4, 6, 4


class Cuda(torch.Tensor):                         # (the checks ask is_cuda; nothing here touches a device)
    is_cuda = True


def _storage(t):
    return t.untyped_storage().data_ptr()


def _what(t):
    return ('%s%s/%s' % (str(t.dtype).split('.')[1], list(t.shape), list(t.stride()))).replace(' ', '')


# ---------------------------------------------------------------------------------------------------------------- the stub engine
class Rec(object):
    """What one entry call leaves behind: the engine calls, the fakes' launches, the storages of the caller's inputs and the engine's results."""

    def __init__(self):
        self.log, self.inputs, self.results = [], {}, {}

    def arg(self, t):
        """A tensor the engine was handed: what it is, and whether it is (a view of) the caller's own tensor or a converted copy."""
        return '%s %s' % (_what(t), self.inputs.get(_storage(t), 'copy'))

    def result(self, name, shape):
        t = torch.zeros(shape)
        self.results[_storage(t)] = name
        return t


R = None                # the current entry's Rec


def _ids(ids):
    return '-' if ids is None else json.dumps(ids)


def _ready(r):
    return '-' if r is None else str(r)


class StubEngine(object):
    """What Network uses of an Engine.  Class attributes set per scenario: group_ok_, vis_keys (None: a network without 'eval_vis')."""
    group_ok_, vis_keys = True, ('conf_map', 'conf_map_prop')
    made = 0

    def __init__(self, config, W_):
        self.b = StubEngine.made
        StubEngine.made += 1
        R.log.append('Engine(%s) #%d' % (W_, self.b))
        self.result_layout = getattr(config, 'result_layout', None) or 'chw'
        self.result_yuv = ('nv12', 'bt709', 'limited') if getattr(config, 'result_yuv', None) else None
        self.frame_itr_num = 0

    def _res(self, tag):
        return R.result('res%d%s' % (self.b, tag), (3, SCALE * H, SCALE * W))

    def _vis(self, tag, want):
        if not want or self.vis_keys is None:
            return None
        return collections.OrderedDict((k, R.result('%s%d%s' % (k, self.b, tag), (1, H, W))) for k in self.vis_keys)

    def takes_pipelined_path(self, frame_ids, want_log=False):
        return frame_ids is not None and not want_log

    def group_ok(self):
        return self.group_ok_

    def set_pipelined(self, on=True):
        R.log.append('#%d.set_pipelined(%s)' % (self.b, on))

    def reset_state(self):
        R.log.append('#%d.reset_state()' % self.b)

    def drain(self):
        R.log.append('#%d.drain()' % self.b)

    def forward(self, lrs, refs, is_first_frame, want_vis=False, frame_ids=None, want_log=False, input_ready=None):
        R.log.append('#%d.forward(%s | %s, first=%r, want_vis=%r, ids=%s, want_log=%r, ready=%s)' % (
            self.b, R.arg(lrs), R.arg(refs), is_first_frame, want_vis, _ids(frame_ids), want_log, _ready(input_ready)))
        vis = self._vis('', want_vis)
        if want_log:
            vis = (vis, collections.OrderedDict((k, R.result('%s%d' % (k, self.b), (1, H, W))) for k in ('dbg_a', 'dbg_b')))
        return self._res(''), vis

    @staticmethod
    def forward_multi(engines, lrs, refs, is_first_frame, frame_ids, input_ready=None):
        R.log.append('forward_multi(#%s, %s | %s, first=%r, ids=%s, ready=%s)' % (
            ','.join(str(e.b) for e in engines), R.arg(lrs), R.arg(refs), is_first_frame, _ids(frame_ids), _ready(input_ready)))
        return [e._res('') for e in engines]

    def forward_group(self, wins, is_first_frame=False, input_ready=None, want_vis=False):
        R.log.append('#%d.forward_group([%s], first=%r, ready=%s, want_vis=%r)' % (
            self.b, '; '.join('%s | %s ids=%s' % (R.arg(lr), R.arg(rf), _ids(ids)) for lr, rf, ids in wins), is_first_frame, _ready(input_ready), want_vis))
        res = [self._res('.%d' % b) for b in range(len(wins))]
        return (res, [self._vis('.%d' % b, True) for b in range(len(wins))]) if want_vis else res

    def phase_a(self, lrs, refs, frame_ids=None, first_hint=False):
        R.log.append('#%d.phase_a(%s | %s, ids=%s, first_hint=%r)' % (self.b, R.arg(lrs), R.arg(refs), _ids(frame_ids), first_hint))
        return 'handle%d' % self.b

    def phase_a_group(self, wins, first_hints=None, streams=None):
        R.log.append('#%d.phase_a_group([%s], first_hints=%r, streams=%r)' % (
            self.b, '; '.join('%s | %s ids=%s' % (R.arg(lr), R.arg(rf), _ids(ids)) for lr, rf, ids in wins), first_hints, streams))
        return ['handle%d.%d' % (self.b, b) for b in range(len(wins))]

    def phase_b(self, handle, is_first_frame, want_vis=False, after_state=None):
        R.log.append('#%d.phase_b(%s, first=%r, want_vis=%r, after_state=%s)' % (self.b, handle, is_first_frame, want_vis, _ready(after_state)))
        return self._res(''), self._vis('', want_vis)

    def phase_b1(self, handle, is_first_frame):
        R.log.append('#%d.phase_b1(%s, first=%r)' % (self.b, handle, is_first_frame))

    def phase_b2(self, handle, want_vis=False):
        R.log.append('#%d.phase_b2(%s, want_vis=%r)' % (self.b, handle, want_vis))
        return self._res(''), self._vis('', want_vis)


def patch_all(setattr_):
    """Install the fakes (setattr_(obj, name, value): monkeypatch.setattr or the recorder's own)."""
    from refvsr_amd import hip, model, ops

    def stack_results(frames, layout=None):
        R.log.append('stack_results(%d, %s)' % (len(frames), layout))
        return torch.stack(list(frames), 0)

    def result_to_yuv420(frames, *params):
        frames = list(frames)
        R.log.append('result_to_yuv420(%s, %s)' % (' '.join(R.results.get(_storage(f), '?') for f in frames), ' '.join(params)))
        return torch.zeros((len(frames), 3 * SCALE * H // 2, SCALE * W), dtype=torch.uint8)
    setattr_(hip, 'lib', lambda: R.log.append('hip.lib()'))
    setattr_(ops, 'stack_results', stack_results)
    setattr_(ops, 'result_to_yuv420', result_to_yuv420)
    setattr_(model.Network, '_engine_cls', StubEngine)
    setattr_(model.Network, '_weights', lambda self, device, call=None: R.log.append('_weights(%s, call=%r)' % (device, call)) or 'W')


# ---------------------------------------------------------------------------------------------------------------- inputs and entries
def inputs():
    """name -> (config.input_yuv, lrs, refs), [n, t, ..]: every kind of tensor the entry check tells apart."""
    g = torch.Generator().manual_seed(0)
    cuda = lambda x: x.as_subclass(Cuda)
    f32 = torch.rand((N, T_FRAMES, 3, H, W), generator=g)
    u8 = torch.randint(0, 256, (N, T_FRAMES, 3, H, W), generator=g, dtype=torch.uint8)
    hwc = torch.randint(0, 256, (N, T_FRAMES, H, W, 3), generator=g, dtype=torch.uint8).permute(0, 1, 4, 2, 3)
    nv12 = torch.randint(0, 256, (N, T_FRAMES, 3 * H // 2, W), generator=g, dtype=torch.uint8)
    p010 = torch.zeros((N, T_FRAMES, 3 * H // 2, W), dtype=torch.uint16)
    tab = collections.OrderedDict()
    tab['float32'] = (None, cuda(f32), cuda(f32.clone()))
    tab['float16'] = (None, cuda(f32.half()), cuda(f32.half()))
    tab['float64'] = (None, cuda(f32.double()), cuda(f32.double()))
    tab['float32 strided'] = (None, cuda(torch.rand((N, T_FRAMES, 3, H, 2 * W), generator=g)[..., ::2]), cuda(f32.clone()))
    tab['uint8 planar'] = (None, cuda(u8), cuda(u8.clone()))
    tab['uint8 channels-last'] = (None, cuda(hwc), cuda(hwc.clone()))
    tab['uint8 other strides'] = (None, cuda(u8), cuda(u8.transpose(-1, -2).contiguous().transpose(-1, -2)))
    tab['uint8 + float32'] = (None, cuda(u8), cuda(f32))
    tab['nv12'] = ('nv12', cuda(nv12), cuda(nv12.clone()))
    tab['p010'] = ('p010', cuda(p010), cuda(p010.clone()))
    tab['nv12 strided'] = ('nv12', cuda(nv12), cuda(torch.zeros((N, T_FRAMES, 3 * H // 2, 2 * W), dtype=torch.uint8)[..., ::2]))
    tab['nv12 two shapes'] = ('nv12', cuda(nv12), cuda(torch.zeros((N, T_FRAMES, 3 * H // 2 + 3, W), dtype=torch.uint8)))
    tab['rgb uint8 under input_yuv'] = ('nv12', cuda(u8), cuda(u8))
    tab['4:2:0 shape without input_yuv'] = (None, cuda(nv12), cuda(nv12))
    tab['host float32'] = (None, f32, f32)
    return tab


IDS = [10, 11, 12]
GROUP_IDS = [[10, 11, 12], [11, 12, 13]]


def entries():
    """name -> (n, run(net, lrs, refs, ready), config fields, StubEngine fields): every public entry that takes frames."""
    en = collections.OrderedDict()

    def add(name, n, run, cfg=None, eng=None):
        en[name] = (n, run, cfg or {}, eng or {})
    for n in (1, 2):
        add('forward n=%d' % n, n, lambda net, lr, rf, rd: net.forward(lr, rf, True, input_ready=rd))
        add('forward n=%d ids' % n, n, lambda net, lr, rf, rd: net.forward(lr, rf, False, frame_ids=IDS, input_ready=rd))     # (n = 2: forward_multi)
    add('forward n=2 ids no group schedule', 2, lambda net, lr, rf, rd: net.forward(lr, rf, False, frame_ids=IDS, input_ready=rd), eng=dict(group_ok_=False))
    add('forward n=1 is_log', 1, lambda net, lr, rf, rd: net.forward(lr, rf, False, is_log=True, frame_ids=IDS, input_ready=rd))
    for n in (1, 2):
        add('forward n=%d is_log save_sample' % n, n, lambda net, lr, rf, rd: net.forward(lr, rf, True, is_log=True, input_ready=rd), cfg=dict(save_sample=True))
    add('forward n=1 is_log save_sample no eval_vis', 1, lambda net, lr, rf, rd: net.forward(lr, rf, True, is_log=True, input_ready=rd),
        cfg=dict(save_sample=True), eng=dict(vis_keys=None))
    add('forward_group', 2, lambda net, lr, rf, rd: net.forward_group(lr, rf, GROUP_IDS, input_ready=rd))
    add('forward_group want_conf', 2, lambda net, lr, rf, rd: net.forward_group(lr, rf, GROUP_IDS, is_first_frame=True, input_ready=rd, want_conf=True))
    add('forward_group want_conf no eval_vis', 2, lambda net, lr, rf, rd: net.forward_group(lr, rf, GROUP_IDS, input_ready=rd, want_conf=True),
        eng=dict(vis_keys=None))
    add('phase_a n=2 ids', 2, lambda net, lr, rf, rd: net.phase_a(lr, rf, frame_ids=IDS, first_hint=True))
    add('phase_a n=1', 1, lambda net, lr, rf, rd: net.phase_a(lr, rf))
    add('phase_a_group', 2, lambda net, lr, rf, rd: net.phase_a_group(lr, rf, GROUP_IDS, first_hints=[True, False]))
    add('phase_a_group of lists', 2, lambda net, lr, rf, rd: net.phase_a_group(list(lr), list(rf), GROUP_IDS))
    return en


def tails():
    """name -> (n, run(net, handles), config fields, StubEngine fields): the entries that take phase_a's handles."""
    tl = collections.OrderedDict()
    for n in (1, 2):
        for is_log, save in ((False, False), (True, False), (True, True)):
            tag = 'n=%d is_log=%d save_sample=%d' % (n, is_log, save)
            tl['phase_b ' + tag] = (n, lambda net, hs, is_log=is_log: net.phase_b(hs, True, is_log=is_log, after_state='after'), dict(save_sample=save), {})
            tl['phase_b1 phase_b2 ' + tag] = (n, lambda net, hs, is_log=is_log: net.phase_b2(net.phase_b1(hs, False), is_log=is_log), dict(save_sample=save), {})
    return tl


def describe(x):
    """The returned value: a dict keeps its keys in order, a tensor is its shape, dtype and -- where it shares the storage of a tensor the
    engine returned -- 'view of <that result>' (n = 1: 'result' is an unsqueeze, not a copy)."""
    if isinstance(x, torch.Tensor):
        name = R.results.get(_storage(x))
        return '%s%s' % (_what(x).split('/')[0], '' if name is None else ' view of ' + name)
    if isinstance(x, dict):
        return [type(x).__name__] + [[k, describe(v)] for k, v in x.items()]
    if isinstance(x, (list, tuple)):
        return [type(x).__name__] + [describe(v) for v in x]
    return repr(x)


def run_entry(net, run, cfg, eng, input_yuv, result_yuv, args):
    """One call on fresh engines -> {'log': [...], 'out': ...} or {'log': [...], 'raised': 'Type: message'}."""
    global R
    R = Rec()
    StubEngine.made = 0
    StubEngine.group_ok_, StubEngine.vis_keys = eng.get('group_ok_', True), eng.get('vis_keys', ('conf_map', 'conf_map_prop'))
    net._engines = []
    net.config.input_yuv, net.config.result_yuv, net.config.save_sample = input_yuv, result_yuv, cfg.get('save_sample', False)
    try:
        out = run(net, *args)
    except (RuntimeError, AssertionError, ValueError, TypeError, NotImplementedError) as e:
        return collections.OrderedDict(log=R.log, raised='%s: %s' % (type(e).__name__, e))
    return collections.OrderedDict(log=R.log, out=describe(out))


def record(setattr_):
    """{'<entry> | <input> | ready=.. | result_yuv=..': what run_entry keeps} + the tails and the calls that take no frames."""
    global R
    from refvsr_amd import get_config
    from refvsr_amd.model import Network
    patch_all(setattr_)
    R = Rec()
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    net = Network(cfg)
    out = collections.OrderedDict()
    for ename, (n, run, cf, eng) in entries().items():
        for iname, (fmt, lrs, refs) in inputs().items():
            for ready in (None, 'ready'):
                for ryuv in (None, 'nv12'):
                    lr, rf = lrs[:n], refs[:n]
                    key = '%s | %s | ready=%s | result_yuv=%s' % (ename, iname, _ready(ready), _ready(ryuv))

                    def go(net_, rd, run=run, lr=lr, rf=rf):
                        R.inputs.update({_storage(lr): 'own', _storage(rf): 'own'})
                        return run(net_, lr, rf, rd)
                    out[key] = run_entry(net, go, cf, eng, fmt, ryuv, (ready,))
    for tname, (n, run, cf, eng) in tails().items():
        for ryuv in (None, 'nv12'):
            def go(net_, n=n, run=run):
                net_.ensure_engines(n, 'dev')
                return run(net_, ['handle%d' % b for b in range(n)])
            out['%s | result_yuv=%s' % (tname, _ready(ryuv))] = run_entry(net, go, cf, eng, None, ryuv, ())

    def other(net_):
        net_.ensure_engines(2, 'dev')
        net_.set_pipelined(True)
        net_.reset()
        with_train = None
        try:
            net_.forward(None, None, True, is_train=True)
        except NotImplementedError as e:
            with_train = '%s: %s' % (type(e).__name__, e)
        return [net_.frame_itr_num, net_.config.pipelined, with_train]
    out['set_pipelined reset is_train'] = run_entry(net, other, {}, {}, None, None, ())
    return out


# ---------------------------------------------------------------------------------------------------------------- the golden file
# The recording repeats itself (a refusal reads the same whatever input_ready and result_yuv are), so the file keeps every distinct log
# line, result and log once and a call as two numbers: {'lines': [..], 'results': [{'out': ..} | {'raised': ..}], 'logs': [[line, ..]],
# 'calls': {'<entry>': {'<input>': [[log, result] per (input_ready, result_yuv) in the order of VARIANTS]}, '<tail>': {'': [.. per
# result_yuv]}, '<other>': {'': [[log, result]]}}}.  The input_ready a line ends with is the call's own: kept as 'ready=@'.
VARIANTS = [' | ready=%s | result_yuv=%s' % (_ready(r), _ready(y)) for r in (None, 'ready') for y in (None, 'nv12')]
TAIL_VARIANTS = [' | result_yuv=%s' % _ready(y) for y in (None, 'nv12')]


def _variants(n):
    return {4: VARIANTS, 2: TAIL_VARIANTS, 1: ['']}[n]


def _own_ready(key):
    return 'ready=%s' % key.split(' | ready=')[1].split(' | ')[0] if ' | ready=' in key else None


def encode(rec):
    tabs = dict(lines=[], results=[], logs=[])

    def idx(name, x):
        if x not in tabs[name]:
            tabs[name].append(x)
        return tabs[name].index(x)
    calls = collections.OrderedDict()
    for key, v in rec.items():
        rd = _own_ready(key)
        log = [idx('lines', ln.replace(rd, 'ready=@') if rd else ln) for ln in v['log']]
        entry, _, iname = key.split(' | ready=')[0].split(' | result_yuv=')[0].partition(' | ')
        calls.setdefault(entry, collections.OrderedDict()).setdefault(iname, []).append(
            [idx('logs', log), idx('results', dict((k, x) for k, x in v.items() if k != 'log'))])
    return collections.OrderedDict(lines=tabs['lines'], results=tabs['results'], logs=tabs['logs'], calls=calls)


def decode(g):
    """The flat {call: {'log': [..], 'out': .. | 'raised': ..}} that record() returns, from the file's tables."""
    out = collections.OrderedDict()
    for group, cs in ((e + (' | ' + i if i else ''), cs) for e, by_input in g['calls'].items() for i, cs in by_input.items()):
        for var, (lg, res) in zip(_variants(len(cs)), cs):
            rd = _own_ready(group + var)
            log = [g['lines'][i].replace('ready=@', rd) if rd else g['lines'][i] for i in g['logs'][lg]]
            out[group + var] = collections.OrderedDict([('log', log)] + list(g['results'][res].items()))
    return out


def load(path):
    """(what the file was recorded from, the flat recording)."""
    with open(path) as fh:
        g = json.load(fh, object_pairs_hook=collections.OrderedDict)
    return g['_recorded_from'], decode(g)


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
    commit = argv[2] if len(argv) > 2 else subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT).decode().strip()
    enc = encode(rec)
    assert decode(enc) == rec
    js = lambda x: json.dumps(x, separators=(',', ':'))
    rows = lambda xs, n: ',\n'.join(','.join(js(x) for x in xs[i:i + n]) for i in range(0, len(xs), n))
    with open(argv[1], 'w') as fh:                              # a line per distinct log line, result, 16 logs, and entry x input
        fh.write('{"_recorded_from": %s,\n"lines": [\n%s],\n"results": [\n%s],\n"logs": [\n%s],\n"calls": {\n%s}\n}\n' % (
            json.dumps(dict(commit=commit, file='refvsr_amd/model.py')), rows(enc['lines'], 1), rows(enc['results'], 1), rows(enc['logs'], 16),
            ',\n'.join('%s:%s' % (json.dumps(k), js(v)) for k, v in enc['calls'].items())))
    print('%d entry calls recorded from %s -> %s' % (len(rec), commit[:12], argv[1]))


if __name__ == '__main__':
    main(sys.argv)
