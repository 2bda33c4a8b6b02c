"""Event traces of run_wavefront / run_sharded with executors that do no network arithmetic (tests/test_shard_trace.py).

Only the public surface of refvsr_amd.shard is used, so the same file records the traces from one tree and checks another.
An executor's carried state is four tiny float32 tensors + frame_itr_num; every forward-branch step updates them by an exact
integer recurrence from (frame, is_first_frame), and the result of a frame is the state after its step: a dropped or misplaced
hand-off or `first` flag changes results.  Every call into the executor, every window fetched and every message is logged in order
with the active lane, as one short token:  <lane><event><args>, lane '-' (none) | a | b | c | m (the receive-posting lane).

Recording (from the repository root):  python tests/shard_trace.py tests/golden/shard_traces.json tests/golden/shard_model.json
"""
import itertools
import json
import os
import queue
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_NUM = 3
MOD = 65521.0
KEYS = ('feat', 'flow', 'feat_up', 'conf')                 # shard.STATE_KEYS; flow has two channels
SHAPES = {'feat': (1, 1, 1), 'flow': (2, 1, 1), 'feat_up': (1, 1, 1), 'conf': (1, 1, 1)}


def step_values(vals, itr, f, first, reset):
    """One forward-branch step on the five state values: v <- (31 v + f + 1 + j) mod 65521, exact in float32; the values restart
    from zero when `first` and whenever the executor's own call counter reaches a multiple of reset (RefVSR.py:168-170)."""
    if first:
        itr = 0
    if itr == 0 or (reset and itr % reset == 0):
        vals = [0.0] * 5
    return [float((31.0 * v + f + 1 + j) % MOD) for j, v in enumerate(vals)], itr + 1


def sequential(nframes, reset):
    out, vals, itr = {}, [0.0] * 5, 0
    for f in range(nframes):
        vals, itr = step_values(vals, itr, f, f == 0, reset)
        out[f] = list(vals)
    return out


class _Lane(object):
    def __init__(self, ex, name):
        self.ex, self.name = ex, name

    def __enter__(self):
        self.prev, self.ex.lane = self.ex.lane, self.name

    def __exit__(self, *exc):
        self.ex.lane = self.prev
        return False


class Exec(object):
    """No lanes, dict state, phase_a + phase_b1 / phase_b2 + __call__ (run_sharded)."""

    def __init__(self, log, reset, nframes):
        self.log_, self.reset, self.nframes, self.lane = log, reset, nframes, '-'
        self.vals, self.itr = [0.0] * 5, 0

    def ev(self, name, *args):
        self.log_.append(self.lane + name + ','.join(str(a) for a in args))

    def _step(self, f, first):
        self.vals, self.itr = step_values(self.vals, self.itr, f, first, self.reset)
        return torch.tensor(self.vals, dtype=torch.float32)

    def _tensors(self):
        v = self.vals
        return {'feat': [v[0]], 'flow': [v[1], v[2]], 'feat_up': [v[3]], 'conf': [v[4]]}

    def __call__(self, lrs, refs, first):
        f = int(lrs[FRAME_NUM // 2])                        # a window is its frame indices (get_window below): the centre is f
        self.ev('call', f, int(first))
        return self._step(f, first)

    def phase_a(self, lrs, refs, f, hint):
        assert int(lrs[FRAME_NUM // 2]) == f
        self.ev('pa', f, int(hint))
        return {'_frame': f}

    def phase_b1(self, h, first):
        self.ev('b1', h['_frame'], int(first))
        h['out'] = self._step(h['_frame'], first)
        return h

    def phase_b2(self, h):
        self.ev('b2', h['_frame'])
        return h['out']

    def export_state(self):
        self.ev('exp')
        st = {k: torch.tensor(v, dtype=torch.float32).view(SHAPES[k]) for k, v in self._tensors().items()}
        st['frame_itr_num'] = self.itr
        return st

    def import_state(self, st):
        self.ev('imp')
        for k in KEYS:
            assert tuple(st[k].shape) == SHAPES[k] and st[k].dtype == torch.float32
        self.vals = [float(st['feat'][0]), float(st['flow'][0]), float(st['flow'][1]), float(st['feat_up'][0]), float(st['conf'][0])]
        self.itr = int(st['frame_itr_num'])


class ExecPacked(Exec):
    """+ the packed single-message state (run_sharded and run_wavefront)."""

    def state_nbytes(self):
        return 24

    def export_state_packed(self):
        self.ev('expp')
        return torch.tensor([float(self.itr)] + self.vals, dtype=torch.float32).view(torch.uint8)

    def import_state_packed(self, buf):
        self.ev('impp')
        v = buf.view(torch.float32).tolist()
        self.itr, self.vals = int(v[0]), v[1:]


class ExecB(Exec):
    """phase_b only (no B1 / B2 split)."""
    phase_b1 = property(lambda self: (_ for _ in ()).throw(AttributeError('phase_b1')))
    phase_b2 = property(lambda self: (_ for _ in ()).throw(AttributeError('phase_b2')))

    def phase_b(self, h, first, after_state=None):
        self.ev('b', h['_frame'], int(first), int(after_state is not None))
        out = self._step(h['_frame'], first)
        if after_state is not None:
            after_state()
        return out


class ExecBAfter(ExecB):
    supports_after_state = True


class ExecLanes(Exec):
    """Lanes a and b with marks, dict state, phase_a_group."""

    def lane_a(self):
        return _Lane(self, 'a')

    def lane_b(self):
        return _Lane(self, 'b')

    def mark(self, what, f):
        self.ev('mk', what, f)

    def wait(self, what, f):
        self.ev('wt', what, f)

    def begin_run(self):
        self.ev('begin')

    def sync(self):
        self.ev('sync')

    def phase_a_group(self, windows, fs, hints):
        assert [int(w_[0][FRAME_NUM // 2]) for w_ in windows] == list(fs)
        self.ev('pg', '.'.join(str(f) for f in fs), '.'.join(str(int(h)) for h in hints))
        return [{'_frame': f} for f in fs]


class ExecLanesPacked(ExecPacked, ExecLanes):
    """Lanes a, b and c, packed state, no phase_a_group."""
    phase_a_group = property(lambda self: (_ for _ in ()).throw(AttributeError('phase_a_group')))

    def lane_c(self):
        return _Lane(self, 'c')


class ExecLanesLate(ExecLanesPacked):
    early_chain = False


class ExecSplit(ExecLanesPacked):
    """+ the two-message hand-off: [counter | feat | flow | conf] first, feat_up second, awaited inside the receiver's step."""
    split_handoff = True
    _pending = None

    def state_split_nbytes(self):
        return 20, 4

    def export_state_split(self):
        self.ev('exps')
        v = self.vals
        return (torch.tensor([float(self.itr), v[0], v[1], v[2], v[4]], dtype=torch.float32).view(torch.uint8),
                torch.tensor([v[3]], dtype=torch.float32).view(torch.uint8))

    def state_tail_buffer(self, device):
        self.ev('tailbuf')
        return torch.empty(4, dtype=torch.uint8)

    def import_state_split(self, head, tail, wait_tail):
        self.ev('imps')
        self._pending = (head.view(torch.float32).tolist(), tail, wait_tail)

    def phase_b1(self, h, first):
        if self._pending is not None:
            v, tail, wait_tail = self._pending
            self._pending = None
            self.ev('tailwait')
            wait_tail()
            self.itr, self.vals = int(v[0]), [v[1], v[2], v[3], float(tail.view(torch.float32)[0]), v[4]]
        return ExecLanesPacked.phase_b1(self, h, first)


class ExecCtx(ExecLanes):
    """+ lane c, the receive-posting lane and the context hooks of run_wavefront(exchange_contexts=True).  A context is two floats
    made from its frame index; phase A must find every context its window needs."""

    def __init__(self, log, reset, nframes):
        ExecLanes.__init__(self, log, reset, nframes)
        self.ctx, self.strict = {}, False

    def lane_c(self):
        return _Lane(self, 'c')

    def comm_lane(self):
        return _Lane(self, 'm')

    def strict_contexts(self, on):
        self.ev('strict', int(on))
        self.strict = bool(on)

    def prepare_context(self, f, lr, ref):
        assert int(lr) == f and int(ref) == f + 100 and f not in self.ctx
        self.ev('prep', f)
        self.ctx[f] = (float(f), float(7 * f + 3))

    def context_nbytes(self):
        self.ev('cnb')
        return 8

    def export_context(self, f):
        self.ev('expc', f)
        return torch.tensor(self.ctx[f], dtype=torch.float32).view(torch.uint8)

    def import_context(self, f, lr, ref, buf):
        assert int(lr) == f and f not in self.ctx
        self.ev('impc', f)
        self.ctx[f] = tuple(buf.view(torch.float32).tolist())
        assert self.ctx[f] == (float(f), float(7 * f + 3))

    def _check(self, f, hint):
        from refvsr_amd import shard
        ids = shard.window_ids(f, self.nframes, FRAME_NUM)
        assert not self.strict or all(i in self.ctx for i in ids[0 if hint else FRAME_NUM // 2:]), 'window %d lacks a context' % f

    def phase_a(self, lrs, refs, f, hint):
        self._check(f, hint)
        return ExecLanes.phase_a(self, lrs, refs, f, hint)

    def phase_a_group(self, windows, fs, hints):
        for f, h in zip(fs, hints):
            self._check(f, h)
        return ExecLanes.phase_a_group(self, windows, fs, hints)


# kind -> (executor class, exchange_contexts, group sizes)
KINDS = (('b12', Exec, False, (1,)), ('b', ExecB, False, (1,)), ('bafter', ExecBAfter, False, (1,)),
         ('lanes', ExecLanes, False, (1, 2, 3)), ('packed', ExecLanesPacked, False, (1,)), ('split', ExecSplit, False, (1,)),
         ('late', ExecLanesLate, False, (1,)), ('ctx', ExecCtx, True, (1, 2, 3)))
FAMILIES = ('balanced', 'hybrid', 'chain', 'cyclic1', 'cyclic2', 'growing')


def family_parts(shard, fam, nframes, world, reset):
    """The partition of a family, or None where the family does not apply (hybrid needs reset_branch)."""
    if fam == 'balanced':
        return shard.partition(nframes, world)
    if fam == 'hybrid':
        return shard.partition_hybrid(nframes, world, reset) if reset else None
    if fam == 'chain':
        return shard.partition_chain(nframes, world)
    if fam.startswith('cyclic'):
        return shard.partition_cyclic(nframes, world, int(fam[6:]))
    return shard.partition_cyclic_growing(nframes, world, 5.3, 1.0, 7.2)


def cases(world):
    """[(case id, spec)] of one world size, in the order the workers run them."""
    out = []
    for nframes, reset in itertools.product((5, 7), (None, 3)):
        tag = 'w%d/n%d/r%s' % (world, nframes, reset or 0)
        for aligned in () if world == 1 else ((False, True) if reset else (False,)):       # run_sharded needs a process group
            for kind in ('call', 'callpacked'):
                out.append(('%s/sharded%d/%s' % (tag, aligned, kind), dict(run='sharded', nframes=nframes, reset=reset, aligned=aligned, kind=kind)))
        for fam in FAMILIES:
            if fam == 'hybrid' and not reset:
                continue
            for kind, _, exchange, groups in KINDS:
                if exchange and world == 1:                 # the context exchange needs a process group as well
                    continue
                for g in groups:
                    out.append(('%s/%s/%s/g%d' % (tag, fam, kind, g), dict(run='wavefront', nframes=nframes, reset=reset, fam=fam, kind=kind, group=g)))
    return out


_CUR = {'log': None, 'ex': None}                            # what the wrapped torch.distributed calls log to


def run_case(shard, spec, world, log):
    """Run one case on this rank, logging into `log`; returns {frame: [state values after its step]}."""
    nframes, reset = spec['nframes'], spec['reset']

    def get_window(f):                                      # (lrs, refs): the window's frame indices, refs + 100
        ex.ev('win', f)
        lrs = torch.tensor(shard.window_ids(f, nframes, FRAME_NUM), dtype=torch.float32)
        return lrs, lrs + 100.0

    on_result = lambda f, out: ex.ev('res', f)
    if spec['run'] == 'sharded':
        ex = (ExecPacked if spec['kind'] == 'callpacked' else Exec)(log, reset, nframes)
        _CUR.update(log=log, ex=ex)
        res = shard.run_sharded(ex, get_window, nframes, FRAME_NUM, reset, 1, 'cpu', aligned=spec['aligned'], on_result=on_result)
    else:
        _, cls, exchange, _ = [k for k in KINDS if k[0] == spec['kind']][0]
        ex = cls(log, reset, nframes)
        _CUR.update(log=log, ex=ex)
        tim = {}
        res = shard.run_wavefront(ex, get_window, nframes, FRAME_NUM, reset, 1, 'cpu', on_result=on_result,
                                  parts=family_parts(shard, spec['fam'], nframes, world, reset), timings=tim, exchange_contexts=exchange,
                                  group=spec['group'])
        log.append('-tim%d,%d,%d' % (tim['blocks'], tim['handoff_messages'], tim['context_messages']))
    return {f: [float(x) for x in v.tolist()] for f, v in res.items()}


def _wrap_dist():
    """Log every point-to-point call of torch.distributed (this process only) and the wait() of every receive."""
    import torch.distributed as dist

    class Work(object):
        def __init__(self, wk, tok):
            self.wk, self.tok = wk, tok

        def wait(self, *a, **k):
            _CUR['log'].append(_CUR['ex'].lane + self.tok)
            return self.wk.wait(*a, **k)

    def wrap(name, fn):
        def call(tensor, *args, **kwargs):
            peer = args[0] if args else kwargs.get('dst', kwargs.get('src'))
            grp = kwargs.get('group', args[1] if len(args) > 1 else None)
            tok = '%s,%s,%d,%s' % (peer, str(tensor.dtype)[6:], tensor.numel(), 'def' if grp is None else 'ctx')
            _CUR['log'].append(_CUR['ex'].lane + name + tok)
            out = fn(tensor, *args, **kwargs)
            return Work(out, 'rwait' + tok) if name == 'irecv' else out
        return call
    for name in ('send', 'recv', 'isend', 'irecv'):
        setattr(dist, name, wrap(name, getattr(dist, name)))


def worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from refvsr_amd import shard
    _wrap_dist()
    for cid, spec in cases(world):
        log = []
        res = run_case(shard, spec, world, log)
        q.put((rank, cid, ' '.join(log), res))
    q.put((rank, None, None, None))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_world(world, timeout=60):
    """{(case id, rank): (trace, results)} of every case of one world size: world 1 in process, else one gloo group of `world`
    spawned processes that runs all cases one after the other (what arrived within `timeout` of the previous case when a worker
    stalls).  Workers that are still alive at the end are killed."""
    out = {}
    if world == 1:
        sys.path.insert(0, ROOT)
        from refvsr_amd import shard
        for cid, spec in cases(1):
            log = []
            res = run_case(shard, spec, 1, log)
            out[(cid, 0)] = (' '.join(log), res)
        return out
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        done = 0
        while done < world:
            try:
                rank, cid, trace, res = q.get(timeout=timeout)
            except queue.Empty:                  # a rank died or waits for a message that never comes: the caller sees what is
                return out                       # missing (and what differs before that)
            if cid is None:
                done += 1
            else:
                out[(cid, rank)] = (trace, {int(f): v for f, v in res.items()})
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:                      # a worker that died leaves its peers waiting in a receive: never leave them behind
            if p.is_alive():
                p.kill()
                p.join(10)
    return out


# ---- the makespan model: predicted_speedup and choose_partition over a grid, as repr() of the floats
MODEL_T = dict(t_a=5.8, t_b1=0.96, t_b2=0.6)
MODEL_EXCHANGE = dict(t_prep=2.0, t_ctx=0.3, t_cold_x=0.5)
MODEL_GROUPS = ((1, None), (4, 7.0))                        # (group, t_a_single)


def model_grid():
    return list(itertools.product((2, 4, 8), (16, 64), (None, 9), MODEL_GROUPS, (None, MODEL_EXCHANGE)))


def model_point(shard, world, nframes, reset, group, exchange):
    """{'speedup/<family>': [repr, repr], 'choose': [blocks, repr, name]} of one grid point."""
    g, t1 = group
    out = {}
    for fam in FAMILIES:
        parts = family_parts(shard, fam, nframes, world, reset)
        if parts is not None:
            sp, span = shard.predicted_speedup(nframes, world, parts, reset, MODEL_T['t_a'], MODEL_T['t_b1'], MODEL_T['t_b2'], 0.3, 4.9,
                                               exchange=exchange, frame_num=5, steps_per_frame=500.0, group=g, t_a_single=t1)
            out['speedup/' + fam] = [repr(sp), repr(span)]
    blocks, sp, name = shard.choose_partition(nframes, world, reset, MODEL_T['t_a'], MODEL_T['t_b1'], MODEL_T['t_b2'], exchange=exchange,
                                              frame_num=5, group=g, t_a_single=t1)
    out['choose'] = [[list(b) for b in blocks], repr(sp), name]
    return out


def model_key(world, nframes, reset, group, exchange):
    return 'w%d/n%d/r%s/g%d/%s' % (world, nframes, reset or 0, group[0], 'x' if exchange else '-')


def _dump(path, items):
    """A JSON object with one line per entry."""
    with open(path, 'w') as fh:
        fh.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in items) + '\n}\n')


# ---- the trace file.  The ~1600 rank traces are made of a few hundred distinct tokens and many are equal (a rank that neither
# sends nor receives does the same in several cases), so the file holds: 'tokens' the vocabulary, most frequent first; 'traces' the
# distinct traces, two characters per event (the token's index in base 64, _B64); 'cases' per case the index of every rank's trace.
# Lossless: load_traces gives back {'<case>@<rank>': 'token token ...'}.
_B64 = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_'


def dump_traces(path, traces):
    """traces: {(case id, rank): 'token token ...'}."""
    count = {}
    for tr in traces.values():
        for tok in tr.split():
            count[tok] = count.get(tok, 0) + 1
    tokens = sorted(count, key=lambda t: (-count[t], t))
    assert len(tokens) <= 64 * 64
    code = {t: _B64[i // 64] + _B64[i % 64] for i, t in enumerate(tokens)}
    coded = {k: ''.join(code[t] for t in tr.split()) for k, tr in traces.items()}
    distinct = sorted(set(coded.values()))
    index = {c: i for i, c in enumerate(distinct)}
    cases_ = {}
    for (cid, rank) in sorted(traces):
        cases_.setdefault(cid, []).append(index[coded[(cid, rank)]])
    with open(path, 'w') as fh:
        fh.write('{"tokens": %s,\n"traces": [\n%s\n],\n"cases": {\n%s\n}}\n' % (
            json.dumps(tokens, separators=(',', ':')), ',\n'.join(json.dumps(c) for c in distinct),
            ',\n'.join('%s:%s' % (json.dumps(c), json.dumps(v, separators=(',', ':'))) for c, v in sorted(cases_.items()))))


def load_traces(path):
    with open(path) as fh:
        d = json.load(fh)
    tok = {_B64[i // 64] + _B64[i % 64]: t for i, t in enumerate(d['tokens'])}
    text = [' '.join(tok[c[i:i + 2]] for i in range(0, len(c), 2)) for c in d['traces']]
    return {'%s@%d' % (cid, rank): text[j] for cid, ids in d['cases'].items() for rank, j in enumerate(ids)}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from refvsr_amd import shard as _shard
    traces = {}
    for w in (1, 2, 3):
        traces.update((k, v[0]) for k, v in run_world(w).items())
    dump_traces(sys.argv[1], traces)
    _dump(sys.argv[2], [(model_key(*pt), model_point(_shard, *pt)) for pt in model_grid()])
