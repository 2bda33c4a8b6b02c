"""Multi-GPU execution of one clip: shard by output-frame index, one process per GPU.

The only cross-frame dependency of the path is the forward-branch state
(forward_feat_prop_prev, forward_flow_prev, forward_feat_prop_UP_prev, forward_conf_map_prop_prev,
frame_itr_num -- RefVSR.py:96-101,279-283).  The backward branch restarts from zeros in every window
(:211-214), and with `reset_branch = R` call k*R behaves as is_first_frame=True (:168-170).  Hence

  * shards that start at a multiple of R are bit-identical to the sequential run with NO
    communication -- `partition(..., aligned=True)`;
  * any other shard boundary needs ONE point-to-point hand-off of the state from rank r to r+1
    (RCCL send/recv over a single xGMI link; 63.8 MB fp32 for RefVSR_small at 270p).  There is no
    all-reduce anywhere on the inference path.

  * the hand-off chain serialises the ranks if each waits for the previous one to finish its whole
    shard (`run_sharded`).  `run_wavefront` splits every frame into phase A -- flows, matching,
    reference encoders, alignment and the whole backward branch, 85-90 % of the work, independent of
    the carried state -- and phase B -- one forward-branch step + the upsampler.  All ranks run phase A
    of all their frames concurrently; phase B then runs as a wavefront rank 0 -> 1 -> ... behind the
    hand-off, so the serial part of an N-rank run is ~(10-15 %) x nframes instead of 100 %.

`run_sharded` / `run_wavefront` are executor-agnostic (anything with forward or phase_a/phase_b and
export_state/import_state), so the protocols are tested on CPU with the gloo backend and the oracle as
executor, and on one GPU with two processes and the real engine.

This module is the transport, the two runners and the HIP adapter `EngineExecutor`.  What a rank issues is data from the pure
module shard_plan (partitions, ContextPlan, the makespan model; no torch): `lane_program` (lane a) and `chain_steps` (the
forward-branch chain).  The runners execute those two lists and the model replays them; the names are re-exported here.
"""
import contextlib
import os
import time

import torch
import torch.distributed as dist

from .shard_plan import (MAX_KEYFRAMES, STATE_KEYS, ContextPlan, as_blocks, chain_steps, choose_partition, group_lane_ops,  # noqa: F401
                         group_time, lane_program, needs_handoff, owner_map, partition, partition_chain, partition_cyclic,
                         partition_cyclic_growing, partition_hybrid, predicted_speedup, simulate_wavefront, window_ids,
                         window_is_hinted)


def _on(buf, device):
    """buf on `device` (a message buffer must live where the transport reads it: gloo wants host memory)."""
    return buf if str(buf.device).startswith(str(device)) else buf.to(device)


def send_state(state, dst, device, async_op=False):
    """Hand the forward-branch state to rank `dst`.

    * `state` a tensor: the packed device buffer of Engine.export_state_packed() (fp16 HWC maps + fp32 flow / conf in
      ONE message, 32.7 MB for RefVSR_small at 270p) -- the RCCL path: one send, no unpack kernels; `async_op=True`
      returns the work handle of an isend so that the sender's remaining kernels (the upsampler of its last frame) run
      under the transfer.
    * `state` a dict of planar fp32 tensors + frame_itr_num (executor-agnostic form, e.g. the oracle on gloo)."""
    if torch.is_tensor(state):
        if async_op:
            return dist.isend(_on(state, device), dst)
        dist.send(_on(state, device), dst)
        return None
    kf = [float(k) for k in (state.get('keyframe_idx') or [])]          # RefVSR_IR: key-frame indices travel with the state
    assert len(kf) <= MAX_KEYFRAMES
    meta = torch.tensor([float(state['frame_itr_num'])] + [float(d) for k in STATE_KEYS for d in state[k].shape[-2:]] +
                        [float(len(kf))] + kf + [0.0] * (MAX_KEYFRAMES - len(kf)), dtype=torch.float32, device=device)
    if async_op:
        # (round 6: the chain may issue a hand-off while lane a still has context messages to send -- a blocking send there can close
        #  a cycle with a peer that waits for one of them; the work handles keep their buffers alive)
        bufs = [meta] + [state[k].contiguous().to(device) for k in STATE_KEYS]
        return _Works([dist.isend(b_, dst) for b_ in bufs], bufs)
    dist.send(meta, dst)
    for k in STATE_KEYS:
        dist.send(state[k].contiguous().to(device), dst)
    return None


class _Works(object):
    """Several isend handles (and the buffers they read) behind one wait()."""

    def __init__(self, works, bufs):
        self.works, self.bufs = works, bufs

    def wait(self):
        for w_ in self.works:
            w_.wait()
        self.bufs = None


def recv_state(src, channels, device, nbytes=None):
    """Counterpart of send_state; nbytes: size of the packed buffer (Engine.state_nbytes) -> returns that buffer."""
    if nbytes is not None:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dist.recv(buf, src)
        return buf
    meta = torch.empty(1 + 2 * len(STATE_KEYS) + 1 + MAX_KEYFRAMES, dtype=torch.float32, device=device)
    dist.recv(meta, src)
    meta = meta.cpu().tolist()
    chans = {'feat': channels, 'flow': 2, 'feat_up': channels, 'conf': 1}
    st = {'frame_itr_num': int(meta[0])}
    nk = int(meta[1 + 2 * len(STATE_KEYS)])
    if nk:
        st['keyframe_idx'] = [int(v) for v in meta[2 + 2 * len(STATE_KEYS):2 + 2 * len(STATE_KEYS) + nk]]
    for i, k in enumerate(STATE_KEYS):
        hh, ww = int(meta[1 + 2 * i]), int(meta[2 + 2 * i])
        buf = torch.empty((chans[k], hh, ww), dtype=torch.float32, device=device)
        dist.recv(buf, src)
        st[k] = buf
    return st


def _import(executor, src, channels, device, split=False):
    """Receive the state from rank src into the executor (packed single-message form when the executor offers it; split=True:
    the two-message form -- the executor starts its forward-branch step on the small message and waits for the 2x state inside it)."""
    if split:
        nb_head, nb_tail = executor.state_split_nbytes()
        head = torch.empty(nb_head, dtype=torch.uint8, device=device)
        tail = executor.state_tail_buffer(device)
        assert tail.dtype == torch.uint8 and tail.numel() == nb_tail
        w_head = dist.irecv(head, src)
        w_tail = dist.irecv(tail, src)
        w_head.wait()
        executor.import_state_split(head, tail, w_tail.wait)
        return
    nb = executor.state_nbytes() if hasattr(executor, 'state_nbytes') else None
    st = recv_state(src, channels, device, nb)
    if nb is not None:
        executor.import_state_packed(st)
    else:
        executor.import_state(st)


def _export(executor):
    return executor.export_state_packed() if hasattr(executor, 'export_state_packed') else executor.export_state()


def _send_split(executor, dst, device, keep):
    """The state as two messages, small one first (Engine.export_state_split); returns the two work handles."""
    head, tail = executor.export_state_split()
    out = []
    for buf in (head, tail):
        buf = _on(buf, device)
        keep.append(buf)
        out.append(dist.isend(buf, dst))
    return out


def run_sharded(executor, get_window, nframes, frame_num, reset_branch, channels, device, aligned=False,
                on_result=None):
    """Run this rank's share of an nframes clip.

    executor(lrs[t,3,h,w], refs, is_first_frame) -> result; executor.export_state()/.import_state(st).
    get_window(f) -> (lrs, refs) of output frame f.  Returns {frame: result} for the local frames."""
    rank, world = dist.get_rank(), dist.get_world_size()
    results = {}
    for f, recv_from, first, send_to in chain_steps(as_blocks(partition(nframes, world, reset_branch, aligned)), rank, reset_branch):
        if recv_from is not None:
            _import(executor, recv_from, channels, device)
        lrs, refs = get_window(f)
        out = executor(lrs, refs, first)
        results[f] = out
        if on_result is not None:
            on_result(f, out)
        if send_to is not None:
            send_state(_export(executor), send_to, device)
    return results


_CTX_GROUP = None


def context_group():
    """A second process group for the context messages of run_wavefront(exchange_contexts=True): its own RCCL communicators and
    streams, so that a hand-off of the B1 chain never queues behind a 32 MB context transfer between the same two ranks.
    Collective on first use (every rank calls run_wavefront)."""
    global _CTX_GROUP
    if _CTX_GROUP is None:
        _CTX_GROUP = dist.new_group(ranks=list(range(dist.get_world_size())))
    return _CTX_GROUP


def run_wavefront(executor, get_window, nframes, frame_num, reset_branch, channels, device, on_result=None, parts=None,
                  timings=None, exchange_contexts=False, group=1):
    """Two-phase run of this rank's share of the clip.  parts: per-rank ranges [(start, end)] * world or a block list
    [(start, end, rank), ...] (default: the balanced contiguous partition).

    executor.phase_a(lrs, refs, frame_index, first_hint) -> handle   (state-free: preparation + backward branch)
    executor.phase_b1(handle, is_first_frame) -> handle              (forward-branch step: carries the state; in frame order)
    executor.phase_b2(handle) -> result                              (BW/FW fusion + upsampler: state-free)

    Order of issue on every rank (round 4): phase A of ALL local frames | per block in chain order: receive the state, B1 of the
    block's frames, send the state | B2 of all local frames.  An executor with two execution lanes (EngineExecutor: two HIP
    streams, `lane_a()` / `lane_b()` + the mark / wait hooks) runs the B1 chain on the second lane: B1(f) starts as soon as
    ITS phase A is done and the state is there, while the first lane is still walking the phase A of later frames -- the serial
    chain over the ranks no longer waits for a rank's whole phase A (round 3: `interleaved=False` of the model).  Executors
    without lanes (the CPU oracle on gloo) run the three groups one after the other: same results, same messages.
    Executors without phase_b1 / phase_b2 run phase_b(handle, first) per frame (B2 then sits on the chain).
    exchange_contexts (executors with prepare_context / export_context / import_context): every per-frame context is prepared
    ONCE, by the owner of its output frame, and sent to the other ranks whose windows need it (ContextPlan) -- the first window
    of a block no longer prepares two (four at a restart) contexts its neighbour prepares as well.  Lane a then walks
    ContextPlan.program(rank): prepare context i (+ isend to its consumers) | receive what window f lacks, then phase A of f (which
    finds every context prepared: a missing one raises, executor.strict_contexts).  Context messages travel in their own process
    group; every rank issues them in increasing frame order.
    group > 1 (round 6; executors with phase_a_group(windows, frames, hints) -> handles): lane a runs phase A in groups of up to
    `group` local windows (group_lane_ops) -- their backward branches as multi-map launches; B1(f) then waits for the group that
    holds f.  Same results, same messages in the same order.
    Results are identical to the sequential run.  Returns {frame: result} for the local frames.  timings (optional dict):
    'issue_a' / 'recv_wait' / 'issue_b1' / 'issue_b2' host seconds, 'handoff_messages' sent, 'blocks' local blocks,
    'context_messages' sent, 'context_wait' host seconds blocked waiting for contexts."""
    # (no process group: ONE rank walking the clip through the executor -- bench.py's one-rank figure; nothing is sent or received)
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)
    blocks = as_blocks(parts if parts is not None else partition(nframes, world), world)
    if hasattr(executor, 'begin_run'):
        executor.begin_run()                                       # (two-lane executors: the lanes wait for the caller's stream)
    lane_a = getattr(executor, 'lane_a', contextlib.nullcontext)
    lane_b = getattr(executor, 'lane_b', contextlib.nullcontext)
    lane_c = getattr(executor, 'lane_c', lane_a)                   # the upsamplers' lane (EngineExecutor: M, behind the backward chains)
    mark = getattr(executor, 'mark', lambda what, f: None)          # record "what of frame f is enqueued up to here"
    wait = getattr(executor, 'wait', lambda what, f: None)          # the CURRENT lane waits for that mark
    tim = {'issue_a': 0.0, 'recv_wait': 0.0, 'issue_b1': 0.0, 'issue_b2': 0.0, 'handoff_messages': 0,
           'blocks': sum(1 for _, _, r in blocks if r == rank), 'context_messages': 0, 'context_wait': 0.0}
    t0 = time.perf_counter()
    handles, keep = {}, []
    results, pending = {}, []
    split = hasattr(executor, 'phase_b1')
    # the hand-off in two messages (the receiver's step starts on the small one): executors that offer it, with the B1 / B2 split
    two_msg = split and bool(getattr(executor, 'split_handoff', False))
    after_state_ok = not split and bool(getattr(executor, 'supports_after_state', False))
    group = int(group) if hasattr(executor, 'phase_a_group') else 1

    # ---- the chain: chain_steps and a cursor.  B1 / B2 executors (round 6): the host does not issue it after ALL of lane a -- after
    # every window (group) of lane a, advance(False) issues the forward-branch steps that can go WITHOUT a blocking receive (a block
    # that starts at a restart or continues a local block: every block of a reset-aligned partition) and, one call later, their
    # upsamplers, so that on shards of tens of frames lane b and the upsamplers run under lane a instead of behind it (a 32-frame
    # shard: the host needs > 60 ms to issue its phase A).  Steps in frame order (the engine carries ONE state); a step that needs a
    # remote state stops the early issue until lane a is through (a blocking receive in the middle of lane a could close a cycle with
    # the context messages this rank has not sent yet).  Sends are asynchronous wherever they are issued -- but for executors with
    # only phase_b, whose whole chain is issued after lane a: per frame phase_b on lane b (B2 then sits on the chain), the send from
    # inside the block's last phase_b where the executor offers that (after_state), else blocking behind it.
    steps = chain_steps(blocks, rank, reset_branch)
    cur = {'b1': 0, 'b2': 0}
    early_chain = split and bool(getattr(executor, 'early_chain', hasattr(executor, 'lane_b')))

    def emit(f, out):
        results[f] = out
        if on_result is not None:
            on_result(f, out)

    def send(dst, async_op=True):                                  # the hand-off behind a block's last forward-branch step
        if two_msg:                                                # (the next block's chain starts as soon as this one ends)
            pending.extend(_send_split(executor, dst, device, keep))
        else:
            pending.append(send_state(_export(executor), dst, device, async_op=async_op))
        tim['handoff_messages'] += 1

    def advance(blocking):
        b2_upto = cur['b1']                                        # upsamplers lag one call: their B1 is long done when lane a gets there
        t2, waited = time.perf_counter(), tim['recv_wait']
        while cur['b1'] < len(steps):
            f, recv_from, first, send_to = steps[cur['b1']]
            if f not in handles or (recv_from is not None and not blocking):
                break                                              # its phase A is not issued yet | no blocking receive inside lane a
            with lane_b():
                if recv_from is not None:
                    t1 = time.perf_counter()
                    _import(executor, recv_from, channels, device, split=two_msg)
                    tim['recv_wait'] += time.perf_counter() - t1
                wait('a', f)
                if split:
                    handles[f] = executor.phase_b1(handles[f], first)
                    mark('b1', f)
                    if send_to is not None:
                        send(send_to)
                else:
                    keep.append(handles.pop(f))
                    if send_to is not None and after_state_ok:     # phase_b sends as soon as the carried state is final
                        emit(f, executor.phase_b(keep[-1], first, after_state=lambda: send(send_to)))
                    else:
                        emit(f, executor.phase_b(keep[-1], first))
                        if send_to is not None:
                            send(send_to, async_op=False)
            cur['b1'] += 1
        t3 = time.perf_counter()
        tim['issue_b1'] += t3 - t2 - (0.0 if split else tim['recv_wait'] - waited)
        if not split:
            return
        if blocking:
            b2_upto = cur['b1']
        with lane_c():
            while cur['b2'] < min(b2_upto, cur['b1']):             # ---- B2: upsamplers, off the chain
                f = steps[cur['b2']][0]
                wait('b1', f)
                h = handles.pop(f)
                keep.append(h)                                     # (two lanes: the handle's tensors stay allocated until the
                emit(f, executor.phase_b2(h))                      #  final synchronisation -- they are read on both streams)
                cur['b2'] += 1
        tim['issue_b2'] += time.perf_counter() - t3

    def issued(fs, hs):                                            # phase A of windows fs is enqueued: their handles
        for f, h in zip(fs, hs):
            handles[f] = h
            mark('a', f)
        if early_chain:
            advance(False)

    # ---- lane a: lane_program.  Without the exchange the windows are fetched right before their op; with it all up front (a
    # context is prepared from the frames of whichever local window holds them) and a missing context is a bug, not recomputed
    plan, window_of, strict = None, get_window, lambda on: None
    if exchange_contexts:
        plan = ContextPlan(nframes, world, blocks, reset_branch, frame_num)
        grp = context_group()
        comm_lane = getattr(executor, 'comm_lane', contextlib.nullcontext)   # an idle lane to post receives from (they then wait for nothing)
        wins = {f: get_window(f) for f, _, _, _ in steps}
        frame_in = {}                                              # (lr, ref) of every frame some local window holds
        for f, (lrs, refs) in wins.items():
            for j, i in enumerate(window_ids(f, nframes, frame_num)):
                frame_in.setdefault(i, (lrs[j], refs[j]))
        window_of = wins.__getitem__
        strict = getattr(executor, 'strict_contexts', strict)
    rx = {}
    try:                                                           # (the executor's strict-context mode ends with the run)
        strict(True)
        with lane_a():
            for op in lane_program(blocks, rank, group, plan):
                kind, x = op[0], op[1]
                if kind == 'ag':
                    issued(x, executor.phase_a_group([window_of(f) for f in x], list(x), [window_is_hinted(f, reset_branch) for f in x]))
                elif kind == 'a1':
                    lrs, refs = window_of(x)
                    issued((x,), [executor.phase_a(lrs, refs, x, window_is_hinted(x, reset_branch))])
                elif kind == 'prep':
                    executor.prepare_context(x, frame_in[x][0], frame_in[x][1])
                elif kind == 'post_recv':
                    with comm_lane():
                        buf = torch.empty(executor.context_nbytes(), dtype=torch.uint8, device=device)
                        rx[x] = (dist.irecv(buf, op[2], group=grp), buf)
                elif kind == 'send':
                    buf = _on(executor.export_context(x), device)
                    pending.append(dist.isend(buf, op[2], group=grp))
                    keep.append(buf)
                    tim['context_messages'] += 1
                else:                                              # 'wait_recv'
                    wk, buf = rx.pop(x)
                    t1 = time.perf_counter()
                    wk.wait()
                    tim['context_wait'] += time.perf_counter() - t1
                    executor.import_context(x, frame_in[x][0], frame_in[x][1], buf)
        assert not rx
        tim['issue_a'] = time.perf_counter() - t0 - tim['issue_b1'] - tim['issue_b2']
        advance(True)                                              # ---- the rest of the chain (blocking receives), then every B2 left
        for wk in pending:
            if wk is not None:
                wk.wait()
        getattr(executor, 'sync', lambda: None)()
    finally:
        strict(False)
    del keep[:]
    if timings is not None:
        timings.update(tim)
    return results


class EngineExecutor(object):
    """Adapter of the HIP `SRNet` (refvsr_amd/model.py) to run_sharded / run_wavefront: windows are named by their frame
    indices (id-keyed window cache, no content compare), the hand-off uses the packed single-message state."""
    supports_after_state = True

    def __init__(self, net, device, h, w, nframes, frame_num, keep_on_device=True, pipelined=True, inputs_materialised=False,
                 split_handoff=True, split_phase_a=True):
        self.net, self.dev, self.h, self.w, self.nframes, self.t = net, device, h, w, nframes, frame_num
        if getattr(getattr(net.Network, 'config', None), 'result_yuv', None) is not None:
            raise RuntimeError("the sharded runner returns RGB results only: config.result_yuv = %r is not supported here (convert the "
                               "gathered results with ops.result_to_yuv420, or run a single-GPU engine)" % (net.Network.config.result_yuv,))
        self.keep = keep_on_device
        self.eng = net.Network.ensure_engines(1, device)[0]
        # run_wavefront: the hand-off as [header | feat | flow | conf] + [feat_up]; the forward-branch step of the receiver starts on
        # the first message (Engine.export_state_split).  RefVSR_IR keeps the one-message form.
        self.split_handoff = bool(split_handoff) and bool(getattr(self.eng, 'split_state_ok', False))
        # cross-call pipelining of forward() (run_sharded): safe by default since round 4 -- the engine's internal streams wait for
        # the caller's stream, on which the windows are copied right before each call (Engine.set_pipelined); a caller whose
        # windows are resident and final before the run says so (inputs_materialised) and gets the full cross-call overlap
        self.eng.set_pipelined(bool(pipelined))
        self.input_ready = 'materialised' if inputs_materialised else None
        # run_wavefront's two execution lanes: phase A (+ B2) on one HIP stream, the B1 chain (+ the hand-off) on another, ordered by
        # per-frame events -- B1(f) runs as soon as phase A of ITS frame is done and the state has arrived
        self._lanes = None
        self._marks = {}
        self._marks_preset = set()
        self._ctx_spec = None
        # round 6: phase-A groups with the preparation on lane a and the backward chains (+ the upsamplers) on a third lane, like a
        # frame group's P | M sections (REFVSR_SHARD_SPLIT_A=0: the whole phase A on lane a, the A/B)
        self.split_phase_a = bool(split_phase_a) and os.environ.get('REFVSR_SHARD_SPLIT_A', '1') != '0' and self.eng.group_ok()

    def _streams(self):
        """(lane a = P: per-frame preparation, flows, context messages | lane b = F: the B1 chain + hand-off | comm | lane c = M: the
        backward chains of the phase-A groups + the upsamplers) -- the stream layout of a frame group (P | F | M)."""
        if self._lanes is None:
            self._lanes = tuple(torch.cuda.Stream(device=self.dev) for _ in range(4))
            self.begin_run()
        return self._lanes

    def begin_run(self):
        """Start of every run_wavefront on this executor: the lanes wait for the caller's stream as it stands -- whatever produced
        the (device-resident) windows / the weights there, also for the SECOND run on one executor (sync() orders the
        caller after the lanes, not the lanes after the caller)."""
        if self._lanes is not None:
            cur = torch.cuda.current_stream(self.dev)
            for s_ in self._lanes:
                s_.wait_stream(cur)

    def comm_lane(self):
        """An otherwise idle stream to post context receives from: a receive posted from lane a would first wait for everything
        lane a has queued (ProcessGroupNCCL orders its stream behind the caller's), i.e. the transfer would not overlap."""
        return torch.cuda.stream(self._streams()[2])

    # ---- per-frame contexts (run_wavefront with exchange_contexts).  Network.forward / phase_a name the frames of batch element b
    #      (b, frame id) towards its engine: the engine-level id of frame f of this single-clip executor is (0, f)
    def prepare_context(self, f, lr, ref):
        self.eng.prepare_context(lr.to(self.dev), ref.to(self.dev), (0, f))
        if self._ctx_spec is None:
            self._ctx_spec = self.eng.context_spec((0, f))

    def context_nbytes(self):
        assert self._ctx_spec is not None, 'no context prepared yet: the message layout comes from the first own context'
        return self.eng.context_nbytes(self._ctx_spec)

    def export_context(self, f):
        return self.eng.export_context((0, f))

    def strict_contexts(self, on):
        """While on, a window that finds one of its contexts missing raises instead of preparing it (Engine.prepare_frame)."""
        self.eng.ctx_strict = bool(on)

    def import_context(self, f, lr, ref, buf):
        b = buf.to(self.dev)
        if b.is_cuda:
            b.record_stream(torch.cuda.current_stream(self.dev))
        self.eng.import_context(lr.to(self.dev), ref.to(self.dev), (0, f), b, self._ctx_spec)

    def lane_a(self):
        return torch.cuda.stream(self._streams()[0])

    def lane_b(self):
        return torch.cuda.stream(self._streams()[1])

    def lane_c(self):
        """Where the upsamplers (B2) go: behind the backward chains on M when the phase-A groups are split over P | M, else lane a."""
        return torch.cuda.stream(self._streams()[3 if self.split_phase_a else 0])

    def mark(self, what, f):
        if what == 'a' and (what, f) in self._marks_preset:       # a split phase-A group: the handle's own event on M is the mark
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self._marks[(what, f)] = ev

    def wait(self, what, f):
        ev = self._marks.get((what, f))
        if ev is not None:
            torch.cuda.current_stream(self.dev).wait_event(ev)

    def _ids(self, f):
        return window_ids(f, self.nframes, self.t)

    def _out(self, r):
        # results never travel between ranks (only the carried state does); a channels-last result (config.result_layout = 'hwc')
        # keeps its layout here: indexing a frame and .cpu() both preserve the strides of a dense tensor
        return r if self.keep else r.cpu()

    def __call__(self, lrs, refs, first, f=None):
        ids = None if f is None else self._ids(f)
        return self._out(self.net(lrs[None].to(self.dev), refs[None].to(self.dev), first, frame_ids=ids,
                                  input_ready=self.input_ready if ids is not None else None)['result'][0])

    def phase_a(self, lrs, refs, f, hint):
        return self.net.Network.phase_a(lrs[None].to(self.dev), refs[None].to(self.dev), frame_ids=self._ids(f), first_hint=hint)

    def phase_a_group(self, windows, fs, hints):
        """phase_a of several local windows in one pass (run_wavefront(group=)): windows [(lrs, refs)], fs their frame indices."""
        streams = None
        if self.split_phase_a:
            lanes = self._streams()
            streams = (lanes[3], (lanes[1],))
        hs = self.net.Network.phase_a_group([w_[0].to(self.dev) for w_ in windows], [w_[1].to(self.dev) for w_ in windows],
                                            [self._ids(f) for f in fs], hints, streams)
        for f, h in zip(fs, hs):
            if h[0].get('ready') is not None:
                self._marks[('a', f)] = h[0]['ready']
                self._marks_preset.add(('a', f))
        return hs

    def phase_b(self, handles, first, after_state=None):
        return self._out(self.net.Network.phase_b(handles, first, after_state=after_state)['result'][0])

    def phase_b1(self, handles, first):
        return self.net.Network.phase_b1(handles, first)

    def phase_b2(self, handles):
        return self._out(self.net.Network.phase_b2(handles)['result'][0])

    def sync(self):
        torch.cuda.synchronize(self.dev)
        if self._lanes is not None:                         # results were produced on the lanes: order them before the caller's stream
            cur = torch.cuda.current_stream(self.dev)
            for s_ in self._lanes:
                cur.wait_stream(s_)
        self._marks.clear()
        self._marks_preset.clear()

    def state_nbytes(self):
        return self.eng.state_nbytes(self.h, self.w)

    def export_state_packed(self):
        return self.eng.export_state_packed()

    def import_state_packed(self, buf):
        self.eng.import_state_packed(buf.to(self.dev))

    # ---- the two-message hand-off
    def state_split_nbytes(self):
        cs = self.eng._state_cs()
        return self.eng.state_head_nbytes(self.h, self.w), 2 * self.h * 2 * self.w * cs * 2

    def export_state_split(self):
        head, feat_up = self.eng.export_state_split()
        return head, feat_up.reshape(-1).view(torch.uint8)

    def state_tail_buffer(self, device):
        """The buffer the second message is received into: the engine's next 2x state itself when the transport writes device
        memory (RCCL), a host buffer otherwise (gloo: copied to the device by the deferred wait)."""
        cs = self.eng._state_cs()
        self._tail = torch.empty((2 * self.h, 2 * self.w, cs), dtype=torch.float16, device=self.dev)
        if str(device).startswith('cuda'):
            return self._tail.view(-1).view(torch.uint8)
        return torch.empty(self._tail.numel() * 2, dtype=torch.uint8, device=device)

    def import_state_split(self, head, tail, wait_tail):
        feat_up = self._tail
        if tail.is_cuda:
            waiter = wait_tail
        else:
            def waiter():
                wait_tail()
                feat_up.copy_(tail.view(torch.float16).view(feat_up.shape))
        self.eng.import_state_head(head.to(self.dev), feat_up, waiter)
