"""Drop-in model shell: `SRNet(config)` with the reference's constructor / forward / state_dict
surface (/root/reference/models/SRNet.py:11-61, models/archs/RefVSR.py:14-101,151-325), executing on
the HIP engine (refvsr_amd/engine.py).

  * `SRNet(config).Network` is resolved through `config.network` exactly like the reference's
    importlib plugin hook (SRNet.py:20-21): `refvsr_amd.archs.<config.network>.Network(config)`.
  * Parameters are registered under the reference's state-dict key names (refvsr_amd/weights.py), so
    `load_state_dict` accepts released checkpoints (with or without the DataParallel `module.`
    prefix, ckpt_manager.py:50-56) and `state_dict()` round-trips.
  * The recurrent forward state lives on the module between calls, like the reference
    (RefVSR.py:96-101,279-283): one module instance == one stream of consecutive frames, not
    thread-safe, not re-entrant.
  * There is NO CPU fallback: inputs must be CUDA (HIP) tensors and the HIP library must be built.
"""
import collections
import importlib
import operator
import os

import torch
import torch.nn as nn

from . import hip, inputs, ops
from .engine import Engine, Weights
from .fingerprint import WEIGHT_CHECKS, weight_check_policy
from .weights import state_spec, strip_module_prefix


_VERSION = operator.attrgetter('_version')


def _register(root, dotted, param):
    mod = root
    parts = dotted.split('.')
    for p in parts[:-1]:
        if not hasattr(mod, p):
            mod.add_module(p, nn.Module())
        mod = getattr(mod, p)
    mod.register_parameter(parts[-1], param)


def _input_yuv(config):
    """config.input_yuv checked (yuv.resolve_input): the format, or None (off)."""
    from . import yuv
    r = yuv.resolve_input(getattr(config, 'input_yuv', None), getattr(config, 'input_yuv_matrix', None),
                          getattr(config, 'input_yuv_range', None), getattr(config, 'input_yuv_chroma', None),
                          getattr(config, 'input_yuv_siting', None))
    return None if r is None else r[0]


_STRICT = {True: '%s: pipelined mode with input_ready= needs uint8 inputs that are contiguous or the channels-last view of [.., h, w, 3] bytes '
                 '(got strides %s): convert before the producer signals, or pass input_ready=None',
           False: 'pipelined mode with input_ready= needs contiguous float32 inputs (got %s, contiguous=%s): convert before the producer '
                  'signals, or pass input_ready=None'}


def _inputs(lrs, refs, what, strict=False, input_yuv=None, dim=5, convert=True):
    """The network's input contract, the ONE entry check (the kinds: inputs.py): float frames in [0, 1] (float16 / float64 are converted
    to float32, as in the reference), or uint8 frames meaning byte / 255 -- contiguous [.., 3, h, w] or the channels-last view of
    [.., h, w, 3] bytes, converted exactly on the device (refvsr_ingest_u8); lrs and refs are both uint8 or both not.  strict: inputs the
    engine reads off the caller's stream order (input_ready= on the pipelined path) are refused instead of converted; convert False
    (forward_group): what would need a conversion is refused, in forward_group's own words and order.  input_yuv (config.input_yuv, a
    format): dense Y'CbCr 4:2:0 windows [.., t, 3h/2, w] instead (`dim` - 1 dimensions), decoded on the device; nothing is converted."""
    if input_yuv is None and not convert:
        for t_ in (lrs, refs):
            if not inputs.as_is(t_) or t_.dim() != dim:
                raise RuntimeError('%s needs contiguous float32 or uint8 [B,t,3,h,w] inputs, or the channels-last view of uint8 '
                                   '[B,t,h,w,3] (got %s, contiguous=%s)' % (what, t_.dtype, t_.is_contiguous()))
        if lrs.dtype != refs.dtype:
            raise RuntimeError('%s: lrs and refs must both be uint8 or both float32 (got %s and %s)' % (what, lrs.dtype, refs.dtype))
        return lrs, refs
    inputs.check_window(lrs, refs, input_yuv, dim, what, 'B, t' if not convert else {5: 'n, t', 4: 't'}[dim])
    if input_yuv is not None:
        return lrs, refs
    u8 = lrs.dtype == torch.uint8
    for t_ in (lrs, refs):
        if strict and not inputs.as_is(t_):
            raise RuntimeError(_STRICT[u8] % ((what, tuple(t_.stride())) if u8 else (t_.dtype, t_.is_contiguous())))
    return tuple(t_ if inputs.as_is(t_) else t_.contiguous() if u8 else t_.float().contiguous() for t_ in (lrs, refs))


class _FlowNetHandle(nn.Module):
    """Placeholder carrying `load_ckpt` so that `SRNet.init()` keeps working (SRNet.py:44-45)."""

    def load_ckpt(self, pretrained):
        sd = torch.load(pretrained, map_location='cpu')
        sd = sd.get('state_dict', sd)
        own = dict(self.named_parameters())
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    own[k].copy_(v)


class Network(nn.Module):
    """HIP implementation of models/archs/RefVSR.py:Network (inference path)."""
    _engine_cls = Engine
    _weights_cls = Weights
    _family = 'RefVSR'                  # which state-dict contract this class carries, whatever name config.network has

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.rank = torch.distributed.get_rank() if config.dist else -1
        self.scale = config.scale
        self.flag_HD_in = config.flag_HD_in
        self.mid_channels = config.mid_channels
        self.add_module('FlowNet', _FlowNetHandle())
        for name, shape in state_spec(config, self._family).items():
            assert name.startswith('Network.')
            p = nn.Parameter(torch.zeros(shape), requires_grad=False)
            _register(self, name[len('Network.'):], p)
        self._plist = None
        self._packed = None
        self._packed_key = None
        self._engines = []
        # weight check (config.weight_check, fingerprint.weight_check_policy): the device fingerprint of the parameters that were packed,
        # the chunk table it is taken with, and the asynchronous checks in flight
        self._fp_table = None               # ops.FingerprintTable of the cached parameter list; None: the host-side detector alone
        self._fp_ptrs = None                # (data pointers, device) the table was built for
        self._fp0 = None                    # fingerprint of the packed parameters (python int, the int64 view of the 64 bits)
        self._fp_dev = None
        self._fp_slots = None               # free slots of the ring: (device int64 [1], pinned int64 [1], event)
        self._fp_pending = collections.deque()      # (slot, call number) of the launched checks, oldest first
        self._calls = 0
        self._just_reset = True             # the next call is the first after construction / .to() / reset() / invalidate()
        self._stale = False                 # invalidate(), or a mismatch found late: the next call re-packs

    # -- weights ------------------------------------------------------------------------------
    def _weights_key(self):
        # cheap change detector (a full walk over named_parameters() costs > 1 ms per call): cached parameter list, summed in-place
        # version counters (copy_ under no_grad), the storage address of EVERY tensor (`p.data = w` anywhere), device and dtype of the
        # first.  What it cannot see -- an in-place write through .data -- the device fingerprint sees (_check_fingerprint)
        if self._plist is None:
            self._plist = list(self.parameters())
        pl = self._plist
        return (len(pl), sum(map(_VERSION, pl)), tuple(map(torch.Tensor.data_ptr, pl)), pl[0].device, pl[0].dtype)

    def _apply(self, fn, *a, **k):               # .to() / .cuda() / .half() replace parameter storage
        self._plist = None
        self._just_reset = True
        return super()._apply(fn, *a, **k)

    def weight_check_mode(self):
        mode = getattr(self.config, 'weight_check', None) or 'auto'
        if mode not in WEIGHT_CHECKS:
            raise ValueError('weight_check must be one of %s, got %r' % (', '.join(WEIGHT_CHECKS), mode))
        return mode

    def _fingerprint_table(self, device, ptrs):
        """The chunk table of the cached parameter list (whose data pointers are `ptrs`), rebuilt when a pointer moved; None for a
        parameter set the kernel does not read -- not all contiguous float32 on `device` (a .half() net, parameters left on the
        host): the host-side detector alone."""
        if self._fp_ptrs != (ptrs, str(device)):
            pl = self._plist
            ok = all(p.is_cuda and p.device == device and p.dtype == torch.float32 and p.is_contiguous() and p.numel() > 0 for p in pl)
            self._fp_table = ops.FingerprintTable([p.detach() for p in pl]) if ok else None
            self._fp_ptrs = (ptrs, str(device))
        return self._fp_table

    def _fp_ring(self, device):
        if self._fp_slots is None or self._fp_dev != str(device):
            self._fp_drop_pending()
            self._fp_dev = str(device)
            depth = max(1, int(getattr(self.config, 'pipe_depth', None) or os.environ.get('REFVSR_PIPE_DEPTH') or 3)) + 1
            self._fp_slots = [(torch.empty(1, dtype=torch.int64, device=device), torch.empty(1, dtype=torch.int64).pin_memory(),
                               torch.cuda.Event()) for _ in range(depth)]
        return self._fp_slots

    def _fp_drop_pending(self):
        """Forget the checks in flight (their reference value is being replaced); their slots are reused once the copies landed."""
        while self._fp_pending:
            slot, _ = self._fp_pending.popleft()
            slot[2].synchronize()
            self._fp_slots.append(slot)

    def _fp_examine(self, wait_all=False):
        """Look at the launched checks that have completed (wait_all: at all of them; otherwise without waiting): the number of the
        earliest call whose fingerprint was not the packed one, or None."""
        bad = None
        while self._fp_pending and (wait_all or self._fp_pending[0][0][2].query()):
            slot, call = self._fp_pending.popleft()
            if wait_all:
                slot[2].synchronize()
            if slot[1].item() != self._fp0 and bad is None:
                bad = call
            self._fp_slots.append(slot)
        return bad

    def _check_fingerprint(self, device, how):
        """One call's fingerprint check, `how` = 'sync' | 'async' (fingerprint.weight_check_policy), on the caller's current stream --
        where the caller's writes to the parameters are ordered.  Returns True when the parameters are no longer the packed ones
        (the caller re-packs); raises when an EARLIER call's check says so: results were returned from stale weights since then."""
        tab = self._fingerprint_table(device, self._packed_key[0][2])
        if tab is None:
            return False
        slots = self._fp_ring(device)
        bad = self._fp_examine()
        if bad is None and not slots:
            slot, call = self._fp_pending.popleft()             # every slot in flight: wait for the oldest
            slot[2].synchronize()
            bad = call if slot[1].item() != self._fp0 else None
            slots.append(slot)
        stale_now = False
        if bad is None:
            with torch.cuda.device(device):
                if how == 'sync':
                    now = int(ops.param_fingerprint(tab).item())           # (the read waits for the caller's stream: every check before it landed)
                    bad = self._fp_examine(wait_all=True)
                    stale_now = now != self._fp0
                else:
                    slot = slots.pop()
                    ops.param_fingerprint(tab, out=slot[0])
                    slot[1].copy_(slot[0], non_blocking=True)
                    slot[2].record()
                    self._fp_pending.append((slot, self._calls))
        if bad is not None:
            n = self._calls - bad
            self._stale = True
            self._fp_drop_pending()
            self.reset()
            raise RuntimeError('refvsr_amd: the parameters were changed in place before call %d of this network (%d call%s ago) and the '
                               'asynchronous weight check has only now seen it: the results returned since that call were computed with '
                               'the old packed weights and are stale.  The weights are re-packed and the recurrent state is reset: '
                               'the next call is right, restart the clip with is_first_frame=True.  Call invalidate() after writing '
                               'parameters through .data inside a pipelined stream, or set config.weight_check = \'sync\'.'
                               % (bad, n, '' if n == 1 else 's'))
        return stale_now

    def _weights(self, device, call=None):
        """The packed weights of the current parameters.  call = (has frame_ids, first frame) for a network call: the device
        fingerprint check of config.weight_check runs as well (None: the host-side detector alone)."""
        key = (self._weights_key(), str(device))
        stale = self._packed is None or self._packed_key != key or self._stale
        if call is not None:
            self._calls += 1
            if not stale:
                how = weight_check_policy(self.weight_check_mode(), call[0], call[1], self._just_reset)
                if how != 'none':
                    stale = self._check_fingerprint(device, how)
            self._just_reset = False
        if stale:
            # the internal streams of a pipelined engine may still be reading the old blobs (nothing records them on those streams):
            # wait for the calls in flight before the allocator may hand the blobs' memory to the new ones
            for e in self._engines:
                e.drain()
            self._fp_drop_pending()
            sd = collections.OrderedDict(('Network.' + k, v.detach()) for k, v in self.named_parameters())
            self._packed = self._weights_cls(self.config, sd, device)
            self._packed_key = key
            self._stale = False
            # the fingerprint of what was packed, on the caller's stream, read synchronously: a pack costs far more than this read
            tab = self._fingerprint_table(device, key[0][2])
            if tab is not None:
                with torch.cuda.device(device):
                    self._fp0 = int(ops.param_fingerprint(tab).item())
            for e in self._engines:
                # everything an engine caches (per-frame matching / encodings / flows, the forward-branch state) was
                # computed with the old weights
                e.W = self._packed
                e.reset_state()
        return self._packed

    def reset(self):
        """Forget the recurrent state (start a new clip)."""
        self._just_reset = True
        for e in self._engines:
            e.reset_state()

    def invalidate(self):
        """Announce that parameters were written in a way the host cannot see (through .data): the next call re-packs the weights
        and restarts the recurrent state.  The documented way to change weights inside a pipelined stream."""
        self._stale = True
        self._just_reset = True

    # mirrors the attributes of the reference module that callers / tests look at
    @property
    def frame_itr_num(self):
        return self._engines[0].frame_itr_num if self._engines else 0

    def engine(self, n=0):
        return self._engines[n]

    def set_pipelined(self, on=True):
        """Cross-call stream pipelining (see Engine.set_pipelined for the contract)."""
        self.config.pipelined = bool(on)
        for e in self._engines:
            e.set_pipelined(on)

    def ensure_engines(self, n, device, call=None):
        """call: (has frame_ids, first frame) when a network call asks -- its weight check runs (see _weights)."""
        W = self._weights(device, call)
        while len(self._engines) < n:
            self._engines.append(self._engine_cls(self.config, W))
        return self._engines

    def _device(self, x):
        """The preamble of every entry that takes frames: the library is loaded (fails loudly if missing), the frames are on the GPU."""
        hip.lib()
        if not x.is_cuda:
            raise RuntimeError('refvsr_amd.Network runs on the GPU only (got a %s tensor); there is no CPU path' % x.device)
        return x.device

    def _outs(self, results, vis=None, dbg=None):
        """The OrderedDict a call returns for the n results [3,sh,sw] of its samples: 'vis' (is_log; dbg: the samples' debug dicts),
        'result' [n,3,sh,sw] (n == 1: a view, no 25 MB copy), 'eval_vis' (vis: the samples' map dicts; RefVSR_IR has none)."""
        outs = collections.OrderedDict()
        if dbg is not None:                                    # RefVSR.py:162-164,219-221,262-263,301-316
            outs['vis'] = collections.OrderedDict((k, torch.stack([d[k] for d in dbg], 0)) for k in (dbg[0] if dbg else ()))
        outs['result'] = results[0].unsqueeze(0) if len(results) == 1 else self._stack(results)
        if vis is not None and vis[0] is not None:
            outs['eval_vis'] = collections.OrderedDict((k, torch.stack([v[k] for v in vis], 0)) for k in vis[0])
        return outs

    def _stack(self, results):
        """n results [3,sh,sw] -> [n,3,sh,sw] in the engines' result layout (config.result_layout = 'hwc': dense [n,sh,sw,3] memory)."""
        return ops.stack_results(results, self._engines[0].result_layout)

    def _with_yuv(self, outs, frames, stacked):
        """config.result_yuv (extension; None = off: nothing is launched, no key): outs['yuv'] = the call's results [3,sh,sw] as Y'CbCr
        4:2:0 frames, batched as 'result' is -- [n, 3sh/2, sw] (stacked) or a tuple of [1, 3sh/2, sw].  ONE refvsr_result_to_yuv420
        launch per network call on the caller's current stream: the stream that receives 'result' and already waits for it,
        pipelined mode included (the rule of the device scorers).  'result' itself is returned as it was."""
        want = self._engines[0].result_yuv
        if want is not None:
            # (format and siting are both the engine's, taken from the config at its construction; an engine that declares no
            # siting is centre-sited.  4:2:2 / 4:4:4 frames -- [n, 2sh, sw] / [n, 3sh, sw] -- and left-sited chroma: one launch as well)
            y = ops.result_yuv(frames, want, getattr(self._engines[0], 'result_yuv_siting', 'centre'))
            outs['yuv'] = y if stacked else tuple(y[b:b + 1] for b in range(y.shape[0]))
        return outs

    def forward(self, lrs, refs, is_first_frame, is_log=False, is_train=False, frame_ids=None, input_ready=None):
        """Same contract as RefVSR.py:151: lrs, refs [n,t,3,h,w] in [0,1] (or uint8: byte / 255, see _inputs); returns OrderedDict with
        'result' [n,3,4h,4w] (+ 'eval_vis' when is_log and config.save_sample; + 'yuv' [n,6h,4w] under config.result_yuv).
        frame_ids / input_ready: extensions (window cache keyed by ids; when the inputs are final -- Engine.set_pipelined).
        Under config.input_yuv lrs, refs are Y'CbCr 4:2:0 windows [n, t, 3h/2, w] instead (uint8 | uint16 by format, see _inputs)."""
        if is_train:
            raise NotImplementedError('refvsr_amd implements the inference path only (is_train=False)')
        n = lrs.shape[0]
        self.ensure_engines(n, self._device(lrs), (frame_ids is not None, bool(is_first_frame)))
        # the engine's internal streams will read the inputs when `input_ready` says so, not in the caller's stream order: a
        # dtype / layout conversion here would be pending work on the caller's stream that nothing waits for -- refused
        # instead of raced against.  (input_ready=None waits for the caller's stream, conversions included; calls that take
        # the sequential path -- is_log, cache or overlap off -- run in the caller's stream order anyway.)
        strict = input_ready is not None and any(e.takes_pipelined_path(frame_ids, bool(is_log)) for e in self._engines[:n])
        lrs, refs = _inputs(lrs, refs, 'forward', strict, _input_yuv(self.config))
        want_vis = bool(is_log and self.config.save_sample)
        results, vis_all, dbg_all = [], [], []
        if (n > 1 and frame_ids is not None and not is_log and
                all(e.takes_pipelined_path(frame_ids, False) and e.group_ok() for e in self._engines[:n])):
            # round 5: the n samples are n independent streams over identical weights -- in steady state their forward-branch steps and
            # backward branches run as multi-map launches (Engine.forward_multi); same results as the loop below, bit for bit
            res = self._engine_cls.forward_multi(self._engines[:n], lrs, refs, bool(is_first_frame),
                                                 [[(b, f) for f in frame_ids] for b in range(n)], input_ready)
            return self._with_yuv(self._outs(res), res, True)
        for b in range(n):
            out, vis = self._engines[b].forward(lrs[b], refs[b], bool(is_first_frame), want_vis,
                                                None if frame_ids is None else [(b, f) for f in frame_ids], want_log=bool(is_log),
                                                input_ready=input_ready)
            if is_log:
                vis, dbg = vis
                dbg_all.append(dbg)
            results.append(out)
            vis_all.append(vis)
        return self._with_yuv(self._outs(results, vis_all if want_vis else None, dbg_all if is_log else None), results, True)

    def forward_group(self, lrs, refs, frame_ids, is_first_frame=False, input_ready=None, want_conf=False):
        """B CONSECUTIVE windows of one stream in one call (extension; see Engine.forward_group): lrs, refs [B,t,3,h,w] -- window b
        is what the b-th of B consecutive forward() calls would get as its n = 1 input -- frame_ids: B lists of t ids.  Returns
        OrderedDict{'result': tuple of B tensors [1,3,sh,sw]} (+ 'yuv': B tensors [1,3sh/2,sw] under config.result_yuv), bit-identical to the B calls; the backward branches and the
        upsamplers' inputs of the B frames run as multi-map launches, the forward-branch steps frame by frame.
        want_conf: the dict also carries 'eval_vis', a tuple of B OrderedDicts of [1,1,h,w] float32 maps -- what forward(window b, ..,
        is_log=True) returns as 'eval_vis' under config.save_sample (RefVSR.py:318-322), bit for bit.  (RefVSR_IR has no such maps:
        no 'eval_vis' key, as in forward().)  Off (the default), no launch is added."""
        dev = self._device(lrs)
        _inputs(lrs, refs, 'forward_group', input_yuv=_input_yuv(self.config), convert=False)
        assert len(frame_ids) == lrs.shape[0] and lrs.shape == refs.shape
        eng = self.ensure_engines(1, dev, (True, bool(is_first_frame)))[0]
        wins = [(lrs[b], refs[b], [(0, f) for f in frame_ids[b]]) for b in range(lrs.shape[0])]
        res = eng.forward_group(wins, bool(is_first_frame), input_ready, want_vis=bool(want_conf))
        res, vis = res if want_conf else (res, None)
        outs = collections.OrderedDict()
        outs['result'] = tuple(r.unsqueeze(0) for r in res)
        if vis is not None and all(v is not None for v in vis):
            outs['eval_vis'] = tuple(collections.OrderedDict((k, x.unsqueeze(0)) for k, x in v.items()) for v in vis)
        return self._with_yuv(outs, res, False)

    # ---- two-phase forward for the multi-GPU wavefront (refvsr_amd/shard.py:run_wavefront; not in the reference) ----
    def phase_a(self, lrs, refs, frame_ids=None, first_hint=False):
        """State-independent part of forward() (preparation + backward branch) for lrs, refs [n,t,3,h,w]."""
        dev = self._device(lrs)
        lrs, refs = _inputs(lrs, refs, 'phase_a', input_yuv=_input_yuv(self.config))
        self.ensure_engines(lrs.shape[0], dev, (frame_ids is not None, bool(first_hint)))
        return [self._engines[b].phase_a(lrs[b], refs[b], None if frame_ids is None else [(b, f) for f in frame_ids],
                                         first_hint) for b in range(lrs.shape[0])]

    def phase_a_group(self, lrs, refs, frame_ids, first_hints=None, streams=None):
        """phase_a of B windows of ONE clip in one pass (round 6; see Engine.phase_a_group): lrs, refs [B,t,3,h,w], frame_ids B lists of t
        ids (or sequences of B window tensors [t,3,h,w]).  Returns B handle lists (one per window, each what phase_a returns for an
        n = 1 call)."""
        dev = self._device(lrs[0])
        assert len(lrs) == len(refs) == len(frame_ids)
        eng = self.ensure_engines(1, dev, (True, False))[0]
        fmt = _input_yuv(self.config)
        wins = [_inputs(lrs[b], refs[b], 'phase_a_group', input_yuv=fmt, dim=4) + ([(0, f) for f in frame_ids[b]],) for b in range(len(lrs))]
        return [[h] for h in eng.phase_a_group(wins, first_hints, streams)]

    def phase_b1(self, handles, is_first_frame):
        """Serial part of phase_b (forward-branch step, carried state); see Engine.phase_b1."""
        for b, h in enumerate(handles):
            self._engines[b].phase_b1(h, bool(is_first_frame))
        return handles

    def phase_b2(self, handles, is_log=False):
        """State-free rest of phase_b (BW/FW fusion + upsampler); same return value as forward()."""
        want_vis = bool(is_log and self.config.save_sample)
        res = [self._engines[b].phase_b2(h, want_vis) for b, h in enumerate(handles)]
        return self._outs([r[0] for r in res], [r[1] for r in res] if want_vis else None, [] if is_log else None)

    def phase_b(self, handles, is_first_frame, is_log=False, after_state=None):
        """State-dependent rest (forward-branch step + upsampler); same return value as forward().
        after_state: see Engine.phase_b (called for sample 0)."""
        want_vis = bool(is_log and self.config.save_sample)
        res = [self._engines[b].phase_b(h, bool(is_first_frame), want_vis, after_state if b == 0 else None)
               for b, h in enumerate(handles)]
        return self._outs([r[0] for r in res], [r[1] for r in res] if want_vis else None, [] if is_log else None)


class SRNet(nn.Module):
    """models/SRNet.py:SRNet surface."""

    def __init__(self, config):
        super().__init__()
        self.rank = torch.distributed.get_rank() if config.dist else -1
        self.config = config
        self.device = config.device
        lib = importlib.import_module('refvsr_amd.archs.{}'.format(config.network))
        self.Network = lib.Network(config)
        self.data = collections.OrderedDict()

    def init(self):
        # dead in the reference too (wi / win are None in every config, SRNet.py:40-45)
        if self.config.wi is not None and self.config.win is not None:
            raise NotImplementedError('weight initialisation is a training feature')

    def input_constructor(self, res):
        b, f, c, h, w = res[:]
        imgs = torch.rand(b, f, c, h, w, device=self.device)
        return {'x': imgs, 'ref': imgs}

    def load_state_dict(self, state_dict, strict=True):
        return super().load_state_dict(strip_module_prefix(state_dict), strict=strict)

    def forward(self, x, ref, is_first_frame=True, is_log=False, is_train=False, frame_ids=None, input_ready=None):
        """frame_ids, input_ready (optional extensions, not in the reference): one id per window frame / when the inputs are
        final -- see Engine.forward and Engine.set_pipelined."""
        return self.Network.forward(x, ref, is_first_frame, is_log=is_log, is_train=is_train, frame_ids=frame_ids, input_ready=input_ready)

    def invalidate(self):
        """Parameters were written through .data (extension, not in the reference): the next call re-packs the weights -- see
        Network.invalidate."""
        self.Network.invalidate()

    def forward_group(self, x, ref, frame_ids, is_first_frame=False, input_ready=None, want_conf=False):
        """B consecutive windows of one stream in one call (extension, not in the reference): see Network.forward_group."""
        return self.Network.forward_group(x, ref, frame_ids, is_first_frame=is_first_frame, input_ready=input_ready, want_conf=want_conf)
