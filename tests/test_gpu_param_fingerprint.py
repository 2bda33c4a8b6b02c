"""The parameter fingerprint on a real MI355X: refvsr_param_fingerprint against its numpy model bit for bit, and the model shell's
weight check end to end -- in-place edits of a parameter that the host-side detector cannot see are picked up (synchronously where
the policy says so, late but loudly on the asynchronous path), unchanged weights are never re-packed."""
import collections

import numpy as np
import pytest
import torch

from refvsr_amd import fingerprint as fp

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 255, 256, 257, 1023, 1025, 100352)
KEY = 'backward_resblocks.main.2.0.conv2.weight'         # second conv of a propagation block: neither first nor last, feeds every result
NFRAMES, T = 10, 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ kernel against model
def _table(dev, seed=11):
    """Tensors of SIZES words as views of one buffer at storage offsets that are 1, 2, 3 (and 0) elements past a 16-byte boundary;
    random bit patterns with -0, NaNs of several payloads, infinities and subnormals among them."""
    rs = np.random.RandomState(seed)
    offs, pos = [], 0
    for i, n in enumerate(SIZES):
        pos = (pos + 3) // 4 * 4 + (1, 2, 3, 0)[i % 4]
        offs.append(pos)
        pos += n
    bits = rs.randint(0, 2 ** 32, size=pos + 8, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x7fc00000, 0x7fc00001, 0xffffffff, 0x7f800000, 0x00000001, 0x00000000, 0xff800000], dtype=np.uint32)
    for o, n in zip(offs, SIZES):
        k = min(n, len(special))
        bits[o:o + k] = special[:k]
        bits[o + n - 1] = special[(o + n) % len(special)]
    buf = torch.from_numpy(bits.view(np.int32).copy()).to(dev)
    tensors = [buf[o:o + n].view(torch.float32) for o, n in zip(offs, SIZES)]
    assert [t.storage_offset() % 4 for t in tensors[:4]] == [1, 2, 3, 0] and all(t.data_ptr() % 4 == 0 for t in tensors)
    return buf, tensors, [bits[o:o + n].copy() for o, n in zip(offs, SIZES)]


def test_kernel_returns_the_models_bits(dev):
    from refvsr_amd import ops
    buf, tensors, words = _table(dev)
    want = fp.as_int64(fp.param_fingerprint_model([w.view(np.float32) for w in words]))
    got = ops.param_fingerprint(tensors)
    assert got.dtype == torch.int64 and got.shape == (1,) and got.is_cuda
    assert int(got.item()) == want
    # every tensor alone (one chunk / several chunks, every alignment), and in another order
    for t, w in zip(tensors, words):
        assert int(ops.param_fingerprint([t]).item()) == fp.as_int64(fp.param_fingerprint_model([w.view(np.float32)])), t.numel()
    rev = fp.as_int64(fp.param_fingerprint_model([w.view(np.float32) for w in words[::-1]]))
    assert int(ops.param_fingerprint(tensors[::-1]).item()) == rev != want
    # a prepared table, its `out` argument, and a flipped word: first, middle and last word of the largest tensor and a 1-word tensor
    tab = ops.FingerprintTable(tensors)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    assert ops.param_fingerprint(tab, out=out) is out and int(out.item()) == want
    ib = buf.view(torch.int32)
    for ti, pos in ((8, 0), (8, SIZES[8] // 2), (8, SIZES[8] - 1), (0, 0), (5, 256)):
        e = tensors[ti].storage_offset() + pos
        ib[e] ^= 1 << 9
        words[ti][pos] ^= np.uint32(1 << 9)
        flipped = int(ops.param_fingerprint(tab).item())
        assert flipped != want and flipped == fp.as_int64(fp.param_fingerprint_model([w.view(np.float32) for w in words])), (ti, pos)
        ib[e] ^= 1 << 9
        words[ti][pos] ^= np.uint32(1 << 9)
    assert int(ops.param_fingerprint(tab).item()) == want


def test_same_value_on_two_streams(dev):
    from refvsr_amd import ops
    _, tensors, words = _table(dev, seed=12)
    want = fp.as_int64(fp.param_fingerprint_model([w.view(np.float32) for w in words]))
    tab = ops.FingerprintTable(tensors)
    torch.cuda.synchronize()
    outs = []
    for st in (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)):
        with torch.cuda.stream(st):
            outs.append(ops.param_fingerprint(tab))
    torch.cuda.synchronize()
    assert [int(o.item()) for o in outs] == [want, want]


def test_refused_tables(dev):
    from refvsr_amd import ops
    with pytest.raises(ValueError, match='empty tensor list'):
        ops.param_fingerprint([])
    x = torch.zeros(4, 6, device=dev)
    with pytest.raises(RuntimeError, match='contiguous float32'):
        ops.param_fingerprint([x.t()])
    with pytest.raises(RuntimeError, match='contiguous float32'):
        ops.param_fingerprint([x.half()])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def clip():
    from refvsr_amd.synth import make_clip
    lr, rf, _ = make_clip(NFRAMES, 16, 16, seed=0, want_gt=False)
    return lr, rf


@pytest.fixture(scope='module')
def sds():
    from refvsr_amd import get_config, make_state_dict
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    sd = make_state_dict(cfg, 1234)
    other = make_state_dict(cfg, 4321)
    edited = collections.OrderedDict(sd)
    edited['Network.' + KEY] = other['Network.' + KEY].clone()
    return sd, edited


def _net(dev, sd, mode='auto', pipelined=False):
    from refvsr_amd import SRNet, get_config
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num = T
    cfg.weight_check = mode
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(sd)
    if pipelined:
        net.Network.set_pipelined(True)
    return net


def _call(net, clip, dev, f, first, ids=True):
    from refvsr_amd.synth import window_indices
    lr, rf = clip
    w = window_indices(f, NFRAMES, T)
    return net(lr[w][None].to(dev), rf[w][None].to(dev), first, frame_ids=w if ids else None)['result'].clone()


@pytest.fixture(scope='module')
def fresh(dev, clip, sds):
    """What a fresh SRNet that got its state dict through load_state_dict returns for a first-frame call on frame 0, for both
    state dicts: with frame ids, positional, and with frame ids in pipelined mode.  Computed once."""
    out = {}
    for name, sd in zip(('orig', 'edited'), sds):
        net = _net(dev, sd)
        r = {'ids': _call(net, clip, dev, 0, True)}
        net.Network.reset()
        r['pos'] = _call(net, clip, dev, 0, True, ids=False)
        net.Network.set_pipelined(True)
        net.Network.reset()
        r['pipe'] = _call(net, clip, dev, 0, True)
        torch.cuda.synchronize()
        out[name] = r
    assert not torch.equal(out['orig']['ids'], out['edited']['ids']), 'the edited parameter must matter to the result'
    return out


def _edit(net, how, w, dev):
    names = [k for k, _ in net.Network.named_parameters()]
    assert 0 < names.index(KEY) < len(names) - 1
    p = dict(net.Network.named_parameters())[KEY]
    v0 = p._version
    if how == 'copy_':
        p.data.copy_(w)
    else:
        p.data = w.clone().to(dev)
    assert p._version == v0, 'the edit is invisible to the version counters'


@pytest.mark.parametrize('how', ['copy_', 'assign'])
def test_in_place_edit_is_picked_up(dev, clip, sds, fresh, how):
    sd, edited = sds
    net = _net(dev, sd)
    pre = _call(net, clip, dev, 0, True)
    _call(net, clip, dev, 1, False)
    assert torch.equal(pre, fresh['orig']['ids'])
    _edit(net, how, edited['Network.' + KEY], dev)
    net.Network.reset()
    got = _call(net, clip, dev, 0, True)
    assert torch.equal(got, fresh['edited']['ids']), 'reset() + first frame after the edit runs on the edited weights'
    assert not torch.equal(got, pre)
    # back to the first weights, then a positional call with no reset(): the check of that call sees it
    _call(net, clip, dev, 1, False)
    _edit(net, how, sd['Network.' + KEY], dev)
    got = _call(net, clip, dev, 0, True, ids=False)
    assert torch.equal(got, fresh['orig']['pos'])
    assert not torch.equal(got, fresh['edited']['pos'])


def test_asynchronous_path_reports_late_and_recovers(dev, clip, sds, fresh):
    sd, edited = sds
    net = _net(dev, sd, pipelined=True)
    _call(net, clip, dev, 0, True)
    for f in (1, 2):
        _call(net, clip, dev, f, False)
    _edit(net, 'copy_', edited['Network.' + KEY], dev)
    _call(net, clip, dev, 3, False)                       # (may be stale: its check is in flight)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r'changed in place before call 4 .*stale.*invalidate\(\)'):
        _call(net, clip, dev, 4, False)
    got = _call(net, clip, dev, 0, True)                  # the stream restarts: right from here on
    torch.cuda.synchronize()
    assert torch.equal(got, fresh['edited']['pipe'])
    # announced with invalidate(): no error, the next call is right
    _call(net, clip, dev, 1, False)
    _edit(net, 'copy_', sd['Network.' + KEY], dev)
    net.invalidate()
    got = _call(net, clip, dev, 0, True)
    torch.cuda.synchronize()
    assert torch.equal(got, fresh['orig']['pipe'])
    for f in (1, 2, 3, 4):
        _call(net, clip, dev, f, False)                   # and nothing is reported later
    torch.cuda.synchronize()
    _call(net, clip, dev, 5, False)


def test_off_mode_keeps_the_host_detector_alone(dev, clip, sds, fresh):
    sd, edited = sds
    net = _net(dev, sd, mode='off')
    pre = _call(net, clip, dev, 0, True)
    _edit(net, 'copy_', edited['Network.' + KEY], dev)
    net.Network.reset()
    assert torch.equal(_call(net, clip, dev, 0, True), pre), "'off': a .data.copy_ is not seen"
    _edit(net, 'assign', edited['Network.' + KEY], dev)
    net.Network.reset()
    assert torch.equal(_call(net, clip, dev, 0, True), fresh['edited']['ids']), "'off': a moved middle pointer is seen"


def test_unchanged_weights_are_never_repacked(dev, clip, sds):
    from refvsr_amd.engine import Weights
    sd, _ = sds
    results = {}
    for mode in ('off', 'auto', 'sync'):
        class Counting(Weights):
            built = 0

            def __init__(self, *a, **k):
                Counting.built += 1
                super().__init__(*a, **k)
        net = _net(dev, sd, mode=mode)
        net.Network._weights_cls = Counting
        outs = [_call(net, clip, dev, 0, True)] + [_call(net, clip, dev, f, False) for f in range(1, 9)]
        torch.cuda.synchronize()
        assert Counting.built == 1, mode
        results[mode] = outs
    for mode in ('auto', 'sync'):
        assert all(torch.equal(a, b) for a, b in zip(results[mode], results['off'])), mode
