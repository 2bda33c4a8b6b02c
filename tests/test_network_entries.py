"""Network's public entries, pinned call by call (CPU): for forward (n = 1, n = 2, with and without frame ids, is_log with and without
save_sample, the forward_multi route), forward_group (with and without want_conf), phase_a, phase_a_group, phase_b and phase_b1 +
phase_b2, over every kind of input the entry check tells apart (float32 / float16 / float64 / strided, uint8 planar / channels-last /
other strides, a byte / float mix, 4:2:0 windows under config.input_yuv, windows of the wrong kind, host tensors), input_ready unset
and set, config.result_yuv off and on: what the engine is handed (dtype, shape, strides, the caller's own tensor or a converted copy,
ids and flags), the returned dict (keys in order; shape, dtype of every value and whether it is a view of the engine's result) or the
refusal (type and full message) must equal what was recorded from the model.py that preceded the rebuild of the frame boundary on one
input source (tests/golden/network_entries.json, recorded with tests/network_entry_trace.py; the commit is the file's first entry)."""
import os
import re

import pytest

import network_entry_trace as net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'network_entries.json')


@pytest.fixture(scope='module')
def golden():
    src, g = net.load(GOLDEN)
    assert re.fullmatch(r'[0-9a-f]{40}', src['commit'])
    return g


@pytest.fixture(scope='module')
def recorded():
    mp = pytest.MonkeyPatch()
    try:
        return net.record(mp.setattr)
    finally:
        mp.undo()


def test_every_entry_call_is_recorded(golden, recorded):
    assert list(recorded) == list(golden)
    n_in = len(net.inputs())
    assert len(golden) == len(net.entries()) * n_in * 4 + len(net.tails()) * 2 + 1


@pytest.mark.parametrize('entry', list(net.entries()) + list(net.tails()) + ['set_pipelined reset is_train'])
def test_network_entry(golden, recorded, entry):
    keys = [k for k in golden if k == entry or k.startswith(entry + ' | ')]
    assert keys
    for k in keys:
        assert recorded[k] == golden[k], k


def test_recorded_calls_reach_every_branch(golden):
    """The cap of the recording: every refusal a test matches, every conversion and every shape of returned dict occur in it."""
    raised = [v['raised'] for v in golden.values() if 'raised' in v]
    for what in ('both be uint8 or both float', 'input_ready', 'contiguous float32', 'need config.input_yuv',
                 r"input_yuv = 'nv12'.*torch.uint8 \[n, t, 3h/2, w\]", r'\[B, t, 3h/2, w\]', r'\[t, 3h/2, w\]', 'one shape', 'not contiguous',
                 'forward_group needs contiguous float32', 'forward_group: lrs and refs must both', 'runs on the GPU only'):
        assert any(re.search(what, r) or what in r for r in raised), what
    assert 'is_train=False' in golden['set_pipelined reset is_train']['out'][-1]
    logs = [ln for v in golden.values() for ln in v['log']]
    for what in ('.forward(', 'forward_multi(', '.forward_group(', '.phase_a(', '.phase_a_group(', '.phase_b(', '.phase_b1(', '.phase_b2(',
                 'stack_results(2, chw)', 'result_to_yuv420(res0 res1, nv12 bt709 limited)', 'result_to_yuv420(res0.0 res0.1,', ' own', ' copy',
                 'uint8[3,3,4,6]/[72,1,18,3] own', 'uint16[3,6,6]', 'hip.lib()', '_weights('):
        assert any(what in ln for ln in logs), what
    # a float16 window is converted by forward and refused by forward_group; the engine sees the caller's own bytes
    assert golden['forward n=1 | float16 | ready=- | result_yuv=-']['log'][-1].count('float32[3,3,4,6]/[72,24,6,1] copy') == 2
    assert 'forward_group' in golden['forward_group | float16 | ready=- | result_yuv=-']['raised']
    assert golden['forward n=1 | uint8 channels-last | ready=ready | result_yuv=-']['log'][-1].count(' own') == 2
    # n = 1: 'result' is a view of the engine's result; n = 2: the stacked copy
    assert golden['forward n=1 | float32 | ready=- | result_yuv=-']['out'] == ['OrderedDict', ['result', 'float32[1,3,16,24] view of res0']]
    assert golden['forward n=2 | float32 | ready=- | result_yuv=-']['out'] == ['OrderedDict', ['result', 'float32[2,3,16,24]']]
    outs = [v['out'] for v in golden.values() if 'out' in v and v['out'][0] == 'OrderedDict']
    shapes = set(tuple(kv[0] for kv in o[1:]) for o in outs)
    assert {('result',), ('result', 'yuv'), ('vis', 'result'), ('vis', 'result', 'eval_vis'), ('vis', 'result', 'eval_vis', 'yuv'),
            ('result', 'eval_vis'), ('result', 'eval_vis', 'yuv')} <= shapes
    # phase_b and phase_b2 return no 'yuv' key under config.result_yuv (kept as it is)
    for k, v in golden.items():
        if k.startswith('phase_b'):
            assert 'yuv' not in [kv[0] for kv in v['out'][1:]], k
