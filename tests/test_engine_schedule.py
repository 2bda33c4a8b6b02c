"""The engine's stream schedule, pinned line by line (CPU): every launch with its stream, every wait_event / wait_stream /
Event.record / synchronize / record_stream with its operands, stream entry and exit, the iteration counter and the cache keys a call
leaves behind -- for forward() (sequential and pipelined), forward_group, forward_multi, phase_a / phase_a_group and phase_b1 /
phase_b2 / phase_b -- must equal the traces recorded from the engine before its call forms were rebuilt on one window walk and one
P | F | M schedule (tests/golden/engine_schedule.json, recorded with tests/engine_schedule_trace.py).  The GPU bit-identity tests
cannot see a missing wait that happens not to race; this test sees it as a missing line."""
import os

import pytest

import engine_schedule_trace as est

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_schedule.json')


@pytest.fixture(scope='module')
def golden():
    return est.load(GOLDEN)


@pytest.fixture(scope='module')
def recorded():
    mp = pytest.MonkeyPatch()
    try:
        return est.record(mp.setattr)
    finally:
        mp.undo()


def test_every_scenario_is_recorded(golden, recorded):
    assert list(recorded) == list(golden)


@pytest.mark.parametrize('name', list(est.scenarios()))
def test_engine_schedule(golden, recorded, name):
    got, want = recorded[name], golden[name]
    for i, (a, b) in enumerate(zip(got['trace'], want['trace'])):
        assert a == b, '%s: line %d differs (after %r)' % (name, i, want['trace'][max(0, i - 3):i])
    assert len(got['trace']) == len(want['trace']), '%s: %d lines, recorded %d' % (name, len(got['trace']), len(want['trace']))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], (name, key)


def test_recorded_traces_reach_every_call_form(golden):
    """The cap of the recording: the operations whose placement the schedule has to get right occur in it."""
    lines = [ln for sc in golden.values() for ln in sc['trace']]
    streams = set(ln.split('|')[0] for ln in lines if not ln.startswith('#'))
    assert {'C', 'P', 'F', 'FP', 'M0', 'M1', 'M0M1', 'M0M1FP', 'A', 'GM', 'B1', 'S0'} <= streams
    for what in ('wait_event', 'wait_stream', '.record(', '.synchronize()', '| rs ', 'ctx(lr', 'in=#', 'enter ', 'exit ', 'pyramid', 'prepare_frame',
                 'resblocks backward_resblocks', 'prop_step', 'compute_up', 'conf_vis', 'ingest_u8', 'spynet', 'flow_resize', 'compare',
                 'warp_planar', 'after_state', 'up_from_lr', 'heads=[head(', 'compare bytes', 'C| yuv420_ingest nv12', 'P| yuv420_ingest nv12',
                 'A| yuv420_ingest nv12', 'S1| yuv420_ingest p010'):
        assert any(what in ln for ln in lines), what
    # the input kinds: a decode launch in every call form, and at once for a context prepared outside a call
    for name, what in (('forward seq uint8', 'ingest_u8'), ('forward seq yuv nv12', 'yuv420_ingest'), ('forward pipelined yuv nv12', 'yuv420_ingest'),
                       ('forward_group yuv nv12 B=2', 'yuv420_ingest'), ('forward_multi n=2 yuv p010', 'yuv420_ingest'),
                       ('phase_a yuv ids=1', 'yuv420_ingest'), ('phase_a yuv ids=0', 'yuv420_ingest'), ('phase_a_group B=3 yuv', 'yuv420_ingest'),
                       ('contexts prepared ahead uint8', 'ingest_u8'), ('contexts prepared ahead yuv', 'yuv420_ingest')):
        assert any(what in ln for ln in golden[name]['trace']), (name, what)
    # a window of another kind or another layout pair: nothing of the previous window is compared (6 = the window's own three frames)
    for name in ('forward seq float then uint8', 'forward seq uint8 ref layout changes'):
        tr = golden[name]['trace']
        assert [ln for ln in tr[tr.index('# forward 1'):tr.index('#- forward 2')] if 'compare' in ln] == ['C| compare bytes 6']


def test_stream_events_name_their_streams(golden):
    """bench.py's per-section events: the keys of an entry and the stream each event was recorded on."""
    for name in ('forward_group stream_events', 'forward_group stream_events first inside'):
        for g in (0,):
            for ev in golden[name]['stream_events.%d' % g]:
                assert sorted(ev) == ['F0', 'F1', 'M0', 'M1', 'P0', 'P1', 'n']
                assert [ev[k].split('@')[1] for k in ('P0', 'P1', 'F0', 'F1', 'M0', 'M1')] == ['P', 'P', 'F', 'F', 'M0M1', 'M0M1']
                assert all(ev[k].split('@')[0].endswith('t') for k in ('P0', 'P1', 'F0', 'F1', 'M0', 'M1'))      # timed events
