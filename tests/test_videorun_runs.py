"""videorun.run(), pinned run by run (CPU), sync loop and stream loop: every set_pipelined / reset / synchronize, every upload and
the file frames it carries, every ops.* call with its shapes, every forward_group call (windows, is_first_frame, a digest of both
window tensors), every event, every staging buffer given back and every sink take / put; then the frame count, the bytes written, the
score file, the fields a run leaves in its config and EVAL, and for a refused run the exception -- must equal the runs recorded from
the videorun.py that preceded its folding onto one options record, one plan and one group step (tests/golden/videorun_runs.json,
recorded with tests/videorun_trace.py; the commit is the file's first entry).  Exact, except the floats of the score lines (within
videorun_trace.REL).  And what tests/test_gpu_videorun_stream.py claims on the device holds here on the stub: for every case both
loops run, the same forward_group calls, the same bytes, the same score file."""
import os
import re

import pytest

import videorun_trace as vrt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'videorun_runs.json')


@pytest.fixture(scope='module')
def golden():
    g = vrt.load(GOLDEN)
    assert list(g)[0] == '_recorded_from' and re.fullmatch(r'[0-9a-f]{40}', g['_recorded_from']['commit'])
    del g['_recorded_from']
    return g


@pytest.fixture(scope='module')
def recorded():
    mp = pytest.MonkeyPatch()
    try:
        return vrt.record(mp.setattr)
    finally:
        mp.undo()


def test_every_scenario_is_recorded(golden, recorded):
    assert list(recorded) == list(golden) == list(vrt.scenarios())
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), 'evalrun_runs.json'))


@pytest.mark.parametrize('name', list(vrt.scenarios()))
def test_videorun_run(golden, recorded, name):
    vrt.same(recorded[name], golden[name], name)


def calls(sc, what='forward_group'):
    return [ln for ln in sc['seq'] if ln.startswith(what)]


@pytest.mark.parametrize('case, sync, stream', vrt.pairs(), ids=[p[0] for p in vrt.pairs()])
def test_the_stream_loop_runs_what_the_sync_loop_runs(recorded, case, sync, stream):
    a, b = recorded[sync], recorded[stream]
    want = vrt.scenarios()[sync]
    if want['raises']:
        assert a['raised'] is not None and b['raised'] is not None
        return
    assert calls(a) and calls(a) == calls(b)
    assert a['bytes'] is not None and a['bytes'] == b['bytes']
    assert a['score'] == b['score'] and a['left']['EVAL.scores'] == b['left']['EVAL.scores']
    assert a['frames'] == b['frames'] == want['data'].get('n', vrt.NA + vrt.NB)
    assert a['left']['EVAL.scene_cuts'] == b['left']['EVAL.scene_cuts']
    assert [a['left'][k] for k in vrt.FIELDS] == [b['left'][k] for k in vrt.FIELDS]


def test_recorded_runs_reach_every_branch(golden):
    """The cap of the recording: a recording that silently skipped a branch of a loop fails here -- and the invariants of the loops
    that a recording can state."""
    want = vrt.scenarios()
    for name, sc in golden.items():
        w = want[name]
        assert (sc['raised'] is not None) == w['raises'], name
        n = w['data'].get('n', vrt.NA + vrt.NB)
        assert ('EVAL.io_stats' in sc['left']) == (not w['raises'] or 'net raises' in name), name
        if w['io'] == 'sync':
            assert sc['left'].get('EVAL.io_stats', '<unset>') == '<unset>', name        # the sync run leaves no io_stats
            assert not any(ln.startswith(('event', 'give', 'sink', 'cuda.Stream')) for ln in sc['seq']), name
        if not w['raises']:
            assert sc['frames'] == n and sc['left']['net.pipelined'] is w['pipelined'], name
            assert sc['seq'][-2:] == (['cuda.synchronize', 'set_pipelined(False)'] if not w['pipelined'] else sc['seq'][-2:]), name
            assert w['pipelined'] == ('set_pipelined(False)' not in sc['seq']), name
            if w['io'] == 'stream':
                frames, uploads, groups, in_flight, held = sc['left']['EVAL.io_stats']
                depth = w['eval'].get('io_depth', 2)
                assert frames == n and uploads == 2 * n == len(calls(sc, 'upload')) and groups == len(calls(sc)), name
                assert in_flight <= depth and held <= w['t'] + (depth + 1) * vrt.G + 2, name
                assert sc['left']['outstanding'] == [0, 0, 0], name
                assert sorted(ln for ln in sc['seq'] if ln.startswith('give')) == sorted('give %s%d' % (s, i) for s in 'LR' for i in range(n)), name
                # every group in flight is retired before a reset: between a reset and the event records before it, as many waits
                rec = wait = 0
                for ln in sc['seq'][3:]:
                    rec, wait = rec + ln.endswith(' record'), wait + ln.endswith(' synchronize') * ln.startswith('event')
                    assert ln != 'reset' or rec == wait, name
                # a group's staging buffers go back behind the wait for its event, never before
                for i, ln in enumerate(sc['seq']):
                    assert not ln.startswith('give') or sc['seq'][i - 1].startswith('give') or re.fullmatch(r'event \d+ synchronize', sc['seq'][i - 1]), name
        if 'scene_cut' in w['eval'] and not w['raises']:
            assert sc['left']['EVAL.scene_cuts'] == [vrt.NA] and calls(sc, 'ops.luma_sad'), name
        if not w['eval'].get('in_down') and not w['eval'].get('out_size') and not w['raises']:
            assert not calls(sc, 'ops.resize_aa') and not calls(sc, 'ops.yuv_to_frames') and not calls(sc, 'ops.result_to_yuv'), name
        if 'scene_cut' not in w['eval']:
            assert not calls(sc, 'ops.luma_sad'), name
    for name in ('scene_cut with cuts', 'score_file without in_down', 'engines of the other kind', 'length mismatch', 'cuts beyond the end'):
        assert golden[name + ' [sync]']['seq'] == [], name
    for name in ('scene_cut with cuts', 'score_file without in_down', 'engines of the other kind'):
        assert golden[name + ' [stream]']['seq'] == [], name
    lines = [ln for sc in golden.values() for ln in sc['seq']]
    for what in ('set_pipelined(True)', 'set_pipelined(False)', 'reset', 'cuda.synchronize', 'cuda.Stream', 'stream synchronize', 'upload uint8[4, 3, 24, 24] L0,L0,L1',
                 'upload uint16[24, 24] L0', 'upload uint8[5, 24, 24] L4,L5,L6,L7,L8', 'ops.luma_sad B=4', 'ops.yuv_to_frames uint8[10, 96, 96]',
                 'ops.yuv_to_frames uint16[', 'ops.resize_aa B=10 float32[10, 3, 64, 96] -> 16x24 uint8', '-> 16x24 float32', '-> 32x48 float32 clamp=True',
                 'ops.score_frames B=4', 'ops.result_to_yuv B=4', 'ops.jpeg_encode B=4', 'ops.jpeg_encode_device B=4', 'i444 q=75', 'first=True', 'first=False',
                 'wins=[[0,0,0,0,0]]', 'wins=[[0,0,0,1,1],[0,0,1,1,1]]', 'event 0 record', 'event 3 synchronize', 'give L10', 'sink.take', 'sink.put length=',
                 'Y4MWriter 64x96 i422 ', 'Y4MWriter 64x96 i444p10 ', 'siting=left', ' full siting', 'MJPEGWriter'):
        assert any(what in ln for ln in lines), what
    stream_raise = golden['net raises in call 2 [stream]']
    assert stream_raise['seq'][-2:] == ['cuda.synchronize', 'set_pipelined(False)'] and stream_raise['left']['net.pipelined'] is False
    assert golden['net raises in call 2 [sync]']['seq'][-2:] == ['cuda.synchronize', 'set_pipelined(False)']
    # the range rule through build_config + main(): the files say full range
    for io_ in ('sync', 'stream'):
        assert golden['main range of the file [%s]' % io_]['header'].endswith('XCOLORRANGE=FULL')
        assert golden['main yuv_range limited [%s]' % io_]['header'].endswith('XCOLORRANGE=LIMITED')
        assert golden['main range of the file [%s]' % io_]['left']['input_yuv_range'] == 'full'
        assert golden['main yuv_range limited [%s]' % io_]['left']['input_yuv_range'] == 'limited'
    own = golden['own config mjpeg [sync]']['left']
    assert own['net.config'] == [own[k] for k in vrt.FIELDS]
