"""evalrun.evaluate(), pinned run by run (CPU): the network entry every frame takes and its arguments, every reset / set_pipelined /
synchronize, every scorer and colour launch with its batch, the score file's text, the log lines, the output tree (decoded pixels of
every PNG, bytes of every Y4M file) and the returned dict -- for qual_quan, quan_FOV and quan_conf_map, host and device metrics,
-qualitative_only / -quantitative_only, --frame_group, --video_out, --input_dtype uint8, --vid_name, a net that is already pipelined and a
net that fails mid-run -- must equal the runs recorded from the evaluate() that preceded its rebuild on one run object
(tests/golden/evalrun_runs.json, recorded with tests/evalrun_trace.py; the commit is the file's first entry).  Exact, except the
per-frame seconds (masked) and numbers printed with five decimals / returned floats (within evalrun_trace.TOL)."""
import os
import re

import pytest

import evalrun_trace as ert

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evalrun_runs.json')


@pytest.fixture(scope='module')
def golden():
    g = ert.load(GOLDEN)
    assert list(g)[0] == '_recorded_from' and re.fullmatch(r'[0-9a-f]{40}', g['_recorded_from']['commit'])
    del g['_recorded_from']
    return g


@pytest.fixture(scope='module')
def recorded():
    mp = pytest.MonkeyPatch()
    try:
        return ert.record(mp.setattr)
    finally:
        mp.undo()


def test_every_scenario_is_recorded(golden, recorded):
    assert list(recorded) == list(golden) == list(ert.scenarios())


@pytest.mark.parametrize('name', list(ert.scenarios()))
def test_evalrun_run(golden, recorded, name):
    ert.same(recorded[name], golden[name], name)


def test_groups_write_the_score_text_of_the_one_frame_loop(golden):
    ert.same(golden['qual_quan host group 3']['score'], golden['qual_quan host group 1']['score'], 'group 3 against group 1')


def test_a_failing_net_leaves_the_video_closed_and_the_net_as_it_was(golden):
    sc = golden['net raises on call 4 y4m group 2']
    assert sc['raised'] == 'RuntimeError: stub: network call 4 fails'
    assert sc['videos_closed'] == [['y4m/0001.y4m', 5, True, True]]            # (path, frames, closed, a whole number of frames on disk)
    assert sc['calls'][-2:] == ['sync', 'set_pipelined(False)'] and sc['net_after']['pipelined'] is False
    on = golden['net already pipelined group 2']
    assert on['calls'][0] == 'set_pipelined(True)' and 'set_pipelined(False)' not in on['calls'] and on['net_after']['pipelined'] is True


def test_recorded_runs_reach_every_branch(golden):
    """The cap of the recording: a recording that silently skipped a branch of the loop fails here."""
    want = ert.scenarios()
    for name, sc in golden.items():
        assert sc['frames'] == want[name]['frames'] and (sc['raised'] is not None) == want[name]['raises'], name
        assert want[name]['raises'] or (sc['res']['frames'] == sc['res']['n_seconds'] == sc['frames']), name
    lines = [ln for sc in golden.values() for ln in sc['score']]
    n, sec = r'\d+\.\d{5}', r'\(<sec>\)'
    shapes = {
        'frame line with scores': r'\[EVAL unit\|RealMCVSR\|\d{4}\]\[\d/2\]\[\d/5\] \d{4}\.png PSNR: %s SSIM: %s %s' % (n, n, sec),
        'frame line without scores': r'\[EVAL unit\|RealMCVSR\|\d{4}\]\[\d/2\]\[\d/5\] \d{4}\.png %s' % sec,
        'MEAN with scores': r'\[MEAN EVAL unit\|RealMCVSR\|\d{4}\]\[\d/2\] PSNR: %s SSIM: %s %s' % (n, n, sec),
        'MEAN without scores': r'\[MEAN EVAL unit\|RealMCVSR\|\d{4}\]\[\d/2\] %s' % sec,
        'MEAN of a FOV block': r'\[MEAN EVAL unit\|RealMCVSR\|\d{4}\]\[\d/2\] %s ' % sec,
        'TOTAL with scores': r'\[TOTAL seeded\|RealMCVSR\] PSNR: %s SSIM: %s %s' % (n, n, sec),
        'TOTAL without scores': r'\[TOTAL seeded\|RealMCVSR\] %s' % sec,
        'TOTAL of a FOV block': r'\[TOTAL seeded\|RealMCVSR\] ',
        'FOV block row': r'\[SSIM-FOV_ring\] \(50\.0-100\.0%%: %s, .*50\.0-50\.0%%: 0\.00000, \) %s' % (n, sec),
    }
    for what, pat in shapes.items():
        assert any(re.fullmatch(pat, ln) for ln in lines), what
    fov = golden['FOV host group 1']
    first = re.fullmatch(shapes['frame line with scores'], fov['score'][0])
    assert first and fov['res']['fov'][0][0][0] == [fov['res']['psnr'][0], fov['res']['ssim'][0]]        # (the line is the table's key-1 fi pair)
    calls = [c for sc in golden.values() for c in sc['calls']]
    for what in ('net(is_first=True', 'net(is_first=False', 'is_log=True', 'frame_ids=-)', 'forward_group(', 'is_first_frame=True, kwargs={"want_conf": true}',
                 'kwargs={})', 'score_frames B=1 ', 'score_frames B=3 ', 'score_regions B=2 ', 'conf_colormap B=4 ', 'conf_colormap B=8 ', 'down=4',
                 'lr=uint8', 'lrs=uint8', 'reset', 'set_pipelined(True)', 'set_pipelined(False)', 'sync'):
        assert any(what in c for c in calls), what
    assert any(int(m.group(1)) > 1 for m in (re.search(r'score_frames .*down=(\d)', c) for c in calls) if m)
    paths = [p for sc in golden.values() for p, _ in sc['tree']]
    assert any(p.endswith('.y4m') for p in paths)
    from refvsr_amd.evalrun import CONF_MAP_DIRS
    for folder in ['input', 'output'] + [d for d, _ in CONF_MAP_DIRS]:
        assert any(p.startswith('png/%s/' % folder) for p in paths) and any(p.startswith('jpg/%s/' % folder) for p in paths), folder
    assert golden['quantitative_only']['tree'] == [] and golden['FOV host group 1']['tree'] == []
