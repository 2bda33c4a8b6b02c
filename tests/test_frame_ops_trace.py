"""The frame-level wrappers of refvsr_amd.ops, pinned call by call (CPU): buffers_equal, bytes_equal, ingest_u8, ingest_frames,
score_frames, score_regions, result_to_yuv420, result_to_yuv, result_yuv, resize_aa, yuv420_ingest, yuv_ingest, yuv_decode,
yuv420_to_frames, yuv_to_frames, jpeg_encode_device, luma_sad, conf_colormap and param_fingerprint run on CPU memory against a
recording stand-in for the library (tests/frame_ops_trace.py).  For 1, MAX, MAX + 1 and 2 MAX + 3 frames, a tensor and a list, every
dtype and layout, every refusal and the three cache cases, the launches (names, scalars, pointer tables as tensor + byte offset, the
chunk walk, the workspaces), the returned tensors and the refusals (type and full message) must equal, byte for byte, what was recorded
from the ops.py that preceded the fold of these wrappers onto one frame check, one chunk walk and one cache
(tests/golden/frame_ops_calls.json; the commit is the file's first entry)."""
import os
import re

import pytest

import frame_ops_trace as trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'frame_ops_calls.json')


@pytest.fixture(scope='module')
def golden():
    return trace.load(GOLDEN)


@pytest.fixture(scope='module')
def recorded():
    return trace.record()


def test_substitutions_are_removed(recorded):
    import torch
    from refvsr_amd import hip, ops
    assert ops.torch is torch and hip.lib.__module__ == 'refvsr_amd.hip' and ops._stream.__module__ == 'refvsr_amd.ops'
    assert not any(k[0].type == 'cpu' for name in trace.CACHES for k in getattr(ops, name))


def test_the_file_is_reproduced_byte_for_byte(golden, recorded):
    src, cases, text = golden
    assert re.fullmatch(r'[0-9a-f]{40}', src['commit']) and src['file'] == 'refvsr_amd/ops.py'
    assert list(recorded) == list(cases) == list(trace.cases())
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert trace.dumps(recorded, src) == text


@pytest.mark.parametrize('case', list(trace.cases()))
def test_frame_op(golden, recorded, case):
    assert recorded[case] == golden[1][case]


def test_recorded_calls_reach_every_branch(golden):
    """What the recording must hold to pin anything: every launch, every chunk size, the offsets into the outputs, both layouts, the
    cache's three behaviours, and every refusal text of the frame section."""
    cases = golden[1]
    logs = [ln for v in cases.values() for r in v for ln in r['log']]
    raised = [r['raised'] for v in cases.values() for r in v if 'raised' in r]
    for fn in ('buffers_equal', 'bytes_equal', 'ingest_u8', 'score_frames', 'score_frames_down', 'score_regions', 'result_to_yuv420', 'result_to_yuv',
               'resize_aa', 'yuv420_to_rgb', 'yuv_to_rgb', 'jpeg_encode', 'luma_sad', 'conf_colormap', 'param_fingerprint'):
        assert any(ln.startswith('refvsr_%s(T' % fn) or ln.startswith('refvsr_%s(m' % fn) for ln in logs), fn
    for what in ('(T16[', '(T1[', '(T3[', '(T32[', 'm1+256, stream0)', 'm1+512, stream0)', ', 18, T16[', ', 17, T', 'm4+408, m4+128', 'm3+39872, 39872',
                 'stream1)', 'stream17)', ' = copy uint8', ' = from_numpy '):
        assert any(what in ln for ln in logs), what
    for what in ('at least 7 x 7', 'at most 2^29 pixels', '1 .. 2^31 - 1 samples', 'results must be dense', 'frames must be dense', 'frames must all be',
                 'at least one frame', 'as many results as ground truths', 'needs even h and w', 'down must be 1, 2 or 4', 'is not a 4:2:0 format',
                 'the down-scale ratio is at most', 'oh, ow must be integers', 'frames must lie on one GPU', 'every frame is one dense',
                 'as many frames on both sides', 'maps must be single', 'empty tensor list', 'contiguous float32 tensors of one GPU',
                 'ground-truth frames must be dense', 'rectangles are (y0, y1, x0, x1)', 'after the down-scale by 2'):
        if what == 'at most 2^29 pixels':                    # (needs a frame of 2^29 pixels: not recorded)
            continue
        assert any(what in r for r in raised), what
    # the same call twice builds one workspace; a second stream builds another; the first stream finds its own again
    twice = cases['score_frames cache: twice, a second stream, the first stream']
    assert [sum('workspace_bytes' in ln for ln in r['log']) for r in twice] == [1, 0, 1, 0]
    assert [[ln for ln in r['log'] if ln.startswith('refvsr_score_frames(')][0].split(', ')[-4] for r in twice] == ['m0+0', 'm0+0', 'm3+0', 'm0+0']
    # ... while the tap tables and the JPEG tables are shared between streams
    for name in ('resize_aa', 'jpeg_encode_device'):
        assert [sum(' = from_numpy ' in ln for ln in r['log']) > 0 for r in cases['%s cache: twice, a second stream, the first stream' % name]] == [True, False, False, False]
    # more than 16 entries: the 18th geometry empties the cache, so the first is built again and the 18th is still there
    for name in ('score_frames', 'score_regions', 'luma_sad', 'conf_colormap'):
        built = [sum('workspace_bytes' in ln for ln in r['log']) for r in cases['%s cache: 18 geometries and the first again' % name]]
        assert built == [1] * 18 + [1, 0], name
    for name in ('resize_aa', 'jpeg_encode_device'):
        built = [sum(' = from_numpy ' in ln for ln in r['log']) > 0 for r in cases['%s cache: 18 geometries and the first again' % name]]
        assert built == [True] * 18 + [True, False], name
    built = [sum('workspace_bytes' in ln for ln in r['log']) for r in cases['param_fingerprint table on 18 streams and the first again'] if r['call'] != 'table']
    assert built == [1] * 18 + [1]
