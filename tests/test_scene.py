"""Scene cuts, host side: the numpy model refvsr_amd/yuv.py:luma_sad, the detector and the plan of refvsr_amd/scene.py (whole-file and
incremental forms), videorun's two options, and the C-ABI of refvsr_luma_sad without a device.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from refvsr_amd import scene, yuv
from refvsr_amd.synth import window_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'refvsr_luma_sad', 'refvsr_luma_sad_workspace_bytes', 'refvsr_scene_max_pairs'}


@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the model
def frame(fmt, y, h=2, w=4):
    """A frame of format fmt with the luma samples y (row-major list of h w raw samples) and arbitrary chroma samples."""
    buf = np.full(yuv.frame_shape(h, w), 77, dtype=yuv.dtype_of(fmt))
    buf[:h] = np.array(y, dtype=buf.dtype).reshape(h, w)
    return buf


@pytest.mark.parametrize('fmt', ['nv12', 'i420'])
def test_luma_sad_model_8_bit(fmt):
    a = frame(fmt, [0, 255, 10, 20, 30, 40, 50, 60])
    b = frame(fmt, [255, 0, 10, 25, 20, 40, 50, 61])
    assert yuv.luma_sad(a, b, 2, 4, fmt) == 255 + 255 + 0 + 5 + 10 + 0 + 0 + 1 == yuv.luma_sad(b, a, 2, 4, fmt)
    assert yuv.luma_sad(a, a, 2, 4, fmt) == 0 and isinstance(yuv.luma_sad(a, b, 2, 4, fmt), int)
    c = a.copy()
    c[2:] = 3                                                    # the chroma planes do not count
    assert yuv.luma_sad(a, c, 2, 4, fmt) == 0


def test_luma_sad_model_p010_ignores_the_low_six_bits():
    codes = [0, 1023, 512, 1, 2, 3, 4, 5]
    a = frame('p010', [c << 6 for c in codes])
    b = frame('p010', [(c << 6) | low for c, low in zip(codes, [63, 1, 32, 0, 17, 5, 62, 9])])
    assert yuv.luma_sad(a, b, 2, 4, 'p010') == 0
    # wrong-model control: a model that does not shift sees the low bits
    assert int(np.abs(a[:2].astype(np.int64) - b[:2].astype(np.int64)).sum()) == 63 + 1 + 32 + 0 + 17 + 5 + 62 + 9 != 0
    d = frame('p010', [((c + k) % 1024) << 6 for k, c in enumerate(codes)])
    assert yuv.luma_sad(a, d, 2, 4, 'p010') == 0 + (1023 - 0) + 2 + 3 + 4 + 5 + 6 + 7         # (1023 + 1 wraps to code 0)


def test_luma_sad_model_i420p10_ignores_the_bits_above_bit_9():
    codes = [0, 1023, 512, 1, 2, 3, 4, 5]
    a = frame('i420p10', codes)
    b = frame('i420p10', [c | (g << 10) for c, g in zip(codes, [63, 1, 32, 0, 17, 5, 62, 9])])
    assert yuv.luma_sad(a, b, 2, 4, 'i420p10') == 0
    assert int(np.abs(a[:2].astype(np.int64) - b[:2].astype(np.int64)).sum()) != 0           # (the unmasked model would not)
    d = frame('i420p10', [1023 - c for c in codes])
    assert yuv.luma_sad(b, d, 2, 4, 'i420p10') == 1023 + 1023 + 1 + 1021 + 1019 + 1017 + 1015 + 1013
    with pytest.raises(TypeError):
        yuv.luma_sad(a.astype(np.uint8), b, 2, 4, 'i420p10')


# ------------------------------------------------------------------------------------------------ the detector
def test_scores_single_spike_one_cut():
    h, w = 10, 20                                                # 200 pixels: a SAD of 200 m is a mean difference of m
    sads = [400, 400, 400, 8000, 400, 400]                       # mafd 2 2 2 40 2 2 for frames 1 .. 6
    s = scene.scene_scores(sads, h, w, 8)
    # frame 0: 0; frame 1: min(2, |2 - 0|); 2, 3: min(2, 0); 4: min(40, 38); 5: min(2, 38); 6: min(2, 0)
    assert s == [0.0, 0.02, 0.0, 0.0, 0.38, 0.02, 0.0]
    assert scene.cuts_from_scores(s, 0.1) == (4,)
    assert scene.cuts_from_scores(s, 0.38) == (4,) and scene.cuts_from_scores(s, 0.39) == ()          # (>= threshold)
    assert scene.cuts_from_scores(s, 0.02) == (1, 4, 5)
    assert scene.cuts_from_scores([1.0, 0.0], 0.5) == ()         # frame 0 is never listed: it always starts a scene


def test_scores_plateau_fires_once():
    h, w = 10, 20
    sads = [200, 6000, 6000, 6000, 6000, 200]                    # mafd 1 30 30 30 30 1
    s = scene.scene_scores(sads, h, w, 8)
    assert s == [0.0, 0.01, 0.29, 0.0, 0.0, 0.0, 0.01]           # the fall back (|1 - 30| = 29) is capped by mafd = 1
    assert scene.cuts_from_scores(s, 0.1) == (2,)


def test_scores_depth_and_clip():
    h, w = 10, 20
    s8 = scene.scene_scores([400, 8000, 400, 51000], h, w, 8)
    s10 = scene.scene_scores([1600, 32000, 1600, 204000], h, w, 10)      # the same picture in 10-bit codes: four times the SAD
    assert s8 == s10 == [0.0, 0.02, 0.38, 0.02, 1.0]                     # (255 - 2) / 100 is clipped to 1
    with pytest.raises(ValueError):
        scene.cuts_from_scores(s8, 0.0)
    with pytest.raises(ValueError):
        scene.cuts_from_scores(s8, 1.01)


def test_detector_frame_by_frame_equals_the_whole_file_form():
    rs = np.random.RandomState(5)
    sads = [int(v) for v in rs.randint(0, 255 * 200, 40)]
    det = scene.SceneDetector(10, 20, 8, 0.2)
    flags = [det.push(v) for v in sads]
    want = scene.scene_scores(sads, 10, 20, 8)
    assert det.scores == want and tuple(det.cuts) == scene.cuts_from_scores(want, 0.2) != ()
    assert [k + 1 for k, f in enumerate(flags) if f] == det.cuts


# ------------------------------------------------------------------------------------------------ the plan
def plain_plan(n, t, G):
    """The plan videorun.run's loop formed before there were cuts: its own three lines."""
    out = []
    for f0 in range(0, n, G):
        fs = list(range(f0, min(f0 + G, n)))
        wins = [window_indices(f, n, t) for f in fs]
        out.append((fs, wins, f0 == 0))
    return out


def incremental(n, t, G, cuts):
    """The plan of scene.GroupPlanner fed one frame at a time, never more than need() frames ahead."""
    p = scene.GroupPlanner(n, t, G)
    out = []
    while not p.done():
        while p.known < p.need():
            assert p.pop() is None                               # not before the frames its windows read are classified
            p.push(p.known in cuts)
        out.append(p.pop())
    assert p.pop() is None and tuple(p.cuts) == tuple(cuts)
    return out


@pytest.mark.parametrize('n, t, G', [(8, 3, 4), (11, 5, 4), (1, 3, 4), (5, 7, 2)])
def test_plan_without_cuts_is_the_plain_plan(n, t, G):
    assert scene.plan_groups(n, t, G, ()) == scene.plan_groups(n, t, G) == plain_plan(n, t, G) == incremental(n, t, G, ())
    assert scene.window_indices(n // 2, n, t) == window_indices(n // 2, n, t)


# a cut at a group boundary | in the middle of a group | two cuts one frame apart (a one-frame clip) | a cut at n - 1 | several
CUT_CASES = [(11, 3, 4, (4,)), (11, 3, 4, (8,)), (11, 3, 4, (5,)), (11, 5, 4, (6,)), (11, 3, 4, (5, 6)), (11, 5, 2, (1, 2)),
             (11, 3, 4, (10,)), (11, 7, 4, (10,)), (12, 5, 4, (3, 4, 9, 11)), (9, 3, 1, (2, 7)), (6, 3, 8, (3,)), (2, 3, 4, (1,))]


@pytest.mark.parametrize('n, t, G, cuts', CUT_CASES)
def test_plan_with_cuts(n, t, G, cuts):
    plan = scene.plan_groups(n, t, G, cuts)
    edges = (0,) + tuple(cuts) + (n,)
    assert scene.clips(n, cuts) == [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]
    clip_of = {f: (s, e) for s, e in scene.clips(n, cuts) for f in range(s, e)}
    assert [f for fs, _, _ in plan for f in fs] == list(range(n))              # every frame once, in order, file-global ids
    for fs, wins, first in plan:
        s, e = clip_of[fs[0]]
        assert 1 <= len(fs) <= G and all(clip_of[f] == (s, e) for f in fs), 'a group crosses a cut'
        assert first == (fs[0] == s)                                           # exactly each clip's first group
        assert len(wins) == len(fs)
        for f, win in zip(fs, wins):
            assert win == [s + i for i in window_indices(f - s, e - s, t)]     # the clip alone, plus its offset
            assert all(s <= i < e for i in win)
        assert not first or fs[0] in edges
    assert sum(first for _, _, first in plan) == len(cuts) + 1
    # every clip is cut into groups from its own first frame on
    for s, e in scene.clips(n, cuts):
        assert [fs for fs, _, _ in plan if s <= fs[0] < e] == [list(range(f0, min(f0 + G, e))) for f0 in range(s, e, G)]
    assert incremental(n, t, G, cuts) == plan


def test_plan_refuses_bad_cuts():
    for bad in ((0,), (8,), (9,), (3, 3), (5, 2), (-1,)):
        with pytest.raises(ValueError):
            scene.plan_groups(8, 3, 4, bad)
    p = scene.GroupPlanner(1, 3, 4)
    p.push(True)                                                 # (frame 0's answer is ignored)
    assert p.pop() == ([0], [[0, 0, 0]], True) and p.done() and p.cuts == []
    with pytest.raises(ValueError):
        p.push(False)


# ------------------------------------------------------------------------------------------------ videorun's options
def test_videorun_options(tmp_path):
    from refvsr_amd import get_config, videorun
    base = ['--lr', 'a.y4m', '--ref', 'b.y4m', '--out', 'c.y4m']
    cfg, _ = videorun.build_config(base)
    assert cfg.EVAL.scene_cut is None and cfg.EVAL.cuts is None
    cfg, _ = videorun.build_config(base + ['--scene_cut', '0.1'])
    assert cfg.EVAL.scene_cut == 0.1 and cfg.EVAL.cuts is None
    cfg, _ = videorun.build_config(base + ['--scene_cut', '1'])
    assert cfg.EVAL.scene_cut == 1.0
    cfg, _ = videorun.build_config(base + ['--cuts', '12,40, 41'])
    assert cfg.EVAL.cuts == (12, 40, 41) and cfg.EVAL.scene_cut is None
    with pytest.raises(ValueError, match='exclude each other'):
        videorun.build_config(base + ['--scene_cut', '0.1', '--cuts', '5'])
    for bad in (['--scene_cut', '0'], ['--scene_cut', '-0.1'], ['--scene_cut', '1.001'], ['--scene_cut', 'nan'], ['--cuts', '5,3'],
                ['--cuts', '4,4'], ['--cuts', '0,3'], ['--cuts', '-2'], ['--cuts', 'x']):
        with pytest.raises(ValueError, match='videorun: --scene_cut / --cuts'):
            videorun.build_config(base + bad)
    ap_help = subprocess.run([sys.executable, '-m', 'refvsr_amd.videorun', '--help'], cwd=ROOT, capture_output=True, text=True).stdout
    flat = ' '.join(ap_help.split())
    assert '--scene_cut' in flat and '--cuts' in flat and '0.1 is a customary starting point' in flat and 'nobody has tuned it' in flat
    # at run(), where the frame count is known: a cut at n or beyond, both fields at once, a bad threshold -- before any device work
    h, w, n = 4, 6, 5
    paths = [str(tmp_path / name) for name in ('uw.y4m', 'w.y4m')]
    for p in paths:
        with yuv.Y4MWriter(p, h, w, 'i420', (24, 1)) as wr:
            for _ in range(n):
                wr.write(np.zeros(yuv.frame_shape(h, w), dtype=np.uint8))
    out = str(tmp_path / 'sr.y4m')
    for field, bad, msg in (('cuts', (5,), r'cuts must lie in \(0, 5\)'), ('cuts', (2, 7), r'cuts must lie in \(0, 5\)'), ('cuts', (0,), 'cuts must lie'),
                            ('cuts', (3, 2), 'strictly increasing'), ('scene_cut', 0.0, r'scene_cut must lie in \(0, 1\]'),
                            ('scene_cut', 2, r'scene_cut must lie in \(0, 1\]')):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        setattr(cfg.EVAL, field, bad)
        with pytest.raises(ValueError, match=msg):
            videorun.run(cfg, paths[0], paths[1], out, net=object())
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.EVAL.scene_cut, cfg.EVAL.cuts = 0.1, (2,)
    with pytest.raises(ValueError, match='exclude each other'):
        videorun.run(cfg, paths[0], paths[1], out, net=object())
    assert not os.path.exists(out)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_binding_and_exports_agree_abi_still_15(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_SCENE_MAX_PAIRS (\d+)', src)
    assert m and int(m.group(1)) == hip.SCENE_MAX_PAIRS == L.refvsr_scene_max_pairs() == 16
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', body))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(hip.EXPORTS) and declared == set(hip.EXPORTS)
    decl = re.search(r'int refvsr_luma_sad\(([^;]*)\);', body).group(1)
    assert decl.count(',') + 1 == len(hip.SIGNATURES['refvsr_luma_sad']) == 10
    nm = subprocess.run(['nm', '-D', '--defined-only', hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r'\bT (refvsr_[a-z0-9_]+)$', nm, flags=re.M))
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15 and re.search(r'#define REFVSR_ABI_VERSION 15\b', src)
    sect = src[src.index('Scene cuts: luma SAD'):src.index('int refvsr_scene_max_pairs(void);')]
    assert 'data_loader/datasets.py:222-234' in sect and 'Replaces nothing in the reference' in sect and 'refvsr_amd/yuv.py:luma_sad' in sect
    kern = re.sub(r'//.*', '', open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'scene.hip')).read())
    assert 'asm' not in kern and 'atomic' not in kern and 'float' not in kern and 'double' not in kern


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_luma_sad_rejects_bad_arguments_without_a_gpu(L):
    a, b = _ptrs(4096), _ptrs(8192)
    ws, sad = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    err = lambda: L.refvsr_last_error().decode()
    f, need = L.refvsr_luma_sad, L.refvsr_luma_sad_workspace_bytes
    big = 1 << 24
    assert f(None, b, 1, 8, 8, 0, ws, big, sad, None) != 0 and 'null frame table' in err()
    assert f(a, None, 1, 8, 8, 0, ws, big, sad, None) != 0 and 'null frame table' in err()
    assert f(_ptrs(0), b, 1, 8, 8, 0, ws, big, sad, None) != 0 and 'null pointer (pair 0)' in err()
    assert f(a, _ptrs(0), 1, 8, 8, 0, ws, big, sad, None) != 0 and 'null pointer (pair 0)' in err()
    assert f(_ptrs(4096, 0), _ptrs(8192, 16384), 2, 8, 8, 0, ws, big, sad, None) != 0 and 'null pointer (pair 1)' in err()
    for n in (0, -1, 17):
        assert f(a, b, n, 8, 8, 0, ws, big, sad, None) != 0 and '1..16 pairs' in err()
        assert need(n, 8, 8) == 0
    for h, w in ((7, 8), (8, 9), (0, 8), (8, 0), (1, 1), (-2, 8)):
        assert f(a, b, 1, h, w, 0, ws, big, sad, None) != 0 and 'even and positive' in err()
        assert need(1, h, w) == 0
    assert f(a, b, 1, 1 << 15, 1 << 15, 0, ws, big, sad, None) != 0 and '2^29' in err()
    assert need(1, 1 << 15, 1 << 15) == 0 and need(1, 1 << 15, 1 << 14) > 0
    for fmt in (-1, 4, 9):
        assert f(a, b, 1, 8, 8, fmt, ws, big, sad, None) != 0 and 'unknown yuv format' in err()
    assert f(a, b, 1, 8, 8, 0, None, big, sad, None) != 0 and 'null workspace / sad' in err()
    assert f(a, b, 1, 8, 8, 0, ws, big, None, None) != 0 and 'null workspace / sad' in err()
    for off in (1, 4, 8):
        assert f(a, b, 1, 8, 8, 0, ctypes.c_void_p((1 << 20) + off), big, sad, None) != 0 and 'workspace must be 16-byte aligned' in err()
    for off in (1, 2, 4):
        assert f(a, b, 1, 8, 8, 0, ws, big, ctypes.c_void_p((1 << 21) + off), None) != 0 and 'sad must be 8-byte aligned' in err()
    n16 = need(16, 270, 480)
    assert n16 > 0 and n16 % 16 == 0 and need(1, 2, 2) == 16
    assert f(_ptrs(*[4096] * 16), _ptrs(*[8192] * 16), 16, 270, 480, 0, ws, n16 - 1, sad, None) != 0
    assert 'workspace too small (%d bytes, %d needed)' % (n16 - 1, n16) in err()
    assert f(a, b, 1, 8, 8, 0, ws, 0, sad, None) != 0 and 'workspace too small' in err()
    for fmt in (2, 3):
        assert f(_ptrs(4097), b, 1, 8, 8, fmt, ws, big, sad, None) != 0 and 'aligned to their samples (pair 0)' in err()
        assert f(a, _ptrs(8193), 1, 8, 8, fmt, ws, big, sad, None) != 0 and 'aligned to their samples (pair 0)' in err()
    # a chunk's 32-bit partial sum cannot overflow: its samples (two 16-byte groups per thread of 256, and the head and the tail)
    kern = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'scene.hip')).read()
    vpt, thr = int(re.search(r'#define SN_VPT (\d+)', kern).group(1)), int(re.search(r'#define SN_THREADS (\d+)', kern).group(1))
    assert (vpt * thr * 16 + 30) * 1023 < 2 ** 32
