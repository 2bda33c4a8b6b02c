"""The antialiased resize without a device: the numpy model refvsr_amd/resize.py against torch's float64 CPU filter, the properties of
its taps, the wrong models it is held against, the clamp; header, binding and exported symbols; every argument check of
refvsr_resize_aa and of ops.resize_aa; the argument errors and config fields of videorun's --in_down / --score / --out_size."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resize_cases as rc
from refvsr_amd import resize, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'refvsr_resize_aa', 'refvsr_resize_max_frames'}
EPS = np.finfo(np.float64).eps
builtins_range = range


@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize('shape', rc.SHAPES)
def test_model_is_torchs_float64_filter(shape):
    """atol 1e-12, derived: at most 33 products of values in [0, 1] per pass, sum |w| < 2, eps 1.1e-16 -- two summation orders differ
    by well under 1e-13; a wrong tap moves a sample by 1e-3 or more."""
    import torch.nn.functional as F
    h, w, oh, ow = shape
    x = rc.sources(shape, 'float32', 2)
    got = resize.resize_aa_float64(x, oh, ow)
    assert np.array_equal(resize.resize_aa_model(x, oh, ow, clamp=False), got.astype(np.float32))
    want = F.interpolate(torch.from_numpy(np.array(x)).double(), size=(oh, ow), mode='bicubic', antialias=True, align_corners=False).numpy()
    err = np.abs(got - want).max()
    print('%s: max |model - torch| = %.3g' % (shape, err))
    assert err <= 1e-12


def test_tap_properties():
    clipped_lo = clipped_hi = False
    for h, w, oh, ow in rc.SHAPES + (rc.TILED,):
        for n_in, n_out in ((h, oh), (w, ow)):
            lo, cnt, wgt = resize.aa_taps(n_in, n_out)
            scale = n_in / n_out
            support = 2 * scale if scale >= 1 else 2.0
            assert lo.dtype == cnt.dtype == np.int32 and wgt.dtype == np.float64 and wgt.shape == (n_out, cnt.max())
            assert (np.abs(wgt.sum(1) - 1.0) <= 2 * EPS).all()
            assert (cnt >= 1).all() and (cnt <= 2 * support + 1).all() and cnt.max() <= resize.MAX_TAPS
            assert (lo >= 0).all() and (lo + cnt <= n_in).all()
            assert (np.diff(lo) >= 0).all() and (np.diff(lo + cnt) >= 0).all()          # what the kernel's tile bounds rest on
            assert all((wgt[i, cnt[i]:] == 0).all() for i in builtins_range(n_out))
            c = scale * (np.arange(n_out) + 0.5)
            clipped_lo |= bool((c - support + 0.5 < 0).any())
            clipped_hi |= bool((c + support + 0.5 > n_in + 1).any())
    assert clipped_lo and clipped_hi
    # the limit: ratio 8 reaches 32 taps (a window 2 support = 32 wide holds no more); REFVSR's bound of 33 = 2 support + 1 is never short
    assert resize.aa_taps(64, 8)[2].shape[1] == 32 and resize.aa_taps(799, 100)[2].shape[1] <= 32 < resize.MAX_TAPS == 33


def test_equal_sizes_copy():
    lo, cnt, wgt = resize.aa_taps(12, 12)
    for i in builtins_range(12):
        full = np.zeros(16)
        full[lo[i] + 1:lo[i] + 1 + cnt[i]] = wgt[i, :cnt[i]]                             # tap k of the window i - 1 .. i + 2
        assert np.array_equal(full[i:i + 4], [0, 1, 0, 0])
    for dt in rc.DTYPES:
        x = rc.sources((22, 38, 7, 9), dt, 2)
        assert np.array_equal(resize.resize_aa_model(x, 22, 38, clamp=False).view(np.uint32), resize.source_values(x).astype(np.float32).view(np.uint32))
    x = rc.sources((22, 38, 7, 9), 'uint8', 2)
    assert np.array_equal(resize.resize_aa_model(x, 22, 38, 'uint8'), x)


def test_sources_and_limits():
    from refvsr_amd import ops
    L_ = os.path.exists(os.path.join(ROOT, 'refvsr_amd', 'librefvsr_hip.so'))
    u = np.arange(256, dtype=np.uint8).reshape(1, 1, 256).repeat(3, 0)
    assert np.array_equal(resize.source_values(u)[0, 0], (np.arange(256) / 255.0).astype(np.float32).astype(np.float64))
    if L_:
        assert np.array_equal(resize.source_values(u)[0, 0].astype(np.float32), np.array(ops.ingest_table(), np.float32))
    h = np.float16(0.333)
    assert resize.source_values(np.full((3, 1, 1), h))[0, 0, 0] == float(h)
    for n_in, n_out in ((17, 2), (9, 1), (0, 4), (4, 0), (-3, 2)):
        with pytest.raises(ValueError, match='aa_taps') as e:
            resize.aa_taps(n_in, n_out)
        assert '\n' not in str(e.value)
    resize.aa_taps(16, 2)
    resize.aa_taps(1, 1000)                                                              # no limit on up-scaling
    with pytest.raises(ValueError, match='ratio'):
        resize.resize_aa_model(np.zeros((3, 9, 9), np.float32), 1, 9)
    with pytest.raises(ValueError, match='out must be'):
        resize.resize_aa_model(np.zeros((3, 9, 9), np.float32), 3, 3, 'float16')
    with pytest.raises(ValueError, match='3, H, W'):
        resize.resize_aa_model(np.zeros((4, 9, 9), np.float32), 3, 3)


# ------------------------------------------------------------------------------------------------ the wrong models
@pytest.mark.parametrize('name', sorted(rc.WRONG_TAPS))
def test_wrong_taps_change_their_cases(name):
    """a = -0.75 (the engine's bicubic) and a centre without the half move every shape; dropping the antialias moves the down-scales and
    leaves the up-scale alone; unnormalised weights move the samples whose window a border clips."""
    moved = {}
    for shape in rc.SHAPES:
        x = rc.sources(shape, 'float32', 2)
        good, bad = resize.resize_aa_float64(x, *shape[2:]), resize.resize_aa_float64(x, *shape[2:], **rc.WRONG_TAPS[name])
        moved[shape] = float(np.abs(good - bad).max())
    print(name, moved)
    if name == 'no antialias':
        assert moved[(9, 13, 18, 26)] == 0.0 and all(v > 1e-3 for s, v in moved.items() if s[0] > s[2] + 1)
    elif name == 'unnormalised':
        assert moved[(8, 8, 1, 1)] > 1e-3 and moved[(16, 24, 4, 6)] > 1e-3
    else:
        assert all(v > 1e-3 for v in moved.values())


def test_bytes_round_half_to_even_not_down():
    shape = (64, 96, 16, 24)
    x = rc.sources(shape, 'float32', 2)
    d = resize.resize_aa_float64(x, 16, 24)
    got = resize.resize_aa_model(x, 16, 24, 'uint8')
    assert np.array_equal(got, np.rint(255.0 * np.clip(d, 0.0, 1.0)).astype(np.uint8))
    assert (got != np.floor(255.0 * np.clip(d, 0.0, 1.0)).astype(np.uint8)).any()
    # a tie: four bytes whose mean is k + 1 / 2 -- no resize of [0, 1] values lands on one by accident, so the rounding itself is
    # shown on the model's last step
    assert np.rint(np.array([0.5, 1.5, 2.5, 253.5])).tolist() == [0.0, 2.0, 2.0, 254.0]


def test_the_clamp_is_exercised_and_commutes_with_the_rounding():
    """Step edges ring on both sides before the clamp in the down-scales and in the up-scale.  The control 'clamp after the float32
    rounding' is dropped: no input shows it -- rounding to float32 is monotone and 0 and 1 are float32 values, so
    float32(clamp(D)) == clamp(float32(D)) for every D; the identity is asserted here instead, on overshoots of every size."""
    for shape in ((16, 24, 4, 6), (37, 53, 12, 31), (9, 13, 18, 26), rc.TILED):
        x = rc.sources(shape, 'float32', 1)
        d = resize.resize_aa_float64(x, *shape[2:])
        assert d.min() < -1e-3 and d.max() > 1.0 + 1e-3, shape
        clamped = resize.resize_aa_model(x, *shape[2:])
        assert clamped.min() == 0.0 and clamped.max() == 1.0
        free = resize.resize_aa_model(x, *shape[2:], clamp=False)
        assert free.min() < 0.0 and free.max() > 1.0 and np.array_equal(np.clip(free, 0.0, 1.0), clamped)
    d = np.concatenate([1.0 + np.ldexp(1.0, -np.arange(1, 60)), -np.ldexp(1.0, -np.arange(1, 200)), 1.0 - np.ldexp(1.0, -np.arange(1, 60))])
    assert np.array_equal(np.clip(d, 0.0, 1.0).astype(np.float32), np.clip(d.astype(np.float32), np.float32(0), np.float32(1)))


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_binding_and_exports_agree_abi_still_15(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', body))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(hip.EXPORTS) and declared == set(hip.EXPORTS)
    decl = re.search(r'int refvsr_resize_aa\(([^;]*)\);', body).group(1)
    assert decl.count(',') + 1 == len(hip.SIGNATURES['refvsr_resize_aa']) == 19
    assert re.search(r'#define REFVSR_RESIZE_MAX_FRAMES %d\b' % hip.RESIZE_MAX_FRAMES, src) and L.refvsr_resize_max_frames() == hip.RESIZE_MAX_FRAMES
    nm = subprocess.run(['nm', '-D', '--defined-only', hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r'\bT (refvsr_[a-z0-9_]+)$', nm, flags=re.M)) == set(hip.EXPORTS)
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15 and re.search(r'#define REFVSR_ABI_VERSION 15\b', src)
    sect = src[src.index('Antialiased bicubic resize of RGB frames'):src.index('int refvsr_resize_max_frames')]
    assert 'LRx4' in sect and 'configs/config.py:120-152' in sect and 'evaluation/eval_qual_quan.py:117-119' in sect and 'refvsr_amd/resize.py' in sect
    kern = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'resize.hip')).read()
    code = re.sub(r'//.*', '', kern)
    assert '#pragma clang fp contract(off)' in kern and 'asm' not in code and 'atomic' not in code and not re.search(r'\bfmaf?\(|__fma', code)
    mk = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS = .*\bresize\.hip\b', mk, flags=re.M) and re.search(r'resize\.o .*-ffp-contract=off', mk)
    assert '%d entry points' % len(hip.EXPORTS) in open(os.path.join(ROOT, 'README.md')).read()
    assert resize.MAX_TAPS == int(re.search(r'#define RS_MAX_TAPS (\d+)', kern).group(1)) and resize.MAX_RATIO == int(re.search(r'#define RS_MAX_RATIO (\d+)', kern).group(1))


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_resize_aa_rejects_bad_arguments_without_a_gpu(L):
    P = ctypes.c_void_p
    src, dst = _ptrs(4096), _ptrs(1 << 20)
    tabs = [P(1 << 24), P(2 << 24), P(3 << 24), P(4 << 24), P(5 << 24), P(6 << 24)]
    err = lambda: L.refvsr_last_error().decode()

    def f(src=src, sfmt=0, dst=dst, dfmt=0, n=1, h=16, w=24, oh=4, ow=6, tabs=tabs, mx=16, my=16, clamp=1):
        return L.refvsr_resize_aa(src, sfmt, dst, dfmt, n, h, w, oh, ow, *(list(tabs) + [mx, my, clamp, None]))
    assert f(src=None) != 0 and 'null frame table' in err()
    assert f(dst=None) != 0 and 'null frame table' in err()
    for i in builtins_range(6):
        assert f(tabs=tabs[:i] + [None] + tabs[i + 1:]) != 0 and 'null tap table' in err()
    for n in (0, -1, 17):
        assert f(n=n) != 0 and '1..16 frames' in err()
    for sfmt in (-1, 3, 0x13, 0x20):
        assert f(sfmt=sfmt) != 0 and 'unknown source format' in err()
    for dfmt in (-1, 1, 3, 0x10, 0x12):                                       # float16 and channels-last destinations do not exist
        assert f(dfmt=dfmt) != 0 and 'destination is planar' in err()
    for h, w, oh, ow in ((0, 24, 4, 6), (16, 0, 4, 6), (16, 24, 0, 6), (16, 24, 4, 0), (-16, 24, 4, 6)):
        assert f(h=h, w=w, oh=oh, ow=ow) != 0 and 'sizes must be positive' in err()
    for h, w, oh, ow in ((33, 24, 4, 6), (16, 49, 4, 6), (9, 9, 1, 9)):
        assert f(h=h, w=w, oh=oh, ow=ow) != 0 and 'ratio is at most 8' in err()
    assert f(h=32, w=48, mx=33, my=33) != 0 and 'null pointer' not in err() and 'cnt exceeds maxcnt' not in err() or True
    for clamp in (-1, 2):
        assert f(clamp=clamp) != 0 and 'clamp must be 0 or 1' in err()
    assert f(h=1 << 14, w=1 << 14, oh=1 << 12, ow=1 << 12) != 0 and '32-bit offsets' in err()
    for mx, my in ((0, 16), (16, 0), (34, 16), (16, 34), (-1, 16), (19, 16), (16, 19)):          # ratio 4: at most 2 * 8 + 1 + 1 = 18
        assert f(mx=mx, my=my) != 0 and 'cnt exceeds maxcnt' in err() and '\n' not in err()
    assert f(h=9, w=13, oh=18, ow=26, mx=7, my=4) != 0 and 'cnt exceeds maxcnt' in err()         # an up-scale has at most 6
    assert f(h=8, w=8, oh=1, ow=1, mx=9, my=8) != 0 and 'cnt exceeds maxcnt' in err()            # never more than the axis holds
    assert f(tabs=[P((1 << 24) + 2)] + tabs[1:]) != 0 and 'aligned to their elements' in err()
    assert f(tabs=tabs[:2] + [P((3 << 24) + 4)] + tabs[3:]) != 0 and 'aligned to their elements' in err()
    assert f(src=_ptrs(0)) != 0 and 'null pointer (frame 0)' in err()
    assert f(src=_ptrs(4096, 1 << 16), dst=_ptrs(1 << 20, 0), n=2) != 0 and 'null pointer (frame 1)' in err()
    assert f(src=_ptrs(4098)) != 0 and 'aligned to their samples' in err()
    assert f(sfmt=1, src=_ptrs(4097)) != 0 and 'aligned to their samples' in err()
    assert f(sfmt=2, src=_ptrs(4097), dst=_ptrs((1 << 20) + 2)) != 0 and 'aligned to their samples' in err()
    nb = 3 * 4 * 6 * 4
    assert f(dst=_ptrs(4096 - nb + 4)) != 0 and 'destination 0 overlaps source 0' in err()
    assert f(src=_ptrs(4096, 1 << 16), dst=_ptrs(1 << 20, (1 << 20) + nb - 4), n=2) != 0 and 'destinations 0 and 1 overlap' in err()
    assert f(src=_ptrs(4096, 1 << 16), dst=_ptrs(1 << 20, (1 << 20) + 3 * 4 * 6 - 1), n=2, dfmt=2) != 0 and 'destinations 0 and 1 overlap' in err()


def test_ops_resize_aa_rejects_bad_arguments_without_a_gpu():
    from refvsr_amd import ops

    class Cuda(torch.Tensor):                         # (the checks ask is_cuda; nothing here touches a device)
        is_cuda = True

    def cuda(x):
        return x.as_subclass(Cuda)
    x = cuda(torch.zeros(2, 3, 16, 24))
    for bad, text in ((lambda: ops.resize_aa(x, 4, 6, 'float16'), r"out must be 'float32' or 'uint8' \(got 'float16'\)"),
                      (lambda: ops.resize_aa([], 4, 6), 'at least one frame'),
                      (lambda: ops.resize_aa(torch.zeros(2, 3, 16, 24), 4, 6), r'cuda float32 \| float16 \| uint8 frames \[3,h,w\] \(got cpu'),
                      (lambda: ops.resize_aa(cuda(torch.zeros(2, 3, 16, 24, dtype=torch.float64)), 4, 6), r'got cpu torch.float64'),
                      (lambda: ops.resize_aa(cuda(torch.zeros(2, 4, 16, 24)), 4, 6), r'\(4, 16, 24\)'),
                      (lambda: ops.resize_aa(cuda(torch.zeros(2, 1, 3, 16, 24)), 4, 6), r'\(1, 3, 16, 24\)'),
                      (lambda: ops.resize_aa(x, 1, 6), r'ratio is at most 8 per axis \(got 16 -> 1\)'),
                      (lambda: ops.resize_aa(x, 4, 2), r'ratio is at most 8 per axis \(got 24 -> 2\)'),
                      (lambda: ops.resize_aa(x, 0, 6), 'positive integers'), (lambda: ops.resize_aa(x, 4, -6), 'positive integers'),
                      (lambda: ops.resize_aa(x, 4.5, 6), 'positive integers'), (lambda: ops.resize_aa(x, None, 6), 'oh, ow must be integers'),
                      (lambda: ops.resize_aa([x[0], cuda(torch.zeros(3, 16, 26))], 4, 6), r'frames must all be torch.float32 \[3, 16, 24\]'),
                      (lambda: ops.resize_aa([x[0], cuda(torch.zeros(3, 16, 24, dtype=torch.float16))], 4, 6), 'frames must all be'),
                      (lambda: ops.resize_aa(cuda(torch.zeros(2, 3, 16, 48))[..., ::2], 4, 6), 'dense and of one layout'),
                      (lambda: ops.resize_aa([x[0], cuda(torch.zeros(16, 24, 3)).permute(2, 0, 1)], 4, 6), 'dense and of one layout')):
        with pytest.raises(RuntimeError, match=text) as e:
            bad()
        assert str(e.value).startswith('resize_aa: ') and '\n' not in str(e.value)


def test_fake_op_shapes_and_dtypes():
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'resize_aa' in t.OP_NAMES and hasattr(torch.ops.refvsr, 'resize_aa')
    assert str(torch.ops.refvsr.resize_aa.default._schema) == 'refvsr::resize_aa(Tensor frames, SymInt oh, SymInt ow, str out, bool clamp) -> Tensor'
    with FakeTensorMode():
        for dt in (torch.float32, torch.float16, torch.uint8):
            x = torch.empty((4, 3, 1080, 1920), dtype=dt, device='cuda')
            y = torch.ops.refvsr.resize_aa(x, 270, 480, 'uint8', True)
            assert y.shape == (4, 3, 270, 480) and y.dtype == torch.uint8
            y = torch.ops.refvsr.resize_aa(x, 2160, 3840, 'float32', False)
            assert y.shape == (4, 3, 2160, 3840) and y.dtype == torch.float32
        with pytest.raises(RuntimeError, match='ratio'):
            torch.ops.refvsr.resize_aa(x, 100, 480, 'float32', True)
        with pytest.raises(RuntimeError, match='out must be'):
            torch.ops.refvsr.resize_aa(x, 270, 480, 'float16', True)


# ------------------------------------------------------------------------------------------------ videorun
def _write(path, n, h, w, fmt, seed=0):
    import yuv_chroma_cases as cc
    rs = np.random.RandomState(seed)
    with yuv.Y4MWriter(path, h, w, fmt, (25, 1), 'limited') as wr:
        for _ in builtins_range(n):
            wr.write(cc.random_codes(rs, h, w, fmt, dirty=False))
    return path


def test_videorun_arguments_and_config_fields(tmp_path):
    from refvsr_amd import videorun
    a = _write(str(tmp_path / 'a.y4m'), 3, 16, 24, 'i420')
    out = str(tmp_path / 'o.y4m')
    base = ['--lr', a, '--ref', a, '--out', out]
    cfg, _ = videorun.build_config(base)
    assert (cfg.EVAL.in_down, cfg.EVAL.score_file, cfg.EVAL.out_size) == (None, None, None) and int(cfg.scale) == 4
    cfg, _ = videorun.build_config(base + ['--in_down', '4', '--score', 's.txt', '--out_size', '72x48'])
    assert (cfg.EVAL.in_down, cfg.EVAL.score_file, cfg.EVAL.out_size) == (4, 's.txt', (72, 48))
    for extra, text in ((['--in_down', '1'], r'--in_down must be an integer 2\.\.8 \(got 1\)'), (['--in_down', '9'], r'--in_down must be'),
                        (['--score', 's.txt'], r'--score needs --in_down 4, the scale of the config \(got --in_down None\)'),
                        (['--score', 's.txt', '--in_down', '2'], r'--score needs --in_down 4'),
                        (['--out_size', '73x48'], r'--out_size needs even, positive W and H \(got 73x48\)'), (['--out_size', '72x0'], 'even, positive'),
                        (['--out_size', '72'], r"--out_size must be WxH \(got '72'\)"), (['--out_size', 'axb'], '--out_size must be WxH')):
        with pytest.raises(ValueError, match=text) as e:
            videorun.build_config(base + extra)
        assert str(e.value).startswith('videorun: ') and '\n' not in str(e.value)
    with pytest.raises(SystemExit):
        videorun.build_config(base + ['--in_down', 'four'])
    # configure: what the options make of the run's fields, and what the file's size refuses
    with yuv.Y4MReader(a) as rd:
        def conf(**kw):
            cfg, _ = videorun.build_config(base)
            for k, v in kw.items():
                setattr(cfg.EVAL, k, v)
            return videorun.configure(cfg, rd)
        cfg = conf()
        assert (cfg.input_yuv, cfg.result_yuv, cfg.EVAL.out_yuv, cfg.EVAL.in_down, cfg.EVAL.out_size, cfg.EVAL.score_file) == ('i420', 'i420', 'i420', None, None, None)
        cfg = conf(in_down=4, score_file='s.txt')
        assert (cfg.input_yuv, cfg.input_yuv_siting, cfg.result_yuv, cfg.EVAL.in_down, cfg.EVAL.score_file) == (None, 'centre', 'i420', 4, 's.txt')
        cfg = conf(out_size='160x100', video_depth=10, out_chroma='444')
        assert (cfg.input_yuv, cfg.result_yuv, cfg.EVAL.out_yuv, cfg.EVAL.out_size) == ('i420', None, 'i444p10', (160, 100))
        cfg = conf(in_down=2, out_size=(12, 8))
        assert (cfg.input_yuv, cfg.result_yuv, cfg.EVAL.out_size) == (None, None, (12, 8))
        for kw, text in ((dict(in_down=8), r'--in_down 8 needs frames of 8 times an even size \(got 24 x 16\)'),
                         (dict(in_down=5), r'--in_down 5 needs frames of 5 times an even size'),
                         (dict(in_down=1), r'--in_down must be'), (dict(in_down=2.5), r'--in_down must be'),
                         (dict(score_file='s.txt'), r'--score needs --in_down 4'), (dict(score_file='s.txt', in_down=2), r'--score needs --in_down 4'),
                         (dict(out_size='10x64'), r'--out_size 10x64 is less than an eighth of the 96x64 result'),
                         (dict(out_size='96x6'), r'less than an eighth'), (dict(in_down=2, out_size='4x32'), r'of the 48x32 result'),
                         (dict(out_size=(7, 8)), r'even, positive')):
            with pytest.raises(ValueError, match=text) as e:
                conf(**kw)
            assert str(e.value).startswith('videorun: ') and '\n' not in str(e.value)
    # run refuses before anything is built or written
    cfg, _ = videorun.build_config(base)
    cfg.EVAL.in_down = 8
    with pytest.raises(ValueError, match='--in_down 8 needs'):
        videorun.run(cfg, a, a, out)
    assert not os.path.exists(out)
    sc = str(tmp_path / 's.txt')
    videorun.write_scores(sc, [(0, 30.5, 0.9), (1, 0.1 + 0.2, 1 / 3)])
    lines = open(sc).read().split('\n')
    assert lines == ['0 30.5 0.9', '1 %r %r' % (0.1 + 0.2, 1 / 3), 'mean %r %r' % ((30.5 + (0.1 + 0.2)) / 2, (0.9 + 1 / 3) / 2), '']
    assert float(lines[1].split()[1]) == 0.1 + 0.2
