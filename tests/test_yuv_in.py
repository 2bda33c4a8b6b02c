"""Y'CbCr 4:2:0 input frames, host side: the numpy model refvsr_amd/yuv.py:yuv420_to_rgb (anchors, round trip, tap sum, tap and
clamp classes, wrong-model controls), the C-ABI of refvsr_yuv420_to_rgb without a device, the config fields, Y4MReader and the
argument errors of videorun.  No GPU needed."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import yuv_in_cases as yc
from refvsr_amd import yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'refvsr_yuv420_to_rgb', 'refvsr_yuv420_in_max_frames'}
builtins_range = range


@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def roundtrip_bound(fmt, matrix, range):
    """Half a luma code plus half a chroma code through the largest gain, plus the float32 rounding of a value in [0, 1]."""
    oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg = yuv.decode_coefficients(fmt, matrix, range)
    return 0.5 * iy + max(cr_r, cb_b) * 0.5 * ic + 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize('fmt', yc.FORMATS)
def test_anchors(fmt):
    """The five published code triples under BT.709 limited: black and white exactly, the primaries within the round-trip bound (the
    table's figures have six significant digits)."""
    s = 2 ** (yuv.depth_of(fmt) - 8)
    bound = roundtrip_bound(fmt, 'bt709', 'limited')
    for code, want in yc.ANCHORS:
        got = yuv.yuv420_to_rgb(yc.constant_frame([c * s for c in code], fmt), 4, 4, fmt)
        assert got.dtype == np.float32 and got.shape == (3, 4, 4) and (got == got[:, :1, :1]).all()
        px = got[:, 0, 0].astype(np.float64)
        print(fmt, code, px)
        if code in ((16, 128, 128), (235, 128, 128)):
            assert px.tolist() == list(want)
        else:
            assert np.abs(px - np.array(want)).max() <= bound
            assert np.abs(px - np.array(want)).max() <= 5e-7 * 2          # and it IS the table's row, to its printed digits


def test_coefficients_are_the_reciprocals_of_the_way_out():
    for fmt, matrix, range in itertools.product(yc.FORMATS, yuv.MATRICES, yuv.RANGES):
        kr, kg, kb, icb, icr, oy, sy, oc, sc = yuv.coefficients(fmt, matrix, range)
        assert yuv.decode_coefficients(fmt, matrix, range) == (oy, 1.0 / sy, oc, 1.0 / sc, 2.0 * (1.0 - kr), 2.0 * (1.0 - kb), kr, kb, 1.0 / kg)
    for bad in (('yv12', 'bt709', 'limited'), ('nv12', 'bt2020', 'limited'), ('nv12', 'bt709', 'pc')):
        with pytest.raises(ValueError):
            yuv.decode_coefficients(*bad)
    with pytest.raises(ValueError, match='chroma'):
        yuv.yuv420_to_rgb(yc.constant_frame((16, 128, 128), 'nv12'), 4, 4, 'nv12', chroma='bicubic')


@pytest.mark.parametrize('fmt', yc.FORMATS)
def test_round_trip_of_constant_colours(fmt):
    """yuv420_to_rgb(rgb_to_yuv420(x)) on constant-colour 4 x 4 frames, every matrix and range: within half a luma code plus half a
    chroma code through the largest gain (1.64 codes of full scale for BT.709 limited)."""
    rs = np.random.RandomState(11)
    colours = np.concatenate([rs.rand(40, 3), np.array(list(itertools.product((0.0, 0.5, 1.0), repeat=3)))]).astype(np.float32)
    for matrix, range in itertools.product(yuv.MATRICES, yuv.RANGES):
        bound = roundtrip_bound(fmt, matrix, range)
        x = np.broadcast_to(colours[:, :, None, None], (len(colours), 3, 4, 4))
        back = yuv.yuv420_to_rgb(yuv.rgb_to_yuv420(x, fmt, matrix, range), 4, 4, fmt, matrix, range)
        err = np.abs(back.astype(np.float64) - x.astype(np.float64)).max()
        print(fmt, matrix, range, 'max error %.6g, bound %.6g (%.3f codes of full scale)' % (err, bound, bound * (2 ** yuv.depth_of(fmt) - 1)))
        assert err <= bound
    assert abs(roundtrip_bound('nv12', 'bt709', 'limited') * 255 - 1.64) < 0.005


@pytest.mark.parametrize('fmt', yc.FORMATS)
def test_tap_sum_is_exact_in_integers_and_in_float64(fmt):
    """m = (9 a + 3 b + 3 c + d) / 16: the integer evaluation (yuv.chroma_taps, and pixel by pixel yc.taps_int) and a float64
    evaluation term by term, in two orders, agree on every case."""
    for name, _, h, w, buf in yc.cases(fmt):
        for c in yuv.codes(buf, h, w, fmt)[1:]:
            ti = yuv.chroma_taps(c)
            assert ti.dtype == np.int64 and ti.max() < 2 ** 15 and np.array_equal(ti, yc.taps_int(c)), name
            y, x = np.mgrid[0:h, 0:w]
            cy, cx = y >> 1, x >> 1
            cy2 = np.clip(cy + np.where(y & 1, 1, -1), 0, h // 2 - 1)
            cx2 = np.clip(cx + np.where(x & 1, 1, -1), 0, w // 2 - 1)
            f = c.astype(np.float64)
            a, b, d, e = f[cy, cx] * 0.5625, f[cy2, cx] * 0.1875, f[cy, cx2] * 0.1875, f[cy2, cx2] * 0.0625
            assert np.array_equal(((a + b) + d) + e, ti * 0.0625) and np.array_equal(a + ((e + d) + b), ti * 0.0625), name
            assert np.array_equal(yuv.chroma_taps(c, 'nearest'), 16 * c[cy, cx])


@pytest.mark.parametrize('fmt', yc.FORMATS)
def test_case_sets_populate_every_class(fmt):
    cs = yc.cases(fmt)
    names = [c[0] for c in cs]
    assert {'random', 'ingamut', 'allcodes', 'tiny'} <= set(names)
    assert ('dirty_low' in names) == (fmt == 'p010') and ('dirty_high' in names) == (fmt == 'i420p10')
    taps = {}
    for c in cs:
        for k, v in yc.tap_classes(c[2], c[3]).items():
            taps[k] = taps.get(k, 0) + v
    assert set(taps) == {'corner', 'top', 'bottom', 'left', 'right', 'interior', 'parity00', 'parity01', 'parity10', 'parity11'}
    assert all(v > 0 for v in taps.values()), taps
    assert yc.tap_classes(2, 2) == dict(corner=4, top=0, bottom=0, left=0, right=0, interior=0, parity00=1, parity01=1, parity10=1, parity11=1)
    cl = {}
    for c in cs:
        for k, v in yc.clamp_classes(c).items():
            cl[k] = cl.get(k, 0) + v
    assert all(cl[k] > 0 for k in ('below', 'inside', 'above')), cl
    g = yc.clamp_classes(yc.case(fmt, 'ingamut'))
    assert (g['below'] + g['above']) < 0.05 * sum(g.values()), g
    r = yc.clamp_classes(yc.case(fmt, 'random'))
    assert r['below'] > 0 and r['above'] > 0
    # every code of every plane
    _, _, h, w, buf = yc.case(fmt, 'allcodes')
    n = 2 ** yuv.depth_of(fmt)
    for p in yuv.codes(buf, h, w, fmt):
        assert np.array_equal(np.unique(p), np.arange(n))
    # the dirty bits are there, and are ignored
    if fmt == 'p010':
        _, _, h, w, buf = yc.case(fmt, 'dirty_low')
        assert (buf & 63).any() and np.array_equal(yuv.yuv420_to_rgb(buf, h, w, fmt), yuv.yuv420_to_rgb(buf & 0xFFC0, h, w, fmt))
    if fmt == 'i420p10':
        _, _, h, w, buf = yc.case(fmt, 'dirty_high')
        assert (buf >> 10).any() and np.array_equal(yuv.yuv420_to_rgb(buf, h, w, fmt), yuv.yuv420_to_rgb(buf & 1023, h, w, fmt))


@pytest.mark.parametrize('fmt', yc.FORMATS)
def test_model_is_the_written_out_arithmetic_and_controls_differ(fmt):
    """The vectorised model equals the pixel-by-pixel restatement on every case; every wrong model changes at least one sample of
    the case built for it."""
    coef = yuv.decode_coefficients(fmt)
    for name, _, h, w, buf in yc.cases(fmt):
        if h * w <= 1024:
            want = yc.decode(yuv.codes(buf, h, w, fmt), coef)
            assert np.array_equal(yuv.yuv420_to_rgb(buf, h, w, fmt).view(np.uint32), want.view(np.uint32)), name
    ctl = yc.controls(fmt)
    assert {'nearest', 'cosited', 'swapped', 'matrix', 'range', 'noclamp', 'float32', 'wrapped', 'layout'} <= set(ctl)
    assert ('noshift' in ctl) == (fmt == 'p010')
    for name, (c, wrong) in ctl.items():
        good = yuv.yuv420_to_rgb(c[4], c[2], c[3], fmt)
        n = int((good.view(np.uint32) != wrong.view(np.uint32)).sum())
        print(fmt, name, '%d of %d samples differ' % (n, good.size))
        assert wrong.shape == good.shape and n >= 1, name


def test_batches_and_refusals():
    b = np.stack([yc.case('nv12', 'random')[4]] * 3)
    out = yuv.yuv420_to_rgb(b, 6, 10, 'nv12')
    assert out.shape == (3, 3, 6, 10) and np.array_equal(out[2], yuv.yuv420_to_rgb(b[0], 6, 10, 'nv12'))
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(b[0], 6, 8, 'nv12')
    with pytest.raises(TypeError):
        yuv.yuv420_to_rgb(b[0], 6, 10, 'p010')


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_binding_and_exports_agree_abi_still_15(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_YUV420_IN_MAX_FRAMES (\d+)', src)
    assert m and int(m.group(1)) == hip.YUV420_IN_MAX_FRAMES == L.refvsr_yuv420_in_max_frames() == hip.INGEST_MAX_FRAMES == 16
    assert re.search(r'REFVSR_YUV_CHROMA_BILINEAR = 0, REFVSR_YUV_CHROMA_NEAREST = 1', src)
    assert (hip.YUV_CHROMA_BILINEAR, hip.YUV_CHROMA_NEAREST) == (0, 1) == (yuv.CHROMA_MODES['bilinear'], yuv.CHROMA_MODES['nearest'])
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', body))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(hip.EXPORTS) and declared == set(hip.EXPORTS)
    decl = re.search(r'int refvsr_yuv420_to_rgb\(([^;]*)\);', body).group(1)
    assert decl.count(',') + 1 == len(hip.SIGNATURES['refvsr_yuv420_to_rgb']) == 9
    nm = subprocess.run(['nm', '-D', '--defined-only', hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NEW_SYMBOLS <= set(re.findall(r'\bT (refvsr_[a-z0-9_]+)$', nm, flags=re.M))
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15 and re.search(r'#define REFVSR_ABI_VERSION 15\b', src)
    sect = src[src.index("Y'CbCr 4:2:0 input frames"):src.index('int refvsr_yuv420_in_max_frames(void);')]
    assert 'data_loader/utils.py:12-41' in sect and 'refvsr_amd/yuv.py' in sect
    kern = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'yuv_in.hip')).read()
    assert '#pragma clang fp contract(off)' in kern and 'asm' not in re.sub(r'//.*', '', kern)


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_kernel_entry_rejects_bad_arguments_without_a_gpu(L):
    src, dst = _ptrs(4096), _ptrs(8192)
    coef = (ctypes.c_double * 9)(*yuv.decode_coefficients('nv12'))
    err = lambda: L.refvsr_last_error().decode()
    f = L.refvsr_yuv420_to_rgb
    assert f(None, dst, 1, 8, 8, 0, 0, coef, None) != 0 and 'null frame table' in err()
    assert f(src, None, 1, 8, 8, 0, 0, coef, None) != 0 and 'null frame table' in err()
    assert f(_ptrs(0), dst, 1, 8, 8, 0, 0, coef, None) != 0 and 'null pointer (frame 0)' in err()
    assert f(src, _ptrs(0), 1, 8, 8, 0, 0, coef, None) != 0 and 'null pointer (frame 0)' in err()
    assert f(_ptrs(4096, 0), _ptrs(8192, 16384), 2, 8, 8, 0, 0, coef, None) != 0 and 'null pointer (frame 1)' in err()
    for n in (0, -1, 17):
        assert f(src, dst, n, 8, 8, 0, 0, coef, None) != 0 and '1..16 frames' in err()
    for h, w in ((7, 8), (8, 9), (0, 8), (8, 0), (1, 1), (-2, 8)):
        assert f(src, dst, 1, h, w, 0, 0, coef, None) != 0 and 'even and positive' in err()
    assert f(src, dst, 1, 1 << 15, 1 << 15, 0, 0, coef, None) != 0 and '2^29' in err()
    for fmt in (-1, 4, 9):
        assert f(src, dst, 1, 8, 8, fmt, 0, coef, None) != 0 and 'unknown yuv format' in err()
    for mode in (-1, 2):
        assert f(src, dst, 1, 8, 8, 0, mode, coef, None) != 0 and 'chroma' in err()
    assert f(src, dst, 1, 8, 8, 0, 0, None, None) != 0 and 'null coefficients' in err()
    for d in (8196, 8200, 8193):
        assert f(src, _ptrs(d), 1, 8, 8, 0, 0, coef, None) != 0 and '16 bytes' in err()
    for fmt in (2, 3):
        assert f(_ptrs(4097), dst, 1, 8, 8, fmt, 0, coef, None) != 0 and 'aligned to its samples' in err()


# ------------------------------------------------------------------------------------------------ host side
def test_config_fields_are_validated_while_the_feature_is_off():
    from refvsr_amd import get_config
    from refvsr_amd.model import _input_yuv
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    assert (cfg.input_yuv, cfg.input_yuv_matrix, cfg.input_yuv_range, cfg.input_yuv_chroma) == (None, 'bt709', 'limited', 'bilinear')
    assert _input_yuv(cfg) is None and yuv.resolve_input(None) is None
    assert yuv.resolve_input('p010', 'bt601', 'full', 'nearest') == ('p010', 'bt601', 'full', 'nearest')
    assert yuv.resolve_input('nv12') == ('nv12', 'bt709', 'limited', 'bilinear')
    for kw in ({'matrix': 'bt2020'}, {'range': 'pc'}, {'chroma': 'bicubic'}):
        with pytest.raises(ValueError):
            yuv.resolve_input(None, **kw)
    with pytest.raises(ValueError, match='input_yuv must be None'):
        yuv.resolve_input('yv12')
    for field, bad in (('input_yuv', 'yv12'), ('input_yuv_matrix', 'bt2020'), ('input_yuv_range', 'pc'), ('input_yuv_chroma', 'bicubic')):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        setattr(cfg, field, bad)
        with pytest.raises(ValueError):
            _input_yuv(cfg)


def test_model_input_contract_on_the_host():
    """Under input_yuv the entry check refuses a 5-D RGB window, a wrong dtype, odd 3h/2 geometry and a non-contiguous window, with
    one line naming the expected shape and dtype; without it a YUV-shaped window is refused."""
    from refvsr_amd import ops
    from refvsr_amd.model import _inputs

    class Cuda(torch.Tensor):                         # (the check asks is_cuda; nothing here touches a device)
        is_cuda = True

    def cuda(x):
        return x.as_subclass(Cuda)
    good = cuda(torch.zeros(1, 3, 27, 26, dtype=torch.uint8))
    lr, rf = _inputs(good, good, 'forward', strict=True, input_yuv='nv12')
    assert lr is good and rf is good
    g16 = cuda(torch.zeros(1, 3, 27, 26, dtype=torch.uint16))
    assert _inputs(g16, g16, 'forward', input_yuv='p010')[0] is g16
    for bad in (cuda(torch.zeros(1, 3, 3, 18, 26, dtype=torch.uint8)),            # an RGB window
                g16, cuda(torch.zeros(1, 3, 27, 26)),                                # wrong dtype
                cuda(torch.zeros(1, 3, 26, 26, dtype=torch.uint8)),                 # 3h/2 = 26: not a multiple of 3
                cuda(torch.zeros(1, 3, 27, 25, dtype=torch.uint8)),                 # odd w
                cuda(torch.zeros(1, 3, 27, 52, dtype=torch.uint8))[..., ::2],       # not contiguous
                torch.zeros(1, 3, 27, 26, dtype=torch.uint8)):                      # not on the device
        with pytest.raises(RuntimeError, match=r"input_yuv = 'nv12'.*torch.uint8 \[n, t, 3h/2, w\]"):
            _inputs(bad, bad, 'forward', input_yuv='nv12')
    with pytest.raises(RuntimeError, match='one shape'):
        _inputs(good, cuda(torch.zeros(1, 3, 30, 26, dtype=torch.uint8)), 'forward', input_yuv='nv12')
    for x in (good, g16):
        with pytest.raises(RuntimeError, match='need config.input_yuv'):
            _inputs(x, x, 'forward')
    assert ops.yuv_window_kind(torch.zeros(27, 26, dtype=torch.uint8), 'i420') == ('yuv', 'i420')
    assert ops.yuv_window_kind(torch.zeros(27, 26, dtype=torch.uint8), 'p010') is None
    assert ops.yuv_geometry(torch.zeros(5, 27, 26)) == (18, 26)


@pytest.mark.parametrize('fmt', ['i420', 'i420p10'])
def test_y4m_reader_against_writer_and_read_y4m(tmp_path, fmt):
    rs = np.random.RandomState(3)
    frames = [yc.random_codes(rs, 6, 10, fmt) for _ in builtins_range(3)]
    path = str(tmp_path / 'a.y4m')
    with yuv.Y4MWriter(path, 6, 10, fmt, (30000, 1001), 'full') as wr:
        for f in frames:
            wr.write(f)
    whole = yuv.read_y4m(path)
    with yuv.Y4MReader(path) as rd:
        assert (rd.h, rd.w, rd.fps, rd.fmt, rd.range) == (6, 10, (30000, 1001), fmt, 'full') == tuple(whole[k] for k in ('h', 'w', 'fps', 'fmt', 'range'))
        assert rd.length == 3 and rd.frames == 0
        got = list(rd)
        assert rd.frames == 3 and rd.read() is None
    assert len(got) == len(whole['frames']) == 3
    for a, b, c in zip(got, whole['frames'], frames):
        assert a.dtype == c.dtype and a.shape == (9, 10) and np.array_equal(a, c) and np.array_equal(b, c)
    # a truncated file: the whole frames are read, the cut one is reported
    data = open(path, 'rb').read()
    cut = str(tmp_path / 'cut.y4m')
    open(cut, 'wb').write(data[:-7])
    with yuv.Y4MReader(cut) as rd:
        assert rd.length == 2
        assert np.array_equal(rd.read(), frames[0]) and np.array_equal(rd.read(), frames[1])
        with pytest.raises(ValueError, match='truncated frame 2'):
            rd.read()
    with pytest.raises(ValueError, match='truncated frame 2'):
        yuv.read_y4m(cut)
    junk = str(tmp_path / 'junk.y4m')
    open(junk, 'wb').write(b'RIFF....\n')
    with pytest.raises(ValueError, match='not a YUV4MPEG2 file'):
        yuv.Y4MReader(junk)
    bad = str(tmp_path / 'bad.y4m')
    open(bad, 'wb').write(data[:data.index(b'\n') + 1] + b'FRAMX\n' + data[-20:])
    with yuv.Y4MReader(bad) as rd, pytest.raises(ValueError, match='FRAME marker'):
        rd.read()


def _write(path, n, h, w, fmt, range='limited', seed=0):
    rs = np.random.RandomState(seed)
    with yuv.Y4MWriter(path, h, w, fmt, (25, 1), range) as wr:
        for _ in builtins_range(n):
            wr.write(yc.random_codes(rs, h, w, fmt))
    return path


def test_videorun_argument_errors(tmp_path):
    from refvsr_amd import videorun
    a = _write(str(tmp_path / 'a.y4m'), 3, 16, 24, 'i420')
    base = ['--lr', a, '--ref', a, '--out', str(tmp_path / 'o.y4m')]
    cfg, args = videorun.build_config(base)
    assert (cfg.frame_num, cfg.EVAL.frame_group, cfg.EVAL.video_depth, cfg.input_yuv_chroma, cfg.EVAL.input_range_set) == (5, 4, None, 'bilinear', False)
    cfg, _ = videorun.build_config(base + ['--frame_num', '3', '--frame_group', '2', '--video_depth', '10', '--yuv_matrix', 'bt601',
                                           '--yuv_range', 'full', '--chroma', 'nearest'])
    assert (cfg.frame_num, cfg.center_idx, cfg.EVAL.frame_group, cfg.EVAL.video_depth) == (3, 1, 2, 10)
    assert (cfg.yuv_matrix, cfg.input_yuv_matrix, cfg.yuv_range, cfg.input_yuv_range, cfg.input_yuv_chroma) == ('bt601', 'bt601', 'full', 'full', 'nearest')
    for extra in (['--video_depth', '12'], ['--yuv_matrix', 'bt2020'], ['--yuv_range', 'pc'], ['--chroma', 'bicubic']):
        with pytest.raises(SystemExit):
            videorun.build_config(base + extra)
    with pytest.raises(SystemExit):
        videorun.build_config(['--lr', a, '--ref', a])
    for extra, text in ((['--frame_num', '4'], 'odd'), (['--frame_num', '1'], 'odd'), (['--frame_group', '0'], 'frame_group')):
        with pytest.raises(ValueError, match=text):
            videorun.build_config(base + extra)
    # the two files must agree, checked before anything is built or written
    for other, text in ((_write(str(tmp_path / 'g.y4m'), 3, 16, 26, 'i420'), 'geometry differs'),
                        (_write(str(tmp_path / 'f.y4m'), 3, 16, 24, 'i420p10'), 'format differs'),
                        (_write(str(tmp_path / 'n.y4m'), 4, 16, 24, 'i420'), r'frame count differs \(3 and 4\)')):
        with pytest.raises(ValueError, match=text):
            videorun.open_pair(a, other)
        with pytest.raises(ValueError, match=text):
            videorun.run(cfg, a, other, str(tmp_path / 'o.y4m'))
    assert not os.path.exists(str(tmp_path / 'o.y4m'))
    lr, ref = videorun.open_pair(a, a)
    cfg, _ = videorun.build_config(base)
    videorun.configure(cfg, lr)
    assert (cfg.input_yuv, cfg.input_yuv_range, cfg.result_yuv) == ('i420', 'limited', 'i420')
    lr.close()
    ref.close()
    full = _write(str(tmp_path / 'full.y4m'), 2, 16, 24, 'i420p10', range='full')
    with yuv.Y4MReader(full) as rd:
        cfg, _ = videorun.build_config(base)
        videorun.configure(cfg, rd)
        assert (cfg.input_yuv, cfg.input_yuv_range, cfg.result_yuv) == ('i420p10', 'full', 'i420p10')
        cfg, _ = videorun.build_config(base + ['--yuv_range', 'limited', '--video_depth', '8'])
        videorun.configure(cfg, rd)
        assert (cfg.input_yuv, cfg.input_yuv_range, cfg.result_yuv) == ('i420p10', 'limited', 'i420')


def test_fake_op_shape_and_dtype():
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'yuv420_to_rgb' in t.OP_NAMES and hasattr(torch.ops.refvsr, 'yuv420_to_rgb')
    assert str(torch.ops.refvsr.yuv420_to_rgb.default._schema) == \
        'refvsr::yuv420_to_rgb(Tensor x, SymInt h, SymInt w, str fmt, str matrix, str range, str chroma) -> Tensor'
    with FakeTensorMode():
        x = torch.empty((2, 5, 27, 26), dtype=torch.uint8, device='cuda')
        y = torch.ops.refvsr.yuv420_to_rgb(x, 18, 26, 'nv12', 'bt709', 'limited', 'bilinear')
        assert y.shape == (2, 5, 3, 18, 26) and y.dtype == torch.float32
        y = torch.ops.refvsr.yuv420_to_rgb(torch.empty((27, 26), dtype=torch.uint16, device='cuda'), 18, 26, 'p010', 'bt601', 'full', 'nearest')
        assert y.shape == (3, 18, 26) and y.dtype == torch.float32
        with pytest.raises(Exception):
            torch.ops.refvsr.yuv420_to_rgb(x, 18, 26, 'p010', 'bt709', 'limited', 'bilinear')
