"""Y'CbCr 4:2:0 result frames, the parts that need no GPU: the numpy model refvsr_amd/yuv.py (the specification of
refvsr_result_to_yuv420) against published codes, its ties and clamp, wrong-model controls, Y4M files, and the boundary -- header,
binding, library, argument checks, config validation, the CLI's options."""
import ctypes
import os
import re

import numpy as np
import pytest

import yuv_cases as yc
from refvsr_amd import yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ('nv12', 'i420', 'p010', 'i420p10')


def _codes(rgb, fmt, matrix, range):
    """(Y, Cb, Cr) of a solid 2 x 2 frame, the shift of p010 taken out."""
    y, cb, cr = yuv.planes(yuv.rgb_to_yuv420(yc.solid(rgb), fmt, matrix, range), 2, 2, fmt)
    sh = yuv.FORMATS[fmt][2]
    assert (y == y[0, 0]).all()
    return int(y[0, 0]) >> sh, int(cb[0, 0]) >> sh, int(cr[0, 0]) >> sh


# ------------------------------------------------------------------------------------------------ model values
@pytest.mark.parametrize('matrix, colour, want', [('bt709', 'red', (63, 102, 240)), ('bt709', 'blue', (32, 240, 118)),
                                                  ('bt709', 'white', (235, 128, 128)), ('bt709', 'black', (16, 128, 128)),
                                                  ('bt601', 'red', (81, 90, 240)), ('bt601', 'blue', (41, 240, 110))])
def test_published_8bit_limited_codes(matrix, colour, want):
    for fmt in ('nv12', 'i420'):
        assert _codes(yc.COLOURS[colour], fmt, matrix, 'limited') == want


def test_10bit_codes_are_the_x4_expressions_own_roundings():
    """Not the 8-bit code times 4: 64 + 876 ey, 512 + 896 m rounded on their own."""
    differs = 0
    for matrix in ('bt709', 'bt601'):
        kr, kb = yuv.MATRICES[matrix]
        kg = 1.0 - kr - kb
        for name in ('red', 'green', 'blue', 'white', 'black', 'yellow'):
            r, g, b = [c / 255.0 for c in yc.COLOURS[name]]
            ey = (kr * r + kg * g) + kb * b
            want = tuple(int(np.rint(v)) for v in (64 + 876 * ey, 512 + 896 * ((b - ey) * (0.5 / (1.0 - kb))), 512 + 896 * ((r - ey) * (0.5 / (1.0 - kr)))))
            for fmt in ('p010', 'i420p10'):
                assert _codes(yc.COLOURS[name], fmt, matrix, 'limited') == want, (matrix, name, fmt)
            differs += want != tuple(4 * c for c in _codes(yc.COLOURS[name], 'i420', matrix, 'limited'))
    assert differs >= 4
    assert _codes(yc.COLOURS['red'], 'p010', 'bt709', 'limited') == (250, 409, 960)


def test_coefficients_are_the_documented_doubles():
    kr, kg, kb, icb, icr, oy, sy, oc, sc = yuv.coefficients('nv12', 'bt709', 'limited')
    assert (kr, kb, kg) == (0.2126, 0.0722, 1.0 - 0.2126 - 0.0722) and (icb, icr) == (0.5 / (1.0 - 0.0722), 0.5 / (1.0 - 0.2126))
    assert (oy, sy, oc, sc) == (16.0, 219.0, 128.0, 224.0)
    assert yuv.coefficients('p010', 'bt601', 'limited')[5:] == (64.0, 876.0, 512.0, 896.0) and yuv.coefficients('i420', 'bt601')[0:3:2] == (0.299, 0.114)
    assert yuv.coefficients('i420', 'bt709', 'full')[5:] == (0.0, 255.0, 128.0, 255.0)
    assert yuv.coefficients('i420p10', 'bt709', 'full')[5:] == (0.0, 1023.0, 512.0, 1023.0)


@pytest.mark.parametrize('fmt', FORMATS)
def test_full_range_grey_ramp_is_the_byte_and_mid_chroma(fmt):
    d, _, sh = yuv.FORMATS[fmt]
    for name in ('grey_ramp', 'grey_all'):
        frame = yc.cases()[name]
        h, w = frame.shape[1:]
        y, cb, cr = yuv.planes(yuv.rgb_to_yuv420(frame, fmt, 'bt709', 'full'), h, w, fmt)
        if d == 8:
            assert np.array_equal(y, frame[0])
        else:
            assert np.array_equal(y >> sh, np.rint(1023.0 * (frame[0].astype(np.float64) / 255.0)).astype(np.int64))
        assert (cb >> sh == 2 ** (d - 1)).all() and (cr >> sh == 2 ** (d - 1)).all()


def test_pure_blue_at_full_range_clamps():
    v = yuv.pre_rounding(yc.solid(yc.COLOURS['blue']), yuv.coefficients('nv12', 'bt709', 'full'))[1][0, 0]
    assert v == 255.5
    assert _codes(yc.COLOURS['blue'], 'nv12', 'bt709', 'full')[1] == 255 and _codes(yc.COLOURS['blue'], 'i420', 'bt709', 'full')[1] == 255
    assert yuv.pre_rounding(yc.solid(yc.COLOURS['blue']), yuv.coefficients('p010', 'bt709', 'full'))[1][0, 0] == 1023.5
    assert _codes(yc.COLOURS['blue'], 'p010', 'bt709', 'full')[1] == 1023 and _codes(yc.COLOURS['red'], 'i420p10', 'bt709', 'full')[2] == 1023


def test_layouts_p010_and_plane_views():
    cs = yc.cases()
    for name in ('detail_u8', 'detail_f32', 'primaries'):
        frame = cs[name]
        h, w = frame.shape[1:]
        lo = yuv.rgb_to_yuv420(frame, 'i420p10', 'bt709', 'limited')
        p010 = yuv.rgb_to_yuv420(frame, 'p010', 'bt709', 'limited')
        assert p010.dtype == np.uint16 and lo.dtype == np.uint16 and p010.shape == lo.shape == (3 * h // 2, w)
        y, cb, cr = yuv.planes(lo, h, w, 'i420p10')
        y2, cb2, cr2 = yuv.planes(p010, h, w, 'p010')
        assert np.array_equal(y2, y << 6) and np.array_equal(cb2, cb << 6) and np.array_equal(cr2, cr << 6)
        assert np.array_equal(p010.reshape(-1)[h * w:], np.stack([cb << 6, cr << 6], -1).reshape(-1))        # NV12 order
        assert np.array_equal(yuv.to_planar(p010, h, w, 'p010'), lo)
        nv12, i420 = (yuv.rgb_to_yuv420(frame, f, 'bt709', 'limited') for f in ('nv12', 'i420'))
        assert nv12.dtype == np.uint8 and np.array_equal(yuv.to_planar(nv12, h, w, 'nv12'), i420) and not np.array_equal(nv12, i420)
    # the views tile the buffer exactly: every sample belongs to exactly one plane
    for fmt in FORMATS:
        for h, w in ((2, 2), (6, 10), (34, 70)):
            buf = np.zeros(yuv.frame_shape(h, w), yuv.dtype_of(fmt))
            views = yuv.planes(buf, h, w, fmt)
            assert [v.shape for v in views] == [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
            for v in views:
                assert np.shares_memory(v, buf)
                v += 1
            assert (buf == 1).all() and yuv.frame_bytes(h, w, fmt) == buf.nbytes
    with pytest.raises(ValueError, match='even'):
        yuv.frame_shape(3, 4)
    # a batch, and a channels-last view of the same values
    b = np.stack([cs['detail_u8'], cs['detail_u8'][:, ::-1].copy()])
    got = yuv.rgb_to_yuv420(b, 'nv12')
    assert got.shape == (2, 9, 10) and np.array_equal(got[1], yuv.rgb_to_yuv420(b[1], 'nv12'))
    hwc = np.ascontiguousarray(cs['detail_u8'].transpose(1, 2, 0)).transpose(2, 0, 1)
    assert np.array_equal(yuv.rgb_to_yuv420(hwc, 'nv12'), yuv.rgb_to_yuv420(cs['detail_u8'], 'nv12'))


def test_float_sources_widen_exactly_and_bytes_divide_in_float64():
    x16 = np.array([0.1, 0.3337, 1.0, 6e-8], np.float16)
    assert np.array_equal(yuv.source_f64(x16), x16.astype(np.float64)) and yuv.source_f64(x16).dtype == np.float64
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(yuv.source_f64(u), u.astype(np.float64) / 255.0)
    assert (yuv.source_f64(u) != (u.astype(np.float32) * np.float32(1 / 255.0)).astype(np.float64)).sum() > 100


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize('case, fmt, matrix, range, plane', yc.TIES)
def test_tie_cases_sit_exactly_on_a_half_code(case, fmt, matrix, range, plane):
    frame = yc.cases()[case]
    h, w = frame.shape[1:]
    mask = yc.tie_mask(frame, fmt, matrix, range, plane)
    assert mask.any(), 'no pre-rounding value of this case is k + 0.5'
    pre = yuv.pre_rounding(frame, yuv.coefficients(fmt, matrix, range))[plane]
    got = yuv.planes(yuv.rgb_to_yuv420(frame, fmt, matrix, range), h, w, fmt)[plane].astype(np.int64) >> yuv.FORMATS[fmt][2]
    lo = np.floor(pre[mask]).astype(np.int64)
    assert np.array_equal(got[mask], lo + (lo & 1))                 # half to even: k + 0.5 -> k for even k, k + 1 for odd k


def test_every_format_has_a_tie_and_some_ties_round_down():
    assert set(t[1] for t in yc.TIES) == set(FORMATS)
    down = 0
    for case, fmt, matrix, range, plane in yc.TIES:
        frame = yc.cases()[case]
        pre = yuv.pre_rounding(frame, yuv.coefficients(fmt, matrix, range))[plane]
        m = yc.tie_mask(frame, fmt, matrix, range, plane)
        down += int((np.floor(pre[m]) % 2 == 0).sum())              # k even: half-even gives k, half-up k + 1
    assert down >= 2


# ------------------------------------------------------------------------------------------------ wrong models
@pytest.mark.parametrize('control', sorted(yc.CONTROLS))
def test_each_control_changes_the_case_built_for_it(control):
    case, fmt, matrix, range = yc.CONTROLS[control]
    frame = yc.cases()[case]
    want = yuv.rgb_to_yuv420(frame, fmt, matrix, range)
    got = yc.control_model(control, frame, fmt, matrix, range)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert not np.array_equal(got, want), 'the %s mistake is invisible on %s' % (control, case)


def test_the_control_harness_without_a_mistake_is_the_model():
    for name, frame in yc.cases().items():
        for fmt in FORMATS:
            assert np.array_equal(yc.control_model(None, frame, fmt, 'bt709', 'limited'), yuv.rgb_to_yuv420(frame, fmt, 'bt709', 'limited')), (name, fmt)


# ------------------------------------------------------------------------------------------------ Y4M
@pytest.mark.parametrize('fmt, tag', [('i420', b'C420jpeg'), ('i420p10', b'C420p10')])
@pytest.mark.parametrize('h, w', [(2, 2), (6, 10), (34, 70)])
def test_y4m_round_trip(tmp_path, fmt, tag, h, w):
    g = np.random.RandomState(h * w)
    frames = [yuv.rgb_to_yuv420(g.rand(3, h, w).astype(np.float32), fmt, 'bt709', 'full') for _ in range(3)]
    path = str(tmp_path / 'clip.y4m')
    with yuv.Y4MWriter(path, h, w, fmt, fps=(30000, 1001), range='full') as wr:
        for f in frames:
            wr.write(f)
        assert wr.frames == 3
    raw = open(path, 'rb').read()
    head = b'YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 %s XCOLORRANGE=FULL\n' % (w, h, tag)
    assert raw.startswith(head + b'FRAME\n')
    assert len(raw) == len(head) + 3 * (6 + yuv.frame_bytes(h, w, fmt))
    if fmt == 'i420p10':
        assert raw[len(head) + 6:len(head) + 8] == bytes([int(frames[0][0, 0]) & 255, int(frames[0][0, 0]) >> 8])      # little-endian
    back = yuv.read_y4m(path)
    assert (back['h'], back['w'], back['fps'], back['fmt'], back['range']) == (h, w, (30000, 1001), fmt, 'full')
    assert len(back['frames']) == 3 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(back['frames'], frames))


def test_y4m_header_defaults_and_refusals(tmp_path):
    assert yuv.y4m_header(4, 6, 'i420') == b'YUV4MPEG2 W6 H4 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n'
    assert yuv.y4m_header(4, 6, 'i420p10', (25, 1), 'full') == b'YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420p10 XCOLORRANGE=FULL\n'
    for fmt, twin in (('nv12', 'i420'), ('p010', 'i420p10')):
        with pytest.raises(ValueError, match="not a Y4M format.*'%s'" % twin):
            yuv.Y4MWriter(str(tmp_path / 'x.y4m'), 4, 6, fmt)
    assert not os.path.exists(str(tmp_path / 'x.y4m'))
    with yuv.Y4MWriter(str(tmp_path / 'y.y4m'), 4, 6, 'i420') as wr:
        with pytest.raises(ValueError, match='i420 frames are uint8'):
            wr.write(np.zeros((6, 6), np.uint16))
        with pytest.raises(ValueError, match='i420 frames are uint8'):
            wr.write(np.zeros((4, 6), np.uint8))
    assert yuv.parse_fps('30') == (30, 1) and yuv.parse_fps('30000:1001') == (30000, 1001)
    for bad in ('0', 'x', '30:0', '1:2:3', ''):
        with pytest.raises(ValueError, match='N or N:D'):
            yuv.parse_fps(bad)


# ------------------------------------------------------------------------------------------------ library and config
@pytest.fixture(scope='module')
def lib():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def test_header_binding_and_library_agree_on_the_yuv_symbols(lib):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    assert re.search(r'REFVSR_YUV_NV12 = 0, REFVSR_YUV_I420 = 1, REFVSR_YUV_P010 = 2, REFVSR_YUV_I420P10 = 3', src)
    assert (hip.YUV_NV12, hip.YUV_I420, hip.YUV_P010, hip.YUV_I420P10) == (0, 1, 2, 3)
    assert yuv.FORMAT_IDS == {'nv12': hip.YUV_NV12, 'i420': hip.YUV_I420, 'p010': hip.YUV_P010, 'i420p10': hip.YUV_I420P10}
    assert re.search(r'#define REFVSR_YUV420_MAX_FRAMES %d\b' % hip.YUV420_MAX_FRAMES, src) and lib.refvsr_yuv420_max_frames() == hip.YUV420_MAX_FRAMES
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'int\s+refvsr_result_to_yuv420\s*\(\s*const void\* const\* src,\s*int src_fmt,\s*void\* const\* dst,\s*int nframes,\s*int h,\s*int w,'
                     r'\s*int yuv_fmt,\s*const double\* coef9,\s*void\* stream\)', code)
    for name in ('refvsr_result_to_yuv420', 'refvsr_yuv420_bytes', 'refvsr_yuv420_max_frames'):
        assert name in hip.EXPORTS and hasattr(ctypes.CDLL(hip.LIB_PATH), name)
    assert hip.ABI_VERSION == 15 and lib.refvsr_abi_version() == 15
    for fmt, fid in yuv.FORMAT_IDS.items():
        for h, w in ((2, 2), (6, 10), (34, 70), (1080, 1920), (4320, 7680)):
            assert lib.refvsr_yuv420_bytes(h, w, fid) == yuv.frame_bytes(h, w, fmt)
        for h, w in ((3, 4), (4, 3), (0, 4), (4, -2)):
            assert lib.refvsr_yuv420_bytes(h, w, fid) == 0
    assert lib.refvsr_yuv420_bytes(4, 4, 4) == 0 and lib.refvsr_yuv420_bytes(4, 4, -1) == 0


def test_argument_checks_answer_before_device_work(lib):
    """Host memory stands in for device pointers (never dereferenced): every refusal comes with its message, on a box without a GPU."""
    from refvsr_amd import hip
    P = ctypes.c_void_p
    buf = (ctypes.c_char * (1 << 16))()
    base = (ctypes.addressof(buf) + 63) & ~63
    at = lambda off: P(base + off)
    arr = lambda *ps: (P * len(ps))(*[p.value for p in ps])
    coef = (ctypes.c_double * 9)(*yuv.coefficients('nv12'))
    err = lambda: lib.refvsr_last_error().decode()
    call = lambda src, sfmt, dst, n, h, w, yfmt, k=coef: lib.refvsr_result_to_yuv420(src, sfmt, dst, n, h, w, yfmt, k, None)

    def expect(rc, text):
        assert rc != 0 and text in err(), err()

    s1, d1 = arr(at(0)), arr(at(8192))
    expect(call(None, hip.RESULT_U8, d1, 1, 8, 8, hip.YUV_NV12), 'result_to_yuv420: null frame table')
    expect(call(s1, hip.RESULT_U8, None, 1, 8, 8, hip.YUV_NV12), 'result_to_yuv420: null frame table')
    expect(call(s1, hip.RESULT_U8, d1, 1, 8, 8, hip.YUV_NV12, None), 'result_to_yuv420: null coefficients')
    expect(call(s1, hip.RESULT_U8, d1, 0, 8, 8, hip.YUV_NV12), 'result_to_yuv420: 1..16 frames per launch')
    expect(call(s1, hip.RESULT_U8, d1, 17, 8, 8, hip.YUV_NV12), 'result_to_yuv420: 1..16 frames per launch')
    for bad in (3, 7, hip.RESULT_HWC | 3, 0x20, -1):
        expect(call(s1, bad, d1, 1, 8, 8, hip.YUV_NV12), 'result_to_yuv420: unknown result format %d' % bad)
    for bad in (4, -1):
        expect(call(s1, hip.RESULT_U8, d1, 1, 8, 8, bad), 'result_to_yuv420: unknown yuv format %d' % bad)
    for h, w in ((7, 8), (8, 7), (0, 8), (8, -2)):
        expect(call(s1, hip.RESULT_U8, d1, 1, h, w, hip.YUV_NV12), 'result_to_yuv420: h, w must be even and positive (got %d x %d)' % (h, w))
    expect(call(s1, hip.RESULT_F32, d1, 1, 1 << 14, 1 << 14, hip.YUV_NV12), 'result_to_yuv420: frame too large for 32-bit offsets')
    expect(call(arr(at(0), P(0)), hip.RESULT_U8, arr(at(8192), at(12288)), 2, 8, 8, hip.YUV_NV12), 'result_to_yuv420: null pointer (frame 1)')
    expect(call(arr(at(0), at(4096)), hip.RESULT_U8, arr(at(8192), P(0)), 2, 8, 8, hip.YUV_NV12), 'result_to_yuv420: null pointer (frame 1)')
    expect(call(arr(at(2)), hip.RESULT_F32, d1, 1, 8, 8, hip.YUV_NV12), 'must be aligned to their samples (frame 0)')
    expect(call(arr(at(1)), hip.RESULT_F16 | hip.RESULT_HWC, d1, 1, 8, 8, hip.YUV_NV12), 'must be aligned to their samples (frame 0)')
    expect(call(s1, hip.RESULT_U8, arr(at(8193)), 1, 8, 8, hip.YUV_P010), 'must be aligned to their samples (frame 0)')
    # 8 x 8 float32: 768 source bytes, 96 (nv12) / 192 (p010) destination bytes
    expect(call(s1, hip.RESULT_F32, arr(at(0)), 1, 8, 8, hip.YUV_NV12), 'result_to_yuv420: destination 0 overlaps source 0')
    expect(call(s1, hip.RESULT_F32, arr(at(764)), 1, 8, 8, hip.YUV_NV12), 'result_to_yuv420: destination 0 overlaps source 0')
    expect(call(arr(at(96)), hip.RESULT_F32, arr(at(4)), 1, 8, 8, hip.YUV_NV12), 'result_to_yuv420: destination 0 overlaps source 0')
    expect(call(arr(at(0), at(4096)), hip.RESULT_F32, arr(at(8192), at(4004)), 2, 8, 8, hip.YUV_NV12), 'result_to_yuv420: destination 1 overlaps source 1')
    expect(call(arr(at(0), at(4096)), hip.RESULT_F32, arr(at(8192), at(8192 + 100)), 2, 8, 8, hip.YUV_P010), 'result_to_yuv420: destinations 0 and 1 overlap')


def test_config_validation_and_defaults():
    from refvsr_amd import get_config
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    assert cfg.result_yuv is None and cfg.yuv_matrix == 'bt709' and cfg.yuv_range == 'limited'
    assert yuv.resolve(None, 'bt709', 'limited') is None and yuv.resolve(None) is None
    assert yuv.resolve('p010', 'bt601', 'full') == ('p010', 'bt601', 'full') and yuv.resolve('nv12') == ('nv12', 'bt709', 'limited')
    with pytest.raises(ValueError, match="result_yuv must be None, 'nv12', 'i420', 'p010' or 'i420p10', got 'yv12'"):
        yuv.resolve('yv12')
    with pytest.raises(ValueError, match="yuv_matrix must be 'bt709' or 'bt601', got 'bt2020'"):
        yuv.resolve('nv12', 'bt2020')
    with pytest.raises(ValueError, match="yuv_range must be 'limited' or 'full', got 'tv'"):
        yuv.resolve(None, 'bt709', 'tv')
    # the engine asks exactly this when it is built (next to result_dtype / result_layout)
    src = open(os.path.join(ROOT, 'refvsr_amd', 'engine.py')).read()
    assert "self.result_yuv = yuv.resolve(getattr(config, 'result_yuv', None), getattr(config, 'yuv_matrix', None), getattr(config, 'yuv_range', None))" in src
    for fmt in ('x', None):
        with pytest.raises(ValueError):
            yuv.coefficients(fmt)


def test_engine_executor_refuses_result_yuv():
    from refvsr_amd import shard
    from refvsr_amd.config import AttrDict

    class Net(object):
        Network = AttrDict(config=AttrDict(result_yuv='nv12'))

    with pytest.raises(RuntimeError, match="sharded runner returns RGB results only: config.result_yuv = 'nv12'"):
        shard.EngineExecutor(Net(), 'cuda:0', 32, 48, 6, 3)


def test_evalrun_options():
    from refvsr_amd import evalrun
    base = ['--config', 'config_RefVSR_small_L1', '--data_offset', '/nowhere']
    cfg = evalrun.build_config(base)
    assert cfg.result_yuv is None and cfg.EVAL.video_out is None and cfg.EVAL.video_fps == (30, 1)
    cfg = evalrun.build_config(base + ['--video_out', 'y4m'])
    assert cfg.result_yuv == 'i420' and cfg.EVAL.video_out == 'y4m' and (cfg.yuv_matrix, cfg.yuv_range) == ('bt709', 'limited')
    cfg = evalrun.build_config(base + ['--video_out', 'y4m', '--video_depth', '10', '--video_fps', '30000:1001', '--yuv_matrix', 'bt601', '--yuv_range', 'full'])
    assert cfg.result_yuv == 'i420p10' and cfg.EVAL.video_fps == (30000, 1001) and (cfg.yuv_matrix, cfg.yuv_range) == ('bt601', 'full')
    assert evalrun.build_config(base + ['--video_fps', '24']).EVAL.video_fps == (24, 1)
    for mode in ('quan_FOV', 'quan_conf_map'):
        with pytest.raises(RuntimeError, match='--video_out writes the frames of the qual_quan loop; --eval_mode %s' % mode):
            evalrun.build_config(base + ['--video_out', 'y4m', '--eval_mode', mode])
        assert evalrun.build_config(base + ['--eval_mode', mode]).EVAL.video_out is None
        cfg = evalrun.build_config(base + ['--video_out', 'y4m'])
        cfg.EVAL.eval_mode = mode                                    # a config edited after the parse is refused by the loop itself
        with pytest.raises(RuntimeError, match='--video_out writes the frames'):
            evalrun.evaluate(cfg, net=object())
    with pytest.raises(ValueError, match='N or N:D'):
        evalrun.build_config(base + ['--video_fps', '30/1'])
    with pytest.raises(SystemExit):
        evalrun.build_config(base + ['--video_depth', '12'])


def test_torch_op_is_registered_with_shape_inference():
    import torch
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'result_to_yuv420' in t.OP_NAMES and hasattr(torch.ops.refvsr, 'result_to_yuv420')
    assert str(torch.ops.refvsr.result_to_yuv420.default._schema) == 'refvsr::result_to_yuv420(Tensor frames, str fmt, str matrix, str range) -> Tensor'
    with FakeTensorMode():
        x = torch.empty((3, 3, 34, 70), dtype=torch.uint8, device='cuda')
        y = torch.ops.refvsr.result_to_yuv420(x, 'nv12', 'bt709', 'limited')
        assert y.shape == (3, 51, 70) and y.dtype == torch.uint8
        y = torch.ops.refvsr.result_to_yuv420(x.half(), 'p010', 'bt601', 'full')
        assert y.shape == (3, 51, 70) and y.dtype == torch.uint16
        for args, text in ((('yv12', 'bt709', 'limited'), 'unknown yuv format'), (('nv12', 'bt2020', 'limited'), 'yuv_matrix must be'),
                           (('nv12', 'bt709', 'tv'), 'yuv_range must be')):
            with pytest.raises(RuntimeError, match=text):
                torch.ops.refvsr.result_to_yuv420(x, *args)
