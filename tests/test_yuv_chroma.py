"""4:2:2, 4:4:4 and left-sited 4:2:0 frames, host side: the layouts, the siting of the numpy models refvsr_amd/yuv.py:rgb_to_yuv and
yuv_to_rgb against ramps and against the arithmetic written out pixel by pixel, crafted ties, wrong-model controls, Y4M tags, the C ABI
of the three entry points without a device, the config fields and the argument errors of videorun.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import yuv_chroma_cases as cc
from refvsr_amd import yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'refvsr_yuv_frame_bytes', 'refvsr_result_to_yuv', 'refvsr_yuv_to_rgb'}
SMALL = ((2, 2), (6, 10), (34, 70))
builtins_range = range


@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('fmt', cc.NEW_FORMATS)
def test_plane_views_tile_the_buffer(fmt):
    cv, ch = yuv.SUBSAMPLING[yuv.sampling_of(fmt)]
    for h, w in SMALL:
        rows, cols = yuv.frame_shape(h, w, fmt)
        assert (rows, cols) == ({'422': 2 * h, '444': 3 * h}[yuv.sampling_of(fmt)], w)
        buf = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
        y, cb, cr = yuv.planes(buf, h, w, fmt)
        assert y.shape == (h, w) and cb.shape == cr.shape == (h // cv, w // ch)
        assert all(np.shares_memory(p, buf) for p in (y, cb, cr))
        assert np.array_equal(np.concatenate([p.reshape(-1) for p in (y, cb, cr)]), buf.reshape(-1))
        back = yuv.pack(y, cb, cr, fmt)
        assert back.dtype == yuv.dtype_of(fmt) and back.shape == (rows, cols) and np.array_equal(back, buf.astype(back.dtype))     # (the cast wraps)
    assert yuv.dtype_of(fmt) == (np.uint16 if fmt.endswith('p10') else np.uint8) and yuv.depth_of(fmt) == (10 if fmt.endswith('p10') else 8)
    with pytest.raises(ValueError, match='even'):
        yuv.frame_shape(3, 4, fmt)                            # 4:4:4 too: the engine's frame checks and refvsr_luma_sad need even sizes
    with pytest.raises(ValueError, match='even'):
        yuv.frame_shape(4, 5, fmt)


def test_pinned_tables_and_old_forms_are_unchanged():
    assert yuv.FORMAT_IDS == {'nv12': 0, 'i420': 1, 'p010': 2, 'i420p10': 3} and sorted(yuv.FORMATS) == sorted(yuv.FORMAT_IDS)
    assert yuv.frame_shape(6, 10) == (9, 10) == yuv.frame_shape(6, 10, 'nv12')
    assert yuv.SAMPLINGS == {'420': 0, '422': 1, '444': 2} and yuv.SITINGS == {'centre': 0, 'left': 1}
    x = cc.detail(6, 10, np.float32)
    for fmt in yuv.FORMATS:
        b = yuv.rgb_to_yuv420(x, fmt, 'bt601', 'full')
        assert np.array_equal(yuv.rgb_to_yuv(x, fmt, 'bt601', 'full', 'centre'), b)
        for chroma in ('bilinear', 'nearest'):
            assert np.array_equal(yuv.yuv_to_rgb(b, 6, 10, fmt, 'bt601', 'full', chroma, 'centre'), yuv.yuv420_to_rgb(b, 6, 10, fmt, 'bt601', 'full', chroma))
    for fmt in ('i444', 'i444p10'):                            # siting: validated, then ignored
        assert np.array_equal(yuv.rgb_to_yuv(x, fmt, siting='left'), yuv.rgb_to_yuv(x, fmt, siting='centre'))
        with pytest.raises(ValueError, match="'centre' or 'left'"):
            yuv.rgb_to_yuv(x, fmt, siting='top')
        with pytest.raises(ValueError, match="'centre' or 'left'"):
            yuv.yuv_to_rgb(yuv.rgb_to_yuv(x, fmt), 6, 10, fmt, siting='top')


def test_frame_bytes_is_the_librarys(L):
    for h, w in SMALL + ((1080, 1920),):
        for fmt in yuv.ALL_FORMATS:
            fid, samp = yuv.FORMAT_IDS[yuv.twin_of(fmt)], yuv.SAMPLINGS[yuv.sampling_of(fmt)]
            assert L.refvsr_yuv_frame_bytes(h, w, fid, samp) == yuv.frame_bytes(h, w, fmt) > 0
            if fmt in yuv.FORMATS:
                assert L.refvsr_yuv_frame_bytes(h, w, fid, 0) == L.refvsr_yuv420_bytes(h, w, fid)
    for args in ((3, 4, 1, 1), (4, 5, 1, 2), (0, 4, 1, 1), (4, 4, 4, 1), (4, 4, 1, 3), (4, 4, 1, -1), (4, 4, 0, 1), (4, 4, 2, 2)):
        assert L.refvsr_yuv_frame_bytes(*args) == 0, args      # odd, empty, unknown format / sampling, semi-planar 4:2:2 / 4:4:4


# ------------------------------------------------------------------------------------------------ siting, against ramps
@pytest.mark.parametrize('sampling', ['420', '422'])
def test_way_in_reads_a_ramp_at_its_sites(sampling):
    """A chroma ramp of 4 codes per luma pixel, sampled at the left sites (x = 2j) or the centre sites (x = 2j + 1/2): the tap sum at
    every interior luma column is exactly 16 (c0 + 4 x); read with the other siting it is off by exactly 2 codes, half a pixel."""
    c0, w2, h2 = 16, 10, 3 if sampling == '420' else 6
    j = np.arange(w2)
    x = np.arange(2 * w2)
    planes = {'left': np.tile(c0 + 8 * j, (h2, 1)), 'centre': np.tile(c0 + 8 * j + 2, (h2, 1))}
    want = 16 * (c0 + 4 * x)
    inner = slice(1, 2 * w2 - 1)
    for siting in ('left', 'centre'):
        other = 'centre' if siting == 'left' else 'left'
        got = yuv.chroma_taps(planes[siting], 'bilinear', sampling, siting)
        assert got.shape == (6, 2 * w2) and (got[:, inner] == want[inner]).all(), siting
        off = yuv.chroma_taps(planes[siting], 'bilinear', sampling, other)
        assert (np.abs(off[:, inner] - want[inner]) == 32).all(), siting
        assert (yuv.chroma_taps(planes[siting], 'nearest', sampling, siting) == 16 * np.repeat(planes[siting][0], 2)).all()


@pytest.mark.parametrize('sampling', ['420', '422'])
def test_way_out_samples_a_ramp_at_its_sites(sampling):
    """A frame whose ecb is linear in x: the value ahead of rint is the ramp's at the sample's site -- the even column for left, the
    middle of the pair for centre -- to 1e-9 code (only float64 rounding of values below 2^10 remains)."""
    h, w = 4, 20
    coef = yuv.coefficients('i420', 'bt709', 'full')
    kr, kg, kb, icb, icr, oy, sy, oc, sc = coef
    x = np.arange(w, dtype=np.float64)
    rgb = np.empty((3, h, w))
    rgb[0] = rgb[1] = 0.5
    rgb[2] = 0.2 + 0.02 * x
    ramp = lambda at: oc + sc * (((0.2 + 0.02 * at) - ((kr + kg) * 0.5 + kb * (0.2 + 0.02 * at))) * icb)
    j = np.arange(w // 2, dtype=np.float64)
    for siting, site in (('left', 2 * j), ('centre', 2 * j + 0.5)):
        cb = yuv.pre_rounding(rgb, coef, sampling, siting)[1]
        assert cb.shape == (h // yuv.SUBSAMPLING[sampling][0], w // 2)
        assert np.abs(cb[:, 1:] - ramp(site)[1:]).max() < 1e-9, siting
        wrong = yuv.pre_rounding(rgb, coef, sampling, 'centre' if siting == 'left' else 'left')[1]
        assert np.abs(np.abs(wrong[:, 1:] - ramp(site)[1:]) - sc * 0.01 * (1.0 - kb) * icb).max() < 1e-9      # half a pixel of the ramp
    # the left edge: l = max(2j - 1, 0) = 0, column 0 stands in for the column in front of the frame
    e = (rgb[2] - ((kr * rgb[0] + kg * rgb[1]) + kb * rgb[2])) * icb
    assert np.abs(yuv.pre_rounding(rgb, coef, sampling, 'left')[1][:, 0] - (oc + sc * (3 * e[0, 0] + e[0, 1]) / 4)).max() < 1e-9


def test_vertical_siting_of_420_left_is_centres():
    """A frame that varies along y only: left and centre give the same chroma, both ways."""
    h, w = 8, 6
    rgb = np.empty((3, h, w))
    rgb[0] = rgb[1] = 0.4
    rgb[2] = (0.1 + 0.1 * np.arange(h))[:, None]
    coef = yuv.coefficients('i420', 'bt709', 'limited')
    a, b = yuv.pre_rounding(rgb, coef, '420', 'left'), yuv.pre_rounding(rgb, coef, '420', 'centre')
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.ptp(a[1][:, 0]) > 10
    c = np.tile((20 + 7 * np.arange(4) ** 2)[:, None], (1, 3))
    assert np.array_equal(yuv.chroma_taps(c, 'bilinear', '420', 'left'), yuv.chroma_taps(c, 'bilinear', '420', 'centre'))


# ------------------------------------------------------------------------------------------------ the arithmetic, written out
def taps_by_hand(c, sampling, siting, chroma):
    """The tap sums of the specification, pixel by pixel."""
    cv, ch = yuv.SUBSAMPLING[sampling]
    hc, wc = c.shape
    out = np.zeros((hc * cv, wc * ch), np.int64)
    for y in builtins_range(hc * cv):
        for x in builtins_range(wc * ch):
            if sampling == '444':
                out[y, x] = 16 * c[y, x]
                continue
            cx, cy = x >> 1, (y >> 1 if cv == 2 else y)
            cyn = min(max(cy + (1 if y & 1 else -1), 0), hc - 1) if cv == 2 else cy
            cxn = min(max(cx + (1 if x & 1 else -1), 0), wc - 1)
            cxr = min(cx + 1, wc - 1)
            if chroma == 'nearest':
                out[y, x] = 16 * c[cy, cx]
            elif sampling == '422' and siting == 'centre':
                out[y, x] = 12 * c[y, cx] + 4 * c[y, cxn]
            elif sampling == '422':
                out[y, x] = 16 * c[y, cx] if x % 2 == 0 else 8 * c[y, cx] + 8 * c[y, cxr]
            elif siting == 'left':
                out[y, x] = 12 * c[cy, cx] + 4 * c[cyn, cx] if x % 2 == 0 else 6 * c[cy, cx] + 2 * c[cyn, cx] + 6 * c[cy, cxr] + 2 * c[cyn, cxr]
            else:
                out[y, x] = 9 * c[cy, cx] + 3 * c[cyn, cx] + 3 * c[cy, cxn] + c[cyn, cxn]
    return out


def mean_by_hand(e, sampling, siting):
    cv, ch = yuv.SUBSAMPLING[sampling]
    h, w = e.shape
    m = np.zeros((h // cv, w // ch))
    for i in builtins_range(h // cv):
        for j in builtins_range(w // ch):
            l = max(2 * j - 1, 0)
            if sampling == '444':
                m[i, j] = e[i, j]
            elif sampling == '422' and siting == 'centre':
                m[i, j] = (e[i, 2 * j] + e[i, 2 * j + 1]) * 0.5
            elif sampling == '422':
                m[i, j] = ((e[i, l] + e[i, 2 * j + 1]) + (e[i, 2 * j] + e[i, 2 * j])) * 0.25
            elif siting == 'left':
                v = lambda x: e[2 * i, x] + e[2 * i + 1, x]
                m[i, j] = ((v(l) + v(2 * j + 1)) + (v(2 * j) + v(2 * j))) * 0.125
            else:
                m[i, j] = ((e[2 * i, 2 * j] + e[2 * i, 2 * j + 1]) + (e[2 * i + 1, 2 * j] + e[2 * i + 1, 2 * j + 1])) * 0.25
    return m


@pytest.mark.parametrize('sampling', ['420', '422', '444'])
@pytest.mark.parametrize('siting', ['centre', 'left'])
def test_model_is_the_written_out_arithmetic(sampling, siting):
    rs = np.random.RandomState(5)
    cv, ch = yuv.SUBSAMPLING[sampling]
    for h, w in ((2, 2), (2, 4), (4, 2), (6, 10)):
        c = rs.randint(0, 1024, (h // cv, w // ch)).astype(np.int64)
        for chroma in ('bilinear', 'nearest'):
            got = yuv.chroma_taps(c, chroma, sampling, siting)
            assert got.max() < 2 ** 15 and np.array_equal(got, taps_by_hand(c, sampling, siting, chroma)), (h, w, chroma)
        e = rs.rand(h, w) - 0.5
        assert np.array_equal(yuv.chroma_mean(e, sampling, siting), mean_by_hand(e, sampling, siting)), (h, w)


# ------------------------------------------------------------------------------------------------ ties and controls
def test_crafted_ties_are_ties_and_round_to_even():
    seen, down = set(), 0
    for fmt, siting, frame, plane, rounds_down in cc.tie_cases():
        v = yuv.pre_rounding(frame, yuv.coefficients(fmt, 'bt709', 'full'), yuv.sampling_of(fmt), yuv.effective_siting(fmt, siting))[plane]
        tie = cc.tie_mask(frame, fmt, siting, plane)
        assert tie[:, -1].any(), (fmt, siting)
        y = int(np.argwhere(tie[:, -1])[0][0])
        k = np.floor(v[y, -1])
        assert (k % 2 == 0) == rounds_down
        code = yuv.planes(yuv.rgb_to_yuv(frame, fmt, 'bt709', 'full', siting), 2, 4, fmt)[plane].astype(np.int64) >> yuv.FORMATS[yuv.twin_of(fmt)][2]
        assert code[y, -1] == (k if rounds_down else k + 1)
        seen.add((yuv.sampling_of(fmt), yuv.effective_siting(fmt, siting)))
        down += bool(rounds_down)
    assert seen == {('420', 'left'), ('422', 'centre'), ('422', 'left'), ('444', 'centre')} and down >= 2


def test_out_controls_change_their_cases():
    names = set()
    for control, frame, fmt, siting in cc.out_controls():
        assert np.array_equal(cc.out_control(None, frame, fmt, siting), yuv.rgb_to_yuv(frame, fmt, 'bt709', 'full', siting)), control
        assert not np.array_equal(cc.out_control(control, frame, fmt, siting), yuv.rgb_to_yuv(frame, fmt, 'bt709', 'full', siting)), control
        names.add(control)
    assert names == {'swap_siting', 'mirror_edge', 'h_before_v', 'avg_vertical_422', 'swap_cbcr', 'filter_444'}
    assert {(f, s) for c, _, f, s in cc.out_controls() if c == 'swap_siting'} == {('i422', 'left'), ('i420', 'centre')}      # both directions


def test_in_controls_change_their_cases():
    rs = np.random.RandomState(3)
    for control, fmt, siting in cc.IN_CONTROLS:
        buf = cc.random_codes(rs, 6, 10, fmt)
        want = yuv.yuv_to_rgb(buf, 6, 10, fmt, siting=siting)
        assert np.array_equal(cc.in_control(None, buf, 6, 10, fmt, siting).view(np.uint32), want.view(np.uint32)), control
        assert not np.array_equal(cc.in_control(control, buf, 6, 10, fmt, siting), want), control
        if control != 'swap_cbcr':                            # (the mistakes in the taps show in the tap sums themselves)
            sampling, cb = yuv.sampling_of(fmt), yuv.codes(buf, 6, 10, fmt)[1]
            assert not np.array_equal(cc.in_control_taps(control, cb, sampling, siting), yuv.chroma_taps(cb, 'bilinear', sampling, siting)), control
    assert {c for c, _, _ in cc.IN_CONTROLS} == {'swap_siting', 'wrong_end', 'mirror_edge', 'swap_cbcr', 'filter_444'}
    assert {s for c, _, s in cc.IN_CONTROLS if c == 'mirror_edge'} == {'centre', 'left'}


def test_half_of_a_sum_has_one_float64_form():
    """(e0 + e1) 0.5 against e0 0.5 + e1 0.5: NOT a control, because no case can tell them apart.  Halving is exact in binary floating
    point, so both round the same real number (e0 + e1) / 2 once: the same float64 for every pair outside the subnormal range -- and
    chroma differences that small give oc in either form.  Shown on a million random pairs and on the 4:2:2 centre ties."""
    rs = np.random.RandomState(9)
    e0, e1 = rs.rand(1000000) - 0.5, (rs.rand(1000000) - 0.5) * 2.0 ** rs.randint(-40, 1, 1000000)
    assert np.array_equal((e0 + e1) * 0.5, e0 * 0.5 + e1 * 0.5)
    for fmt, siting, frame, plane, _ in cc.tie_cases():
        if (yuv.sampling_of(fmt), siting) == ('422', 'centre'):
            kr, kg, kb, icb, icr = yuv.coefficients(fmt, 'bt709', 'full')[:5]
            r, g, b = yuv.source_f64(frame)
            ey = (kr * r + kg * g) + kb * b
            for e in ((b - ey) * icb, (r - ey) * icr):
                assert np.array_equal((e[:, 0::2] + e[:, 1::2]) * 0.5, e[:, 0::2] * 0.5 + e[:, 1::2] * 0.5)


# ------------------------------------------------------------------------------------------------ Y4M
TAGS = (('i420', 'centre', b'C420jpeg', None), ('i420', 'left', b'C420mpeg2', None), ('i420p10', 'centre', b'C420p10', None),
        ('i420p10', 'left', b'C420p10', b'XCHROMASITING=LEFT'), ('i422', 'left', b'C422', None), ('i422', 'centre', b'C422', b'XCHROMASITING=CENTRE'),
        ('i422p10', 'left', b'C422p10', None), ('i422p10', 'centre', b'C422p10', b'XCHROMASITING=CENTRE'), ('i444', 'centre', b'C444', None),
        ('i444p10', 'left', b'C444p10', None))


@pytest.mark.parametrize('fmt, siting, tag, extra', TAGS)
def test_y4m_round_trip_of_every_tag(tmp_path, fmt, siting, tag, extra):
    rs = np.random.RandomState(4)
    for h, w in SMALL:
        frames = [cc.random_codes(rs, h, w, fmt, dirty=False) for _ in builtins_range(2)]
        path = str(tmp_path / ('%d_%d.y4m' % (h, w)))
        with yuv.Y4MWriter(path, h, w, fmt, (30000, 1001), 'full', siting) as wr:
            for f in frames:
                wr.write(f)
        tok = open(path, 'rb').readline().split()
        assert tok[6] == tag and ((extra in tok) if extra else not any(t.startswith(b'XCHROMASITING') for t in tok))
        whole = yuv.read_y4m(path)
        with yuv.Y4MReader(path) as rd:
            want = (h, w, (30000, 1001), fmt, 'full', yuv.effective_siting(fmt, siting))
            assert (rd.h, rd.w, rd.fps, rd.fmt, rd.range, rd.siting) == want == tuple(whole[k] for k in ('h', 'w', 'fps', 'fmt', 'range', 'siting'))
            assert rd.length == 2
            got = list(rd)
        for a, b, c in zip(got, whole['frames'], frames):
            assert a.dtype == c.dtype and a.shape == yuv.frame_shape(h, w, fmt) and np.array_equal(a, c) and np.array_equal(b, c)
        with pytest.raises(ValueError, match='Y4MWriter'):
            with yuv.Y4MWriter(path, h, w, fmt) as wr:
                wr.write(np.zeros((yuv.frame_shape(h, w, fmt)[0] + 1, w), dtype=yuv.dtype_of(fmt)))


def test_y4m_headers():
    # today's two headers, byte for byte
    assert yuv.y4m_header(6, 10, 'i420', (30, 1), 'limited') == b'YUV4MPEG2 W10 H6 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n'
    assert yuv.y4m_header(6, 10, 'i420p10', (30000, 1001), 'full') == b'YUV4MPEG2 W10 H6 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n'
    assert yuv.y4m_header(6, 10, 'i422') == b'YUV4MPEG2 W10 H6 F30:1 Ip A1:1 C422 XCOLORRANGE=LIMITED\n'          # 4:2:2: left unless told
    assert yuv.y4m_header(6, 10, 'i420p10', siting='left') == b'YUV4MPEG2 W10 H6 F30:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED XCHROMASITING=LEFT\n'
    with pytest.raises(ValueError, match='not a Y4M format'):
        yuv.y4m_header(6, 10, 'nv12')
    # the headers ffmpeg writes
    hd = yuv.parse_y4m_header(b'YUV4MPEG2 W1920 H1080 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED', 'phone_uw.y4m')
    assert hd == {'h': 1080, 'w': 1920, 'fps': (30000, 1001), 'fmt': 'i420', 'range': 'limited', 'siting': 'left'}
    hd = yuv.parse_y4m_header(b'YUV4MPEG2 W352 H288 F25:1 Ip A128:117', 'foreman.y4m')                            # no C token: 4:2:0
    assert (hd['fmt'], hd['siting'], hd['range']) == ('i420', 'centre', 'limited')
    for tag, fmt, siting in (('C420', 'i420', 'centre'), ('C420jpeg', 'i420', 'centre'), ('C420p10', 'i420p10', 'centre'), ('C422', 'i422', 'left'),
                             ('C422p10', 'i422p10', 'left'), ('C444', 'i444', 'centre'), ('C444p10', 'i444p10', 'centre')):
        hd = yuv.parse_y4m_header(('YUV4MPEG2 W8 H4 F25:1 Ip A1:1 %s' % tag).encode(), 'a.y4m')
        assert (hd['fmt'], hd['siting']) == (fmt, siting), tag
    assert yuv.parse_y4m_header(b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 C422 XCHROMASITING=CENTRE', 'a.y4m')['siting'] == 'centre'
    assert yuv.parse_y4m_header(b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 C444 XCHROMASITING=LEFT', 'a.y4m')['siting'] == 'centre'


@pytest.mark.parametrize('line, text', [
    (b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 C420paldv', r'clip\.y4m: C420paldv \(top-left sited chroma\)'),
    (b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 Cmono', r'clip\.y4m: Cmono '), (b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 Cmono16', r'clip\.y4m: Cmono16 '),
    (b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 C411', r'clip\.y4m: C411 \(unknown chroma tag\)'), (b'YUV4MPEG2 W8 H4 F25:1 Ip A1:1 C420p12', r'clip\.y4m: C420p12'),
    (b'YUV4MPEG2 W8 H4 F25:1 It A1:1 C420jpeg', r'clip\.y4m: interlaced file \(It\)'), (b'YUV4MPEG2 W8 H4 F25:1 Ib A1:1', r'clip\.y4m: interlaced file \(Ib\)'),
    (b'YUV4MPEG2 W8 H4 F25:1 Im A1:1 C422', r'clip\.y4m: interlaced file \(Im\)'), (b'YUV4MPEG2 W8 H4 F25:1 Ip C422 XCHROMASITING=TOP', r'clip\.y4m: XCHROMASITING=TOP'),
    (b'YUV4MPEG2 W7 H4 F25:1 Ip C444', r'clip\.y4m: .*even'), (b'YUV4MPEG2 H4 F25:1 Ip C444', r'clip\.y4m: .*no W token')])
def test_y4m_refusals_name_the_file(tmp_path, line, text):
    with pytest.raises(ValueError, match=text) as e:
        yuv.parse_y4m_header(line, 'clip.y4m')
    assert '\n' not in str(e.value)
    path = str(tmp_path / 'clip.y4m')
    open(path, 'wb').write(line + b'\nFRAME\n' + bytes(64))
    with pytest.raises(ValueError, match=text):
        yuv.Y4MReader(path)
    with pytest.raises(ValueError, match=text):
        yuv.read_y4m(path)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_binding_and_exports_agree_abi_still_15(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    assert re.search(r'REFVSR_YUV_SAMPLING_420 = 0, REFVSR_YUV_SAMPLING_422 = 1, REFVSR_YUV_SAMPLING_444 = 2', src)
    assert re.search(r'REFVSR_YUV_SITING_CENTRE = 0, REFVSR_YUV_SITING_LEFT = 1', src)
    assert (hip.YUV_SAMPLING_420, hip.YUV_SAMPLING_422, hip.YUV_SAMPLING_444) == (0, 1, 2) == tuple(yuv.SAMPLINGS[k] for k in ('420', '422', '444'))
    assert (hip.YUV_SITING_CENTRE, hip.YUV_SITING_LEFT) == (0, 1) == (yuv.SITINGS['centre'], yuv.SITINGS['left'])
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', body))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(hip.EXPORTS) and declared == set(hip.EXPORTS)
    for name, nargs in (('refvsr_result_to_yuv', 11), ('refvsr_yuv_to_rgb', 11)):
        decl = re.search(r'int %s\(([^;]*)\);' % name, body).group(1)
        assert decl.count(',') + 1 == len(hip.SIGNATURES[name]) == nargs
    assert re.search(r'size_t refvsr_yuv_frame_bytes\(int h, int w, int yuv_fmt, int sampling\);', body)
    nm = subprocess.run(['nm', '-D', '--defined-only', hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r'\bT (refvsr_[a-z0-9_]+)$', nm, flags=re.M)) == set(hip.EXPORTS)
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15 and re.search(r'#define REFVSR_ABI_VERSION 15\b', src)
    sect = src[src.index("Y'CbCr 4:2:2 and 4:4:4 frames"):src.index('size_t refvsr_yuv_frame_bytes')]
    assert 'data_loader/utils.py:12-41' in sect and 'evaluation/eval_qual_quan.py:117-119' in sect and 'refvsr_amd/yuv.py' in sect
    for name in ('yuv.hip', 'yuv_in.hip'):
        kern = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', name)).read()
        code = re.sub(r'//.*', '', kern)
        assert '#pragma clang fp contract(off)' in kern and 'asm' not in code and 'atomic' not in code
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert '%d entry points' % len(hip.EXPORTS) in readme


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_yuv_to_rgb_rejects_bad_arguments_without_a_gpu(L):
    src, dst = _ptrs(4096), _ptrs(8192)
    coef = (ctypes.c_double * 9)(*yuv.decode_coefficients('i422'))
    err = lambda: L.refvsr_last_error().decode()
    f = L.refvsr_yuv_to_rgb
    for samp, sit in ((1, 0), (1, 1), (2, 0), (0, 1), (0, 0)):             # (4:2:0 / centre: refvsr_yuv420_to_rgb's own refusals)
        fmt = 1
        assert f(None, dst, 1, 8, 8, fmt, samp, sit, 0, coef, None) != 0 and 'null frame table' in err()
        assert f(src, None, 1, 8, 8, fmt, samp, sit, 0, coef, None) != 0 and 'null frame table' in err()
        assert f(_ptrs(0), dst, 1, 8, 8, fmt, samp, sit, 0, coef, None) != 0 and 'null pointer (frame 0)' in err()
        assert f(_ptrs(4096, 0), _ptrs(8192, 16384), 2, 8, 8, fmt, samp, sit, 0, coef, None) != 0 and 'null pointer (frame 1)' in err()
        for n in (0, -1, 17):
            assert f(src, dst, n, 8, 8, fmt, samp, sit, 0, coef, None) != 0 and '1..16 frames' in err()
        for h, w in ((7, 8), (8, 9), (0, 8), (8, 0), (1, 1), (-2, 8)):
            assert f(src, dst, 1, h, w, fmt, samp, sit, 0, coef, None) != 0 and 'even and positive' in err()
        assert f(src, dst, 1, 1 << 15, 1 << 15, fmt, samp, sit, 0, coef, None) != 0 and '2^29' in err()
        for mode in (-1, 2):
            assert f(src, dst, 1, 8, 8, fmt, samp, sit, mode, coef, None) != 0 and 'chroma' in err()
        assert f(src, dst, 1, 8, 8, fmt, samp, sit, 0, None, None) != 0 and 'null coefficients' in err()
        for d in (8196, 8200, 8193):
            assert f(src, _ptrs(d), 1, 8, 8, fmt, samp, sit, 0, coef, None) != 0 and '16 bytes' in err()
        assert f(_ptrs(4097), dst, 1, 8, 8, 3, samp, sit, 0, coef, None) != 0 and 'aligned to its samples' in err()
    for fmt in (-1, 4, 9):
        assert f(src, dst, 1, 8, 8, fmt, 1, 0, 0, coef, None) != 0 and 'unknown yuv format' in err()
    for samp in (-1, 3):
        assert f(src, dst, 1, 8, 8, 1, samp, 0, 0, coef, None) != 0 and 'sampling must be' in err()
    for sit in (-1, 2):
        assert f(src, dst, 1, 8, 8, 1, 2, sit, 0, coef, None) != 0 and 'siting must be' in err()          # 4:4:4 too: checked, then ignored
    for fmt in (0, 2):
        for samp in (1, 2):
            assert f(src, dst, 1, 8, 8, fmt, samp, 0, 0, coef, None) != 0 and 'semi-planar' in err() and '\n' not in err()


def test_result_to_yuv_rejects_bad_arguments_without_a_gpu(L):
    src, dst = _ptrs(4096), _ptrs(1 << 20)
    coef = (ctypes.c_double * 9)(*yuv.coefficients('i422'))
    err = lambda: L.refvsr_last_error().decode()
    f = L.refvsr_result_to_yuv
    for samp, sit in ((1, 0), (1, 1), (2, 1), (0, 1), (0, 0)):             # (4:2:0 / centre: refvsr_result_to_yuv420's own refusals)
        assert f(None, 0, dst, 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'null frame table' in err()
        assert f(src, 0, None, 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'null frame table' in err()
        assert f(src, 0, dst, 1, 8, 8, 1, samp, sit, None, None) != 0 and 'null coefficients' in err()
        for n in (0, -1, 17):
            assert f(src, 0, dst, n, 8, 8, 1, samp, sit, coef, None) != 0 and '1..16 frames' in err()
        for sfmt in (-1, 3, 0x13, 0x20):
            assert f(src, sfmt, dst, 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'unknown result format' in err()
        for h, w in ((7, 8), (8, 9), (0, 8), (8, 0), (-2, 8)):
            assert f(src, 0, dst, 1, h, w, 1, samp, sit, coef, None) != 0 and 'even and positive' in err()
        assert f(src, 0, dst, 1, 1 << 14, 1 << 14, 1, samp, sit, coef, None) != 0 and '32-bit offsets' in err()
        assert f(_ptrs(0), 0, dst, 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'null pointer (frame 0)' in err()
        assert f(src, 0, _ptrs(0), 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'null pointer (frame 0)' in err()
        assert f(_ptrs(4098), 0, dst, 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'aligned to their samples' in err()
        assert f(src, 2, _ptrs((1 << 20) + 1), 1, 8, 8, 3, samp, sit, coef, None) != 0 and 'aligned to their samples' in err()
        # a destination is refvsr_yuv_frame_bytes long: one that ends where the source begins is fine up to there, and overlaps beyond
        nb = L.refvsr_yuv_frame_bytes(8, 8, 1, samp)
        assert f(src, 2, _ptrs(4096 - nb + 1), 1, 8, 8, 1, samp, sit, coef, None) != 0 and 'destination 0 overlaps source 0' in err()
        assert f(_ptrs(4096, 8192), 2, _ptrs(1 << 20, (1 << 20) + nb - 1), 2, 8, 8, 1, samp, sit, coef, None) != 0 and 'destinations 0 and 1 overlap' in err()
    for fmt in (-1, 4, 9):
        assert f(src, 0, dst, 1, 8, 8, fmt, 1, 0, coef, None) != 0 and 'unknown yuv format' in err()
    for samp in (-1, 3):
        assert f(src, 0, dst, 1, 8, 8, 1, samp, 0, coef, None) != 0 and 'sampling must be' in err()
    for sit in (-1, 2):
        assert f(src, 0, dst, 1, 8, 8, 1, 2, sit, coef, None) != 0 and 'siting must be' in err()
    for fmt in (0, 2):
        for samp in (1, 2):
            assert f(src, 0, dst, 1, 8, 8, fmt, samp, 1, coef, None) != 0 and 'semi-planar' in err() and '\n' not in err()


def _refusals(L, entry, cases, good, order, extra=()):
    """[(prefix, text behind it)] of `entry` for every case: `good` with the case's arguments replaced, passed in `order` (`extra`: the
    (position, value) pairs of the arguments only the general entry has)."""
    out = []
    for case in cases:
        args = [dict(good, **case)[k] for k in order] + [None]                 # (the stream)
        for pos, val in extra:
            args.insert(pos, val)
        assert entry(*args) != 0, case
        out.append(tuple(L.refvsr_last_error().decode().split(': ', 1)))
    return out


def test_both_entries_of_a_direction_refuse_in_the_same_words(L):
    """One list of bad arguments per direction, fed to the 4:2:0 entry and to the general entry under every sampling and siting it
    launches: the text behind the prefix is the same.  (What the 4:2:0 entry cannot say -- a sampling, a siting -- is not in the
    lists: the two tests above hold those.)"""
    hw_bad = [dict(h=h, w=w) for h, w in ((7, 8), (8, 9), (0, 8), (8, 0), (1, 1), (-2, 8))]
    out_good = dict(src=_ptrs(4096), sfmt=0, dst=_ptrs(1 << 20), n=1, h=8, w=8, fmt=1, coef=(ctypes.c_double * 9)(*yuv.coefficients('i420')))
    out_bad = ([dict(src=None), dict(dst=None), dict(coef=None)] + [dict(n=n) for n in (0, -1, 17)] + [dict(sfmt=s) for s in (-1, 3, 0x13, 0x20)]
               + [dict(fmt=f) for f in (-1, 4, 9)] + hw_bad + [dict(h=1 << 14, w=1 << 14), dict(src=_ptrs(0)), dict(dst=_ptrs(0)),
                  dict(src=_ptrs(4096, 0), dst=_ptrs(1 << 20, 1 << 21), n=2), dict(src=_ptrs(4098)), dict(sfmt=2, dst=_ptrs((1 << 20) + 1), fmt=3),
                  dict(sfmt=2, dst=_ptrs(4096)), dict(src=_ptrs(4096, 8192), sfmt=2, dst=_ptrs(1 << 20, (1 << 20) + 16), n=2)])
    in_good = dict(src=_ptrs(4096), dst=_ptrs(8192), n=1, h=8, w=8, fmt=1, chroma=0, coef=(ctypes.c_double * 9)(*yuv.decode_coefficients('i420')))
    in_bad = ([dict(src=None), dict(dst=None), dict(src=_ptrs(0)), dict(dst=_ptrs(0)), dict(src=_ptrs(4096, 0), dst=_ptrs(8192, 16384), n=2)]
              + [dict(n=n) for n in (0, -1, 17)] + hw_bad + [dict(h=1 << 15, w=1 << 15)] + [dict(fmt=f) for f in (-1, 4, 9)]
              + [dict(chroma=c) for c in (-1, 2)] + [dict(coef=None)] + [dict(dst=_ptrs(d)) for d in (8196, 8200, 8193)] + [dict(src=_ptrs(4097), fmt=3)])
    for plain, general, names, good, bad, order in (
            (L.refvsr_result_to_yuv420, L.refvsr_result_to_yuv, ('result_to_yuv420', 'result_to_yuv'), out_good, out_bad,
             ('src', 'sfmt', 'dst', 'n', 'h', 'w', 'fmt', 'coef')),
            (L.refvsr_yuv420_to_rgb, L.refvsr_yuv_to_rgb, ('yuv420_to_rgb', 'yuv_to_rgb'), in_good, in_bad,
             ('src', 'dst', 'n', 'h', 'w', 'fmt', 'chroma', 'coef'))):
        want = _refusals(L, plain, bad, good, order)
        assert all(prefix == names[0] and text for prefix, text in want), want
        at = order.index('fmt') + 1                                            # sampling, siting stand behind the format
        for samp, sit in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)):
            got = _refusals(L, general, bad, good, order, ((at, samp), (at + 1, sit)))
            assert [t for _, t in got] == [t for _, t in want], (names[1], samp, sit)
            assert all(prefix in names for prefix, _ in got), got


# ------------------------------------------------------------------------------------------------ config, engine entry, videorun
def test_config_fields_are_validated_while_the_feature_is_off():
    from refvsr_amd import get_config
    from refvsr_amd.model import _input_yuv
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    assert (cfg.result_yuv, cfg.input_yuv, cfg.yuv_siting, cfg.input_yuv_siting) == (None, None, 'centre', 'centre')
    assert _input_yuv(cfg) is None
    for fmt in cc.NEW_FORMATS:
        assert yuv.resolve(fmt, 'bt601', 'full') == (fmt, 'bt601', 'full')
        assert yuv.resolve_input(fmt, 'bt601', 'full', 'nearest') == (fmt, 'bt601', 'full', 'nearest')
    assert yuv.resolve_input('nv12', siting='centre') == ('nv12', 'bt709', 'limited', 'bilinear')              # today's tuple
    assert yuv.resolve_input('nv12', siting='left') == ('nv12', 'bt709', 'limited', 'bilinear', 'left')
    assert yuv.resolve_input('i422', siting='left') == ('i422', 'bt709', 'limited', 'bilinear', 'left')
    assert yuv.resolve_input('i444', siting='left') == ('i444', 'bt709', 'limited', 'bilinear')                # 4:4:4: nothing to site
    assert yuv.resolve_siting(None) == 'centre' and yuv.resolve_siting('left') == 'left'
    with pytest.raises(ValueError, match="input_yuv_siting must be 'centre' or 'left'"):
        yuv.resolve_input(None, siting='top')
    with pytest.raises(ValueError, match="yuv_siting must be 'centre' or 'left'"):
        yuv.resolve_siting('top-left')
    for field in ('result_yuv', 'input_yuv'):
        with pytest.raises(ValueError, match='%s must be None' % field):
            (yuv.resolve if field == 'result_yuv' else yuv.resolve_input)('i440')
    cfg.input_yuv_siting = 'top'
    with pytest.raises(ValueError, match='input_yuv_siting'):
        _input_yuv(cfg)
    cfg.input_yuv_siting, cfg.input_yuv = 'left', 'i422p10'
    assert _input_yuv(cfg) == 'i422p10'
    # the engine checks both fields at its construction, the features off
    src = open(os.path.join(ROOT, 'refvsr_amd', 'engine.py')).read()
    assert "yuv.resolve_siting(getattr(config, 'yuv_siting', None))" in src and "getattr(config, 'input_yuv_siting', None))" in src


def test_window_checks_and_source_keys():
    from refvsr_amd import inputs, ops
    from refvsr_amd.model import _inputs

    class Cuda(torch.Tensor):                         # (the check asks is_cuda; nothing here touches a device)
        is_cuda = True

    def cuda(x):
        return x.as_subclass(Cuda)
    w422, w444 = cuda(torch.zeros(1, 3, 36, 26, dtype=torch.uint8)), cuda(torch.zeros(1, 3, 54, 26, dtype=torch.uint16))
    assert _inputs(w422, w422, 'forward', strict=True, input_yuv='i422')[0] is w422
    assert _inputs(w444, w444, 'forward', input_yuv='i444p10')[0] is w444
    assert _inputs(w422[0], w422[0], 'phase_a_group', input_yuv='i422', dim=4)[0].shape == (3, 36, 26)
    for fmt, rows, bad in (('i422', '2h', cuda(torch.zeros(1, 3, 38, 26, dtype=torch.uint8))),              # 2h = 38: h odd
                           ('i422', '2h', w444), ('i444p10', '3h', w422),                                 # the other sample type
                           ('i444p10', '3h', cuda(torch.zeros(1, 3, 51, 26, dtype=torch.uint16))),        # 3h = 51: h odd
                           ('i444', '3h', cuda(torch.zeros(1, 3, 54, 25, dtype=torch.uint8))),            # odd w
                           ('i422', '2h', cuda(torch.zeros(1, 3, 3, 18, 26, dtype=torch.uint8)))):        # an RGB window
        with pytest.raises(RuntimeError, match=r"input_yuv = '%s'.*\[n, t, %s, w\]" % (fmt, rows)) as e:
            _inputs(bad, bad, 'forward', input_yuv=fmt)
        assert '\n' not in str(e.value)
    assert ops.yuv_window_kind(torch.zeros(36, 26, dtype=torch.uint8), 'i422') == ('yuv', 'i422')
    assert ops.yuv_window_kind(torch.zeros(27, 26, dtype=torch.uint8), 'i422') is None
    assert ops.yuv_geometry(torch.zeros(5, 36, 26), 'i422') == (18, 26) == ops.yuv_geometry(torch.zeros(5, 54, 26), 'i444p10') == ops.yuv_geometry(torch.zeros(5, 27, 26))
    # the window cache's key holds format (so sampling) and siting
    x = torch.zeros(3, 36, 26, dtype=torch.uint8)
    keys = [inputs.source_of(x, x, yuv.resolve_input(f, siting=s)).key for f, s in (('i422', 'left'), ('i422', 'centre'), ('i420', 'left'), ('i420', 'centre'), ('i444', 'left'))]
    assert len(set(keys)) == 5 and keys[3] == ('yuv', 'i420', 'bt709', 'limited', 'bilinear')
    assert inputs.source_of(x, x, yuv.resolve_input('i422', siting='left')).geometry(x) == (18, 26)


def _write(path, n, h, w, fmt, siting=None, seed=0):
    rs = np.random.RandomState(seed)
    with yuv.Y4MWriter(path, h, w, fmt, (25, 1), 'limited', siting) as wr:
        for _ in builtins_range(n):
            wr.write(cc.random_codes(rs, h, w, fmt, dirty=False))
    return path


def test_videorun_arguments_and_pairs(tmp_path):
    from refvsr_amd import videorun
    a = _write(str(tmp_path / 'a.y4m'), 3, 16, 24, 'i420', 'left')
    base = ['--lr', a, '--ref', a, '--out', str(tmp_path / 'o.y4m')]
    cfg, _ = videorun.build_config(base)
    assert (cfg.EVAL.in_siting, cfg.EVAL.out_chroma, cfg.EVAL.out_siting) == (None, None, None)
    cfg, _ = videorun.build_config(base + ['--in_siting', 'centre', '--out_chroma', '444', '--out_siting', 'left', '--video_depth', '10'])
    assert (cfg.EVAL.in_siting, cfg.EVAL.out_chroma, cfg.EVAL.out_siting) == ('centre', '444', 'left')
    for extra in (['--in_siting', 'top'], ['--out_chroma', '411'], ['--out_chroma', '440'], ['--out_siting', 'topleft']):
        with pytest.raises(SystemExit):
            videorun.build_config(base + extra)
    # the two files must agree in sampling, depth and siting
    for other, text in ((_write(str(tmp_path / 'c.y4m'), 3, 16, 24, 'i420', 'centre'), r'format differs \(i420 with left- and centre-sited'),
                        (_write(str(tmp_path / 'd.y4m'), 3, 16, 24, 'i422'), r'format differs \(i420 and i422\)'),
                        (_write(str(tmp_path / 'e.y4m'), 3, 16, 24, 'i444p10'), r'format differs \(i420 and i444p10\)')):
        with pytest.raises(ValueError, match=text) as e:
            videorun.open_pair(a, other)
        assert '\n' not in str(e.value)
        with pytest.raises(ValueError, match=text):
            videorun.run(videorun.build_config(base)[0], a, other, str(tmp_path / 'o.y4m'))        # (refused before anything is built)
    assert not os.path.exists(str(tmp_path / 'o.y4m'))
    lr, ref = videorun.open_pair(a, str(tmp_path / 'c.y4m'), 'left')       # --in_siting declares one siting for both
    assert (lr.siting, ref.siting) == ('left', 'left')
    lr.close()
    ref.close()
    bad = str(tmp_path / 'paldv.y4m')
    open(bad, 'wb').write(b'YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420paldv\n')
    with pytest.raises(ValueError, match=r'paldv\.y4m: C420paldv'):
        videorun.open_pair(a, bad)
    # configure: the output keeps the input's sampling and siting unless told otherwise; 4:2:2 output is left-sited unless told
    for fmt, siting, opts, want in (('i420', 'left', {}, ('i420', 'left', 'i420', 'left')),
                                    ('i420', 'centre', {}, ('i420', 'centre', 'i420', 'centre')),
                                    ('i420', 'centre', {'out_chroma': '422'}, ('i420', 'centre', 'i422', 'left')),
                                    ('i420', 'centre', {'out_chroma': '422', 'out_siting': 'centre'}, ('i420', 'centre', 'i422', 'centre')),
                                    ('i422p10', 'left', {}, ('i422p10', 'left', 'i422p10', 'left')),
                                    ('i422', 'left', {'video_depth': 10, 'out_chroma': '444'}, ('i422', 'left', 'i444p10', 'left')),
                                    ('i444', None, {'out_chroma': '420'}, ('i444', 'centre', 'i420', 'centre')),
                                    ('i420p10', 'left', {'video_depth': 8, 'out_siting': 'centre'}, ('i420p10', 'left', 'i420', 'centre'))):
        p = _write(str(tmp_path / 'x.y4m'), 1, 16, 24, fmt, siting)
        with yuv.Y4MReader(p) as rd:
            cfg, _ = videorun.build_config(base)
            for k, v in opts.items():
                setattr(cfg.EVAL, k, v)
            videorun.configure(cfg, rd)
            assert (cfg.input_yuv, cfg.input_yuv_siting, cfg.result_yuv, cfg.yuv_siting) == want, (fmt, siting, opts)
            cfg.EVAL.out_chroma = '411'
            with pytest.raises(ValueError, match='--out_chroma'):
                videorun.configure(cfg, rd)


def test_fake_ops_shapes_and_dtypes():
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert {'result_to_yuv', 'yuv_to_rgb'} <= set(t.OP_NAMES) and hasattr(torch.ops.refvsr, 'result_to_yuv') and hasattr(torch.ops.refvsr, 'yuv_to_rgb')
    assert str(torch.ops.refvsr.yuv_to_rgb.default._schema) == \
        'refvsr::yuv_to_rgb(Tensor x, SymInt h, SymInt w, str fmt, str matrix, str range, str chroma, str siting) -> Tensor'
    assert str(torch.ops.refvsr.result_to_yuv.default._schema) == 'refvsr::result_to_yuv(Tensor frames, str fmt, str matrix, str range, str siting) -> Tensor'
    with FakeTensorMode():
        for fmt, rows, dt in (('i422', 36, torch.uint8), ('i444p10', 54, torch.uint16), ('nv12', 27, torch.uint8)):
            x = torch.empty((2, 5, rows, 26), dtype=dt, device='cuda')
            y = torch.ops.refvsr.yuv_to_rgb(x, 18, 26, fmt, 'bt709', 'limited', 'bilinear', 'left')
            assert y.shape == (2, 5, 3, 18, 26) and y.dtype == torch.float32
            r = torch.empty((4, 3, 18, 26), dtype=torch.float16, device='cuda')
            z = torch.ops.refvsr.result_to_yuv(r, fmt, 'bt601', 'full', 'centre')
            assert z.shape == (4, rows, 26) and z.dtype == dt
        with pytest.raises(RuntimeError, match='siting'):
            torch.ops.refvsr.result_to_yuv(r, 'i422', 'bt601', 'full', 'top')
        with pytest.raises(RuntimeError, match='rows'):
            torch.ops.refvsr.yuv_to_rgb(torch.empty((2, 27, 26), dtype=torch.uint8, device='cuda'), 18, 26, 'i422', 'bt709', 'limited', 'bilinear', 'left')
