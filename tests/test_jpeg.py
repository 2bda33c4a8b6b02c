"""The JPEG model refvsr_amd/jpeg.py on the CPU: Pillow reads what it writes and finds the quality Pillow's own encoder gives, the file
has the structure the text promises, every crafted frame of tests/jpeg_cases.py takes the path it is named after, every wrong reading
of the text changes the bytes of the frame built for it, and the argument checks of ops.jpeg_encode and videorun answer without a GPU."""
import io
import warnings

import numpy as np
import pytest

import jpeg_cases as jc
from refvsr_amd import jpeg, yuv


def decode(data):
    """Pillow's decode of a file, any warning an error: (uint8 [h, w, 3], the image)."""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        im = Image.open(io.BytesIO(data))
        im.load()
    return np.asarray(im), im


def segments(data):
    """[(marker, body)] up to and including SOS, and the offset of the entropy-coded data."""
    assert data[:2] == b'\xff\xd8'
    out, p = [(0xd8, b'')], 2
    while True:
        assert data[p] == 0xff
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], 'big')
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xda:
            return out, p


# ------------------------------------------------------------------------------------------------ validity
@pytest.mark.parametrize('h,w', jc.SIZES)
@pytest.mark.parametrize('fmt', jc.FORMATS)
def test_pillow_reads_the_matrix(fmt, h, w):
    buf = jc.matrix_frame(h, w, fmt)
    for q in jc.QUALITIES:
        for r in jc.restarts(h, w, fmt):
            data = jpeg.encode_model(buf, h, w, fmt, q, r)
            px, im = decode(data)
            assert im.size == (w, h) and im.mode == 'RGB' and im.format == 'JPEG' and px.shape == (h, w, 3)
            assert data[:len(jpeg.header(h, w, fmt, q, r))] == jpeg.header(h, w, fmt, q, r) and data[-2:] == jpeg.EOI
            assert len(data) - len(jpeg.header(h, w, fmt, q, r)) - 2 <= jpeg.capacity(h, w, fmt, r)


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / max(float(((a.astype(np.float64) - b) ** 2).mean()), 1e-12))


QUALITY_MARGIN = 0.12       # dB: twice the largest shortfall measured (0.055 dB), rounded up


@pytest.mark.parametrize('source', ['natural 136x240', 'natural 30x50', 'noise 30x50'])
def test_quality_is_pillows(source):
    """PSNR against the RGB source of Pillow's decode of our file >= that of Pillow's own save(quality, subsampling) minus a margin.
    Measured shortfalls (positive: ours is lower), dB, at quality 1 / 50 / 75 / 90 / 100:
      natural 136x240  i420 +0.001 +0.003 +0.017 +0.005 +0.011   i444 +0.000 -0.005 -0.008 -0.009 -0.342
      natural 30x50    i420 +0.018 +0.009 +0.044 +0.054 -0.050   i444 +0.000 +0.003 -0.013 -0.049 -0.459
      noise 30x50      i420 -0.008 -0.010 +0.005 -0.005 +0.001   i444 +0.000 +0.005 +0.010 +0.055 -0.378
    The expectation of a margin of 0 does not hold: the float64 transform wins where the transform decides (4:4:4 at quality 100, by
    0.3 - 0.5 dB), but Pillow converts RGB to Y'CbCr and subsamples chroma in its own integer arithmetic while our frames come from
    yuv.rgb_to_yuv, and either can come out a few hundredths of a dB ahead.  The largest shortfall is 0.055 dB; the margin is twice
    that."""
    from PIL import Image
    kind, size = source.split()
    h, w = (int(v) for v in size.split('x'))
    rgb = jc.natural_rgb(h, w, seed=3 if h > 100 else 4) if kind == 'natural' else jc.noise_rgb(h, w, seed=1)
    for fmt, sub in (('i420', 2), ('i444', 0)):
        for q in jc.QUALITIES:
            ours = decode(jpeg.encode_model(jc.to_yuv(rgb, fmt), h, w, fmt, q, 4))[0].transpose(2, 0, 1)
            b = io.BytesIO()
            Image.fromarray(rgb.transpose(1, 2, 0)).save(b, 'JPEG', quality=q, subsampling=sub)
            pil = decode(b.getvalue())[0].transpose(2, 0, 1)
            short = psnr(pil, rgb) - psnr(ours, rgb)
            print('%s %s q%d: ours %.3f dB, Pillow %.3f dB, shortfall %+.3f dB' % (source, fmt, q, psnr(ours, rgb), psnr(pil, rgb), short))
            assert short <= QUALITY_MARGIN, (source, fmt, q, short)


def test_tables_are_the_ones_pillow_writes():
    """Pillow's encoder writes the Annex K tables and scales them the customary way: our numbers are its numbers."""
    from PIL import Image
    im = Image.fromarray(jc.noise_rgb(16, 16).transpose(1, 2, 0))
    for q in (1, 10, 49, 50, 51, 75, 90, 100):
        b = io.BytesIO()
        im.save(b, 'JPEG', quality=q, subsampling=2)
        segs, _ = segments(b.getvalue())
        theirs = b''.join(body for m, body in segs if m == 0xdb)
        ours = b''.join(body for m, body in segments(jpeg.header(16, 16, 'i420', q, 1))[0] if m == 0xdb)
        assert ours == theirs, q
        assert sorted(body for m, body in segs if m == 0xc4) == sorted(
            body for m, body in segments(jpeg.header(16, 16, 'i420', q, 1))[0] if m == 0xc4) or b''.join(
            body for m, body in segs if m == 0xc4) == b''.join(body for m, body in segments(jpeg.header(16, 16, 'i420', q, 1))[0] if m == 0xc4)
    for code, length in jpeg.huffman_tables():
        used = [(int(length[s]), int(code[s])) for s in range(256) if length[s]]
        assert len(set(used)) == len(used) and sum(2.0 ** -l for l, _ in used) < 1.0          # a prefix code, the all-ones word left free
    assert [int((l > 0).sum()) for _, l in jpeg.huffman_tables()] == [12, 162, 12, 162]
    assert jpeg.MAX_BLOCK_BITS == 11 + 11 + 63 * (16 + 10) and max(int(l.max()) for _, l in jpeg.huffman_tables()) == 16
    assert max(int(jpeg.huffman_tables()[k][1][:12].max()) for k in (0, 2)) == 11


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize('fmt', jc.FORMATS)
def test_marker_order_dri_and_restart_markers(fmt):
    buf, h, w, _, q, _ = jc.crafted()['rst_cycle']
    buf = buf if fmt == 'i420' else jc.matrix_frame(h, w, fmt)
    for r in (1, 3, 7):
        data = jpeg.encode_model(buf, h, w, fmt, q, r)
        segs, p = segments(data)
        assert [m for m, _ in segs] == [0xd8, 0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
        assert segs[1][1] == b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
        assert [b[0] for m, b in segs if m == 0xdb] == [0, 1] and [b[0] for m, b in segs if m == 0xc4] == [0x00, 0x10, 0x01, 0x11]
        sof = segs[4][1]
        assert sof[0] == 8 and int.from_bytes(sof[1:3], 'big') == h and int.from_bytes(sof[3:5], 'big') == w
        assert sof[5:] == bytes([3, 1, 0x22 if fmt == 'i420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert int.from_bytes(segs[9][1], 'big') == r
        assert segs[10][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
        ecs = data[p:-2]
        n = jpeg.intervals(h, w, fmt, r)
        assert n >= 9 or r > 1
        marks = [ecs[i + 1] for i in range(len(ecs) - 1) if ecs[i] == 0xff and ecs[i + 1] != 0x00]
        assert marks == [0xd0 + (i & 7) for i in range(n - 1)]                # RST0 .. RST7 in a cycle, nothing else behind an 0xFF
        assert ecs[-1] != 0xff and data[-2:] == jpeg.EOI
        assert ecs == jpeg.entropy_data(buf, h, w, fmt, q, r)
    assert jpeg.intervals(h, w, fmt, 1) >= 9


def test_restart_past_the_frame_and_default():
    buf, h, w, fmt = jc.matrix_frame(18, 34, 'i420'), 18, 34, 'i420'
    data = jpeg.encode_model(buf, h, w, fmt, 75, 65535)
    segs, p = segments(data)
    assert int.from_bytes(segs[9][1], 'big') == 65535 and b'\xff\xd0' not in data[p:-2]
    assert jpeg.encode_model(buf, h, w, fmt, 75) == jpeg.encode_model(buf, h, w, fmt, 75, jpeg.DEFAULT_RESTART)
    assert jpeg.encode_model(buf, h, w, fmt) == jpeg.encode_model(buf, h, w, fmt, 90, None)


def test_split_mjpeg_round_trip(tmp_path):
    files = [jpeg.encode_model(b, h, w, fmt, q, r) for b, h, w, fmt, q, r in (jc.crafted()[k] for k in ('ff_bytes', 'rst_cycle', 'clamp', 'zrl'))]
    path = str(tmp_path / 'x.mjpeg')
    with jpeg.MJPEGWriter(path) as wr:
        for f in files:
            wr.write(f)
        wr.write(np.frombuffer(files[0], np.uint8))                           # (a buffer of the ring: any bytes-like object)
    assert wr.frames == 5 and wr.bytes == sum(len(f) for f in files) + len(files[0])
    data = open(path, 'rb').read()
    assert data == b''.join(files) + files[0] and jpeg.split_mjpeg(data) == files + [files[0]]
    sink = io.BytesIO()
    wr = jpeg.MJPEGWriter(sink)
    wr.write(files[1])
    wr.close()
    assert sink.getvalue() == files[1] and not sink.closed
    with pytest.raises(ValueError, match='one complete JPEG file'):
        jpeg.MJPEGWriter(io.BytesIO()).write(files[0][:-2])
    with pytest.raises(ValueError, match='no EOI'):
        jpeg.split_mjpeg(files[0][:-2])
    with pytest.raises(ValueError, match='SOI expected at byte %d' % len(files[0])):
        jpeg.split_mjpeg(files[0] + b'junk')


# ------------------------------------------------------------------------------------------------ crafted frames take their paths
def syms(name):
    buf, h, w, fmt, q, r = jc.crafted()[name]
    return jpeg.symbols(buf, h, w, fmt, q, r)


def luma_blocks(name):
    """The symbol lists of the luma blocks of a crafted 4:4:4 frame, in coding order."""
    return [s for iv in syms(name) for c, s in iv if c == 0]


def ratios(name):
    """F / Q of the luma blocks of a crafted 4:4:4 frame: float64 [blocks, 8, 8]."""
    buf, h, w, fmt, q, _ = jc.crafted()[name]
    y = yuv.planes(buf, h, w, fmt)[0]
    return jpeg.fdct(jpeg.blocks(y).astype(np.float64) - 128.0)[0] / jpeg.quant_tables(q)[0].reshape(8, 8).astype(np.float64)


def test_ties_round_to_even():
    v = ratios('ties')
    assert [float(v[k, 0, 0]) for k in range(4)] == [1.5, -1.5, 8.5, -8.5]          # constant blocks: DC = 8 (v - 128) exactly
    assert float(v[4, 0, 4]) == 0.5 and float(v[5, 0, 4]) == -0.5                    # the column patterns
    co = jpeg.coefficients(*jc.crafted()['ties'][:5])[0]
    assert [int(co[k, 0, 0]) for k in range(4)] == [2, -2, 8, -8]
    assert int(co[4, 0, jpeg.ZIGZAG.index(4)]) == 0 and int(co[5, 0, jpeg.ZIGZAG.index(4)]) == 0
    # a constant block of +-1 is no tie in float64, which is why +-0.5 comes from a pattern
    assert float(jpeg.fdct(np.full((8, 8), 1.0))[0, 0]) != 8.0


def test_zero_runs():
    b = luma_blocks('zrl')
    assert b[0] == [(2, 3), (0x02, 2), (jpeg.ZRL, 0), (0x21, -1), (jpeg.EOB, 0)]
    b = luma_blocks('zrl_twice')
    assert b[0] == [(2, -2), (jpeg.ZRL, 0), (jpeg.ZRL, 0), (0x71, 1), (jpeg.EOB, 0)]
    assert b[1] == [(2, 2), (jpeg.ZRL, 0), (jpeg.ZRL, 0), (jpeg.ZRL, 0), (0x11, -1), (jpeg.EOB, 0)]


def test_last_position_has_no_eob():
    b = luma_blocks('last_position')
    assert b[0][-1] == (0xe1, 1) and b[0].count((jpeg.ZRL, 0)) == 3 and (jpeg.EOB, 0) not in b[0]
    assert b[1][-1][1] == -1 and (jpeg.EOB, 0) not in b[1]
    assert all(s[-1] == (jpeg.EOB, 0) for iv in syms('last_position') for c, s in iv if c != 0)


def test_zero_block_after_a_dc_and_equal_dcs():
    b = luma_blocks('zero_after_dc')
    assert b[1] == [(b[1][0][0], -b[0][0][1]), (jpeg.EOB, 0)] and b[1][0][1] != 0      # all-zero block: its DC difference, EOB only
    assert b[2] == [(0, 0), (jpeg.EOB, 0)]                                              # and a difference of 0: size 0
    b = luma_blocks('dc_equal')                                                          # R = 2: the predictor is reset ahead of block 2
    assert b[1][0] == (0, 0) and b[2][0] == b[0][0] and b[0][0][1] != 0 and b[3][0][1] != 0


def test_largest_magnitudes_at_quality_100():
    """The frame built for the clamps reaches the largest values 8-bit samples can give -- AC +-1020 (size 10), DC -1024 (size 11) and
    1016 (size 10) -- which lie inside the clamps: [-1023, 1023] and [-1024, 1023] never bind on 8-bit input (jpeg_cases.crafted has the bound)."""
    v = ratios('clamp')
    assert round(float(v[0, 4, 4]), 6) == 1020.0 and round(float(v[1, 4, 4]), 6) == -1020.0
    assert round(float(v[2, 0, 0]), 6) == -1024.0 and round(float(v[3, 0, 0]), 6) == 1016.0      # (-1024.0000000000002 in float64)
    C = jpeg.dct_table()
    assert float(np.abs(C).sum(axis=1).max()) ** 2 * 128.0 < 1024.5                      # no AC coefficient can pass 1024
    b = luma_blocks('clamp')
    vals = [val for s in b[:2] for _, val in s[1:]]
    assert max(vals) == 1020 and min(vals) == -1020 and {sym & 15 for s in b[:2] for sym, val in s[1:] if abs(val) == 1020} == {10}
    assert b[2][0] == (11, -1024) and b[3][0] == (10, 1016)                              # (R = 1: every DC is coded against 0)
    assert [(11, -1024), (jpeg.EOB, 0)] in [s for iv in syms('clamp') for c, s in iv if c == 1]      # chroma too (Cb = 0)


def test_ff_bytes_in_data_and_in_padding():
    buf, h, w, fmt, q, r = jc.crafted()['ff_bytes']
    iv = jpeg.symbols(buf, h, w, fmt, q, r)[0]
    data = jpeg.interval_bytes(iv)
    assert data.endswith(b'\xff\x00') and data != jpeg.interval_bytes(iv, ('no_pad_stuffing',))     # the padded byte is 0xFF
    assert data != jpeg.interval_bytes(iv, ('pad_zeros',))                                          # ... and made by padding
    assert b'\xff\x00' in data[:-2]                                                                 # a data byte 0xFF
    assert jpeg.entropy_data(buf, h, w, fmt, q, r).startswith(data + b'\xff\xd0')
    decode(jpeg.encode_model(buf, h, w, fmt, q, r))


@pytest.mark.parametrize('name', ['partial_420', 'partial_444'])
def test_partial_mcus_repeat_the_edge(name):
    buf, h, w, fmt, q, r = jc.crafted()[name]
    my, mx, bpm = jpeg.geometry(h, w, fmt)
    m = 16 if fmt == 'i420' else 8
    assert h % m and w % m and (my, mx) == (-(-h // m), -(-w // m))
    y = yuv.planes(buf, h, w, fmt)[0]
    e = jpeg.extend(y, m)
    assert e.shape == (my * m, mx * m) and (e[:h, :w] == y).all() and (e[h:, :w] == y[-1]).all() and (e[:, w:] == e[:, w - 1:w]).all()
    px, _ = decode(jpeg.encode_model(buf, h, w, fmt, q, r))
    ref = yuv.yuv_to_rgb(buf, h, w, fmt, 'bt601', 'full', 'bilinear', 'centre')
    assert psnr(px.transpose(2, 0, 1), ref * 255.0) > 30.0                                          # edges included


@pytest.mark.parametrize('wrong', jpeg.WRONG_MODELS)
def test_wrong_readings_change_the_bytes(wrong):
    """Each wrong reading of the text changes the file of the crafted frame built for it -- and only such a reading does."""
    buf, h, w, fmt, q, r = jc.crafted()[jc.CONTROLS[wrong]]
    right = jpeg.encode_model(buf, h, w, fmt, q, r)
    assert right == jpeg.encode_model(buf, h, w, fmt, q, r, wrong=())
    assert jpeg.encode_model(buf, h, w, fmt, q, r, wrong=(wrong,)) != right


# ------------------------------------------------------------------------------------------------ arguments
def test_model_argument_checks():
    buf = jc.matrix_frame(8, 8, 'i420')
    for bad, text in ((dict(fmt='i422'), "'i420' or 'i444'"), (dict(fmt='nv12'), "'i420' or 'i444'"), (dict(fmt='jpg'), 'yuv format must be'),
                      (dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(quality=90.0), 'quality'), (dict(quality=True), 'quality'),
                      (dict(restart=0), 'restart'), (dict(restart=65536), 'restart'), (dict(restart=2.0), 'restart'),
                      (dict(h=7), 'even'), (dict(w=0), 'even'), (dict(h=65536, w=2), '65535'), (dict(h=16), 'frame is uint8')):
        kw = dict(dict(h=8, w=8, fmt='i420', quality=90, restart=None), **bad)
        with pytest.raises(ValueError, match=text):
            jpeg.encode_model(buf, kw['h'], kw['w'], kw['fmt'], kw['quality'], kw['restart'])
    with pytest.raises(ValueError, match='frame is uint8'):
        jpeg.encode_model(buf.astype(np.uint16), 8, 8, 'i420')
    assert jpeg.capacity(16, 16, 'i420', 1) == 2 * ((6 * jpeg.MAX_BLOCK_BITS + 7) // 8) + 2
    assert jpeg.capacity(16, 32, 'i444', 3) == 2 * (2 * ((9 * jpeg.MAX_BLOCK_BITS + 7) // 8) + 2) + 2 * ((6 * jpeg.MAX_BLOCK_BITS + 7) // 8) + 2


def test_ops_argument_checks_need_no_gpu():
    """Format, quality, restart and size are ValueErrors; dtype, shape and -- last -- the device RuntimeErrors, as in result_to_yuv."""
    import torch
    from refvsr_amd import ops
    x = torch.zeros((2, 12, 8), dtype=torch.uint8)
    for fn in (ops.jpeg_encode, ops.jpeg_encode_device):
        for args, exc, text in (((x, 8, 8, 'i422'), ValueError, "'i420' or 'i444'"), ((x, 8, 8, 'i420p10'), ValueError, "'i420' or 'i444'"),
                                ((x, 8, 8, 'bmp'), ValueError, 'yuv format must be'),
                                ((x, 8, 8, 'i420', 0), ValueError, 'quality must be an integer 1..100'),
                                ((x, 8, 8, 'i420', 90, 0), ValueError, 'restart interval must be None or an integer 1..65535'),
                                ((x, 8, 7, 'i420'), ValueError, 'even'), ((x, 8.0, 8, 'i420'), ValueError, 'h and w must be integers'),
                                ((x, 8, 8, 'i444'), RuntimeError, r'i444 frames at 8 x 8 are \[.., 24, 8\]'),
                                ((x.to(torch.int16), 8, 8, 'i420'), RuntimeError, 'frames are torch.uint8'),
                                (([x[0], x[1, :6]], 8, 8, 'i420'), RuntimeError, r'one dense \[12, 8\] buffer'),
                                (([x[0].t().contiguous().t()], 8, 8, 'i420'), RuntimeError, r'one dense \[12, 8\] buffer'),
                                (([], 8, 8, 'i420'), RuntimeError, 'at least one frame'),
                                ((x, 8, 8, 'i420'), RuntimeError, 'frames must lie on one GPU')):
            with pytest.raises(exc, match=text):
                fn(*args)


def test_custom_op_is_registered():
    import torch
    import refvsr_amd.torch_ops as t
    assert 'jpeg_encode' in t.OP_NAMES
    schema = str(torch.ops.refvsr.jpeg_encode.default._schema)
    assert 'Tensor x, SymInt h, SymInt w, str fmt, SymInt quality, SymInt restart' in schema and schema.endswith('-> (Tensor, Tensor, Tensor)')


def test_videorun_options_and_refusals():
    from refvsr_amd import videorun
    base = ['--lr', 'a.y4m', '--ref', 'b.y4m']
    for out, extra, want in (('x.mjpeg', [], 'mjpeg'), ('x.MJPG', [], 'mjpeg'), ('x.y4m', [], 'y4m'), ('x.jpg', [], 'y4m'),
                             ('x.y4m', ['--out_format', 'mjpeg'], 'mjpeg'), ('x.mjpeg', ['--out_format', 'y4m'], 'y4m'),
                             ('-', ['--out_format', 'mjpeg'], 'mjpeg'), ('-', [], 'y4m')):
        cfg, _ = videorun.build_config(base + ['--out', out] + extra)
        assert cfg.EVAL.out_format == want and cfg.EVAL.jpeg_quality == 90
    cfg, _ = videorun.build_config(base + ['--out', 'x.mjpeg', '--jpeg_quality', '75', '--out_chroma', '444', '--out_siting', 'centre', '--video_depth', '8'])
    assert cfg.EVAL.jpeg_quality == 75
    for extra, text in ((['--out_chroma', '422'], r'^videorun: an mjpeg result is 4:2:0 or 4:4:4 \(--out_chroma 422 is not built\)$'),
                        (['--video_depth', '10'], r'^videorun: an mjpeg result has 8 bits per sample \(got --video_depth 10\)$'),
                        (['--out_siting', 'left'], r'^videorun: an mjpeg result has centre-sited chroma, as JFIF defines it \(got --out_siting left\)$'),
                        (['--jpeg_quality', '0'], r'^videorun: --jpeg_quality must be an integer 1..100 \(got 0\)$'),
                        (['--jpeg_quality', '101'], r'^videorun: --jpeg_quality must be an integer 1..100 \(got 101\)$')):
        with pytest.raises(ValueError, match=text):
            videorun.build_config(base + ['--out', 'x.mjpeg'] + extra)
        videorun.build_config(base + ['--out', 'x.y4m'] + [e for e in extra if 'jpeg' not in e and e not in ('0', '101')])      # fine for y4m
    with pytest.raises(ValueError, match='--out_format must be y4m or mjpeg'):
        videorun.out_format('avi', 'x.y4m')


class _Reader(object):
    h, w, fmt, siting, range, fps = 64, 96, 'i420p10', 'left', 'limited', (30, 1)


def test_configure_sets_what_jfif_means():
    """10-bit, left-sited, limited-range BT.709 input: the mjpeg result is 8-bit 'i420' | 'i444', BT.601, full range, centre-sited, and
    the input's description stays the input's; without the option configure() sets what it set before."""
    from refvsr_amd import get_config, videorun
    for chroma, want in ((None, 'i420'), ('444', 'i444')):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        cfg.yuv_matrix = cfg.input_yuv_matrix = 'bt709'
        cfg.EVAL.out_format, cfg.EVAL.out_chroma = 'mjpeg', chroma
        videorun.configure(cfg, _Reader)
        assert (cfg.result_yuv, cfg.EVAL.out_yuv, cfg.yuv_matrix, cfg.yuv_range, cfg.yuv_siting) == (want, want, 'bt601', 'full', 'centre')
        assert (cfg.input_yuv, cfg.input_yuv_matrix, cfg.input_yuv_range, cfg.input_yuv_siting) == ('i420p10', 'bt709', 'limited', 'left')
        assert cfg.EVAL.jpeg_quality == 90
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.yuv_matrix = 'bt709'
    videorun.configure(cfg, _Reader)
    assert (cfg.result_yuv, cfg.yuv_matrix, cfg.yuv_siting) == ('i420p10', 'bt709', 'left') and getattr(cfg, 'yuv_range', None) in (None, 'limited')
    for field, value, text in (('out_chroma', '422', 'not built'), ('video_depth', 10, '8 bits'), ('out_siting', 'left', 'centre-sited'),
                               ('jpeg_quality', 200, 'jpeg_quality')):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        cfg.EVAL.out_format = 'mjpeg'
        setattr(cfg.EVAL, field, value)
        with pytest.raises(ValueError, match=text):
            videorun.configure(cfg, _Reader)


def test_frame_sink_writes_variable_lengths():
    """streamio.FrameSink with a length per frame: the MJPEG writer gets buffer[:length], or the bytes given in its place, in order."""
    from refvsr_amd import streamio
    files = [jpeg.encode_model(b, h, w, fmt, q, r) for b, h, w, fmt, q, r in (jc.crafted()[k] for k in ('zrl', 'clamp', 'ff_bytes'))]
    out = io.BytesIO()
    wr = jpeg.MJPEGWriter(out)
    run = streamio.Run()
    ring = [np.zeros(900, np.uint8) for _ in range(2)]
    sink = streamio.FrameSink(run, wr, ring, 'sink', 5.0)
    try:
        for k, f in enumerate(files + files):
            b = sink.take()
            if len(f) <= len(b):
                b[:len(f)] = np.frombuffer(f, np.uint8)
                sink.put(b, len(f))
            else:
                sink.put(b, data=f)                                              # (a file larger than a slot of the ring)
        sink.finish()
    finally:
        sink.close()
    assert len(files[2]) > 900 and wr.frames == 6 and jpeg.split_mjpeg(out.getvalue()) == files + files
