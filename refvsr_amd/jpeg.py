"""Baseline JPEG of Y'CbCr frames: the specification of refvsr_jpeg_encode (csrc/jpeg.hip) as a numpy model, and MJPEG streams.

Pure numpy, no torch (as yuv.py and resize.py): the kernels return the bytes of encode_model.  Extension -- the reference's consumer
writes a JPEG per frame on the host (evaluation/eval_qual_quan.py:107-129); here the entropy-coded data is made on the device from
the Y'CbCr frames refvsr_result_to_yuv produces, so that a tenth of the 4:2:0 bytes leaves it.

Input: ONE dense 8-bit 'i420' or 'i444' frame as yuv.planes reads it, h and w even and >= 2 (and <= 65535, the SOF0 fields).  JFIF is
BT.601, full range, centre-sited chroma: the frames of result_to_yuv(frames, 'i420' | 'i444', 'bt601', 'full', 'centre').

File: SOI, APP0 (JFIF 1.01, density 1:1), two DQT, SOF0, four DHT, DRI, SOS, entropy-coded data, EOI.  Sampling factors: 4:2:0 has
Y 2 x 2, Cb and Cr 1 x 1 (an MCU is 16 x 16 luma samples, its blocks Y00 Y01 Y10 Y11 Cb Cr); 4:4:4 has 1 x 1 throughout (an MCU is
8 x 8, its blocks Y Cb Cr).  Planes are extended to whole MCUs by repeating their last column and last row.

Quantisation tables: the example tables of ITU-T T.81 Annex K.1 scaled the customary way, s = 5000 // q (q < 50) | 200 - 2 q,
entry = clip((base s + 50) // 100, 1, 255), q = 1..100.

Transform, all float64, every product and every sum rounded on its own (no fused multiply-add), in this order:
  s = code - 128
  rows     t[y][u] = sum over x of s[y][x] C[u][x]      x ascending, the accumulator starts from the x = 0 product
  columns  F[v][u] = sum over y of t[y][u] C[v][y]      y ascending likewise
  C[k][j] = a(k) cos((2 j + 1) k pi / 16), a(0) = sqrt(1 / 8), a(k) = 1 / 2: dct_table(), made once by numpy and handed to the kernel
  (no cosine on the device)
  q = rint(F / Q)  (the float64 quotient, half to even), clamped to [-1024, 1023] (DC) | [-1023, 1023] (AC)

Entropy coding: zigzag order; DC as the difference to the previous block of the same component; (run, size) symbols with ZRL and EOB,
no EOB where zigzag position 63 is non-zero; the typical Huffman tables of Annex K.3 - K.6; a negative value v is the low `size` bits
of v - 1; every 0xFF byte of entropy-coded data is followed by 0x00.

Restart intervals of R MCUs (1 <= R <= 65535; DEFAULT_RESTART where None): after each interval but the last, the bits are padded to
a byte with 1-bits -- through the stuffing rule: a padded 0xFF gets its 0x00 --, RSTm follows, m = interval index mod 8, and the three
DC predictors return to 0.  The last interval is padded the same way and EOI follows.  Every interval is an independent, byte-aligned
piece: that is what the device coder's parallelism is made of (one wave per interval).

The private `wrong` argument of the model functions switches on one deliberately wrong reading of the text above (WRONG_MODELS): the
controls of tests/test_jpeg.py, which show that each crafted case tells the reading apart.  Nothing else passes it.
"""
import sys
from fractions import Fraction

import numpy as np

from . import yuv

FORMATS = ('i420', 'i444')
DEFAULT_RESTART = 4                                # MCUs per restart interval where none is given (profiles/jpeg_timing.txt)
WRONG_MODELS = ('half_away', 'contracted', 'descending', 'no_dc_reset', 'pad_zeros', 'no_pad_stuffing', 'swapped_chroma_tables',
                'zero_edges')

# ITU-T T.81 Annex K.1: the example luminance and chrominance quantisation tables, rows v of columns u
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61,
           12, 12, 14, 19, 26, 58, 60, 55,
           14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77,
           24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101,
           72, 92, 95, 98, 112, 100, 103, 99)
K1_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99,
             18, 21, 26, 66, 99, 99, 99, 99,
             24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# zigzag position -> natural index 8 v + u
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def _rows(*first):
    """HUFFVAL rows 'r1 .. rA' of the AC tables: (first, last) low nibbles per high nibble."""
    return tuple(hi << 4 | lo for hi, a, b in first for lo in range(a, b + 1))


# Annex K.3 - K.6: (BITS: codes per length 1..16, HUFFVAL: the symbols in code order)
K3_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
K4_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
K5_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
              (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
               0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a)
              + _rows((1, 6, 10), (2, 5, 10), (3, 4, 10), (4, 3, 10), (5, 3, 10), (6, 3, 10), (7, 3, 10), (8, 3, 10), (9, 2, 10),
                      (10, 2, 10), (11, 2, 10), (12, 2, 10), (13, 2, 10), (14, 1, 10), (15, 1, 10)))
K6_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
                (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
                 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
                 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a)
                + _rows((3, 5, 10), (4, 3, 10), (5, 3, 10), (6, 3, 10), (7, 3, 10), (8, 2, 10), (9, 2, 10), (10, 2, 10), (11, 2, 10),
                        (12, 2, 10), (13, 2, 10), (14, 2, 10), (15, 2, 10)))
HUFFMAN_SPECS = (K3_DC_LUMA, K5_AC_LUMA, K4_DC_CHROMA, K6_AC_CHROMA)      # the order of the DHT segments and of huffman_tables()
ZRL, EOB = 0xf0, 0x00

# the most bits one block can take: a DC code (<= 11 bits, K.4) with 11 value bits, 63 AC codes (<= 16 bits) with 10 value bits
# (a run of zeros costs less than the coefficients it replaces: a ZRL is 11 bits for 16 positions)
MAX_BLOCK_BITS = 22 + 63 * 26


def check_format(fmt):
    if fmt not in FORMATS:
        yuv.check_format(fmt)
        raise ValueError("jpeg: frames are 'i420' or 'i444' (8-bit, planar; 4:2:2 is not built), got %r" % (fmt,))
    return fmt


def check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError('jpeg quality must be an integer 1..100, got %r' % (quality,))
    return int(quality)


def check_restart(restart):
    """restart checked: None -> DEFAULT_RESTART, else an integer 1..65535 (the DRI field)."""
    if restart is None:
        return DEFAULT_RESTART
    if isinstance(restart, bool) or not isinstance(restart, (int, np.integer)) or not 1 <= restart <= 65535:
        raise ValueError('jpeg restart interval must be None or an integer 1..65535 MCUs, got %r' % (restart,))
    return int(restart)


def check_size(h, w):
    yuv.frame_shape(h, w)
    if h > 65535 or w > 65535:
        raise ValueError('jpeg frames are at most 65535 x 65535 (got %d x %d)' % (h, w))
    return h, w


def geometry(h, w, fmt):
    """(MCU rows, MCU columns, blocks per MCU) of an h x w frame."""
    check_size(h, w)
    m = 16 if check_format(fmt) == 'i420' else 8
    return (h + m - 1) // m, (w + m - 1) // m, 6 if fmt == 'i420' else 3


def intervals(h, w, fmt, restart=None):
    """Restart intervals of a frame."""
    my, mx, _ = geometry(h, w, fmt)
    r = check_restart(restart)
    return (my * mx + r - 1) // r


def quant_tables(quality):
    """(luma, chroma): int64 [64] each, natural order (8 v + u)."""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(base, np.int64) * s + 50) // 100, 1, 255) for base in (K1_LUMA, K1_CHROMA))


def dct_table():
    """C [8, 8] float64, C[k][j] = a(k) cos((2 j + 1) k pi / 16): the 64 doubles the model and the kernel both read."""
    k, j = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    a = np.full((8, 1), 0.5)
    a[0, 0] = np.sqrt(1.0 / 8.0)
    return a * np.cos((2.0 * j + 1.0) * k * np.pi / 16.0)


def huffman_codes(spec):
    """(code, length): int64 [256] each per symbol of one (BITS, HUFFVAL) table; length 0 where the table has no code."""
    bits, vals = spec
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            code[vals[k]], length[vals[k]] = c, n
            c += 1
            k += 1
        c <<= 1
    assert k == len(vals)
    return code, length


_HUFFMAN = None


def huffman_tables():
    """((code, length) of DC luma, AC luma, DC chroma, AC chroma): int64 [256] arrays per symbol."""
    global _HUFFMAN
    if _HUFFMAN is None:
        _HUFFMAN = tuple(huffman_codes(s) for s in HUFFMAN_SPECS)
    return _HUFFMAN


def huffman_lut():
    """The table the kernel reads: uint32 [4, 256], length << 16 | code, in the order of huffman_tables()."""
    return np.stack([(l << 16 | c).astype(np.uint32) for c, l in huffman_tables()])


def capacity(h, w, fmt, restart=None):
    """An upper bound of the entropy-coded bytes of one frame (RST markers included, EOI not).  A block takes at most
    MAX_BLOCK_BITS = 22 + 63 * 26 bits: the longest DC code (11 bits) with its 11 value bits, and 63 times the longest AC code (16 bits)
    with 10 value bits -- zeros only make a block shorter, a ZRL's 11 bits stand for 16 positions.  An interval of b blocks is then at
    most ceil(b MAX_BLOCK_BITS / 8) bytes, padding included; stuffing can at most double them; its RST marker adds 2."""
    my, mx, bpm = geometry(h, w, fmt)
    r, n = check_restart(restart), my * mx
    full, last = divmod(n, r)
    per = lambda mcus: 2 * ((mcus * bpm * MAX_BLOCK_BITS + 7) // 8) + 2
    return full * per(r) + (per(last) if last else 0)


# ------------------------------------------------------------------------------------------------ header
def _segment(marker, body):
    return bytes((0xff, marker)) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)


def header(h, w, fmt, quality=90, restart=None):
    """The bytes of a file before its entropy-coded data: SOI .. SOS.  The host writes them; the kernel never does."""
    check_size(h, w)
    ql, qc = quant_tables(quality)
    r = check_restart(restart)
    zz = np.array(ZIGZAG)
    out = [b'\xff\xd8', _segment(0xe0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    for k, q in enumerate((ql, qc)):
        out.append(_segment(0xdb, bytes([k]) + bytes(int(v) for v in q[zz])))
    out.append(_segment(0xc0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes(
        [3, 1, 0x22 if check_format(fmt) == 'i420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for ident, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFFMAN_SPECS):
        out.append(_segment(0xc4, bytes([ident]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xdd, r.to_bytes(2, 'big')))
    out.append(_segment(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(out)


EOI = b'\xff\xd9'


def assemble(head, data):
    """One file from header() and a frame's entropy-coded data."""
    return head + bytes(data) + EOI


# ------------------------------------------------------------------------------------------------ transform
def extend(plane, m, wrong=()):
    """A plane extended to multiples of m rows and columns by repeating its last row and column."""
    h, w = plane.shape
    ph, pw = -h % m, -w % m
    return np.pad(plane, ((0, ph), (0, pw)), mode='constant' if 'zero_edges' in wrong else 'edge')


def blocks(plane):
    """[H, W] (multiples of 8) -> [H / 8, W / 8, 8, 8]."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _fdct_exact(s, C):
    """The 'contracted' control: each pass's sum in exact arithmetic, rounded once."""
    out = np.empty(s.shape, np.float64)
    Cf = [[Fraction(float(c)) for c in row] for row in C]
    for idx in np.ndindex(*s.shape[:-2]):
        b = s[idx]
        t = [[float(sum(Fraction(float(b[y][x])) * Cf[u][x] for x in range(8))) for u in range(8)] for y in range(8)]
        out[idx] = [[float(sum(Fraction(t[y][u]) * Cf[v][y] for y in range(8))) for u in range(8)] for v in range(8)]
    return out


def fdct(s, wrong=()):
    """F [..., 8 (v), 8 (u)] of level-shifted samples s [..., 8 (y), 8 (x)], float64, in the order of the module text."""
    s = np.asarray(s, np.float64)
    C = dct_table()
    if 'contracted' in wrong:
        return _fdct_exact(s, C)
    order = range(7, -1, -1) if 'descending' in wrong else range(8)
    t = None
    for x in order:
        p = s[..., :, x, None] * C[:, x]                    # [..., y, u]
        t = p if t is None else t + p
    F = None
    for y in order:
        p = t[..., y, None, :] * C[:, y, None]              # [..., v, u]
        F = p if F is None else F + p
    return F


def quantise(F, q, wrong=()):
    """rint(F / Q) (half to even) and the clamps; F [..., 8, 8] float64, q int [64] natural order -> int64 [..., 64] in zigzag order."""
    v = (F / np.asarray(q, np.float64).reshape(8, 8)).reshape(F.shape[:-2] + (64,))
    r = np.sign(v) * np.floor(np.abs(v) + 0.5) if 'half_away' in wrong else np.rint(v)
    lo = np.full(64, -1023.0)
    lo[0] = -1024.0
    return np.clip(r, lo, 1023.0).astype(np.int64)[..., np.array(ZIGZAG)]


def coefficients(buf, h, w, fmt, quality=90, wrong=()):
    """The quantised coefficients of a frame in coding order: (int64 [MCUs, blocks per MCU, 64] in zigzag order, the component 0 | 1 |
    2 of each block of an MCU)."""
    my, mx, bpm = geometry(h, w, fmt)
    buf = np.asarray(buf)
    if buf.dtype != np.uint8 or buf.shape != yuv.frame_shape(h, w, fmt):
        raise ValueError('jpeg: a %d x %d %s frame is uint8 %s (got %s %s)' % (h, w, fmt, yuv.frame_shape(h, w, fmt), buf.dtype, buf.shape))
    ql, qc = quant_tables(quality)
    y, cb, cr = yuv.planes(buf, h, w, fmt)
    m = 16 if fmt == 'i420' else 8
    zz = [quantise(fdct(blocks(extend(p, mp, wrong)).astype(np.float64) - 128.0, wrong), q, wrong)
          for p, mp, q in ((y, m, ql), (cb, 8, qc), (cr, 8, qc))]
    out = np.empty((my, mx, bpm, 64), np.int64)
    if fmt == 'i420':
        yb = zz[0].reshape(my, 2, mx, 2, 64)
        for b in range(4):
            out[:, :, b] = yb[:, b >> 1, :, b & 1]
        out[:, :, 4], out[:, :, 5] = zz[1], zz[2]
        comps = (0, 0, 0, 0, 1, 2)
    else:
        for c in range(3):
            out[:, :, c] = zz[c]
        comps = (0, 1, 2)
    return out.reshape(my * mx, bpm, 64), comps


# ------------------------------------------------------------------------------------------------ entropy coding
def size_of(v):
    """The size category of a value: the bits of |v|."""
    return int(abs(int(v))).bit_length()


def block_symbols(zz, pred):
    """The symbols of one block, zz int [64] in zigzag order, pred the DC predictor: [(symbol, value)] -- first (size, difference) of
    the DC, then (run << 4 | size, value) per non-zero AC with (ZRL, 0) for every 16 zeros ahead of it, (EOB, 0) last unless position
    63 is non-zero."""
    d = int(zz[0]) - pred
    out = [(size_of(d), d)]
    last = 0
    for k in np.flatnonzero(zz[1:]) + 1:
        run = int(k) - last - 1
        out.extend([(ZRL, 0)] * (run >> 4))
        v = int(zz[k])
        out.append(((run & 15) << 4 | size_of(v), v))
        last = int(k)
    if last != 63:
        out.append((EOB, 0))
    return out


def symbols(buf, h, w, fmt, quality=90, restart=None, wrong=()):
    """The symbol stream of a frame: [interval][block] -> (component, block_symbols)."""
    co, comps = coefficients(buf, h, w, fmt, quality, wrong)
    r = check_restart(restart)
    out, pred = [], [0, 0, 0]
    for m0 in range(0, co.shape[0], r):
        if 'no_dc_reset' not in wrong:
            pred = [0, 0, 0]
        iv = []
        for m in range(m0, min(m0 + r, co.shape[0])):
            for b, c in enumerate(comps):
                iv.append((c, block_symbols(co[m, b], pred[c])))
                pred[c] = int(co[m, b, 0])
        out.append(iv)
    return out


def stuff(data):
    return data.replace(b'\xff', b'\xff\x00')


def interval_bytes(iv, wrong=()):
    """The bytes of one restart interval (no marker): the codes of its blocks' symbols, padded with 1-bits, stuffed."""
    tabs = huffman_tables()
    if 'swapped_chroma_tables' in wrong:
        tabs = (tabs[2], tabs[3], tabs[0], tabs[1])
    acc, n = 0, 0
    for c, syms in iv:
        dc, ac = (tabs[0], tabs[1]) if c == 0 else (tabs[2], tabs[3])
        for i, (sym, v) in enumerate(syms):
            code, length = dc if i == 0 else ac
            l = int(length[sym])
            assert l, 'no code for symbol %#x' % sym
            acc, n = acc << l | int(code[sym]), n + l
            sz = sym & 15 if i else sym
            if sz:
                acc, n = acc << sz | ((v - 1 if v < 0 else v) & ((1 << sz) - 1)), n + sz
    pad = -n % 8
    whole = (acc >> (n % 8)).to_bytes(n // 8, 'big') if n >= 8 else b''
    if not pad:
        return stuff(whole)
    tail = (acc & ((1 << (8 - pad)) - 1)) << pad | (0 if 'pad_zeros' in wrong else (1 << pad) - 1)
    return stuff(whole) + (bytes([tail]) if 'no_pad_stuffing' in wrong else stuff(bytes([tail])))


def entropy_data(buf, h, w, fmt, quality=90, restart=None, wrong=()):
    """The entropy-coded data of a frame, RST markers included: what refvsr_jpeg_encode writes for it."""
    ivs = symbols(buf, h, w, fmt, quality, restart, wrong)
    out = []
    for i, iv in enumerate(ivs):
        out.append(interval_bytes(iv, wrong))
        if i + 1 < len(ivs):
            out.append(bytes((0xff, 0xd0 + (i & 7))))
    return b''.join(out)


def encode_model(buf, h, w, fmt, quality=90, restart=None, wrong=()):
    """One complete JFIF file of one frame: the definition."""
    return assemble(header(h, w, fmt, quality, restart), entropy_data(buf, h, w, fmt, quality, restart, wrong))


# ------------------------------------------------------------------------------------------------ MJPEG
def _scan_file(data, pos, what):
    """The end (one past EOI) of the JPEG file that starts at data[pos]."""
    if data[pos:pos + 2] != b'\xff\xd8':
        raise ValueError('%s: SOI expected at byte %d' % (what, pos))
    p = pos + 2
    while True:                                                 # marker segments up to SOS
        if p + 4 > len(data) or data[p] != 0xff:
            raise ValueError('%s: marker expected at byte %d' % (what, p))
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], 'big')
        p += 2 + n
        if m == 0xda:
            break
    while True:                                                 # entropy-coded data: 0xFF is followed by 0x00 or RSTm until EOI
        p = data.find(b'\xff', p)
        if p < 0 or p + 1 >= len(data):
            raise ValueError('%s: the file that starts at byte %d has no EOI' % (what, pos))
        m = data[p + 1]
        p += 2
        if m == 0xd9:
            return p
        if m != 0x00 and not 0xd0 <= m <= 0xd7:
            raise ValueError('%s: marker %#04x inside entropy-coded data at byte %d' % (what, m, p - 2))


def split_mjpeg(data, what='mjpeg'):
    """The JPEG files of a stream MJPEGWriter wrote, one bytes object each: cut at EOI / SOI."""
    data = bytes(data)
    out, pos = [], 0
    while pos < len(data):
        end = _scan_file(data, pos, what)
        out.append(data[pos:end])
        pos = end
    return out


class MJPEGWriter(object):
    """An MJPEG stream: complete JPEG files back to back, nothing between them and no header of its own -- the stream carries no
    frame rate (ffmpeg reads it with -f mjpeg -framerate N).  The surface of yuv.Y4MWriter: write(file bytes), close(), frames, name;
    path: a path, '-' (sys.stdout.buffer) or a binary file object; close() flushes and closes only a file opened here.  A sink that
    went away (BrokenPipeError) is a one-line ValueError naming it."""

    def __init__(self, path):
        self.frames = 0
        self.bytes = 0
        self.name = yuv.sink_name(path)
        self.owned = not (path == '-' or hasattr(path, 'write'))
        self.fh = open(path, 'wb') if self.owned else sys.stdout.buffer if path == '-' else path

    def write(self, data):
        data = memoryview(data).cast('B') if not isinstance(data, (bytes, bytearray)) else data
        if len(data) < 4 or bytes(data[:2]) != b'\xff\xd8' or bytes(data[-2:]) != EOI:
            raise ValueError('MJPEGWriter: a frame is one complete JPEG file, SOI .. EOI (got %d bytes)' % len(data))
        try:
            self.fh.write(data)
        except BrokenPipeError:
            raise ValueError('%s: the sink closed the pipe behind frame %d' % (self.name, self.frames))
        self.frames += 1
        self.bytes += len(data)

    def close(self):
        if self.fh is not None:
            fh, self.fh = self.fh, None
            try:
                fh.close() if self.owned else fh.flush()
            except BrokenPipeError:
                raise ValueError('%s: the sink closed the pipe behind frame %d' % (self.name, self.frames))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
