"""Y'CbCr 4:2:0 frames, out and in: the specifications of refvsr_result_to_yuv420 (csrc/yuv.hip) and of refvsr_yuv420_to_rgb
(csrc/yuv_in.hip) as numpy models, and Y4M files.

Pure numpy, no torch (as the models of metrics.py): the kernel returns the bits of rgb_to_yuv420.  Extension -- the reference's
consumer writes PNG / JPG (evaluation/eval_qual_quan.py:117-119); every video consumer (encoders, raw-video pipes, players, .y4m)
takes 4:2:0 instead, 1.5 samples per pixel where RGB has 3.

Formats (a frame is ONE dense buffer of 3 h w / 2 samples, viewed as [3 h / 2, w]; h, w even):
  'nv12'     Y [h, w], then interleaved CbCr [h/2, w/2, 2]     uint8
  'i420'     Y [h, w], Cb [h/2, w/2], Cr [h/2, w/2]            uint8
  'p010'     the nv12 layout                                   uint16, the 10-bit code in the high bits (code << 6)
  'i420p10'  the i420 layout                                   uint16, the code in the low bits

Arithmetic, all float64, every operation rounded on its own (no fused multiply-add), in this order:
  source  r, g, b: a float32 / float16 result widened exactly; a uint8 result byte u is u / 255.0 (the float64 quotient)
  pixel   ey = (kr r + kg g) + kb b;  Y = rint(oy + sy ey);  ecb = (b - ey) icb;  ecr = (r - ey) icr
  block   m = ((e00 + e01) + (e10 + e11)) 0.25  (centre-sited: the box average of the unquantised chroma);  C = rint(oc + sc m)
rint rounds half to even; every code is clamped to [0, 2^d - 1] before the cast (pure blue at full range gives 255.5).

The way in (yuv420_to_rgb; extension -- the reference's loader reads PNGs, data_loader/utils.py:12-41), float64 in the same manner:
  codes   nv12 / i420: the byte;  p010: sample >> 6 (the low six bits are ignored);  i420p10: sample & 1023
  chroma  at luma pixel (y, x), centre-sited -- the inverse siting of the box average above:  (cy, cx) = (y >> 1, x >> 1),
          cy' = clamp(cy + (y & 1 ? 1 : -1), 0, h/2 - 1), cx' likewise,
          m = (9 C[cy,cx] + 3 C[cy',cx] + 3 C[cy,cx'] + C[cy',cx']) 0.0625  (an integer below 2^15 times a power of two: exact in
          any order);  chroma = 'nearest': m = C[cy,cx]
  pixel   ey = (Y - oy) iy;  ecb = (mcb - oc) ic;  ecr = (mcr - oc) ic;  r = ey + cr_r ecr;  b = ey + cb_b ecb;
          g = ((ey - kr r) - kb b) ikg
  output  r, g, b clamped to [0, 1] (decoded video is routinely out of gamut; the network's contract is frames in [0, 1]), then
          rounded once to float32
with (oy, iy = 1 / sy, oc, ic = 1 / sc, cr_r = 2 (1 - kr), cb_b = 2 (1 - kb), kr, kb, ikg = 1 / kg) of decode_coefficients.

luma_sad: the sum of absolute differences of two frames' luma codes (the same codes), the model of refvsr_luma_sad (csrc/scene.hip)
behind videorun's scene-cut detector (scene.py).
"""
import os

import numpy as np

# name -> (bit depth, semi-planar (interleaved CbCr), left shift of the code)
FORMATS = {'nv12': (8, True, 0), 'i420': (8, False, 0), 'p010': (10, True, 6), 'i420p10': (10, False, 0)}
FORMAT_IDS = {'nv12': 0, 'i420': 1, 'p010': 2, 'i420p10': 3}          # REFVSR_YUV_* of include/refvsr_hip.h
MATRICES = {'bt709': (0.2126, 0.0722), 'bt601': (0.299, 0.114)}       # (kr, kb)
RANGES = ('limited', 'full')
PLANAR_TWIN = {'nv12': 'i420', 'p010': 'i420p10'}


def check_format(fmt):
    if fmt not in FORMATS:
        raise ValueError('yuv format must be one of %s, got %r' % (', '.join("'%s'" % k for k in FORMATS), fmt))
    return fmt


def check_matrix(matrix):
    if matrix not in MATRICES:
        raise ValueError("yuv_matrix must be 'bt709' or 'bt601', got %r" % (matrix,))
    return matrix


def check_range(range):
    if range not in RANGES:
        raise ValueError("yuv_range must be 'limited' or 'full', got %r" % (range,))
    return range


def resolve(result_yuv, matrix=None, range=None):
    """config.result_yuv / yuv_matrix / yuv_range checked: None (off) or (format, matrix, range); ValueError for a bad name -- also
    for a bad matrix or range while the format is off, so that a typo does not wait for the day the feature is switched on."""
    m, r = check_matrix(matrix or 'bt709'), check_range(range or 'limited')
    if result_yuv is None:
        return None
    if result_yuv not in FORMATS:
        raise ValueError("result_yuv must be None, 'nv12', 'i420', 'p010' or 'i420p10', got %r" % (result_yuv,))
    return (result_yuv, m, r)


def depth_of(fmt):
    return FORMATS[check_format(fmt)][0]


def dtype_of(fmt):
    return np.uint8 if depth_of(fmt) == 8 else np.uint16


def coefficients(fmt='nv12', matrix='bt709', range='limited'):
    """The nine doubles (kr, kg, kb, icb, icr, oy, sy, oc, sc) the model and the kernel both get, computed once in Python float64."""
    d = depth_of(fmt)
    kr, kb = MATRICES[check_matrix(matrix)]
    kg = 1.0 - kr - kb
    icb = 0.5 / (1.0 - kb)
    icr = 0.5 / (1.0 - kr)
    s = 2.0 ** (d - 8)
    if check_range(range) == 'limited':
        oy, sy, oc, sc = 16 * s, 219 * s, 128 * s, 224 * s
    else:
        oy, sy, oc, sc = 0.0, float(2 ** d - 1), float(2 ** (d - 1)), float(2 ** d - 1)
    return (kr, kg, kb, icb, icr, float(oy), float(sy), float(oc), float(sc))


def frame_shape(h, w):
    """[3 h / 2, w]: the view of a frame's buffer."""
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError('4:2:0 frames need even, positive h and w (got %d x %d)' % (h, w))
    return (3 * h // 2, w)


def frame_bytes(h, w, fmt):
    """Bytes of one frame (== refvsr_yuv420_bytes)."""
    r, c = frame_shape(h, w)
    return r * c * (1 if depth_of(fmt) == 8 else 2)


def source_f64(x):
    """A result array as the float64 source value: floats widened exactly, a byte u as u / 255.0."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.astype(np.float64) / 255.0
    if x.dtype not in (np.float32, np.float16, np.float64):
        raise TypeError('results are float32, float16 or uint8 (got %s)' % x.dtype)
    return x.astype(np.float64)


def pre_rounding(rgb, coef):
    """(oy + sy ey [h, w], oc + sc mcb [h/2, w/2], oc + sc mcr [h/2, w/2]) of one [3, h, w] frame: the values rint sees."""
    kr, kg, kb, icb, icr, oy, sy, oc, sc = coef
    v = source_f64(rgb)
    assert v.ndim == 3 and v.shape[0] == 3, 'a frame is [3, h, w]'
    frame_shape(*v.shape[1:])
    r, g, b = v[0], v[1], v[2]
    ey = (kr * r + kg * g) + kb * b
    out = [oy + sy * ey]
    for e in ((b - ey) * icb, (r - ey) * icr):
        m = ((e[0::2, 0::2] + e[0::2, 1::2]) + (e[1::2, 0::2] + e[1::2, 1::2])) * 0.25
        out.append(oc + sc * m)
    return tuple(out)


def quantise(v, depth):
    """rint (half to even), then the clamp to [0, 2^depth - 1]; float64 in, int64 out."""
    return np.clip(np.rint(v), 0.0, float(2 ** depth - 1)).astype(np.int64)


def pack(y, cb, cr, fmt):
    """Integer code planes -> the frame's buffer [3 h / 2, w] in the format's layout and sample type."""
    d, semi, shift = FORMATS[check_format(fmt)]
    h, w = y.shape
    dt = dtype_of(fmt)
    c = np.stack([cb, cr], axis=-1).reshape(-1) if semi else np.concatenate([cb.reshape(-1), cr.reshape(-1)])
    flat = np.concatenate([np.asarray(y).reshape(-1), c]).astype(np.int64) << shift
    return flat.astype(dt).reshape(frame_shape(h, w))


def rgb_to_yuv420(rgb, fmt='nv12', matrix='bt709', range='limited'):
    """The model: a [3, h, w] result (float32 | float16 | uint8, any strides) -> the frame's buffer [3 h / 2, w]; a [B, 3, h, w] batch
    -> [B, 3 h / 2, w]."""
    rgb = np.asarray(rgb)
    if rgb.ndim == 4:
        return np.stack([rgb_to_yuv420(f, fmt, matrix, range) for f in rgb])
    d = depth_of(fmt)
    yv, cbv, crv = pre_rounding(rgb, coefficients(fmt, matrix, range))
    return pack(quantise(yv, d), quantise(cbv, d), quantise(crv, d), fmt)


def planes(buf, h, w, fmt):
    """The (Y [h, w], Cb [h/2, w/2], Cr [h/2, w/2]) views of a frame's buffer; together they tile it exactly."""
    d, semi, _ = FORMATS[check_format(fmt)]
    flat = np.asarray(buf).reshape(-1)
    assert flat.size == 3 * h * w // 2 and frame_shape(h, w), 'a frame holds 3 h w / 2 samples'
    n, q = h * w, h * w // 4
    y = flat[:n].reshape(h, w)
    if semi:
        c = flat[n:].reshape(h // 2, w // 2, 2)
        return y, c[..., 0], c[..., 1]
    return y, flat[n:n + q].reshape(h // 2, w // 2), flat[n + q:].reshape(h // 2, w // 2)


def to_planar(buf, h, w, fmt):
    """A frame's buffer in its planar twin's layout (nv12 -> i420, p010 -> i420p10 with the code in the low bits)."""
    d, semi, shift = FORMATS[check_format(fmt)]
    y, cb, cr = planes(buf, h, w, fmt)
    return pack(y.astype(np.int64) >> shift, cb.astype(np.int64) >> shift, cr.astype(np.int64) >> shift, PLANAR_TWIN.get(fmt, fmt))


# ------------------------------------------------------------------------------------------------ the way in
CHROMA_MODES = {'bilinear': 0, 'nearest': 1}                           # REFVSR_YUV_CHROMA_* of include/refvsr_hip.h


def check_chroma(chroma):
    if chroma not in CHROMA_MODES:
        raise ValueError("yuv chroma mode must be 'bilinear' or 'nearest', got %r" % (chroma,))
    return chroma


def resolve_input(input_yuv, matrix=None, range=None, chroma=None):
    """config.input_yuv / input_yuv_matrix / input_yuv_range / input_yuv_chroma checked: None (off) or (format, matrix, range, chroma);
    ValueError for a bad name, also while the format is off (as resolve)."""
    m, r, c = check_matrix(matrix or 'bt709'), check_range(range or 'limited'), check_chroma(chroma or 'bilinear')
    if input_yuv is None:
        return None
    if input_yuv not in FORMATS:
        raise ValueError("input_yuv must be None, 'nv12', 'i420', 'p010' or 'i420p10', got %r" % (input_yuv,))
    return (input_yuv, m, r, c)


def decode_coefficients(fmt='nv12', matrix='bt709', range='limited'):
    """The nine doubles (oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg) the decoding model and its kernel both get, computed once in Python
    float64 from coefficients(): the reciprocals are taken here, no division happens on the device."""
    kr, kg, kb, _, _, oy, sy, oc, sc = coefficients(fmt, matrix, range)
    return (oy, 1.0 / sy, oc, 1.0 / sc, 2.0 * (1.0 - kr), 2.0 * (1.0 - kb), kr, kb, 1.0 / kg)


def codes(buf, h, w, fmt):
    """The integer code planes (Y [h, w], Cb [h/2, w/2], Cr [h/2, w/2]; int64) of a frame's buffer."""
    d, _, shift = FORMATS[check_format(fmt)]
    buf = np.asarray(buf)
    if buf.dtype != dtype_of(fmt):
        raise TypeError('%s frames are %s (got %s)' % (fmt, np.dtype(dtype_of(fmt)).name, buf.dtype))
    # (p010: the code in the high bits, sample >> 6; the others: the low d bits -- all eight of a byte, sample & 1023 of i420p10)
    return tuple((p.astype(np.int64) >> shift) & (2 ** d - 1) for p in planes(buf, h, w, fmt))


def luma_sad(a, b, h, w, fmt):
    """The model of refvsr_luma_sad (csrc/scene.hip): the sum of absolute differences of the luma codes of two frames' buffers, a
    Python int (integer arithmetic on codes(): a p010 sample's low six bits and an i420p10 sample's bits above bit 9 do not count)."""
    ya, yb = codes(a, h, w, fmt)[0], codes(b, h, w, fmt)[0]
    return int(np.abs(ya - yb).sum(dtype=np.int64))


def chroma_taps(c, chroma='bilinear'):
    """The integer tap sum 16 m [h, w] of a chroma code plane [h/2, w/2] (int64): 9 C[cy,cx] + 3 C[cy',cx] + 3 C[cy,cx'] + C[cy',cx']
    at every luma pixel, the neighbours clamped at the edges; 'nearest': 16 C[cy,cx]."""
    h2, w2 = c.shape
    y, x = np.arange(2 * h2), np.arange(2 * w2)
    cy, cx = y >> 1, x >> 1
    if check_chroma(chroma) == 'nearest':
        return 16 * c[cy][:, cx]
    cy2 = np.clip(cy + np.where(y & 1, 1, -1), 0, h2 - 1)
    cx2 = np.clip(cx + np.where(x & 1, 1, -1), 0, w2 - 1)
    return 9 * c[cy][:, cx] + 3 * c[cy2][:, cx] + 3 * c[cy][:, cx2] + c[cy2][:, cx2]


def decode_pre_clamp(buf, h, w, fmt='nv12', matrix='bt709', range='limited', chroma='bilinear'):
    """(r, g, b) float64 [h, w] of one frame before the clamp to [0, 1] and the rounding to float32."""
    oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg = decode_coefficients(fmt, matrix, range)
    yc, cbc, crc = codes(buf, h, w, fmt)
    ey = (yc.astype(np.float64) - oy) * iy
    ecb = (chroma_taps(cbc, chroma).astype(np.float64) * 0.0625 - oc) * ic
    ecr = (chroma_taps(crc, chroma).astype(np.float64) * 0.0625 - oc) * ic
    r = ey + cr_r * ecr
    b = ey + cb_b * ecb
    g = ((ey - kr * r) - kb * b) * ikg
    return r, g, b


def yuv420_to_rgb(buf, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear'):
    """The model of the way in: a frame's buffer [3 h / 2, w] (uint8 | uint16 by format) -> float32 [3, h, w] in [0, 1]; a
    [B, 3 h / 2, w] batch -> [B, 3, h, w]."""
    buf = np.asarray(buf)
    if buf.ndim == 3:
        return np.stack([yuv420_to_rgb(f, h, w, fmt, matrix, range, chroma) for f in buf])
    if buf.shape != frame_shape(h, w):
        raise ValueError('a %d x %d frame is %s (got %s)' % (h, w, frame_shape(h, w), buf.shape))
    return np.stack([np.clip(v, 0.0, 1.0) for v in decode_pre_clamp(buf, h, w, fmt, matrix, range, chroma)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ Y4M
def parse_fps(text):
    """'30' | '30000:1001' -> (num, den)."""
    parts = str(text).split(':')
    try:
        num, den = (int(parts[0]), 1) if len(parts) == 1 else (int(parts[0]), int(parts[1]))
        if len(parts) > 2 or num <= 0 or den <= 0:
            raise ValueError
    except ValueError:
        raise ValueError("frame rate must be N or N:D with positive integers, got %r" % (text,))
    return num, den


def y4m_header(h, w, fmt, fps=(30, 1), range='limited'):
    frame_shape(h, w)
    if fmt in PLANAR_TWIN:
        raise ValueError("%r is not a Y4M format (Y4M frames are planar): use %r" % (fmt, PLANAR_TWIN[fmt]))
    tag = 'C420jpeg' if depth_of(fmt) == 8 else 'C420p10'
    return ('YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n' % (w, h, fps[0], fps[1], tag, check_range(range).upper())).encode('ascii')


class Y4MWriter(object):
    """A .y4m file of 'i420' (C420jpeg) or 'i420p10' (C420p10, little-endian samples) frames: the header, then `FRAME\\n` and the
    planes Y, Cb, Cr per frame -- which is the frame's buffer as it lies in memory."""

    def __init__(self, path, h, w, fmt='i420', fps=(30, 1), range='limited'):
        self.header = y4m_header(h, w, fmt, fps, range)
        self.h, self.w, self.fmt = h, w, fmt
        self.frames = 0
        self.fh = open(path, 'wb')
        self.fh.write(self.header)

    def write(self, buf):
        a = np.asarray(buf)
        if a.shape != frame_shape(self.h, self.w) or a.dtype != dtype_of(self.fmt):
            raise ValueError('Y4MWriter: %s frames are %s %s (got %s %s)' % (self.fmt, np.dtype(dtype_of(self.fmt)).name,
                                                                          frame_shape(self.h, self.w), a.dtype, a.shape))
        self.fh.write(b'FRAME\n')
        self.fh.write(np.ascontiguousarray(a).astype(a.dtype.newbyteorder('<'), copy=False).tobytes())
        self.frames += 1

    def close(self):
        if self.fh is not None:
            self.fh.close()
            self.fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def parse_y4m_header(line, path):
    """The header line (without its newline) -> dict(h, w, fps, fmt, range)."""
    tok = line.decode('ascii', 'replace').split(' ')
    if tok[0] != 'YUV4MPEG2':
        raise ValueError('%s: not a YUV4MPEG2 file' % path)
    f = dict((t[0], t[1:]) for t in tok[1:] if t and t[0] != 'X')
    x = dict(t[1:].split('=', 1) for t in tok[1:] if t and t[0] == 'X' and '=' in t)
    fmt = {'420jpeg': 'i420', '420p10': 'i420p10'}[f['C']]
    return {'h': int(f['H']), 'w': int(f['W']), 'fps': parse_fps(f['F']), 'fmt': fmt, 'range': x.get('COLORRANGE', 'LIMITED').lower()}


class Y4MReader(object):
    """A .y4m file Y4MWriter wrote, read one frame at a time (read_y4m holds the whole file): the header fields of read_y4m as
    attributes (h, w, fps, fmt, range) and, by iteration or read(), one frame buffer [3 h / 2, w] after the other; read() returns
    None at the end of the file and raises ValueError for a truncated frame or a missing FRAME marker."""

    def __init__(self, path):
        self.path = path
        self.fh = open(path, 'rb')
        try:
            line = self.fh.readline(4096)
            if not line.endswith(b'\n'):
                raise ValueError('%s: not a YUV4MPEG2 file' % path)
            hd = parse_y4m_header(line[:-1], path)
        except Exception:
            self.close()
            raise
        self.h, self.w, self.fps, self.fmt, self.range = hd['h'], hd['w'], hd['fps'], hd['fmt'], hd['range']
        self.frames = 0             # frames read so far
        # whole frames in the file, by its size (a truncated last frame is not counted; read() reports it)
        self.length = (os.fstat(self.fh.fileno()).st_size - len(line)) // (6 + frame_bytes(self.h, self.w, self.fmt))

    def read(self):
        mark = self.fh.read(6)
        if not mark:
            return None
        if mark != b'FRAME\n':
            raise ValueError('%s: FRAME marker expected before frame %d' % (self.path, self.frames))
        nbytes = frame_bytes(self.h, self.w, self.fmt)
        raw = self.fh.read(nbytes)
        if len(raw) != nbytes:
            raise ValueError('%s: truncated frame %d' % (self.path, self.frames))
        self.frames += 1
        dt = dtype_of(self.fmt)
        return np.frombuffer(raw, dtype=np.dtype(dt).newbyteorder('<')).astype(dt).reshape(frame_shape(self.h, self.w))

    def __iter__(self):
        while True:
            f = self.read()
            if f is None:
                return
            yield f

    def close(self):
        if self.fh is not None:
            self.fh.close()
            self.fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_y4m(path):
    """-> dict(h, w, fps=(num, den), fmt='i420' | 'i420p10', range, frames=[buffers [3 h / 2, w]]) of a file Y4MWriter wrote."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'\n')
    hd = parse_y4m_header(data[:end], path)
    h, w, fmt = hd['h'], hd['w'], hd['fmt']
    nbytes = frame_bytes(h, w, fmt)
    frames, pos = [], end + 1
    while pos < len(data):
        if data[pos:pos + 6] != b'FRAME\n':
            raise ValueError('%s: FRAME marker expected at byte %d' % (path, pos))
        pos += 6
        raw = data[pos:pos + nbytes]
        if len(raw) != nbytes:
            raise ValueError('%s: truncated frame %d' % (path, len(frames)))
        frames.append(np.frombuffer(raw, dtype=np.dtype(dtype_of(fmt)).newbyteorder('<')).astype(dtype_of(fmt)).reshape(frame_shape(h, w)))
        pos += nbytes
    return dict(hd, frames=frames)
