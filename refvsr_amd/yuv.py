"""Y'CbCr 4:2:0 result frames: the specification of refvsr_result_to_yuv420 (csrc/yuv.hip) as a numpy model, and Y4M files.

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
"""
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


def read_y4m(path):
    """-> dict(h, w, fps=(num, den), fmt='i420' | 'i420p10', range, frames=[buffers [3 h / 2, w]]) of a file Y4MWriter wrote."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'\n')
    tok = data[:end].decode('ascii').split(' ')
    if tok[0] != 'YUV4MPEG2':
        raise ValueError('%s: not a YUV4MPEG2 file' % path)
    f = dict((t[0], t[1:]) for t in tok[1:] if t[0] != 'X')
    x = dict(t[1:].split('=', 1) for t in tok[1:] if t[0] == 'X' and '=' in t)
    h, w = int(f['H']), int(f['W'])
    fmt = {'420jpeg': 'i420', '420p10': 'i420p10'}[f['C']]
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
    return {'h': h, 'w': w, 'fps': parse_fps(f['F']), 'fmt': fmt, 'range': x.get('COLORRANGE', 'LIMITED').lower(), 'frames': frames}
