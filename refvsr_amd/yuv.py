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

Samplings and sitings (rgb_to_yuv, yuv_to_rgb: the models of refvsr_result_to_yuv and refvsr_yuv_to_rgb).  Four more planar formats,
one dense buffer each as above, Y [h, w], Cb [h / cv, w / ch], Cr [h / cv, w / ch]:
  'i422'  'i422p10'   (cv, ch) = (1, 2)   [2 h, w]      uint8 | uint16, the code in the low bits
  'i444'  'i444p10'   (cv, ch) = (1, 1)   [3 h, w]
h and w stay even for all of them (4:4:4 would not need it; the engine's frame checks and refvsr_luma_sad do).  Semi-planar 4:2:2 /
4:4:4 (NV16, P210, NV24) does not exist here.  siting = 'centre' (a chroma sample lies in the middle of its luma pair: JPEG, the 4:2:0
above) | 'left' (on the pair's even column: MPEG-2, what decoders deliver as NV12 / P010 and what 4:2:2 means in Y4M); vertically a
4:2:0 sample lies between its two rows in both.  Siting is checked and then ignored for 4:4:4.
  luma x   0   1   2   3   4   5
  centre     0       1       2           sample j at x = 2j + 1/2
  left     0       1       2             sample j at x = 2j
  out   e = ecb | ecr as above, unquantised, l = max(2j - 1, 0):
          4:4:4         m = e
          4:2:2 centre  m = (e[y,2j] + e[y,2j+1]) 0.5
          4:2:2 left    m = ((e[y,l] + e[y,2j+1]) + (e[y,2j] + e[y,2j])) 0.25          the [1 2 1] / 4 filter, the left edge clamped
          4:2:0 left    v[x] = e[2i,x] + e[2i+1,x];  m = ((v[l] + v[2j+1]) + (v[2j] + v[2j])) 0.125
        then C = rint(oc + sc m) and the clamp, as above
  in    the integer tap sum 16 m, cx = x >> 1, cx' the clamped neighbour as above, cxr = min(cx + 1, w/2 - 1), cy and cy' as above:
          4:4:4                 16 C[y,x]
          4:2:2 centre          12 C[y,cx] + 4 C[y,cx']
          4:2:2 left   even x   16 C[y,cx]                    odd x  8 C[y,cx] + 8 C[y,cxr]
          4:2:0 left   even x   12 C[cy,cx] + 4 C[cy',cx]     odd x  6 C[cy,cx] + 2 C[cy',cx] + 6 C[cy,cxr] + 2 C[cy',cxr]
          'nearest'             16 x the own sample, every sampling
        everything behind the tap sum as above

Y4M: the C tag names sampling, depth and, for 4:2:0, the siting (420jpeg = 420 = no tag: centre; 420mpeg2: left; 422*: left, Y4M
defines 4:2:2 as co-sited); what a tag cannot say (420p10 left, 422 centre) is an XCHROMASITING=LEFT | CENTRE token, which the writer
adds and the reader honours.  Top-left siting (420paldv), mono and interlaced files are refused by name.
"""
import io
import os
import select
import sys

import numpy as np

# name -> (bit depth, semi-planar (interleaved CbCr), left shift of the code)
FORMATS = {'nv12': (8, True, 0), 'i420': (8, False, 0), 'p010': (10, True, 6), 'i420p10': (10, False, 0)}
FORMAT_IDS = {'nv12': 0, 'i420': 1, 'p010': 2, 'i420p10': 3}          # REFVSR_YUV_* of include/refvsr_hip.h
MATRICES = {'bt709': (0.2126, 0.0722), 'bt601': (0.299, 0.114)}       # (kr, kb)
RANGES = ('limited', 'full')
PLANAR_TWIN = {'nv12': 'i420', 'p010': 'i420p10'}
SAMPLINGS = {'420': 0, '422': 1, '444': 2}                            # REFVSR_YUV_SAMPLING_* of include/refvsr_hip.h
SUBSAMPLING = {'420': (2, 2), '422': (1, 2), '444': (1, 1)}           # (cv, ch): luma rows and columns per chroma sample
SITINGS = {'centre': 0, 'left': 1}                                    # REFVSR_YUV_SITING_*
# the 4:2:2 / 4:4:4 formats: name -> (its 4:2:0 twin: depth, sample type, shift and format id are the twin's; sampling)
CHROMA_FORMATS = {'i422': ('i420', '422'), 'i444': ('i420', '444'), 'i422p10': ('i420p10', '422'), 'i444p10': ('i420p10', '444')}
ALL_FORMATS = tuple(FORMATS) + tuple(CHROMA_FORMATS)


def check_format(fmt):
    if fmt not in FORMATS and fmt not in CHROMA_FORMATS:
        raise ValueError('yuv format must be one of %s, got %r' % (', '.join("'%s'" % k for k in ALL_FORMATS), fmt))
    return fmt


def twin_of(fmt):
    """The 4:2:0 format of the same depth, sample type and shift (a 4:2:0 format is its own): its FORMATS / FORMAT_IDS entries hold
    for fmt, and refvsr_luma_sad reads fmt's luma plane under the twin's id."""
    return CHROMA_FORMATS[fmt][0] if check_format(fmt) in CHROMA_FORMATS else fmt


def sampling_of(fmt):
    return CHROMA_FORMATS[fmt][1] if check_format(fmt) in CHROMA_FORMATS else '420'


def check_siting(siting, what='yuv siting'):
    if siting not in SITINGS:
        raise ValueError("%s must be 'centre' or 'left', got %r" % (what, siting))
    return siting


def effective_siting(fmt, siting):
    """siting checked; 'centre' for 4:4:4, where it means nothing."""
    return 'centre' if sampling_of(fmt) == '444' and check_siting(siting) else check_siting(siting)


def check_matrix(matrix):
    if matrix not in MATRICES:
        raise ValueError("yuv_matrix must be 'bt709' or 'bt601', got %r" % (matrix,))
    return matrix


def check_range(range):
    if range not in RANGES:
        raise ValueError("yuv_range must be 'limited' or 'full', got %r" % (range,))
    return range


def _config_format(fmt, field):
    """config.result_yuv / input_yuv (not None) checked: the format, or the field's ValueError."""
    if fmt not in FORMATS and fmt not in CHROMA_FORMATS:
        raise ValueError("%s must be None, 'nv12', 'i420', 'p010' or 'i420p10', got %r (or a 4:2:2 / 4:4:4 form: %s)"
                         % (field, fmt, ', '.join("'%s'" % f for f in CHROMA_FORMATS)))
    return fmt


def resolve(result_yuv, matrix=None, range=None):
    """config.result_yuv / yuv_matrix / yuv_range checked: None (off) or (format, matrix, range); ValueError for a bad name -- also
    for a bad matrix or range while the format is off, so that a typo does not wait for the day the feature is switched on."""
    m, r = check_matrix(matrix or 'bt709'), check_range(range or 'limited')
    if result_yuv is None:
        return None
    return (_config_format(result_yuv, 'result_yuv'), m, r)


def resolve_siting(siting, what='yuv_siting'):
    """config.yuv_siting / input_yuv_siting checked -- also while the format is off (as resolve): 'centre' (None: the default) | 'left'."""
    return check_siting(siting or 'centre', what)


def depth_of(fmt):
    return FORMATS[twin_of(fmt)][0]


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


def frame_shape(h, w, fmt=None):
    """[3 h / 2, w]: the view of a frame's buffer; with a format, that format's: [2 h, w] for 4:2:2, [3 h, w] for 4:4:4."""
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError('4:2:0 frames need even, positive h and w (got %d x %d)' % (h, w) if fmt is None or fmt in FORMATS else
                         '%s frames need even, positive h and w, as every format here (got %d x %d)' % (fmt, h, w))
    cv, ch = SUBSAMPLING[sampling_of(fmt)] if fmt is not None else (2, 2)
    return (h + 2 * (h // cv) // ch, w)


def frame_bytes(h, w, fmt):
    """Bytes of one frame (== refvsr_yuv_frame_bytes; 4:2:0: == refvsr_yuv420_bytes)."""
    r, c = frame_shape(h, w, fmt)
    return r * c * (1 if depth_of(fmt) == 8 else 2)


def source_f64(x):
    """A result array as the float64 source value: floats widened exactly, a byte u as u / 255.0."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.astype(np.float64) / 255.0
    if x.dtype not in (np.float32, np.float16, np.float64):
        raise TypeError('results are float32, float16 or uint8 (got %s)' % x.dtype)
    return x.astype(np.float64)


def chroma_mean(e, sampling='420', siting='centre'):
    """The mean m [h / cv, w / ch] of the unquantised chroma e [h, w] (float64) that one chroma sample stands for."""
    if sampling == '444':
        return e
    if check_siting(siting) == 'centre':
        if sampling == '422':
            return (e[:, 0::2] + e[:, 1::2]) * 0.5
        return ((e[0::2, 0::2] + e[0::2, 1::2]) + (e[1::2, 0::2] + e[1::2, 1::2])) * 0.25
    l = np.maximum(np.arange(0, e.shape[1], 2) - 1, 0)              # the odd column left of the pair, clamped
    if sampling == '422':
        return ((e[:, l] + e[:, 1::2]) + (e[:, 0::2] + e[:, 0::2])) * 0.25
    v = e[0::2] + e[1::2]
    return ((v[:, l] + v[:, 1::2]) + (v[:, 0::2] + v[:, 0::2])) * 0.125


def pre_rounding(rgb, coef, sampling='420', siting='centre'):
    """(oy + sy ey [h, w], oc + sc mcb [h/2, w/2], oc + sc mcr [h/2, w/2]) of one [3, h, w] frame: the values rint sees (the chroma
    planes [h / cv, w / ch] of the sampling)."""
    kr, kg, kb, icb, icr, oy, sy, oc, sc = coef
    v = source_f64(rgb)
    assert v.ndim == 3 and v.shape[0] == 3, 'a frame is [3, h, w]'
    frame_shape(*v.shape[1:])
    r, g, b = v[0], v[1], v[2]
    ey = (kr * r + kg * g) + kb * b
    out = [oy + sy * ey]
    for e in ((b - ey) * icb, (r - ey) * icr):
        out.append(oc + sc * chroma_mean(e, sampling, siting))
    return tuple(out)


def quantise(v, depth):
    """rint (half to even), then the clamp to [0, 2^depth - 1]; float64 in, int64 out."""
    return np.clip(np.rint(v), 0.0, float(2 ** depth - 1)).astype(np.int64)


def pack(y, cb, cr, fmt):
    """Integer code planes -> the frame's buffer [3 h / 2, w] in the format's layout and sample type."""
    d, semi, shift = FORMATS[twin_of(fmt)]
    h, w = y.shape
    dt = dtype_of(fmt)
    c = np.stack([cb, cr], axis=-1).reshape(-1) if semi else np.concatenate([cb.reshape(-1), cr.reshape(-1)])
    flat = np.concatenate([np.asarray(y).reshape(-1), c]).astype(np.int64) << shift
    return flat.astype(dt).reshape(frame_shape(h, w, fmt))


def rgb_to_yuv(rgb, fmt='i422', matrix='bt709', range='limited', siting='centre'):
    """The model of every format and siting: a [3, h, w] result (float32 | float16 | uint8, any strides) -> the frame's buffer
    frame_shape(h, w, fmt); a [B, 3, h, w] batch -> [B, ...]."""
    rgb = np.asarray(rgb)
    if rgb.ndim == 4:
        return np.stack([rgb_to_yuv(f, fmt, matrix, range, siting) for f in rgb])
    d = depth_of(fmt)
    yv, cbv, crv = pre_rounding(rgb, coefficients(fmt, matrix, range), sampling_of(fmt), effective_siting(fmt, siting))
    return pack(quantise(yv, d), quantise(cbv, d), quantise(crv, d), fmt)


def rgb_to_yuv420(rgb, fmt='nv12', matrix='bt709', range='limited'):
    """rgb_to_yuv of a 4:2:0 format, centre-sited: the frame's buffer [3 h / 2, w]."""
    return rgb_to_yuv(rgb, fmt, matrix, range, 'centre')


def planes(buf, h, w, fmt):
    """The (Y [h, w], Cb [h/2, w/2], Cr [h/2, w/2]) views of a frame's buffer (the chroma planes [h / cv, w / ch] of the format's
    sampling); together they tile it exactly."""
    d, semi, _ = FORMATS[twin_of(fmt)]
    cv, ch = SUBSAMPLING[sampling_of(fmt)]
    flat = np.asarray(buf).reshape(-1)
    rows, _ = frame_shape(h, w, fmt)
    assert flat.size == rows * w, 'a %s frame holds %d samples' % (fmt, rows * w)
    n, q = h * w, (h // cv) * (w // ch)
    y = flat[:n].reshape(h, w)
    if semi:
        c = flat[n:].reshape(h // 2, w // 2, 2)
        return y, c[..., 0], c[..., 1]
    return y, flat[n:n + q].reshape(h // cv, w // ch), flat[n + q:].reshape(h // cv, w // ch)


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


def resolve_input(input_yuv, matrix=None, range=None, chroma=None, siting=None):
    """config.input_yuv / input_yuv_matrix / input_yuv_range / input_yuv_chroma / input_yuv_siting checked: None (off) or (format,
    matrix, range, chroma) -- with 'left' behind it where the frames are left-sited (centre, and 4:4:4, keep the four: the arguments of
    ops.yuv420_ingest; the five are those of ops.yuv_ingest); ValueError for a bad name, also while the format is off (as resolve)."""
    m, r, c = check_matrix(matrix or 'bt709'), check_range(range or 'limited'), check_chroma(chroma or 'bilinear')
    s = resolve_siting(siting, 'input_yuv_siting')
    if input_yuv is None:
        return None
    _config_format(input_yuv, 'input_yuv')
    return (input_yuv, m, r, c) if effective_siting(input_yuv, s) == 'centre' else (input_yuv, m, r, c, s)


def decode_coefficients(fmt='nv12', matrix='bt709', range='limited'):
    """The nine doubles (oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg) the decoding model and its kernel both get, computed once in Python
    float64 from coefficients(): the reciprocals are taken here, no division happens on the device."""
    kr, kg, kb, _, _, oy, sy, oc, sc = coefficients(fmt, matrix, range)
    return (oy, 1.0 / sy, oc, 1.0 / sc, 2.0 * (1.0 - kr), 2.0 * (1.0 - kb), kr, kb, 1.0 / kg)


def codes(buf, h, w, fmt):
    """The integer code planes (Y [h, w], Cb [h/2, w/2], Cr [h/2, w/2]; int64) of a frame's buffer."""
    d, _, shift = FORMATS[twin_of(fmt)]
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


def chroma_taps(c, chroma='bilinear', sampling='420', siting='centre'):
    """The integer tap sum 16 m [h, w] of a chroma code plane [h/2, w/2] (int64): 9 C[cy,cx] + 3 C[cy',cx] + 3 C[cy,cx'] + C[cy',cx']
    at every luma pixel, the neighbours clamped at the edges; 'nearest': 16 C[cy,cx].  With a sampling and a siting: the plane is
    [h / cv, w / ch] and the sum is the module text's."""
    if sampling == '444':
        check_chroma(chroma), check_siting(siting)
        return 16 * c
    h2, w2 = c.shape
    cv = SUBSAMPLING[sampling][0]
    y, x = np.arange(cv * h2), np.arange(2 * w2)
    cy, cx = y >> (cv - 1), x >> 1
    if check_chroma(chroma) == 'nearest':
        check_siting(siting)
        return 16 * c[cy][:, cx]
    # two horizontal taps of weights (wa, wb), together 4; then the vertical 3 : 1 of 4:2:0, or x 4
    if check_siting(siting) == 'centre':
        cx2 = np.clip(cx + np.where(x & 1, 1, -1), 0, w2 - 1)
        wa, wb = 3, 1
    else:
        cx2 = np.minimum(cx + 1, w2 - 1)
        wa, wb = np.where(x & 1, 2, 4), np.where(x & 1, 2, 0)
    if sampling == '422':
        return 4 * wa * c[:, cx] + 4 * wb * c[:, cx2]
    cy2 = np.clip(cy + np.where(y & 1, 1, -1), 0, h2 - 1)
    return 3 * wa * c[cy][:, cx] + wa * c[cy2][:, cx] + 3 * wb * c[cy][:, cx2] + wb * c[cy2][:, cx2]


def decode_pre_clamp(buf, h, w, fmt='nv12', matrix='bt709', range='limited', chroma='bilinear', siting='centre'):
    """(r, g, b) float64 [h, w] of one frame before the clamp to [0, 1] and the rounding to float32."""
    oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg = decode_coefficients(fmt, matrix, range)
    yc, cbc, crc = codes(buf, h, w, fmt)
    sampling = sampling_of(fmt)
    ey = (yc.astype(np.float64) - oy) * iy
    ecb = (chroma_taps(cbc, chroma, sampling, siting).astype(np.float64) * 0.0625 - oc) * ic
    ecr = (chroma_taps(crc, chroma, sampling, siting).astype(np.float64) * 0.0625 - oc) * ic
    r = ey + cr_r * ecr
    b = ey + cb_b * ecb
    g = ((ey - kr * r) - kb * b) * ikg
    return r, g, b


def yuv_to_rgb(buf, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear', siting='centre'):
    """The model of the way in for every format and siting: a frame's buffer frame_shape(h, w, fmt) (uint8 | uint16 by format) ->
    float32 [3, h, w] in [0, 1]; a [B, ...] batch -> [B, 3, h, w]."""
    buf = np.asarray(buf)
    if buf.ndim == 3:
        return np.stack([yuv_to_rgb(f, h, w, fmt, matrix, range, chroma, siting) for f in buf])
    if buf.shape != frame_shape(h, w, fmt):
        raise ValueError('a %d x %d %s frame is %s (got %s)' % (h, w, fmt, frame_shape(h, w, fmt), buf.shape))
    return np.stack([np.clip(v, 0.0, 1.0) for v in decode_pre_clamp(buf, h, w, fmt, matrix, range, chroma, siting)]).astype(np.float32)


def yuv420_to_rgb(buf, h, w, fmt, matrix='bt709', range='limited', chroma='bilinear'):
    """yuv_to_rgb of a 4:2:0 format, centre-sited: a frame's buffer [3 h / 2, w], or a [B, 3 h / 2, w] batch."""
    if np.shape(buf)[-2:] != frame_shape(h, w):
        raise ValueError('a %d x %d frame is %s (got %s)' % (h, w, frame_shape(h, w), np.shape(buf)[-2:]))
    return yuv_to_rgb(buf, h, w, fmt, matrix, range, chroma, 'centre')


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


# C tag -> (format, the siting the tag means; None: 4:4:4 has none)
Y4M_TAGS = {'420jpeg': ('i420', 'centre'), '420': ('i420', 'centre'), '420mpeg2': ('i420', 'left'), '420p10': ('i420p10', 'centre'),
            '422': ('i422', 'left'), '422p10': ('i422p10', 'left'), '444': ('i444', None), '444p10': ('i444p10', None)}
Y4M_DEFAULT_SITING = {'420': 'centre', '422': 'left', '444': 'centre'}        # of a sampling, where nobody says otherwise


def y4m_tag(fmt, siting=None):
    """(C tag, XCHROMASITING value or None) of a planar format; siting None: the sampling's default."""
    if fmt in PLANAR_TWIN:
        raise ValueError("%r is not a Y4M format (Y4M frames are planar): use %r" % (fmt, PLANAR_TWIN[fmt]))
    sampling, p10 = sampling_of(fmt), 'p10' if depth_of(fmt) == 10 else ''
    siting = effective_siting(fmt, Y4M_DEFAULT_SITING[sampling] if siting is None else siting)
    if sampling == '420':
        tag = ('420jpeg' if siting == 'centre' else '420mpeg2') if not p10 else '420p10'
    else:
        tag = sampling + p10
    means = Y4M_TAGS[tag][1]
    return 'C' + tag, None if means is None or means == siting else siting.upper()


def y4m_header(h, w, fmt, fps=(30, 1), range='limited', siting=None):
    frame_shape(h, w, check_format(fmt))
    tag, extra = y4m_tag(fmt, siting)
    return ('YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s%s\n' % (w, h, fps[0], fps[1], tag, check_range(range).upper(),
                                                                        ' XCHROMASITING=%s' % extra if extra else '')).encode('ascii')


def sink_name(f):
    """What messages call a source or a sink: the path, '<stdin>' / '<stdout>' style names of file objects, '-' as it is."""
    return f if isinstance(f, str) else str(getattr(f, 'name', None) or '<%s>' % type(f).__name__)


class Y4MWriter(object):
    """A .y4m file of 'i420' (C420jpeg) or 'i420p10' (C420p10, little-endian samples) frames: the header, then `FRAME\\n` and the
    planes Y, Cb, Cr per frame -- which is the frame's buffer as it lies in memory.  Also 'i422', 'i444' and their 10-bit forms, and
    a siting (y4m_tag has the tags; None: the sampling's default).
    path: a path, '-' (sys.stdout.buffer) or a binary file object -- a pipe to an encoder; close() flushes and closes only a file
    opened here.  A sink that went away (BrokenPipeError) is a one-line ValueError naming it."""

    def __init__(self, path, h, w, fmt='i420', fps=(30, 1), range='limited', siting=None):
        self.header = y4m_header(h, w, fmt, fps, range, siting)
        self.h, self.w, self.fmt = h, w, fmt
        self.frames = 0
        self.name = sink_name(path)
        self.owned = not (path == '-' or hasattr(path, 'write'))
        self.fh = open(path, 'wb') if self.owned else sys.stdout.buffer if path == '-' else path
        try:
            self._put(self.header)
        except Exception:
            self.fh, fh = None, self.fh
            if self.owned:
                fh.close()
            raise

    def _put(self, *parts):
        try:
            for p in parts:
                self.fh.write(p)
        except BrokenPipeError:
            raise ValueError('%s: the sink closed the pipe behind frame %d' % (self.name, self.frames))

    def write(self, buf):
        a = np.asarray(buf)
        if a.shape != frame_shape(self.h, self.w, self.fmt) or a.dtype != dtype_of(self.fmt):
            raise ValueError('Y4MWriter: %s frames are %s %s (got %s %s)' % (self.fmt, np.dtype(dtype_of(self.fmt)).name,
                                                                          frame_shape(self.h, self.w, self.fmt), a.dtype, a.shape))
        self._put(b'FRAME\n', np.ascontiguousarray(a).astype(a.dtype.newbyteorder('<'), copy=False).tobytes())
        self.frames += 1

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


def parse_y4m_header(line, path):
    """The header line (without its newline) -> dict(h, w, fps, fmt, range, siting); siting is 'centre' for 4:4:4."""
    tok = line.decode('ascii', 'replace').split(' ')
    if tok[0] != 'YUV4MPEG2':
        raise ValueError('%s: not a YUV4MPEG2 file' % path)
    f = dict((t[0], t[1:]) for t in tok[1:] if t and t[0] != 'X')
    x = dict(t[1:].split('=', 1) for t in tok[1:] if t and t[0] == 'X' and '=' in t)
    for k in 'WHF':
        if k not in f:
            raise ValueError('%s: the YUV4MPEG2 header has no %s token' % (path, k))
    if f.get('I', 'p') not in ('p', '?'):
        raise ValueError('%s: interlaced file (I%s): only progressive frames are read' % (path, f['I']))
    tag = f.get('C', '420')                                          # no C token: 4:2:0, the format's default
    if tag not in Y4M_TAGS:
        why = 'top-left sited chroma' if tag == '420paldv' else 'no chroma' if tag.startswith('mono') else 'unknown chroma tag'
        raise ValueError('%s: C%s (%s) is not read: one of %s' % (path, tag, why, ', '.join('C' + k for k in Y4M_TAGS)))
    fmt, siting = Y4M_TAGS[tag]
    said = x.get('CHROMASITING')
    if said is not None:
        if said.lower() not in SITINGS:
            raise ValueError('%s: XCHROMASITING=%s: LEFT or CENTRE' % (path, said))
        siting = said.lower()
    try:
        h, w = int(f['H']), int(f['W'])
        frame_shape(h, w, fmt)
    except ValueError as e:
        raise ValueError('%s: %s' % (path, e))
    return {'h': h, 'w': w, 'fps': parse_fps(f['F']), 'fmt': fmt, 'range': x.get('COLORRANGE', 'LIMITED').lower(),
            'siting': effective_siting(fmt, siting or 'centre')}


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
        self.h, self.w, self.fps, self.fmt, self.range, self.siting = hd['h'], hd['w'], hd['fps'], hd['fmt'], hd['range'], hd['siting']
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
        return np.frombuffer(raw, dtype=np.dtype(dt).newbyteorder('<')).astype(dt).reshape(frame_shape(self.h, self.w, self.fmt))

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


class StreamStopped(Exception):
    """Y4MStreamReader: its `stop` event was set while it waited for data."""


class Y4MStreamReader(object):
    """A Y4M stream read strictly front to back -- a pipe from a decoder: no seek, no stat, so `length` is None and the end shows
    when it comes.  source: a path (a regular file or a FIFO; opened unbuffered), '-' (sys.stdin.buffer) or a binary file object.
    The attributes of Y4MReader (h, w, fps, fmt, range, siting, frames); read() returns the next frame buffer or None at a clean end
    of the stream, readinto(buf) fills a caller's writable, C-contiguous array of the frame's shape and dtype (a pinned staging buffer)
    and returns True, or False at the end.  Every read loops over short reads: a pipe delivers what is there.  A frame marker is a
    line -- `FRAME`, optional space-separated parameters, `\\n`, at most 80 bytes; a stream that ends inside a frame raises
    ValueError('..: truncated frame k').  The header goes through parse_y4m_header: what Y4MReader refuses is refused here, in the
    same words.
    stop (None, or an object with is_set(): a threading.Event): where the source is an unbuffered descriptor (a path, '-', a raw
    file object), a wait for data ends with StreamStopped within 0.1 s of the event -- a reader thread can always be ended."""

    length = None

    def __init__(self, source, stop=None):
        self.path = sink_name(source)
        self.stop = stop
        self.owned = isinstance(source, str) and source != '-'
        if self.owned:
            self.fh = open(source, 'rb', buffering=0)
        elif source == '-':
            self.fh = getattr(sys.stdin.buffer, 'raw', sys.stdin.buffer)       # (nothing is buffered yet when a run starts)
        else:
            self.fh = source
        self._fd = None
        if isinstance(self.fh, io.RawIOBase):                                   # unbuffered: the descriptor says whether data waits
            try:
                self._fd = self.fh.fileno()
            except (OSError, ValueError, AttributeError):
                self._fd = None
        self.frames = 0
        try:
            line = bytearray()
            while not line.endswith(b'\n') and len(line) < 4096:                # byte by byte: nothing behind the newline is taken
                c = self._some(1)
                if not c:
                    break
                line += c
            if not line.endswith(b'\n'):
                raise ValueError('%s: not a YUV4MPEG2 file' % self.path)
            hd = parse_y4m_header(bytes(line[:-1]), self.path)
        except Exception:
            self.close()
            raise
        self.h, self.w, self.fps, self.fmt, self.range, self.siting = hd['h'], hd['w'], hd['fps'], hd['fmt'], hd['range'], hd['siting']

    def _wait(self):
        if self._fd is not None and self.stop is not None:
            while not select.select([self._fd], [], [], 0.1)[0]:
                if self.stop.is_set():
                    raise StreamStopped(self.path)

    def _some(self, n):
        """Up to n bytes, b'' at the end of the stream."""
        while True:
            self._wait()
            got = self.fh.read(n)
            if got is not None:                                                 # (None: a non-blocking descriptor without data)
                return got

    def _fill(self, view):
        """Reads until `view` (a byte memoryview) is full; the bytes read -- less than len(view) only at the end of the stream."""
        pos, into = 0, getattr(self.fh, 'readinto', None)
        while pos < len(view):
            self._wait()
            if into is not None:
                k = into(view[pos:])
            else:
                got = self.fh.read(len(view) - pos)
                k = None if got is None else len(got)
                if k:
                    view[pos:pos + k] = got
            if k is None:
                continue
            if k == 0:
                break
            pos += k
        return pos

    def _marker(self):
        """The FRAME line of the next frame: True, or False at a clean end of the stream."""
        mark = bytearray(6)
        k = self._fill(memoryview(mark))
        if k == 0:
            return False
        bad = k < 6 or bytes(mark[:5]) != b'FRAME' or mark[5:6] not in (b'\n', b' ')
        while not bad and not mark.endswith(b'\n'):                             # parameters: to the end of the line
            c = self._some(1)
            mark += c
            bad = not c or len(mark) > 80
        if bad:
            raise ValueError('%s: FRAME marker expected before frame %d' % (self.path, self.frames))
        return True

    def readinto(self, buf):
        shape, dt = frame_shape(self.h, self.w, self.fmt), np.dtype(dtype_of(self.fmt))
        if not isinstance(buf, np.ndarray) or buf.shape != shape or buf.dtype != dt or not buf.flags.c_contiguous or not buf.flags.writeable:
            raise ValueError('%s: readinto needs a writable, contiguous %s array of shape %s (got %s)' % (
                self.path, dt.name, shape, '%s %s' % (buf.dtype, buf.shape) if isinstance(buf, np.ndarray) else type(buf).__name__))
        if not self._marker():
            return False
        view = memoryview(buf).cast('B')
        if self._fill(view) != len(view):
            raise ValueError('%s: truncated frame %d' % (self.path, self.frames))
        if sys.byteorder == 'big' and dt.itemsize > 1:                          # (the stream's samples are little-endian)
            buf.byteswap(True)
        self.frames += 1
        return True

    def read(self):
        buf = np.empty(frame_shape(self.h, self.w, self.fmt), dtype_of(self.fmt))
        return buf if self.readinto(buf) else None

    def __iter__(self):
        while True:
            f = self.read()
            if f is None:
                return
            yield f

    def close(self):
        if self.fh is not None:
            fh, self.fh = self.fh, None
            if self.owned:
                fh.close()

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
        frames.append(np.frombuffer(raw, dtype=np.dtype(dtype_of(fmt)).newbyteorder('<')).astype(dtype_of(fmt)).reshape(frame_shape(h, w, fmt)))
        pos += nbytes
    return dict(hd, frames=frames)
