"""Crafted frames and wrong-model controls for the Y'CbCr 4:2:0 -> RGB conversion on the way in (refvsr_amd/yuv.py:yuv420_to_rgb is the
model, csrc/yuv_in.hip the kernel).  Pure numpy; shared by tests/test_yuv_in.py (the model) and tests/test_gpu_yuv_in.py (the kernel).

A case is (name, fmt, h, w, buf): one frame's buffer [3h/2, w] in the format's layout and sample type.  Every format's set holds
  random      random codes over the whole code range (about 28 % of the decoded samples leave [0, 1]: both clamp sides)
  ingamut     rgb_to_yuv420 of smooth RGB in [0.1, 0.9]: fewer than 5 % of the samples are clamped (the unclamped interior)
  allcodes    every code of every plane (256, or 1024)
  tiny        2 x 2: one chroma block, every tap clamped
and p010 a case with dirty low bits, i420p10 one with dirty high bits (both are ignored by the model).
"""
import numpy as np

from refvsr_amd import yuv

FORMATS = ('nv12', 'i420', 'p010', 'i420p10')
ANCHORS = (((16, 128, 128), (0.0, 0.0, 0.0)), ((235, 128, 128), (1.0, 1.0, 1.0)), ((63, 102, 240), (1.0, 0.00229273, 0.0)),
           ((32, 240, 118), (0.0027558, 0.00029563, 1.0)), ((173, 42, 26), (0.0, 1.0, 0.0044771)))

_CACHE = {}


def constant_frame(code, fmt, h=4, w=4):
    """A frame of one (Y, Cb, Cr) code triple (codes of the format's depth)."""
    return yuv.pack(np.full((h, w), code[0]), np.full((h // 2, w // 2), code[1]), np.full((h // 2, w // 2), code[2]), fmt)


def random_codes(rs, h, w, fmt):
    top = 2 ** yuv.depth_of(fmt)
    return yuv.pack(rs.randint(0, top, (h, w)), rs.randint(0, top, (h // 2, w // 2)), rs.randint(0, top, (h // 2, w // 2)), fmt)


def smooth_rgb(rs, h, w):
    """RGB in [0.1, 0.9]: a low-frequency colour field plus a little noise (neighbouring chroma blocks nearly agree)."""
    y, x = np.mgrid[0:h, 0:w]
    ph = rs.rand(3, 2) * 6.0
    base = np.stack([0.5 + 0.3 * np.sin(ph[c, 0] + 0.11 * y) * np.cos(ph[c, 1] + 0.07 * x) for c in range(3)])
    return np.clip(base + 0.02 * (rs.rand(3, h, w) - 0.5), 0.1, 0.9).astype(np.float32)


def all_codes(rs, fmt):
    n = 2 ** yuv.depth_of(fmt)
    s = int(round(np.sqrt(n)))                       # chroma planes of s x s hold each code once, the luma plane four times
    y = rs.permutation(np.tile(np.arange(n), 4)).reshape(2 * s, 2 * s)
    return 2 * s, 2 * s, yuv.pack(y, rs.permutation(n).reshape(s, s), rs.permutation(n).reshape(s, s), fmt)


def cases(fmt):
    """[(name, fmt, h, w, buf)] of one format, built once and left unchanged."""
    if fmt not in _CACHE:
        rs = np.random.RandomState(7 + yuv.FORMAT_IDS[fmt])
        out = [('random', fmt, 6, 10, random_codes(rs, 6, 10, fmt)),
               ('ingamut', fmt, 18, 26, yuv.rgb_to_yuv420(smooth_rgb(rs, 18, 26), fmt)),
               ('tiny', fmt, 2, 2, random_codes(rs, 2, 2, fmt))]
        h, w, buf = all_codes(rs, fmt)
        out.append(('allcodes', fmt, h, w, buf))
        if fmt == 'p010':
            dirty = random_codes(rs, 6, 10, fmt) | rs.randint(0, 64, (9, 10)).astype(np.uint16)
            out.append(('dirty_low', fmt, 6, 10, dirty))
        if fmt == 'i420p10':
            dirty = random_codes(rs, 6, 10, fmt) | (rs.randint(0, 64, (9, 10)) << 10).astype(np.uint16)
            out.append(('dirty_high', fmt, 6, 10, dirty))
        for c in out:
            c[4].setflags(write=False)
        _CACHE[fmt] = out
    return _CACHE[fmt]


def case(fmt, name):
    return next(c for c in cases(fmt) if c[0] == name)


def tap_classes(h, w):
    """Counts of the luma pixels of an h x w frame by the position of their chroma taps: corner (both neighbours clamped), top / bottom
    and left / right edge (one clamped), interior; and by the parities of y and x."""
    y, x = np.mgrid[0:h, 0:w]
    ey, ex = (y == 0) | (y == h - 1), (x == 0) | (x == w - 1)
    out = {'corner': int((ey & ex).sum()), 'top': int(((y == 0) & ~ex).sum()), 'bottom': int(((y == h - 1) & ~ex).sum()),
           'left': int(((x == 0) & ~ey).sum()), 'right': int(((x == w - 1) & ~ey).sum()), 'interior': int((~ey & ~ex).sum())}
    for py in (0, 1):
        for px in (0, 1):
            out['parity%d%d' % (py, px)] = int((((y & 1) == py) & ((x & 1) == px)).sum())
    return out


def clamp_classes(c, matrix='bt709', range='limited', chroma='bilinear'):
    """Counts of a case's decoded samples below 0, inside [0, 1] and above 1, before the clamp."""
    v = np.stack(yuv.decode_pre_clamp(c[4], c[2], c[3], c[1], matrix, range, chroma))
    return {'below': int((v < 0).sum()), 'inside': int(((v >= 0) & (v <= 1)).sum()), 'above': int((v > 1).sum())}


# ------------------------------------------------------------------------------------------------ wrong models
def taps_int(c, wrap=False, cosited=False):
    """The integer tap sum 16 m of a chroma code plane, written out pixel by pixel (independent of yuv.chroma_taps).  wrap: the edge
    taps wrap around instead of being clamped.  cosited: horizontally left co-sited chroma (even x: the block's own sample, odd x: the
    mean of the block's and the next one's), vertically centre-sited."""
    h2, w2 = c.shape
    out = np.zeros((2 * h2, 2 * w2), dtype=np.int64)
    for y in range(2 * h2):
        for x in range(2 * w2):
            cy, cx = y >> 1, x >> 1
            cy2, cx2 = cy + (1 if y & 1 else -1), cx + (1 if x & 1 else -1)
            if wrap:
                cy2, cx2 = cy2 % h2, cx2 % w2
            else:
                cy2, cx2 = min(max(cy2, 0), h2 - 1), min(max(cx2, 0), w2 - 1)
            if cosited:
                cxn = min(cx + 1, w2 - 1)
                near, far = (2 * c[cy, cx], 2 * c[cy2, cx]) if x % 2 == 0 else (c[cy, cx] + c[cy, cxn], c[cy2, cx] + c[cy2, cxn])
                out[y, x] = 6 * near + 2 * far                      # (3/4, 1/4 vertically; sixteenths)
            else:
                out[y, x] = 9 * c[cy, cx] + 3 * c[cy2, cx] + 3 * c[cy, cx2] + c[cy2, cx2]
    return out


def decode(planes, coef, taps=taps_int, dtype=np.float64, clamp=True):
    """The model's pixel arithmetic over integer code planes (Y, Cb, Cr), with the parts a control replaces: the tap sum, the
    arithmetic type (every operation rounded to `dtype`), the clamp."""
    f = dtype
    oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg = (f(v) for v in coef)
    yc, cbc, crc = planes
    ey = (yc.astype(f) - oy) * iy
    ecb = (taps(cbc).astype(f) * f(0.0625) - oc) * ic
    ecr = (taps(crc).astype(f) * f(0.0625) - oc) * ic
    r = ey + cr_r * ecr
    b = ey + cb_b * ecb
    g = ((ey - kr * r) - kb * b) * ikg
    v = np.stack([r, g, b])
    assert v.dtype == f
    return (np.clip(v, f(0.0), f(1.0)) if clamp else v).astype(np.float32)


def controls(fmt):
    """{name: (case, wrong result float32 [3, h, w])}: each wrong model on a case of this format built to show it (tests assert that
    it differs from the model on at least one sample)."""
    rnd, gam = case(fmt, 'random'), case(fmt, 'ingamut')
    _, _, h, w, buf = rnd
    coef = yuv.decode_coefficients(fmt)
    pl = yuv.codes(buf, h, w, fmt)
    gpl = yuv.codes(gam[4], gam[2], gam[3], fmt)
    out = {
        'nearest': (rnd, yuv.yuv420_to_rgb(buf, h, w, fmt, chroma='nearest')),
        'cosited': (rnd, decode(pl, coef, taps=lambda c: taps_int(c, cosited=True))),
        'swapped': (rnd, decode((pl[0], pl[2], pl[1]), coef)),
        'matrix': (gam, yuv.yuv420_to_rgb(gam[4], gam[2], gam[3], fmt, matrix='bt601')),
        'range': (gam, yuv.yuv420_to_rgb(gam[4], gam[2], gam[3], fmt, range='full')),
        'noclamp': (rnd, decode(pl, coef, clamp=False)),
        'float32': (gam, decode(gpl, coef, dtype=np.float32)),
        'wrapped': (rnd, decode(pl, coef, taps=lambda c: taps_int(c, wrap=True))),
        # the other chroma layout: interleaved read as planar, or planar read as interleaved
        'layout': (rnd, decode(_relayout(buf, h, w, fmt), coef)),
    }
    if fmt == 'p010':
        raw = tuple(p.astype(np.int64) & 1023 for p in yuv.planes(buf, h, w, fmt))
        out['noshift'] = (rnd, decode(raw, coef))
    return out


def _relayout(buf, h, w, fmt):
    """The code planes of a frame whose chroma is read in the OTHER layout (semi-planar as planar and the reverse)."""
    d, semi, shift = yuv.FORMATS[fmt]
    flat = (np.asarray(buf).reshape(-1).astype(np.int64) >> shift) & (2 ** d - 1)
    n, q = h * w, h * w // 4
    y = flat[:n].reshape(h, w)
    if semi:                                             # read as planar: Cb is the first half of the interleaved run
        return y, flat[n:n + q].reshape(h // 2, w // 2), flat[n + q:].reshape(h // 2, w // 2)
    c = flat[n:].reshape(h // 2, w // 2, 2)
    return y, c[..., 0], c[..., 1]
