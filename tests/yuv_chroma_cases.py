"""Crafted frames and wrong-model controls for the samplings and sitings of refvsr_amd/yuv.py (rgb_to_yuv, yuv_to_rgb: the models of
refvsr_result_to_yuv and refvsr_yuv_to_rgb).  Shared by tests/test_yuv_chroma.py (the model on its own) and
tests/test_gpu_yuv_chroma.py (the kernels against the model on the same frames).  Pure numpy.

A control is the model with one deliberate mistake; out_controls() / IN_CONTROLS name, for every control, the case whose output the
mistake changes -- a control that changes nothing would show that the cases cannot see that mistake."""
import numpy as np

from refvsr_amd import yuv

NEW_FORMATS = ('i422', 'i444', 'i422p10', 'i444p10')
# every valid (format, siting): four 4:2:0 formats x 2, two 4:2:2 x 2, two 4:4:4 (siting means nothing there)
PAIRS = tuple((f, s) for f in ('nv12', 'i420', 'p010', 'i420p10', 'i422', 'i422p10') for s in ('centre', 'left')) + (('i444', 'centre'), ('i444p10', 'centre'))
# the pairs the 4:2:0 / centre kernels do not serve
NEW_PAIRS = tuple(p for p in PAIRS if not (p[0] in yuv.FORMATS and p[1] == 'centre'))
MODES = (('bt709', 'limited'), ('bt709', 'full'), ('bt601', 'limited'))
SIZES = ((2, 2), (2, 4), (4, 2), (6, 10), (18, 26), (34, 70), (270, 480), (4, 1040))

# uint8 2 x 4 frames (row-major) of ONE channel, the other two zero, at bt709 / full range: the pre-rounding value of the LAST chroma
# sample of a row (for left siting: the one that reads the column in front of its pair) is exactly k + 0.5; `down`: k is even, rint
# rounds down.  Found by search, as the blocks of tests/yuv_cases.py; (format, siting) -> ((channel, bytes, down), ...)
TIE_FRAMES = {
    ('i420', 'left'): (('r', (251, 121, 199, 12, 148, 59, 200, 202), True), ('r', (180, 74, 254, 25, 137, 238, 246, 159), False),
                       ('b', (92, 83, 179, 213, 113, 16, 96, 154), False)),
    ('nv12', 'left'): (('r', (125, 223, 76, 183, 166, 239, 133, 177), False), ('r', (175, 128, 200, 234, 81, 64, 153, 188), True),
                       ('b', (139, 65, 249, 21, 136, 31, 249, 47), True)),
    ('i422', 'centre'): (('b', (206, 125, 82, 108, 194, 226, 98, 212), False), ('r', (218, 78, 145, 154, 160, 159, 89, 49), True),
                         ('r', (244, 117, 201, 114, 54, 102, 173, 237), True)),
    ('i422', 'left'): (('r', (18, 101, 43, 127, 56, 204, 135, 242), False), ('r', (113, 223, 63, 103, 100, 98, 61, 222), True),
                       ('b', (86, 74, 165, 64, 179, 140, 250, 187), True)),
    ('i444', 'centre'): (('b', (167, 161, 126, 152, 127, 135, 68, 209), True), ('r', (252, 48, 55, 51, 111, 255, 229, 115), False),
                         ('r', (153, 17, 50, 191, 122, 17, 235, 252), False)),
    ('i420p10', 'left'): (('b', (65, 153, 62, 42, 5, 76, 69, 147), True), ('r', (227, 251, 57, 59, 33, 98, 62, 34), True)),
    ('p010', 'left'): (('r', (205, 102, 3, 207, 225, 141, 61, 102), True), ('b', (88, 32, 87, 121, 70, 100, 81, 91), True)),
    ('i422p10', 'centre'): (('r', (57, 194, 16, 154, 194, 233, 164, 16), True), ('b', (19, 177, 89, 16, 23, 3, 30, 140), True)),
    ('i422p10', 'left'): (('r', (198, 60, 30, 220, 15, 179, 180, 155), True), ('b', (207, 62, 119, 40, 218, 114, 231, 26), True)),
    ('i444p10', 'centre'): (('b', (77, 150, 78, 85, 83, 202, 3, 223), True), ('r', (55, 24, 10, 233, 147, 208, 219, 85), True)),
}


def tie_frame(channel, values):
    a = np.zeros((3, 2, 4), np.uint8)
    a['rgb'.index(channel)] = np.array(values, np.uint8).reshape(2, 4)
    return a


def tie_cases():
    """(format, siting, frame [3, 2, 4] uint8, chroma plane index 1 = Cb | 2 = Cr, rounds down) of every crafted tie; matrix bt709,
    range full."""
    return [(fmt, siting, tie_frame(ch, u), 1 if ch == 'b' else 2, down) for (fmt, siting), ts in sorted(TIE_FRAMES.items()) for ch, u, down in ts]


def tie_mask(frame, fmt, siting, plane):
    v = yuv.pre_rounding(frame, yuv.coefficients(fmt, 'bt709', 'full'), yuv.sampling_of(fmt), yuv.effective_siting(fmt, siting))[plane]
    return v == np.floor(v) + 0.5


def detail(h=6, w=10, dtype=np.uint8, seed=7):
    """Every pixel differs from its neighbours."""
    g = np.random.RandomState(seed)
    return g.randint(0, 256, (3, h, w)).astype(np.uint8) if dtype == np.uint8 else g.rand(3, h, w).astype(dtype)


def random_codes(rs, h, w, fmt, dirty=True):
    """One frame of random codes in the format's layout; dirty: the bits of a 10-bit sample that the model ignores set at random
    (p010: the low six, the planar 10-bit formats: the high six)."""
    d, _, shift = yuv.FORMATS[yuv.twin_of(fmt)]
    shape = yuv.frame_shape(h, w, fmt)
    x = (rs.randint(0, 2 ** d, shape).astype(np.int64) << shift)
    if dirty and d == 10:
        x = x | (rs.randint(0, 64, shape) << (0 if shift else 10))
    return x.astype(yuv.dtype_of(fmt))


# ------------------------------------------------------------------------------------------------ wrong models, the way out
def out_control(control, rgb, fmt, siting):
    """yuv.rgb_to_yuv (bt709, full) with one mistake."""
    d, sampling = yuv.depth_of(fmt), yuv.sampling_of(fmt)
    siting = yuv.effective_siting(fmt, siting)
    kr, kg, kb, icb, icr, oy, sy, oc, sc = yuv.coefficients(fmt, 'bt709', 'full')
    r, g, b = yuv.source_f64(rgb)
    ey = (kr * r + kg * g) + kb * b
    planes = [yuv.quantise(oy + sy * ey, d)]
    for e in ((b - ey) * icb, (r - ey) * icr):
        w = e.shape[1]
        j2 = np.arange(0, w, 2)
        if control == 'swap_siting':
            m = yuv.chroma_mean(e, sampling, 'left' if siting == 'centre' else 'centre')
        elif control == 'mirror_edge':                       # [1 2 1] with the left edge mirrored: column 1 in front of column 0
            l = np.abs(j2 - 1)
            v = e if sampling == '422' else e[0::2] + e[1::2]
            m = ((v[:, l] + v[:, 1::2]) + (v[:, 0::2] + v[:, 0::2])) * (0.25 if sampling == '422' else 0.125)
        elif control == 'h_before_v':                        # 4:2:0 left: each row's [1 2 1] first, then the two rows
            l = np.maximum(j2 - 1, 0)
            hs = (e[:, l] + e[:, 1::2]) + (e[:, 0::2] + e[:, 0::2])
            m = (hs[0::2] + hs[1::2]) * 0.125
        elif control == 'avg_vertical_422':                  # 4:2:2 taken for 4:2:0: every row pair shares its mean
            m = np.repeat(yuv.chroma_mean(e, '420', siting), 2, axis=0)
        elif control == 'filter_444':                        # 4:4:4 chroma low-passed as if it were to be decimated
            p = np.pad(e, ((0, 0), (1, 1)), mode='edge')
            m = ((p[:, :-2] + p[:, 2:]) + (p[:, 1:-1] + p[:, 1:-1])) * 0.25
        else:
            m = yuv.chroma_mean(e, sampling, siting)
        planes.append(yuv.quantise(oc + sc * m, d))
    if control == 'swap_cbcr':
        planes[1], planes[2] = planes[2], planes[1]
    return yuv.pack(planes[0], planes[1], planes[2], fmt)


# a tie of 4:2:0 left (found by search among 13 044 ties) that the other order of the same eight additions moves off the tie, to the
# other side of rint: the two orders agree on nearly every frame, being the same sum up to float64 rounding
H_BEFORE_V_FRAME = ('r', (254, 69, 84, 233, 190, 143, 235, 232))


def out_controls():
    """[(control, frame, format, siting)]: the cases built to see each control."""
    edge = np.zeros((3, 2, 4), np.uint8)
    edge[2, :, 1] = 255                                      # one blue column at x = 1: the mirrored edge counts it twice for pair 0
    return [('swap_siting', detail(), 'i422', 'left'), ('swap_siting', detail(), 'i420', 'centre'),      # left as centre, centre as left
            ('mirror_edge', edge, 'i422', 'left'), ('mirror_edge', edge, 'i420p10', 'left'),
            ('h_before_v', tie_frame(*H_BEFORE_V_FRAME), 'i420', 'left'),
            ('avg_vertical_422', detail(), 'i422p10', 'centre'),
            ('swap_cbcr', detail(), 'i444', 'centre'),
            ('filter_444', detail(), 'i444p10', 'centre')]


# ------------------------------------------------------------------------------------------------ wrong models, the way in
def in_control_taps(control, c, sampling, siting):
    """yuv.chroma_taps ('bilinear') with one mistake in the horizontal neighbour."""
    if control == 'swap_siting':
        return yuv.chroma_taps(c, 'bilinear', sampling, 'left' if siting == 'centre' else 'centre')
    if control == 'filter_444':                              # 4:4:4 chroma low-passed as if it had been decimated
        p = np.pad(c, ((0, 0), (1, 1)), mode='edge')
        return 4 * p[:, :-2] + 8 * c + 4 * p[:, 2:]
    if control not in ('wrong_end', 'mirror_edge'):
        return yuv.chroma_taps(c, 'bilinear', sampling, siting)
    h2, w2 = c.shape
    x = np.arange(2 * w2)
    cx = x >> 1
    if siting == 'centre':
        n, wa, wb = cx + np.where(x & 1, 1, -1), 3, 1
    else:
        n, wa, wb = cx + (-1 if control == 'wrong_end' else 1), np.where(x & 1, 2, 4), np.where(x & 1, 2, 0)     # wrong_end: the LEFT neighbour
    if control == 'mirror_edge':                             # the column beyond an edge is the one inside it, not the edge column again
        cx2 = np.where(n < 0, 1, np.where(n > w2 - 1, w2 - 2, n))
    else:
        cx2 = np.clip(n, 0, w2 - 1)
    if sampling == '422':
        return 4 * wa * c[:, cx] + 4 * wb * c[:, cx2]
    y = np.arange(2 * h2)
    cy = y >> 1
    cy2 = np.clip(cy + np.where(y & 1, 1, -1), 0, h2 - 1)
    return 3 * wa * c[cy][:, cx] + wa * c[cy2][:, cx] + 3 * wb * c[cy][:, cx2] + wb * c[cy2][:, cx2]


def in_control(control, buf, h, w, fmt, siting):
    """yuv.yuv_to_rgb (bt709, limited, bilinear) with one mistake: the arithmetic behind the tap sum written out again."""
    oy, iy, oc, ic, cr_r, cb_b, kr, kb, ikg = yuv.decode_coefficients(fmt, 'bt709', 'limited')
    yc, cbc, crc = yuv.codes(buf, h, w, fmt)
    if control == 'swap_cbcr':
        cbc, crc = crc, cbc
    sampling, siting = yuv.sampling_of(fmt), yuv.effective_siting(fmt, siting)
    ey = (yc.astype(np.float64) - oy) * iy
    ecb = (in_control_taps(control, cbc, sampling, siting).astype(np.float64) * 0.0625 - oc) * ic
    ecr = (in_control_taps(control, crc, sampling, siting).astype(np.float64) * 0.0625 - oc) * ic
    r = ey + cr_r * ecr
    b = ey + cb_b * ecb
    g = ((ey - kr * r) - kb * b) * ikg
    return np.stack([np.clip(v, 0.0, 1.0) for v in (r, g, b)]).astype(np.float32)


# (control, format, siting): the frames are random codes, 6 x 10
IN_CONTROLS = (('swap_siting', 'i420', 'left'), ('swap_siting', 'i422', 'centre'), ('wrong_end', 'i422', 'left'), ('wrong_end', 'nv12', 'left'),
               ('mirror_edge', 'i420', 'centre'), ('mirror_edge', 'i422p10', 'left'), ('swap_cbcr', 'p010', 'left'), ('swap_cbcr', 'i444', 'centre'),
               ('filter_444', 'i444', 'centre'))
