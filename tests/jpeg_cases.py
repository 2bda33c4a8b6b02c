"""The cases of tests/test_jpeg.py (CPU: the model against Pillow and against its own wrong readings) and tests/test_gpu_jpeg.py (the
kernels against the model): the validity matrix, the sources and the crafted frames.  Pure numpy; frames are the dense 'i420' / 'i444'
buffers refvsr_amd/jpeg.py codes.

Crafted frames are built in the coefficient domain where a path needs particular coefficients: `from_coefficients` inverts the DCT of
the wanted (zigzag position -> value) times the quantiser and rounds to pixels; at quality 50 the pixel rounding (at most 1/2 per pixel)
moves a coefficient by far less than half a quantiser step (>= 10), so exactly the wanted values come out.  The tie and the 0xFF frames
were found by search (fixed vectors and seeds below); every test that uses one asserts from the symbol stream or the transform that
the path it is named after is taken.
"""
import numpy as np

from refvsr_amd import jpeg, yuv

FORMATS = ('i420', 'i444')
QUALITIES = (1, 50, 75, 90, 100)
SIZES = ((2, 2), (8, 8), (16, 16), (18, 34), (30, 50), (136, 240))


def restarts(h, w, fmt):
    """R of the matrix: 1, 3, one MCU row, more than the frame's MCUs."""
    my, mx, _ = jpeg.geometry(h, w, fmt)
    return (1, 3, mx, my * mx + 5)


def natural_rgb(h, w, seed=0):
    """A natural-like uint8 [3, h, w] frame: the ground-truth frame of synth.make_clip, cropped."""
    from refvsr_amd.synth import make_clip
    gt = make_clip(1, (h + 3) // 4, (w + 3) // 4, seed=seed)[2][0].numpy()
    return np.rint(np.clip(gt[:, :h, :w], 0.0, 1.0) * 255.0).astype(np.uint8)


def noise_rgb(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (3, h, w), dtype=np.uint8)


def to_yuv(rgb, fmt):
    """The frame JFIF means: BT.601, full range, centre-sited."""
    return yuv.rgb_to_yuv(rgb, fmt, 'bt601', 'full', 'centre')


_MATRIX_FRAMES = {}


def matrix_frame(h, w, fmt):
    """The frame of a matrix case (made once): natural-like, noise added so that high frequencies survive quality 90."""
    key = (h, w, fmt)
    if key not in _MATRIX_FRAMES:
        rgb = natural_rgb(h, w, seed=3).astype(np.int64) + np.random.default_rng(h * 1000 + w).integers(-12, 13, (3, h, w))
        _MATRIX_FRAMES[key] = to_yuv(np.clip(rgb, 0, 255).astype(np.uint8), fmt)
    return _MATRIX_FRAMES[key]


def matrix():
    """(fmt, quality, h, w, R) of the validity matrix."""
    return [(fmt, q, h, w, r) for fmt in FORMATS for q in QUALITIES for h, w in SIZES for r in restarts(h, w, fmt)]


# ------------------------------------------------------------------------------------------------ crafted frames
def idct(F):
    C = jpeg.dct_table()
    return C.T @ np.asarray(F, np.float64) @ C


def from_coefficients(coefs, q):
    """An 8 x 8 uint8 block whose quantised coefficients are {zigzag position: value} under the table q (natural order)."""
    F = np.zeros(64)
    for k, v in coefs.items():
        F[jpeg.ZIGZAG[k]] = v * int(q[jpeg.ZIGZAG[k]])
    px = np.rint(idct(F.reshape(8, 8)) + 128.0)
    assert px.min() >= 0 and px.max() <= 255, 'coefficients out of the pixel range'
    return px.astype(np.uint8)


def frame444(luma_blocks, cb=128, cr=128):
    """An 'i444' frame of one row of 8 x 8 luma blocks (uint8 [8, 8] each; a number: a constant block), constant chroma:
    (buf, h, w)."""
    y = np.concatenate([np.full((8, 8), b, np.uint8) if np.isscalar(b) else np.asarray(b, np.uint8) for b in luma_blocks], axis=1)
    h, w = y.shape
    buf = np.concatenate([y, np.full((h, w), cb, np.uint8), np.full((h, w), cr, np.uint8)])
    return buf, h, w


def columns(r):
    """A block of eight equal rows 128 + r[x]: F[0][u] carries everything, F[0][4] = r0 - r1 - r2 + r3 + r4 - r5 - r6 + r7 in exact
    arithmetic."""
    return np.tile(128 + np.asarray(r, np.int64), (8, 1)).astype(np.uint8)


# column patterns found by search: the model's F[0][4] is exactly +12 / -12 (F / Q = +-0.5 at quality 50, Q = 24)
HALF_POS = (-19, -5, -18, 18, -6, -1, 5, 0)
HALF_NEG = (-5, -12, 6, 11, -7, 12, 16, 11)
# column patterns with F[0][4] one rounding away from a tie: a different summation order, or one rounding per sum, moves the quantised value
ORDER_TIE = (70, -56, -94, 26, -50, -74, 98, -16)
CONTRACT_TIE = (-27, -74, -36, -3, 61, -29, -1, 9)
Q50 = jpeg.quant_tables(50)[0]


def crafted():
    """name -> (buf, h, w, fmt, quality, R)."""
    c = {}
    # constant blocks v: DC = 8 (v - 128) exactly for these v; Q = 16 at quality 50: F / Q = 1.5, -1.5, 8.5, -8.5; then the two +-0.5 ties
    # (a constant block of v - 128 = +-1 is no tie: the model's F is 8.000000000000002)
    c['ties'] = frame444([131, 125, 145, 111, columns(HALF_POS), columns(HALF_NEG)]) + ('i444', 50, 2)
    c['order_tie'] = frame444([columns(ORDER_TIE), columns(CONTRACT_TIE)]) + ('i444', 50, 1)
    c['zrl'] = frame444([from_coefficients({0: 3, 1: 2, 20: -1}, Q50), 128]) + ('i444', 50, 4)
    c['zrl_twice'] = frame444([from_coefficients({0: -2, 40: 1}, Q50), from_coefficients({50: -1}, Q50)]) + ('i444', 50, 4)
    c['last_position'] = frame444([from_coefficients({0: 1, 63: 1}, Q50), from_coefficients({5: 2, 63: -1}, Q50)]) + ('i444', 50, 4)
    c['zero_after_dc'] = frame444([200, 128, 128, 60]) + ('i444', 50, 4)
    c['dc_equal'] = frame444([90, 90, 90, 200]) + ('i444', 50, 2)
    # the largest magnitudes 8-bit samples can give at quality 100 (Q = 1): 0 / 255 in the sign pattern of the (4, 4) basis function makes
    # F[4][4] = +-(32 * 127 + 32 * 128) / 8 = +-1020, the most any AC coefficient reaches (sum |C[4][x]| is the largest row sum: 2 sqrt 2);
    # constant 0 and 255 give the DC range -1024 .. 1016.  The clamps of the model (+-1023, -1024) therefore never bind on 8-bit input:
    # they guard the coder's tables, and this frame goes as close to them as a frame can
    sign = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    board = np.where(np.outer(sign, sign) > 0, 255, 0).astype(np.uint8)
    c['clamp'] = frame444([board, 255 - board, 0, 255], cb=0, cr=255) + ('i444', 100, 1)
    # noise at quality 100, R = 1 (seed found by search): interval 0 holds a data byte 0xFF and ends in a padded 0xFF, stuffed
    c['ff_bytes'] = (np.random.default_rng(3).integers(0, 256, (24, 16), dtype=np.uint8), 8, 16, 'i444', 100, 1)
    # 18 x 34: one partial MCU column and one partial MCU row in both samplings; bright edges, so that zero padding shows
    rgb = np.clip(natural_rgb(18, 34, seed=5).astype(np.int64) + 60, 0, 255).astype(np.uint8)
    c['partial_420'] = (to_yuv(rgb, 'i420'), 18, 34, 'i420', 90, 2)
    c['partial_444'] = (to_yuv(rgb, 'i444'), 18, 34, 'i444', 90, 3)
    # >= 9 intervals: the RST index wraps
    c['rst_cycle'] = (matrix_frame(50, 66, 'i420'), 50, 66, 'i420', 75, 1)          # 4 x 5 MCUs
    return c


# wrong reading -> the crafted frame that tells it apart
CONTROLS = {'half_away': 'ties', 'contracted': 'order_tie', 'descending': 'order_tie', 'no_dc_reset': 'dc_equal', 'pad_zeros': 'zrl',
            'no_pad_stuffing': 'ff_bytes', 'swapped_chroma_tables': 'zrl', 'zero_edges': 'partial_420'}
