"""Crafted frames and wrong-model controls for the Y'CbCr 4:2:0 conversion (refvsr_amd/yuv.py is the model, csrc/yuv.hip the kernel).
Shared by tests/test_yuv.py (the model against published codes, ties, controls) and tests/test_gpu_yuv.py (the kernel against the
model on the same frames).  Pure numpy.

A case is a [3, h, w] array (uint8, float32 or float16).  A control is the model with one deliberate mistake; control_cases() names,
for every control, the (case, format, matrix, range) whose output the mistake changes -- a control that changes nothing would
show that the cases cannot see that mistake."""
import numpy as np

from refvsr_amd import yuv

COLOURS = {'red': (255, 0, 0), 'green': (0, 255, 0), 'blue': (0, 0, 255), 'white': (255, 255, 255), 'black': (0, 0, 0),
           'yellow': (255, 255, 0), 'cyan': (0, 255, 255), 'magenta': (255, 0, 255)}

# uint8 2 x 2 blocks (row-major) of ONE channel, the other two zero, whose four chroma values sum to an exact half code at full range:
# 8 bits: sc m = sum(u) / 8, a tie when sum(u) % 8 == 4;  10 bits: sc m = 1023 sum(u) / 2040, a tie when sum(u) % 340 == 0
TIE_BLOCKS_8 = (('b', (31, 202, 244, 151)), ('b', (197, 94, 0, 113)), ('b', (254, 79, 175, 192)), ('r', (242, 41, 199, 50)), ('r', (175, 155, 11, 71)))
TIE_BLOCKS_10 = (('b', (163, 83, 76, 18)), ('b', (102, 84, 71, 83)), ('r', (216, 74, 33, 17)), ('r', (54, 44, 46, 196)))


def _blocks(blocks):
    a = np.zeros((3, 2, 2 * len(blocks)), np.uint8)
    for j, (ch, u) in enumerate(blocks):
        a['rgb'.index(ch), :, 2 * j:2 * j + 2] = np.array(u, np.uint8).reshape(2, 2)
    return a


def solid(rgb, h=2, w=2, dtype=np.uint8):
    a = np.empty((3, h, w), dtype)
    for c in range(3):
        a[c] = rgb[c]
    return a


def cases():
    """name -> [3, h, w] frame."""
    out = {}
    out['primaries'] = np.concatenate([solid(COLOURS[k]) for k in ('red', 'green', 'blue', 'white', 'black', 'yellow', 'cyan', 'magenta')], axis=2)
    ramp = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(8, 32), 2, axis=0), 2, axis=1)      # 2 x 2 blocks of one grey
    out['grey_ramp'] = np.stack([ramp, ramp, ramp])
    out['grey_all'] = np.stack([np.arange(256, dtype=np.uint8).reshape(8, 32)] * 3)                      # every byte, four per block
    out['blue'] = solid(COLOURS['blue'])
    g = np.random.RandomState(7)
    out['detail_u8'] = g.randint(0, 256, (3, 6, 10)).astype(np.uint8)                                   # every pixel of a block differs
    out['detail_f32'] = g.rand(3, 6, 10).astype(np.float32)
    # saturated colours next to each other: block averages that differ from any single site by tens of codes
    dot = np.zeros((3, 2, 2), np.uint8)
    dot[0, 0, 0] = dot[2, 0, 0] = 255                                                                    # one magenta pixel, top left
    out['edges'] = np.concatenate([solid(COLOURS['red'], 2, 1), solid(COLOURS['blue'], 2, 1), solid(COLOURS['green'], 2, 1), solid(COLOURS['white'], 2, 1),
                                   dot], axis=2)
    # ties of the luma: greys whose products are exact (powers of two, and BT.709's (kr + kg) + kb == 1.0 in float64)
    for dt, name in ((np.float32, 'f32'), (np.float16, 'f16')):
        out['tie_y_' + name] = np.concatenate([solid((0.5,) * 3, dtype=dt), solid((0.125,) * 3, dtype=dt)], axis=2)
    out['tie_c8'] = _blocks(TIE_BLOCKS_8)
    out['tie_c10'] = _blocks(TIE_BLOCKS_10)
    return out


# (case, format, matrix, range, plane index 0 = Y | 1 = Cb | 2 = Cr): the pre-rounding value of at least one sample is exactly k + 0.5
TIES = (('tie_y_f32', 'nv12', 'bt709', 'limited', 0), ('tie_y_f16', 'i420', 'bt709', 'full', 0),
        ('tie_y_f32', 'p010', 'bt709', 'limited', 0), ('tie_y_f16', 'i420p10', 'bt709', 'full', 0),
        ('tie_c8', 'nv12', 'bt709', 'full', 1), ('tie_c8', 'i420', 'bt709', 'full', 2),
        ('tie_c10', 'p010', 'bt709', 'full', 1), ('tie_c10', 'i420p10', 'bt709', 'full', 2))


def tie_mask(frame, fmt, matrix, range, plane):
    v = yuv.pre_rounding(frame, yuv.coefficients(fmt, matrix, range))[plane]
    return v == np.floor(v) + 0.5


# ------------------------------------------------------------------------------------------------ wrong models
def control_model(control, rgb, fmt, matrix, range):
    """yuv.rgb_to_yuv420 with one mistake."""
    d = yuv.depth_of(fmt)
    if control == 'swap_range':
        range = 'full' if range == 'limited' else 'limited'
    if control == 'swap_matrix':
        matrix = 'bt601' if matrix == 'bt709' else 'bt709'
    kr, kg, kb, icb, icr, oy, sy, oc, sc = yuv.coefficients(fmt, matrix, range)
    rgb = np.asarray(rgb)
    if control == 'recip255' and rgb.dtype == np.uint8:
        v = (rgb.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float64)
    else:
        v = yuv.source_f64(rgb)
    r, g, b = v
    ey = (kr * r + kg * g) + kb * b
    hi = float(2 ** d - 1)
    rnd = np.trunc if control == 'trunc' else np.rint
    if control == 'no_clamp':
        q = lambda x: rnd(x).astype(np.int64) & (2 ** (8 if d == 8 else 16) - 1)        # the cast's wrap-around
    else:
        q = lambda x: np.clip(rnd(x), 0.0, hi).astype(np.int64)
    planes = [q(oy + sy * ey)]
    for e in ((b - ey) * icb, (r - ey) * icr):
        e00, e01, e10, e11 = e[0::2, 0::2], e[0::2, 1::2], e[1::2, 0::2], e[1::2, 1::2]
        if control == 'left_sited':
            planes.append(q(oc + sc * ((e00 + e10) * 0.5)))
        elif control == 'top_left':
            planes.append(q(oc + sc * e00))
        elif control == 'avg_after_quant':
            c = [q(oc + sc * x).astype(np.float64) for x in (e00, e01, e10, e11)]
            planes.append(q(((c[0] + c[1]) + (c[2] + c[3])) * 0.25))
        else:
            planes.append(q(oc + sc * (((e00 + e01) + (e10 + e11)) * 0.25)))
    if control == 'swap_cbcr':
        planes[1], planes[2] = planes[2], planes[1]
    return yuv.pack(planes[0], planes[1], planes[2], fmt)


# control -> (case, format, matrix, range) built to see it
CONTROLS = {
    'swap_cbcr': ('primaries', 'nv12', 'bt709', 'limited'),
    'left_sited': ('edges', 'i420', 'bt709', 'limited'),
    'top_left': ('detail_u8', 'nv12', 'bt709', 'limited'),
    'trunc': ('tie_y_f32', 'nv12', 'bt709', 'limited'),
    'no_clamp': ('blue', 'i420', 'bt709', 'full'),
    'swap_range': ('primaries', 'p010', 'bt709', 'limited'),
    'swap_matrix': ('primaries', 'i420p10', 'bt601', 'limited'),
    'recip255': ('tie_c8', 'nv12', 'bt709', 'full'),
    'avg_after_quant': ('detail_f32', 'p010', 'bt709', 'limited'),
}
