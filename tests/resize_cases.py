"""Shared cases of the antialiased resize (tests/test_resize.py on the CPU, tests/test_gpu_resize.py on the device): the shapes, the
seeded sources and the wrong models the numpy model is held against.  numpy only."""
import numpy as np

# (H, W, oh, ow): ratio 4 | non-integer ratios, odd sizes | ratio ~3 / ~1.7 | ratio 4, one full tile wide | just below 1 | ratio 2 |
# up-scale by 2 | one output sample (every tap clipped at both borders) | ratio 8, the 33-tap limit (32 taps inside the frame)
SHAPES = ((16, 24, 4, 6), (22, 38, 7, 9), (37, 53, 12, 31), (64, 96, 16, 24), (30, 42, 29, 41), (18, 26, 9, 13), (9, 13, 18, 26),
          (8, 8, 1, 1), (64, 40, 8, 5))
# several 16 x 64 output tiles, partial ones on both axes (the device test adds it)
TILED = (135, 241, 34, 61)
DTYPES = ('float32', 'float16', 'uint8')

_SOURCES = {}


def step_edges(h, w, oh, ow):
    """A frame [3, h, w] of 0 / 1 blocks about three output samples wide, the three channels shifted against each other: every edge
    rings below 0 and above 1 before the clamp."""
    by, bx = max(2, 3 * -(-h // oh)), max(2, 3 * -(-w // ow))
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    return np.stack([(((y + c) // by + (x + 2 * c) // bx) % 2).astype(np.float64) for c in range(3)])


def sources(shape, dtype, n=1):
    """n seeded frames [n, 3, h, w] of `dtype` for a shape: frame 0 is step_edges, the others uniform noise over the full range; built
    once per key and left unchanged."""
    key = (shape, dtype, n)
    if key not in _SOURCES:
        h, w, oh, ow = shape
        x = np.random.RandomState(1000 * h + 10 * w + oh + n).rand(n, 3, h, w)
        x[0] = step_edges(h, w, oh, ow)
        x = np.rint(255.0 * x).astype(np.uint8) if dtype == 'uint8' else x.astype(dtype)
        x.setflags(write=False)
        _SOURCES[key] = x
    return _SOURCES[key]


# the wrong models: keyword arguments of resize.aa_taps (through resize_aa_model) that are NOT the specification
WRONG_TAPS = {'a = -0.75': dict(a=-0.75), 'no antialias': dict(antialias=False), 'unnormalised': dict(normalise=False),
              'centre without the half': dict(half=0.0)}
