"""Antialiased separable bicubic resize (extension): the numpy model of refvsr_resize_aa (refvsr_amd/csrc/resize.hip), pure numpy.

The filter is the "BI" degradation of the SR literature and of the paper's pre-training stage -- Keys' cubic with a = -0.5, stretched
by the down-scale ratio (support 2 scale), weights normalised per output sample, as Pillow, MATLAB imresize and
torch.nn.functional.interpolate(mode='bicubic', antialias=True, align_corners=False) compute it.  It replaces the offline step that
made the dataset's LRx4 folders, and the consumer's resize behind the image writer.  The bicubic inside the engine (A = -0.75, four
taps, no antialias: metrics.down_bicubic_model) is another filter and stays what it is.

Everything is float64 with every operation rounded on its own (no fused multiply-add), horizontal pass first, sums in ascending tap
order starting from the first product; the kernel returns these bits.
"""
import numpy as np

A = -0.5
MAX_RATIO = 8                 # n_in / n_out per axis
MAX_TAPS = 33                 # 2 * (2 * MAX_RATIO) + 1


def cubic(x, a=A):
    """Keys' kernel at x (float64 array), the two polynomials as refvsr_resize_aa's tables are made of them."""
    x = np.abs(np.asarray(x, np.float64))
    near = ((a + 2.0) * x - (a + 3.0)) * (x * x) + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def check_sizes(n_in, n_out, what='aa_taps'):
    """ValueError (one line) unless 1 <= n_out, 1 <= n_in <= MAX_RATIO n_out."""
    if int(n_in) != n_in or int(n_out) != n_out or n_in < 1 or n_out < 1:
        raise ValueError('%s: sizes must be positive integers (got %r -> %r)' % (what, n_in, n_out))
    if n_in > MAX_RATIO * n_out:
        raise ValueError('%s: the down-scale ratio is at most %d per axis (got %d -> %d)' % (what, MAX_RATIO, n_in, n_out))


def aa_taps(n_in, n_out, a=A, antialias=True, normalise=True, half=0.5):
    """The taps of one axis: (lo int32 [n_out], cnt int32 [n_out], w float64 [n_out, max cnt]); output i is the sum over k < cnt[i] of
    w[i, k] src[lo[i] + k], w[i, k] = 0 for k >= cnt[i].  a, antialias, normalise, half: the model's own constants; other values are
    the wrong models the tests hold against it."""
    check_sizes(n_in, n_out)
    n_in, n_out = int(n_in), int(n_out)
    scale = float(n_in) / float(n_out)
    down = scale >= 1.0 and antialias
    support = 2.0 * scale if down else 2.0
    inv = 1.0 / scale if down else 1.0
    lo, cnt, rows = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), []
    for i in range(n_out):
        c = scale * (i + half)
        l_ = max(0, int(c - support + 0.5))
        h_ = min(n_in, int(c + support + 0.5))
        raw = cubic((np.arange(l_, h_, dtype=np.float64) - c + 0.5) * inv, a)
        if normalise:
            s = raw[0]
            for v in raw[1:]:                         # ascending k
                s = s + v
            raw = raw / s
        lo[i], cnt[i] = l_, h_ - l_
        rows.append(raw)
    w = np.zeros((n_out, int(cnt.max())), np.float64)
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return lo, cnt, w


_TABLE = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)      # refvsr_ingest_u8's byte -> float table (ingest_table.h)


def source_values(x):
    """float64 values of a source array: float32 / float16 widened, a byte through the ingest table (float32) and widened."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return _TABLE[x].astype(np.float64)
    if x.dtype not in (np.float32, np.float16, np.float64):
        raise ValueError('resize_aa_model: float32 | float16 | uint8 sources (got %s)' % x.dtype)
    return x.astype(np.float64)


def _pass(v, taps):
    """Σ_k w[j, k] v[..., lo[j] + k] along the last axis, the products added in ascending k starting from the first."""
    lo, cnt, w = taps
    n = v.shape[-1]
    lo = lo.astype(np.int64)
    acc = w[:, 0] * v[..., lo]
    for k in range(1, w.shape[1]):
        acc = np.where(k < cnt, acc + w[:, k] * v[..., np.minimum(lo + k, n - 1)], acc)
    return acc


def resize_aa_float64(x, oh, ow, **wrong):
    """D of the module header, float64 [.., 3, oh, ow], unclamped and unrounded."""
    v = source_values(x)
    if v.ndim < 3 or v.shape[-3] != 3:
        raise ValueError('resize_aa_model: [.., 3, H, W] frames (got %s)' % (tuple(v.shape),))
    H, W = v.shape[-2:]
    check_sizes(H, oh, 'resize_aa_model')
    check_sizes(W, ow, 'resize_aa_model')
    t = _pass(v, aa_taps(W, ow, **wrong))                                   # [.., H, ow]
    return np.ascontiguousarray(np.swapaxes(_pass(np.swapaxes(t, -1, -2), aa_taps(H, oh, **wrong)), -1, -2))


def resize_aa_model(x, oh, ow, out='float32', clamp=True, **wrong):
    """x [.., 3, H, W] float32 | float16 | uint8 -> [.., 3, oh, ow]: out = 'float32': float32(clamp(D, 0, 1)), one rounding (clamp
    False: float32(D)); out = 'uint8': round-half-even of 255 clamp(D, 0, 1) (always clamped)."""
    if out not in ('float32', 'uint8'):
        raise ValueError("resize_aa_model: out must be 'float32' or 'uint8' (got %r)" % (out,))
    d = resize_aa_float64(x, oh, ow, **wrong)
    if out == 'uint8':
        return np.rint(255.0 * np.clip(d, 0.0, 1.0)).astype(np.uint8)
    return (np.clip(d, 0.0, 1.0) if clamp else d).astype(np.float32)
