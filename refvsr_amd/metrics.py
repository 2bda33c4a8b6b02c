"""Host side of the device scorer (refvsr_score_frames, csrc/score.hip): the PSNR of a device-computed mse, and a numpy float64 model of
the kernel -- its tile decomposition, its direct 7-term window sums and its fixed reduction order -- that the CPU suite can run against
evalrun.psnr / evalrun.ssim (trainers/trainer.py:252-254, evaluation/metrics.py:17-18).

The field-of-view evaluation (evaluation/eval_quan_FOV.py:155-192 on evaluation/metrics.py:18-30) lives here too: the seven rectangles
its 16 masked scores are made of (fov_rects), the table those scores form from rectangle sums (fov_table), a numpy model of
refvsr_score_regions (score_regions_model) and the whole-array float64 host path (fov_scores_host).

The confidence-map evaluation (evaluation/eval_quan_conf_map.py:64-100,148-165) has its numpy model here as well: conf_colormap_model,
the steps of refvsr_conf_colormap (csrc/colormap.hip) one by one."""
import math

import numpy as np

TILE = (32, 64)          # window origins per workgroup (SC_TH, SC_TW of csrc/score.hip)
THREADS = 256            # threads per workgroup: lane = column, wave = 8 output rows
C1, C2 = 0.01 * 0.01, 0.03 * 0.03
NORM = 49.0 / 48.0


def psnr_from_mse(mse):
    """10 log10(1 / mse) in float64; inf for mse == 0 (what evalrun.psnr returns for identical frames)."""
    mse = float(mse)
    return float('inf') if mse == 0.0 else 10.0 * math.log10(1.0 / mse)


def _tree(v):
    """The kernels' LDS tree over one float64 per thread: red[t] += red[t + s] for s = 128, 64, .. 1."""
    v = np.array(v, dtype=np.float64)
    s = v.size // 2
    while s > 0:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    return v[0]


def _strided_sum(v):
    """Thread t of 256 sums elements t, t + 256, .. in order; then the tree."""
    v = np.asarray(v, dtype=np.float64)
    n = -(-v.size // THREADS) * THREADS
    pad = np.zeros(n, dtype=np.float64)
    pad[:v.size] = v
    acc = np.zeros(THREADS, dtype=np.float64)
    for row in pad.reshape(-1, THREADS):
        acc = acc + row
    return _tree(acc)


def _seq7(x, axis):
    """Direct 7-term sums along `axis`, first term to last (left to right / top to bottom)."""
    n = x.shape[axis] - 6
    sl = lambda k: np.take(x, np.arange(k, k + n), axis=axis)
    acc = sl(0)
    for k in range(1, 7):
        acc = acc + sl(k)
    return acc


def score_frames_model(a, b, tile=TILE, win=7):
    """(mse, ssim) of one pair a, b [3,h,w] (numpy or torch; float32 values, as the kernel sees them after widening fp16 / looking
    bytes up) exactly as csrc/score.hip computes them: per (channel, tile) workgroup the owned samples' (a - b)^2 summed per staging
    thread, the windows' SSIM from direct 7-term sums summed per (column, 8-row group) thread, the 256-thread tree, and the frame's
    partial sums in the finishing kernel's order.  win = 0: ssim = 0.0."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[0] == 3
    _, h, w = a.shape
    th, tw = tile
    assert h >= 7 and w >= 7 and win in (0, 7) and th % 4 == 0 and tw * 4 == THREADS
    ih, iw, rows = th + 6, tw + 6, th // 4
    nty, ntx = -(-(h - 6) // th), -(-(w - 6) // tw)
    part_m, part_s = [], []
    ne = -(-ih * iw // THREADS) * THREADS
    for c in range(3):
        for ty in range(nty):
            for tx in range(ntx):
                y0, x0 = ty * th, tx * tw
                ta, tb = np.zeros((ih, iw)), np.zeros((ih, iw))
                hh, ww = min(ih, h - y0), min(iw, w - x0)
                ta[:hh, :ww] = a[c, y0:y0 + hh, x0:x0 + ww]
                tb[:hh, :ww] = b[c, y0:y0 + hh, x0:x0 + ww]
                own_h = h - y0 if ty == nty - 1 else th
                own_w = w - x0 if tx == ntx - 1 else tw
                d = ta - tb
                d2 = np.where((np.arange(ih)[:, None] < own_h) & (np.arange(iw)[None, :] < own_w), d * d, 0.0).reshape(-1)
                d2 = np.concatenate([d2, np.zeros(ne - d2.size)])
                acc = np.zeros(THREADS)
                for row in d2.reshape(-1, THREADS):          # element e = t, t + 256, ..: staging thread t's running sum
                    acc = acc + row
                part_m.append(_tree(acc))
                ss = np.zeros(THREADS)
                if win:
                    t = [_seq7(_seq7(x, 1), 0) for x in (ta, tb, ta * ta, tb * tb, ta * tb)]        # [th, tw] each
                    ua, ub = t[0] / 49.0, t[1] / 49.0
                    va, vb, vab = NORM * (t[2] / 49.0 - ua * ua), NORM * (t[3] / 49.0 - ub * ub), NORM * (t[4] / 49.0 - ua * ub)
                    s = ((2.0 * ua * ub + C1) * (2.0 * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2))
                    ok = ((y0 + np.arange(th))[:, None] <= h - 7) & ((x0 + np.arange(tw))[None, :] <= w - 7)
                    s = np.where(ok, s, 0.0).reshape(4, rows, tw)                                  # [wave, row of the wave, lane]
                    acc = np.zeros((4, tw))
                    for o in range(rows):
                        acc = acc + s[:, o]
                    ss = acc.reshape(-1)                                                           # thread = 64 wave + lane
                part_s.append(_tree(ss))
    mse = _strided_sum(part_m) / (3.0 * h * w)
    ssim = _strided_sum(part_s) / (3.0 * (h - 6) * (w - 6)) if win else 0.0
    return float(mse), float(ssim)


# ------------------------------------------------------------------------------------------------ down-scaled scoring (flag_HD_in)
DOWN_W = (-3.0 / 32.0, 19.0 / 32.0, 19.0 / 32.0, -3.0 / 32.0)      # Keys' cubic, A = -0.75, at the fraction 1 / 2: exact in binary


def _down_taps(n, s):
    """[4][n] source indices of the n output positions along an axis of s n samples: i0 = s x + s / 2 - 2, clamped into the axis."""
    i0 = s * np.arange(n) + s // 2 - 2
    return [np.clip(i0 + k, 0, s * n - 1) for k in range(4)]


def _down_axis(x, s, axis, weights, taps):
    """One pass of the down-scale along `axis`: the four weighted taps added first to last."""
    t = taps(x.shape[axis] // s, s)
    sl = lambda k: np.float64(weights[k]) * np.take(x, t[k], axis=axis)
    acc = sl(0) + sl(1)
    acc = acc + sl(2)
    return acc + sl(3)


def down_bicubic_model(a, s, weights=DOWN_W, taps=_down_taps):
    """float32 [3, h, w]: the bicubic down-scale by s = 2 | 4 of a float32 [3, s h, s w] frame (numpy or torch), the image both
    reference definitions score at an exact integer factor --
      models/loss/Loss.py:91-92   F.interpolate(sr, scale_factor=1 / scale, mode='bicubic', align_corners=False) (.clamp(0, 1), PSNR :141)
      evaluation/eval_qual_quan.py:85-92   cv2.resize(output, fx=1 / scale, fy=1 / scale, INTER_CUBIC) (not clamped, SSIM)
    -- as refvsr_score_frames_down computes it (csrc/score.hip): float64 on the float32 value of every sample; horizontal pass
    W0 a[i0] + W1 a[i0 + 1] + W2 a[i0 + 2] + W3 a[i0 + 3] added left to right, i0 = s x + s / 2 - 2, indices clamped to [0, n - 1];
    vertical pass the same over the four row sums, top to bottom; rounded once to float32.
    (weights, taps: the definition's two ingredients, which the tests replace by wrong ones to show that their bars can tell.)"""
    a = _as64(a)
    assert s in (2, 4) and a.ndim == 3 and a.shape[0] == 3 and a.shape[1] % s == 0 and a.shape[2] % s == 0
    return _down_axis(_down_axis(a, s, 2, weights, taps), s, 1, weights, taps).astype(np.float32)


def score_frames_down_model(a, g, s, win=7):
    """(mse, ssim) of one result a [3, s h, s w] against the ground truth g [3, h, w] as refvsr_score_frames_down computes them: with
    D = down_bicubic_model(a, s), the mse of score_frames_model on clip(D, 0, 1) (Loss.py:92,141 clamps before the PSNR) and its ssim
    on the unclamped D (eval_qual_quan.py:85-92 does not clamp)."""
    d = down_bicubic_model(a, s)
    mse, _ = score_frames_model(np.clip(d, np.float32(0), np.float32(1)), g, win=0)
    _, ssim = score_frames_model(d, g, win=win) if win else (0.0, 0.0)
    return mse, ssim


# ------------------------------------------------------------------------------------------------ field-of-view evaluation
FOV_KEYS = (1, 0.9, 0.8, 0.7, 0.6, 0.5)        # eval_quan_FOV.py:26
MAX_RECTS = 8                                   # REFVSR_SCORE_MAX_RECTS


def fov_crop_ratio(key):
    """eval_quan_FOV.py:167, evaluated as the reference evaluates it (Python floats): 20, 10, 6, 5, 4 for 0.9 .. 0.5."""
    return int(1 / ((1 - key) / 2))


def fov_rects(h, w):
    """The seven rectangles (y0, y1, x0, x1), half-open, that every mask of eval_quan_FOV.py:155-192 is one of or a difference of
    two of: the whole frame, the valid crop of the plain SSIM, and R(key) = [h // cr : h - h // cr, w // cr : w - w // cr] for
    key = 0.9 .. 0.5.  Below 20 rows or columns h // 20 == 0: R(0.9) is the whole frame and the reference divides by an empty mask."""
    h, w = int(h), int(w)
    if h < 20 or w < 20:
        raise ValueError('fov_rects: the FOV masks need frames of at least 20 x 20 (got %d x %d)' % (h, w))
    rects = [(0, h, 0, w), (3, h - 3, 3, w - 3)]
    for key in FOV_KEYS[1:]:
        cr = fov_crop_ratio(key)
        rects.append((h // cr, h - h // cr, w // cr, w - w // cr))
    return rects


def _area3(r):
    return 3.0 * (r[1] - r[0]) * (r[3] - r[2])


def fov_table(sums, h, w):
    """float64 [6 keys][fi, fo, fr][psnr, ssim] of one frame from sums [7][2] = {sum (a - b)^2, sum S} over fov_rects(h, w)
    (refvsr_score_regions / score_regions_model / host_region_sums): fi = R(key), fo = frame - R(key), fr = R(key) - R(0.5); key 1:
    fi = the plain psnr / ssim (whole-frame mse, S over the valid crop), fo = 0, fr = frame - R(0.5); key 0.5: fr = 0 -- exact 0.0
    where the reference reports 0, inf PSNR where a region's error is zero."""
    sums = np.asarray(sums, dtype=np.float64)
    rects = fov_rects(h, w)
    assert sums.shape == (len(rects), 2)
    cnt = [_area3(r) for r in rects]
    mean = lambda se, ss, n: (psnr_from_mse(se / n), ss / n)
    full, inner = 0, len(rects) - 1
    table = np.zeros((len(FOV_KEYS), 3, 2), dtype=np.float64)
    for k in range(len(FOV_KEYS)):
        r = k + 1                                               # R(key)'s rectangle (key 1: the valid crop)
        if k == 0:
            table[k, 0] = (psnr_from_mse(sums[full, 0] / cnt[full]), sums[r, 1] / cnt[r])
            r = full
        else:
            table[k, 0] = mean(sums[r, 0], sums[r, 1], cnt[r])
            table[k, 1] = mean(sums[full, 0] - sums[r, 0], sums[full, 1] - sums[r, 1], cnt[full] - cnt[r])
        if r != inner:
            table[k, 2] = mean(sums[r, 0] - sums[inner, 0], sums[r, 1] - sums[inner, 1], cnt[r] - cnt[inner])
    return table


def _as64(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _ssim_map(ta, tb):
    """S at the (rows - 6) x (cols - 6) centres of ta, tb: direct 7-term sums left to right, then top to bottom."""
    t = [_seq7(_seq7(x, -1), -2) for x in (ta, tb, ta * ta, tb * tb, ta * tb)]
    ua, ub = t[0] / 49.0, t[1] / 49.0
    va, vb, vab = NORM * (t[2] / 49.0 - ua * ua), NORM * (t[3] / 49.0 - ub * ub), NORM * (t[4] / 49.0 - ua * ub)
    return ((2.0 * ua * ub + C1) * (2.0 * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2))


def _reflect(i, n):
    """scipy.ndimage 'reflect' = numpy 'symmetric' (d c b a | a b c d | d c b a), then clamped (rg_reflect of csrc/score.hip)."""
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    return np.maximum(i, 0)


def score_regions_model(a, b, rects, tile=TILE):
    """sums [R][2] = {sum (a - b)^2, sum S} over rects (y0, y1, x0, x1) of one pair a, b [3,h,w] exactly as refvsr_score_regions
    computes them: per (channel, tile of 32 x 64 pixel centres) workgroup the 38 x 70 input tile staged through the symmetric-reflect
    index, S and the centre's (a - b)^2 per (column, 8-row group) thread added top to bottom to the rectangles that hold the centre, a
    64-lane tree per wave, ((w0 + w1) + w2) + w3, and in the finishing kernel partial sum i in slice i mod 64, a slice in order, the
    slices in order.  (A rectangle that misses a tile is skipped by the kernel; its partial sum is the 0.0 computed here.)"""
    a, b = _as64(a), _as64(b)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[0] == 3
    _, h, w = a.shape
    th, tw = tile
    rects = [tuple(int(v) for v in r) for r in rects]
    assert h >= 7 and w >= 7 and 1 <= len(rects) <= MAX_RECTS and th % 4 == 0 and tw * 4 == THREADS
    for y0, y1, x0, x1 in rects:
        assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w
    rows = th // 4
    nty, ntx = -(-h // th), -(-w // tw)
    part = []                                                   # [3 nty ntx][R][2]
    for c in range(3):
        for ty in range(nty):
            for tx in range(ntx):
                cy, cx = ty * th, tx * tw
                iy, ix = _reflect(cy - 3 + np.arange(th + 6), h), _reflect(cx - 3 + np.arange(tw + 6), w)
                ta, tb = a[c][iy][:, ix], b[c][iy][:, ix]
                s = _ssim_map(ta, tb)                           # [th, tw]
                d = ta[3:-3, 3:-3] - tb[3:-3, 3:-3]
                d2 = d * d
                oy, ox = (cy + np.arange(th))[:, None], (cx + np.arange(tw))[None, :]
                out = np.zeros((len(rects), 2))
                for r, (y0, y1, x0, x1) in enumerate(rects):
                    inside = (oy >= y0) & (oy < y1) & (ox >= x0) & (ox < x1)
                    for k, v in enumerate((d2, s)):
                        v = np.where(inside, v, 0.0).reshape(4, rows, tw)       # [wave, row of the wave, lane]
                        acc = np.zeros((4, tw))
                        for o in range(rows):
                            acc = acc + v[:, o]
                        wv = [_tree(acc[g]) for g in range(4)]
                        out[r, k] = ((wv[0] + wv[1]) + wv[2]) + wv[3]
                part.append(out)
    part = np.array(part)
    sl = np.zeros((64,) + part.shape[1:])
    for i in range(part.shape[0]):
        sl[i % 64] = sl[i % 64] + part[i]
    total = sl[0]
    for g in range(1, 64):
        total = total + sl[g]
    return total


def host_region_sums(a, b, rects):
    """sums [R][2] over rects from whole-array float64 numpy: (a - b)^2 and the full SSIM map (symmetric padding by 3, direct 7-term
    sums), each rectangle a plain slice sum."""
    a, b = _as64(a), _as64(b)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[0] == 3 and a.shape[1] >= 7 and a.shape[2] >= 7
    d2 = (a - b) ** 2
    pad = lambda x: np.pad(x, ((0, 0), (3, 3), (3, 3)), mode='symmetric')
    s = _ssim_map(pad(a), pad(b))
    return np.array([[d2[:, y0:y1, x0:x1].sum(), s[:, y0:y1, x0:x1].sum()] for y0, y1, x0, x1 in rects], dtype=np.float64)


def fov_scores_host(a, b):
    """The FOV table [6][3][2] of one pair a, b [3,h,w] on the host in float64 (`--eval_mode quan_FOV --metrics host`)."""
    h, w = a.shape[-2:]
    return fov_table(host_region_sums(a, b, fov_rects(h, w)), h, w)


# ------------------------------------------------------------------------------------------------ confidence maps as images
def conf_colormap_model(x):
    """uint8 [h, w, 3] (RGB): one confidence map [.., h, w] (numpy or torch, numel == h * w, finite) min/max-normalised and coloured
    with matplotlib's inferno exactly as csrc/colormap.hip computes it, all float32: lo = min x, a = x - lo, span = max a, y = a / span
    (the IEEE quotient), idx = min((int)(y * 256), 255), out = T[idx] with T the library's table (refvsr_colormap_table; no matplotlib
    here).  A constant map (span = 0, y = NaN) is matplotlib's "bad" colour: zero bytes.  Bit for bit what
    evaluation/eval_quan_conf_map.py:79-84,126,150 writes (x - x.min(), / x.max(), colormap(x)[:, :, :3], torch.Tensor, * 255, the
    rounding cast of cv2.imwrite)."""
    from . import ops
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, dtype=np.float32)
    h, w = x.shape[-2:]
    assert x.size == h * w, 'conf_colormap_model: one [.., h, w] map'
    x = x.reshape(h, w)
    table = np.array(ops.colormap_table(), dtype=np.uint8)
    lo = x.min()
    a = x - lo
    span = a.max()
    with np.errstate(invalid='ignore', divide='ignore'):
        y = a / span
    assert y.dtype == np.float32
    bad = np.isnan(y)
    idx = np.minimum(np.where(bad, np.float32(0), y * np.float32(256)).astype(np.int64), 255)
    out = table[idx]
    out[bad] = 0
    return out
