"""Host side of the device scorer (refvsr_score_frames, csrc/score.hip): the PSNR of a device-computed mse, and a numpy float64 model of
the kernel -- its tile decomposition, its direct 7-term window sums and its fixed reduction order -- that the CPU suite can run against
evalrun.psnr / evalrun.ssim (trainers/trainer.py:252-254, evaluation/metrics.py:17-18)."""
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
