"""Cases, float64 references and checks for the kernels that are not convolutions: the warps, spynet_level_input, resize,
aligned_sample, the block gathers, dcn_sample and the EDVR pools / upsample / attention kernels (csrc/resample.hip, gather.hip, edvr.hip).

Every reference (ref_*) is a plain numpy restatement of ONE kernel, written over a number type T: with T = np.float64 it is the
reference, with T = np.float32 the same chain rounded after every operation (numpy never contracts to an FMA).  Each names the
kernel lines its rounding points come from.  Nothing of refvsr_amd or of the oracle goes into a reference.

  * EXACT cases: inputs on which the fp32 chain has no rounding at all -- every traced step of the float32 evaluation equals the
    float64 one (Case.assert_exact; checked, not assumed).  Operation order and FMA contraction then cannot matter, the store is one
    round-to-nearest-even of an exact number and the kernel must return the reference's BITS.
  * GENERAL cases: the edges exactness cannot reach, under  |got - want64| <= ulp16(want64) / 2 + delta  (fp16 stores) or
    <= delta (fp32 stores), delta = 4 x max E_ref, E_ref = |float32 evaluation - float64 evaluation| of the same reference on the
    case's own inputs (the 4 covers what the GPU may legitimately do differently from numpy: FMA contraction, tap order, its own
    cosf / sinf).  Kernels with __expf add 2^-20 |want| (EXPF_REL): the kernel evaluates exp(x) as exp2(x * log2 e); the fp32
    product x * log2 e carries a relative error of 2^-24, i.e. an absolute error of up to 8 * 1.4427 * 2^-24 = 2^-20.5 at |x| <= 8,
    which exp2 turns into a relative error of ln 2 * 2^-20.5 = 2^-21 of the exponential; the sigmoid's derivative weighs it by
    e / (1 + e) < 1, and the factor 2 left over covers the 1 ulp of v_exp_f32 and the reciprocal.
  * CONTROLS, from the reference alone: the share of outputs of an exact sampler case that changes under (a) truncation instead of
    floor, (b) the other padding mode, (c) align_corners flipped, (d) one corner tap's weight swapped with its neighbour's, (e) for
    dcn_sample the closed validity interval [0, h-1] x [0, w-1] instead of the open (-1, h) x (-1, w).  Each one that applies must
    change >= 1 % and >= 8 outputs; the populated tap classes (>= 4 outputs each) are asserted too.
    (The LITERAL closed interval [-1, h] is NOT a usable control: at py = -1 the only row in range has weight ly = 0 and at py = h
    no row is in range, so both intervals give the same outputs everywhere -- Case 'dcn' pins that as control 'e_literal' == 0.
    A bilinear footprint on a rectangle has 0, 1, 2 or 4 taps in range, never 3: class 'taps3' is asserted EMPTY.)
"""
import numpy as np

from exact_cases import CTL_B_COUNT, CTL_B_MIN

F32, F64 = np.float32, np.float64
EXPF_REL = 2.0 ** -20
E_REF_BAR = 2e-5                  # max E_ref <= E_REF_BAR * max|input|: the project's fp32-interpolation bar
CLASS_MIN = 4
RS_BICUBIC, RS_BILINEAR, RS_BILINEAR_AC, RS_NEAREST = 0, 1, 2, 3          # include/refvsr_hip.h: REFVSR_RS_*


def rng(seed):
    return np.random.RandomState(int(seed))


class Trace(object):
    """Records every intermediate of one evaluation; two traces (float32, float64) are compared step by step."""

    def __init__(self):
        self.steps = []

    def __call__(self, name, a):
        self.steps.append((name, np.asarray(a)))
        return a


def _notrace(name, a):
    return a


def f16_store(v):
    """The fp16 store of a kernel: ONE round-to-nearest-even (numpy converts float64 -> float16 directly)."""
    return np.asarray(v, dtype=F64).astype(np.float16).astype(F64)


def ulp16(v):
    """Spacing of fp16 numbers at |v| (denormals: 2^-24)."""
    a = np.abs(np.asarray(v, dtype=F64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def _sigmoid(T, x):
    """1 / (1 + __expf(-x)) (edvr.hip:29,82,200): exp overflows to inf -> 0 in float32."""
    with np.errstate(over='ignore', under='ignore'):
        return (T(1) / (T(1) + np.exp(-x.astype(T)))).astype(T)


# ---- warp (common.h:96-148, resample.hip:273-396) ---------------------------------------------------------------------------------
def _linspace(T, n):
    """rv_linspace_m1p1 (common.h:96-99): two-sided evaluation."""
    j = np.arange(n)
    step = T(2) / T(n - 1)
    return np.where(j < n // 2, T(-1) + step * j.astype(T), T(1) - step * (n - 1 - j).astype(T)).astype(T)


def _floor(a, mut):
    return np.trunc(a) if mut == 'a' else np.floor(a)


def warp_coords(T, flow, hin, win, mut=None, tr=_notrace):
    """warp_coord_uv (common.h:111-128).  Returns x0, y0 (int, clamped to [-2, n + 1]), tx, ty."""
    hf, wf = flow.shape[1:]
    u, v = flow[0].astype(T), flow[1].astype(T)
    gx = tr('gx', _linspace(T, wf)[None, :] + tr('du', u / ((T(win) - T(1)) / T(2))))
    gy = tr('gy', _linspace(T, hf)[:, None] + tr('dv', v / ((T(hin) - T(1)) / T(2))))
    if mut == 'c':                                        # align_corners=True un-normalisation
        xs = (gx + T(1)) / T(2) * T(win - 1)
        ys = (gy + T(1)) / T(2) * T(hin - 1)
    else:
        xs = tr('xs', tr('xs2', tr('xs1', tr('xs0', gx + T(1)) * T(win)) - T(1)) / T(2))
        ys = tr('ys', tr('ys2', tr('ys1', tr('ys0', gy + T(1)) * T(hin)) - T(1)) / T(2))
    fx, fy = _floor(xs, mut), _floor(ys, mut)
    tx, ty = tr('tx', xs - fx), tr('ty', ys - fy)
    x0 = np.clip(fx, -2.0, win + 1.0).astype(np.int64)
    y0 = np.clip(fy, -2.0, hin + 1.0).astype(np.int64)
    return x0, y0, tx.astype(T), ty.astype(T), xs, ys


def _blend4(T, x, x0, y0, tx, ty, mode, mut=None, tr=_notrace):
    """Four-tap blend in tap order 00, 01, 10, 11 (warp_group16, common.h:131-148; warp_planar_kernel, resample.hip:372-377).
    mode 'zeros': taps outside the map contribute nothing; 'border': indices clamped."""
    c, hin, win = x.shape
    w = [tr('w00', tr('1-ty', T(1) - ty) * tr('1-tx', T(1) - tx)), tr('w01', (T(1) - ty) * tx),
         tr('w10', ty * (T(1) - tx)), tr('w11', ty * tx)]
    if mut == 'd':
        w[0], w[1] = w[1], w[0]
    acc = np.zeros((c,) + x0.shape, dtype=T)
    nvalid = np.zeros(x0.shape, dtype=np.int64)
    xv = x.astype(T)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < hin) & (xx >= 0) & (xx < win)
        val = xv[:, np.clip(yy, 0, hin - 1), np.clip(xx, 0, win - 1)]
        term = tr('p%d' % k, w[k][None] * val)
        if mode == 'zeros':
            term = np.where(ok[None], term, T(0))
        acc = tr('s%d' % k, acc + term)
        nvalid += ok
    return acc, nvalid


def ref_warp(T, p, mut=None, tr=_notrace):
    """models/utils.py:35-43: zeros padding, linspace(-1, 1) grid, align_corners=False.  out: fp16 (nhwc16) | fp32 (planar)."""
    x, flow = p['x'], p['flow']
    if p.get('up2'):                                       # warp_nhwc16_up2 (resample.hip:321-340): flow = flow_up2(flow_lr), fp32 values
        flow = ref_flow_up2(T, flow, tr=tr).astype(T)
    x0, y0, tx, ty, _, _ = warp_coords(T, flow, x.shape[1], x.shape[2], mut, tr)
    out, _ = _blend4(T, x, x0, y0, tx, ty, 'border' if mut == 'b' else 'zeros', mut, tr)
    return {'out': out}


def warp_classes(p):
    """Tap class of every output pixel of an (exact) warp case, from the float64 chain."""
    x, flow = p['x'], p['flow']
    hin, win = x.shape[1:]
    x0, y0, tx, ty, xs, ys = warp_coords(F64, flow, hin, win)
    _, nvalid = _blend4(F64, x[:1], x0, y0, tx, ty, 'zeros')

    def axis(s, n):
        return {'in': (s >= 0) & (s <= n - 1), 'lo': (s > -1) & (s < 0), 'hi': (s > n - 1) & (s < n),
                'out_lo': (s > -2) & (s <= -1), 'out_hi': (s >= n) & (s < n + 1), 'wild': (s <= -2) | (s >= n + 1)}
    X, Y = axis(xs, win), axis(ys, hin)
    cl = {'taps4': nvalid == 4, 'taps3': nvalid == 3,
          'side_left': X['lo'] & Y['in'] & (nvalid == 2), 'side_right': X['hi'] & Y['in'] & (nvalid == 2),
          'side_top': X['in'] & Y['lo'] & (nvalid == 2), 'side_bottom': X['in'] & Y['hi'] & (nvalid == 2),
          'corner_tl': X['lo'] & Y['lo'], 'corner_tr': X['hi'] & Y['lo'], 'corner_bl': X['lo'] & Y['hi'], 'corner_br': X['hi'] & Y['hi'],
          'out_left': X['out_lo'] & (nvalid == 0), 'out_right': X['out_hi'] & (nvalid == 0),
          'out_top': Y['out_lo'] & (nvalid == 0), 'out_bottom': Y['out_hi'] & (nvalid == 0),
          'on_integer': (tx == 0) & (ty == 0) & (nvalid > 0), 'wild': (X['wild'] | Y['wild']) & (nvalid == 0)}
    for k in ('corner_tl', 'corner_tr', 'corner_bl', 'corner_br'):
        cl[k] = cl[k] & (nvalid == 1)
    return cl


# ---- resize (resample.hip:80-183, common.h:150-213) -------------------------------------------------------------------------------
def _cubic_w(T, t, tr=_notrace):
    """rv_cubic_taps (common.h:177-187), A = -0.75."""
    A = T(-0.75)

    def far(x):
        return ((A * x - T(5) * A) * x + T(8) * A) * x - T(4) * A

    def near(x):
        return ((A + T(2)) * x - (A + T(3))) * x * x + T(1)
    return [tr('cw0', far(t + T(1))), tr('cw1', near(t)), tr('cw2', near(T(1) - t)), tr('cw3', far(T(2) - t))]


def resize_taps(T, mode, n_in, n_out, scale, mut=None, tr=_notrace):
    """src_taps (resample.hip:90-113): per output index up to 4 (index, weight) pairs."""
    o = np.arange(n_out).astype(T)
    s = T(scale)
    if mode == RS_BICUBIC:
        x = tr('cx', (o + T(0.5)) * s - T(0.5)) if mut != 'c' else o * (T(n_in - 1) / T(max(n_out - 1, 1)))
        fl = _floor(x, mut)
        w = _cubic_w(T, tr('ct', x - fl), tr)
        idx = [np.clip(fl.astype(np.int64) - 1 + k, 0, n_in - 1) for k in range(4)]
    elif mode == RS_NEAREST:
        idx = [np.minimum(np.floor(tr('nx', o * s)).astype(np.int64), n_in - 1)]
        w = [np.ones(n_out, dtype=T)]
    else:
        if (mode == RS_BILINEAR_AC) != (mut == 'c'):       # rv_bilinear_ac_src (common.h:154-161)
            sc = T(n_in - 1) / T(n_out - 1) if n_out > 1 else T(0)
            x = tr('ax', o * tr('asc', sc))
        else:
            if mode == RS_BILINEAR_AC:
                s = T(n_in) / T(n_out)
            x = np.maximum(tr('bx', (o + T(0.5)) * s - T(0.5)), T(0))
        i0 = np.minimum(x.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = tr('l1', x - i0.astype(T))
        idx, w = [i0, i1], [tr('l0', T(1) - l1), l1]
    if mut == 'd':
        w[0], w[1] = w[1], w[0]
    return idx, [a.astype(T) for a in w]


def ref_resize(T, p, mut=None, tr=_notrace):
    """resize_kernel (resample.hip:118-159): row chains r = sum wx * v, acc = sum wy * r, then (acc - mean) / std, * chan_mul,
    clamp to [0, 1]; planar fp32 store or ONE fp16 rounding (nhwc16)."""
    x = p['x'].astype(T)
    c, h, w = x.shape
    oh, ow = p['out_hw']
    sc = p.get('src_scale') or (F32(h) / F32(oh), F32(w) / F32(ow))        # ops.resize passes python floats into a float argument
    iy, wy = resize_taps(T, p['mode'], h, oh, F32(sc[0]), mut, tr)
    ix, wx = resize_taps(T, p["mode"], w, ow, F32(sc[1]), mut, tr)
    acc = np.zeros((c, oh, ow), dtype=T)
    for j in range(len(iy)):
        r = np.zeros((c, oh, ow), dtype=T)
        for i in range(len(ix)):
            r = tr('r%d%d' % (j, i), r + tr('q%d%d' % (j, i), wx[i][None, None, :] * x[:, iy[j]][:, :, ix[i]]))
        acc = tr('a%d' % j, acc + tr('m%d' % j, wy[j][None, :, None] * r))
    if p.get('mean') is not None:
        acc = (acc - np.asarray(p['mean'], dtype=F32).astype(T)[:, None, None]) / np.asarray(p['std'], dtype=F32).astype(T)[:, None, None]
    if p.get('chan_mul') is not None:
        acc = tr('mul', acc * np.asarray(p['chan_mul'], dtype=F32).astype(T)[:, None, None])
    if p.get('clamp01'):
        acc = np.minimum(np.maximum(acc, T(0)), T(1))
    return {'out': acc.astype(T)}


def ref_flow_up2(T, flow, tr=_notrace):
    """F.interpolate(flow, x2, bilinear, align_corners=True) * 2 (ops.flow_up2; rv_bilinear_ac2_at, common.h:164-173)."""
    c, h, w = flow.shape
    return ref_resize(T, {'x': flow, 'out_hw': (2 * h, 2 * w), 'mode': RS_BILINEAR_AC, 'src_scale': (0.0, 0.0), 'chan_mul': [2.0] * c}, tr=tr)['out']


# ---- spynet_level_input (resample.hip:409-464) ---------------------------------------------------------------------------------------
def ref_flow_warp_border(T, x, flow, mut=None, tr=_notrace):
    """mmedit flow_warp, align_corners=True, border padding (resample.hip:443-458)."""
    c, h, w = x.shape
    u, v = flow[0].astype(T), flow[1].astype(T)
    jj, ii = np.arange(w).astype(T)[None, :], np.arange(h).astype(T)[:, None]
    gx = T(2) * (jj + u) / T(max(w - 1, 1)) - T(1)
    gy = T(2) * (ii + v) / T(max(h - 1, 1)) - T(1)
    xs = np.minimum(np.maximum((gx + T(1)) / T(2) * T(w - 1), T(0)), T(w - 1))
    ys = np.minimum(np.maximum((gy + T(1)) / T(2) * T(h - 1), T(0)), T(h - 1))
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    tx, ty = (xs - x0.astype(T)).astype(T), (ys - y0.astype(T)).astype(T)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = x.astype(T)
    out = (T(1) - ty) * ((T(1) - tx) * s[:, y0, x0] + tx * s[:, y0, x1]) + ty * ((T(1) - tx) * s[:, y1, x0] + tx * s[:, y1, x1])
    clamped = {'left': xs <= 0, 'right': xs >= w - 1, 'top': ys <= 0, 'bottom': ys >= h - 1}
    return out.astype(T), clamped


def ref_spynet_level_input(T, p, mut=None, tr=_notrace):
    """out8 = fp16 [ref | flow_warp_border(supp, flow_up) | flow_up], flow_up = flow_up2(flow_prev) or 0 (fp32 store)."""
    outs, ups = [], []
    for b in range(len(p['ref'])):
        ref, supp = p['ref'][b], p['supp'][b]
        h, w = ref.shape[1:]
        if p['flow_prev'] is not None:
            fp = p['flow_prev'][b].astype(T)
            iy, wy = resize_taps(T, RS_BILINEAR_AC, h // 2, h, 0.0)
            ix, wx = resize_taps(T, RS_BILINEAR_AC, w // 2, w, 0.0)
            g = lambda j, i: fp[:, iy[j]][:, :, ix[i]]
            up = (wy[0][None, :, None] * (wx[0] * g(0, 0) + wx[1] * g(0, 1)) + wy[1][None, :, None] * (wx[0] * g(1, 0) + wx[1] * g(1, 1))) * T(2)
        else:
            up = np.zeros((2, h, w), dtype=T)
        up = up.astype(T)
        wrp, _ = ref_flow_warp_border(T, supp, up)
        outs.append(np.concatenate([ref.astype(T), wrp, up], 0))
        ups.append(up)
    return {'out': np.stack(outs), 'flow_up': np.stack(ups)}


# ---- aligned_sample (gather.hip:80-129) ----------------------------------------------------------------------------------------------
def _reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def aligned_coords(T, affine, ks, mut=None, tr=_notrace):
    h, w = affine.shape[1:]
    H2, W2 = h * ks, w * ks
    Y, X = np.arange(H2), np.arange(W2)
    li, a = Y // ks, Y % ks
    lj, b = X // ks, X % ks
    aff = affine.astype(F32).astype(T)
    s_x, s_y = aff[0][li][:, lj], aff[1][li][:, lj]
    th = tr('th', (aff[2][li][:, lj] - T(1)) * T(F32(1.0472)))
    half = (ks - 1) // 2
    off_a = (a.astype(T) - T(half) - T(0.5))[:, None]
    off_b = (b.astype(T) - T(half) - T(0.5))[None, :]
    px, py = tr('px', off_a * s_x), tr('py', off_b * s_y)
    cs, sn = np.cos(th).astype(T), np.sin(th).astype(T)
    rx = tr('rx', tr('rx0', px * cs) + tr('rx1', py * (-sn)))
    ry = tr('ry', tr('ry0', px * sn) + tr('ry1', py * cs))
    hp1, wp1 = T(H2 + 1), T(W2 + 1)
    pr = tr('pr', tr('pr1', tr('pr0', rx + T(half)) + T(0.5)) + (1 + ks * li).astype(T)[:, None])
    pc = tr('pc', tr('pc1', tr('pc0', ry + T(half)) + T(0.5)) + (1 + ks * lj).astype(T)[None, :])
    r0, c0 = _floor(pr, mut), _floor(pc, mut)
    raw = dict(pr=pr, pc=pc, r0=r0, c0=c0)
    r1, c1 = np.clip(r0 + T(1), T(0), hp1), np.clip(c0 + T(1), T(0), wp1)
    r0, c0 = np.clip(r0, T(0), hp1), np.clip(c0, T(0), wp1)
    pr, pc = np.clip(pr, T(0), hp1), np.clip(pc, T(0), wp1)
    return dict(r0=r0, r1=r1, c0=c0, c1=c1, pr=pr, pc=pc, raw=raw, H2=H2, W2=W2)


def ref_aligned_sample(T, p, mut=None, tr=_notrace):
    """AlignedConv2d sampler: reflection pad 1, floor / ceil corners, clamped coordinates, g_lt, g_rb, g_lb, g_rt blend in that
    order (gather.hip:113-127), fp16 store."""
    x, ks = p['x'].astype(T), p['ks']
    k = aligned_coords(T, p['affine'], ks, mut, tr)
    r0, r1, c0, c1, pr, pc, H2, W2 = k['r0'], k['r1'], k['c0'], k['c1'], k['pr'], k['pc'], k['H2'], k['W2']
    ya, yb = tr('ya', T(1) + tr('dr0', r0 - pr)), tr('yb', T(1) - tr('dr1', r1 - pr))
    xa, xb = tr('xa', T(1) + tr('dc0', c0 - pc)), tr('xb', T(1) - tr('dc1', c1 - pc))
    g = {'lt': tr('g_lt', ya * xa), 'rb': tr('g_rb', yb * xb), 'lb': tr('g_lb', ya * xb), 'rt': tr('g_rt', yb * xa)}
    if mut == 'd':
        g['lt'], g['lb'] = g['lb'], g['lt']

    def src(i, n):
        i = i.astype(np.int64) - 1
        return np.clip(i, 0, n - 1) if mut == 'b' else _reflect(i, n)
    sr0, sr1, sc0, sc1 = src(r0, H2), src(r1, H2), src(c0, W2), src(c1, W2)
    out = tr('t0', g['lt'][None] * x[:, sr0, sc0])
    out = tr('t1', out + tr('u1', g['rb'][None] * x[:, sr1, sc1]))
    out = tr('t2', out + tr('u2', g['lb'][None] * x[:, sr0, sc1]))
    out = tr('t3', out + tr('u3', g['rt'][None] * x[:, sr1, sc0]))
    return {'out': out.astype(T)}


def aligned_classes(p):
    k = aligned_coords(F64, p['affine'], p['ks'])
    raw, H2, W2 = k['raw'], k['H2'], k['W2']
    return {'reflect_top': k['r0'] == 0, 'reflect_bottom': k['r1'] == H2 + 1, 'reflect_left': k['c0'] == 0, 'reflect_right': k['c1'] == W2 + 1,
            'pr_lo': raw['pr'] < 0, 'pr_hi': raw['pr'] > H2 + 1, 'pc_lo': raw['pc'] < 0, 'pc_hi': raw['pc'] > W2 + 1,
            'r1_lo': raw['r0'] + 1 < 0, 'r1_hi': raw['r0'] + 1 > H2 + 1, 'c1_lo': raw['c0'] + 1 < 0, 'c1_hi': raw['c0'] + 1 > W2 + 1,
            'interior': (raw['pr'] > 1) & (raw['pr'] < H2) & (raw['pc'] > 1) & (raw['pc'] < W2)}


# ---- block gathers (gather.hip:6-62) -----------------------------------------------------------------------------------------------
def ref_block_gather(T, p, mut=None, tr=_notrace):
    """out[c, s y + ky, s x + kx] = value[c, s ry + ky, s rx + kx], (ry, rx) = divmod(idx[y, x], wv // s): copies."""
    v, idx, s = p['value'].astype(T), p['idx'], p['s']
    gh, gw = idx.shape
    hv, wv = v.shape[1:]
    wr = wv // s
    oy, ox = np.arange(gh * s), np.arange(gw * s)
    id_ = idx[oy // s][:, ox // s]
    sy = np.minimum((id_ // wr) * s + (oy % s)[:, None], hv - 1)
    sx = np.minimum((id_ % wr) * s + (ox % s)[None, :], wv - 1)
    return {'out': v[:, sy, sx]}


# ---- dcn_sample (edvr.hip:15-51) -------------------------------------------------------------------------------------------------------
def dcn_coords(T, om, dg, tr=_notrace):
    h, w = om.shape[1:]
    omT = om.astype(F32).astype(T)
    k, g = np.arange(9), np.arange(dg)
    oy = omT[(g[None, :] * 18 + 2 * k[:, None])]              # [9, dg, h, w]
    ox = omT[(g[None, :] * 18 + 2 * k[:, None] + 1)]
    mr = omT[(2 * dg * 9 + g[None, :] * 9 + k[:, None])]
    py = tr('py', (np.arange(h)[None, None, :, None] + (k // 3 - 1)[:, None, None, None]).astype(T) + oy)
    px = tr('px', (np.arange(w)[None, None, None, :] + (k % 3 - 1)[:, None, None, None]).astype(T) + ox)
    return py, px, mr


def ref_dcn_sample(T, p, mut=None, tr=_notrace):
    """cols[k C + g 8 + j] = sigmoid(mask) * bilinear(x_g, y + ky - 1 + oy, x + kx - 1 + ox): 0 outside (-1, h) x (-1, w), corner
    pixels outside the map contribute 0; taps added in order 00, 01, 10, 11, then * m, then fp16 (edvr.hip:29-50)."""
    x, om, dg = p['x'].astype(T), p['om'], p['dg']
    c, h, w = x.shape
    py, px, mr = dcn_coords(T, om, dg, tr)
    m = _sigmoid(T, mr)
    tr('m', np.where(m < 2.0 ** -40, 0, m))                   # below 2^-40 no product with |acc| < 2^15 reaches fp16's 2^-24
    if mut == 'e':
        inside = (py >= 0) & (px >= 0) & (py <= h - 1) & (px <= w - 1)
    elif mut == 'e_literal':
        inside = (py >= -1) & (px >= -1) & (py <= h) & (px <= w)
    else:
        inside = (py > -1) & (px > -1) & (py < h) & (px < w)
    fy, fx = _floor(py, mut), _floor(px, mut)
    ly, lx = tr('ly', py - fy).astype(T), tr('lx', px - fx).astype(T)
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    wg = [tr('w0', (T(1) - ly) * (T(1) - lx)), tr('w1', (T(1) - ly) * lx), tr('w2', ly * (T(1) - lx)), tr('w3', ly * lx)]
    if mut == 'd':
        wg[0], wg[1] = wg[1], wg[0]
    xg = x.reshape(dg, 8, h, w)
    gi = np.arange(dg)[None, :, None, None]
    acc = np.zeros((9, dg, 8, h, w), dtype=T)
    for t in range(4):
        yy, xx = y0 + (t >> 1), x0 + (t & 1)
        if mut == 'b':
            ok = inside
        else:
            ok = inside & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        val = np.moveaxis(xg[gi, :, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], -1, 2)      # [9, dg, 8, h, w]
        acc = tr('s%d' % t, acc + np.where(ok[:, :, None], tr('p%d' % t, wg[t][:, :, None] * val), T(0)))
    out = acc * m[:, :, None]
    tr('out16', f16_store(out))                               # the product with a saturated mask is compared after its store
    return {'out': out.reshape(9 * c, h, w).astype(T)}


def dcn_classes(p):
    py, px, _ = dcn_coords(F64, p['om'], p['dg'])
    h, w = p['om'].shape[1:]
    iny, inx = (py >= 0) & (py <= h - 1), (px >= 0) & (px <= w - 1)
    return {'inside': iny & inx, 'band_top': (py > -1) & (py < 0) & inx, 'band_bottom': (py > h - 1) & (py < h) & inx,
            'band_left': (px > -1) & (px < 0) & iny, 'band_right': (px > w - 1) & (px < w) & iny,
            'at_-1_y': py == -1, 'at_h': py == h, 'at_-1_x': px == -1, 'at_w': px == w}


# ---- EDVR pools, upsample, attention (edvr.hip:70-211); 2 x 2 pools (resample.hip:185-223) ---------------------------------------------
def ref_pool3s2(T, p, mut=None, tr=_notrace):
    """MaxPool2d / AvgPool2d(3, 2, 1), the average counting the padding: avg = fp32(sum * fp32(1 / 9)) -- the sum of nine fp16
    numbers is exact here, the product is ONE fp32 rounding whatever T -- then fp16 (edvr.hip:123-138)."""
    x = p['x'].astype(T)
    c, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    fill = -np.inf if p['is_max'] else 0.0
    xp = np.full((c, h + 2, w + 2), fill, dtype=T)
    xp[:, 1:-1, 1:-1] = x
    acc = np.full((c, ho, wo), fill, dtype=T)
    for dy in range(3):
        for dx in range(3):
            t = xp[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2][:, :ho, :wo]
            acc = np.maximum(acc, t) if p['is_max'] else tr('s%d%d' % (dy, dx), acc + t)
    if p['is_max']:
        return {'out': acc}
    if T is F64:
        return {'out': (acc * F64(F32(1.0) / F32(9.0))).astype(F32).astype(F64)}
    return {'out': acc * (F32(1.0) / F32(9.0))}


def ref_up2_bilinear(T, p, mut=None, tr=_notrace):
    """nn.Upsample(x2, bilinear, align_corners=False) * mul: top / bottom row blends, then the column blend, * mul, fp16
    (edvr.hip:163-178)."""
    x = p['x'].astype(T)
    c, h, w = x.shape

    def taps(n):
        o = np.arange(2 * n).astype(T)
        s = o * (T(n - 1) / T(2 * n - 1)) if mut == 'c' else np.maximum((o + T(0.5)) * T(0.5) - T(0.5), T(0))
        i0 = np.minimum(s.astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), tr('l', s - i0.astype(T)).astype(T)
    y0, y1, ly = taps(h)
    x0, x1, lx = taps(w)
    wl, wr = T(1) - lx, lx
    if mut == 'd':
        wl, wr = wr, wl
    top = tr('top', tr('t0', wl * x[:, y0][:, :, x0]) + tr('t1', wr * x[:, y0][:, :, x1]))
    bot = tr('bot', tr('b0', wl * x[:, y1][:, :, x0]) + tr('b1', wr * x[:, y1][:, :, x1]))
    out = tr('o', tr('o0', (T(1) - ly)[None, :, None] * top) + tr('o1', ly[None, :, None] * bot))
    return {'out': tr('om', out * T(F32(p['mul']))).astype(T)}


def ref_tsa_weight(T, p, mut=None, tr=_notrace):
    """out[i C + c] = aligned_i[c] * sigmoid(sum_c emb_i[c] emb_ref[c]), the sum in channel order (edvr.hip:76-90), fp16."""
    outs = []
    er = p['emb_ref'].astype(T)
    for al, em in zip(p['aligned'], p['emb']):
        dot = np.zeros(er.shape[1:], dtype=T)
        prod = em.astype(T) * er
        for ch in range(er.shape[0]):
            dot = dot + prod[ch]
        outs.append(al.astype(T) * _sigmoid(T, dot)[None])
    return {'out': np.concatenate(outs, 0).astype(T)}


def ref_tsa_blend(T, p, mut=None, tr=_notrace):
    """feat * sigmoid(attn) * 2 + add, fp16 (edvr.hip:200)."""
    return {'out': (p['feat'].astype(T) * _sigmoid(T, p['attn']) * T(2) + p['add'].astype(T)).astype(T)}


def ref_pool2(T, p, mut=None, tr=_notrace):
    """avgpool2 = 0.25 * (((a + b) + c) + d), maxpool2, max2 (resample.hip:185-216): planar fp32."""
    x = p['x'].astype(T)
    if p['kind'] == 'max2':
        return {'out': np.maximum(x, p['y'].astype(T))}
    h, w = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    a, b, c, d = x[:, 0:h:2, 0:w:2], x[:, 0:h:2, 1:w:2], x[:, 1:h:2, 0:w:2], x[:, 1:h:2, 1:w:2]
    if p['kind'] == 'max':
        return {'out': np.maximum(np.maximum(a, b), np.maximum(c, d))}
    return {'out': tr('avg', T(0.25) * tr('s2', tr('s1', tr('s0', a + b) + c) + d))}


REFS = {'warp': ref_warp, 'resize': ref_resize, 'spynet': ref_spynet_level_input, 'aligned': ref_aligned_sample,
        'gather': ref_block_gather, 'dcn': ref_dcn_sample, 'pool3s2': ref_pool3s2, 'up2': ref_up2_bilinear,
        'tsa_weight': ref_tsa_weight, 'tsa_blend': ref_tsa_blend, 'pool2': ref_pool2}
CLASSES = {'warp': warp_classes, 'aligned': aligned_classes, 'dcn': dcn_classes}
EXPF_OPS = ('dcn', 'tsa_weight', 'tsa_blend')


# ---- a case ------------------------------------------------------------------------------------------------------------------------------
class Case(object):
    """op: key of REFS; p: the inputs (float64 / int numpy arrays of numbers the kernel's input type holds); fmt: store format of each
    output ('f16' | 'f32'); exact: bit-for-bit case; muts: the controls that apply; run: how test_gpu_sampling.py feeds it."""

    def __init__(self, name, op, p, fmt, exact, muts=(), run=None, untraced=None, bits_only=False):
        self.name, self.op, self.p, self.fmt, self.exact, self.muts = name, op, p, fmt, exact, tuple(muts)
        self.run = run or {}
        self.untraced = untraced          # mask of pixels whose chain is NOT exact by design (wild flows): their result must be 0
        self.bits_only = bits_only        # saturating sigmoids: exp overflows in float32 only; the stored bits are what is compared
        self._c = {}

    def ref(self, T, mut=None, tr=_notrace):
        return REFS[self.op](T, self.p, mut, tr)

    def store(self, outs):
        return {k: (f16_store(v) if self.fmt[k] == 'f16' else np.asarray(v, dtype=F64).astype(F32).astype(F64)) for k, v in outs.items()}

    @property
    def want64(self):
        if 'w64' not in self._c:
            self._c['w64'] = {k: np.asarray(v, dtype=F64) for k, v in self.ref(F64).items()}
        return self._c['w64']

    @property
    def want(self):
        """The stored values (float64 arrays holding fp16 / fp32 numbers): what an exact kernel returns, bit for bit."""
        if 'w' not in self._c:
            self._c['w'] = self.store(self.want64)
        return self._c['w']

    @property
    def got32(self):
        if 'g32' not in self._c:
            self._c['g32'] = {k: np.asarray(v, dtype=F64) for k, v in self.ref(F32).items()}
        return self._c['g32']

    # -- exact cases
    def assert_exact(self):
        """Every traced step of the float32 chain equals the float64 chain (and so does the stored result)."""
        assert self.exact
        t32, t64 = Trace(), Trace()
        o32, o64 = self.ref(F32, tr=t32), self.ref(F64, tr=t64)
        assert [n for n, _ in t32.steps] == [n for n, _ in t64.steps]
        if not self.bits_only:
            for (n, a), (_, b) in zip(t32.steps, t64.steps):
                assert a.dtype == F32 or n == 'out16', '%s: step %s of the float32 chain was computed in %s' % (self.name, n, a.dtype)
                a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
                if self.untraced is not None and a.shape[-2:] == self.untraced.shape:
                    a, b = np.where(self.untraced, 0, a), np.where(self.untraced, 0, b)
                assert np.array_equal(a, b), '%s: step %s is not exact in float32 (%d of %d differ)' % (self.name, n, int((a != b).sum()), a.size)
        s32, s64 = self.store(o32), self.store(o64)
        for k in s64:
            assert np.array_equal(s32[k], s64[k]), (self.name, k)
            assert np.isfinite(s64[k]).all()
        if self.untraced is not None:
            assert not s64['out'][:, self.untraced].any(), 'wild flows must give exactly 0'
        return len(t32.steps)

    def controls(self):
        """{mutation: (share, count)} of stored outputs that change, from the reference alone."""
        if 'ctl' not in self._c:
            w = self.want['out']
            self._c['ctl'] = {}
            for m in self.muts:
                n = int((self.store(self.ref(F64, mut=m))['out'] != w).sum())
                self._c['ctl'][m] = (n / float(w.size), n)
        return self._c['ctl']

    def classes(self):
        """{class: number of outputs (pixels x channels)} of the populated tap classes."""
        if self.op not in CLASSES or not self.exact:
            return {}
        if 'cls' not in self._c:
            out = self.want['out']
            per = {k: v for k, v in CLASSES[self.op](self.p).items()}
            self._c['cls'] = {k: int(v.sum()) * (out.size // v.size) for k, v in per.items()}
        return self._c['cls']

    def assert_strong(self):
        for m, (share, n) in self.controls().items():
            if m == 'e_literal':
                assert n == 0, 'the closed interval [-1, h] changed an output: the module docstring says it cannot'
                continue
            assert share >= CTL_B_MIN and n >= CTL_B_COUNT, '%s: control (%s) changes only %d outputs (%.2f %%)' % (self.name, m, n, 100 * share)
        for k, n in self.classes().items():
            if k == 'taps3':
                assert n == 0
            else:
                assert n >= CLASS_MIN, '%s: tap class %s has %d outputs' % (self.name, k, n)

    def tap_class(self, idx):
        """Names of the classes of output element idx = (channel, y, x) of 'out', for failure reports."""
        if self.op not in CLASSES:
            return ''
        ch, y, x = idx
        if self.op == 'dcn':                                  # channel = tap * C + group * 8 + j; the class maps are [9, dg, h, w]
            c = self.p['x'].shape[0]
            at = (ch // c, (ch % c) // 8, y, x)
        else:
            at = (y, x)
        return '+'.join(k for k, v in CLASSES[self.op](self.p).items() if v[at]) or 'none'

    # -- general cases
    def e_ref(self):
        return {k: float(np.abs(self.got32[k] - self.want64[k]).max()) for k in self.want64}

    def max_input(self):
        m = 0.0
        for v in self.p.values():
            for a in (v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(a, np.ndarray) and a.dtype.kind == 'f' and a.size:
                    m = max(m, float(np.abs(a).max()))
        return m

    def delta(self, k='out'):
        return 4.0 * self.e_ref()[k]

    def bound(self, k='out'):
        """Elementwise acceptance bracket of a general case."""
        w = self.want64[k]
        b = np.full(w.shape, self.delta(k))
        if self.op in EXPF_OPS:
            b = b + EXPF_REL * np.abs(w)
        if self.fmt[k] == 'f16':
            b = b + ulp16(w) / 2
        return b

    def line(self):
        if self.exact:
            ctl = ' '.join('(%s)=%.1f%%/%d' % (m, 100 * s, n) for m, (s, n) in self.controls().items())
            cls = self.classes()
            return 'exact controls: %s%s' % (ctl or '-', (' classes>=%d' % min(n for k, n in cls.items() if k != 'taps3')) if cls else '')
        return 'general ' + ' '.join('delta[%s]=%.3e' % (k, self.delta(k)) for k in self.want64)


def mismatch_report(case, got, k='out', limit=3):
    """(count, text): where an exact case's result differs from the reference's bits."""
    want = case.want[k]
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return 0, '0 of %d' % want.size
    txt = ['%d of %d' % (len(bad), want.size)]
    for i in bad[:limit]:
        i = tuple(int(j) for j in i)
        txt.append('%s got %r want %r [%s]' % (i, float(got[i]), float(want[i]), case.tap_class(i) if k == 'out' else ''))
    return len(bad), '; '.join(txt)


def within_report(case, got, k='out'):
    """(ok, text) of a general case: every element inside its bracket, none excluded."""
    err = np.abs(got - case.want64[k])
    b = case.bound(k)
    over = err > b
    i = np.unravel_index(int(np.argmax(err - b)), err.shape)
    used = err - (b - case.delta(k))                         # what the observed error needs of delta, beyond the half ulp / __expf terms
    return not over.any(), '%s: delta=%.3e observed=%.3e (max|got-want|=%.3e) outside=%d of %d%s' % (
        k, case.delta(k), max(float(used.max()), 0.0), float(err.max()), int(over.sum()), err.size,
        ' worst at %s: err-bound=%.3e' % (tuple(int(j) for j in i), float((err - b)[i])) if over.any() else '')


# ---- generators ------------------------------------------------------------------------------------------------------------------------
def int_map(g, c, h, w, lim=8):
    return g.randint(-lim, lim + 1, size=(c, h, w)).astype(F64)


def f16_map(g, c, h, w, scale=1.0):
    return (g.standard_normal((c, h, w)) * scale).astype(np.float16).astype(F64)


def f32_map(g, c, h, w, scale=1.0):
    return (g.standard_normal((c, h, w)) * scale).astype(F32).astype(F64)


def placed_flow(g, hf, wf, hin, win):
    """Flows (multiples of 1/4) PLACED so that every tap class is populated: each pixel gets a target sample coordinate per axis
    (inside, the partial bands, just outside, the centre pixel exactly) and the multiple of 1/4 that lands nearest to it
    (within 0.15 pixel: the band targets sit mid-band); the last pixels get wild flows (+-1e6, +-2^30).  Returns flow, wild mask."""
    def solve(target, j, nf, n):                          # xs = j n / (nf - 1) + u n / (n - 1) - 0.5
        return np.round((target + 0.5 - j * n / (nf - 1.0)) * (n - 1.0) / n * 4) / 4

    def target(kind, n):
        return {'in': g.uniform(0.3, n - 1.3), 'lo': -0.5, 'hi': n - 0.5, 'out_lo': -1.5, 'out_hi': n + 0.5, 'mid': (n - 1) / 2.0}[kind]
    pairs = [('lo', 'in'), ('hi', 'in'), ('in', 'lo'), ('in', 'hi'), ('lo', 'lo'), ('hi', 'lo'), ('lo', 'hi'), ('hi', 'hi'),
             ('out_lo', 'in'), ('out_hi', 'in'), ('in', 'out_lo'), ('in', 'out_hi'), ('mid', 'mid'), ('in', 'in')]
    flow = np.zeros((2, hf, wf))
    wild = np.zeros((hf, wf), dtype=bool)
    order = g.permutation(hf * wf)
    wilds = [(1e6, 0), (-1e6, 0), (0, 2.0 ** 30), (0, -2.0 ** 30), (2.0 ** 30, -1e6), (-2.0 ** 30, 1e6), (0.25, 1e6), (-1e6, -0.25)]
    for n, pix in enumerate(order):
        y, x = divmod(int(pix), wf)
        if n < len(wilds):
            flow[:, y, x] = wilds[n]
            wild[y, x] = True
            continue
        kx, ky = pairs[n % len(pairs)] if n < 5 * len(pairs) or g.uniform() < 0.3 else ('in', 'in')
        flow[0, y, x] = solve(target(kx, win), x, wf, win)
        flow[1, y, x] = solve(target(ky, hin), y, hf, hin)
    return flow, wild


def placed_affine(g, h, w, ks):
    """Scales (multiples of 1/4 in [-6, 6]), rotation channel 1: border cells alternate between 6 (the coordinate leaves the padded
    map: pr / pc and r1 / c1 clamp at both ends) and the value that lands in the reflected ring with a fractional weight."""
    frac, mid = (2.5, 4.0) if ks == 2 else (1.5, 2.0)       # mid: the coordinate lands in (-1, 0), where floor and truncation part
    a = np.ones((3, h, w))
    a[:2] = g.randint(-24, 25, size=(2, h, w)) / 4.0
    for edges in ((a[0, 0, :], a[0, -1, :]), (a[1, :, 0], a[1, :, -1])):
        for edge in edges:
            edge[0::3], edge[1::3], edge[2::3] = 6.0, frac, mid
    return a


def placed_dcn(g, h, w, dg):
    """Offsets (multiples of 1/4) and mask logits in {0, +100, -100}: random inside offsets, and for a share of the samples the
    coordinate is put into the partial bands, exactly on -1 and exactly on h / w."""
    om = np.zeros((27 * dg, h, w))
    om[:18 * dg] = g.randint(-12, 13, size=(18 * dg, h, w)) / 4.0
    om[18 * dg:] = g.choice([0.0, 0.0, 100.0, -100.0], size=(9 * dg, h, w))
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for gi in range(dg):
        for k in range(9):
            sel = g.uniform(size=(h, w))
            base_y, base_x = ys + k // 3 - 1, xs + k % 3 - 1
            for lo, tgt_y, tgt_x in ((0.00, -1.0, None), (0.04, h, None), (0.08, None, -1.0), (0.12, None, w), (0.16, -0.25, None),
                                     (0.20, h - 0.75, None), (0.24, None, -0.5), (0.28, None, w - 0.25)):
                m = (sel >= lo) & (sel < lo + 0.04)
                if tgt_y is not None:
                    om[gi * 18 + 2 * k][m] = (tgt_y - base_y + 0 * xs)[m]
                    om[gi * 18 + 2 * k + 1][m] = (g.randint(0, 4 * (w - 1) + 1, size=(h, w)) / 4.0 - base_x)[m]
                else:
                    om[gi * 18 + 2 * k + 1][m] = (tgt_x - base_x + 0 * ys)[m]
                    om[gi * 18 + 2 * k][m] = (g.randint(0, 4 * (h - 1) + 1, size=(h, w)) / 4.0 - base_y)[m]
    return om


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
WARP_GEOS = [(5, 9, 5, 9), (9, 17, 9, 17), (17, 33, 17, 33), (9, 17, 5, 9), (17, 33, 9, 17)]
F16, F32S = {'out': 'f16'}, {'out': 'f32'}


def warp_exact(name, seed, geo, c, planar):
    def make():
        g = rng(seed)
        hf, wf, hin, win = geo
        flow, wild = placed_flow(g, hf, wf, hin, win)
        return Case(name, 'warp', {'x': int_map(g, c, hin, win), 'flow': flow}, F32S if planar else F16, True, 'abcd',
                    {'entry': 'warp_planar' if planar else 'warp_nhwc16'}, untraced=wild)
    return make


def warp_general(name, seed, geo, c, entry):
    def make():
        g = rng(seed)
        hf, wf, hin, win = geo
        x = f32_map(g, c, hin, win) if entry == 'warp_planar' else f16_map(g, c, hin, win)
        if entry == 'warp_nhwc16_up2':
            p = {'x': x, 'flow': f32_map(g, 2, hf // 2, wf // 2, 2.0), 'up2': True}
        else:
            p = {'x': x, 'flow': f32_map(g, 2, hf, wf, 3.0)}
        return Case(name, 'warp', p, F32S if entry == 'warp_planar' else F16, False, run={'entry': entry})
    return make


def _resize_exact(name, seed, mode, hw, out_hw, scale, variant, lim=8, muts=''):
    def make():
        g = rng(seed)
        p = {'x': int_map(g, 3, hw[0], hw[1], lim), 'out_hw': out_hw, 'mode': mode, 'src_scale': scale}
        if variant == 'clamp':
            p.update(chan_mul=[0.125, 0.25, 0.5], clamp01=True)
        return Case(name, 'resize', p, F16 if variant == 'nhwc16' else F32S, True, muts if variant == 'planar' else '', {'nhwc16': variant == 'nhwc16'})
    return make


def _resize_general(name, seed, mode, hw, out_hw, scale=None, c=3, **kw):
    def make():
        g = rng(seed)
        p = dict(x=f32_map(g, c, hw[0], hw[1]), out_hw=out_hw, mode=mode, src_scale=scale, **kw)
        nh = p.pop('nhwc16', False)
        return Case(name, 'resize', p, F16 if nh else F32S, False, run={'nhwc16': nh})
    return make


def _aligned(name, seed, hw, ks, cs, exact):
    def make():
        g = rng(seed)
        h, w = hw
        if exact:
            p = {'x': int_map(g, cs, h * ks, w * ks), 'affine': placed_affine(g, h, w, ks), 'ks': ks}
        else:
            p = {'x': f16_map(g, cs, h * ks, w * ks), 'affine': (g.uniform(-3, 3, size=(3, h, w))).astype(F32).astype(F64), 'ks': ks}
        return Case(name, 'aligned', p, F16, exact, 'abd' if exact else '')
    return make


def _dcn(name, seed, hw, dg, exact):
    def make():
        g = rng(seed)
        h, w = hw
        if exact:
            p = {'x': int_map(g, 8 * dg, h, w), 'om': placed_dcn(g, h, w, dg), 'dg': dg}
        else:
            om = f32_map(g, 27 * dg, h, w, 2.5)
            om[18 * dg:] = np.clip(om[18 * dg:], -8, 8)
            p = {'x': f16_map(g, 8 * dg, h, w), 'om': om, 'dg': dg}
        return Case(name, 'dcn', p, F16, exact, ('a', 'd', 'e', 'e_literal') if exact else ())
    return make


def _gather(name, seed, s, kind):
    def make():
        g = rng(seed)
        gh, gw, hr, wr = 5, 7, 6, 9                        # index grid, patch grid of the value map
        idx = g.randint(0, hr * wr, size=(gh, gw))
        idx.flat[:4] = [0, hr * wr - 1, wr - 1, wr]         # the first, the last, the last of a row and the first of the next
        if kind == 'nhwc16':
            v = f16_map(g, 24, hr * s, wr * s)
        else:
            v = f32_map(g, 3, hr * s, wr * s)
        return Case(name, 'gather', {'value': v, 'idx': idx, 's': s}, F16 if kind != 'planar' else F32S, True, run={'kind': kind})
    return make


def _pool3(name, seed, hw, is_max, exact):
    def make():
        g = rng(seed)
        x = int_map(g, 16, hw[0], hw[1]) if exact else f16_map(g, 16, hw[0], hw[1])
        return Case(name, 'pool3s2', {'x': x, 'is_max': is_max}, F16, exact)
    return make


def _up2(name, seed, hw, mul, exact):
    def make():
        g = rng(seed)
        x = int_map(g, 16, hw[0], hw[1]) if exact else f16_map(g, 16, hw[0], hw[1])
        return Case(name, 'up2', {'x': x, 'mul': mul}, F16, exact, 'cd' if exact else '')
    return make


def _pool2(name, seed, kind, exact):
    def make():
        g = rng(seed)
        mk = int_map if exact else f32_map
        p = {'x': mk(g, 5, 7, 11), 'kind': kind}
        if kind == 'max2':
            p['y'] = mk(g, 5, 7, 11)
        return Case(name, 'pool2', p, F32S, exact)
    return make


def _spynet(name, seed, hw, batch, with_prev, big):
    def make():
        g = rng(seed)
        h, w = hw
        p = {'ref': [f32_map(g, 3, h, w) for _ in range(batch)], 'supp': [f32_map(g, 3, h, w) for _ in range(batch)],
             'flow_prev': [f32_map(g, 2, h // 2, w // 2, big) for _ in range(batch)] if with_prev else None}
        return Case(name, 'spynet', p, {'out': 'f16', 'flow_up': 'f32'}, False)
    return make


def _tsa_weight(name, seed, t, sat):
    def make():
        g = rng(seed)
        c, h, w = 64, 5, 7
        if sat:                                              # dot in {0, +128, -128}: sigmoid exactly 0.5, 1, 0 in float32
            er = np.zeros((c, h, w))
            er[0] = 4.0
            emb = []
            for _ in range(t):
                e = np.zeros((c, h, w))
                e[0] = g.choice([0.0, 32.0, -32.0], size=(h, w))
                emb.append(e)
            al = [int_map(g, c, h, w) for _ in range(t)]
        else:                                                # logits bounded by |x| <= 8
            er = f16_map(g, c, h, w, 0.5)
            emb = [f16_map(g, c, h, w, 0.5) for _ in range(t)]
            for e in emb:
                d = np.abs((e * er).sum(0)).max()
                if d > 8:
                    e *= 0.5 ** np.ceil(np.log2(d / 8))
            al = [f16_map(g, c, h, w) for _ in range(t)]
        return Case(name, 'tsa_weight', {'aligned': al, 'emb': emb, 'emb_ref': er}, F16, sat, bits_only=sat)
    return make


def _tsa_blend(name, seed, sat):
    def make():
        g = rng(seed)
        c, h, w = 64, 5, 7
        if sat:
            p = {'feat': int_map(g, c, h, w), 'attn': g.choice([0.0, 100.0, -100.0], size=(c, h, w)), 'add': int_map(g, c, h, w)}
        else:
            p = {'feat': f16_map(g, c, h, w), 'attn': np.clip(f16_map(g, c, h, w, 3.0), -8, 8), 'add': f16_map(g, c, h, w)}
        return Case(name, 'tsa_blend', p, F16, sat, bits_only=sat)
    return make


def _table():
    t, seed = {}, [1000]

    def add(name, maker, *a):
        seed[0] += 1
        assert name not in t
        t[name] = maker(name, seed[0], *a)
    # warps: every geometry at cs = 8 and 24, cs = 64 at wf = 33 (33 x 8 lanes cross one 256-thread block); planar c = 1, 3, 5
    for geo in WARP_GEOS:
        for cs in (8, 24) + ((64,) if geo[1] == 33 else ()):
            add('warp_nhwc16 x %dx%d<-%dx%d cs%d' % (geo + (cs,)), warp_exact, geo, cs, False)
    for geo, c in ((WARP_GEOS[2], 1), (WARP_GEOS[1], 3), (WARP_GEOS[0], 5), (WARP_GEOS[3], 3), (WARP_GEOS[4], 1)):
        add('warp_planar x %dx%d<-%dx%d c%d' % (geo + (c,)), warp_exact, geo, c, True)
    for geo in ((7, 13, 7, 13), (19, 45, 19, 45), (14, 26, 7, 13)):
        add('warp_nhwc16 g %dx%d<-%dx%d cs24' % geo, warp_general, geo, 24, 'warp_nhwc16')
        add('warp_planar g %dx%d<-%dx%d c3' % geo, warp_general, geo, 3, 'warp_planar')
    for geo in ((14, 26, 14, 26), (38, 90, 38, 90), (14, 26, 7, 13)):
        add('warp_nhwc16_up2 g %dx%d<-%dx%d cs24' % geo, warp_general, geo, 24, 'warp_nhwc16_up2')
    # resize
    # (x4: cubic weights on the 2^-11 grid, 2-D products on 2^-22 -- the map is kept to [-2, 2] so that the sums stay below 2^24 of them;
    # controls that do not apply: x0.5 samples at 2 o + 0.5 >= 0, where truncation IS floor, with both bilinear weights 0.5)
    for label, mode, hw, out_hw, scale, lim, muts in (
            ('bicubic x2', RS_BICUBIC, (5, 9), (10, 18), (0.5, 0.5), 8, 'acd'), ('bicubic x4', RS_BICUBIC, (5, 9), (20, 36), (0.25, 0.25), 2, 'acd'),
            ('bicubic x0.5', RS_BICUBIC, (10, 18), (5, 9), (2.0, 2.0), 8, 'cd'), ('bilinear x2', RS_BILINEAR, (5, 9), (10, 18), (0.5, 0.5), 8, 'cd'),
            ('bilinear x0.5', RS_BILINEAR, (10, 18), (5, 9), (2.0, 2.0), 8, 'c'), ('bilinear_ac 5->9', RS_BILINEAR_AC, (5, 5), (9, 9), (0.0, 0.0), 8, 'cd'),
            ('bilinear_ac 9->17', RS_BILINEAR_AC, (9, 9), (17, 17), (0.0, 0.0), 8, 'cd'), ('nearest x0.5', RS_NEAREST, (10, 18), (5, 9), (2.0, 2.0), 8, ''),
            ('nearest x2', RS_NEAREST, (5, 9), (10, 18), (0.5, 0.5), 8, '')):
        for variant in ('planar', 'nhwc16', 'clamp'):
            add('resize x %s %s' % (label, variant), _resize_exact, mode, hw, out_hw, scale, variant, lim, muts)
    add('resize g bilinear 18x26->32x32', _resize_general, RS_BILINEAR, (18, 26), (32, 32))
    add('resize g bilinear 32x32->18x26', _resize_general, RS_BILINEAR, (32, 32), (18, 26))
    add('resize g bicubic 7x13->10x19', _resize_general, RS_BICUBIC, (7, 13), (10, 19))
    add('resize g bicubic 7x13->10x19 nhwc16', lambda n, s: _resize_general(n, s, RS_BICUBIC, (7, 13), (10, 19), nhwc16=True))
    add('resize g bilinear_ac x2 (flow_up2)', lambda n, s: _resize_general(n, s, RS_BILINEAR_AC, (9, 15), (18, 30), (0.0, 0.0), c=2, chan_mul=[2.0, 2.0]))
    add('resize g bilinear mean/std', lambda n, s: _resize_general(n, s, RS_BILINEAR, (13, 19), (16, 32), mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]))
    add('resize g bicubic mean/std clamp', lambda n, s: _resize_general(n, s, RS_BICUBIC, (13, 19), (26, 38), (0.5, 0.5), mean=[0.485, 0.456, 0.406],
                                                                           std=[0.229, 0.224, 0.225], clamp01=True))
    add('resize g nearest 7x13->10x19', _resize_general, RS_NEAREST, (7, 13), (10, 19))
    # aligned_sample
    for ks in (2, 4):
        for hw in ((3, 5), (7, 9)):
            for cs in (8, 24):
                add('aligned_sample x ks%d %dx%d cs%d' % ((ks,) + hw + (cs,)), _aligned, hw, ks, cs, True)
        add('aligned_sample g rotation ks%d 7x9 cs16' % ks, _aligned, (7, 9), ks, 16, False)
    # dcn_sample
    for dg in (1, 8):
        for hw in ((5, 7), (9, 17)):
            add('dcn_sample x dg%d %dx%d' % ((dg,) + hw), _dcn, hw, dg, True)
    add('dcn_sample g dg8 9x13', _dcn, (9, 13), 8, False)
    # block gathers
    for s in (1, 2, 4):
        for kind in ('nhwc16', 'rgb16', 'planar'):
            add('block_gather x %s s%d' % (kind, s), _gather, s, kind)
    # pools, upsample
    for hw in ((5, 7), (6, 8)):
        for is_max in (1, 0):
            add('pool3s2 x %s %dx%d' % (('max' if is_max else 'avg',) + hw), _pool3, hw, is_max, True)
        for mul in (1.0, 2.0):
            add('up2_bilinear x mul%g %dx%d' % ((mul,) + hw), _up2, hw, mul, True)
    add('pool3s2 g avg 9x13', _pool3, (9, 13), 0, False)
    add('up2_bilinear g mul2 9x13', _up2, (9, 13), 2.0, False)
    for kind in ('avg', 'max', 'max2'):
        add('pool2 x %s' % kind, _pool2, kind, True)
    add('pool2 g avg', _pool2, 'avg', False)
    # spynet_level_input
    for hw in ((6, 10), (18, 30)):
        add('spynet_level_input g %dx%d flow_prev' % hw, _spynet, hw, 1, True, 6.0)
        add('spynet_level_input g %dx%d no flow' % hw, _spynet, hw, 1, False, 0.0)
    add('spynet_level_input g 18x30 batch8', _spynet, (18, 30), 8, True, 6.0)
    # attention
    for tt in (1, 5, 8):
        add('tsa_weight g t%d' % tt, _tsa_weight, tt, False)
    add('tsa_weight x saturated t5', _tsa_weight, 5, True)
    add('tsa_blend g random', _tsa_blend, False)
    add('tsa_blend x saturated', _tsa_blend, True)
    return t


TABLE = _table()
NAMES = list(TABLE)
EXACT = [n for n in NAMES if n.split(' ')[1] == 'x']                     # '<entry> x ...' exact, '<entry> g ...' general
GENERAL = [n for n in NAMES if n not in EXACT]
_CACHE = {}


def get_case(name):
    if name not in _CACHE:
        _CACHE[name] = TABLE[name]()
        assert _CACHE[name].exact == (name in EXACT)
    return _CACHE[name]
