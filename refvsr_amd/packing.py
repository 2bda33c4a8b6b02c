"""Host-side packing of conv weights into the MFMA fragment order consumed by
refvsr_conv_mfma (refvsr_amd/csrc/conv_mfma.hip).

GEMM view: D[row][pixel] = sum_k Wk[row][k] * X[k][pixel].
  k-block = (tap, cg) (tap = ky*ks + kx, cg = 16-byte channel group of the concatenated, padded
  input: 8 halfs, or 4 floats in f32 mode), placed at slot kslot(ky, kx, cg) -- even-parity blocks
  ((kx + cg) & 1 == 0) first, then the odd ones, so that the two K-blocks one ds_read_b128 lane group
  mixes never collide on LDS banks (csrc/common.h:rv_kslot); K-step s covers slots 4s..4s+3; lane l of a
  wave supplies slot 4s + (l>>4) for row (l&15) of a 16-row tile.
  fp16 : packed[z][s][m][hi|lo][lane][8] = split(Wk[(z*MT+m)*16 + (lane&15)][(4s + (lane>>4))*8 : +8])
         with hi = fp16(w), lo = fp16(w - hi)  (two MFMAs per fragment, ~22-bit weights)
  f32  : packed[z][s][m][lane][4]        = Wk[...][(4s + (lane>>4))*4 : +4]
Rows are the conv output channels, except for pixel-shuffle convs where row r = sub*C + c holds
conv channel c*4 + sub so that a lane's 4 consecutive rows are 4 consecutive channels of ONE
output pixel (mmedit upsample.py:49-50 pixel_shuffle fused into the store).

The specialised 3x3 kernels (csrc/conv24.hip, resblock24.hip, resblock48.hip) read blobs instead: one fragment filler (_fill_frags)
over the K order c24_kblock and a table of row layouts (_ROW_LAYOUTS) builds the fragments of every one of them; blob_plan says which
blob a conv carries.
"""
import collections

import numpy as np
import torch

from . import hip


def _np(x):
    """fp32 numpy array of a tensor (any device, any dtype) or of anything numpy takes."""
    return x.detach().cpu().float().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)


def _pad8(c):
    return (c + 7) // 8 * 8


def _padg(c, g):
    return (c + g - 1) // g * g


def choose_mt(cout):
    n_mt = (cout + 15) // 16
    if n_mt <= 3:
        return n_mt
    if n_mt % 3 == 0:
        return 3
    if n_mt % 2 == 0:
        return 2
    return 3


def keven(ks, ncg):
    """Number of even-parity K-blocks (csrc/common.h:rv_keven)."""
    ce, co = (ncg + 1) >> 1, ncg >> 1
    return ks * (((ks + 1) >> 1) * ce + (ks >> 1) * co)


def ksteps(ks, ncg):
    return (ks * ks * ncg + (keven(ks, ncg) & 1) + 3) // 4


def kslot(ty, tx, cg, ks, ncg):
    """Slot of K-block (ty, tx, cg) in the packed K order (csrc/common.h:rv_kslot, same closed form)."""
    ce, co = (ncg + 1) >> 1, ncg >> 1
    p = (tx + cg) & 1
    c0, c1 = (co, ce) if p else (ce, co)
    row = ((ks + 1) >> 1) * c0 + (ks >> 1) * c1
    rank = ty * row + ((tx + 1) >> 1) * c0 + (tx >> 1) * c1 + (cg >> 1)
    if not p:
        return rank
    E = keven(ks, ncg)
    return E + (E & 1) + rank


def kmatrix(w, src_channels, shuffle=False, grp=8):
    """Wk [rows, G*grp] (fp32 numpy) + row->conv-channel map.  src_channels: real channel count of each
    concatenated HWC source (each is padded to a multiple of grp channels in its own buffer)."""
    w = np.asarray(w, np.float32)
    cout, cin, ks, _ = w.shape
    assert sum(src_channels) == cin, (src_channels, cin)
    pads = [_padg(c, grp) for c in src_channels]
    ncg = sum(pads) // grp
    # padded-channel index -> original input channel (or -1)
    cmap = []
    base = 0
    for c, p in zip(src_channels, pads):
        cmap += [base + i if i < c else -1 for i in range(p)]
        base += c
    cmap = np.asarray(cmap)
    rows = np.arange(cout)
    if shuffle:
        C = cout // 4
        rows = (np.arange(cout) % C) * 4 + np.arange(cout) // C      # row r -> conv channel
    G = ks * ks * ncg
    Wk = np.zeros((cout, G * grp), np.float32)
    valid = cmap >= 0
    for tap in range(ks * ks):
        ky, kx = divmod(tap, ks)
        blk = np.zeros((cout, ncg * grp), np.float32)
        blk[:, valid] = w[rows][:, cmap[valid], ky, kx]
        Wk[:, tap * ncg * grp:(tap + 1) * ncg * grp] = blk
    return Wk, rows, ncg


def pack_conv(w, b, src_channels, shuffle=False, mt=None, f32=False, hi_only=False):
    """Returns dict(wpack, bias fp32 [nz*MT*16], cout, ksteps, mt, ksize, cpads, shuffle, f32, hi_only).
    wpack: fp16 [nz,S,MT,2,64,8] (hi, lo), fp16 [nz,S,MT,1,64,8] (hi_only: plain fp16 weights, descriptor mode 2: the streamed
    kernels only -- SPyNet's 7x7 convs) or fp32 [nz,S,MT,64,4]."""
    w, b = _np(w), _np(b)
    cout, cin, ks, _ = w.shape
    grp = 4 if f32 else 8
    assert not (f32 and shuffle)
    Wk, rows, ncg = kmatrix(w, src_channels, shuffle, grp)
    S = ksteps(ks, ncg)
    MT = mt or choose_mt(cout)
    n_mt = (cout + 15) // 16
    nz = (n_mt + MT - 1) // MT
    R = nz * MT * 16
    full = np.zeros((R, S * 4 * grp), np.float32)
    for tap in range(ks * ks):
        for cg in range(ncg):
            g, j = tap * ncg + cg, kslot(tap // ks, tap % ks, cg, ks, ncg)
            full[:cout, j * grp:(j + 1) * grp] = Wk[:, g * grp:(g + 1) * grp]
    # [nz, MT, lr, S, q, grp] -> [nz, S, MT, q, lr, grp]
    frag = full.reshape(nz, MT, 16, S, 4, grp).transpose(0, 3, 1, 4, 2, 5).reshape(nz, S, MT, 64, grp)
    frag = torch.from_numpy(np.ascontiguousarray(frag))
    assert not (f32 and hi_only)
    if f32:
        wpack = frag
    elif hi_only:
        assert S > 16 and MT <= 2 and not shuffle, 'hi_only weights are for the streamed convs (more than 16 K-steps, MT <= 2)'
        wpack = frag.to(torch.float16).unsqueeze(3).contiguous()           # [nz,S,MT,1,64,8]
    else:
        hi = frag.to(torch.float16)
        lo = (frag - hi.float()).to(torch.float16)
        wpack = torch.stack([hi, lo], 3).contiguous()           # [nz,S,MT,2,64,8]
    bias = np.zeros(R, np.float32)
    bias[:cout] = b[rows]
    return dict(wpack=wpack, bias=torch.from_numpy(bias), cout=cout, ksteps=S, mt=MT, ksize=ks,
                cpads=[_padg(c, grp) for c in src_channels], shuffle=shuffle, f32=f32, hi_only=hi_only,
                raw=(torch.from_numpy(w.copy()), torch.from_numpy(b.copy())),       # fp32 originals: repacking for specialised kernels
                src_channels=list(src_channels))


# ---- blobs of the specialised 3x3 kernels (csrc/conv24.hip, resblock24.hip, resblock48.hip) ---------------------------------------
def rb24_kblock(s, q):
    """K-block (K-step s, quarter q = lane >> 4) of the fused 24-channel block's K order -> (ty, tx, cg) of the 3x3 x 24-channel
    window, or None for the zero block: the three-group table of c24_kblock (csrc/resblock24.hip:refvsr_resblock24_kblock makes the
    same reduction; tests/test_host.py pins them together)."""
    return c24_kblock(3, s, q)


def pack_resblock(c, wfmt, w1, b1, w2, b2):
    """One fused c-channel block (c = 24 | 48) -> uint8 blob: the fragment parts of the two convs' pack_conv24 blobs back to back,
    then their two bias tails (32 | 64 floats each):  [conv1 fragments][conv2 fragments][b1][b2]."""
    tail = 4 * _nbias(c)
    blobs = []
    for w, b in ((w1, b1), (w2, b2)):
        assert tuple(w.shape) == (c, c, 3, 3), tuple(w.shape)
        blobs.append(pack_conv24(w, b, [c], wfmt=wfmt))
    return torch.cat([x[:-tail] for x in blobs] + [x[-tail:] for x in blobs])


def pack_resblock24(w1, b1, w2, b2):
    """uint8 [43264] for refvsr_resblock24_chain: fragments fp16 [7 K-steps][3][64 lanes][8] per conv (row layout 'hi_lo24')."""
    return pack_resblock(24, 'hi_lo', w1, b1, w2, b2)


def pack_resblock24_f16w(w1, b1, w2, b2):
    """uint8 [28928] for refvsr_resblock24_chain_f16w (config.weight_precision = 'fp16'): [7 K-steps][2 fragments] per conv (row
    layout 'fp16').  No lo halves: the kernel computes with fp16(W), bit for bit what refvsr_resblock24_chain computes on
    pack_resblock24(fp16(W))."""
    return pack_resblock(24, 'fp16', w1, b1, w2, b2)


def c24_steps(ncg):
    return {1: 3, 2: 5, 3: 7, 4: 9, 6: 14, 7: 18, 12: 27}[ncg]


def c24_kblock(ncg, s, q):
    """K-block (K-step s, quarter q) of the conv24 blob for ncg 16-byte channel groups of the concatenated (padded) sources
    -> (ty, tx, cg) or None for a zero block; csrc/conv24.hip:c24_kblock is the same table (tests/test_host.py pins them).
    A K-step takes four slots u = tx * (ncg | 1) + cg of the staged window whose LDS offsets are (immediate) + (one of <= 4
    per-lane patterns), the blocks of quarters (0, 1) and of (2, 3) having slot offsets of equal parity."""
    perm = (0, 2, 1, 3)
    if ncg == 1:
        return None if q == 3 else (s, perm[q], 0)
    if ncg == 3:
        if s < 6:
            u = 4 * (s & 1) + perm[q]
            return s >> 1, u // 3, u % 3
        return None if q == 3 else (q, 2, 2)
    if ncg == 4:
        return s // 3, s % 3, perm[q]
    if ncg == 2:
        if s < 3:
            u = (0, 4, 1, 3)[q]
            return s, u // 3, u % 3
        if s == 3:
            return q & 1, 2, q >> 1
        return None if q & 1 else (2, 2, q >> 1)
    if ncg == 7:                                    # two steps per tap: cg = {0, 2, 1, 3}, then {4, 6, 5, zero block}
        if s & 1:
            return None if q == 3 else (s // 6, (s // 2) % 3, 4 + perm[q])
        return s // 6, (s // 2) % 3, perm[q]
    if ncg == 12:                                   # three steps per tap: cg = 4 j + {0, 2, 1, 3}
        return s // 9, (s // 3) % 3, 4 * (s % 3) + perm[q]
    if ncg == 6:
        if s < 9:
            return s // 3, s % 3, perm[q]
        if s < 12:
            return s - 9, (0, 1, 0, 1)[q], (4, 5, 5, 4)[q]
        if s == 12:
            return q & 1, 2, 4 + (q >> 1)
        return None if q & 1 else (2, 2, 4 + (q >> 1))
    raise ValueError(ncg)


# Row layouts of a fragment set: cout -> [(f, r, half, c, n)]: rows c .. c + n of hi (half 0: fp16(w)) or lo (half 1: fp16(w - hi)) go
# to rows r .. r + n of fragment f; rows nobody names stay zero.  NF = 1 + the largest f.
_ROW_LAYOUTS = {
    # 24 outputs, hi + lo (NF = 3): f = 0: hi(W[r])   f = 1: lo(W[r])   f = 2: hi(W[16 + r]) if r < 8 else lo(W[8 + r])
    'hi_lo24': lambda cout: [(0, 0, 0, 0, 16), (1, 0, 1, 0, 16), (2, 0, 0, 16, 8), (2, 8, 1, 16, 8)],
    # 16 m outputs, hi + lo (NF = cout / 8): f = 2 m: hi(W[16 m + r])   f = 2 m + 1: lo(W[16 m + r])
    'hi_lo16': lambda cout: [(2 * m + half, 0, half, 16 * m, 16) for m in range(cout // 16) for half in (0, 1)],
    # plain fp16 (NF = ceil(cout / 16)): f = m: fp16(W[16 m + r]), rows past the output channels zero
    'fp16': lambda cout: [(m, 0, 0, 16 * m, min(16, cout - 16 * m)) for m in range((cout + 15) // 16)],
    # the 3-row output head (NF = 1): rows 0-2 = hi(W[r]), rows 8-10 = lo(W[r - 8]) (the kernel folds rows r and r + 8)
    'head': lambda cout: [(0, 0, 0, 0, 3), (0, 8, 1, 0, 3)],
}


def _fill_frags(Wk, ncg, layout):
    """Wk [cout, 9 * ncg * 8] (kmatrix: K-block g = tap * ncg + cg) -> fp16 [S][NF][4][16][8]: lane l = (q = l >> 4, r = l & 15) of
    K-step s holds the 8 (padded) input channels of K-block c24_kblock(ncg, s, q) for row r of fragment f of the row layout."""
    halves = [Wk.astype(np.float16)]
    halves.append((Wk - halves[0].astype(np.float32)).astype(np.float16))
    rows = _ROW_LAYOUTS[layout](Wk.shape[0])
    S = c24_steps(ncg)
    frag = np.zeros((S, 1 + max(f for f, _, _, _, _ in rows), 4, 16, 8), np.float16)
    for s_ in range(S):
        for q in range(4):
            kb = c24_kblock(ncg, s_, q)
            if kb is None:
                continue
            ty, tx, cg = kb
            g = (ty * 3 + tx) * ncg + cg
            for f, r, half, c, n in rows:
                frag[s_, f, q, r:r + n] = halves[half][c:c + n, g * 8:g * 8 + 8]
    return frag


def _blob(frag, b, nb):
    """uint8 blob of one conv: the fragments, then nb bias floats (b, zero-padded)."""
    bb = np.zeros(nb, np.float32)
    bb[:len(b)] = b
    return torch.from_numpy(np.concatenate([frag.reshape(-1).view(np.uint8), bb.view(np.uint8)]))


def _nbias(cout):
    return 64 if cout == 48 else 32


def pack_conv_hr_last(w_hr, b_hr, w_last, b_last):
    """uint8 [43264] blob for refvsr_conv_hr_last (mid_channels = 24): the resblock24 block layout with conv1 = conv_hr (24 -> 24)
    and conv2 = the output head conv_last (24 -> 3): pack_conv_last's one fragment per K-step in slot (s, 0), slots (s, 1) and (s, 2)
    zero; b1 = conv_hr's bias, b2 = [b_last, 0, ...]."""
    assert tuple(w_hr.shape) == (24, 24, 3, 3) and tuple(w_last.shape) == (3, 24, 3, 3), (tuple(w_hr.shape), tuple(w_last.shape))
    hr, last = pack_conv24(w_hr, b_hr, [24]), pack_conv_last(w_last, b_last)
    conv2 = torch.zeros((RB24_S, RB24_NF, 1024), dtype=torch.uint8)
    conv2[:, 0] = last[:-128].view(RB24_S, 1024)
    return torch.cat([hr[:-128], conv2.view(-1), hr[-128:], last[-128:]])


def pack_conv_last(w, b):
    """uint8 blob of the output head for refvsr_conv_last: 3x3, C -> 3 (C = 24 | 48).  [S K-steps][ONE fragment: 64 lanes x 8 halfs]
    in the row layout 'head' + 32 bias floats."""
    w, b = _np(w), _np(b)
    assert w.shape[0] == 3 and w.shape[1] in (24, 48) and tuple(w.shape[2:]) == (3, 3), w.shape
    Wk, _, ncg = kmatrix(w, [w.shape[1]])
    return _blob(_fill_frags(Wk, ncg, 'head'), b, 32)


# blob sizes of the fused blocks (csrc/resblock24.hip, resblock48.hip), from their K-steps, fragments per K-step and bias floats
RB24_S, RB24_NF, RB24_NF_F16W = c24_steps(3), 3, 2          # the 24-channel block: hi + lo | fp16 weight format
RB24_WB = RB24_S * RB24_NF * 1024                           # fragment bytes of one 24 -> 24 conv
RB24_BLOB = 2 * (RB24_WB + 128)
RB24_F16W_BLOB = 2 * (RB24_S * RB24_NF_F16W * 1024 + 128)
RB48_WB = c24_steps(6) * 6 * 1024                           # fragment bytes of one 48 -> 48 conv
RB48_BLOB = 2 * (RB48_WB + 256)
assert (RB24_BLOB, RB24_F16W_BLOB, RB48_BLOB) == (hip.RESBLOCK24_BLOB_BYTES, hip.RESBLOCK24_F16W_BLOB_BYTES, hip.RESBLOCK48_BLOB_BYTES)


def pack_resblock48(w1, b1, w2, b2):
    """uint8 [172544] for refvsr_resblock48_chain: [14 K-steps][6 fragments = hi | lo of output channels 0-15, 16-31, 32-47] per
    conv (row layout 'hi_lo16'), b1 and b2 as 64 floats each (48.. = 0)."""
    return pack_resblock(48, 'hi_lo', w1, b1, w2, b2)


def conv24_ok(w_shape, src_channels, shuffle=False, f32=False, shuffle_group=False, half_group=False):
    """Shapes served by the specialised kernels (csrc/conv24.hip): 3x3, 24 / 32 / 48 output channels, the listed inputs --
    the same lists as the library's refvsr_conv{24,32,48}_supported (pinned against each other in tests/test_capi.py).
    shuffle_group=True (internal, pack_conv_shuffle2 only): the 24 -> 48 row groups of the pixel-shuffle conv, which
    refvsr_conv48 itself does NOT serve (a plain 24 -> 48 conv goes to the generic kernel)."""
    cout, cin, ks, _ = w_shape
    pads = [_pad8(c) for c in src_channels]
    if ks != 3 or shuffle or f32:
        return False
    if cout == 24:
        return pads in ([24], [16], [8, 24], [24, 24]) or (half_group and pads == [48, 48])
    if cout == 32:
        return pads in ([32], [8])              # AlignedConv2d: the 32 -> 32 convs and the RGB stem
    if cout == 48:
        return pads in ([48], [16], [48, 48], [8, 48]) or (shuffle_group and pads == [24])
    return False


def conv_shuffle2_ok(w_shape, src_channels, f32=False):
    """C -> 4 C 3x3 pixel-shuffle convs served by refvsr_conv_shuffle2 (csrc/conv24.hip): C = 24 | 48."""
    cout, cin, ks, _ = w_shape
    return ks == 3 and not f32 and list(src_channels) in ([24], [48]) and cin == src_channels[0] and cout == 4 * cin


# The four A/B knobs of blob_plan as plain booleans (True: that family of specialised kernels is switched off)
BlobFlags = collections.namedtuple('BlobFlags', 'no_conv24 no_conv32 no_conv48x2 no_conv_shuffle2')
BlobFlags.__new__.__defaults__ = (False,) * 4


def blob_plan(w_shape, src_channels, shuffle=False, f32=False, hi_only=False, wfmt='hi_lo', flags=BlobFlags()):
    """(kind, blob_wfmt) of the specialised blob a conv carries next to its generic packing.  kind: None | 'conv24' (pack_conv24:
    refvsr_conv24 / 32 / 48) | 'shuffle2' (pack_conv_shuffle2).  wfmt: the engine's weight format ('fp16': the packer was handed
    fp16-representable weights); blob_wfmt: the format of the blob -- 'fp16' where the shape has a refvsr_*_f16w twin (24 | 32
    outputs, the C = 24 pixel-shuffle conv), other shapes keep the hi + lo layout (lo halves = 0 on such weights)."""
    cout, cin = w_shape[0], w_shape[1]
    if flags.no_conv24 or hi_only:
        return None, 'hi_lo'
    two48 = cout == 48 and len(src_channels) == 2                # 48 + 48 -> 48 as two channel halves (A/B knob)
    if (conv24_ok(w_shape, src_channels, shuffle, f32) and not (cout == 32 and flags.no_conv32) and
            not (two48 and flags.no_conv48x2)):
        return 'conv24', 'fp16' if wfmt == 'fp16' and cout in (24, 32) else 'hi_lo'
    if shuffle and conv_shuffle2_ok(w_shape, src_channels, f32) and not flags.no_conv_shuffle2:
        return 'shuffle2', 'fp16' if wfmt == 'fp16' and cin == 24 else 'hi_lo'
    return None, 'hi_lo'


def pack_conv24(w, b, src_channels, shuffle_group=False, half_group=False, wfmt='hi_lo'):
    """uint8 blob of one conv for refvsr_conv24 / refvsr_conv48: fp16 [S][NF][64 lanes][8] (_fill_frags) + bias floats (32 | 64), in
    the row layout 'hi_lo24' (24 outputs) | 'hi_lo16' (32 | 48 outputs: NF = 4 | 6), or for wfmt='fp16' (the refvsr_*_f16w twins,
    ABI 15) 'fp16': NF = 2 | 2 | 3 for 24 | 32 | 48 outputs, same bias tail."""
    assert wfmt in ('hi_lo', 'fp16'), wfmt
    w, b = _np(w), _np(b)
    assert conv24_ok(w.shape, src_channels, shuffle_group=shuffle_group, half_group=half_group), (w.shape, src_channels)
    cout = w.shape[0]
    if cout == 48 and [_pad8(c) for c in src_channels] == [48, 48]:
        # 48 + 48 -> 48 (refvsr_conv48's two-source form): two channel-half blobs of the 24-output layout (NCG = 12 plan), back to back
        return torch.cat([pack_conv24(w[0:24], b[0:24], src_channels, half_group=True, wfmt=wfmt),
                          pack_conv24(w[24:48], b[24:48], src_channels, half_group=True, wfmt=wfmt)])
    Wk, _, ncg = kmatrix(w, src_channels)
    layout = 'fp16' if wfmt == 'fp16' else 'hi_lo24' if cout == 24 else 'hi_lo16'
    return _blob(_fill_frags(Wk, ncg, layout), b, _nbias(cout))


def pack_conv_shuffle2(w, b, wfmt='hi_lo'):
    """uint8 blobs of the C -> 4 C pixel-shuffle conv for refvsr_conv_shuffle2 (C = 24 | 48): 2 | 4 conv48-style blobs of 48 output
    rows, back to back.  F.pixel_shuffle(2) puts conv channel 4 c + 2 dy + dx at channel c of sub-pixel (dy, dx); the kernel wants
    a lane's four consecutive accumulator rows to be four consecutive channels of one sub-pixel:
      C = 24: blob z = dy, row R -> sub-pixel dx = R // 24, channel R % 24;   C = 48: blob z = 2 dy + dx, row R = channel R.
    wfmt='fp16': the blobs in pack_conv24's fp16 weight format (refvsr_conv_shuffle2_f16w, C = 24)."""
    w, b = _np(w), _np(b)
    c = w.shape[1]
    assert conv_shuffle2_ok(tuple(w.shape), [c]), tuple(w.shape)
    blobs = []
    for z in range(2 if c == 24 else 4):
        R = np.arange(48)
        rows = 4 * (R % 24) + 2 * z + R // 24 if c == 24 else 4 * R + z
        blobs.append(pack_conv24(w[rows], b[rows], [c], shuffle_group=True, wfmt=wfmt))
    return torch.cat(blobs)
