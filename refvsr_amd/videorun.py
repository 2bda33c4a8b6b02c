"""Video in, video out (extension): super-resolve a pair of .y4m files -- the ultra-wide LR stream and the wide reference stream --
into a .y4m file, Y'CbCr on both sides of the network (4:2:0, 4:2:2 or 4:4:4; centre- or left-sited chroma, as the files say):

    python -m refvsr_amd.videorun --config config_RefVSR_small_L1 --ckpt_abs_name CKPT --lr uw.y4m --ref w.y4m --out sr.y4m
        [--frame_num 5] [--frame_group 4] [--video_depth 8|10] [--yuv_matrix bt709|bt601] [--yuv_range limited|full]
        [--chroma bilinear|nearest] [--scene_cut 0.1 | --cuts 12,40,...]
        [--in_siting centre|left] [--out_chroma 420|422|444] [--out_siting centre|left]
        [--in_down K [--score scores.txt]] [--out_size WxH]
        [--io sync|stream|auto] [--io_depth 2] [--io_timeout 120]
        [--out_format y4m|mjpeg] [--jpeg_quality 90]

The files are read frame by frame (yuv.Y4MReader), the windows are the reference's (evalrun.window_indices: clip edges replicate
frames, data_loader/datasets.py:222-234), the network runs forward_group with frame ids, config.input_yuv taken from the files and
config.result_yuv = 'i420' | 'i420p10' (--out_chroma: the 'i422' / 'i444' forms), and 'yuv' goes to the output through
yuv.Y4MWriter.  No scores, no images: evalrun.py has those.  The input's sampling and siting are the files' (C420mpeg2: left; C422:
left; --in_siting overrides what a file says); the output keeps both unless told otherwise, so its C tag is the input's.

A file with cuts (--scene_cut T: found from the LR stream's luma, ops.luma_sad + scene.py; --cuts: given) is run as the reference would
run its scenes as separate clips: windows clamped at the cuts, no group across one, Network.reset() and is_first_frame at each
(scene.GroupPlanner).  With neither option the file is one clip, as before.

--in_down K (2..8) evaluates the way the paper does: every file frame is decoded once at file size (ops.yuv_to_frames) and down-scaled
once by K with the antialiased bicubic ops.resize_aa -- the 'BI' degradation that made the dataset's LRx4 folders -- and the network
runs on those frames as RGB windows (uint8 from 8-bit files: what an LRx4 PNG holds; float32 from 10-bit ones), config.input_yuv off.
--score FILE (K == config.scale) then scores every result against the LR stream's own file frame, decoded float32, on the device
(ops.score_frames): a line `frame psnr ssim` per frame and a final `mean` line.  --out_size WxH writes the result at another size:
config.result_yuv off, each group's results through ops.resize_aa and ops.result_to_yuv.  All three are off by default, and off
means the calls, the launches and the bytes of a run without them.

--out sr.mjpeg (or --out_format mjpeg) writes an MJPEG stream: one baseline JPEG file per frame, back to back (jpeg.MJPEGWriter), the
entropy-coded data made on the device (ops.jpeg_encode: about a tenth of the 4:2:0 bytes leaves it).  JFIF fixes the output's colour:
config.result_yuv = 'i420' ('i444' with --out_chroma 444), BT.601, full range, centre-sited, 8 bits, whatever the input files say --
--yuv_matrix and --yuv_range then describe the input only.  --out_chroma 422, --video_depth 10 and --out_siting left are refused; a
10-bit input with an 8-bit JPEG result is fine, and --out_size, --in_down, --score, --scene_cut and --cuts combine with it as with
y4m.  The stream carries no frame rate: ffmpeg reads it with -f mjpeg -framerate N.  Off by default: a run without the options makes
no new launch and writes the bytes it wrote before.

Pipes (--io).  Frames of this size come from a decoder process and go to an encoder process: --lr, --ref and --out may be FIFOs, one of
--lr / --ref and --out may be '-' (with --out - every message goes to stderr):

    DECODER .. | python -m refvsr_amd.videorun .. --lr - --ref w.fifo --out - | ENCODER ..

--io sync is the loop above: read, stack and upload, forward_group, read back, write, one after the other on one thread, three
regular files (run_sync).  --io stream is the same plan and the same calls -- configure(), prepare(), scene.GroupPlanner with the
length unknown, forward_group with the same windows, ids and is_first_frame, Network.reset() at each scene -- and the same bytes, with
the I/O around the calls instead of between them (run_stream): one reader thread per input and one writer thread (streamio.py; host
memory and file descriptors only, every GPU call is made on the caller's thread and stream); every file frame goes to the device once,
from a pinned staging ring into a frame store, and the windows are stacked there (the sync loop uploads a frame t times); results leave
through a pinned ring behind an event, --io_depth groups in flight, only the oldest waited for.  --io auto (default) is stream when one
of the three ends is '-' or no regular file, else sync.  An input that delivers nothing for --io_timeout seconds ends the run instead
of hanging it.  config.EVAL.io_stats says where the wall time went; profiles/videorun_stream_timing.txt has it measured.

What a feature adds is written once (DESIGN.md 2.r'; tests/test_videorun_runs.py pins both loops call by call on the CPU): options()
is EVAL as one checked record, check_pair() / checked_cuts() the header stage, prepare() gives the one Plan both loops read, classify()
turns frames into scenes, group_step() is a group on the device, finish() and pipelined() the tail; a loop keeps how frames come and go.
"""
import argparse
import collections
import contextlib
import os
import sys
import time

import numpy as np
import torch

from . import metrics, scene
from .evalrun import load_checkpoint
from .yuv import (Y4MReader, Y4MWriter, check_chroma, check_matrix, check_range, depth_of, effective_siting, resolve_input,
                  sampling_of, sink_name)


OUT_FORMATS = ('y4m', 'mjpeg')
IO_MODES = ('sync', 'stream', 'auto')


def out_format(fmt, out_path):
    """EVAL.out_format checked and resolved: 'y4m' | 'mjpeg'; None: by the extension of a path, .mjpeg / .mjpg is mjpeg, everything
    else (and '-' and file objects) y4m."""
    if fmt is None:
        return 'mjpeg' if isinstance(out_path, str) and out_path.lower().endswith(('.mjpeg', '.mjpg')) else 'y4m'
    if fmt not in OUT_FORMATS:
        raise ValueError('videorun: --out_format must be y4m or mjpeg (got %r)' % (fmt,))
    return fmt


def _integer(flag, lo, hi, default):
    """check(v): an integer lo..hi; None: the default."""
    def check(v):
        if v is None:
            return default
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError('videorun: %s must be an integer %d..%d (got %r)' % (flag, lo, hi, v))
        return int(v)
    return check


check_in_down = _integer('--in_down', 2, 8, None)     # EVAL.in_down: None (off) or K
check_io_depth = _integer('--io_depth', 1, 4, 2)      # EVAL.io_depth: the groups in flight in the stream loop


def check_out_size(size):
    """EVAL.out_size: None (off), 'WxH' or (W, H), both even and positive -> (W, H)."""
    if size is None:
        return None
    try:
        w, h = (int(v) for v in (size.lower().split('x') if isinstance(size, str) else size))
    except (TypeError, ValueError):
        raise ValueError('videorun: --out_size must be WxH (got %r)' % (size,))
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise ValueError('videorun: --out_size needs even, positive W and H (got %dx%d)' % (w, h))
    return w, h


def check_io_timeout(s):
    """EVAL.io_timeout: the seconds a source may deliver nothing, or the sink take nothing, before the run ends (None: 120)."""
    if s is None:
        return 120.0
    try:
        v = float(s)
    except (TypeError, ValueError):
        v = float('nan')
    if not 0.0 < v < float('inf'):
        raise ValueError('videorun: --io_timeout must be a positive number of seconds (got %r)' % (s,))
    return v


def _one_of(flag, values, text):
    """check(v): None stays None (the run decides from the input), anything else is one of `values` (compared as written)."""
    def check(v):
        if v is not None and str(v) not in values:
            raise ValueError('videorun: %s must be %s (got %r)' % (flag, text, v))
        return v
    return check


def _or(default):
    return lambda v: default if v is None else v


# The EVAL fields videorun knows: name -> check; check(value) is the checked value, check(None) the default of a field that is not set.
OPTIONS = collections.OrderedDict((
    ('ckpt_abs_name', _or(None)), ('frame_group', lambda g: max(1, int(4 if g is None else g or 1))),
    ('scene_cut', lambda th: None if th is None else scene.check_threshold(th)), ('cuts', _or(None)),
    ('in_siting', _or(None)), ('out_chroma', _one_of('--out_chroma', ('420', '422', '444'), '420, 422 or 444')),
    ('out_siting', _one_of('--out_siting', ('centre', 'left'), "'centre' or 'left'")), ('video_depth', _one_of('--video_depth', ('8', '10'), '8 or 10')),
    ('in_down', check_in_down), ('score_file', _or(None)), ('out_size', check_out_size),
    ('io', _or('auto')), ('io_depth', check_io_depth), ('io_timeout', check_io_timeout),
    ('out_format', _or(None)), ('jpeg_quality', _or(90)),
    # input_range_set: config.input_yuv_range is given, not the file's to set; out_range_from_input: config.yuv_range is the LR header's
    ('input_range_set', bool), ('out_range_from_input', bool),
))
Options = collections.namedtuple('Options', tuple(OPTIONS))


def options(config, paths=None):
    """config.EVAL as a checked, immutable record (OPTIONS), or the one-line ValueError of a field or of a pair of fields (refusals).
    paths = (lr, ref, out): out_format and io are resolved against them -- 'y4m' | 'mjpeg' and 'sync' | 'stream'; without them
    (configure() called on its own) they stay what EVAL says."""
    o = dict((name, check(getattr(config.EVAL, name, None))) for name, check in OPTIONS.items())
    if paths is not None:
        o['out_format'], o['io'] = out_format(o['out_format'], paths[2]), io_mode(o['io'], *paths)
    refusals(o, int(config.scale))
    return Options(**o)


def refusals(o, scale):
    """What the fields refuse of each other, one line each."""
    if o['scene_cut'] is not None and o['cuts'] is not None:
        raise ValueError('videorun: scene_cut and cuts exclude each other')
    if o['score_file'] is not None and o['in_down'] != scale:
        raise ValueError('videorun: --score needs --in_down %d, the scale of the config (got --in_down %s)' % (scale, o['in_down']))
    if o['out_format'] == 'mjpeg':
        from . import jpeg
        if o['out_chroma'] is not None and str(o['out_chroma']) not in ('420', '444'):
            raise ValueError('videorun: an mjpeg result is 4:2:0 or 4:4:4 (--out_chroma %s is not built)' % (o['out_chroma'],))
        if o['video_depth'] not in (None, 8):
            raise ValueError('videorun: an mjpeg result has 8 bits per sample (got --video_depth %s)' % (o['video_depth'],))
        if o['out_siting'] not in (None, 'centre'):
            raise ValueError("videorun: an mjpeg result has centre-sited chroma, as JFIF defines it (got --out_siting %s)" % (o['out_siting'],))
        try:
            o['jpeg_quality'] = jpeg.check_quality(o['jpeg_quality'])
        except ValueError:
            raise ValueError('videorun: --jpeg_quality must be an integer 1..100 (got %r)' % (o['jpeg_quality'],))


def is_stream_end(p):
    """An end of the run that is not a regular file: '-', a file object, a FIFO, a device (/dev/null).  A path that does not exist yet
    is the regular file it will be."""
    return not isinstance(p, str) or p == '-' or (os.path.exists(p) and not os.path.isfile(p))


def io_mode(io, lr_path, ref_path, out_path):
    """EVAL.io checked and resolved: 'sync' | 'stream'.  'auto' (None: the default) is 'stream' when one of the three ends is no
    regular file; 'sync' needs three regular files; at most one input can be '-'."""
    io = io or 'auto'
    if io not in IO_MODES:
        raise ValueError('videorun: --io must be one of %s (got %r)' % (', '.join(IO_MODES), io))
    if lr_path == '-' and ref_path == '-':
        raise ValueError("videorun: --lr and --ref cannot both be '-': there is one standard input")
    piped = [p for p in (lr_path, ref_path, out_path) if is_stream_end(p)]
    if io == 'sync' and piped:
        raise ValueError('videorun: --io sync reads and writes regular files (%s is none): --io stream, or --io auto' % sink_name(piped[0]))
    return 'stream' if io == 'stream' or piped else 'sync'


def open_pair(lr_path, ref_path, siting=None):
    """The two readers of a run; ValueError (one line) unless geometry, format (sampling, depth and chroma siting) and frame count
    agree.  siting ('centre' | 'left'; --in_siting): what both files' chroma siting is taken to be, whatever their headers say."""
    with contextlib.ExitStack() as opened:
        lr = opened.enter_context(Y4MReader(lr_path))
        ref = opened.enter_context(Y4MReader(ref_path))
        check_pair(lr, ref, siting, (lr_path, ref_path))
        opened.pop_all()                              # (both stay open: the run closes them)
    return lr, ref


def check_pair(lr, ref, siting, names):
    """The header stage of both loops: the --in_siting override, then the one-line ValueError of two readers that are not the streams
    of one run -- pair_mismatch, and where the lengths are known (regular files) a frame count that differs or is 0."""
    if siting is not None:
        lr.siting, ref.siting = effective_siting(lr.fmt, siting), effective_siting(ref.fmt, siting)
    bad = pair_mismatch(lr, ref)
    if bad is None and lr.length is not None and ref.length is not None:
        if lr.length != ref.length:
            bad = 'frame count differs (%d and %d)' % (lr.length, ref.length)
        elif lr.length < 1:
            bad = 'no frames'
    if bad:
        raise ValueError('videorun: %s and %s: %s' % (names[0], names[1], bad))


def pair_mismatch(lr, ref):
    """What keeps two readers from being the streams of one run -- geometry, format, chroma siting -- or None."""
    if (lr.h, lr.w) != (ref.h, ref.w):
        return 'geometry differs (%d x %d and %d x %d)' % (lr.h, lr.w, ref.h, ref.w)
    if lr.fmt != ref.fmt:
        return 'format differs (%s and %s)' % (lr.fmt, ref.fmt)
    if lr.siting != ref.siting:
        return 'format differs (%s with %s- and %s-sited chroma; --in_siting declares one for both)' % (lr.fmt, lr.siting, ref.siting)
    return None


def checked_cuts(cuts, n=None):
    """EVAL.cuts as scene.check_cuts takes them (n: the frame count, where it is known), its refusal in videorun's words."""
    try:
        return scene.check_cuts(cuts or (), n)
    except ValueError as e:
        raise ValueError('videorun: %s%s' % (e, '' if n is None else ' (%d frames)' % n))


def configure(config, reader, opt=None):
    """The run's fields of `config` from the LR file: input_yuv (always the files' format), input_yuv_siting (the reader's: the file's,
    or check_pair's override), input_yuv_range (the file's XCOLORRANGE unless set: EVAL.input_range_set), result_yuv (by
    EVAL.video_depth; None: the input's depth -- and by EVAL.out_chroma '420' | '422' | '444'; None: the input's sampling), yuv_siting
    (EVAL.out_siting; None: 'left' for 4:2:2 output, which is what its tag means, else the input's).
    EVAL.in_down (K; None: off): input_yuv is None -- the network gets RGB windows, the run decodes and down-scales the files' frames;
    the file must be K times an even size.  EVAL.out_size ((W, H); None: off): result_yuv is None -- the run resizes and converts --
    and the format the run would have used is left in EVAL.out_yuv (always set).  EVAL.score_file needs in_down == config.scale.
    EVAL.out_format == 'mjpeg': the result is what JFIF means -- 'i420' ('i444' under out_chroma 444), 8 bits, and config.yuv_matrix =
    'bt601', yuv_range = 'full', yuv_siting = 'centre' for the output, whatever the files say (refusals() has what it refuses).
    opt: the run's options() (None: taken from config.EVAL here)."""
    E = config.EVAL
    opt = opt or options(config)
    mjpeg, down, size = opt.out_format == 'mjpeg', opt.in_down, opt.out_size
    if down is not None and (reader.h % down or reader.w % down or (reader.h // down) % 2 or (reader.w // down) % 2):
        raise ValueError('videorun: --in_down %d needs frames of %d times an even size (got %d x %d)' % (down, down, reader.w, reader.h))
    if size is not None:
        rh, rw = (int(config.scale) * (v // (down or 1)) for v in (reader.h, reader.w))
        if rw > 8 * size[0] or rh > 8 * size[1]:
            raise ValueError('videorun: --out_size %dx%d is less than an eighth of the %dx%d result on an axis' % (size + (rw, rh)))
    E.in_down, E.out_size, E.score_file = down, size, opt.score_file
    config.input_yuv = reader.fmt if down is None else None
    config.input_yuv_siting = reader.siting
    out = str(opt.out_chroma or ('420' if mjpeg else sampling_of(reader.fmt)))
    config.yuv_siting = 'centre' if mjpeg else opt.out_siting or ('left' if out == '422' else reader.siting)
    if not opt.input_range_set:
        config.input_yuv_range = reader.range
    depth = 8 if mjpeg else opt.video_depth or depth_of(reader.fmt)
    E.out_yuv = 'i%s%s' % (out, '' if depth == 8 else 'p10')
    config.result_yuv = E.out_yuv if size is None else None
    if mjpeg:
        E.jpeg_quality = opt.jpeg_quality
        config.yuv_matrix, config.yuv_range = 'bt601', 'full'
    return config


# What both loops read of a run: t frames per window, G per group; down, size, score_file: --in_down K, --out_size (W, H), --score FILE
# (None: off); decode: the arguments of ops.yuv_to_frames under --in_down; the output's format, (h, w), range, matrix, siting, JPEG quality
Plan = collections.namedtuple('Plan', 'opt net dev t G down size score_file decode out_yuv out_hw out_range matrix siting mjpeg quality')


def prepare(config, lr, net=None, opt=None):
    """What both loops do between the LR header and the first frame: configure(), the network (built here unless passed in) with the
    run's formats in its config, the refusals of a network that already runs otherwise.  Returns the run's Plan."""
    opt = opt or options(config)
    configure(config, lr, opt)
    mjpeg, down, size = opt.out_format == 'mjpeg', opt.in_down, opt.out_size
    if net is None:
        from . import SRNet
        net = SRNet(config).to('cuda').eval()
        if opt.ckpt_abs_name:
            load_checkpoint(net, opt.ckpt_abs_name)
    nc = net.Network.config
    if nc is not config:                              # (a caller's net may carry a config of its own)
        for k in ('input_yuv', 'input_yuv_range', 'input_yuv_siting', 'result_yuv', 'yuv_siting') + (('yuv_matrix', 'yuv_range') if mjpeg else ()):
            setattr(nc, k, getattr(config, k))
    if net.Network._engines and (net.Network._engines[0].input_yuv is None) != (down is not None):
        raise RuntimeError('videorun: the network passed in already runs %s config.input_yuv; pass a fresh one' % ('with' if down else 'without'))
    if net.Network._engines and size is not None and net.Network._engines[0].result_yuv is not None:
        raise RuntimeError('videorun: the network passed in already runs with config.result_yuv; pass a fresh one')
    scale = int(config.scale)
    rh, rw = (lr.h * scale, lr.w * scale) if down is None else (lr.h // down * scale, lr.w // down * scale)
    decode = None
    if down is not None:                              # fmt, matrix, range, chroma, siting of ops.yuv_to_frames for the files' frames
        decode = (resolve_input(lr.fmt, getattr(config, 'input_yuv_matrix', None), getattr(config, 'input_yuv_range', None),
                                getattr(config, 'input_yuv_chroma', None), lr.siting) + ('centre',))[:5]
    return Plan(opt=opt, net=net, dev=next(net.parameters()).device, t=int(config.frame_num), G=opt.frame_group, down=down, size=size,
                score_file=opt.score_file, decode=decode, out_yuv=config.EVAL.out_yuv,
                out_hw=(rh, rw) if size is None else (size[1], size[0]), out_range=getattr(config, 'yuv_range', None) or 'limited',
                matrix=getattr(config, 'yuv_matrix', None) or 'bt709', siting=config.yuv_siting, mjpeg=mjpeg, quality=opt.jpeg_quality)


def open_writer(p, out_path, fps):
    """The run's writer: a yuv.Y4MWriter, or a jpeg.MJPEGWriter for an MJPEG stream."""
    if p.mjpeg:
        from .jpeg import MJPEGWriter
        return MJPEGWriter(out_path)
    return Y4MWriter(out_path, p.out_hw[0], p.out_hw[1], p.out_yuv, fps, p.out_range, p.siting)


def classify(planner, det, cutset, new, sads):
    """Frames `new` (consecutive indices, just read) -> scenes, into the planner: membership in the given cuts, or under --scene_cut
    (det: the scene.SceneDetector) frame 0 opens the first scene and ONE sads(pairs) call -- the loop's own: the SADs of the LR frames
    k in `pairs` against their predecessors, as a list -- scores the new consecutive pairs."""
    if det is None:
        for k in new:
            planner.push(k in cutset)
        return
    if new and new[0] == 0:
        planner.push(False)                           # (frame 0 opens the first scene)
    pairs = [k for k in new if k > 0]
    if pairs:
        for sad in sads(pairs):
            planner.push(det.push(sad))


def group_step(p, group, windows, small, retire_all=None):
    """One group of the plan on the device, nothing read back: Network.reset() at a scene start (a scene is a clip of its own;
    retire_all(): what the loop has to finish first), the windows, forward_group, the scores (the unscaled result against the LR file
    frame, one 16-byte row per frame; None without --score) and the frames to write.  Returns (lrs, rfs, got, scores, frames)."""
    from . import ops
    fs, wins, first = group
    if first and fs[0] > 0:
        if retire_all is not None:
            retire_all()
        p.net.Network.reset()
    lrs, rfs = windows(wins)
    got = p.net.Network.forward_group(lrs, rfs, wins, is_first_frame=first)
    sc = ops.score_frames([r[0] for r in got['result']], [small[f][2] for f in fs]) if p.score_file is not None else None
    if p.size is None:
        ys = [y[0] for y in got['yuv']]
    else:
        ys = resized_yuv(ops, [r[0] for r in got['result']], p.size, p.out_yuv, p.matrix, p.out_range, p.siting)
    return lrs, rfs, got, sc, ys


def down_scaled_windows(p, lr, small, held, wins, load):
    """--in_down: the windows as RGB tensors [B, t, 3, h / K, w / K].  small: frame index -> (lr, ref) down-scaled (+ the LR decode
    under --score: its ground truth), kept for the frames in `held` (the frames the run still holds).  A file frame not in it yet is
    decoded once at file size (ops.yuv_to_frames) and resized once (ops.resize_aa: uint8 from 8-bit files, float32 from 10-bit ones)
    -- the LR and the reference frames of a call together; load(new) -> their buffers on the device, [2 len(new), rows, w], LR first."""
    from . import ops
    for k in [k for k in small if k not in held]:
        del small[k]
    new = sorted({i for w_ in wins for i in w_ if i not in small})
    if new:
        full = ops.yuv_to_frames(load(new), lr.h, lr.w, *p.decode)
        lo = ops.resize_aa(full, lr.h // p.down, lr.w // p.down, 'uint8' if depth_of(lr.fmt) == 8 else 'float32')
        for q, i in enumerate(new):
            small[i] = (lo[q], lo[len(new) + q], full[q] if p.score_file is not None else None)
    return tuple(torch.stack([torch.stack([small[i][j] for i in w_]) for w_ in wins]) for j in (0, 1))


def resized_yuv(ops, results, size, fmt, matrix, range, siting):
    """--out_size: results [3, sh, sw] -> [B, rows, W] frames of `fmt` at size = (W, H): ops.resize_aa (clamped float32), then
    ops.result_to_yuv -- one launch each per group."""
    return ops.result_to_yuv(ops.resize_aa(results, size[1], size[0], 'float32', True), fmt, matrix, range, effective_siting(fmt, siting))


def score_rows(fs, rows):
    """--score: (frame, psnr, ssim) of the frames fs from their {mse, ssim} rows (a list, read back)."""
    return [(f, metrics.psnr_from_mse(m), s_) for f, (m, s_) in zip(fs, rows)]


def write_scores(path, scores):
    """--score: `frame psnr ssim` per frame (repr of the float64s: they read back bit for bit), then `mean psnr ssim` -- the sums in
    frame order over the count."""
    with open(path, 'w') as f:
        for fr, p, s_ in scores:
            f.write('%d %r %r\n' % (fr, p, s_))
        k = max(len(scores), 1)
        f.write('mean %r %r\n' % (sum(p for _, p, _ in scores) / k, sum(s_ for _, _, s_ in scores) / k))


def finish(config, p, cuts, scores):
    """What a finished run leaves behind: EVAL.scene_cuts, and under --score EVAL.scores and the score file."""
    config.EVAL.scene_cuts = tuple(cuts)
    if p.score_file is not None:
        config.EVAL.scores = scores
        write_scores(p.score_file, scores)


@contextlib.contextmanager
def pipelined(net, always_synchronize=False):
    """The network pipelined and reset for the run; on the way out, however the run ended, no device work is pending (where the state
    is restored, or always: the stream loop's copies) and the network is pipelined or not as it was found."""
    was = bool(getattr(net.Network.config, 'pipelined', False))
    net.Network.set_pipelined(True)
    net.Network.reset()
    try:
        yield
    finally:
        if always_synchronize or not was:
            torch.cuda.synchronize()
        if not was:
            net.Network.set_pipelined(False)


def run(config, lr_path, ref_path, out_path, net=None):
    """Super-resolve lr_path with ref_path into out_path; returns (frames written, seconds in the network calls).  config: a model
    config (EVAL.frame_group, frame_num, yuv_matrix / yuv_range for the output, input_yuv_matrix / input_yuv_chroma for the input);
    net: an SRNet built from that config (None: built here, EVAL.ckpt_abs_name loaded) -- its engines must not exist yet, they take
    the input format from the config at their construction.
    EVAL.scene_cut (a scene-score threshold in (0, 1]) or EVAL.cuts (frame indices in (0, n), increasing) make every scene a clip of
    its own; the cuts the run used are left in config.EVAL.scene_cuts (a tuple; empty without the options), and under scene_cut the
    seconds include the detector's upload and its ops.luma_sad call per group.
    EVAL.in_down / EVAL.score_file / EVAL.out_size: the module header; the scores are left in config.EVAL.scores, a list of (frame,
    psnr, ssim), and the seconds include the decode, the resizes and the scorer.
    EVAL.io ('sync' | 'stream' | 'auto'; None: 'auto'), EVAL.io_depth, EVAL.io_timeout: the module header and run_stream(), which takes
    over when the mode is 'stream' -- the paths may then be '-', FIFOs or binary file objects, and the seconds are the loop's wall time."""
    opt = options(config, (lr_path, ref_path, out_path))
    config.EVAL.out_format = opt.out_format
    return (run_stream if opt.io == 'stream' else run_sync)(config, opt, lr_path, ref_path, out_path, net)


def run_sync(config, opt, lr_path, ref_path, out_path, net):
    """run() under EVAL.io = 'sync': three regular files, one thread, one step after the other."""
    from . import ops
    lr, ref = open_pair(lr_path, ref_path, opt.in_siting)
    writer = None
    try:
        n = lr.length
        cuts = checked_cuts(opt.cuts, n)
        if opt.out_range_from_input:
            config.yuv_range = lr.range
        p = prepare(config, lr, net, opt)
        dev = p.dev
        writer = open_writer(p, out_path, lr.fps)
        planner = scene.GroupPlanner(n, p.t, p.G)
        det = scene.SceneDetector(lr.h, lr.w, depth_of(lr.fmt), opt.scene_cut) if opt.scene_cut is not None else None
        held = collections.OrderedDict()                  # frame index -> (lr buffer, ref buffer): the frames the next windows read
        small = {}                                        # --in_down: frame index -> (lr, ref) down-scaled [3, h / K, w / K] (+ the LR decode)
        scores, cutset = [], set(cuts)
        nread, seconds = 0, 0.0

        def read_to(upto):
            """Frames [nread, upto) of both files into `held`; their indices."""
            nonlocal nread
            new = list(range(nread, upto))
            for k in new:
                a, b = lr.read(), ref.read()
                if a is None or b is None:
                    raise ValueError('videorun: %s: truncated file' % (lr_path if a is None else ref_path))
                held[k] = (a, b)
            nread = max(nread, upto)
            return new

        def sads(pairs):
            """The detector's own upload -- the new LR frames and the one before them -- and its ONE ops.luma_sad call; timed."""
            nonlocal seconds
            t0 = time.time()
            x = torch.from_numpy(np.stack([held[k][0] for k in range(pairs[0] - 1, pairs[-1] + 1)])).to(dev)
            out = ops.luma_sad(x[1:], x[:-1], lr.h, lr.w, lr.fmt).cpu().tolist()
            seconds += time.time() - t0
            return out

        def windows(wins):
            """The host stack of t copies per window, uploaded; --in_down: a file frame not seen yet goes to the device once."""
            if p.down is None:
                return tuple(torch.from_numpy(np.stack([np.stack([held[i][j] for i in w_]) for w_ in wins])).to(dev) for j in (0, 1))
            return down_scaled_windows(p, lr, small, held, wins, lambda new: torch.from_numpy(np.stack([held[i][j] for j in (0, 1) for i in new])).to(dev))

        with pipelined(p.net), torch.no_grad():
            while not planner.done():
                classify(planner, det, cutset, read_to(planner.need()), sads)
                fs, wins, first = planner.pop()
                for k in [k for k in held if k < min(wins[0])]:
                    del held[k]
                t0 = time.time()
                _, _, _, sc, ys = group_step(p, (fs, wins, first), windows, small)
                if sc is not None:
                    scores.extend(score_rows(fs, sc.cpu().tolist()))
                if p.mjpeg:                               # (the files of the group: only the compressed bytes leave the device)
                    ys = ops.jpeg_encode(ys, p.out_hw[0], p.out_hw[1], p.out_yuv, p.quality)
                else:
                    ys = [y.cpu().numpy() for y in ys] if p.size is None else ys.cpu().numpy()
                seconds += time.time() - t0
                for y in ys:
                    writer.write(y)
        finish(config, p, det.cuts if det is not None else cuts, scores)
        return writer.frames, seconds
    finally:
        lr.close()
        ref.close()
        if writer is not None:
            writer.close()


def sample_dtype(fmt):
    return torch.uint8 if depth_of(fmt) == 8 else torch.uint16


def stacked(frames):
    """torch.stack of device frames of one shape; 16-bit samples are stacked as int16 bit patterns (a plain copy either way)."""
    if frames[0].dtype != torch.uint16:
        return torch.stack(frames)
    return torch.stack([f.view(torch.int16) for f in frames]).view(torch.uint16)


def held_bound(t, G, D):
    """The frames of one input stream the stream loop holds at most, on the device (frame store + the slots of the groups in flight) as
    in the pinned staging ring: t + (D + 1) G + 2."""
    return t + (D + 1) * G + 2


def run_stream(config, opt, lr_path, ref_path, out_path, net):
    """run() under EVAL.io = 'stream' (module header): the same configure(), plan (scene.GroupPlanner, length unknown), calls and
    bytes, with reader and writer threads (streamio.py) around the calls and every file frame uploaded once.  All GPU calls are made
    here, on the caller's thread and current stream; the threads touch pinned host memory and file descriptors only.

    A frame goes from its pinned staging buffer to a device slot of the frame store (non_blocking), the windows of a group are stacked
    on the device from the store and handed to forward_group with input_ready=None -- the engine's internal streams wait for the
    caller's stream, which has the copies and the stacking on it, and record the windows for the allocator (INTEGRATION, input_ready).
    The group's frames are copied to pinned output buffers (non_blocking) with an event behind them; up to EVAL.io_depth groups are
    in flight, and only the oldest one's event is ever waited for.  Until that event has completed the group keeps what its call was
    given and what it returned -- the windows, the store slots evicted under it, its staging and output buffers.  At a scene start the
    groups in flight are retired first: Network.reset() finds the device where the sync loop's reset finds it.
    Returns (frames written, wall seconds of the loop); config.EVAL.io_stats has the split."""
    from . import ops, streamio
    from .yuv import Y4MStreamReader, frame_shape
    D, timeout = opt.io_depth, opt.io_timeout
    t, G = int(config.frame_num), opt.frame_group
    ring = (D + 1) * G + t // 2                       # D groups in flight and one being read; the first group reads t // 2 ahead
    assert ring <= held_bound(t, G, D)
    names = [sink_name(p) for p in (lr_path, ref_path)]
    io = streamio.Run()
    srcs = [streamio.FrameSource(io, lambda stop, p=p: Y4MStreamReader(p, stop), name, ring, timeout) for p, name in zip((lr_path, ref_path), names)]
    sink = writer = None
    finished = False
    wall0 = time.time()
    stats = dict(frames=0, uploads=0, groups=0, max_in_flight=0, max_held=0, read_wait=0.0, device_wait=0.0, write_wait=0.0, wall=0.0)
    try:
        tens = []                                         # per input: id(numpy view) -> the pinned tensor it views

        def staging(rd):
            pin = torch.empty((ring,) + frame_shape(rd.h, rd.w, rd.fmt), dtype=sample_dtype(rd.fmt)).pin_memory()
            views = [pin[i].numpy() for i in range(ring)]
            tens.append(dict((id(v), pin[i]) for i, v in enumerate(views)))
            return views

        # each ring goes to its thread as soon as that stream's header is here: the LR thread drains its pipe while the other opens
        lr = srcs[0].header()
        srcs[0].provide(staging(lr))
        ref = srcs[1].header()
        check_pair(lr, ref, opt.in_siting, names)
        srcs[1].provide(staging(ref))
        cuts = checked_cuts(opt.cuts)
        if opt.out_range_from_input:
            config.yuv_range = lr.range
        p = prepare(config, lr, net, opt)
        dev, out_hw = p.dev, p.out_hw
        writer = open_writer(p, out_path, lr.fps)
        if p.mjpeg:
            # a slot of the ring holds a file of up to the frame's own bytes: header, data, EOI (a larger one -- noise at quality 100 --
            # takes the slow way in retire())
            from . import jpeg
            head = jpeg.header(out_hw[0], out_hw[1], p.out_yuv, p.quality)
            head_np = np.frombuffer(head, np.uint8)
            slot = len(head) + int(np.prod(frame_shape(out_hw[0], out_hw[1], p.out_yuv))) + 2
            copies = torch.cuda.Stream(dev)               # the retired group's copies: never behind the groups still in flight
            out_pin = torch.empty(((D + 1) * G, slot), dtype=torch.uint8).pin_memory()
        else:
            out_pin = torch.empty(((D + 1) * G,) + frame_shape(out_hw[0], out_hw[1], p.out_yuv), dtype=sample_dtype(p.out_yuv)).pin_memory()
        out_views = [out_pin[i].numpy() for i in range(out_pin.shape[0])]
        out_tens = dict((id(v), out_pin[i]) for i, v in enumerate(out_views))
        sink = streamio.FrameSink(io, writer, out_views, sink_name(out_path), timeout)

        planner = scene.GroupPlanner(None, p.t, p.G)
        det = scene.SceneDetector(lr.h, lr.w, depth_of(lr.fmt), opt.scene_cut) if opt.scene_cut is not None else None
        store = collections.OrderedDict()                 # frame index -> (lr slot, ref slot) on the device: what the next windows read
        small = {}                                        # --in_down: frame index -> (lr, ref) down-scaled (+ the LR decode), as in run_sync()
        flight = collections.deque()                      # the groups in flight, oldest first
        staged = []                                       # staging buffers uploaded since the last call: (source, buffer)
        scores, cutset = [], set(cuts)
        nread, ended = 0, False

        def retire():
            """The oldest group in flight: wait for its event, hand its frames to the sink, give its staging buffers back."""
            g = flight.popleft()
            t0 = time.time()
            g['event'].synchronize()
            stats['device_wait'] += time.time() - t0
            if g['scores'] is not None:
                scores.extend(score_rows(g['fs'], g['scores'].tolist()))
            for src, b in g['staged']:
                src.give(b)
            if g['jpeg'] is not None:
                g['out'] = retire_jpeg(*g['jpeg'])
            for b in g['out']:
                sink.put(*b) if isinstance(b, tuple) else sink.put(b)
            stats['frames'] += len(g['out'])

        def retire_all():
            while flight:
                retire()

        def retire_jpeg(dst, meta):
            """The files of a retired group: its sizes came with its event; exactly the compressed bytes of every frame are copied into
            a slot of the pinned ring, between the header and EOI the host writes there.  -> [(buffer, length, data)] for sink.put."""
            offs, sizes = meta[0].tolist(), meta[1].tolist()
            out = []
            with torch.cuda.stream(copies):
                for o, n in zip(offs, sizes):
                    b = sink.take()
                    if len(head) + n + 2 <= slot:
                        out_tens[id(b)][len(head):len(head) + n].copy_(dst[o:o + n], non_blocking=True)
                        out.append((b, len(head) + n + 2, None))
                    else:
                        out.append((b, None, jpeg.assemble(head, dst[o:o + n].cpu().numpy().tobytes())))
            copies.synchronize()
            for b, n, data in out:
                if data is None:
                    b[:len(head)] = head_np
                    b[n - 2:n] = (0xff, 0xd9)
            return out

        def read_to(upto):
            """Frames [nread, upto) of both streams, as far as they go, into the store -- ONE upload per file frame; their indices.
            Behind the last frame the length is known: the refusals that need it, and the planner is told."""
            nonlocal nread, ended
            new = []
            while not ended and nread < upto:
                pair = streamio.next_pair(srcs[0], srcs[1])
                if pair is None:
                    ended = True
                    break
                slots = []
                for j, (_, b) in enumerate(pair):
                    slots.append(tens[j][id(b)].to(dev, non_blocking=True, copy=True))
                    staged.append((srcs[j], b))
                store[nread] = tuple(slots)
                stats['uploads'] += 2
                new.append(nread)
                nread += 1
            return new

        def sads(pairs):
            """One ops.luma_sad call on the store's slots: no upload of its own."""
            t0 = time.time()
            out = ops.luma_sad([store[k][0] for k in pairs], [store[k - 1][0] for k in pairs], lr.h, lr.w, lr.fmt).cpu().tolist()
            stats['device_wait'] += time.time() - t0
            return out

        def windows(wins):
            """Stacked on the device from the store, --in_down too: no upload of its own."""
            if p.down is None:
                return tuple(stacked([store[i][j] for w_ in wins for i in w_]).unflatten(0, (len(wins), t)) for j in (0, 1))
            return down_scaled_windows(p, lr, small, store, wins, lambda new: stacked([store[i][j] for j in (0, 1) for i in new]))

        with pipelined(p.net, True), torch.no_grad():
            while True:
                if len(flight) >= D:
                    retire()
                if not ended:
                    classify(planner, det, cutset, read_to(planner.need()), sads)
                    if ended:
                        if nread == 0:
                            raise ValueError('videorun: %s and %s: no frames' % tuple(names))
                        checked_cuts(cuts, nread)
                        planner.finish()
                group = planner.pop()
                if group is None:
                    assert planner.done()
                    break
                held = [store.pop(k) for k in [k for k in store if k < min(group[1][0])]]     # below the oldest window still to come
                stats['max_held'] = max(stats['max_held'], len(store) + len(held) + sum(len(g['held']) for g in flight))
                lrs, rfs, got, sc_d, ys = group_step(p, group, windows, small, retire_all)
                sc = None
                if sc_d is not None:
                    sc = torch.empty(sc_d.shape, dtype=sc_d.dtype).pin_memory()
                    sc.copy_(sc_d, non_blocking=True)
                out, enc = [], None
                if p.mjpeg:                               # the encode goes out with the group; its sizes come back with its event
                    dst, offsets, sizes = ops.jpeg_encode_device(ys, out_hw[0], out_hw[1], p.out_yuv, p.quality)
                    meta = torch.empty((2, len(ys)), dtype=torch.int64).pin_memory()
                    meta[0].copy_(offsets, non_blocking=True)
                    meta[1].copy_(sizes, non_blocking=True)
                    enc = (dst, meta)
                else:
                    for y in ys:
                        out.append(sink.take())
                        out_tens[id(out[-1])].copy_(y, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                flight.append(dict(event=event, fs=group[0], out=out, staged=staged, held=held, scores=sc, jpeg=enc, keep=(lrs, rfs, got, sc_d, ys)))
                staged = []
                stats['groups'] += 1
                stats['max_in_flight'] = max(stats['max_in_flight'], len(flight))
            retire_all()
            sink.finish()
        finish(config, p, det.cuts if det is not None else cuts, scores)
        finished = True
        return writer.frames, time.time() - wall0
    finally:
        # no thread alive, whatever happened (pipelined() has left no device work pending); the first error stays the one that is raised
        for x in srcs + ([sink] if sink is not None else []):
            x.close()
        stats['read_wait'] = sum(s.waited for s in srcs)
        stats['write_wait'] = sink.waited if sink is not None else 0.0
        stats['wall'] = time.time() - wall0
        config.EVAL.io_stats = stats
        try:
            if writer is not None:
                writer.close()
        except ValueError:
            if finished:                                  # (behind an earlier error that one is the one to raise)
                raise


def build_config(argv=None):
    from .config import get_config
    ap = argparse.ArgumentParser(description='RefVSR on .y4m files: 4:2:0 in, 4:2:0 out (MI355X HIP path)')
    ap.add_argument('--config', '-c', type=str, default='config_RefVSR_small_L1')
    ap.add_argument('--ckpt_abs_name', '-ckpt_abs_name', type=str, default=None)
    ap.add_argument('--lr', required=True, help='the ultra-wide LR stream (.y4m: C420jpeg, C420mpeg2, C420p10, C422, C444 and their 10-bit forms)')
    ap.add_argument('--ref', required=True, help='the wide reference stream (.y4m of the same geometry, format and length)')
    ap.add_argument('--out', required=True, help='the result (.y4m; .mjpeg / .mjpg: an MJPEG stream)')
    ap.add_argument('--out_format', default=None, choices=list(OUT_FORMATS),
                    help='y4m, or mjpeg: one baseline JPEG per frame, coded on the device, BT.601 full range as JFIF defines it '
                         '(default: by the extension of --out, .mjpeg / .mjpg is mjpeg)')
    ap.add_argument('--jpeg_quality', type=int, default=None, metavar='Q', help='--out_format mjpeg: the quality 1..100 (default 90)')
    ap.add_argument('--frame_num', type=int, default=5)
    ap.add_argument('--frame_group', type=int, default=4)
    ap.add_argument('--video_depth', type=int, default=None, choices=[8, 10], help='bits per sample of --out (default: the input files\')')
    ap.add_argument('--yuv_matrix', default='bt709', choices=['bt709', 'bt601'], help='luma coefficients, input and output')
    ap.add_argument('--yuv_range', default=None, choices=['limited', 'full'], help="code range, input and output (default: the LR file's XCOLORRANGE)")
    ap.add_argument('--chroma', default='bilinear', choices=['bilinear', 'nearest'], help='chroma up-sampling of the input')
    ap.add_argument('--in_siting', default=None, choices=['centre', 'left'],
                    help="chroma siting of the input, whatever the files say (default: the files': C420jpeg centre, C420mpeg2 and C422 left)")
    ap.add_argument('--out_chroma', default=None, choices=['420', '422', '444'], help="chroma sampling of --out (default: the input files')")
    ap.add_argument('--out_siting', default=None, choices=['centre', 'left'],
                    help="chroma siting of --out (default: the input's; left for 4:2:2 output, which is what its tag means)")
    ap.add_argument('--scene_cut', type=float, default=None, metavar='T',
                    help='run every scene as a clip of its own; a frame starts a scene where the scene score of the LR stream\'s luma '
                         '(min(mafd, |mafd - previous mafd|) / 100, mafd = mean absolute luma difference to the previous frame on the 8-bit '
                         'scale) is at least T, 0 < T <= 1.  0.1 is a customary starting point; nobody has tuned it for this project.  '
                         'Default: off, the file is one clip')
    ap.add_argument('--cuts', type=str, default=None, metavar='F,F,...',
                    help='the same with the cuts given (an edit list): the indices of the frames that start a scene, increasing, in (0, frames)')
    ap.add_argument('--in_down', type=int, default=None, metavar='K',
                    help='evaluate the way the paper does: decode every file frame at file size, down-scale it by K = 2..8 with the antialiased '
                         'bicubic (the BI degradation of the LRx4 folders) and run the network on that; the file must be K times an even size')
    ap.add_argument('--score', type=str, default=None, metavar='FILE',
                    help='with --in_down K, K the scale of the config: PSNR and SSIM of every result against the LR stream\'s own frame, '
                         'computed on the device; a line `frame psnr ssim` per frame and a final `mean` line')
    ap.add_argument('--out_size', type=str, default=None, metavar='WxH',
                    help='write the result at W x H (even; at least an eighth of the result per axis, up-scaling allowed) through the '
                         'antialiased bicubic instead of at scale x input')
    ap.add_argument('--io', default=None, choices=list(IO_MODES),
                    help="sync: read, run and write one after the other (regular files).  stream: reader and writer threads around the "
                         "network calls, every file frame uploaded once; --lr or --ref (one of them) and --out may be '-' or a FIFO.  "
                         "auto (default): stream when --lr, --ref or --out is '-' or no regular file, else sync")
    ap.add_argument('--io_depth', type=int, default=None, metavar='D', help='--io stream: frame groups in flight, 1..4 (default 2)')
    ap.add_argument('--io_timeout', type=float, default=None, metavar='S',
                    help='--io stream: seconds an input may deliver nothing, or the output take nothing, before the run ends (default 120)')
    args = ap.parse_args(argv)
    try:
        scene_cut = None if args.scene_cut is None else scene.check_threshold(args.scene_cut)
        cuts = None if args.cuts is None else scene.check_cuts(int(c) for c in args.cuts.split(',') if c.strip())
    except ValueError as e:
        raise ValueError('videorun: --scene_cut / --cuts: %s' % (e,))
    if args.frame_num < 3 or args.frame_num % 2 == 0:
        raise ValueError('videorun: --frame_num must be odd and >= 3 (got %d)' % args.frame_num)
    if args.frame_group < 1:
        raise ValueError('videorun: --frame_group must be >= 1 (got %d)' % args.frame_group)
    cfg = get_config('RefVSR_CVPR2022', 'eval', args.config, '')
    cfg.frame_num = args.frame_num
    cfg.center_idx = cfg.frame_num // 2
    cfg.yuv_matrix = cfg.input_yuv_matrix = check_matrix(args.yuv_matrix)
    cfg.input_yuv_chroma = check_chroma(args.chroma)
    E = cfg.EVAL
    E.input_range_set = args.yuv_range is not None
    if args.yuv_range is not None:
        cfg.yuv_range = cfg.input_yuv_range = check_range(args.yuv_range)
    E.scene_cut, E.cuts, E.score_file = scene_cut, cuts, args.score
    for k in ('ckpt_abs_name', 'frame_group', 'video_depth', 'in_siting', 'out_chroma', 'out_siting', 'in_down', 'out_size', 'io', 'io_depth',
              'io_timeout', 'out_format', 'jpeg_quality'):
        setattr(E, k, getattr(args, k))
    opt = options(cfg, (args.lr, args.ref, args.out))           # every refusal that needs no file, before one is opened; EVAL as checked
    for k in ('in_down', 'out_size', 'io', 'io_depth', 'io_timeout', 'out_format', 'jpeg_quality'):
        setattr(E, k, getattr(opt, k))
    cfg.device, cfg.cuda = 'cuda', True
    return cfg, args


def main(argv=None):
    cfg, args = build_config(argv)
    cfg.EVAL.out_range_from_input = not cfg.EVAL.input_range_set      # (the header is read once: by the reader run() opens)
    if args.out == '-':                           # the frames own stdout: whatever the run prints goes to stderr
        with contextlib.redirect_stdout(sys.stderr):
            frames, seconds = run(cfg, args.lr, args.ref, sys.__stdout__.buffer)
    else:
        frames, seconds = run(cfg, args.lr, args.ref, args.out)
    scenes = '' if cfg.EVAL.scene_cut is None and cfg.EVAL.cuts is None else ', %d scenes' % (len(cfg.EVAL.scene_cuts) + 1)
    line = '[VIDEO %s] %d frames -> %s (%.5f sec / frame%s)' % (args.config, frames, args.out, seconds / max(frames, 1), scenes)
    if cfg.EVAL.io == 'stream':
        st = cfg.EVAL.io_stats
        line += ' [stream: the whole loop; waits %.3f s read, %.3f s device, %.3f s write; %d uploads, %d groups, %d in flight]' % (
            st['read_wait'], st['device_wait'], st['write_wait'], st['uploads'], st['groups'], st['max_in_flight'])
    print(line, file=sys.stderr if args.out == '-' else sys.stdout)           # (with --out - the frames own stdout)
    return 0 if frames else 1


if __name__ == '__main__':
    sys.exit(main())
