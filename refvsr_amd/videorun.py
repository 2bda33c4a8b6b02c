"""Video in, video out (extension): super-resolve a pair of .y4m files -- the ultra-wide LR stream and the wide reference stream --
into a .y4m file, Y'CbCr on both sides of the network (4:2:0, 4:2:2 or 4:4:4; centre- or left-sited chroma, as the files say):

    python -m refvsr_amd.videorun --config config_RefVSR_small_L1 --ckpt_abs_name CKPT --lr uw.y4m --ref w.y4m --out sr.y4m
        [--frame_num 5] [--frame_group 4] [--video_depth 8|10] [--yuv_matrix bt709|bt601] [--yuv_range limited|full]
        [--chroma bilinear|nearest] [--scene_cut 0.1 | --cuts 12,40,...]
        [--in_siting centre|left] [--out_chroma 420|422|444] [--out_siting centre|left]
        [--in_down K [--score scores.txt]] [--out_size WxH]

The files are read frame by frame (yuv.Y4MReader), the windows are the reference's (evalrun.window_indices: clip edges replicate
frames, data_loader/datasets.py:222-234), the network runs forward_group with frame ids, config.input_yuv taken from the files and
config.result_yuv = 'i420' | 'i420p10' (--out_chroma: the 'i422' / 'i444' forms), and 'yuv' goes to the output through
yuv.Y4MWriter.  No scores, no images: evalrun.py has those.  The input's sampling and siting are the files' (C420mpeg2: left; C422:
left; --in_siting overrides what a file says); the output keeps both unless told otherwise, so its C tag is the input's.

A file with cuts (--scene_cut T: found from the LR stream's luma, ops.luma_sad + scene.py; --cuts: given) is run as the reference would
run its scenes as separate clips: windows clamped at the cuts, no group across one, Network.reset() and is_first_frame at each
(scene.plan_groups / scene.GroupPlanner).  With neither option the file is one clip, as before.

--in_down K (2..8) evaluates the way the paper does: every file frame is decoded once at file size (ops.yuv_to_frames) and down-scaled
once by K with the antialiased bicubic ops.resize_aa -- the 'BI' degradation that made the dataset's LRx4 folders -- and the network
runs on those frames as RGB windows (uint8 from 8-bit files: what an LRx4 PNG holds; float32 from 10-bit ones), config.input_yuv off.
--score FILE (K == config.scale) then scores every result against the LR stream's own file frame, decoded float32, on the device
(ops.score_frames): a line `frame psnr ssim` per frame and a final `mean` line.  --out_size WxH writes the result at another size:
config.result_yuv off, each group's results through ops.resize_aa and ops.result_to_yuv.  All three are off by default, and off
means the calls, the launches and the bytes of a run without them.
"""
import argparse
import collections
import sys
import time

import numpy as np
import torch

from . import metrics, scene
from .evalrun import load_checkpoint
from .yuv import (Y4MReader, Y4MWriter, check_chroma, check_matrix, check_range, check_siting, depth_of, effective_siting, resolve_input,
                  sampling_of)


def open_pair(lr_path, ref_path, siting=None):
    """The two readers of a run; ValueError (one line) unless geometry, format (sampling, depth and chroma siting) and frame count
    agree.  siting ('centre' | 'left'; --in_siting): what both files' chroma siting is taken to be, whatever their headers say."""
    lr = Y4MReader(lr_path)
    try:
        ref = Y4MReader(ref_path)
        if siting is not None:
            lr.siting, ref.siting = effective_siting(lr.fmt, siting), effective_siting(ref.fmt, siting)
    except Exception:
        lr.close()
        raise
    bad = None
    if (lr.h, lr.w) != (ref.h, ref.w):
        bad = 'geometry differs (%d x %d and %d x %d)' % (lr.h, lr.w, ref.h, ref.w)
    elif lr.fmt != ref.fmt:
        bad = 'format differs (%s and %s)' % (lr.fmt, ref.fmt)
    elif lr.siting != ref.siting:
        bad = 'format differs (%s with %s- and %s-sited chroma; --in_siting declares one for both)' % (lr.fmt, lr.siting, ref.siting)
    elif lr.length != ref.length:
        bad = 'frame count differs (%d and %d)' % (lr.length, ref.length)
    elif lr.length < 1:
        bad = 'no frames'
    if bad:
        lr.close()
        ref.close()
        raise ValueError('videorun: %s and %s: %s' % (lr_path, ref_path, bad))
    return lr, ref


def configure(config, reader):
    """The run's fields of `config` from the LR file: input_yuv (always the files' format), input_yuv_siting (the reader's: the file's,
    or open_pair's override), input_yuv_range (the file's XCOLORRANGE unless set: EVAL.input_range_set), result_yuv (by
    EVAL.video_depth; None: the input's depth -- and by EVAL.out_chroma '420' | '422' | '444'; None: the input's sampling), yuv_siting
    (EVAL.out_siting; None: 'left' for 4:2:2 output, which is what its tag means, else the input's).
    EVAL.in_down (K; None: off): input_yuv is None -- the network gets RGB windows, run() decodes and down-scales the files' frames;
    the file must be K times an even size.  EVAL.out_size ((W, H); None: off): result_yuv is None -- run() resizes and converts -- and
    the format the run would have used is left in EVAL.out_yuv (always set).  EVAL.score_file needs in_down == config.scale."""
    E = config.EVAL
    down, size, score = check_in_down(getattr(E, 'in_down', None)), check_out_size(getattr(E, 'out_size', None)), getattr(E, 'score_file', None)
    if score is not None and down != int(config.scale):
        raise ValueError('videorun: --score needs --in_down %d, the scale of the config: the result is scored against the file frame '
                         '(got --in_down %s)' % (int(config.scale), down))
    if down is not None and (reader.h % down or reader.w % down or (reader.h // down) % 2 or (reader.w // down) % 2):
        raise ValueError('videorun: --in_down %d needs frames of %d times an even size (got %d x %d)' % (down, down, reader.w, reader.h))
    if size is not None:
        rh, rw = (int(config.scale) * (v // (down or 1)) for v in (reader.h, reader.w))
        if rw > 8 * size[0] or rh > 8 * size[1]:
            raise ValueError('videorun: --out_size %dx%d is less than an eighth of the %dx%d result on an axis' % (size + (rw, rh)))
    E.in_down, E.out_size, E.score_file = down, size, score
    config.input_yuv = reader.fmt if down is None else None
    config.input_yuv_siting = reader.siting
    out = getattr(E, 'out_chroma', None) or sampling_of(reader.fmt)
    if str(out) not in ('420', '422', '444'):
        raise ValueError('videorun: --out_chroma must be 420, 422 or 444 (got %r)' % (out,))
    siting = getattr(E, 'out_siting', None) or ('left' if str(out) == '422' else reader.siting)
    try:
        config.yuv_siting = check_siting(siting)
    except ValueError:
        raise ValueError("videorun: --out_siting must be 'centre' or 'left' (got %r)" % (siting,))
    if not getattr(E, 'input_range_set', False):
        config.input_yuv_range = reader.range
    depth = getattr(E, 'video_depth', None) or depth_of(reader.fmt)
    if depth not in (8, 10):
        raise ValueError('videorun: --video_depth must be 8 or 10 (got %r)' % (depth,))
    E.out_yuv = 'i%s%s' % (out, '' if depth == 8 else 'p10')
    config.result_yuv = E.out_yuv if size is None else None
    return config


def check_in_down(k):
    """EVAL.in_down: None (off) or an integer 2..8."""
    if k is None:
        return None
    if isinstance(k, bool) or int(k) != k or not 2 <= int(k) <= 8:
        raise ValueError('videorun: --in_down must be an integer 2..8 (got %r)' % (k,))
    return int(k)


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


def run(config, lr_path, ref_path, out_path, net=None):
    """Super-resolve lr_path with ref_path into out_path; returns (frames written, seconds in the network calls).  config: a model
    config (EVAL.frame_group, frame_num, yuv_matrix / yuv_range for the output, input_yuv_matrix / input_yuv_chroma for the input);
    net: an SRNet built from that config (None: built here, EVAL.ckpt_abs_name loaded) -- its engines must not exist yet, they take
    the input format from the config at their construction.
    EVAL.scene_cut (a scene-score threshold in (0, 1]) or EVAL.cuts (frame indices in (0, n), increasing) make every scene a clip of
    its own; the cuts the run used are left in config.EVAL.scene_cuts (a tuple; empty without the options), and under scene_cut the
    seconds include the detector's upload and its ops.luma_sad call per group.
    EVAL.in_down / EVAL.score_file / EVAL.out_size: the module header; the scores are left in config.EVAL.scores, a list of (frame,
    psnr, ssim), and the seconds include the decode, the resizes and the scorer."""
    E = config.EVAL
    threshold, cuts = getattr(E, 'scene_cut', None), getattr(E, 'cuts', None)
    if threshold is not None and cuts is not None:
        raise ValueError('videorun: scene_cut and cuts exclude each other')
    if threshold is not None:
        threshold = scene.check_threshold(threshold)
    lr, ref = open_pair(lr_path, ref_path, getattr(E, 'in_siting', None))
    writer = None
    was_pipelined = None
    try:
        try:
            cuts = scene.check_cuts(cuts or (), lr.length)
        except ValueError as e:
            raise ValueError('videorun: %s (%d frames)' % (e, lr.length))
        configure(config, lr)
        if net is None:
            from . import SRNet
            net = SRNet(config).to('cuda').eval()
            if config.EVAL.ckpt_abs_name:
                load_checkpoint(net, config.EVAL.ckpt_abs_name)
        nc = net.Network.config
        if nc is not config:                              # (a caller's net may carry a config of its own)
            for k in ('input_yuv', 'input_yuv_range', 'input_yuv_siting', 'result_yuv', 'yuv_siting'):
                setattr(nc, k, getattr(config, k))
        down, size, score_file = E.in_down, E.out_size, E.score_file
        if net.Network._engines and (net.Network._engines[0].input_yuv is None) != (down is not None):
            raise RuntimeError('videorun: the network passed in already runs %s config.input_yuv; pass a fresh one' % ('with' if down else 'without'))
        if net.Network._engines and size is not None and net.Network._engines[0].result_yuv is not None:
            raise RuntimeError('videorun: the network passed in already runs with config.result_yuv; pass a fresh one')
        dev = next(net.parameters()).device
        n, t, G = lr.length, int(config.frame_num), max(1, int(getattr(config.EVAL, 'frame_group', 4) or 1))
        scale = int(config.scale)
        out_range = getattr(config, 'yuv_range', None) or 'limited'
        rh, rw = (lr.h * scale, lr.w * scale) if down is None else (lr.h // down * scale, lr.w // down * scale)
        writer = Y4MWriter(out_path, rh if size is None else size[1], rw if size is None else size[0], E.out_yuv, lr.fps, out_range, config.yuv_siting)
        scores = []
        was_pipelined = bool(getattr(nc, 'pipelined', False))
        net.Network.set_pipelined(True)
        net.Network.reset()
        held = collections.OrderedDict()                  # frame index -> (lr buffer, ref buffer): the frames the next windows read
        nread, seconds = 0, 0.0

        def read_to(upto):
            """Frames [nread, upto) of both files into `held`; the new LR buffers."""
            nonlocal nread
            new = []
            while nread < upto:
                a, b = lr.read(), ref.read()
                if a is None or b is None:
                    raise ValueError('videorun: %s: truncated file' % (lr_path if a is None else ref_path))
                held[nread] = (a, b)
                new.append(a)
                nread += 1
            return new

        small = {}                                        # --in_down: frame index -> (lr, ref) down-scaled [3, h / K, w / K] (+ the LR decode)

        def down_scaled(wins):
            """--in_down: the windows as RGB tensors [B, t, 3, h / K, w / K].  A file frame not seen yet goes to the device once, is
            decoded once at file size and resized once -- the LR and the reference frames of a call together; the LR stream's float32
            decode stays as the ground truth of --score."""
            from . import ops
            for k in [k for k in small if k not in held]:
                del small[k]
            new = sorted({i for w_ in wins for i in w_ if i not in small})
            if new:
                x = torch.from_numpy(np.stack([held[i][j] for j in (0, 1) for i in new])).to(dev)
                full = ops.yuv_to_frames(x, lr.h, lr.w, *decode)
                lo = ops.resize_aa(full, lr.h // down, lr.w // down, 'uint8' if depth_of(lr.fmt) == 8 else 'float32')
                for q, i in enumerate(new):
                    small[i] = (lo[q], lo[len(new) + q], full[q] if score_file is not None else None)
            return tuple(torch.stack([torch.stack([small[i][j] for i in w_]) for w_ in wins]) for j in (0, 1))

        if down is not None:
            r_in = resolve_input(lr.fmt, getattr(config, 'input_yuv_matrix', None), getattr(config, 'input_yuv_range', None),
                                 getattr(config, 'input_yuv_chroma', None), lr.siting)
            decode = r_in if len(r_in) == 5 else r_in + ('centre',)          # fmt, matrix, range, chroma, siting of ops.yuv_to_frames

        def detected_groups():
            """The plan under --scene_cut, group by group: the new LR frames of a group and the last one before them go to the device
            once, ONE ops.luma_sad call scores the new consecutive pairs, scene.SceneDetector turns the integers into cuts."""
            nonlocal seconds
            from . import ops
            det = scene.SceneDetector(lr.h, lr.w, depth_of(lr.fmt), threshold)
            planner = scene.GroupPlanner(n, t, G)
            last = None                                   # the LR frame ahead of the next new ones
            while not planner.done():
                new = read_to(planner.need())
                if new:
                    t0 = time.time()
                    if last is None:
                        planner.push(False)               # (frame 0 opens the first scene)
                    fr = ([] if last is None else [last]) + new
                    if len(fr) > 1:
                        x = torch.from_numpy(np.stack(fr)).to(dev)
                        for sad in ops.luma_sad(x[1:], x[:-1], lr.h, lr.w, lr.fmt).cpu().tolist():
                            planner.push(det.push(sad))
                    last = new[-1]
                    seconds += time.time() - t0
                yield planner.pop()
            found.extend(det.cuts)

        found = []
        if threshold is not None:
            groups = detected_groups()
        else:
            found.extend(cuts)
            groups = scene.plan_groups(n, t, G, cuts)
        with torch.no_grad():
            for fs, wins, first in groups:
                read_to(max(i for w_ in wins for i in w_) + 1)
                for k in [k for k in held if k < min(wins[0])]:
                    del held[k]
                t0 = time.time()
                if first and fs[0] > 0:                   # a scene is a clip of its own: the state of the last one ends here
                    net.Network.reset()
                if down is None:
                    lrs = torch.from_numpy(np.stack([np.stack([held[i][0] for i in w_]) for w_ in wins])).to(dev)
                    rfs = torch.from_numpy(np.stack([np.stack([held[i][1] for i in w_]) for w_ in wins])).to(dev)
                else:
                    lrs, rfs = down_scaled(wins)
                got = net.Network.forward_group(lrs, rfs, wins, is_first_frame=first)
                if score_file is not None:                # (the unscaled result against the LR file frame: one 16-byte row per frame)
                    from . import ops
                    sc = ops.score_frames([r[0] for r in got['result']], [small[f][2] for f in fs]).cpu().tolist()
                    scores.extend((f, metrics.psnr_from_mse(m), s_) for f, (m, s_) in zip(fs, sc))
                if size is None:
                    ys = [y[0].cpu().numpy() for y in got['yuv']]
                else:
                    from . import ops
                    ys = resized_yuv(ops, [r[0] for r in got['result']], size, E.out_yuv, getattr(config, 'yuv_matrix', None) or 'bt709', out_range,
                                     config.yuv_siting).cpu().numpy()
                seconds += time.time() - t0
                for y in ys:
                    writer.write(y)
        config.EVAL.scene_cuts = tuple(found)
        if score_file is not None:
            config.EVAL.scores = scores
            write_scores(score_file, scores)
        return writer.frames, seconds
    finally:
        lr.close()
        ref.close()
        if writer is not None:
            writer.close()
        if was_pipelined is False:
            torch.cuda.synchronize()
            net.Network.set_pipelined(False)


def resized_yuv(ops, results, size, fmt, matrix, range, siting):
    """--out_size: results [3, sh, sw] -> [B, rows, W] frames of `fmt` at size = (W, H): ops.resize_aa (clamped float32), then
    ops.result_to_yuv -- one launch each per group."""
    return ops.result_to_yuv(ops.resize_aa(results, size[1], size[0], 'float32', True), fmt, matrix, range, effective_siting(fmt, siting))


def write_scores(path, scores):
    """--score: `frame psnr ssim` per frame (repr of the float64s: they read back bit for bit), then `mean psnr ssim` -- the sums in
    frame order over the count."""
    with open(path, 'w') as f:
        for fr, p, s_ in scores:
            f.write('%d %r %r\n' % (fr, p, s_))
        k = max(len(scores), 1)
        f.write('mean %r %r\n' % (sum(p for _, p, _ in scores) / k, sum(s_ for _, _, s_ in scores) / k))


def build_config(argv=None):
    from .config import get_config
    ap = argparse.ArgumentParser(description='RefVSR on .y4m files: 4:2:0 in, 4:2:0 out (MI355X HIP path)')
    ap.add_argument('--config', '-c', type=str, default='config_RefVSR_small_L1')
    ap.add_argument('--ckpt_abs_name', '-ckpt_abs_name', type=str, default=None)
    ap.add_argument('--lr', required=True, help='the ultra-wide LR stream (.y4m: C420jpeg, C420mpeg2, C420p10, C422, C444 and their 10-bit forms)')
    ap.add_argument('--ref', required=True, help='the wide reference stream (.y4m of the same geometry, format and length)')
    ap.add_argument('--out', required=True, help='the result (.y4m)')
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
    args = ap.parse_args(argv)
    if args.scene_cut is not None and args.cuts is not None:
        raise ValueError('videorun: --scene_cut and --cuts exclude each other')
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
    E.ckpt_abs_name, E.frame_group, E.video_depth = args.ckpt_abs_name, args.frame_group, args.video_depth
    E.scene_cut, E.cuts = scene_cut, cuts
    E.in_siting, E.out_chroma, E.out_siting = args.in_siting, args.out_chroma, args.out_siting
    E.in_down, E.score_file, E.out_size = check_in_down(args.in_down), args.score, check_out_size(args.out_size)
    if E.score_file is not None and E.in_down != int(cfg.scale):
        raise ValueError('videorun: --score needs --in_down %d, the scale of the config (got --in_down %s)' % (int(cfg.scale), E.in_down))
    cfg.device, cfg.cuda = 'cuda', True
    return cfg, args


def main(argv=None):
    cfg, args = build_config(argv)
    if not cfg.EVAL.input_range_set:
        with Y4MReader(args.lr) as rd:
            cfg.yuv_range = rd.range              # (the output keeps the input's range unless --yuv_range says otherwise)
    frames, seconds = run(cfg, args.lr, args.ref, args.out)
    scenes = '' if cfg.EVAL.scene_cut is None and cfg.EVAL.cuts is None else ', %d scenes' % (len(cfg.EVAL.scene_cuts) + 1)
    print('[VIDEO %s] %d frames -> %s (%.5f sec / frame%s)' % (args.config, frames, args.out, seconds / max(frames, 1), scenes))
    return 0 if frames else 1


if __name__ == '__main__':
    sys.exit(main())
