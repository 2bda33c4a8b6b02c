#!/usr/bin/env python3
"""Where videorun's wall time goes: whole-run wall seconds per frame of videorun.run() -- open, read, upload, network, read-back, write,
close -- on one synthetic 544 x 960 8-bit 4:2:0 pair (config_RefVSR_small_L1, t = 5, groups of 4; the result is 2176 x 3840), the
files in --dir (a memory file system: the disk is not what is measured), alternating passes of

  --io sync                      the loop that reads, runs and writes one after the other
  --io stream                    reader and writer threads around the calls, every file frame uploaded once
  --io stream --out /dev/null    the same with nothing to write

one network for all of them (run() resets it), one warm-up pass first.  Beside the wall figures: the sync loop's own clock (its
network-call section) and the stream loop's config.EVAL.io_stats.  No bar: the report states what was measured.

Usage: tools/bench_videorun_io.py [--frames 64] [--passes 3] [--dir /dev/shm] [--io_depth 2] [--out FILE]"""
import argparse
import gc
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from refvsr_amd import yuv  # noqa: E402

_out = []


def say(line=''):
    print(line, flush=True)
    _out.append(line)


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--dir', default='/dev/shm', help='where the .y4m files go (removed afterwards)')
    ap.add_argument('--io_depth', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    from refvsr_amd import SRNet, get_config, make_state_dict, videorun
    from refvsr_amd.synth import make_clip
    dev = torch.device('cuda:0')
    nfr, t, G, h, w, name = args.frames, 5, 4, 544, 960, 'config_RefVSR_small_L1'
    say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    say('videorun.run(), %d x %d i420 pair -> %d x %d i420, %d frames (8 synthetic frames repeated), %s, t = %d, groups of %d, io_depth %d, '
        'files in %s: whole-run wall seconds per frame, %d alternating passes after a warm-up pass'
        % (h, w, 4 * h, 4 * w, nfr, name, t, G, args.io_depth, args.dir, args.passes))
    tmp = tempfile.mkdtemp(dir=args.dir, prefix='videorun_io_')
    try:
        lr, rf, _ = make_clip(8, h, w, seed=3, want_gt=False)
        paths = []
        for tag, x in (('uw', lr), ('w', rf)):
            paths.append(os.path.join(tmp, tag + '.y4m'))
            ys = yuv.rgb_to_yuv420(x.numpy(), 'i420', 'bt709', 'limited')
            with yuv.Y4MWriter(paths[-1], h, w, 'i420', (24, 1), 'limited') as wr:
                for k in range(nfr):
                    wr.write(ys[k % 8])
        out = os.path.join(tmp, 'sr.y4m')
        variants = (('--io sync                  ', dict(io='sync'), out), ('--io stream                ', dict(io='stream'), out),
                    ('--io stream --out /dev/null', dict(io='stream'), '/dev/null'))
        cfg0 = get_config('p', 'm', name)
        cfg0.frame_num, cfg0.save_sample = t, False
        net = SRNet(cfg0).to(dev).eval()
        net.load_state_dict(make_state_dict(cfg0, 1234))
        wall, own, stats, sizes = dict((k, []) for k, _, _ in variants), [], dict((k, []) for k, _, _ in variants), {}
        for p in range(args.passes + 1):                              # (pass 0 warms up: engine, allocator, page cache)
            for key, kw, dst in variants:
                cfg = get_config('p', 'm', name)
                cfg.frame_num, cfg.save_sample = t, False
                cfg.EVAL.frame_group, cfg.EVAL.io_depth, cfg.EVAL.io_timeout = G, args.io_depth, 60
                for k, v in kw.items():
                    setattr(cfg.EVAL, k, v)
                gc.collect()
                torch.cuda.synchronize()
                t0 = time.time()
                n, s = videorun.run(cfg, paths[0], paths[1], dst, net=net)
                torch.cuda.synchronize()
                dt = time.time() - t0
                assert n == nfr
                if dst == out:
                    sizes[key] = os.path.getsize(out)
                    os.remove(out)
                if p:
                    wall[key].append(dt / n)
                    if kw['io'] == 'sync':
                        own.append(s / n)
                    else:
                        stats[key].append(cfg.EVAL.io_stats)
        assert len(set(sizes.values())) == 1
        say('input %.1f MB per stream, output %.1f MB' % (os.path.getsize(paths[0]) / 1e6, list(sizes.values())[0] / 1e6))
        for key, _, _ in variants:
            say('wall sec / frame  %s  %s  median %.4f' % (key, ' '.join('%.4f' % x for x in wall[key]), med(wall[key])))
        say('the sync loop\'s own clock (upload, network calls, read-back; no file reads or writes)  %s  median %.4f sec / frame'
            % (' '.join('%.4f' % x for x in own), med(own)))
        for key, _, _ in variants:
            for st in stats[key]:
                say('io_stats  %s  frames %d uploads %d groups %d max_in_flight %d max_held %d | of %.3f s wall the caller waited %.3f s for '
                    'reads, %.3f s for the device, %.3f s for writes' % (key, st['frames'], st['uploads'], st['groups'], st['max_in_flight'],
                                                                         st['max_held'], st['wall'], st['read_wait'], st['device_wait'], st['write_wait']))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(_out) + '\n')


if __name__ == '__main__':
    main()
