"""A/B of config.weight_precision ('hi_lo' vs 'fp16') on the flagship workload shape: RefVSR_small_L1 at 270 x 480, t = 5,
pipelined, forward_group of 4 windows, inputs resident on the device.  Own timing loop (bench.py stays the yardstick of the
default): the two modes are timed interleaved, REPS passes each, median frames/s reported.  One JSON line per mode on stdout.

    python tools/bench_weight_precision.py [--frames 64] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(mode, dev):
    from refvsr_amd import SRNet, get_config, make_state_dict
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.save_sample = 5, False
    cfg.weight_precision = mode
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234, variant='plausible'))
    net.Network.set_pipelined(True)
    return net


def one_pass(net, lr, rf, wins, G):
    """First window per-frame, then the rest as forward_group calls of G windows; returns frames/s of the grouped part."""
    net.Network.reset()
    with torch.no_grad():
        net(lr[wins[0]][None], rf[wins[0]][None], True, frame_ids=wins[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for i in range(1, len(wins) - G + 1, G):
            ws = wins[i:i + G]
            net.forward_group(torch.stack([lr[w] for w in ws], 0), torch.stack([rf[w] for w in ws], 0), ws)
            n += G
        torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=65)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--group', type=int, default=4)
    ap.add_argument('--modes', default='hi_lo,fp16')
    a = ap.parse_args()
    from refvsr_amd.synth import make_clip, window_indices
    dev = torch.device('cuda:0')
    lr, rf, _ = make_clip(a.frames, 270, 480, seed=0, want_gt=False)
    lr, rf = lr.to(dev), rf.to(dev)
    wins = [window_indices(f, a.frames, 5) for f in range(a.frames)]
    modes = a.modes.split(',')
    nets = {m: build(m, dev) for m in modes}
    for m in modes:                                  # warm-up: kernels loaded, allocator primed
        one_pass(nets[m], lr, rf, wins[:1 + 2 * a.group], a.group)
    fps = {m: [] for m in modes}
    for _ in range(a.reps):
        for m in modes:
            fps[m].append(one_pass(nets[m], lr, rf, wins, a.group))
    for m in modes:
        print(json.dumps(dict(tool='bench_weight_precision', weight_precision=m, size='270x480', t=5, group=a.group,
                              frames=a.frames, reps=a.reps, fps_median=round(statistics.median(fps[m]), 2),
                              fps_all=[round(v, 2) for v in fps[m]])))
    if len(modes) == 2:
        print(json.dumps(dict(tool='bench_weight_precision', ratio='%s/%s' % (modes[1], modes[0]),
                              value=round(statistics.median(fps[modes[1]]) / statistics.median(fps[modes[0]]), 4))))


if __name__ == '__main__':
    main()
