"""Timing of refvsr_score_regions (the FOV evaluation's rectangle sums) beside refvsr_score_frames on the same tensors, beside the float64
host path, and inside a whole evaluate() call.  Own timing loop (bench.py stays the yardstick and is not changed).

  kernel    one launch pair (tile + finish) for 4 frames of 1080 x 1920, uint8 result + uint8 channels-last ground truth, the seven FOV
            rectangles; device events around ITERS launches back to back, the two scorers alternated PASSES times, median over passes
  host      metrics.fov_scores_host on one such frame (one run after one warm-up run, host clock)
  evaluate  a synthetic 270 x 480 -> 1080 x 1920 dataset (tools/make_synth_dataset.py), RefVSR_small_L1 with seeded weights,
            --metrics device --quantitative_only --frame_group 4: `--eval_mode quan_FOV` against `--eval_mode qual_quan`, alternated REPS
            times in one process; wall-clock time of the whole evaluate() call over its frames

Writes the report to --out and one JSON line per measurement on stdout.

    python tools/bench_score_regions.py [--reps 3] [--out profiles/score_regions_timing.txt]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

H, W, FRAMES = 1080, 1920, 4
ITERS, PASSES = 25, 7


def make_pair(n, dev):
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, generator=g)
    b = (a.int() + torch.randint(-6, 7, (n, 3, H, W), generator=g)).clamp(0, 255).to(torch.uint8)
    return a.to(dev), b.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).to(dev)


def kernel_leg(lines, dev):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects
    a, b = make_pair(FRAMES, dev)
    rects = fov_rects(H, W)
    legs = {'score_regions (7 FOV rectangles)': lambda: ops.score_regions(a, b, rects), 'score_frames': lambda: ops.score_frames(a, b)}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(PASSES):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / ITERS)
    med = {k: statistics.median(v) for k, v in us.items()}
    for k in legs:
        lines.append(dict(leg='kernel', what='%s: tile + finish launches, device events around %d launches, %d alternated passes' % (k, ITERS, PASSES),
                          inputs='uint8 + uint8 hwc', frames_per_launch=FRAMES, us_per_launch_median=round(med[k], 1),
                          us_per_frame_median=round(med[k] / FRAMES, 1), us_per_launch_all=[round(v, 1) for v in us[k]]))
    k0, k1 = list(legs)
    lines.append(dict(leg='kernel', what='score_regions / score_frames, medians', ratio=round(med[k0] / med[k1], 2),
                      difference_us_per_frame=round((med[k0] - med[k1]) / FRAMES, 1)))


def host_leg(lines, dev):
    from refvsr_amd.metrics import fov_scores_host
    a, b = (x[0].cpu().float() / 255.0 for x in make_pair(1, dev))
    fov_scores_host(a[:, :64, :64], b[:, :64, :64])
    t0 = time.perf_counter()
    fov_scores_host(a, b)
    lines.append(dict(leg='host', what='metrics.fov_scores_host, one 1080 x 1920 frame, float64 numpy, one run', seconds=round(time.perf_counter() - t0, 3)))


def eval_leg(reps, lines, clips, frames):
    import make_synth_dataset
    from refvsr_amd import SRNet, evalrun, get_config, make_state_dict
    root = tempfile.mkdtemp(prefix='evalfov_')
    make_synth_dataset.make(root, clips=clips, frames=frames, h=270, w=480)
    ck = os.path.join(root, 'RefVSR_small_L1.pytorch')
    torch.save(make_state_dict(get_config('p', 'm', 'config_RefVSR_small_L1'), 1234, variant='plausible'), ck)

    def one(eval_mode, tag):
        cfg = evalrun.build_config(['--config', 'config_RefVSR_small_L1', '--mode', 'bench', '--data_offset', root, '--output_offset',
                                    os.path.join(root, 'o_' + tag), '--frame_num', '5', '--ckpt_abs_name', ck, '--quantitative_only',
                                    '--frame_group', '4', '--metrics', 'device', '--eval_mode', eval_mode])
        net = SRNet(cfg).to('cuda').eval()
        evalrun.load_checkpoint(net, ck)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evalrun.evaluate(cfg, net=net, log=lambda *_: None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / res['frames'], res

    one('quan_FOV', 'warm')                                   # code objects, allocator, the loader's first touch of the files
    per = {'qual_quan': [], 'quan_FOV': []}
    psnr = {}
    for r in range(reps):
        for mode in per:
            s, res = one(mode, '%s%d' % (mode, r))
            per[mode].append(s)
            psnr[mode] = res['psnr']
    for mode in per:
        lines.append(dict(leg='evaluate', eval_mode=mode, metrics='device', dataset='%d clips x %d frames 270x480 -> 1080x1920' % (clips, frames),
                          frame_group=4, ms_per_frame_all=[round(1e3 * v, 2) for v in per[mode]]))
    lines.append(dict(leg='evaluate', what='quan_FOV - qual_quan per alternation', ms_per_frame_all=[round(1e3 * (f - q), 2) for q, f in zip(per['qual_quan'], per['quan_FOV'])],
                      max_abs_dpsnr_db_of_the_frame_lines=max(abs(p - q) for p, q in zip(psnr['qual_quan'], psnr['quan_FOV']))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--clips', type=int, default=2)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--skip', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_regions_timing.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_score_regions needs a GPU'
    dev = torch.device('cuda:0')
    lines = []
    if 'kernel' not in a.skip:
        kernel_leg(lines, dev)
    if 'host' not in a.skip:
        host_leg(lines, dev)
    if 'evaluate' not in a.skip:
        eval_leg(a.reps, lines, a.clips, a.frames)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('# python tools/bench_score_regions.py --reps %d --clips %d --frames %d on %s\n' % (a.reps, a.clips, a.frames, torch.cuda.get_device_name(0)))
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
            print(json.dumps(dict(tool='bench_score_regions', **ln)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
