"""A/B of `evalrun --metrics host` against `--metrics device` (refvsr_score_frames) on a whole evaluate() call.  Own timing loop (bench.py
stays the yardstick and is not changed).  A synthetic 270 x 480 -> 1080 x 1920 dataset (2 clips x 16 frames, tools/make_synth_dataset.py),
RefVSR_small_L1 with seeded weights, --quantitative_only --frame_group 4; the modes are alternated REPS times in one process and the
figure is the wall-clock time of the whole evaluate() call over its frames (NOT the score file's per-frame seconds: evalrun stops that
clock before it scores).  A third leg, `skip`, is the device loop with the scorer's launches replaced by zeros (a switch local to this
tool; the ground-truth upload and the 16-byte copy remain), so device - skip is the cost of the two kernels in the loop.  Also times
the kernel alone with device events (1 and 4 frames per launch, fp32 + fp32 and uint8 + uint8 channels-last) beside its HBM floor and
fp64 operation count (refvsr_amd/flops.py:score_frames_flop).  Writes the report to --out and one JSON line per measurement on stdout.

The `hd` leg is the same for the flag_HD_in configs (refvsr_score_frames_down: ground truth 1080 x 1920, result 4320 x 7680 made on the
device, factor 4): device events around the fused scorer for 1 and 4 frames per launch beside the bytes it must read; the fused scores
against refvsr_score_frames on torch's own GPU F.interpolate of the same frame, at the model-against-torch bars of
tests/test_score_down.py (the only check at the full 8K size: the suite allocates no such frame); and the wall-clock time per frame of
evaluate() on RefVSR_small_MFID_8K with --metrics host and --metrics device, alternated.  A failed comparison fails the tool.

    python tools/bench_eval_metrics.py [--reps 3] [--out profiles/score_frames.txt] [--skip kernel,evaluate,hd]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM_SPEC_TBPS, HBM_MEASURED_TBPS = 8.0, 6.29          # MI355X: data sheet / a float4 copy


def eval_leg(reps, lines, clips, frames):
    import make_synth_dataset
    from refvsr_amd import SRNet, evalrun, get_config, make_state_dict, ops
    root = tempfile.mkdtemp(prefix='evalmetrics_')
    make_synth_dataset.make(root, clips=clips, frames=frames, h=270, w=480)
    ck = os.path.join(root, 'RefVSR_small_L1.pytorch')
    torch.save(make_state_dict(get_config('p', 'm', 'config_RefVSR_small_L1'), 1234, variant='plausible'), ck)
    real_score = ops.score_frames

    def one(mode, tag):
        cfg = evalrun.build_config(['--config', 'config_RefVSR_small_L1', '--mode', 'bench', '--data_offset', root, '--output_offset',
                                    os.path.join(root, 'o_' + tag), '--frame_num', '5', '--ckpt_abs_name', ck, '--quantitative_only',
                                    '--frame_group', '4', '--metrics', 'host' if mode == 'host' else 'device'])
        net = SRNet(cfg).to('cuda').eval()
        evalrun.load_checkpoint(net, ck)
        if mode == 'skip':
            ops.score_frames = lambda outs, gts, win=7, down=1: torch.zeros((len(outs), 2), dtype=torch.float64, device=outs[0].device)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evalrun.evaluate(cfg, net=net, log=lambda *_: None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            ops.score_frames = real_score
        return dt / res['frames'], res

    one('device', 'warm')                                     # code objects, allocator, the loader's first touch of the files
    per = {'host': [], 'device': [], 'skip': []}
    psnr = {}
    for r in range(reps):
        for mode in ('host', 'device', 'skip'):
            s, res = one(mode, '%s%d' % (mode, r))
            per[mode].append(s)
            psnr[mode] = res['psnr']
    dp = max(abs(p - q) for p, q in zip(psnr['host'], psnr['device']))
    for mode in per:
        lines.append(dict(leg='evaluate', mode=mode, dataset='%d clips x %d frames 270x480 -> 1080x1920' % (clips, frames), frame_group=4,
                          ms_per_frame_all=[round(1e3 * v, 2) for v in per[mode]]))
    wins = [d < h for h, d in zip(per['host'], per['device'])]
    lines.append(dict(leg='evaluate', what='host / device per alternation', ratio_all=[round(h / d, 2) for h, d in zip(per['host'], per['device'])],
                      device_faster_every_time=all(wins), device_minus_skip_ms_all=[round(1e3 * (d - s), 2) for d, s in zip(per['device'], per['skip'])],
                      max_abs_dpsnr_db=dp))
    return all(wins)


def kernel_leg(lines, dev):
    from refvsr_amd import flops, ops
    h, w = 1080, 1920
    g = torch.Generator().manual_seed(0)
    for name, mk in (('fp32 + fp32', lambda n: (torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g))),
                     ('uint8 + uint8 hwc', lambda n: (torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=g),
                                                      torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g).permute(0, 3, 1, 2)))):
        for n in (1, 4):
            a, b = (x.to(dev) for x in mk(n))
            for _ in range(3):
                ops.score_frames(a, b)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            iters = 50
            e0.record()
            for _ in range(iters):
                ops.score_frames(a, b)
            e1.record()
            e1.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / iters
            nbytes = n * 3 * h * w * (a.element_size() + b.element_size())
            lines.append(dict(leg='kernel', what='score_frames (tile + finish launches, device events, %d calls back to back)' % iters, inputs=name,
                              frames_per_launch=n, us_per_launch=round(us, 1), us_per_frame=round(us / n, 1), algorithmic_MB=round(nbytes / 1e6, 1),
                              hbm_floor_us_spec=round(nbytes / (HBM_SPEC_TBPS * 1e6), 1), hbm_floor_us_measured_bw=round(nbytes / (HBM_MEASURED_TBPS * 1e6), 1),
                              fp64_GFLOP=round(n * flops.score_frames_flop(h, w) / 1e9, 3),
                              fp64_TFLOPs_achieved=round(n * flops.score_frames_flop(h, w) / (us * 1e-6) / 1e12, 2)))


def hd_leg(reps, lines, dev, frames):
    import make_synth_dataset
    import torch.nn.functional as F
    from refvsr_amd import SRNet, evalrun, get_config, make_state_dict, ops
    from refvsr_amd.metrics import psnr_from_mse
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_score_down import PSNR_BAR, SSIM_BAR          # model against torch, measured on the CPU: the bars of this comparison
    h, w, s = 1080, 1920, 4
    g = torch.Generator().manual_seed(0)
    gt = torch.randint(0, 256, (4, h, w, 3), dtype=torch.uint8, generator=g).permute(0, 3, 1, 2).to(dev)
    up = F.interpolate((gt.float() / 255.0).contiguous(), scale_factor=s, mode='bicubic', align_corners=False)
    big = (up + 0.03 * torch.randn(up.shape, device=dev)).clamp_(0, 1).contiguous()          # [4, 3, 4320, 7680] float32, made where it is scored
    del up
    ok = True
    for n in (1, 4):
        a, b = big[:n], gt[:n]
        for _ in range(3):
            ops.score_frames(a, b, down=s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters = 20
        e0.record()
        for _ in range(iters):
            ops.score_frames(a, b, down=s)
        e1.record()
        e1.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / iters
        nbytes = n * 3 * h * w * (s * s * a.element_size() + b.element_size())
        lines.append(dict(leg='hd kernel', what='score_frames(down=4) (tile + finish launches, device events, %d calls back to back)' % iters,
                          inputs='fp32 4320x7680 + uint8 hwc 1080x1920', frames_per_launch=n, us_per_launch=round(us, 1), us_per_frame=round(us / n, 1),
                          algorithmic_MB=round(nbytes / 1e6, 1), effective_TBps=round(nbytes / (us * 1e-6) / 1e12, 3),
                          hbm_floor_us_spec=round(nbytes / (HBM_SPEC_TBPS * 1e6), 1), hbm_floor_us_measured_bw=round(nbytes / (HBM_MEASURED_TBPS * 1e6), 1)))
    fused = ops.score_frames(big, gt, down=s).cpu()
    for i in range(big.shape[0]):
        d = F.interpolate(big[i:i + 1], scale_factor=1.0 / s, mode='bicubic', align_corners=False)
        two = torch.stack([ops.score_frames(d.clamp(0, 1), gt[i:i + 1], win=0)[0, 0], ops.score_frames(d, gt[i:i + 1])[0, 1]]).cpu()
        dp = abs(psnr_from_mse(fused[i, 0]) - psnr_from_mse(two[0]))
        ds = abs(float(fused[i, 1]) - float(two[1]))
        good = dp <= PSNR_BAR and ds <= SSIM_BAR
        ok = ok and good
        lines.append(dict(leg='hd check', what='fused down=4 scorer against score_frames on torch GPU F.interpolate(bicubic) of the same 8K frame',
                          frame=i, psnr_db=round(psnr_from_mse(fused[i, 0]), 6), ssim=round(float(fused[i, 1]), 9), abs_dpsnr_db=dp, abs_dssim=ds,
                          bars=[PSNR_BAR, SSIM_BAR], within_bars=good))
    del big, gt, d
    torch.cuda.empty_cache()
    print('# hd: kernel leg and 8K comparison done, writing the 1080 x 1920 dataset', file=sys.stderr, flush=True)

    name = 'config_RefVSR_small_MFID_8K'
    root = tempfile.mkdtemp(prefix='evalmetrics_hd_')
    make_synth_dataset.make(root, hd=True, clips=1, frames=frames, h=h, w=w)
    ck = os.path.join(root, 'RefVSR_small_MFID_8K.pytorch')
    torch.save(make_state_dict(get_config('p', 'm', name), 1234, variant='plausible'), ck)

    def one(mode, tag):
        cfg = evalrun.build_config(['--config', name, '--mode', 'bench', '--data_offset', root, '--output_offset', os.path.join(root, 'o_' + tag),
                                    '--frame_num', '3', '--ckpt_abs_name', ck, '--quantitative_only', '--frame_group', '4', '--metrics', mode])
        net = SRNet(cfg).to('cuda').eval()
        evalrun.load_checkpoint(net, ck)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evalrun.evaluate(cfg, net=net, log=lambda *_: None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / res['frames'], res

    one('device', 'warm')
    per, got = {'host': [], 'device': []}, {}
    for r in range(reps):
        for mode in ('host', 'device'):
            t, got[mode] = one(mode, '%s%d' % (mode, r))
            per[mode].append(t)
            print('# hd: evaluate %s %d: %.3f s per frame' % (mode, r, t), file=sys.stderr, flush=True)
    for mode in per:
        lines.append(dict(leg='hd evaluate', mode=mode, config=name, dataset='1 clip x %d frames 1080x1920 -> 4320x7680' % frames, frame_group=4,
                          s_per_frame_all=[round(v, 3) for v in per[mode]]))
    dp = max(abs(p - q) for p, q in zip(got['host']['psnr'], got['device']['psnr']))
    ds = max(abs(p - q) for p, q in zip(got['host']['ssim'], got['device']['ssim']))
    lines.append(dict(leg='hd evaluate', what='host / device per alternation', ratio_all=[round(a / b, 2) for a, b in zip(per['host'], per['device'])],
                      max_abs_dpsnr_db=dp, max_abs_dssim=ds, psnr=[round(v, 5) for v in got['device']['psnr']],
                      ssim=[round(v, 5) for v in got['device']['ssim']]))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--clips', type=int, default=2)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--hd_frames', type=int, default=5)
    ap.add_argument('--skip', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_frames.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines, ok = [], True
    if 'kernel' not in a.skip:
        kernel_leg(lines, dev)
    if 'evaluate' not in a.skip:
        ok = eval_leg(a.reps, lines, a.clips, a.frames)
    if 'hd' not in a.skip:
        ok = hd_leg(a.reps, lines, dev, a.hd_frames) and ok
    with open(a.out, 'w') as fh:
        fh.write('# python tools/bench_eval_metrics.py --reps %d --clips %d --frames %d --hd_frames %d --skip %r on %s\n'
                 % (a.reps, a.clips, a.frames, a.hd_frames, a.skip, torch.cuda.get_device_name(0)))
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
            print(json.dumps(dict(tool='bench_eval_metrics', **ln)), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
