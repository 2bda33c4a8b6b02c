"""A/B of 8-bit input frames (uint8, converted on the device by refvsr_ingest_u8) against float32 input frames.  Own timing loops
(bench.py stays the yardstick and is not changed; its PCIe-inclusive loader is reused as it is).  Every A/B is interleaved, REPS
passes each, median reported.  Writes the report to --out (default profiles/r08_input_u8_ab.txt) and one JSON line per
measurement on stdout.

  kernel    refvsr_ingest_u8 on one window (t = 5, LR + ref = 10 frames, one launch) at 270 x 480 and 1080 x 1920, planar and
            channels-last sources, GB/s (bytes read + written) against the HBM roof; the fp32 clone it replaces alongside
  group     configs[1] (RefVSR_small_L1, 270 x 480, t = 5), forward_group of 4 windows, pipelined: inputs resident on the device
  pcie      the same with pinned host windows copied on a copy stream, double-buffered (bench.py:pcie_inclusive_pass): whole windows
            and frames_once
  8k        configs[4] (RefVSR_MFID_8K, 1080 x 1920, t = 7), one forward() per frame, PCIe-inclusive
  loader    evalrun's host loader (ClipSet.__getitem__: PNG decode + conversion) per output frame, tools/make_synth_dataset.py data

    python tools/bench_input_u8.py [--reps 5] [--skip 8k,loader]
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

HBM_TBPS = 8.0          # MI355X HBM3E peak


def med(v):
    return statistics.median(v)


def kernel_leg(reps, lines, dev):
    from refvsr_amd import ops
    for h, w in ((270, 480), (1080, 1920)):
        fb = 3 * h * w
        raw = torch.randint(0, 256, (2, 5, fb), dtype=torch.uint8, device=dev)
        src = {'planar': [raw[i, j].view(3, h, w) for i in range(2) for j in range(5)],
               'hwc': [raw[i, j].view(h, w, 3).permute(2, 0, 1) for i in range(2) for j in range(5)]}
        dst = [torch.empty((3, h, w), dtype=torch.float32, device=dev) for _ in range(10)]
        f32 = torch.rand((10, 3, h, w), device=dev)
        iters = 200 if h < 1080 else 40

        def t_ingest(lay):
            pairs = list(zip(src[lay], dst))
            ops.ingest_u8(pairs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                ops.ingest_u8(pairs)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        def t_clone():
            [f32[i].clone() for i in range(10)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                for i in range(10):
                    f32[i].clone()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        ms = {'planar': [], 'hwc': [], 'clone': []}
        for _ in range(reps):
            ms['planar'].append(t_ingest('planar'))
            ms['hwc'].append(t_ingest('hwc'))
            ms['clone'].append(t_clone())
        for k, v in ms.items():
            nbytes = 10 * fb * (5 if k != 'clone' else 8)
            m = med(v)
            gbs = nbytes / (m * 1e-3) / 1e9
            lines.append(dict(leg='kernel', what='ingest_u8 ' + k if k != 'clone' else 'fp32 clone x10 (replaced)', size='%dx%d' % (h, w),
                              frames=10, ms=round(m, 4), us_all=[round(1e3 * x, 1) for x in v], GBps=round(gbs, 1),
                              pct_hbm_roof=round(100 * gbs / (HBM_TBPS * 1e3), 1)))


def _net(name, t, dev):
    from refvsr_amd import SRNet, get_config, make_state_dict
    cfg = get_config('p', 'm', name)
    cfg.frame_num, cfg.save_sample = t, False
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234, variant='plausible'))
    net.Network.set_pipelined(True)
    return net


def _bytes(x):
    return torch.round(x * 255.0).to(torch.uint8)


def group_leg(reps, lines, dev, frames=65, G=4):
    from refvsr_amd.synth import make_clip, window_indices
    lr, rf, _ = make_clip(17, 270, 480, seed=0, want_gt=False)              # (17 distinct frames, cycled: the cache is keyed by id)
    cyc = [k % 17 for k in range(frames)]
    lr, rf = lr[cyc], rf[cyc]
    wins = [window_indices(f, frames, 5) for f in range(frames)]
    data = {'float32': (lr.to(dev), rf.to(dev)), 'uint8': (_bytes(lr).to(dev), _bytes(rf).to(dev))}
    nets = {k: _net('config_RefVSR_small_L1', 5, dev) for k in data}

    def one_pass(k, ws_all):
        net, (a, b) = nets[k], data[k]
        net.Network.reset()
        with torch.no_grad():
            net(a[ws_all[0]][None], b[ws_all[0]][None], True, frame_ids=ws_all[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for i in range(1, len(ws_all) - G + 1, G):
                ws = ws_all[i:i + G]
                net.forward_group(torch.stack([a[w] for w in ws], 0), torch.stack([b[w] for w in ws], 0), ws)
                n += G
            torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for k in data:
        one_pass(k, wins[:1 + 2 * G])
    fps = {k: [] for k in data}
    for _ in range(reps):
        for k in data:
            fps[k].append(one_pass(k, wins))
    for k in data:
        lines.append(dict(leg='group', config='configs[1] RefVSR_small_L1 270x480 t=5', group=G, input_dtype=k, inputs='resident',
                          fps_median=round(med(fps[k]), 2), fps_all=[round(v, 2) for v in fps[k]]))
    # PCIe-inclusive: bench.py's loader (pinned host windows, copy stream, double-buffered), whole windows and frames_once
    import bench
    args = argparse.Namespace(warmup=4, steps=60)
    nfr = args.warmup + args.steps
    all_w = [window_indices(f, nfr, 5) for f in range(nfr)]
    host = {'float32': (torch.stack([lr[w] for w in all_w]), torch.stack([rf[w] for w in all_w]))}
    host['uint8'] = (_bytes(host['float32'][0]), _bytes(host['float32'][1]))
    for once in (False, True):
        res = {k: [] for k in host}
        for _ in range(max(1, reps // 2)):
            for k in host:
                r = bench.pcie_inclusive_pass(nets[k], args, host[k][0], host[k][1], all_w, 0, G, dev, passes=2, frames_once=once)
                res[k] += r['samples']
        for k in host:
            per = host[k][0][0, 0].numel() * host[k][0].element_size() * 2 / 1e6
            lines.append(dict(leg='pcie', config='configs[1] RefVSR_small_L1 270x480 t=5', group=G, input_dtype=k,
                              loader='frames_once' if once else 'whole windows',
                              h2d_mb_per_frame=round(per * (1 if once else 5), 2), fps_median=round(med(res[k]), 2),
                              fps_all=[round(v, 2) for v in res[k]]))
    del nets


def eightk_leg(reps, lines, dev):
    import bench
    from refvsr_amd.synth import make_clip, window_indices
    args = argparse.Namespace(warmup=2, steps=8)
    nfr = args.warmup + args.steps
    lr, rf, _ = make_clip(nfr, 270, 480, seed=0, want_gt=False)            # (content: a 270p clip upsampled, cheap to make)
    up = lambda x: torch.nn.functional.interpolate(x, size=(1080, 1920), mode='bilinear', align_corners=False).clamp(0, 1)
    lr, rf = up(lr), up(rf)
    all_w = [window_indices(f, nfr, 7) for f in range(nfr)]
    host = {'float32': (torch.stack([lr[w] for w in all_w]), torch.stack([rf[w] for w in all_w]))}
    del lr, rf
    host['uint8'] = (_bytes(host['float32'][0]), _bytes(host['float32'][1]))
    nets = {k: _net('config_RefVSR_MFID_8K', 7, dev) for k in host}
    res = {k: [] for k in host}
    for _ in range(max(1, reps // 2)):
        for k in host:
            r = bench.pcie_inclusive_pass(nets[k], args, host[k][0], host[k][1], all_w, 0, 1, dev, passes=2)
            res[k] += r['samples']
    for k in host:
        per = host[k][0][0].numel() * host[k][0].element_size() * 2 / 1e6
        lines.append(dict(leg='8k', config='configs[4] RefVSR_MFID_8K 1080x1920 t=7', calls='one forward() per frame', input_dtype=k,
                          loader='whole windows', h2d_mb_per_frame=round(per, 1), fps_median=round(med(res[k]), 3),
                          fps_all=[round(v, 3) for v in res[k]]))


def loader_leg(reps, lines):
    import make_synth_dataset
    from refvsr_amd import evalrun
    root = tempfile.mkdtemp(prefix='u8ds_')
    make_synth_dataset.make(root, clips=1, frames=12, h=270, w=480)
    ms = {'float32': [], 'uint8': []}
    for _ in range(reps):
        for k in ms:
            cfg = evalrun.build_config(['--config', 'config_RefVSR_small_L1', '--mode', 'bench', '--data_offset', root, '--output_offset',
                                        os.path.join(root, 'o'), '--frame_num', '5', '--input_dtype', k])
            ds = evalrun.ClipSet(cfg)
            t0 = time.perf_counter()
            for i in range(len(ds)):
                it = ds[i]
                it['LR_UW'].contiguous() if k == 'float32' else it['LR_UW']
            ms[k].append(1e3 * (time.perf_counter() - t0) / len(ds))
    for k in ms:
        lines.append(dict(leg='loader', what='evalrun.ClipSet item (PNG decode + window stack, clip cache as in evaluate)', size='270x480',
                          input_dtype=k, ms_per_frame_median=round(med(ms[k]), 3), ms_all=[round(v, 3) for v in ms[k]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_input_u8_ab.txt'))
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(',') if x)
    dev = torch.device('cuda:0')
    lines = []
    legs = [('kernel', lambda: kernel_leg(a.reps, lines, dev)), ('group', lambda: group_leg(a.reps, lines, dev)),
            ('8k', lambda: eightk_leg(a.reps, lines, dev)), ('loader', lambda: loader_leg(a.reps, lines))]
    done = []
    for name, fn in legs:
        if name in skip:
            continue
        n0 = len(lines)
        fn()
        done.append(name)
        for ln in lines[n0:]:
            print(json.dumps(dict(tool='bench_input_u8', **ln)), flush=True)
    with open(a.out, 'w') as fh:
        fh.write('# tools/bench_input_u8.py --reps %d on %s; legs measured: %s; skipped: %s\n'
                 % (a.reps, torch.cuda.get_device_name(0), ','.join(done), ','.join(sorted(skip)) or 'none'))
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
