"""Timing of refvsr_conf_colormap (the confidence-map images of --eval_mode quan_conf_map): one entry-point call = the min / max launch
and the paint launch for 16 maps (four maps x a frame group of four).  Own timing loop (bench.py stays the yardstick and is not
changed).  Device events around ITERS calls back to back, PASSES passes per size, median over passes; the bytes a call has to move
(two fp32 reads and one 3-byte write per pixel = 11 bytes) over that time is the achieved rate -- at these sizes the maps sit in the
caches, so it is a rate of the call, not of HBM.

Writes the report to --out and one JSON line per measurement on stdout.

    python tools/bench_conf_colormap.py [--out profiles/conf_colormap.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((270, 480), (1080, 1920))
MAPS, ITERS, PASSES = 16, 50, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conf_colormap.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_conf_colormap needs a GPU'
    from refvsr_amd import metrics, ops
    dev = torch.device('cuda:0')
    lines = []
    for h, w in SIZES:
        g = torch.Generator().manual_seed(h)
        maps = [(torch.rand(1, h, w, generator=g) * (1.0 + k) - 0.25 * k).to(dev) for k in range(MAPS)]
        for _ in range(3):
            outs = ops.conf_colormap(maps)
        torch.cuda.synchronize()
        same = bool((outs[3].cpu().numpy() == metrics.conf_colormap_model(maps[3])).all())
        us = []
        for _ in range(PASSES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                ops.conf_colormap(maps)
            e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / ITERS)
        med = statistics.median(us)
        nbytes = MAPS * h * w * 11
        lines.append(dict(what='ops.conf_colormap: %d maps of %d x %d per call (two launches + %d output allocations), device events around %d '
                               'calls, %d passes' % (MAPS, h, w, MAPS, ITERS, PASSES),
                          us_per_call_median=round(med, 1), us_per_map_median=round(med / MAPS, 2), us_per_call_all=[round(v, 1) for v in us],
                          bytes_per_call=nbytes, gb_per_s_at_median=round(nbytes / med / 1e3, 1), equals_numpy_model=same))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('# python tools/bench_conf_colormap.py on %s\n' % torch.cuda.get_device_name(0))
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
            print(json.dumps(dict(tool='bench_conf_colormap', **ln)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
