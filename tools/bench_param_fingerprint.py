"""Cost of the weight check's pieces per parameter set (RefVSR_small, the 48-channel RefVSR and RefVSR_IR): the host walk over the
parameters' data_ptr()s and version counters (Network._weights_key), one ops.param_fingerprint call on the host (two launches), the
two kernels on the device (events around ITERS calls back to back), and one synchronous 8-byte read.  Own timing loop (bench.py
stays the yardstick and is not changed).  Under `rocprofv3 --kernel-trace --stats` the kernels' own durations come out per grid
size (tools/weight_check_ab.py reads the trace: one grid size per parameter set).

    python tools/bench_param_fingerprint.py [--out profiles/weight_check_kernel.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (('small', 'config_RefVSR_small_L1'), ('48-channel', 'config_RefVSR_L1'), ('IR', 'config_RefVSR_IR_L1'))
ITERS, PASSES = 50, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weight_check_kernel.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_param_fingerprint needs a GPU'
    from refvsr_amd import SRNet, fingerprint, get_config, make_state_dict, ops
    dev = torch.device('cuda:0')
    lines = []
    for tag, name in CONFIGS:
        cfg = get_config('p', 'm', name)
        net = SRNet(cfg).to(dev).eval()
        net.load_state_dict(make_state_dict(cfg, 1234))
        N = net.Network
        params = [p.detach() for p in N.parameters()]
        words = sum(p.numel() for p in params)
        tab = ops.FingerprintTable(params)
        out = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(3):
            ops.param_fingerprint(tab, out=out)
        torch.cuda.synchronize()
        same = int(out.item()) == fingerprint.as_int64(fingerprint.param_fingerprint_model([p.cpu().numpy() for p in params]))
        N._weights_key()
        t0 = time.perf_counter()
        for _ in range(200):
            N._weights_key()
        key_us = (time.perf_counter() - t0) / 200 * 1e6
        dev_us, host_us, read_us = [], [], []
        for _ in range(PASSES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(ITERS):
                ops.param_fingerprint(tab, out=out)
            e1.record()
            host_us.append((time.perf_counter() - t0) / ITERS * 1e6)
            e1.synchronize()
            dev_us.append(1e3 * e0.elapsed_time(e1) / ITERS)
            t0 = time.perf_counter()
            for _ in range(ITERS):
                ops.param_fingerprint(tab, out=out).item()
            read_us.append((time.perf_counter() - t0) / ITERS * 1e6)
        med = statistics.median(dev_us)
        lines.append(dict(what='%s (%s): %d tensors, %d words = %.1f MB, %d chunks' % (tag, name, len(params), words, 4e-6 * words, tab.nchunks),
                          grid=tab.nchunks, host_key_walk_us=round(key_us, 1), host_us_per_call_median=round(statistics.median(host_us), 1),
                          device_us_per_call_median=round(med, 1), device_us_per_call_all=[round(v, 1) for v in dev_us],
                          sync_call_and_read_us_median=round(statistics.median(read_us), 1),
                          gb_per_s_at_median=round(4 * words / med / 1e3, 1), equals_numpy_model=same))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('# python tools/bench_param_fingerprint.py on %s (%d calls back to back per pass, %d passes)\n'
                 % (torch.cuda.get_device_name(0), ITERS, PASSES))
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')
            print(json.dumps(dict(tool='bench_param_fingerprint', **ln)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
