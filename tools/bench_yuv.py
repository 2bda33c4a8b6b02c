#!/usr/bin/env python3
"""Y'CbCr 4:2:0 result frames (refvsr_result_to_yuv420, config.result_yuv) on the GPU, in one command:

  1. the kernel alone: 1080 x 1920 and 4320 x 7680, 'nv12' and 'p010', from a float32 planar and a uint8 channels-last result.  Device
     events around LAUNCHES launches, median of REPEATS repeats after warm-up.  Two columns: 'rotated' walks source and destination
     buffers through a set larger than the 256 MB Infinity Cache (every launch reads from HBM), 'hot' re-uses one buffer (the
     in-pipeline case: the output head has just written the frame).  us per launch and TB/s over the algorithmic bytes (source read
     once, frame written once).
     Yardstick, alternating with it in the same repeats on the same frames: refvsr_convert_result_hwc (float32 planar -> uint8
     channels-last), which reads the same float32 frame and writes twice the bytes.  Bar: the float32-planar conversion takes at most
     1.25 x the yardstick's time (printed per line as ok / MISSES);
  2. in the frame: frames/s of forward_group (four windows, pipelined, config_RefVSR_small_L1, 270 x 480 -> 1080 x 1920, uint8
     channels-last results) with result_yuv = 'nv12' against None, alternating passes in one process; then the same with the
     consumer's copy included -- 'yuv' copied to pinned host memory per group against the uint8 'result' copied there.  No bar.

  3. --ab DIR: no GPU work -- the summary of tools/gpu_runs/yuv_out_timing.sh's bench.py passes (parent_<n>.json / new_<n>.json in DIR,
     the parent commit and this tree alternating in one call, the feature off): every pass's frames/s, the medians, and whether this
     tree's median lies within the spread of the parent's own passes.

Usage: tools/bench_yuv.py [--out FILE] [--skip-8k] [--only 12] [--ab DIR]"""
import argparse
import ctypes as C
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from refvsr_amd import hip, ops, yuv  # noqa: E402

LAUNCHES, REPEATS, WARMUP = 48, 7, 2
CACHE_BYTES = 256 << 20
dev = torch.device('cuda:0')
_out = []


def say(line=''):
    print(line, flush=True)
    _out.append(line)


def device_us(fns):
    """us per launch of the launches in `fns`, issued back to back between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for fn in fns:
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / len(fns) * 1e3


def alternate(variants):
    """{name: [us per launch, one per repeat]}: every repeat times every variant's launch list once, in turn."""
    gc.collect()
    gc.disable()
    try:
        for fns in variants.values():
            for _ in range(WARMUP):
                for fn in fns:
                    fn()
        torch.cuda.synchronize()
        res = dict((k, []) for k in variants)
        for _ in range(REPEATS):
            for k, fns in variants.items():
                res[k].append(device_us(fns))
        return res
    finally:
        gc.enable()


def med(v):
    return sorted(v)[len(v) // 2]


def kernel(sizes):
    say('== 1. refvsr_result_to_yuv420 alone: device us per launch, median of %d repeats x %d launches [min .. max], TB/s over algorithmic bytes' % (REPEATS, LAUNCHES))
    say('   yardstick = refvsr_convert_result_hwc (float32 planar -> uint8 channels-last) on the same frames in the same repeats; bar: f32-chw <= 1.25 x yardstick')
    lib = hip.lib()
    st = ops._stream()
    P = C.c_void_p
    g = torch.Generator().manual_seed(1)
    for h, w in sizes:
        npix = h * w
        base = torch.rand(3, h, w, generator=g)
        for fmt in ('nv12', 'p010'):
            coef = (C.c_double * 9)(*yuv.coefficients(fmt, 'bt709', 'limited'))
            dbytes = yuv.frame_bytes(h, w, fmt)
            ddt = torch.uint8 if yuv.depth_of(fmt) == 8 else torch.uint16
            for sname, sfmt, es in (('f32-chw', hip.RESULT_F32, 4), ('u8-hwc', hip.RESULT_U8 | hip.RESULT_HWC, 1)):
                sbytes = 3 * npix * es
                nbuf = max(2, CACHE_BYTES // (sbytes + dbytes) + 2)           # the set walked per pass exceeds the Infinity Cache
                if sname == 'f32-chw':
                    srcs = [(base + 0).to(dev) for _ in range(nbuf)]
                else:
                    srcs = [(base * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().to(dev).permute(2, 0, 1) for _ in range(nbuf)]
                dsts = [torch.empty(yuv.frame_shape(h, w), dtype=ddt, device=dev) for _ in range(nbuf)]
                tabs = [((P * 1)(s.data_ptr()), (P * 1)(d.data_ptr())) for s, d in zip(srcs, dsts)]

                def conv(i):
                    ps, pd = tabs[i]
                    return lambda: lib.refvsr_result_to_yuv420(ps, sfmt, pd, 1, h, w, yuv.FORMAT_IDS[fmt], coef, st)
                assert conv(0)() == 0, lib.refvsr_last_error()
                torch.cuda.synchronize()
                exact = bool((dsts[0].cpu().numpy() == yuv.rgb_to_yuv420(srcs[0].cpu().numpy(), fmt)).all()) if npix <= 1080 * 1920 else None
                variants = {'rotated': [conv(i % nbuf) for i in range(LAUNCHES)], 'hot': [conv(0)] * LAUNCHES}
                ybytes = 0
                if sname == 'f32-chw':
                    ydst = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
                    ybytes = sbytes + 3 * npix

                    def yard(i):
                        s, d = srcs[i], ydst[i]
                        return lambda: lib.refvsr_convert_result_hwc(P(s.data_ptr()), h, w, hip.RESULT_U8 | hip.RESULT_HWC, P(d.data_ptr()), st)
                    assert yard(0)() == 0, lib.refvsr_last_error()
                    variants['yard_rotated'] = [yard(i % nbuf) for i in range(LAUNCHES)]
                    variants['yard_hot'] = [yard(0)] * LAUNCHES
                r = alternate(variants)
                tbs = lambda us, nbytes: nbytes / (us * 1e-6) / 1e12
                line = '%4dx%-4d %-5s %-7s (%2d buffers)' % (h, w, fmt, sname, nbuf)
                for k in ('rotated', 'hot'):
                    line += '  %s %8.1f us [%8.1f .. %8.1f] %5.2f TB/s' % (k, med(r[k]), min(r[k]), max(r[k]), tbs(med(r[k]), sbytes + dbytes))
                if exact is not None:
                    line += '  model bits=%s' % exact
                say(line)
                if ybytes:
                    line = '%4dx%-4d yardstick convert_result_hwc  ' % (h, w)
                    for k in ('rotated', 'hot'):
                        y = r['yard_' + k]
                        ratio = med(r[k]) / med(y)
                        line += '  %s %8.1f us [%8.1f .. %8.1f] %5.2f TB/s  yuv/yardstick %.3f %s' % (k, med(y), min(y), max(y), tbs(med(y), ybytes), ratio,
                                                                                                  'ok' if ratio <= 1.25 else 'MISSES the 1.25 bar')
                    say(line)
                del srcs, dsts, tabs, variants
                torch.cuda.empty_cache()


def frame_rate(steps=20, passes=3):
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    say()
    say('== 2. forward_group (4 windows, pipelined, config_RefVSR_small_L1, 270x480 -> 1080x1920, uint8 channels-last results): frames/s per pass of '
        '%d steps, alternating' % steps)
    t, G = 5, 4
    nfr = G * steps
    lr8, rf8, _ = make_clip(8, 270, 480, seed=0, want_gt=False)    # eight synthetic frames, walked back and forth: a continuous clip
    walk = [(0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1)[k % 14] for k in range(nfr)]
    lr, rf = lr8[walk].to(dev), rf8[walk].to(dev)
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    all_lr = torch.stack([lr[w] for w in wins], 0).contiguous()
    all_rf = torch.stack([rf[w] for w in wins], 0).contiguous()
    nets = {}
    for name, fmt in (('rgb', None), ('nv12', 'nv12')):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        cfg.frame_num, cfg.save_sample, cfg.result_dtype, cfg.result_layout, cfg.result_yuv = t, False, 'uint8', 'hwc', fmt
        net = SRNet(cfg).to(dev).eval()
        net.load_state_dict(make_state_dict(cfg, 1234))
        net.Network.set_pipelined(True)
        nets[name] = net
    sh, sw = 1080, 1920
    pinned = {'rgb': torch.empty((2, G, sh, sw, 3), dtype=torch.uint8).pin_memory(), 'nv12': torch.empty((2, G, 3 * sh // 2, sw), dtype=torch.uint8).pin_memory()}
    clip_no = [0]

    def one_pass(name, to_host):
        net = nets[name]
        clip_no[0] += 1
        ids = lambda f: [(clip_no[0], i) for i in wins[f]]
        last = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, f in enumerate(range(0, nfr, G)):
            last = net.forward_group(all_lr[f:f + G], all_rf[f:f + G], [ids(f + b) for b in range(G)], is_first_frame=(f == 0), input_ready='materialised')
            if to_host:                                            # the consumer's copy, on the stream that received the frames (two slots in turn)
                key = 'yuv' if name == 'nv12' else 'result'
                for b, x in enumerate(last[key]):
                    pinned[name][k & 1, b].copy_(x[0] if name == 'nv12' else x[0].permute(1, 2, 0), non_blocking=True)
        torch.cuda.synchronize()
        return nfr / (time.perf_counter() - t0), last

    for to_host, title in ((False, 'frames stay on the device'), (True, 'every group copied to pinned host memory (rgb: uint8 hwc result 3 B/px; nv12: yuv 1.5 B/px)')):
        fps = {'rgb': [], 'nv12': []}
        last = {}
        for name in nets:
            one_pass(name, to_host)
        gc.collect()
        gc.disable()
        try:
            for _ in range(passes):
                for name in nets:
                    v, last[name] = one_pass(name, to_host)
                    fps[name].append(v)
        finally:
            gc.enable()
        same = all(torch.equal(a, b) for a, b in zip(last['rgb']['result'], last['nv12']['result']))
        say('-- ' + title)
        for name in ('rgb', 'nv12'):
            say('frames/s  result_yuv=%-5s %s  median %.1f' % ('None' if name == 'rgb' else "'nv12'", ' '.join('%.1f' % x for x in fps[name]), med(fps[name])))
        say("nv12/None %.3f  spread of None %.1f frames/s  'result' of the last group equal=%s" % (med(fps['nv12']) / med(fps['rgb']), max(fps['rgb']) - min(fps['rgb']), same))


def ab_summary(path):
    import glob
    import json
    import re
    runs, order = {'parent': [], 'new': []}, []
    found = []
    for f in glob.glob(os.path.join(path, '*.json')):
        m = re.match(r'^(parent|new)_(\d+)\.json$', os.path.basename(f))
        if m:
            found.append((int(m.group(2)), m.group(1), f))
    for _, tree, f in sorted(found):
        rec = None
        for ln in open(f):
            if ln.strip().startswith('{'):
                try:
                    rec = json.loads(ln)
                except ValueError:
                    pass
        if rec and rec.get('value'):
            runs[tree].append(float(rec['value']))
            order.append(tree)
    say()
    say('== 3. the default path: bench.py --gpus 1 --steps 20 --warmup 5 (side legs off), result_yuv = None, passes in the order ' + ' '.join(order))
    if not runs['parent'] or not runs['new']:
        say('not measured')
        return
    for tree in ('parent', 'new'):
        say('frames/s  %-6s %s  median %.2f' % (tree, ' '.join('%.2f' % v for v in runs[tree]), med(runs[tree])))
    spread = max(runs['parent'] + runs['new']) - min(runs['parent'] + runs['new'])
    pspread = max(runs['parent']) - min(runs['parent'])
    diff = med(runs['new']) - med(runs['parent'])
    say('new - parent %+.2f frames/s (%.3f x); spread of the parent\'s own passes %.2f, of all passes %.2f  %s' % (
        diff, med(runs['new']) / med(runs['parent']), pspread, spread, 'within the spread' if abs(diff) <= spread else 'OUTSIDE the spread'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--skip-8k', action='store_true')
    ap.add_argument('--only', default='12', help='which measurements to run, e.g. 1')
    ap.add_argument('--ab', default=None, help='directory with parent_<n>.json / new_<n>.json bench.py lines to summarise (no GPU work)')
    args = ap.parse_args()
    if args.ab:
        ab_summary(args.ab)
        if args.out:
            with open(args.out, 'a') as f:
                f.write('\n'.join(_out) + '\n')
        return
    say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    sizes = [(1080, 1920)] + ([] if args.skip_8k else [(4320, 7680)])
    for key, fn in (('1', lambda: kernel(sizes)), ('2', frame_rate)):
        if key in args.only:
            fn()
            if args.out:                                           # (kept current: a later step that fails loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'w') as f:
                    f.write('\n'.join(_out) + '\n')


if __name__ == '__main__':
    main()
