#!/usr/bin/env python3
"""Channels-last result frames (config.result_layout = 'hwc', REFVSR_RESULT_HWC) against planar ones, on the GPU, in one command:

  1. head kernel time: refvsr_conv_last_fmt (C = 24, 48) and refvsr_conv_hr_last_fmt, uint8 and float32, 1080 x 1920 and 4320 x 7680,
     device events over LAUNCHES launches after warm-up, REPEATS repeats, 'chw' and 'hwc' alternating inside every repeat -- and, with
     --prev LIB, the planar launch of a previous build of the library in the same alternation (the planar path must not have moved);
  2. frames/s of forward_group (four windows, pipelined, config_RefVSR_small_L1, 270 x 480 -> 1080 x 1920, uint8 results), alternating
     passes of the two layouts;
  3. the device scorers on channels-last against planar results (score_frames and score_regions at 1080 x 1920, score_frames(down=4)
     on a 4320 x 7680 result): recorded, no bar;
  4. what the consumer gains: host time per uint8 frame of .cpu() + evalrun.write_frame's array preparation up to Image.fromarray.

Condition of 1 and 2 (printed per line as ok / SLOWER): the 'hwc' figure is no worse than the 'chw' figure by more than that session's
min-to-max spread of the 'chw' repeats.  Usage: tools/bench_result_layout.py [--prev LIB] [--out FILE] [--skip-8k]"""
import argparse
import ctypes as C
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from refvsr_amd import hip, ops  # noqa: E402

LAUNCHES, REPEATS, WARMUP = 50, 5, 5
dev = torch.device('cuda:0')
P = lambda t: C.c_void_p(t.data_ptr())
_out = []


def say(line=''):
    print(line, flush=True)
    _out.append(line)


def load_prev(path):
    h = C.CDLL(path)
    for name in ('refvsr_conv_last_fmt', 'refvsr_conv_hr_last_fmt'):
        fn = getattr(h, name)
        fn.argtypes = hip.SIGNATURES[name]
        fn.restype = C.c_int
    return h


def device_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternate(variants, iters=LAUNCHES, repeats=REPEATS):
    """{name: [us per launch, one per repeat]}: every repeat times every variant once, in turn."""
    gc.collect()
    gc.disable()
    try:
        for fn in variants.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        res = dict((k, []) for k in variants)
        for _ in range(repeats):
            for k, fn in variants.items():
                res[k].append(device_us(fn, iters))
        return res
    finally:
        gc.enable()


def verdict(chw, hwc, smaller_is_better=True):
    """'ok' when hwc is no worse than chw by more than chw's min-to-max spread (medians compared)."""
    med = lambda v: sorted(v)[len(v) // 2]
    spread = max(chw) - min(chw)
    bad = med(hwc) > med(chw) + spread if smaller_is_better else med(hwc) < med(chw) - spread
    return med(chw), med(hwc), spread, 'SLOWER' if bad else 'ok'


def heads(prev, sizes):
    from refvsr_amd.packing import pack_conv_hr_last, pack_conv_last
    say('== 1. head kernels: device us per launch, median of %d repeats x %d launches [min .. max]' % (REPEATS, LAUNCHES))
    g = torch.Generator().manual_seed(1)
    for h, w in sizes:
        bh, bw = h // 4, w // 4
        base = torch.rand(3, bh, bw, generator=g).to(dev)
        for kind, c in (('conv_last', 24), ('conv_last', 48), ('conv_hr_last', 24)):
            what = '%s C=%d %dx%d' % (kind, c, h, w)
            if not ops.conv_last_ok(c, h, w):
                say('%-34s not measured: the entry point takes maps below 2^31 bytes (h w C 2 = %.2f GB)' % (what, h * w * c * 2 / 2 ** 30))
                continue
            x = (torch.randn(h, w, c, device=dev) * 0.5).half()
            if kind == 'conv_last':
                blob = pack_conv_last(torch.randn(3, c, 3, 3, generator=g) * 0.03, torch.randn(3, generator=g) * 0.1).to(dev)
                call = lambda lib, out, fmt: lib.refvsr_conv_last_fmt(P(x), c, h, w, P(blob), P(base), bh, bw, P(out), fmt, ops._stream())
            else:
                blob = pack_conv_hr_last(torch.randn(24, 24, 3, 3, generator=g) / 216 ** 0.5, torch.randn(24, generator=g) * 0.1,
                                         torch.randn(3, 24, 3, 3, generator=g) * 0.04, torch.randn(3, generator=g) * 0.1).to(dev)
                call = lambda lib, out, fmt: lib.refvsr_conv_hr_last_fmt(P(x), h, w, P(blob), 0.1, P(base), bh, bw, P(out), fmt, ops._stream())
            for dt in ('uint8', 'float32'):
                tdt, fmt = ops.result_format(dt)
                o_chw = torch.empty((3, h, w), dtype=tdt, device=dev)
                o_hwc = torch.empty((h, w, 3), dtype=tdt, device=dev)
                o_prev = torch.empty((3, h, w), dtype=tdt, device=dev)
                cur = hip.lib()
                assert call(cur, o_chw, fmt) == 0 and call(cur, o_hwc, fmt | hip.RESULT_HWC) == 0
                torch.cuda.synchronize()
                same = torch.equal(o_hwc.permute(2, 0, 1), o_chw)
                variants = {'chw': lambda: call(cur, o_chw, fmt), 'hwc': lambda: call(cur, o_hwc, fmt | hip.RESULT_HWC)}
                if prev is not None:
                    assert call(prev, o_prev, fmt) == 0
                    torch.cuda.synchronize()
                    same = same and torch.equal(o_prev, o_chw)
                    variants['prev_chw'] = lambda: call(prev, o_prev, fmt)
                r = alternate(variants)
                mc, mh, spread, v = verdict(r['chw'], r['hwc'])
                line = '%-34s %-7s chw %8.1f [%8.1f .. %8.1f]  hwc %8.1f [%8.1f .. %8.1f]  hwc/chw %.3f  chw spread %.1f  %s  equal=%s' % (
                    what, dt, mc, min(r['chw']), max(r['chw']), mh, min(r['hwc']), max(r['hwc']), mh / mc, spread, v, same)
                if prev is not None:
                    pv = sorted(r['prev_chw'])
                    line += '  | previous build chw %8.1f [%8.1f .. %8.1f]  new/previous %.3f' % (pv[len(pv) // 2], pv[0], pv[-1], mc / pv[len(pv) // 2])
                say(line)
                del o_chw, o_hwc, o_prev
            del x
            torch.cuda.empty_cache()


def frame_rate(steps=20, passes=3):
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    say()
    say('== 2. forward_group (4 windows, pipelined, config_RefVSR_small_L1, 270x480 -> 1080x1920, uint8): frames/s per pass of %d steps, '
        'layouts alternating' % steps)
    t, G = 5, 4
    nfr = G * steps
    lr8, rf8, _ = make_clip(8, 270, 480, seed=0, want_gt=False)    # eight synthetic frames, walked back and forth: a continuous clip
    walk = [(0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1)[k % 14] for k in range(nfr)]
    lr, rf = lr8[walk].to(dev), rf8[walk].to(dev)
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    all_lr = torch.stack([lr[w] for w in wins], 0).contiguous()
    all_rf = torch.stack([rf[w] for w in wins], 0).contiguous()
    nets = {}
    for layout in ('chw', 'hwc'):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        cfg.frame_num, cfg.save_sample, cfg.result_dtype, cfg.result_layout = t, False, 'uint8', layout
        net = SRNet(cfg).to(dev).eval()
        net.load_state_dict(make_state_dict(cfg, 1234))
        net.Network.set_pipelined(True)
        nets[layout] = net
    clip_no = [0]

    def one_pass(net):
        clip_no[0] += 1
        ids = lambda f: [(clip_no[0], i) for i in wins[f]]
        last = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(0, nfr, G):
            last = net.forward_group(all_lr[f:f + G], all_rf[f:f + G], [ids(f + b) for b in range(G)], is_first_frame=(f == 0),
                                     input_ready='materialised')['result']
        torch.cuda.synchronize()
        return nfr / (time.perf_counter() - t0), last

    fps = {'chw': [], 'hwc': []}
    last = {}
    for layout, net in nets.items():                               # warm-up pass each
        one_pass(net)
    gc.collect()
    gc.disable()
    try:
        for _ in range(passes):
            for layout, net in nets.items():
                v, last[layout] = one_pass(net)
                fps[layout].append(v)
    finally:
        gc.enable()
    same = all(torch.equal(a, b) for a, b in zip(last['chw'], last['hwc']))
    dense = all(a.permute(0, 2, 3, 1).is_contiguous() for a in last['hwc'])
    mc, mh, spread, v = verdict(fps['chw'], fps['hwc'], smaller_is_better=False)
    say('frames/s  chw %s  median %.1f' % (' '.join('%.1f' % x for x in fps['chw']), mc))
    say('frames/s  hwc %s  median %.1f' % (' '.join('%.1f' % x for x in fps['hwc']), mh))
    say('hwc/chw %.3f  chw spread %.1f frames/s  %s  last group equal=%s  hwc dense [n,sh,sw,3]=%s' % (mh / mc, spread, v, same, dense))


def scorers(skip_8k):
    from refvsr_amd.metrics import fov_rects
    say()
    say('== 3. device scorers, channels-last against planar results (device us per call of one frame pair; recorded, no bar)')
    g = torch.Generator().manual_seed(3)

    def pair(dt, h, w, gh, gw):
        a = torch.randint(0, 256, (1, 3, h, w), dtype=torch.uint8, generator=g).to(dev)
        if dt == 'float32':
            a = a.float() / 255.0
        gt = torch.randint(0, 256, (1, gh, gw, 3), dtype=torch.uint8, generator=g).to(dev).permute(0, 3, 1, 2)
        return a, a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), gt

    cases = [('score_frames 1080x1920', 1080, 1920, 1, lambda a, t: ops.score_frames(a, t)),
             ('score_regions 1080x1920', 1080, 1920, 1, lambda a, t: ops.score_regions(a, t, fov_rects(1080, 1920)))]
    if not skip_8k:
        cases.append(('score_frames(down=4) 4320x7680', 4320, 7680, 4, lambda a, t: ops.score_frames(a, t, down=4)))
    for what, h, w, down, fn in cases:
        for dt in ('uint8', 'float32'):
            a, ah, gt = pair(dt, h, w, h // down, w // down)
            same = torch.equal(fn(a, gt), fn(ah, gt))
            r = alternate({'chw': lambda: fn(a, gt), 'hwc': lambda: fn(ah, gt)}, iters=20)
            mc, mh, spread, _ = verdict(r['chw'], r['hwc'])
            say('%-34s %-7s chw %8.1f [%8.1f .. %8.1f]  hwc %8.1f [%8.1f .. %8.1f]  hwc/chw %.3f  equal bits=%s' % (
                what, dt, mc, min(r['chw']), max(r['chw']), mh, min(r['hwc']), max(r['hwc']), mh / mc, same))
            del a, ah, gt
            torch.cuda.empty_cache()


def consumer(skip_8k):
    from PIL import Image
    say()
    say('== 4. host ms per uint8 frame on this machine\'s host: .cpu(), then write_frame\'s array preparation up to Image.fromarray '
        '(best of 5)')
    g = torch.Generator().manual_seed(4)
    for h, w in [(1080, 1920)] + ([] if skip_8k else [(4320, 7680)]):
        x = torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g).to(dev)
        frames = {'chw': x, 'hwc': x.permute(1, 2, 0).contiguous().permute(2, 0, 1)}
        for layout, fr in frames.items():
            t_cpu, t_img, t_raw = [], [], []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = fr.detach().cpu()
                t1 = time.perf_counter()
                im = Image.fromarray(c.numpy().transpose(1, 2, 0))
                t2 = time.perf_counter()
                raw = c.numpy().transpose(1, 2, 0).tobytes()
                t3 = time.perf_counter()
                t_cpu.append(t1 - t0)
                t_img.append(t2 - t1)
                t_raw.append(t3 - t2)
                del im, raw
            say('%dx%d %s: .cpu() %.2f ms  Image.fromarray(transpose) %.2f ms  (.tobytes() for a raw-video pipe %.2f ms)  sum to the image %.2f ms' % (
                h, w, layout, min(t_cpu) * 1e3, min(t_img) * 1e3, min(t_raw) * 1e3, (min(t_cpu) + min(t_img)) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prev', default=None, help='a previous build of librefvsr_hip.so: its planar head launches are timed alongside')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--skip-8k', action='store_true')
    ap.add_argument('--only', default='1234', help='which measurements to run, e.g. 13')
    args = ap.parse_args()
    say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    prev = load_prev(args.prev) if args.prev else None
    if prev is None:
        say('(no --prev library: the previous build\'s planar head was not measured)')
    sizes = [(1080, 1920)] + ([] if args.skip_8k else [(4320, 7680)])
    for key, fn in (('1', lambda: heads(prev, sizes)), ('2', frame_rate), ('3', lambda: scorers(args.skip_8k)), ('4', lambda: consumer(args.skip_8k))):
        if key in args.only:
            fn()
            if args.out:                                           # (kept current: a later step that fails loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'w') as f:
                    f.write('\n'.join(_out) + '\n')


if __name__ == '__main__':
    main()
