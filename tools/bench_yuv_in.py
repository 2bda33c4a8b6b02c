#!/usr/bin/env python3
"""Y'CbCr 4:2:0 input frames (refvsr_yuv420_to_rgb, config.input_yuv) on the GPU, in one command:

  1. the kernel alone: 270 x 480 x 10 frames and 1080 x 1920 x 6 frames per launch, 'nv12' and 'p010'.  Device events around LAUNCHES
     launches, median of REPEATS repeats after warm-up.  Two columns: 'rotated' walks source and destination buffers through a set
     larger than the 256 MB Infinity Cache (every launch reads from HBM), 'hot' re-uses one set.  us per launch and TB/s over the
     algorithmic bytes (every source sample read once, every float written once).  Beside it, alternating with it in the same repeats
     on the same geometry: refvsr_ingest_u8 on channels-last bytes (3 bytes in, 12 out per pixel).  No bar.
  2. in the frame: frames/s of forward_group (four windows, pipelined, config_RefVSR_small_L1, 270 x 480) with input_yuv = 'nv12'
     against uint8 channels-last input, alternating passes in one process, the windows resident on the device; then the same with
     every group's windows copied from pinned host memory first (nv12: 1.5 B/px, uint8: 3 B/px).  No bar: the expectation is equality
     within the spread of the passes.

Usage: tools/bench_yuv_in.py [--out FILE] [--only 12]"""
import argparse
import ctypes as C
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def kernel():
    say('== 1. refvsr_yuv420_to_rgb alone: device us per launch, median of %d repeats x %d launches [min .. max], TB/s over algorithmic bytes' % (REPEATS, LAUNCHES))
    say('   beside it refvsr_ingest_u8 (channels-last bytes) on the same geometry in the same repeats')
    lib = hip.lib()
    st = ops._stream()
    P = C.c_void_p
    rs = np.random.RandomState(1)
    for h, w, nf in ((270, 480, 10), (1080, 1920, 6)):
        npix = h * w
        obytes = nf * 12 * npix
        u8bytes = nf * 3 * npix
        for fmt in ('nv12', 'p010'):
            coef = (C.c_double * 9)(*yuv.decode_coefficients(fmt, 'bt709', 'limited'))
            sdt = np.uint8 if yuv.depth_of(fmt) == 8 else np.uint16
            sbytes = nf * yuv.frame_bytes(h, w, fmt)
            nset = max(2, CACHE_BYTES // (sbytes + obytes) + 2)           # the sets walked per pass exceed the Infinity Cache
            host = (rs.randint(0, 2 ** yuv.depth_of(fmt), (nf,) + yuv.frame_shape(h, w)) << yuv.FORMATS[fmt][2]).astype(sdt)
            srcs = [torch.from_numpy(host).to(dev) for _ in range(nset)]
            u8s = [torch.from_numpy(rs.randint(0, 256, (nf, h, w, 3)).astype(np.uint8)).to(dev) for _ in range(nset)]
            dsts = [torch.empty((nf, 3, h, w), dtype=torch.float32, device=dev) for _ in range(nset)]
            tabs = [((P * nf)(*[s[i].data_ptr() for i in range(nf)]), (P * nf)(*[u[i].data_ptr() for i in range(nf)]),
                     (P * nf)(*[d[i].data_ptr() for i in range(nf)])) for s, u, d in zip(srcs, u8s, dsts)]

            def conv(k):
                ps, _, pd = tabs[k]
                return lambda: lib.refvsr_yuv420_to_rgb(ps, pd, nf, h, w, yuv.FORMAT_IDS[fmt], 0, coef, st)

            def ing(k):
                _, pu, pd = tabs[k]
                return lambda: lib.refvsr_ingest_u8(pu, pd, nf, h, w, hip.INGEST_HWC, st)
            assert conv(0)() == 0, lib.refvsr_last_error()
            torch.cuda.synchronize()
            exact = bool((dsts[0][0].cpu().numpy().view(np.uint32) == yuv.yuv420_to_rgb(host[0], h, w, fmt).view(np.uint32)).all())
            assert ing(0)() == 0, lib.refvsr_last_error()
            r = alternate({'rotated': [conv(i % nset) for i in range(LAUNCHES)], 'hot': [conv(0)] * LAUNCHES,
                           'u8_rotated': [ing(i % nset) for i in range(LAUNCHES)], 'u8_hot': [ing(0)] * LAUNCHES})
            tbs = lambda us, nbytes: nbytes / (us * 1e-6) / 1e12
            for name, pre, nbytes in (('yuv420_to_rgb %-4s' % fmt, '', sbytes + obytes), ('ingest_u8 hwc     ', 'u8_', u8bytes + obytes)):
                line = '%4dx%-4d x %2d frames  %s (%2d sets)' % (h, w, nf, name, nset)
                for k in ('rotated', 'hot'):
                    v = r[pre + k]
                    line += '  %s %8.1f us [%8.1f .. %8.1f] %5.2f TB/s' % (k, med(v), min(v), max(v), tbs(med(v), nbytes))
                say(line + ('  model bits=%s' % exact if not pre else ''))
            del srcs, u8s, dsts, tabs
            torch.cuda.empty_cache()


def frame_rate(steps=20, passes=3):
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    say()
    say('== 2. forward_group (4 windows, pipelined, config_RefVSR_small_L1, 270x480 -> 1080x1920): frames/s per pass of %d steps, alternating' % steps)
    t, G, h, w = 5, 4, 270, 480
    nfr = G * steps
    lr8, rf8, _ = make_clip(8, h, w, seed=0, want_gt=False)    # eight synthetic frames, walked back and forth: a continuous clip
    walk = [(0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1)[k % 14] for k in range(nfr)]
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    host, nets = {}, {}
    for name in ('u8', 'nv12'):
        if name == 'u8':                                        # channels-last bytes [nfr, t, h, w, 3], passed as the [.., 3, h, w] view
            fr = [(x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() for x in (lr8, rf8)]
        else:
            fr = [torch.from_numpy(yuv.rgb_to_yuv420(x.numpy(), 'nv12')) for x in (lr8, rf8)]
        host[name] = [torch.stack([x[walk][wi] for wi in wins], 0).contiguous().pin_memory() for x in fr]
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        cfg.frame_num, cfg.save_sample = t, False
        cfg.input_yuv = 'nv12' if name == 'nv12' else None
        net = SRNet(cfg).to(dev).eval()
        net.load_state_dict(make_state_dict(cfg, 1234))
        net.Network.set_pipelined(True)
        nets[name] = net
    view = lambda name, x: x.permute(0, 1, 4, 2, 3) if name == 'u8' else x
    resident = dict((name, [x.to(dev) for x in host[name]]) for name in host)
    clip_no = [0]

    def one_pass(name, from_host):
        net = nets[name]
        clip_no[0] += 1
        ids = lambda f: [(clip_no[0], i) for i in wins[f]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(0, nfr, G):
            if from_host:           # the producer's copy, on the caller's stream: input_ready=None makes the internal streams wait for it
                a, b = (x[f:f + G].to(dev, non_blocking=True) for x in host[name])
                net.forward_group(view(name, a), view(name, b), [ids(f + k) for k in range(G)], is_first_frame=(f == 0))
            else:
                a, b = (x[f:f + G] for x in resident[name])
                net.forward_group(view(name, a), view(name, b), [ids(f + k) for k in range(G)], is_first_frame=(f == 0), input_ready='materialised')
        torch.cuda.synchronize()
        return nfr / (time.perf_counter() - t0)

    for from_host, title in ((False, 'windows resident on the device'),
                             (True, "every group's windows copied from pinned host memory (nv12: 1.5 B/px, uint8 hwc: 3 B/px)")):
        fps = {'u8': [], 'nv12': []}
        for name in nets:
            one_pass(name, from_host)
        gc.collect()
        gc.disable()
        try:
            for _ in range(passes):
                for name in nets:
                    fps[name].append(one_pass(name, from_host))
        finally:
            gc.enable()
        say('-- ' + title)
        for name, label in (('u8', 'uint8 hwc input  '), ('nv12', "input_yuv='nv12' ")):
            say('frames/s  %s %s  median %.1f' % (label, ' '.join('%.1f' % x for x in fps[name]), med(fps[name])))
        say('nv12/uint8 %.3f  spread of the uint8 passes %.1f frames/s, of the nv12 passes %.1f' % (
            med(fps['nv12']) / med(fps['u8']), max(fps['u8']) - min(fps['u8']), max(fps['nv12']) - min(fps['nv12'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--only', default='12', help='which measurements to run, e.g. 1')
    args = ap.parse_args()
    say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for key, fn in (('1', kernel), ('2', frame_rate)):
        if key in args.only:
            fn()
            if args.out:                                           # (kept current: a later step that fails loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'w') as f:
                    f.write('\n'.join(_out) + '\n')


if __name__ == '__main__':
    main()
