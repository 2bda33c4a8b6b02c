#!/usr/bin/env python3
"""The antialiased resize (refvsr_resize_aa) on the GPU, in one command:

  1. the kernel alone: 1080 x 1920 -> 270 x 480 (4 frames per launch; float32 planar source, float32 and uint8 destination) and
     4320 x 7680 -> 2160 x 3840 (one frame; float32 planar and uint8 channels-last source), each beside refvsr_yuv_to_rgb and
     refvsr_result_to_yuv ('i420') on a frame of the source's size -- kernels that also pass once over such a frame.  Device events
     around LAUNCHES launches, median of REPEATS repeats after warm-up.  'rotated' walks source and destination through a set
     larger than the 256 MB Infinity Cache (every launch reads from HBM), 'hot' re-uses one set.  us per launch and TB/s over the
     algorithmic bytes (every source sample read once, every output sample written once).  No bar.
  2. videorun on one synthetic clip (544 x 960 .y4m pair, 8 frames, config_RefVSR_small_L1, t = 5, groups of 4): seconds per frame
     without the options, with --out_size 1920x1088, with --in_down 4, with --in_down 4 --score.  No bar.

Usage: tools/bench_resize_aa.py [--out FILE] [--only 12]"""
import argparse
import ctypes as C
import gc
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from refvsr_amd import hip, ops, resize, yuv  # noqa: E402

LAUNCHES, REPEATS, WARMUP = 12, 5, 2
CACHE_BYTES = 256 << 20
dev = torch.device('cuda:0')
P = C.c_void_p
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


def alternate(variants, repeats=REPEATS):
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
        for _ in range(repeats):
            for k, fns in variants.items():
                res[k].append(device_us(fns))
        return res
    finally:
        gc.enable()


def med(v):
    return sorted(v)[len(v) // 2]


def tables(tensors, nf):
    return [(P * nf)(*[t[i].data_ptr() for i in range(nf)]) for t in tensors]


def kernels(lib, st):
    say('== 1. refvsr_resize_aa alone, beside the YUV kernels on a frame of the source\'s size: device us per launch, median of %d repeats x '
        '%d launches [min .. max], TB/s over the algorithmic bytes' % (REPEATS, LAUNCHES))
    rs = np.random.RandomState(1)
    for h, w, oh, ow, nf, cases in ((1080, 1920, 270, 480, 4, (('float32', False, 'float32'), ('float32', False, 'uint8'))),
                                    (4320, 7680, 2160, 3840, 1, (('float32', False, 'float32'), ('uint8', True, 'float32')))):
        variants, meta, keep = {}, [], []
        taps = ops._resize_taps(dev, h, w, oh, ow)
        tp = [ops._ptr(t) for t in taps[:6]]
        for dt, hwc, out in cases:
            es, ds = (4 if dt == 'float32' else 1), (4 if out == 'float32' else 1)
            nbytes = nf * 3 * (h * w * es + oh * ow * ds)
            nset = max(2, CACHE_BYTES // nbytes + 2)
            shape = (nf, h, w, 3) if hwc else (nf, 3, h, w)
            host = rs.rand(*shape).astype(np.float32) if dt == 'float32' else rs.randint(0, 256, shape).astype(np.uint8)
            srcs = [torch.from_numpy(host).to(dev) for _ in range(nset)]
            dsts = [torch.empty((nf, 3, oh, ow), dtype=torch.float32 if out == 'float32' else torch.uint8, device=dev) for _ in range(nset)]
            ps, pd = tables(srcs, nf), tables(dsts, nf)
            sfmt = (hip.RESULT_F32 if dt == 'float32' else hip.RESULT_U8) | (hip.RESULT_HWC if hwc else 0)
            dfmt = hip.RESULT_F32 if out == 'float32' else hip.RESULT_U8

            def go(k, ps=ps, pd=pd, sfmt=sfmt, dfmt=dfmt):
                return lambda: lib.refvsr_resize_aa(ps[k], sfmt, pd[k], dfmt, nf, h, w, oh, ow, *(tp + [taps[6], taps[7], 1, st]))
            assert go(0)() == 0, lib.refvsr_last_error()
            torch.cuda.synchronize()
            note = ''
            if h < 2000:
                x0 = np.moveaxis(host[0], -1, 0) if hwc else host[0]
                note = '  model bits=%s' % bool((dsts[0][0].cpu().numpy() == resize.resize_aa_model(x0, oh, ow, out)).all())
            name = 'resize_aa %s %s -> %s' % (dt, 'hwc' if hwc else 'chw', out)
            variants[name + ' rotated'] = [go(i % nset) for i in range(LAUNCHES)]
            variants[name + ' hot'] = [go(0)] * LAUNCHES
            meta.append((name, nset, nbytes, note))
            keep.append((srcs, dsts, ps, pd))
        # the two YUV kernels on the same frame size
        fbytes, ybytes = nf * 12 * h * w, nf * yuv.frame_bytes(h, w, 'i420')
        nset = max(2, CACHE_BYTES // (fbytes + ybytes) + 2)
        ys = [torch.from_numpy(rs.randint(0, 256, (nf,) + yuv.frame_shape(h, w, 'i420')).astype(np.uint8)).to(dev) for _ in range(nset)]
        fs = [torch.rand((nf, 3, h, w), dtype=torch.float32, device=dev) for _ in range(nset)]
        py, pf = tables(ys, nf), tables(fs, nf)
        cin = (C.c_double * 9)(*yuv.decode_coefficients('i420', 'bt709', 'limited'))
        cout = (C.c_double * 9)(*yuv.coefficients('i420', 'bt709', 'limited'))
        fid = yuv.FORMAT_IDS['i420']
        for name, call in (('yuv_to_rgb i420 -> float32', lambda k: lib.refvsr_yuv_to_rgb(py[k], pf[k], nf, h, w, fid, 0, 0, 0, cin, st)),
                           ('result_to_yuv float32 -> i420', lambda k: lib.refvsr_result_to_yuv(pf[k], hip.RESULT_F32, py[k], nf, h, w, fid, 0, 0, cout, st))):
            assert call(0) == 0, lib.refvsr_last_error()
            variants[name + ' rotated'] = [(lambda k=i % nset, call=call: call(k)) for i in range(LAUNCHES)]
            variants[name + ' hot'] = [(lambda call=call: call(0))] * LAUNCHES
            meta.append((name, nset, fbytes + ybytes, ''))
        r = alternate(variants)
        for name, nset, nbytes, note in meta:
            line = '%4dx%-4d -> %4dx%-4d x %d  %-34s (%d sets)' % (h, w, oh, ow, nf, name, nset)
            for k in ('rotated', 'hot'):
                v = r['%s %s' % (name, k)]
                line += '  %s %8.1f us [%8.1f .. %8.1f] %5.2f TB/s' % (k, med(v), min(v), max(v), nbytes / (med(v) * 1e-6) / 1e12)
            say(line + note)
        del variants, meta, keep, ys, fs, py, pf
        torch.cuda.empty_cache()


def video(passes=2):
    from refvsr_amd import SRNet, get_config, make_state_dict, videorun
    from refvsr_amd.synth import make_clip
    say()
    nfr, t, G, h, w = 8, 5, 4, 544, 960
    say('== 2. videorun, %d x %d .y4m pair (i420), %d frames, config_RefVSR_small_L1, t = %d, groups of %d: seconds per frame (the run\'s own '
        'clock: upload, network, conversions, read-back), one figure per pass, passes alternating' % (h, w, nfr, t, G))
    with tempfile.TemporaryDirectory() as tmp:
        lr, rf, _ = make_clip(nfr, h, w, seed=3, want_gt=False)
        paths = []
        for tag, x in (('uw', lr), ('w', rf)):
            paths.append(os.path.join(tmp, tag + '.y4m'))
            with yuv.Y4MWriter(paths[-1], h, w, 'i420', (24, 1), 'limited') as wr:
                for f in yuv.rgb_to_yuv420(x.numpy(), 'i420', 'bt709', 'limited'):
                    wr.write(f)
        variants = (('no option           (-> 2176 x 3840)', {}), ('--out_size 1920x1088                ', dict(out_size='1920x1088')),
                    ('--in_down 4         (-> 544 x 960)  ', dict(in_down=4)), ('--in_down 4 --score (-> 544 x 960)  ', dict(in_down=4, score_file=os.path.join(tmp, 's.txt'))))
        secs = dict((k, []) for k, _ in variants)
        for p in range(passes + 1):                                   # (pass 0 warms up: engines, tap tables, allocator)
            for name, kw in variants:
                cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
                cfg.frame_num, cfg.save_sample = t, False
                cfg.EVAL.frame_group = G
                for k, v in kw.items():
                    setattr(cfg.EVAL, k, v)
                net = SRNet(cfg).to(dev).eval()
                net.load_state_dict(make_state_dict(cfg, 1234))
                n, s = videorun.run(cfg, paths[0], paths[1], os.path.join(tmp, 'sr.y4m'), net=net)
                if p:
                    secs[name].append(s / n)
                del net
                gc.collect()
                torch.cuda.empty_cache()
        for name, _ in variants:
            say('sec / frame  %s %s  median %.4f' % (name, ' '.join('%.4f' % x for x in secs[name]), med(secs[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--only', default='12', help='which measurements to run, e.g. 1')
    args = ap.parse_args()
    say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    lib, st = hip.lib(), ops._stream()
    for key, fn in (('1', lambda: kernels(lib, st)), ('2', video)):
        if key in args.only:
            fn()
            if args.out:                                           # (kept current: a later step that fails loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'w') as f:
                    f.write('\n'.join(_out) + '\n')


if __name__ == '__main__':
    main()
