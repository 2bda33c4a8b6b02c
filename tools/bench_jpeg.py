#!/usr/bin/env python3
"""The device JPEG encoder (refvsr_jpeg_encode, videorun --out x.mjpeg) on the GPU:

  1. the encoder alone, beside refvsr_result_to_yuv on the same frames and beside Pillow's save of the same frame on the host: one and
     four 1080 x 1920 frames and one 2176 x 3840 frame (synth's ground-truth frames), 'i420' and 'i444', quality 75 and 90, the default
     restart interval.  Device events around CALLS calls (five launches each), median of REPEATS repeats after warm-up.  'rotated'
     walks frame sets larger than the 256 MB Infinity Cache (every call reads its frames from HBM), 'hot' re-uses one set.  Checked
     against the numpy model first (1080p; the 4K frame against Pillow's decoder).  The compressed size against the I420 size.
  2. the restart interval: R = 1, 2, 4, 8 and one MCU row on the 1080p and the 4K frame ('i420', quality 90): device time (hot) and
     file size.  jpeg.DEFAULT_RESTART is chosen from this table.
  3. videorun, seconds per frame as the command prints them under --io stream (the loop's wall time), on a 544 x 960 i420 pair of
     --frames frames in --dir: the parent commit's command with --out x.y4m, this tree with --out x.y4m and with --out x.mjpeg, in
     alternating passes, every pass a fresh process under its own time limit; the bytes each wrote.

Usage: tools/bench_jpeg.py [--only 123] [--out FILE] [--parent DIR] [--frames 32] [--passes 3] [--dir /dev/shm]"""
import argparse
import ctypes as C
import gc
import io
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CALLS, REPEATS, WARMUP = 12, 5, 2
CACHE_BYTES = 256 << 20
_out = []


def say(line=''):
    print(line, flush=True)
    _out.append(line)


def med(v):
    return sorted(v)[len(v) // 2]


def device_us(fns):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for fn in fns:
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / len(fns) * 1e3


def timed(variants):
    """{name: [callables]} -> {name: the device us per call of every repeat}, the variants alternated."""
    import torch
    gc.collect()
    gc.disable()
    try:
        for fns in variants.values():
            for _ in range(WARMUP):
                for fn in fns:
                    fn()
        torch.cuda.synchronize()
        r = dict((k, []) for k in variants)
        for _ in range(REPEATS):
            for k, fns in variants.items():
                r[k].append(device_us(fns))
    finally:
        gc.enable()
    return r


def source_frames(n, h, w):
    """n natural-like uint8 [3, h, w] frames: synth's ground truth."""
    from refvsr_amd.synth import make_clip
    gt = make_clip(n, h // 4, w // 4, seed=3)[2].numpy()
    return np.rint(np.clip(gt, 0.0, 1.0) * 255.0).astype(np.uint8)


class Encoder(object):
    """refvsr_jpeg_encode on preallocated buffers: `sets` rotating sets of the same n frames."""

    def __init__(self, yuvs, h, w, fmt, quality, restart, sets):
        import torch
        from refvsr_amd import hip, jpeg, ops, yuv
        self.lib, self.n, self.h, self.w, self.fmt, self.q, self.r = hip.lib(), len(yuvs), h, w, fmt, quality, jpeg.check_restart(restart)
        dev = yuvs.device
        self.samp = yuv.SAMPLINGS[yuv.sampling_of(fmt)]
        self.tabs = ops._jpeg_tables(dev, quality, fmt)
        self.bound = self.lib.refvsr_jpeg_capacity(h, w, self.samp, self.r)
        self.wsb = self.lib.refvsr_jpeg_workspace_bytes(self.n, h, w, self.samp, self.r)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.dst = torch.empty(self.n * self.bound, dtype=torch.uint8, device=dev)
        self.meta = torch.zeros((2, self.n), dtype=torch.int64, device=dev)
        self.sets = [yuvs] + [yuvs.clone() for _ in range(sets - 1)]
        self.ptrs = [(C.c_void_p * self.n)(*[s[i].data_ptr() for i in range(self.n)]) for s in self.sets]
        self.st = ops._stream()

    def call(self, k=0):
        P = C.c_void_p
        qt, dct, lut = self.tabs
        rc = self.lib.refvsr_jpeg_encode(self.ptrs[k % len(self.ptrs)], self.n, self.h, self.w, self.samp, P(qt.data_ptr()), P(dct.data_ptr()),
                                         P(lut.data_ptr()), self.r, P(self.dst.data_ptr()), self.n * self.bound, P(self.meta.data_ptr() + 8 * self.n),
                                         P(self.meta.data_ptr()), P(self.ws.data_ptr()), self.wsb, self.st)
        assert rc == 0, self.lib.refvsr_last_error()

    def files(self):
        import torch
        from refvsr_amd import jpeg
        self.call(0)
        torch.cuda.synchronize()
        off, size = self.meta[0].tolist(), self.meta[1].tolist()
        head = jpeg.header(self.h, self.w, self.fmt, self.q, self.r)
        return [jpeg.assemble(head, self.dst[o:o + s].cpu().numpy().tobytes()) for o, s in zip(off, size)]


def pillow_ms(rgb, quality, fmt):
    """(ms of one save on one core, frames per second of 16 threads saving the same frame) -- Pillow releases the GIL while it codes."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(rgb.transpose(1, 2, 0)))
    save = lambda _=None: im.save(io.BytesIO(), 'JPEG', quality=quality, subsampling=2 if fmt == 'i420' else 0)
    one = []
    for _ in range(3):
        t0 = time.perf_counter()
        save()
        one.append(time.perf_counter() - t0)
    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        list(ex.map(save, range(32)))
        par = 32 / (time.perf_counter() - t0)
    return med(one) * 1e3, par


def kernels(only_r=False):
    import torch
    from PIL import Image
    from refvsr_amd import jpeg, ops, yuv
    dev = torch.device('cuda:0')
    rgb = {(1080, 1920): source_frames(4, 1080, 1920), (2176, 3840): source_frames(1, 2176, 3840)}
    if not only_r:
        say('== 1. refvsr_jpeg_encode alone (R = %d, five launches per call): device us per call, median of %d repeats x %d calls [min .. max];' % (
            jpeg.DEFAULT_RESTART, REPEATS, CALLS))
        say('   result_to_yuv of the same frames (uint8 RGB in) beside it; Pillow save of one frame on the host: ms on one core, frames/s of 16 threads')
        for (h, w), n in (((1080, 1920), 1), ((1080, 1920), 4), ((2176, 3840), 1)):
            res = torch.from_numpy(rgb[(h, w)][:n]).to(dev)
            for fmt in ('i420', 'i444'):
                y = ops.result_to_yuv(res, fmt, 'bt601', 'full', 'centre')
                nset = max(2, CACHE_BYTES // (n * yuv.frame_bytes(h, w, fmt)) + 2)
                to_yuv = timed({'yuv': [lambda: ops.result_to_yuv(res, fmt, 'bt601', 'full', 'centre')] * CALLS})['yuv']
                for q in (75, 90):
                    enc = Encoder(y, h, w, fmt, q, None, nset)
                    files = enc.files()
                    if h == 1080:
                        ok = files[0] == jpeg.encode_model(y[0].cpu().numpy(), h, w, fmt, q)
                    else:
                        ok = Image.open(io.BytesIO(files[0])).size == (w, h) and len(jpeg.split_mjpeg(files[0])) == 1
                    calls = max(CALLS, nset)
                    r = timed({'rotated': [lambda k=k: enc.call(k) for k in range(calls)], 'hot': [lambda: enc.call(0)] * CALLS})
                    pm, pf = pillow_ms(rgb[(h, w)][0], q, fmt)
                    size = sum(len(f) for f in files) / n
                    say('%4dx%-4d x %d %s q%d (%3d sets)  rotated %8.1f us [%8.1f .. %8.1f]  hot %8.1f us [%8.1f .. %8.1f]  result_to_yuv %7.1f us  |  Pillow %6.1f ms, '
                        '%5.1f frames/s on 16 threads  |  %8d bytes per frame = %.3f of I420 (%d)  %s=%s' % (
                            h, w, n, fmt, q, nset, med(r['rotated']), min(r['rotated']), max(r['rotated']), med(r['hot']), min(r['hot']), max(r['hot']),
                            med(to_yuv), pm, pf, size, size / yuv.frame_bytes(h, w, 'i420'), yuv.frame_bytes(h, w, 'i420'),
                            'model bytes' if h == 1080 else 'Pillow reads it', ok))
                    del enc
                    torch.cuda.empty_cache()
    say()
    say("== 2. the restart interval, 'i420' quality 90, one frame: device us per call (hot), median of %d x %d calls, and the file's bytes" % (REPEATS, CALLS))
    for h, w in ((1080, 1920), (2176, 3840)):
        y = ops.result_to_yuv(torch.from_numpy(rgb[(h, w)][:1]).to(dev), 'i420', 'bt601', 'full', 'centre')
        row = jpeg.geometry(h, w, 'i420')[1]
        for r_ in (1, 2, 4, 8, 16, row):
            enc = Encoder(y, h, w, 'i420', 90, r_, 1)
            size = len(enc.files()[0])
            t = timed({'hot': [lambda: enc.call(0)] * CALLS})['hot']
            say('%4dx%-4d R = %3d%s  %6d intervals  %8.1f us [%8.1f .. %8.1f]  %8d bytes' % (
                h, w, r_, ' (one MCU row)' if r_ == row else '              ', jpeg.intervals(h, w, 'i420', r_), med(t), min(t), max(t), size))
            del enc
            torch.cuda.empty_cache()


def videorun_passes(folder, parent, frames, passes):
    from refvsr_amd import yuv
    from refvsr_amd.synth import make_clip
    h, w = 544, 960
    say()
    say('== 3. videorun --io stream on a 544 x 960 i420 pair -> 2176 x 3840, %d frames (8 synthetic frames repeated), config_RefVSR_small_L1, --frame_num 5' % frames)
    say('   --frame_group 4, files in %s: seconds per frame as the command prints them (the loop\'s wall time), %d alternating passes, every pass a fresh process' % (folder, passes))
    lr, rf, _ = make_clip(8, h, w, seed=3, want_gt=False)
    paths = [os.path.join(folder, 'jpeg_bench_%s.y4m' % k) for k in ('uw', 'w')]
    for p, x in zip(paths, (lr, rf)):
        ys = yuv.rgb_to_yuv420(x.numpy(), 'i420')
        with yuv.Y4MWriter(p, h, w, 'i420', (24, 1), 'limited') as wr:
            for k in range(frames):
                wr.write(ys[k % 8])
    base = [sys.executable, '-m', 'refvsr_amd.videorun', '--lr', paths[0], '--ref', paths[1], '--frame_num', '5', '--frame_group', '4', '--io', 'stream']
    variants = [('parent commit, x.y4m ', parent, 'y4m'), ('this tree, x.y4m     ', ROOT, 'y4m'), ('this tree, x.mjpeg   ', ROOT, 'mjpeg')]
    res, size = dict((v[0], []) for v in variants), {}
    ok = True
    try:
        for p in range(passes + 1):                                     # (pass 0 warms the page cache and is not counted)
            for name, tree, ext in variants:
                out = os.path.join(folder, 'jpeg_bench_sr.' + ext)
                r = subprocess.run(['timeout', '-k', '10', '300'] + base + ['--out', out], cwd=tree, capture_output=True, text=True)
                m = re.search(r'\(([0-9.]+) sec / frame', r.stdout)
                if r.returncode != 0 or not m:
                    say('%s FAILED (exit %d): %s' % (name, r.returncode, (r.stderr or r.stdout)[-400:]))
                    return False
                if p:
                    res[name].append(float(m.group(1)))
                size[name] = os.path.getsize(out)
                if ext == 'mjpeg' and p == passes:
                    from refvsr_amd import jpeg
                    ok = len(jpeg.split_mjpeg(open(out, 'rb').read())) == frames
                os.remove(out)
    finally:
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
    for name, _, _ in variants:
        v = res[name]
        say('sec / frame  %s %s  median %.5f  spread %.5f  %11d bytes written' % (name, ' '.join('%.5f' % x for x in v), med(v), max(v) - min(v), size[name]))
    a, b, c = (med(res[v[0]]) for v in variants)
    say('this tree y4m - parent %+.5f sec / frame;  mjpeg - this tree y4m %+.5f sec / frame (%+.2f %%);  mjpeg bytes / y4m bytes %.4f;  split_mjpeg finds every frame: %s' % (
        b - a, c - b, 100 * (c - b) / b, size[variants[2][0]] / size[variants[1][0]], ok))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--only', default='123', help='which measurements to run, e.g. 12')
    ap.add_argument('--parent', default='build/parent', help='a built checkout of the parent commit')
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--dir', default='/dev/shm')
    args = ap.parse_args()
    ok = True
    try:
        if '1' in args.only or '2' in args.only:
            import torch
            say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
            kernels(only_r='1' not in args.only)
        if '3' in args.only:
            ok = videorun_passes(os.path.abspath(args.dir), os.path.abspath(args.parent), args.frames, args.passes)
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(_out) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
