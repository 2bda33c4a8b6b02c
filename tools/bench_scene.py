#!/usr/bin/env python3
"""Scene cuts (refvsr_luma_sad, videorun --scene_cut) on the GPU:

  1. the kernel alone: 5 pairs per call (a group of four new frames and the one before them) at 270 x 480 and 1080 x 1920, 'nv12' and
     'p010'.  Device events around LAUNCHES calls (two launches each), median of REPEATS repeats after warm-up.  Two columns:
     'rotated' walks frame sets larger than the 256 MB Infinity Cache (every call reads from HBM), 'hot' re-uses one set.  us per
     call and GB/s over the 2 h w samplesize bytes of every pair.  Checked against the numpy model first.  No bar.
  2. videorun, seconds per frame as the command prints them, on a cut-free 64-frame 270 x 480 .y4m pair (--make-file writes it, on the
     CPU, and checks with the numpy model that no score reaches the threshold): the parent commit's command, this tree without
     options, this tree with --scene_cut 0.1, in alternating passes, every pass a fresh process under its own time limit.

Usage: tools/bench_scene.py --make-file DIR | [--out FILE] [--only 12] [--files DIR] [--parent DIR] [--passes 3]"""
import argparse
import ctypes as C
import gc
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

LAUNCHES, REPEATS, WARMUP = 48, 7, 2
CACHE_BYTES = 256 << 20
THRESHOLD = 0.1
NFRAMES, H, W = 64, 270, 480
_out = []


def say(line=''):
    print(line, flush=True)
    _out.append(line)


def med(v):
    return sorted(v)[len(v) // 2]


def make_file(folder):
    """uw.y4m / w.y4m: 64 synthetic 270 x 480 frames, i420.  synth's clip moves half an LR pixel per frame; its motion is scaled to a
    tenth (frame 0 + (frame k - frame 0) / 10) so that frame 1, scored against a still picture, stays below the threshold too."""
    from refvsr_amd import scene, yuv
    from refvsr_amd.synth import make_clip
    os.makedirs(folder, exist_ok=True)
    lr, rf, _ = make_clip(NFRAMES, H, W, seed=0, want_gt=False)
    ys = [yuv.rgb_to_yuv420((0.9 * x[:1] + 0.1 * x).numpy(), 'i420') for x in (lr, rf)]
    s = scene.scene_scores([yuv.luma_sad(ys[0][k], ys[0][k - 1], H, W, 'i420') for k in range(1, NFRAMES)], H, W, 8)
    assert scene.cuts_from_scores(s, THRESHOLD) == (), s
    for name, y in zip(('uw', 'w'), ys):
        with yuv.Y4MWriter(os.path.join(folder, name + '.y4m'), H, W, 'i420', (24, 1), 'limited') as wr:
            for f in y:
                wr.write(f)
    print('%s: %d frames %d x %d, largest scene score %.4f (threshold %.2f)' % (folder, NFRAMES, H, W, max(s), THRESHOLD))


def kernel():
    import torch
    from refvsr_amd import hip, ops, yuv
    dev = torch.device('cuda:0')

    def device_us(fns):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for fn in fns:
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(fns) * 1e3

    say('== 1. refvsr_luma_sad alone, 5 pairs per call: device us per call, median of %d repeats x %d calls [min .. max], GB/s over the' % (REPEATS, LAUNCHES))
    say('   2 h w samplesize bytes of every pair')
    lib = hip.lib()
    st = ops._stream()
    P = C.c_void_p
    rs = np.random.RandomState(1)
    npairs = 5
    for h, w in ((270, 480), (1080, 1920)):
        for fmt in ('nv12', 'p010'):
            sdt = np.uint8 if yuv.depth_of(fmt) == 8 else np.uint16
            nbytes = npairs * 2 * h * w * np.dtype(sdt).itemsize
            wbytes = (npairs + 1) * yuv.frame_bytes(h, w, fmt)
            nset = max(2, CACHE_BYTES // wbytes + 2)                 # the windows walked per pass exceed the Infinity Cache
            host = (rs.randint(0, 2 ** yuv.depth_of(fmt), (npairs + 1,) + yuv.frame_shape(h, w)) << yuv.FORMATS[fmt][2]).astype(sdt)
            wins = [torch.from_numpy(host).to(dev) for _ in range(nset)]
            nws = lib.refvsr_luma_sad_workspace_bytes(npairs, h, w)
            ws = torch.empty(nws // 4, dtype=torch.int32, device=dev)
            sad = torch.zeros(npairs, dtype=torch.int64, device=dev)
            tabs = [((P * npairs)(*[x[i + 1].data_ptr() for i in range(npairs)]), (P * npairs)(*[x[i].data_ptr() for i in range(npairs)])) for x in wins]

            def call(k):
                pa, pb = tabs[k]
                return lambda: lib.refvsr_luma_sad(pa, pb, npairs, h, w, yuv.FORMAT_IDS[fmt], P(ws.data_ptr()), nws, P(sad.data_ptr()), st)
            assert call(0)() == 0, lib.refvsr_last_error()
            torch.cuda.synchronize()
            exact = sad.cpu().tolist() == [yuv.luma_sad(host[i + 1], host[i], h, w, fmt) for i in range(npairs)]
            variants = {'rotated': [call(i % nset) for i in range(LAUNCHES)], 'hot': [call(0)] * LAUNCHES}
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
            line = '%4dx%-4d x %d pairs  luma_sad %-4s (%3d sets)' % (h, w, npairs, fmt, nset)
            for k in ('rotated', 'hot'):
                v = r[k]
                line += '  %s %7.1f us [%7.1f .. %7.1f] %7.1f GB/s' % (k, med(v), min(v), max(v), nbytes / (med(v) * 1e-6) / 1e9)
            say(line + '  model integers=%s' % exact)
            del wins, tabs
            torch.cuda.empty_cache()


def videorun_passes(files, parent, passes):
    say()
    say('== 2. videorun on a cut-free %d-frame %d x %d i420 file, config_RefVSR_small_L1, --frame_num 5 --frame_group 4: seconds per frame as the' % (NFRAMES, H, W))
    say('   command prints them (network calls with their uploads and read-backs; under --scene_cut also the detector), %d alternating passes,' % passes)
    say('   every pass a fresh process')
    base = [sys.executable, '-m', 'refvsr_amd.videorun', '--lr', os.path.join(files, 'uw.y4m'), '--ref', os.path.join(files, 'w.y4m'),
            '--frame_num', '5', '--frame_group', '4']
    variants = [('parent commit          ', parent, []), ('this tree, no option   ', ROOT, []), ('this tree, --scene_cut  ', ROOT, ['--scene_cut', str(THRESHOLD)])]
    res = dict((name, []) for name, _, _ in variants)
    sums = {}
    for p in range(passes):
        for name, tree, extra in variants + ([variants[0]] if p == passes - 1 else []):      # (the parent first and last)
            out = os.path.join(files, 'sr_%d.y4m' % len(sums))
            r = subprocess.run(['timeout', '-k', '10', '240'] + base + ['--out', out] + extra, cwd=tree, capture_output=True, text=True)
            m = re.search(r'\(([0-9.]+) sec / frame(, (\d+) scenes)?\)', r.stdout)
            if r.returncode != 0 or not m:
                say('%s FAILED (exit %d): %s' % (name, r.returncode, (r.stderr or r.stdout)[-400:]))
                return False
            res[name].append(float(m.group(1)))
            with open(out, 'rb') as f:
                sums.setdefault(name, set()).add(hash(f.read()))
            os.remove(out)
            if m.group(3):
                assert m.group(3) == '1', r.stdout
    for name, _, _ in variants:
        v = res[name]
        say('sec / frame  %s %s  median %.5f  spread %.5f' % (name, ' '.join('%.5f' % x for x in v), med(v), max(v) - min(v)))
    say('the three commands wrote the same bytes: %s' % (len(set.union(*sums.values())) == 1))
    mp, mn, ms = (med(res[name]) for name, _, _ in variants)
    say('no option - parent %+.5f sec / frame (%+.2f %%);  --scene_cut - no option %+.5f sec / frame (%+.2f %%)' % (
        mn - mp, 100 * (mn - mp) / mp, ms - mn, 100 * (ms - mn) / mn))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--make-file', default=None, metavar='DIR', help='write the cut-free test file pair into DIR (CPU only) and stop')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--only', default='12', help='which measurements to run, e.g. 1')
    ap.add_argument('--files', default='build/scene_timing', help='the folder --make-file wrote')
    ap.add_argument('--parent', default='build/parent', help='a built checkout of the parent commit')
    ap.add_argument('--passes', type=int, default=3)
    args = ap.parse_args()
    if args.make_file:
        return make_file(args.make_file)
    ok = True
    if '1' in args.only:
        import torch
        say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
        kernel()
    if '2' in args.only:
        ok = videorun_passes(os.path.abspath(args.files), os.path.abspath(args.parent), args.passes)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(_out) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
