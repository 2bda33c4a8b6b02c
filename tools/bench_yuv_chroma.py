#!/usr/bin/env python3
"""4:2:2, 4:4:4 and left-sited frames (refvsr_yuv_to_rgb, refvsr_result_to_yuv) on the GPU, in one command:

  1. each new kernel alone, both ways: 1080 x 1920 (4 frames per launch) and 4320 x 7680 (one frame), next to the 4:2:0 / centre
     kernel of the same repeats.  Device events around LAUNCHES launches, median of REPEATS repeats after warm-up.  'rotated' walks
     source and destination through a set larger than the 256 MB Infinity Cache (every launch reads from HBM), 'hot' re-uses one
     set.  us per launch, TB/s over the algorithmic bytes (every source sample read once, every output sample written once) and that
     rate's share of the 8 TB/s HBM roof.  No bar.
  2. the 4:2:0 launches of a PARENT library (--parent: the librefvsr_hip.so of a built checkout of the parent commit) and of this
     tree's, loaded side by side into this process, in alternating passes: centre-sited through the 4:2:0 entries, each way and from
     a uint8 channels-last result, left-sited on the way out through the general entry.  A slowdown beyond the spread of the parent's
     own passes is a regression.
  3. forward_group (four windows, pipelined, config_RefVSR_small_L1, 270 x 480 -> 1080 x 1920) frames/s with result_yuv = 'i444p10'
     (6 bytes of 'yuv' per output pixel beside the result) against result_yuv = None, alternating passes; then the same with what
     a consumer takes copied to pinned host memory after every group: 'yuv' where there is one (1.5 or 6 bytes per pixel), the
     float32 'result' otherwise (12).  No bar.

Usage: tools/bench_yuv_chroma.py [--out FILE] [--only 123] [--parent PATH/librefvsr_hip.so]"""
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

LAUNCHES, REPEATS, WARMUP = 24, 7, 2
CACHE_BYTES = 256 << 20
ROOF = 8.0                     # TB/s, HBM3E of the MI355X
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


def ids(fmt, siting):
    return yuv.FORMAT_IDS[yuv.twin_of(fmt)], yuv.SAMPLINGS[yuv.sampling_of(fmt)], yuv.SITINGS[yuv.effective_siting(fmt, siting)]


def tables(tensors, nf):
    return [(P * nf)(*[t[i].data_ptr() for i in range(nf)]) for t in tensors]


def report(title, h, w, nf, nset, r, nbytes, note=''):
    line = '%4dx%-4d x %d  %-22s (%d sets)' % (h, w, nf, title, nset)
    for k in ('rotated', 'hot'):
        v = r[k]
        tbs = nbytes / (med(v) * 1e-6) / 1e12
        line += '  %s %8.1f us [%8.1f .. %8.1f] %5.2f TB/s %4.1f %%' % (k, med(v), min(v), max(v), tbs, 100.0 * tbs / ROOF)
    say(line + note)


GEOMETRIES = ((1080, 1920, 4), (4320, 7680, 1))


def kernels_in(lib, st):
    say('== 1a. refvsr_yuv_to_rgb alone (bilinear): device us per launch, median of %d repeats x %d launches [min .. max], TB/s over '
        'algorithmic bytes, %% of the %g TB/s roof; the first line of each geometry is the 4:2:0 / centre kernel in the same repeats' % (REPEATS, LAUNCHES, ROOF))
    rs = np.random.RandomState(1)
    for h, w, nf in GEOMETRIES:
        obytes = nf * 12 * h * w
        variants, meta = {}, []
        for fmt, siting in (('nv12', 'centre'), ('nv12', 'left'), ('i420p10', 'left'), ('i422', 'left'), ('i422p10', 'centre'), ('i444', 'centre'), ('i444p10', 'centre')):
            fid, samp, sit = ids(fmt, siting)
            coef = (C.c_double * 9)(*yuv.decode_coefficients(fmt, 'bt709', 'limited'))
            sbytes = nf * yuv.frame_bytes(h, w, fmt)
            nset = max(2, CACHE_BYTES // (sbytes + obytes) + 2)
            host = (rs.randint(0, 2 ** yuv.depth_of(fmt), (nf,) + yuv.frame_shape(h, w, fmt)) << yuv.FORMATS[yuv.twin_of(fmt)][2]).astype(yuv.dtype_of(fmt))
            srcs = [torch.from_numpy(host).to(dev) for _ in range(nset)]
            dsts = [torch.empty((nf, 3, h, w), dtype=torch.float32, device=dev) for _ in range(nset)]
            ps, pd = tables(srcs, nf), tables(dsts, nf)

            def conv(k, ps=ps, pd=pd, fid=fid, samp=samp, sit=sit, coef=coef):
                return lambda: lib.refvsr_yuv_to_rgb(ps[k], pd[k], nf, h, w, fid, samp, sit, 0, coef, st)
            assert conv(0)() == 0, lib.refvsr_last_error()
            torch.cuda.synchronize()
            exact = h > 2000 or bool((dsts[0][0].cpu().numpy().view(np.uint32) == yuv.yuv_to_rgb(host[0], h, w, fmt, siting=siting).view(np.uint32)).all())
            name = '%s %s' % (fmt, siting)
            variants[name + ' rotated'] = [conv(i % nset) for i in range(LAUNCHES)]
            variants[name + ' hot'] = [conv(0)] * LAUNCHES
            meta.append((name, nset, sbytes + obytes, exact, (srcs, dsts, ps, pd)))
        r = alternate(variants)
        for name, nset, nbytes, exact, _ in meta:
            report('in  ' + name, h, w, nf, nset, {'rotated': r[name + ' rotated'], 'hot': r[name + ' hot']}, nbytes, '' if h > 2000 else '  model bits=%s' % exact)
        del variants, meta
        torch.cuda.empty_cache()


def kernels_out(lib, st):
    say()
    say('== 1b. refvsr_result_to_yuv alone (float32 planar results): the same columns; the first line is the 4:2:0 / centre kernel')
    rs = np.random.RandomState(2)
    for h, w, nf in GEOMETRIES:
        sbytes = nf * 12 * h * w
        host = rs.rand(nf, 3, h, w).astype(np.float32)
        variants, meta = {}, []
        nsrc = max(2, CACHE_BYTES // sbytes + 2)
        srcs = [torch.from_numpy(host).to(dev) for _ in range(nsrc)]
        ps = tables(srcs, nf)
        for fmt, siting in (('nv12', 'centre'), ('nv12', 'left'), ('i420p10', 'left'), ('i422', 'left'), ('i422p10', 'centre'), ('i444', 'centre'), ('i444p10', 'centre')):
            fid, samp, sit = ids(fmt, siting)
            coef = (C.c_double * 9)(*yuv.coefficients(fmt, 'bt709', 'limited'))
            obytes = nf * yuv.frame_bytes(h, w, fmt)
            dsts = [torch.empty((nf,) + yuv.frame_shape(h, w, fmt), dtype=torch.uint8 if yuv.depth_of(fmt) == 8 else torch.uint16, device=dev) for _ in range(nsrc)]
            pd = tables(dsts, nf)

            def conv(k, pd=pd, fid=fid, samp=samp, sit=sit, coef=coef):
                return lambda: lib.refvsr_result_to_yuv(ps[k], hip.RESULT_F32, pd[k], nf, h, w, fid, samp, sit, coef, st)
            assert conv(0)() == 0, lib.refvsr_last_error()
            torch.cuda.synchronize()
            exact = h > 2000 or bool((dsts[0][0].cpu().numpy() == yuv.rgb_to_yuv(host[0], fmt, siting=siting)).all())
            name = '%s %s' % (fmt, siting)
            variants[name + ' rotated'] = [conv(i % nsrc) for i in range(LAUNCHES)]
            variants[name + ' hot'] = [conv(0)] * LAUNCHES
            meta.append((name, sbytes + obytes, exact, (dsts, pd)))
        r = alternate(variants)
        for name, nbytes, exact, _ in meta:
            report('out ' + name, h, w, nf, nsrc, {'rotated': r[name + ' rotated'], 'hot': r[name + ' hot']}, nbytes, '' if h > 2000 else '  model bits=%s' % exact)
        del variants, meta, srcs, ps
        torch.cuda.empty_cache()


def bind_parent(path):
    """The parent library's four conversion entries, bound beside this tree's (another file: another copy of the code and its state)."""
    lib = C.CDLL(path)
    for name in ('refvsr_yuv420_to_rgb', 'refvsr_result_to_yuv420', 'refvsr_yuv_to_rgb', 'refvsr_result_to_yuv'):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip.SIGNATURES[name], C.c_int
    return lib


# (way, format, siting, the results' form on the way out).  Centre goes through the 4:2:0 entries, left through the general ones:
# the left-sited 4:2:0 instances of the way out are the ones whose instruction stream is not the parent's (profiles/yuv_one_kernel.txt)
AB_ROWS = (('in ', 'nv12', 'centre', None), ('out', 'nv12', 'centre', 'f32'), ('in ', 'i420', 'centre', None), ('out', 'i420', 'centre', 'f32'),
           ('in ', 'i420p10', 'centre', None), ('out', 'i420p10', 'centre', 'f32'), ('out', 'nv12', 'centre', 'u8 hwc'),
           ('out', 'nv12', 'left', 'f32'), ('out', 'i420p10', 'left', 'f32'), ('out', 'i420', 'left', 'u8 hwc'))


def parent_ab(lib, parent_path, st, passes=5):
    say()
    say('== 2. the 4:2:0 launches, parent library against this tree\'s in one process: us per launch (rotated), one figure per pass of '
        '%d launches, passes alternating parent, new, parent, ...' % LAUNCHES)
    if not parent_path or not os.path.exists(parent_path):
        say('not measured: no parent library at %r' % (parent_path,))
        return
    old = bind_parent(parent_path)
    rs = np.random.RandomState(3)
    for h, w, nf in GEOMETRIES:
        for way, fmt, siting, form in AB_ROWS:
            fid, samp, sit = ids(fmt, siting)
            coef = (C.c_double * 9)(*(yuv.decode_coefficients if way == 'in ' else yuv.coefficients)(fmt, 'bt709', 'limited'))
            u8 = form == 'u8 hwc'
            ybytes, fbytes = nf * yuv.frame_bytes(h, w, fmt), nf * (3 if u8 else 12) * h * w
            nset = max(2, CACHE_BYTES // (ybytes + fbytes) + 2)
            host = (rs.randint(0, 2 ** yuv.depth_of(fmt), (nf,) + yuv.frame_shape(h, w)) << yuv.FORMATS[fmt][2]).astype(yuv.dtype_of(fmt))
            ys = [torch.from_numpy(host).to(dev) for _ in range(nset)]
            fs = [torch.randint(0, 256, (nf, h, w, 3), dtype=torch.uint8, device=dev) if u8 else torch.rand((nf, 3, h, w), dtype=torch.float32, device=dev)
                  for _ in range(nset)]
            py, pf = tables(ys, nf), tables(fs, nf)
            sfmt = hip.RESULT_U8 | hip.RESULT_HWC if u8 else hip.RESULT_F32
            if way == 'in ' and siting == 'centre':
                call = lambda L_, k: L_.refvsr_yuv420_to_rgb(py[k], pf[k], nf, h, w, fid, 0, coef, st)
            elif siting == 'centre':
                call = lambda L_, k: L_.refvsr_result_to_yuv420(pf[k], sfmt, py[k], nf, h, w, fid, coef, st)
            elif way == 'in ':
                call = lambda L_, k: L_.refvsr_yuv_to_rgb(py[k], pf[k], nf, h, w, fid, samp, sit, 0, coef, st)
            else:
                call = lambda L_, k: L_.refvsr_result_to_yuv(pf[k], sfmt, py[k], nf, h, w, fid, samp, sit, coef, st)
            assert call(old, 0) == 0 and call(lib, 0) == 0
            mk = lambda L_: [(lambda k=i % nset: call(L_, k)) for i in range(LAUNCHES)]
            r = alternate({'parent': mk(old), 'new': mk(lib)}, passes)
            sp = max(r['parent']) - min(r['parent'])
            d = med(r['new']) - med(r['parent'])
            say('%4dx%-4d x %d %s %-7s %-6s %-6s  parent %s  median %.1f | new %s  median %.1f | new - parent %+.1f us, spread of the parent\'s passes %.1f: %s'
                % (h, w, nf, way, fmt, siting, form or '', ' '.join('%.1f' % x for x in r['parent']), med(r['parent']), ' '.join('%.1f' % x for x in r['new']),
                   med(r['new']), d, sp, 'within the spread' if d <= sp else 'SLOWER than the spread'))
            del ys, fs, py, pf
            torch.cuda.empty_cache()


def frame_rate(steps=20, passes=3):
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    say()
    say("== 3. forward_group (4 windows, pipelined, config_RefVSR_small_L1, 270x480 -> 1080x1920), windows resident: frames/s per pass of %d steps, alternating" % steps)
    t, G, h, w = 5, 4, 270, 480
    nfr = G * steps
    lr8, rf8, _ = make_clip(8, h, w, seed=0, want_gt=False)
    walk = [(0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1)[k % 14] for k in range(nfr)]
    wins = [window_indices(f, nfr, t) for f in range(nfr)]
    lrs, rfs = (torch.stack([x[walk][wi] for wi in wins], 0).contiguous().to(dev) for x in (lr8, rf8))
    nets = {}
    for name, fmt in (('none', None), ('i420', 'i420'), ('i444p10', 'i444p10')):
        cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
        cfg.frame_num, cfg.save_sample, cfg.result_yuv = t, False, fmt
        net = SRNet(cfg).to(dev).eval()
        net.load_state_dict(make_state_dict(cfg, 1234))
        net.Network.set_pipelined(True)
        nets[name] = net
    clip_no = [0]
    sh, sw = 4 * h, 4 * w
    pinned = {'none': torch.empty((G, 3, sh, sw), dtype=torch.float32).pin_memory(),
              'i420': torch.empty((G,) + yuv.frame_shape(sh, sw, 'i420'), dtype=torch.uint8).pin_memory(),
              'i444p10': torch.empty((G,) + yuv.frame_shape(sh, sw, 'i444p10'), dtype=torch.uint16).pin_memory()}

    def one_pass(name, to_host=False):
        net = nets[name]
        clip_no[0] += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(0, nfr, G):
            out = net.forward_group(lrs[f:f + G], rfs[f:f + G], [[(clip_no[0], i) for i in wins[f + k]] for k in range(G)], is_first_frame=(f == 0),
                                    input_ready='materialised')
            if to_host:             # on the caller's stream, which already waits for the group's results
                for k, x in enumerate(out['result'] if name == 'none' else out['yuv']):
                    pinned[name][k].copy_(x[0], non_blocking=True)
        torch.cuda.synchronize()
        assert ('yuv' in out) == (name != 'none')
        return nfr / (time.perf_counter() - t0)
    for to_host, title in ((False, 'results left on the device'),
                           (True, "every group's output copied to pinned host memory: 'yuv' (i420 1.5 B/px, i444p10 6 B/px), or the float32 'result' (12 B/px)")):
        fps = dict((k, []) for k in nets)
        for name in nets:
            one_pass(name, to_host)
        gc.collect()
        gc.disable()
        try:
            for _ in range(passes):
                for name in nets:
                    fps[name].append(one_pass(name, to_host))
        finally:
            gc.enable()
        say('-- ' + title)
        for name, label in (('none', 'result_yuv = None     '), ('i420', "result_yuv = 'i420'   "), ('i444p10', "result_yuv = 'i444p10'")):
            say('frames/s  %s %s  median %.1f' % (label, ' '.join('%.1f' % x for x in fps[name]), med(fps[name])))
        say("i444p10 / None %.3f, i420 / None %.3f; spread of the None passes %.1f frames/s, of the i444p10 passes %.1f" % (
            med(fps['i444p10']) / med(fps['none']), med(fps['i420']) / med(fps['none']), max(fps['none']) - min(fps['none']),
            max(fps['i444p10']) - min(fps['i444p10'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--only', default='123', help='which measurements to run, e.g. 1')
    ap.add_argument('--parent', default='build/parent/refvsr_amd/librefvsr_hip.so', help="the parent commit's built library (measurement 2)")
    args = ap.parse_args()
    say('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    lib, st = hip.lib(), ops._stream()
    for key, fn in (('1', lambda: (kernels_in(lib, st), kernels_out(lib, st))), ('2', lambda: parent_ab(lib, args.parent, st)), ('3', frame_rate)):
        if key in args.only:
            fn()
            if args.out:                                           # (kept current: a later step that fails loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'w') as f:
                    f.write('\n'.join(_out) + '\n')


if __name__ == '__main__':
    main()
