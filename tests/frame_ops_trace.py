"""The frame-level wrappers of refvsr_amd.ops on the CPU (tests/test_frame_ops_trace.py): which library calls each public function
makes -- names, scalar arguments, pointer tables, chunking, cached workspaces -- what it returns, and every refusal, type and message.

The real functions run on CPU memory under three substitutions, installed by `tracing()` and removed in its `finally`:
  * device tensors are CPU tensors of a subclass whose is_cuda is True (Cuda); the name `torch` as ops sees it is a proxy whose
    empty / ones / zeros / empty_like / from_numpy return such tensors and note them as 'm<k>' (k counts over one case);
  * hip.lib() is a stand-in: every launch returns 0 and logs its name and arguments -- a pointer as '<tensor>+<byte offset>', a
    pointer table as 'T<n>[..]' of such entries, runs folded -- never an address; the pure host queries (HOST_QUERIES) go to the real
    library, which loads without a GPU, and are logged with their result;
  * ops._stream() returns a fixed handle ('stream<k>'; a case switches it with the pseudo-call 'stream').
A tensor is named after the caller's argument it belongs to ('a0', 'a1[3]', 'a0[2].1': position, list index, pair member) or after
the allocation ('m<k>'); a copy that ops makes of an argument (clone, contiguous) counts as an allocation.

Recording (from the root of the tree whose ops.py is to be pinned):
    python tests/frame_ops_trace.py tests/golden/frame_ops_calls.json [commit]
Host cost of three wrappers under the stand-in (2000 calls, 5 repeats each):
    python tests/frame_ops_trace.py --time [calls repeats]
"""
import collections
import contextlib
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_QUERIES = ('refvsr_score_workspace_bytes', 'refvsr_score_regions_workspace_bytes', 'refvsr_conf_colormap_workspace_bytes',
                'refvsr_param_fingerprint_workspace_bytes', 'refvsr_luma_sad_workspace_bytes', 'refvsr_jpeg_workspace_bytes',
                'refvsr_jpeg_capacity', 'refvsr_yuv_frame_bytes', 'refvsr_yuv420_bytes', 'refvsr_ingest_table', 'refvsr_colormap_table')
CACHES = ('_SCORE_WS', '_REGION_WS', '_SAD_WS', '_COLORMAP_WS', '_RESIZE_TAPS', '_JPEG_TABLES')
STREAMS = [0x1000 + 0x100 * k for k in range(20)]
REFUSALS = (RuntimeError, AssertionError, ValueError, TypeError, IndexError, AttributeError)


class Cuda(torch.Tensor):                         # (the wrappers ask is_cuda; nothing here touches a device)
    is_cuda = True

    def clone(self, *a, **kw):
        return T.adopt(super().clone(*a, **kw))

    def contiguous(self, *a, **kw):
        r = super().contiguous(*a, **kw)
        return r if r is self or _base(r) == _base(self) else T.adopt(r)


def cuda(t):
    return t.as_subclass(Cuda)


def _base(t):
    return t.untyped_storage().data_ptr()


def _what(t):
    return ('%s%s/%s' % (str(t.dtype).split('.')[1], list(t.shape), list(t.stride()))).replace(' ', '')


class Trace(object):
    """The state of one case: the known memory (name, first byte, bytes; the tensors are kept alive, so no address comes twice), the
    log, the current stream handle."""

    def __init__(self, quiet=False):
        self.quiet = quiet                         # the timing runs: nothing is noted or logged
        self.reset()

    def reset(self):
        self.regions, self.keep, self.log, self.made, self.stream = [], [], [], 0, STREAMS[0]

    def note(self, name, t):
        st = t.untyped_storage()
        if st.nbytes() and not any(b == st.data_ptr() for _, b, _ in self.regions):
            self.regions.append((name, st.data_ptr(), st.nbytes()))
            self.keep.append(t)

    def adopt(self, t, how='copy'):
        """A tensor ops made itself: it becomes 'm<k>'."""
        t = cuda(t)
        if not self.quiet:
            name = 'm%d' % self.made
            self.made += 1
            self.note(name, t)
            self.log.append('%s = %s %s' % (name, how, _what(t)))
        return t

    def note_args(self, name, x):
        if isinstance(x, torch.Tensor):
            self.note(name, x)
        elif isinstance(x, tuple):
            for i, v in enumerate(x):
                self.note_args('%s.%d' % (name, i), v)
        elif isinstance(x, list):
            for i, v in enumerate(x):
                self.note_args('%s[%d]' % (name, i), v)

    def where(self, addr):
        """(name, byte offset) of an address."""
        if not addr:
            return ('null', 0)
        if addr in STREAMS:
            return ('stream%d' % STREAMS.index(addr), 0)
        for name, b, n in self.regions:
            if b <= addr < b + n:
                return (name, addr - b)
        return ('?', 0)

    def table(self, addrs):
        """A pointer table, runs folded: 'a0[0..15]+0' (consecutive list members at one offset), 'm1+0:192x16' (16 entries 192 bytes
        apart in one tensor)."""
        ent, out, i = [self.where(a) for a in addrs], [], 0
        while i < len(ent):
            name, off = ent[i]
            m = re.match(r'^(.*)\[(\d+)\]((?:\.\d+)?)$', name)
            j = i + 1
            if m:
                stem, k0, member = m.group(1), int(m.group(2)), m.group(3)
                while j < len(ent) and ent[j] == ('%s[%d]%s' % (stem, k0 + j - i, member), off):
                    j += 1
                if j - i > 2:
                    out.append('%s[%d..%d]%s+%d' % (stem, k0, k0 + j - i - 1, member, off))
                    i = j
                    continue
                j = i + 1
            if j < len(ent) and ent[j][0] == name:
                step = ent[j][1] - off
                while j < len(ent) and ent[j] == (name, off + (j - i) * step):
                    j += 1
                if j - i > 2:
                    out.append('%s+%d:%dx%d' % (name, off, step, j - i))
                    i = j
                    continue
            out.append('%s+%d' % (name, off))
            i += 1
        return 'T%d[%s]' % (len(ent), ' '.join(out))

    def arg(self, a):
        if a is None:
            return 'null'
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return self.table([a[i] for i in range(len(a))])
            return '[%s]' % ' '.join('%.17g' % v if isinstance(v, float) else str(v) for v in a)
        if isinstance(a, C.c_void_p):
            name, off = self.where(a.value)
            return name if name == 'null' or name.startswith('stream') else '%s+%d' % (name, off)
        return '%.9g' % a if isinstance(a, float) else repr(a)

    def describe(self, x):
        """A returned value: a tensor is where it lies and what it is."""
        if isinstance(x, torch.Tensor):
            return '%s+%d %s' % (self.where(x.data_ptr()) + (_what(x),))
        if isinstance(x, (list, tuple)):
            return [type(x).__name__] + [self.describe(v) for v in x]
        return repr(x)


T = Trace()


class Lib(object):
    """Stands in for the ctypes handle of hip.lib()."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if not name.startswith('refvsr_'):
            raise AttributeError(name)
        if name in HOST_QUERIES:
            fn = getattr(self._real(), name)

            def query(*args):
                r = fn(*args)
                if not T.quiet:
                    T.log.append('%s(%s) -> %s' % (name, ', '.join(T.arg(a) for a in args if not isinstance(a, C.Array)), r))
                return r
            return query

        def launch(*args):
            if not T.quiet:
                T.log.append('%s(%s)' % (name, ', '.join(T.arg(a) for a in args)))
            return 0
        return launch


class TorchProxy(object):
    """Stands in for the module `torch` inside refvsr_amd.ops (as tests/footprint.py:TorchProxy): the allocation calls give Cuda
    tensors that the trace knows."""

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        return T.adopt(torch.zeros(*size, **kw), 'empty')

    def zeros(self, *size, **kw):
        return T.adopt(torch.zeros(*size, **kw), 'zeros')

    def ones(self, *size, **kw):
        return T.adopt(torch.ones(*size, **kw), 'ones')

    def empty_like(self, x, **kw):
        return T.adopt(torch.zeros_like(x, **kw), 'empty_like')

    def from_numpy(self, a):
        return T.adopt(torch.from_numpy(a), 'from_numpy')


@contextlib.contextmanager
def tracing(quiet=False):
    """The three substitutions, and the six module caches emptied; everything is put back on the way out."""
    global T
    from refvsr_amd import hip, ops
    real_lib, real_torch, real_stream = hip.lib, ops.torch, ops._stream
    assert real_torch is torch, 'refvsr_amd.ops.torch is already replaced'
    held = [(getattr(ops, n), dict(getattr(ops, n))) for n in CACHES]
    T = Trace(quiet)
    lib = Lib(real_lib)
    try:
        hip.lib, ops.torch, ops._stream = (lambda: lib), TorchProxy(), (lambda: C.c_void_p(T.stream))
        for cache, _ in held:
            cache.clear()
        yield ops
    finally:
        hip.lib, ops.torch, ops._stream = real_lib, real_torch, real_stream
        for cache, was in held:
            cache.clear()
            cache.update(was)
        T = Trace()


# ---------------------------------------------------------------------------------------------------------------- inputs
F32, F16, U8, U16, F64, I64 = torch.float32, torch.float16, torch.uint8, torch.uint16, torch.float64, torch.int64
COUNTS = (1, 16, 17, 35)                          # 1, MAX, MAX + 1, 2 MAX + 3 of every *_MAX_* constant of the frame ops (16)
PAIR_COUNTS = (1, 32, 33, 67)                     # the same of the 32 pairs of buffers_equal / bytes_equal


def z(shape, dt=F32):
    return cuda(torch.zeros(shape, dtype=dt))


def frames(b, h, w, dt=F32, hwc=False, as_list=False):
    """b frames [3, h, w]: one [b, 3, h, w] tensor or a list of separate tensors, planar or the channels-last view."""
    if as_list:
        return [z((h, w, 3), dt).permute(2, 0, 1) if hwc else z((3, h, w), dt) for _ in range(b)]
    return z((b, h, w, 3), dt).permute(0, 3, 1, 2) if hwc else z((b, 3, h, w), dt)


def strided(shape, dt=F32):
    """A tensor of the shape whose last dimension has stride 2."""
    return z(tuple(shape[:-1]) + (2 * shape[-1],), dt)[..., ::2]


def misaligned(shape, dt=U8):
    n = int(np.prod(shape))
    return z((n + 1,), dt)[1:].view(shape)


def yuvf(b, rows, w, dt=U8, as_list=False):
    return [z((rows, w), dt) for _ in range(b)] if as_list else z((b, rows, w), dt)


def pairs(b, src, dst=None):
    """[(src frame, dst float32 [3,h,w])] over the frames of src (a tensor or a list); dst frames of one [b, 3, h, w] tensor."""
    src = list(src)
    h, w = dst if dst else src[0].shape[1:]
    return list(zip(src, z((b, 3, h, w))))


def cases():
    """name -> [(function name | 'stream' | 'table', args, kwargs)]: the calls of one case, made in order on emptied caches."""
    cs = collections.OrderedDict()

    def add(name, *calls):
        assert name not in cs, name
        cs[name] = [(c[0], c[1], c[2] if len(c) > 2 else {}) for c in calls]

    # ---- buffers_equal, bytes_equal
    for n in PAIR_COUNTS:
        add('buffers_equal %d pairs' % n, ('buffers_equal', ([(z((3, 8, 8)), z((3, 8, 8))) for _ in range(n)],)))
        add('bytes_equal %d pairs' % n, ('bytes_equal', ([(a, b) for a, b in zip(frames(n, 8, 8, U8), frames(n, 8, 8, U8, as_list=True))],)))
    add('buffers_equal no pairs', ('buffers_equal', ([],)))
    add('buffers_equal two shapes in a pair', ('buffers_equal', ([(z((3, 8, 8)), z((3, 8, 12)))],)))
    add('buffers_equal second pair of another size', ('buffers_equal', ([(z((3, 8, 8)), z((3, 8, 8))), (z((3, 8, 12)), z((3, 8, 12)))],)))
    add('buffers_equal float16', ('buffers_equal', ([(z((3, 8, 8), F16), z((3, 8, 8), F16))],)))
    add('buffers_equal strided', ('buffers_equal', ([(strided((3, 8, 8)), z((3, 8, 8)))],)))
    add('bytes_equal channels-last and uint16', ('bytes_equal', ([(a, b) for a, b in zip(frames(2, 8, 12, U8, True), frames(2, 8, 12, U8, True, True))],)),
        ('bytes_equal', ([(z((12, 8), U16), z((12, 8), U16))],)))
    add('bytes_equal float32', ('bytes_equal', ([(z((3, 8, 8)), z((3, 8, 8)))],)))
    add('bytes_equal strided', ('bytes_equal', ([(strided((3, 8, 8), U8), z((3, 8, 8), U8))],)))
    add('bytes_equal uint8 against uint16', ('bytes_equal', ([(z((3, 8, 8), U8), z((3, 8, 4), U16))],)))

    # ---- ingest_u8, ingest_frames
    for n in COUNTS:
        add('ingest_u8 %d planar' % n, ('ingest_u8', (pairs(n, frames(n, 8, 12, U8)),)))
        add('ingest_frames %d frames' % n, ('ingest_frames', (z((n, 3, 8, 12), U8),)))
    mixed = [f for ab in zip(frames(17, 8, 12, U8, as_list=True), frames(17, 8, 12, U8, True)) for f in ab]
    add('ingest_u8 both layouts mixed', ('ingest_u8', (pairs(34, mixed),)))
    add('ingest_u8 no pairs', ('ingest_u8', ([],)))
    add('ingest_u8 strided source', ('ingest_u8', (pairs(1, [strided((3, 8, 8), U8)]),)))
    add('ingest_u8 float source', ('ingest_u8', (pairs(1, [z((3, 8, 8))]),)))
    add('ingest_u8 source of another size', ('ingest_u8', (pairs(2, [z((3, 8, 8), U8), z((3, 8, 12), U8)]),)))
    add('ingest_u8 float16 destination', ('ingest_u8', ([(z((3, 8, 8), U8), z((3, 8, 8), F16))],)))
    add('ingest_u8 destination of another size', ('ingest_u8', ([(z((3, 8, 8), U8), z((3, 8, 8))), (z((3, 8, 8), U8), z((3, 8, 12)))],)))
    add('ingest_u8 host destination', ('ingest_u8', ([(z((3, 8, 8), U8), torch.zeros((3, 8, 8)))],)))
    add('ingest_frames [2, 3, 3, h, w]', ('ingest_frames', (z((2, 3, 3, 8, 12), U8),)))
    add('ingest_frames [3, h, w]', ('ingest_frames', (z((3, 8, 12), U8),)))
    add('ingest_frames channels-last', ('ingest_frames', (frames(3, 8, 12, U8, True),)))
    add('ingest_frames channels-last window [2, 3, 3, h, w]', ('ingest_frames', (z((2, 3, 8, 12, 3), U8).permute(0, 1, 4, 2, 3),)))
    add('ingest_frames strided', ('ingest_frames', (strided((3, 3, 8, 12), U8),)))
    add('ingest_frames misaligned', ('ingest_frames', (misaligned((3, 3, 8, 12)),)))
    add('ingest_frames misaligned channels-last', ('ingest_frames', (misaligned((3, 8, 12, 3)).permute(0, 3, 1, 2),)))
    add('ingest_frames float32', ('ingest_frames', (z((3, 3, 8, 12)),)))
    add('ingest_frames [h, w]', ('ingest_frames', (z((8, 12), U8),)))
    add('ingest_frames four channels', ('ingest_frames', (z((2, 4, 8, 12), U8),)))
    add('ingest_frames host', ('ingest_frames', (torch.zeros((2, 3, 8, 12), dtype=U8),)))

    # ---- score_frames, score_regions
    for n in COUNTS:
        for as_list in (False, True):
            add('score_frames %d %s' % (n, 'list' if as_list else 'tensor'), ('score_frames', (frames(n, 8, 12, as_list=as_list), frames(n, 8, 12, as_list=as_list))))
        add('score_regions %d' % n, ('score_regions', (frames(n, 8, 12), frames(n, 8, 12), [(0, 8, 0, 12), (1, 7, 2, 9)])))
    for dt in (F32, F16, U8):
        for hwc in (False, True):
            for gdt, ghwc in ((F32, False), (U8, False), (U8, True)):
                add('score_frames %s %s against %s %s' % (dt, 'hwc' if hwc else 'chw', gdt, 'hwc' if ghwc else 'chw'),
                    ('score_frames', (frames(2, 8, 12, dt, hwc), frames(2, 8, 12, gdt, ghwc, as_list=True))))
    for down in (1, 2, 4):
        for win in (7, 0):
            add('score_frames down %d win %d' % (down, win), ('score_frames', (frames(17, 8 * down, 12 * down, U8, True), frames(17, 8, 12)), dict(win=win, down=down)))
    add('score_frames down 3', ('score_frames', (frames(1, 24, 24), frames(1, 8, 8)), dict(down=3)))
    add('score_frames no frames', ('score_frames', ([], [])))
    add('score_frames more results than ground truths', ('score_frames', (frames(2, 8, 8), frames(1, 8, 8))))
    add('score_frames float64 results of another shape', ('score_frames', (frames(1, 8, 12, F64), frames(1, 8, 8))))
    add('score_frames float16 ground truth', ('score_frames', (frames(1, 8, 8), frames(1, 8, 8, F16))))
    add('score_frames two shapes', ('score_frames', (frames(1, 8, 12), frames(1, 8, 8))))
    add('score_frames second pair of another shape', ('score_frames', ([z((3, 8, 8)), z((3, 8, 12))], [z((3, 8, 8)), z((3, 8, 12))])))
    add('score_frames down 2 against results of the same size', ('score_frames', (frames(1, 8, 8), frames(1, 8, 8)), dict(down=2)))
    add('score_frames host results', ('score_frames', (torch.zeros((1, 3, 8, 8)), frames(1, 8, 8))))
    add('score_frames two result dtypes', ('score_frames', ([z((3, 8, 8)), z((3, 8, 8), F16)], frames(2, 8, 8))))
    add('score_frames strided results', ('score_frames', (strided((1, 3, 8, 8)), frames(1, 8, 8))))
    add('score_frames two result layouts', ('score_frames', (frames(1, 8, 8, as_list=True) + frames(1, 8, 8, hwc=True, as_list=True), frames(2, 8, 8))))
    add('score_frames strided result and strided ground truth', ('score_frames', (strided((1, 3, 8, 8)), strided((1, 3, 8, 8)))))
    add('score_frames strided ground truth in the first pair, strided result in the second',
        ('score_frames', ([z((3, 8, 8)), strided((3, 8, 8))], [strided((3, 8, 8)), z((3, 8, 8))])))
    add('score_frames strided result in the first pair, pairs of another shape in the second',
        ('score_frames', ([strided((3, 8, 8)), z((3, 8, 12))], [z((3, 8, 8)), z((3, 8, 12))])))
    add('score_frames strided ground truth', ('score_frames', (frames(1, 8, 8), strided((1, 3, 8, 8)))))
    add('score_frames two ground-truth layouts', ('score_frames', (frames(2, 8, 8), frames(1, 8, 8, U8, as_list=True) + frames(1, 8, 8, U8, True, True))))
    add('score_frames 6 x 8', ('score_frames', (frames(1, 6, 8), frames(1, 6, 8))))
    add('score_frames down 2 of 6 x 8', ('score_frames', (frames(1, 12, 16), frames(1, 6, 8)), dict(down=2)))
    for nr in (0, 1, 8):
        add('score_regions %d rectangles' % nr, ('score_regions', (frames(17, 8, 12, F16, True), frames(17, 8, 12, U8, True), [(r, 8, 0, 12 - r) for r in range(nr)])))
    add('score_regions a rectangle of three numbers', ('score_regions', (frames(1, 8, 8), frames(1, 8, 8), [(0, 8, 0)])))
    add('score_regions no frames', ('score_regions', ([], [], [(0, 8, 0, 8)])))
    add('score_regions two shapes', ('score_regions', (frames(1, 8, 12), frames(1, 8, 8), [(0, 8, 0, 8)])))
    add('score_regions strided results', ('score_regions', (strided((1, 3, 8, 8)), frames(1, 8, 8), [(0, 8, 0, 8)])))
    add('score_regions 8 x 6', ('score_regions', (frames(1, 8, 6), frames(1, 8, 6), [(0, 8, 0, 6)])))

    # ---- result_to_yuv420, result_to_yuv, result_yuv, resize_aa: the result-frame check and its chunk walk
    takers = (('result_to_yuv420', ()), ('result_to_yuv', ()), ('resize_aa', (4, 6)))
    for fn, tail in takers:
        for n in COUNTS:
            for as_list in (False, True):
                add('%s %d %s' % (fn, n, 'list' if as_list else 'tensor'), (fn, (frames(n, 8, 12, as_list=as_list),) + tail))
        for dt in (F32, F16, U8):
            for hwc in (False, True):
                add('%s %s %s' % (fn, dt, 'hwc' if hwc else 'chw'), (fn, (frames(2, 8, 12, dt, hwc),) + tail))
        add('%s no frames' % fn, (fn, ([],) + tail))
        add('%s float64 [h, w] frames' % fn, (fn, ([z((8, 12), F64)],) + tail))
        add('%s float64' % fn, (fn, (frames(1, 8, 12, F64),) + tail))
        add('%s [1, 3, h, w] frames' % fn, (fn, ([z((1, 3, 8, 12))],) + tail))
        add('%s four channels' % fn, (fn, (z((1, 4, 8, 12)),) + tail))
        add('%s host' % fn, (fn, (torch.zeros((1, 3, 8, 12)),) + tail))
        add('%s second frame of another shape' % fn, (fn, ([z((3, 8, 12)), z((3, 8, 8))],) + tail))
        add('%s second frame of another dtype' % fn, (fn, ([z((3, 8, 12)), z((3, 8, 12), F16)],) + tail))
        add('%s second frame on the host' % fn, (fn, ([z((3, 8, 12)), torch.zeros((3, 8, 12))],) + tail))
        add('%s strided' % fn, (fn, (strided((2, 3, 8, 12)),) + tail))
        add('%s second frame strided and of another shape' % fn, (fn, ([z((3, 8, 12)), strided((3, 8, 8))],) + tail))
        add('%s first frame strided and second of another shape' % fn, (fn, ([strided((3, 8, 12)), z((3, 8, 8))],) + tail))
        add('%s two layouts' % fn, (fn, (frames(1, 8, 12, as_list=True) + frames(1, 8, 12, hwc=True, as_list=True),) + tail))
    for fn in ('result_to_yuv420', 'result_to_yuv'):
        add('%s odd h' % fn, (fn, (frames(1, 7, 12),)))
        add('%s odd w and strided' % fn, (fn, (strided((1, 3, 8, 7)),)))
        add('%s unknown matrix and no frames' % fn, (fn, ([],), dict(matrix='bt2020')))
        add('%s unknown range' % fn, (fn, (frames(1, 8, 12),), dict(range='tv')))
        add('%s unknown format' % fn, (fn, (frames(1, 8, 12),), dict(fmt='yv12')))
        add('%s 2 x 2' % fn, (fn, (frames(3, 2, 2, U8, True),)))
    for fmt in ('nv12', 'i420', 'p010', 'i420p10'):
        add('result_to_yuv420 %s bt601 full' % fmt, ('result_to_yuv420', (frames(2, 2, 2), fmt, 'bt601', 'full')))
        add('result_to_yuv %s left' % fmt, ('result_to_yuv', (frames(2, 2, 2), fmt), dict(siting='left')))
        add('result_to_yuv %s centre' % fmt, ('result_to_yuv', (frames(2, 2, 2), fmt)))
    add('result_to_yuv420 i422', ('result_to_yuv420', (frames(1, 8, 12), 'i422')))
    for fmt in ('i422', 'i444', 'i422p10', 'i444p10'):
        add('result_to_yuv %s' % fmt, ('result_to_yuv', (frames(2, 2, 2, F16), fmt, 'bt601', 'full', 'left')))
    add('result_to_yuv unknown siting and no frames', ('result_to_yuv', ([],), dict(siting='top')))
    add('result_to_yuv i422 odd w', ('result_to_yuv', (frames(1, 8, 7), 'i422')))
    add('result_to_yuv i444 odd w', ('result_to_yuv', (frames(1, 8, 7), 'i444')))
    for params in (('nv12', 'bt709', 'limited'), ('i420p10', 'bt601', 'full'), ('i422', 'bt709', 'limited'), ('i444', 'bt709', 'full')):
        for siting in ('centre', 'left'):
            add('result_yuv %s %s' % (' '.join(params), siting), ('result_yuv', (frames(17, 2, 2, U8), params, siting)))
    add('result_yuv no frames', ('result_yuv', ([], ('nv12', 'bt709', 'limited'))))
    add('result_yuv unknown siting', ('result_yuv', (frames(1, 2, 2), ('nv12', 'bt709', 'limited'), 'top')))
    for out in ('float32', 'uint8'):
        for clamp in (True, False):
            add('resize_aa %s clamp %s' % (out, clamp), ('resize_aa', (frames(17, 8, 12, U8, True), 12, 8), dict(out=out, clamp=clamp)))
    add('resize_aa up', ('resize_aa', (frames(2, 8, 12), 20, 31)))
    add('resize_aa float16 output and no frames', ('resize_aa', ([], 4, 6), dict(out='float16')))
    add('resize_aa ratio 9 and strided', ('resize_aa', (strided((1, 3, 9, 8)), 1, 8)))
    add('resize_aa ratio 9 across', ('resize_aa', (frames(1, 8, 18), 8, 2)))
    add('resize_aa zero output', ('resize_aa', (frames(1, 8, 12), 0, 6)))
    add('resize_aa float sizes', ('resize_aa', (frames(1, 8, 12), 4.0, 6)))
    add('resize_aa sizes of another kind', ('resize_aa', (frames(1, 8, 12), None, 'x')))

    # ---- yuv420_ingest, yuv_ingest, yuv_decode, yuv420_to_frames, yuv_to_frames
    for n in COUNTS:
        for as_list in (False, True):
            add('yuv420_ingest %d %s' % (n, 'list' if as_list else 'tensor'), ('yuv420_ingest', (pairs(n, yuvf(n, 3, 2, as_list=as_list), (2, 2)),)))
            add('yuv_ingest %d %s' % (n, 'list' if as_list else 'tensor'), ('yuv_ingest', (pairs(n, yuvf(n, 4, 2, as_list=as_list), (2, 2)),)))
        add('yuv420_to_frames %d' % n, ('yuv420_to_frames', (yuvf(n, 12, 12), 8, 12, 'nv12')))
        add('yuv_to_frames %d' % n, ('yuv_to_frames', (yuvf(n, 16, 12), 8, 12, 'i422')))
    for fmt in ('nv12', 'i420', 'p010', 'i420p10'):
        dt = U8 if fmt in ('nv12', 'i420') else U16
        add('yuv420_ingest %s bt601 full nearest' % fmt, ('yuv420_ingest', (pairs(2, yuvf(2, 3, 2, dt), (2, 2)), fmt, 'bt601', 'full', 'nearest')))
        add('yuv_ingest %s left' % fmt, ('yuv_ingest', (pairs(2, yuvf(2, 3, 2, dt), (2, 2)), fmt), dict(siting='left')))
        add('yuv_ingest %s centre' % fmt, ('yuv_ingest', (pairs(2, yuvf(2, 3, 2, dt), (2, 2)), fmt)))
        add('yuv420_to_frames %s [2, 2, rows, w]' % fmt, ('yuv420_to_frames', (z((2, 2, 3, 2), dt), 2, 2, fmt, 'bt601', 'full', 'nearest')))
        add('yuv_to_frames %s left' % fmt, ('yuv_to_frames', (z((2, 3, 2), dt), 2, 2, fmt), dict(siting='left')))
    for fmt, rows in (('i422', 4), ('i444', 6), ('i422p10', 4), ('i444p10', 6)):
        dt = U16 if fmt.endswith('p10') else U8
        add('yuv_ingest %s' % fmt, ('yuv_ingest', (pairs(2, yuvf(2, rows, 2, dt), (2, 2)), fmt, 'bt601', 'full', 'nearest', 'left')))
        add('yuv_to_frames %s' % fmt, ('yuv_to_frames', (z((2, rows, 2), dt), 2, 2, fmt, 'bt601', 'full', 'nearest', 'left')))
        add('yuv_decode %s' % fmt, ('yuv_decode', (pairs(2, yuvf(2, rows, 2, dt), (2, 2)), (fmt, 'bt709', 'limited', 'bilinear'))))
    add('yuv_decode nv12', ('yuv_decode', (pairs(17, yuvf(17, 3, 2), (2, 2)), ('nv12', 'bt709', 'limited', 'bilinear'))))
    add('yuv_decode nv12 centre', ('yuv_decode', (pairs(2, yuvf(2, 3, 2), (2, 2)), ('nv12', 'bt709', 'limited', 'bilinear', 'centre'))))
    add('yuv_decode nv12 left', ('yuv_decode', (pairs(2, yuvf(2, 3, 2), (2, 2)), ('nv12', 'bt709', 'limited', 'bilinear', 'left'))))
    for fn, rows in (('yuv420_ingest', 3), ('yuv_ingest', 4)):
        add('%s no pairs and unknown chroma' % fn, (fn, ([],), dict(chroma='bicubic')))
        add('%s unknown chroma' % fn, (fn, (pairs(1, yuvf(1, rows, 2), (2, 2)),), dict(chroma='bicubic')))
        add('%s unknown matrix' % fn, (fn, (pairs(1, yuvf(1, rows, 2), (2, 2)),), dict(matrix='bt2020')))
        add('%s uint16 frames' % fn, (fn, (pairs(1, yuvf(1, rows, 2, U16), (2, 2)),)))
        add('%s frames of another size' % fn, (fn, (pairs(1, yuvf(1, 2 * rows, 4), (2, 2)),)))
        add('%s strided frames' % fn, (fn, (pairs(1, [strided((rows, 2), U8)], (2, 2)),)))
        add('%s float16 destination' % fn, (fn, ([(z((rows, 2), U8), z((3, 2, 2), F16))],)))
        add('%s second destination of another size' % fn, (fn, ([(z((rows, 2), U8), z((3, 2, 2))), (z((rows, 2), U8), z((3, 2, 4)))],)))
    add('yuv_ingest unknown siting', ('yuv_ingest', (pairs(1, yuvf(1, 4, 2), (2, 2)),), dict(siting='top')))
    for fn, fmt, rows in (('yuv420_to_frames', 'nv12', 3), ('yuv_to_frames', 'i422', 4)):
        add('%s [rows, w]' % fn, (fn, (z((rows, 2), U8), 2, 2, fmt)))
        add('%s strided' % fn, (fn, (strided((3, rows, 2), U8), 2, 2, fmt)))
        add('%s misaligned' % fn, (fn, (misaligned((3, rows, 2)), 2, 2, fmt)))
        add('%s uint16' % fn, (fn, (z((3, rows, 2), U16), 2, 2, fmt)))
        add('%s frames of another size' % fn, (fn, (z((3, rows, 2), U8), 4, 2, fmt)))
        add('%s [w]' % fn, (fn, (z((2,), U8), 2, 2, fmt)))
        add('%s host' % fn, (fn, (torch.zeros((3, rows, 2), dtype=U8), 2, 2, fmt)))
    add('yuv_to_frames unknown siting', ('yuv_to_frames', (z((3, 4, 2), U8), 2, 2, 'i422'), dict(siting='top')))
    add('yuv_to_frames p010 strided', ('yuv_to_frames', (strided((3, 3, 2), U16), 2, 2, 'p010')))

    # ---- jpeg_encode_device
    for n in COUNTS:
        add('jpeg_encode_device %d tensor' % n, ('jpeg_encode_device', (yuvf(n, 12, 8), 8, 8, 'i420')))
        add('jpeg_encode_device %d list' % n, ('jpeg_encode_device', (yuvf(n, 24, 8, as_list=True), 8, 8, 'i444')))
    add('jpeg_encode_device [rows, w]', ('jpeg_encode_device', (z((12, 8), U8), 8, 8, 'i420')))
    add('jpeg_encode_device [2, 2, rows, w] quality 50 restart 1', ('jpeg_encode_device', (z((2, 2, 12, 8), U8), 8, 8, 'i420', 50, 1)))
    add('jpeg_encode_device 8 x 12', ('jpeg_encode_device', (z((2, 12, 12), U8), 8, 12, 'i420'), dict(restart=7)))
    add('jpeg_encode_device nv12, quality 0', ('jpeg_encode_device', (z((1, 12, 8), U8), 8, 8, 'nv12', 0)))
    add('jpeg_encode_device quality 0, restart 0', ('jpeg_encode_device', (z((1, 12, 8), U8), 8, 8, 'i420', 0, 0)))
    add('jpeg_encode_device restart 0, float h', ('jpeg_encode_device', (z((1, 12, 8), U8), 8.0, 8, 'i420', 90, 0)))
    add('jpeg_encode_device bool w, no frames', ('jpeg_encode_device', ([], 8, True, 'i420')))
    add('jpeg_encode_device h of 65536, no frames', ('jpeg_encode_device', ([], 65536, 8, 'i420')))
    add('jpeg_encode_device tensor of another size', ('jpeg_encode_device', (z((1, 12, 12), U8), 8, 8, 'i420')))
    add('jpeg_encode_device [w] tensor', ('jpeg_encode_device', (z((8,), U8), 8, 8, 'i420')))
    add('jpeg_encode_device no frames', ('jpeg_encode_device', ([], 8, 8, 'i420')))
    add('jpeg_encode_device uint16 tensor', ('jpeg_encode_device', (z((1, 12, 8), U16), 8, 8, 'i420')))
    add('jpeg_encode_device a frame that is no tensor', ('jpeg_encode_device', ([z((12, 8), U8), None], 8, 8, 'i420')))
    add('jpeg_encode_device second frame of another size and on the host', ('jpeg_encode_device', ([z((12, 8), U8), torch.zeros((12, 12), dtype=U8)], 8, 8, 'i420')))
    add('jpeg_encode_device strided', ('jpeg_encode_device', (strided((1, 12, 8), U8), 8, 8, 'i420')))
    add('jpeg_encode_device second frame on the host', ('jpeg_encode_device', ([z((12, 8), U8), torch.zeros((12, 8), dtype=U8)], 8, 8, 'i420')))

    # ---- luma_sad, conf_colormap
    for n in COUNTS:
        add('luma_sad %d tensor' % n, ('luma_sad', (yuvf(n, 3, 2), yuvf(n, 3, 2), 2, 2, 'nv12')))
        add('luma_sad %d list' % n, ('luma_sad', (yuvf(n, 12, 12, U16, True), yuvf(n, 12, 12, U16, True), 8, 12, 'p010')))
        add('conf_colormap %d' % n, ('conf_colormap', ([z((1, 8, 12)) for _ in range(n)],)))
    w9 = z((18, 3, 2), U8)
    add('luma_sad views of one window', ('luma_sad', (w9[:17], w9[1:], 2, 2, 'i420')))
    for fmt, rows, dt in (('i420p10', 3, U16), ('i422', 4, U8), ('i444p10', 6, U16)):
        add('luma_sad %s' % fmt, ('luma_sad', (yuvf(2, rows, 2, dt), yuvf(2, rows, 2, dt), 2, 2, fmt)))
    add('luma_sad no frames', ('luma_sad', ([], [], 2, 2, 'nv12')))
    add('luma_sad two counts, odd h', ('luma_sad', (yuvf(2, 3, 2), yuvf(1, 3, 2), 3, 2, 'nv12')))
    add('luma_sad odd w, frames of another size', ('luma_sad', (yuvf(1, 3, 2), yuvf(1, 3, 2), 2, 3, 'nv12')))
    add('luma_sad 0 x 2', ('luma_sad', (yuvf(1, 3, 2), yuvf(1, 3, 2), 0, 2, 'nv12')))
    add('luma_sad frames of another size', ('luma_sad', (yuvf(1, 3, 2), yuvf(1, 6, 4), 2, 2, 'nv12')))
    add('luma_sad uint16 nv12', ('luma_sad', (yuvf(1, 3, 2, U16), yuvf(1, 3, 2, U16), 2, 2, 'nv12')))
    add('luma_sad strided', ('luma_sad', (yuvf(1, 3, 2), strided((1, 3, 2), U8), 2, 2, 'nv12')))
    add('luma_sad host', ('luma_sad', (yuvf(1, 3, 2), torch.zeros((1, 3, 2), dtype=U8), 2, 2, 'nv12')))
    add('conf_colormap [1, 1, h, w] and [h, w] maps', ('conf_colormap', ([z((1, 1, 8, 12)), z((8, 12)), z((1, 8, 12))],)))
    add('conf_colormap views of one tensor', ('conf_colormap', (z((17, 1, 8, 12)),)))
    add('conf_colormap no maps', ('conf_colormap', ([],)))
    add('conf_colormap float16 and of another size', ('conf_colormap', ([z((1, 8, 12)), z((1, 8, 8), F16)],)))
    add('conf_colormap strided', ('conf_colormap', ([strided((1, 8, 12))],)))
    add('conf_colormap [w] map', ('conf_colormap', ([z((1, 12)), z((12,))],)))
    add('conf_colormap host', ('conf_colormap', ([torch.zeros((1, 8, 12))],)))
    add('conf_colormap second map of another size', ('conf_colormap', ([z((1, 8, 12)), z((1, 8, 8))],)))
    add('conf_colormap [2, h, w] map', ('conf_colormap', ([z((2, 8, 12))],)))
    add('conf_colormap [0, w] map', ('conf_colormap', ([z((0, 12))],)))

    # ---- param_fingerprint
    ps = lambda: [z((5000,)), z((3, 7)), z((1,))]
    add('param_fingerprint list', ('param_fingerprint', (ps(),)))
    add('param_fingerprint list and out', ('param_fingerprint', (ps(), z((1,), I64))))
    add('param_fingerprint table twice, a second stream, the first again',
        ('table', (ps(),)), ('param_fingerprint', ('table',)), ('param_fingerprint', ('table', z((1,), I64))), ('stream', (1,)),
        ('param_fingerprint', ('table',)), ('stream', (0,)), ('param_fingerprint', ('table',)))
    add('param_fingerprint table on 18 streams and the first again', ('table', (ps(),)),
        *[c for k in list(range(18)) + [0] for c in (('stream', (k,)), ('param_fingerprint', ('table',)))])
    add('param_fingerprint no tensors', ('param_fingerprint', ([],)))
    add('param_fingerprint table of no tensors', ('table', ([],)))
    add('param_fingerprint float16 tensor', ('param_fingerprint', ([z((4,)), z((4,), F16)],)))
    add('param_fingerprint strided tensor', ('param_fingerprint', ([strided((4, 4))],)))
    add('param_fingerprint host tensor', ('param_fingerprint', ([z((4,)), torch.zeros((4,))],)))
    add('param_fingerprint int32 out', ('param_fingerprint', (ps(), z((1,), torch.int32))))
    add('param_fingerprint out of two', ('param_fingerprint', (ps(), z((2,), I64))))
    add('param_fingerprint host out', ('param_fingerprint', (ps(), torch.zeros((1,), dtype=I64))))

    # ---- the caches: the same call twice, the same geometry on a second stream, 18 geometries and the first again
    def cache_case(name, call):
        """call(k) -> the call of geometry k (0: the first)."""
        add('%s cache: twice, a second stream, the first stream' % name, call(0), call(0), ('stream', (1,)), call(0), ('stream', (0,)), call(0))
        add('%s cache: 18 geometries and the first again' % name, *[call(k) for k in list(range(18)) + [0, 17]])
    cache_case('score_frames', lambda k: ('score_frames', (frames(2, 8, 8 + k), frames(2, 8, 8 + k))))
    cache_case('score_regions', lambda k: ('score_regions', (frames(2, 8 + k, 8), frames(2, 8 + k, 8), [(0, 8, 0, 8)])))
    cache_case('luma_sad', lambda k: ('luma_sad', (yuvf(2, 3, 2 + 2 * k), yuvf(2, 3, 2 + 2 * k), 2, 2 + 2 * k, 'nv12')))
    cache_case('conf_colormap', lambda k: ('conf_colormap', ([z((1, 8, 8 + k))],)))
    cache_case('resize_aa', lambda k: ('resize_aa', (frames(2, 8, 8), 8, 8 + k)))
    cache_case('jpeg_encode_device', lambda k: ('jpeg_encode_device', (z((2, 12, 8), U8), 8, 8, 'i420', 90 - k)))
    add('resize_aa and jpeg_encode_device caches: the keys', ('resize_aa', (frames(1, 8, 12), 8, 12)), ('resize_aa', (frames(1, 12, 8), 8, 12)),
        ('resize_aa', (frames(1, 8, 12), 12, 8)), ('resize_aa', (frames(1, 8, 12, U8, True), 8, 12), dict(out='uint8')),
        ('jpeg_encode_device', (z((1, 12, 8), U8), 8, 8, 'i420')), ('jpeg_encode_device', (z((1, 24, 8), U8), 8, 8, 'i444')),
        ('jpeg_encode_device', (z((1, 12, 16), U8), 8, 16, 'i420')))
    add('score_frames and score_regions keep caches apart', ('score_frames', (frames(1, 8, 8), frames(1, 8, 8))),
        ('score_regions', (frames(1, 8, 8), frames(1, 8, 8), [(0, 8, 0, 8)])), ('score_frames', (frames(1, 16, 16), frames(1, 8, 8)), dict(down=2)))
    return cs


# ---------------------------------------------------------------------------------------------------------------- running
def run_case(ops, calls):
    """[{'call': .., 'log': [..], 'out': .. | 'raised': 'Type: message'}] of one case, on emptied caches."""
    T.reset()
    for n in CACHES:
        getattr(ops, n).clear()
    table, out = None, []
    for k, (fn, args, kw) in enumerate(calls):
        if fn == 'stream':
            T.stream = STREAMS[args[0]]
            continue
        T.log = []
        rec = collections.OrderedDict(call=fn)
        for i, a in enumerate(args):
            T.note_args('c%d.a%d' % (k, i) if len(calls) > 1 else 'a%d' % i, a)
        try:
            if fn == 'table':
                table = ops.FingerprintTable(*args)
                res = [table.nchunks, list(table.pointers) == [t.data_ptr() for t in table.tensors], T.describe(table.chunks)]
            else:
                res = T.describe(getattr(ops, fn)(*[table if isinstance(a, str) and a == 'table' else a for a in args], **kw))
            rec['log'], rec['out'] = T.log, res
        except REFUSALS as e:
            rec['log'], rec['raised'] = T.log, '%s: %s' % (type(e).__name__, e)
        out.append(rec)
    return out


def record():
    """{case: run_case(..)} of every case, under the substitutions."""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    with tracing() as ops:
        return collections.OrderedDict((name, run_case(ops, calls)) for name, calls in cases().items())


def dumps(rec, src):
    """The golden file's text: a line per case."""
    return '{"_recorded_from": %s,\n"cases": {\n%s}\n}\n' % (json.dumps(src, sort_keys=True), ',\n'.join(
        '%s:%s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in rec.items()))


def load(path):
    """(what the file was recorded from, the recording, the file's text)."""
    with open(path) as fh:
        text = fh.read()
    g = json.loads(text, object_pairs_hook=collections.OrderedDict)
    return g['_recorded_from'], g['cases'], text


def host_cost(calls=2000, repeats=5):
    """Seconds per `calls` calls of three wrappers on 4 frames of 8 x 8 under the quiet stand-in: {name: [repeats numbers]}."""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    out = collections.OrderedDict()
    with tracing(quiet=True) as ops:
        a, g = frames(4, 8, 8), frames(4, 8, 8)
        for name, fn in (('score_frames', lambda: ops.score_frames(a, g)), ('result_to_yuv420', lambda: ops.result_to_yuv420(a)),
                         ('resize_aa', lambda: ops.resize_aa(a, 4, 4))):
            for _ in range(200):
                fn()
            out[name] = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                out[name].append(time.perf_counter() - t0)
    return out


def main(argv):
    if argv[1] == '--time':
        calls, repeats = [int(v) for v in argv[2:4]] if len(argv) > 3 else (2000, 5)
        for name, ts in host_cost(calls, repeats).items():
            ts = sorted(ts)
            print('%-18s %d calls, %d repeats [ms]: %s   median %.2f  spread (max - min) %.2f' % (
                name, calls, repeats, ' '.join('%.2f' % (1e3 * t) for t in ts), 1e3 * ts[len(ts) // 2], 1e3 * (ts[-1] - ts[0])))
        return
    rec = record()
    commit = argv[2] if len(argv) > 2 else subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT).decode().strip()
    with open(argv[1], 'w') as fh:
        fh.write(dumps(rec, dict(commit=commit, file='refvsr_amd/ops.py')))
    print('%d cases, %d calls recorded from %s -> %s' % (len(rec), sum(len(v) for v in rec.values()), commit[:12], argv[1]))


if __name__ == '__main__':
    main(sys.argv)
