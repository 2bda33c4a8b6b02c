"""Memory fences for the kernel suites: does a launch touch only its own memory?

The exact suites prove values.  This module lets them prove, with one more launch per case, that a kernel (1) writes nothing before
or behind its outputs and scratch maps, (2) does not compute with what lies before or behind its inputs, and (3) does not depend on
its pointers sitting at the start of an allocation.

fenced_input(t_cpu, dev, poison)   a dense device view of t_cpu inside a larger flat buffer of the same dtype.  The lead and the
    tail each take fence_bytes(bytes of the tensor) = max(bytes, 64 KiB) rounded up to a multiple of 256 bytes, so the view keeps
    the 16-byte alignment the blobs and the vector loads need.  poison='nan' fills both fences with quiet NaN (all-ones bytes for
    integer dtypes: a NaN read as fp16 or fp32): for data that enters arithmetic, where a read past the map then shows up as a NaN in
    the result.  poison='benign' fills them with zeros: for anything a kernel turns into an address or a coordinate (indices,
    candidate tables, flags, flows, offsets, affine parameters), where a wild value could make an already-wrong kernel fault.  The
    benign fence moves the view off storage offset 0 and lets inputs_unchanged() see a write into it; it detects NO stray read.
inputs_unchanged()                 every buffer handed out by fenced_input since reset_inputs(): view AND fences still hold their
    initial bytes.
fenced_outputs(ops)                context manager: the name `torch` as refvsr_amd.ops sees it becomes a proxy whose empty / empty_like /
    zeros / ones return views into flat buffers with 0xA5-filled fences of the same sizing rule (the global torch module is never
    patched; the name is restored in a `finally`).  check(results=[...]) synchronises and asserts that every fence byte of every
    buffer is still 0xA5 and that EVERY result tensor lies inside a recorded buffer -- a result that reached the caller through an
    allocation the proxy does not cover fails instead of escaping.  Scratch maps allocated inside ops are fenced the same way.
fence_weights(obj)                 re-homes the device weights of an ops.ConvWeights (wpack, bias, blob24, and the descriptor's
    pointers), of a blob chain (blobs) or a bare blob tensor into NaN-fenced views.

Limits of what this proves:
  * A load past a map whose value a select discards is invisible here, and harmless unless it crosses into unmapped memory.  This
    module does not try to show that: nothing in it places a buffer against an unmapped page or otherwise invites a fault.
  * A NaN that reaches a `fminf` / `fmaxf` clamp is invisible to no_nan(): `fminf(fmaxf(NaN, 0), 1)` is 0.  The base frame of the output
    heads is the case: a read past it is detected by the bit equality with a reference whose base is not zero, not by this module.
  * A stray write farther away than one fence width (at least the output's own size, at least 64 KiB) is not seen.  The suites'
    shapes (19 x 45 and 33 x 70 maps against 4-, 8- and 16-row tiles, the 2 x 2 to 34 x 70 matching and sampling shapes) make a
    mis-strided store overrun by at most a tile's rows of the same map, which is within the fence.
  * Base pointers that are not 16-byte aligned are out of scope: fences are multiples of 256 bytes on purpose.
  * The kernels that carry their own canaries (yuv, yuv_in, jpeg, resize_aa, scene, colormap, ingest, score, result conversion)
    are not covered here.

Device-agnostic torch code: tests/test_footprint.py runs it on CPU tensors (fenced_outputs(ops, cpu=True))."""
import contextlib

import torch

FENCE_MIN = 64 << 10
FENCE_ALIGN = 256
OUT_BYTE = 0xA5
INTERCEPTED = ('empty', 'empty_like', 'zeros', 'ones')


def fence_bytes(nbytes):
    """Bytes of one fence (lead or tail) around a tensor of nbytes."""
    return (max(int(nbytes), FENCE_MIN) + FENCE_ALIGN - 1) // FENCE_ALIGN * FENCE_ALIGN


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Fenced(object):
    """A flat uint8 buffer [lead | view bytes | tail] and the typed view in its middle."""

    def __init__(self, shape, dtype, device, fill):
        esz = torch.empty((), dtype=dtype).element_size()
        self.nbytes = _numel(shape) * esz
        self.lead = self.tail = fence_bytes(self.nbytes)
        self.buf = torch.empty(self.lead + self.nbytes + self.tail, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.buf[:self.lead] = fill
        self.buf[self.lead + self.nbytes:] = fill
        self.view = self.buf[self.lead:self.lead + self.nbytes].view(dtype).view(tuple(shape))
        self.fill = fill

    def holds(self, t):
        p, v = t.data_ptr(), self.view.data_ptr()
        return t.device == self.buf.device and (v <= p < v + self.nbytes or (t.numel() == 0 and p == v))

    def damage(self):
        """[(side, first offset, last offset, value at first, count)] of fence bytes that no longer hold the fill; offsets are in
        bytes relative to the first byte of the view (negative: before it)."""
        out = []
        for side, lo, hi in (('lead', 0, self.lead), ('tail', self.lead + self.nbytes, self.buf.numel())):
            f = self.buf[lo:hi]
            bad = (f != self.fill).nonzero().flatten()
            if bad.numel():
                i0, i1 = int(bad[0]), int(bad[-1])
                out.append((side, lo + i0 - self.lead, lo + i1 - self.lead, int(f[i0]), int(bad.numel())))
        return out


def marked_buffer(t_cpu, dev):
    """A Fenced record whose view holds t_cpu between 0xA5 fences: for a buffer a test hands to the library itself and the kernel
    reads AND writes (record.damage() must stay empty)."""
    r = Fenced(tuple(t_cpu.shape), t_cpu.dtype, dev, OUT_BYTE)
    r.view.copy_(t_cpu)
    return r


# ---- inputs ---------------------------------------------------------------------------------------------------------------
_INPUTS = []


def reset_inputs():
    del _INPUTS[:]


def fenced_input(t_cpu, dev, poison):
    """A dense view on `dev` holding t_cpu, inside a flat buffer of t_cpu's dtype whose lead and tail are poisoned (see the module's
    docstring: 'nan' for data that enters arithmetic, 'benign' = zeros for anything that becomes an address or a coordinate; the
    benign fence detects no stray read, it only moves the view off storage offset 0).  Recorded for inputs_unchanged()."""
    assert poison in ('nan', 'benign'), poison
    t_cpu = t_cpu.contiguous()
    esz = t_cpu.element_size()
    n = t_cpu.numel()
    lead = fence_bytes(n * esz) // esz
    host = torch.empty(2 * lead + n, dtype=t_cpu.dtype)
    for f in (host[:lead], host[lead + n:]):
        if poison == 'benign':
            f.zero_()
        elif t_cpu.dtype.is_floating_point:
            f.fill_(float('nan'))
        else:
            f.view(torch.uint8).fill_(0xFF)                    # a quiet NaN when read as fp16 or as fp32
    host[lead:lead + n] = t_cpu.reshape(-1)
    buf = host.to(dev)
    if buf is host:                                            # CPU: keep the snapshot apart from the live buffer
        buf = host.clone()
    view = buf[lead:lead + n].view(t_cpu.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    _INPUTS.append((buf, view, lead * esz, lead * esz, host.view(torch.uint8)))
    return view


def inputs_unchanged():
    """None when every fenced input since reset_inputs() still holds its initial bytes, view and fences; else a description."""
    for k, (buf, view, lead, tail, snap) in enumerate(_INPUTS):
        now = buf.cpu().view(torch.uint8)
        if not torch.equal(now, snap):
            bad = (now != snap).nonzero().flatten()
            return 'fenced input %d %s %s: bytes %d .. %d relative to the view changed (view holds %d bytes)' % (
                k, tuple(view.shape), view.dtype, int(bad[0]) - lead, int(bad[-1]) - lead, view.numel() * view.element_size())
    return None


def fence_weights(obj):
    """Re-home device weights into NaN-fenced views, in place: an ops.ConvWeights (wpack, bias, blob24 where present; desc.wpack /
    desc.bias follow), a blob chain (.blobs: stride unchanged, 16-byte aligned) or, for a bare blob tensor, the fenced copy is
    returned.  Returns obj (or the new tensor)."""
    if isinstance(obj, torch.Tensor):
        return fenced_input(obj.cpu(), obj.device, 'nan')
    if hasattr(obj, 'blobs'):
        obj.blobs = fenced_input(obj.blobs.cpu(), obj.blobs.device, 'nan')
        assert obj.blobs.shape[1] == obj.stride and obj.blobs.data_ptr() % 16 == 0
        return obj
    for name in ('wpack', 'bias', 'blob24'):
        t = getattr(obj, name)
        if t is not None:
            setattr(obj, name, fenced_input(t.cpu(), t.device, 'nan'))
    obj.desc.wpack, obj.desc.bias = obj.wpack.data_ptr(), obj.bias.data_ptr()
    return obj


# ---- outputs --------------------------------------------------------------------------------------------------------------
class TorchProxy(object):
    """Stands in for the module `torch` inside refvsr_amd.ops: every attribute is torch's, except the allocation calls ops uses
    (INTERCEPTED), which return fenced views for CUDA results (cpu=True: for CPU results as well -- the harness's own test)."""

    def __init__(self, cpu=False):
        self._cpu = cpu
        self.records = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _fenced(self, shape, dtype, device):
        dtype = dtype or torch.get_default_dtype()
        device = torch.device(device if device is not None else 'cpu')
        if device.type == 'cuda' or (self._cpu and device.type == 'cpu'):
            r = Fenced(shape, dtype, device, OUT_BYTE)
            self.records.append(r)
            return r.view
        return None

    @staticmethod
    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], int):
            return tuple(size[0])
        return tuple(size)

    def empty(self, *size, dtype=None, device=None, **kw):
        v = self._fenced(self._shape(size), dtype, device)
        return torch.empty(*size, dtype=dtype, device=device, **kw) if v is None else v

    def empty_like(self, x, dtype=None, device=None, **kw):
        v = self._fenced(tuple(x.shape), dtype or x.dtype, device if device is not None else x.device)
        return torch.empty_like(x, dtype=dtype, device=device, **kw) if v is None else v

    def zeros(self, *size, dtype=None, device=None, **kw):
        v = self._fenced(self._shape(size), dtype, device)
        return torch.zeros(*size, dtype=dtype, device=device, **kw) if v is None else v.zero_()

    def ones(self, *size, dtype=None, device=None, **kw):
        v = self._fenced(self._shape(size), dtype, device)
        return torch.ones(*size, dtype=dtype, device=device, **kw) if v is None else v.fill_(1)


def _flatten(x):
    if x is None:
        return
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            for t in _flatten(v):
                yield t
    else:
        for v in x:
            for t in _flatten(v):
                yield t


class OutputFences(object):
    def __init__(self, proxy):
        self.proxy = proxy

    @property
    def records(self):
        return self.proxy.records

    def problems(self, results=()):
        """[description] of every damaged fence and every unfenced result (empty: all is well).  Synchronises first."""
        if any(r.buf.is_cuda for r in self.records):
            torch.cuda.synchronize()
        out = []
        for k, r in enumerate(self.records):
            for side, first, last, val, n in r.damage():
                out.append('fenced allocation %d %s %s (%d bytes): %s fence damaged, %d bytes between offsets %d and %d relative to the view, '
                           'first holds 0x%02x' % (k, tuple(r.view.shape), r.view.dtype, r.nbytes, side, n, first, last, val))
        res = list(_flatten(results))
        for k, t in enumerate(res):
            if not any(r.holds(t) for r in self.records):
                out.append('result %d of %d %s %s on %s is not inside a fenced allocation' % (k, len(res), tuple(t.shape), t.dtype, t.device))
        return out

    def check(self, results=()):
        bad = self.problems(results)
        assert not bad, '\n'.join(bad)


@contextlib.contextmanager
def fenced_outputs(ops_module, cpu=False):
    """`with fenced_outputs(ops) as fo: r = ops.something(...); fo.check(results=[r])`: see the module's docstring."""
    real = ops_module.torch
    assert real is torch, 'refvsr_amd.ops.torch is already replaced'
    proxy = TorchProxy(cpu)
    setattr(ops_module, 'torch', proxy)
    try:
        yield OutputFences(proxy)
    finally:
        setattr(ops_module, 'torch', real)


def no_nan(results):
    """None when no floating result holds a NaN, else a description."""
    for k, t in enumerate(_flatten(results)):
        if t.dtype.is_floating_point and bool(torch.isnan(t).any()):
            return 'result %d %s %s holds %d NaN' % (k, tuple(t.shape), t.dtype, int(torch.isnan(t).sum()))
    return None


def judge(fo, results, plain=None):
    """The fenced run's verdict as one string ('' = conditions (a) fences intact and results fenced, (b) results equal to the plain
    run's raw tensors when given, (c) no NaN, (d) inputs unchanged all hold)."""
    bad = fo.problems(results)
    res = list(_flatten(results))
    if plain is not None:
        pl = list(_flatten(plain))
        if len(pl) != len(res):
            bad.append('fenced run returned %d tensors, the plain run %d' % (len(res), len(pl)))
        for k, (a, b) in enumerate(zip(res, pl)):
            if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(a.cpu(), b.cpu()):
                bad.append('result %d %s differs from the plain run' % (k, tuple(a.shape)))
    for msg in (no_nan(results), inputs_unchanged()):
        if msg:
            bad.append(msg)
    return '\n'.join(bad)
