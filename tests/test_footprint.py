"""The fence harness of tests/footprint.py on CPU tensors: what it hands out, what it detects, and that it covers every allocation
call of refvsr_amd/ops.py."""
import ast
import os
import re

import pytest
import torch

import footprint as fp
from refvsr_amd import ops

OPS_PY = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), 'ops.py')
CPU = torch.device('cpu')

# torch.<allocator>(...) / x.new_*(...) calls of ops.py that the proxy need not intercept because they only ever make host
# memory, as {name: why}.  There is none today: every allocator call in ops.py makes device memory and is intercepted.
HOST_ONLY = {}
ALLOCATOR = re.compile(r'^(empty|zeros|ones|full|new_)\w*$|^(tensor|arange)$')


def allocator_calls(source):
    """{name} of the torch.<name>(...) calls with an allocator's name, and of the .new_*(...) method calls, in source."""
    names = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and ALLOCATOR.match(node.func.attr):
            base = node.func.value
            if (isinstance(base, ast.Name) and base.id == 'torch') or node.func.attr.startswith('new_'):
                names.add(node.func.attr)
    return names


def uncovered(source):
    return sorted(allocator_calls(source) - set(fp.INTERCEPTED) - set(HOST_ONLY))


def test_fence_sizing_rule():
    assert fp.fence_bytes(0) == fp.fence_bytes(1) == fp.fence_bytes(65536) == 65536
    assert fp.fence_bytes(65537) == 65536 + 256 and fp.fence_bytes(19 * 45 * 24 * 2) == 65536
    assert fp.fence_bytes(33 * 70 * 48 * 2) == 221952 and fp.fence_bytes(221952) % 256 == 0


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.int32, torch.uint8, torch.float64])
@pytest.mark.parametrize('poison', ['nan', 'benign'])
def test_fenced_input_view_and_fences(dtype, poison):
    fp.reset_inputs()
    t = (torch.arange(19 * 45 * 3) % 97).reshape(19, 45, 3).to(dtype)
    v = fp.fenced_input(t, CPU, poison)
    assert v.shape == t.shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 16 == 0 and torch.equal(v, t)
    assert v.storage_offset() * v.element_size() == fp.fence_bytes(t.numel() * t.element_size())
    buf, view, lead, tail, _ = fp._INPUTS[-1]
    assert view is v and lead == tail == fp.fence_bytes(t.numel() * t.element_size()) and buf.dtype == dtype
    assert buf.numel() * buf.element_size() == lead + tail + t.numel() * t.element_size()
    n = lead // t.element_size()
    for f in (buf[:n], buf[n + t.numel():]):
        if poison == 'benign':
            assert not f.any()
        elif dtype.is_floating_point:
            assert torch.isnan(f).all()
        else:
            assert bool((f.view(torch.uint8) == 0xFF).all())      # all-ones bytes: a NaN whichever float type reads them
            raw = f.view(torch.uint8)[:256].clone()
            assert torch.isnan(raw.view(torch.float16)).all() and torch.isnan(raw.view(torch.float32)).all()
    assert fp.inputs_unchanged() is None
    fp.reset_inputs()


@pytest.mark.parametrize('where', ['view', 'lead_near', 'lead_far', 'tail_near', 'tail_far'])
def test_inputs_unchanged_sees_a_byte(where):
    fp.reset_inputs()
    fp.fenced_input(torch.zeros(4, 8, dtype=torch.float16), CPU, 'nan')
    v = fp.fenced_input(torch.ones(5, 7, dtype=torch.float32), CPU, 'benign')
    buf, _, lead, tail, _ = fp._INPUTS[-1]
    raw = buf.view(torch.uint8)
    at = {'view': lead + 3, 'lead_near': lead - 1, 'lead_far': 0, 'tail_near': lead + 140, 'tail_far': raw.numel() - 1}[where]
    assert fp.inputs_unchanged() is None
    raw[at] ^= 0x40
    msg = fp.inputs_unchanged()
    assert msg and 'fenced input 1' in msg and ('bytes %d .. %d ' % (at - lead, at - lead)) in msg
    assert torch.equal(v, torch.ones(5, 7)) == (where != 'view')
    fp.reset_inputs()
    assert fp.inputs_unchanged() is None


def alloc_all(t):
    """One call of every intercepted allocator, through the name `torch` as ops sees it."""
    x = t.empty((5, 7, 8), dtype=torch.float16, device=CPU)
    return [x, t.empty(3, 4, dtype=torch.float32, device=CPU), t.empty_like(x), t.zeros(11, dtype=torch.int32, device=CPU),
            t.ones(6, dtype=torch.int32, device=CPU), t.empty((2, 5), dtype=torch.uint8, device=CPU), t.empty_like(x.permute(2, 0, 1))]


def test_fenced_outputs_views_and_clean_run():
    with fp.fenced_outputs(ops, cpu=True) as fo:
        assert ops.torch is not torch and ops.torch.float16 is torch.float16 and ops.torch.cuda is torch.cuda
        res = alloc_all(ops.torch)
        want = [((5, 7, 8), torch.float16), ((3, 4), torch.float32), ((5, 7, 8), torch.float16), ((11,), torch.int32), ((6,), torch.int32),
                ((2, 5), torch.uint8), ((8, 5, 7), torch.float16)]
        assert len(fo.records) == len(res) == len(want)
        for r, rec, (shape, dtype) in zip(res, fo.records, want):
            assert tuple(r.shape) == shape and r.dtype == dtype and r.is_contiguous() and r.data_ptr() % 16 == 0
            nbytes = r.numel() * r.element_size()
            assert rec.lead == rec.tail == fp.fence_bytes(nbytes) and rec.buf.numel() == 2 * rec.lead + nbytes
            assert r.data_ptr() == rec.buf.data_ptr() + rec.lead
            assert bool((rec.buf[:rec.lead] == fp.OUT_BYTE).all()) and bool((rec.buf[rec.lead + nbytes:] == fp.OUT_BYTE).all())
        assert not res[3].any() and bool((res[4] == 1).all())
        for r in res:                                             # a kernel that stays inside its outputs
            r.view(-1).view(torch.uint8).fill_(0x11)
        hwc, _ = ops._result_empty(4, 6, torch.uint8, CPU, 'hwc')                  # through ops itself: the channels-last result view
        assert tuple(hwc.shape) == (3, 4, 6) and not hwc.is_contiguous()
        fo.check(results=[res, (hwc, None), {'k': list(res[0])}])
        assert fp.judge(fo, res, [r.clone() for r in res]) == ''
    assert ops.torch is torch


def test_host_allocations_pass_through_without_the_switch():
    with fp.fenced_outputs(ops) as fo:
        x = ops.torch.empty((4, 4), dtype=torch.float32, device=CPU)
        y = ops.torch.zeros(3, dtype=torch.int64)
        assert not fo.records and x.storage_offset() == 0 and not y.any()
        assert fo.problems([x]) and not fo.problems([])
    assert ops.torch is torch


@pytest.mark.parametrize('which', range(7))
@pytest.mark.parametrize('where', ['before', 'after', 'lead_far', 'tail_far'])
def test_one_stray_byte_fails_check(which, where):
    with fp.fenced_outputs(ops, cpu=True) as fo:
        res = alloc_all(ops.torch)
        fo.check(results=res)
        rec = fo.records[which]
        at = {'before': rec.lead - 1, 'after': rec.lead + rec.nbytes, 'lead_far': 0, 'tail_far': rec.buf.numel() - 1}[where]
        rec.buf[at] = 0x00
        off = at - rec.lead
        with pytest.raises(AssertionError) as e:
            fo.check(results=res)
        side = 'lead' if off < 0 else 'tail'
        assert ('fenced allocation %d ' % which) in str(e.value) and (side + ' fence damaged, 1 bytes between offsets %d and %d ' % (off, off)) in str(e.value)
        assert 'first holds 0x00' in str(e.value)
        assert len(fo.problems(res)) == 1 and fp.judge(fo, res) != ''
    assert ops.torch is torch


def test_damage_reports_first_and_last_offset():
    with fp.fenced_outputs(ops, cpu=True) as fo:
        x = ops.torch.empty((10, 8), dtype=torch.float16, device=CPU)
        rec = fo.records[0]
        rec.buf[rec.lead + rec.nbytes:rec.lead + rec.nbytes + 16] = 0x3c           # one more row of fp16 behind the map
        rec.buf[rec.lead + rec.nbytes + 100] = 0x7f
        assert rec.damage() == [('tail', 160, 260, 0x3c, 17)]
        assert fo.problems([x]) and 'between offsets 160 and 260' in fo.problems([x])[0]


def test_torch_is_restored_after_an_exception():
    with pytest.raises(RuntimeError):
        with fp.fenced_outputs(ops, cpu=True):
            assert ops.torch is not torch
            raise RuntimeError('kernel failed')
    assert ops.torch is torch
    with fp.fenced_outputs(ops, cpu=True):                          # and the harness can be entered again
        pass
    assert ops.torch is torch


def test_unfenced_result_fails_the_condition():
    with fp.fenced_outputs(ops, cpu=True) as fo:
        good = ops.torch.empty((4, 8), dtype=torch.float16, device=CPU)
        good.zero_()
        for stray in (torch.empty((4, 8), dtype=torch.float16), good.clone(), torch.stack([good, good]), fo.records[0].buf[:16]):
            fo.check(results=[good])
            with pytest.raises(AssertionError) as e:
                fo.check(results=[good, stray])
            assert 'result 1 of 2' in str(e.value) and 'not inside a fenced allocation' in str(e.value)
            assert fp.judge(fo, [good, stray]) != ''
        fo.check(results=[good, good[2:], good.t()])                # views of a fenced result are fenced


def test_judge_sees_nan_and_difference():
    fp.reset_inputs()
    with fp.fenced_outputs(ops, cpu=True) as fo:
        a = ops.torch.zeros((4, 8), dtype=torch.float16, device=CPU)
        plain = torch.zeros(4, 8, dtype=torch.float16)
        assert fp.judge(fo, [a], [plain]) == ''
        plain[3, 7] = 1
        assert 'differs from the plain run' in fp.judge(fo, [a], [plain])
        a[0, 0] = float('nan')
        assert 'NaN' in fp.judge(fo, [a])
        assert 'returned 1 tensors' in fp.judge(fo, [a], [plain, plain])


class Holder(object):
    pass


def test_fence_weights_rehomes_and_keeps_values():
    from refvsr_amd import packing
    fp.reset_inputs()
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(24, 24, 3, 3, generator=g), torch.randn(24, generator=g)
    pk = packing.pack_conv(w, b, [24], False)
    cw = ops.ConvWeights(pk, CPU)
    old = dict((k, getattr(cw, k).clone()) for k in ('wpack', 'bias', 'blob24') if getattr(cw, k) is not None)
    assert 'wpack' in old and 'bias' in old
    assert fp.fence_weights(cw) is cw
    for k, v in old.items():
        t = getattr(cw, k)
        assert torch.equal(t, v) and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.storage_offset() > 0 and t.dtype == v.dtype
    assert cw.desc.wpack == cw.wpack.data_ptr() and cw.desc.bias == cw.bias.data_ptr()
    ch = Holder()
    ch.blobs, ch.stride = torch.arange(3 * 4096, dtype=torch.int64).reshape(3, 4096).to(torch.uint8), 4096
    keep = ch.blobs.clone()
    fp.fence_weights(ch)
    assert torch.equal(ch.blobs, keep) and ch.blobs.data_ptr() % 16 == 0 and ch.blobs.storage_offset() == fp.fence_bytes(3 * 4096)
    blob = fp.fence_weights(keep[0])
    assert torch.equal(blob, keep[0]) and blob.storage_offset() > 0
    assert len(fp._INPUTS) == len(old) + 2 and fp.inputs_unchanged() is None
    cw.bias[0] += 1
    assert fp.inputs_unchanged()
    fp.reset_inputs()


def test_every_allocator_call_of_ops_is_intercepted():
    with open(OPS_PY) as f:
        src = f.read()
    found = allocator_calls(src)
    assert {'empty', 'empty_like', 'zeros', 'ones'} <= found, 'the scan no longer finds the calls it is there for: %s' % sorted(found)
    assert not uncovered(src), 'ops.py allocates through %s, which the fence proxy does not intercept' % uncovered(src)
    for k in fp.INTERCEPTED:
        assert callable(getattr(fp.TorchProxy, k))
    assert not set(HOST_ONLY) & set(fp.INTERCEPTED)


@pytest.mark.parametrize('line, name', [('out = torch.full((h, w), 0.0, device=dev)', 'full'), ('out = torch.zeros_like(x)', 'zeros_like'),
                                        ('out = x.new_empty((h, w))', 'new_empty'), ('i = torch.arange(n, device=dev)', 'arange'),
                                        ('t = torch.tensor([1, 2], device=dev)', 'tensor'), ('o = torch.empty_strided(s, st)', 'empty_strided')])
def test_an_unknown_allocator_in_ops_would_fail(line, name):
    with open(OPS_PY) as f:
        src = f.read()
    assert uncovered(src + '\n\ndef later(x, h, w, n, s, st, dev):\n    %s\n' % line) == [name]
