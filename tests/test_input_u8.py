"""8-bit input frames, host side: the library's byte -> float table against the reference loader's arithmetic, the C-ABI of the
ingest and byte-compare entry points (header, binding and exported symbols agree; bad arguments are refused before any device work),
the model's input contract, evalrun's --input_dtype and the fake op.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

NEW_SYMBOLS = {'refvsr_ingest_u8', 'refvsr_ingest_table', 'refvsr_ingest_max_frames', 'refvsr_bytes_equal'}


@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def test_table_is_the_reference_loaders_quotient_bit_for_bit(L):
    """T[u] == float32(float64(u) / 255) (data_loader/utils.py:28) == numpy's float32 u / 255 (evalrun.read_frame), for all 256 bytes;
    multiplying by the reciprocal would not be (recorded: it differs on 126 values)."""
    from refvsr_amd import ops
    u = np.arange(256)
    want = (u / 255.).astype(np.float32)
    got = np.array(ops.ingest_table(), dtype=np.float32)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert (u.astype(np.float32) / np.float32(255.0)).view(np.uint32).tolist() == want.view(np.uint32).tolist()
    recip = u.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((recip != want).sum()) == 126


def test_header_binding_and_exports_agree_abi_still_15(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_INGEST_MAX_FRAMES (\d+)', src)
    assert m and int(m.group(1)) == hip.INGEST_MAX_FRAMES == L.refvsr_ingest_max_frames() == 16
    assert re.search(r'REFVSR_INGEST_PLANAR = 0, REFVSR_INGEST_HWC = 1', src) and (hip.INGEST_PLANAR, hip.INGEST_HWC) == (0, 1)
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', body))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(hip.EXPORTS)
    assert hip.SIGNATURES['refvsr_bytes_equal'] == hip.SIGNATURES['refvsr_buffers_equal']
    nm = subprocess.run(['nm', '-D', '--defined-only', hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r'\bT (refvsr_[a-z0-9_]+)$', nm, flags=re.M))
    assert NEW_SYMBOLS <= exported
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15
    assert re.search(r'#define REFVSR_ABI_VERSION 15\b', src)
    assert not any(n.endswith('_f16w') for n in NEW_SYMBOLS)
    # every new export cites the reference code it replaces
    sect = src[src.index('8-bit input frames'):src.index('int refvsr_ingest_max_frames(void);')]
    assert 'data_loader/utils.py:12-41' in sect and 'models/archs/RefVSR.py:151' in sect


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_ingest_rejects_bad_arguments_without_a_gpu(L):
    ok = _ptrs(4096)
    dst = _ptrs(4096)
    err = lambda: L.refvsr_last_error().decode()
    assert L.refvsr_ingest_u8(None, dst, 1, 8, 8, 0, None) != 0 and 'null' in err()
    assert L.refvsr_ingest_u8(ok, None, 1, 8, 8, 0, None) != 0 and 'null' in err()
    assert L.refvsr_ingest_u8(_ptrs(0), dst, 1, 8, 8, 0, None) != 0 and 'null pointer' in err()
    assert L.refvsr_ingest_u8(ok, _ptrs(0), 1, 8, 8, 0, None) != 0 and 'null pointer' in err()
    for n in (0, -1, 17):
        assert L.refvsr_ingest_u8(ok, dst, n, 8, 8, 0, None) != 0 and '1..16 frames' in err()
    for lay in (-1, 2, 7):
        assert L.refvsr_ingest_u8(ok, dst, 1, 8, 8, lay, None) != 0 and 'layout' in err()
    for h, w in ((7, 8), (8, 9), (0, 8), (8, 0), (1, 1)):
        assert L.refvsr_ingest_u8(ok, dst, 1, h, w, 1, None) != 0 and 'even' in err()
    assert L.refvsr_ingest_u8(_ptrs(4098), dst, 1, 8, 8, 0, None) != 0 and 'aligned' in err()
    assert L.refvsr_ingest_u8(ok, _ptrs(4100), 1, 8, 8, 0, None) != 0 and 'aligned' in err()
    assert L.refvsr_ingest_table(None) != 0


def test_bytes_equal_rejects_bad_arguments_without_a_gpu(L):
    a, b, fl = _ptrs(4096), _ptrs(4097), ctypes.c_void_p(8192)
    err = lambda: L.refvsr_last_error().decode()
    assert L.refvsr_bytes_equal(None, b, 1, 16, fl, None) != 0
    assert L.refvsr_bytes_equal(a, b, 1, 16, None, None) != 0
    assert L.refvsr_bytes_equal(_ptrs(0), b, 1, 16, fl, None) != 0 and 'null pointer' in err()
    assert L.refvsr_bytes_equal(a, b, 0, 16, fl, None) != 0 and L.refvsr_bytes_equal(a, b, 33, 16, fl, None) != 0
    assert L.refvsr_bytes_equal(a, b, 1, 0, fl, None) != 0 and 'empty' in err()
    # the float compare keeps its contract: 16-byte sizes and alignment
    assert L.refvsr_buffers_equal(a, b, 1, 16, fl, None) != 0 and 'unaligned' in err()
    assert L.refvsr_buffers_equal(a, a, 1, 15, fl, None) != 0 and 'multiple of 16' in err()


def test_u8_layouts():
    from refvsr_amd import hip, ops
    x = torch.zeros(2, 5, 18, 26, 3, dtype=torch.uint8)
    assert ops.u8_layout(x.permute(0, 1, 4, 2, 3)) == hip.INGEST_HWC
    assert ops.u8_layout(x.permute(0, 1, 4, 2, 3)[1]) == hip.INGEST_HWC
    assert ops.u8_layout(x.permute(0, 1, 4, 2, 3)[1, 2]) == hip.INGEST_HWC
    p = torch.zeros(2, 5, 3, 18, 26, dtype=torch.uint8)
    assert ops.u8_layout(p) == ops.u8_layout(p[0]) == ops.u8_layout(p[0, 3]) == hip.INGEST_PLANAR
    assert ops.u8_layout(p.transpose(-1, -2)) is None and ops.u8_layout(p[..., ::2]) is None
    assert ops.u8_layout(p.float()) is None


def test_model_input_contract_on_the_host():
    """Network._inputs (the entry check of forward / phase_a / phase_a_group): bytes pass through unconverted in the two layouts,
    other strides are made contiguous (refused when strict), a byte / float mix raises, float inputs keep their .float()."""
    from refvsr_amd import ops
    from refvsr_amd.model import _inputs
    b = torch.randint(0, 256, (1, 3, 3, 8, 10), dtype=torch.uint8)
    hwc = torch.randint(0, 256, (1, 3, 8, 10, 3), dtype=torch.uint8).permute(0, 1, 4, 2, 3)
    for x in (b, hwc):
        lr, rf = _inputs(x, x, 'forward', strict=True)
        assert lr is x and rf is x
    odd = b.transpose(-1, -2)
    lr, _ = _inputs(odd, odd, 'forward')
    assert lr.dtype == torch.uint8 and lr.is_contiguous() and torch.equal(lr, odd)
    with pytest.raises(RuntimeError, match='input_ready'):
        _inputs(odd, odd, 'forward', strict=True)
    with pytest.raises(RuntimeError, match='both be uint8 or both float'):
        _inputs(b, b.float(), 'forward')
    with pytest.raises(RuntimeError, match='both be uint8 or both float'):
        _inputs(b.double(), b, 'phase_a')
    lr, rf = _inputs(b.double() / 255, b.half(), 'forward')
    assert lr.dtype == rf.dtype == torch.float32
    with pytest.raises(RuntimeError, match='contiguous float32'):
        _inputs(b.half(), b.half(), 'forward', strict=True)
    assert ops.u8_layout(hwc) is not None


def test_evalrun_parses_input_dtype_and_reads_bytes(tmp_path):
    from refvsr_amd import evalrun, ops
    import make_synth_dataset
    root = str(tmp_path / 'ds')
    make_synth_dataset.make(root, clips=1, frames=3, h=16, w=24)
    base = ['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', root, '--output_offset', str(tmp_path / 'o'),
            '--frame_num', '3']
    assert evalrun.build_config(base).input_dtype == 'float32'
    cfg = evalrun.build_config(base + ['--input_dtype', 'uint8'])
    assert cfg.input_dtype == 'uint8'
    with pytest.raises(SystemExit):
        evalrun.build_config(base + ['--input_dtype', 'float16'])
    ds8, ds32 = evalrun.ClipSet(cfg), evalrun.ClipSet(evalrun.build_config(base))
    for i in range(len(ds8)):
        a, b = ds8[i], ds32[i]
        for k in ('LR_UW', 'LR_REF_W'):
            assert a[k].dtype == torch.uint8 and ops.u8_layout(a[k]) is not None and a[k].shape == b[k].shape
            conv = torch.from_numpy((a[k].numpy() / 255.).astype(np.float32))
            assert torch.equal(conv, b[k])
        assert a['HR_UW'].dtype == torch.float32 and torch.equal(a['HR_UW'], b['HR_UW'])
        g = evalrun.stack_frames([a['LR_UW'], a['LR_UW']])
        assert g.shape == (2,) + tuple(a['LR_UW'].shape) and ops.u8_layout(g) is not None and torch.equal(g[1], a['LR_UW'])


def test_fake_op_shape_and_dtype():
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'ingest_u8' in t.OP_NAMES and hasattr(torch.ops.refvsr, 'ingest_u8')
    assert str(torch.ops.refvsr.ingest_u8.default._schema) == 'refvsr::ingest_u8(Tensor x) -> Tensor'
    with FakeTensorMode():
        x = torch.empty((2, 5, 3, 18, 26), dtype=torch.uint8, device='cuda')
        y = torch.ops.refvsr.ingest_u8(x)
        assert y.shape == x.shape and y.dtype == torch.float32
        y = torch.ops.refvsr.ingest_u8(torch.empty((5, 18, 26, 3), dtype=torch.uint8, device='cuda').permute(0, 3, 1, 2))
        assert y.shape == (5, 3, 18, 26) and y.dtype == torch.float32
