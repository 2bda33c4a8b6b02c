"""Channels-last result frames (config.result_layout = 'hwc', REFVSR_RESULT_HWC), the part that runs without a GPU: the configuration
field and its resolver, the CLI flag, the claim that evalrun.write_frame's image bytes do not depend on the layout, the agreement of the
header, the binding and the built library on the new symbol and flag, and the host-side refusal of unknown out_fmt bits (host memory
stands in for device pointers, as in tests/test_capi.py: validation precedes any device work)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def channels_last(x):
    """The [.., 3, h, w] view of a dense [.., h, w, 3] copy of x: what the engine returns under result_layout = 'hwc'."""
    return x.movedim(-3, -1).contiguous().movedim(-1, -3)


# ------------------------------------------------------------------------------------------------ configuration, CLI
def test_default_layout_is_planar_for_every_config():
    from refvsr_amd import ops
    from refvsr_amd.config import CONFIG_NAMES, get_config
    for name in CONFIG_NAMES:
        cfg = get_config('p', 'm', name)
        assert cfg.result_layout == 'chw', name
        assert ops.check_result_layout(cfg.result_layout) == 'chw'
    assert ops.check_result_layout(None) == 'chw' and ops.check_result_layout('hwc') == 'hwc'
    assert ops.check_result_layout('') == 'chw'            # (not set = the default, as for result_dtype)


@pytest.mark.parametrize('bad', ['nhwc', 'HWC', 'bgr', 'chw ', 1, 'hwc,chw'])
def test_bad_layout_is_a_value_error_that_names_the_choices(bad):
    from refvsr_amd import ops
    with pytest.raises(ValueError, match="'chw' or 'hwc'"):
        ops.check_result_layout(bad)


def test_cli_flag(tmp_path):
    from refvsr_amd import evalrun
    base = ['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', str(tmp_path), '--output_offset', str(tmp_path / 'o')]
    assert evalrun.build_config(base).result_layout == 'chw'
    assert evalrun.build_config(base + ['--result_layout', 'hwc']).result_layout == 'hwc'
    assert evalrun.build_config(base + ['--result_layout', 'chw']).result_layout == 'chw'
    assert evalrun.build_config(['--result_layout', 'hwc']).result_layout == 'hwc'
    with pytest.raises(SystemExit):
        evalrun.build_config(base + ['--result_layout', 'nhwc'])


def test_layout_helpers():
    from refvsr_amd import ops
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7)
    y = channels_last(x)
    assert ops.result_layout_of(x) == 'chw' and ops.result_layout_of(x[0]) == 'chw'
    assert ops.result_layout_of(y) == 'hwc' and ops.result_layout_of(y[0]) == 'hwc' and ops.result_layout_of(y[0].half()) == 'hwc'
    assert ops.result_layout_of(x[:, :, :, :-1]) is None and ops.result_layout_of(x[:, :2]) is None
    frames = [y[0], y[1]]
    st = ops.stack_results(frames, 'hwc')
    assert st.shape == x.shape and torch.equal(st, x) and st.permute(0, 2, 3, 1).is_contiguous()
    assert ops.stack_results([x[0], x[1]], 'chw').is_contiguous() and ops.stack_results([x[0], x[1]]).is_contiguous()
    # what a caller does next keeps the layout: a one-frame view and the copy to the host
    assert ops.result_layout_of(y[0].unsqueeze(0)) == 'hwc' and ops.result_layout_of(y.cpu()) == 'hwc'


# ------------------------------------------------------------------------------------------------ the written images
@pytest.mark.parametrize('ext', ['png', 'jpg'])
@pytest.mark.parametrize('dtype', ['uint8', 'float32', 'float16'])
def test_write_frame_bytes_do_not_depend_on_the_layout(tmp_path, dtype, ext):
    from refvsr_amd import evalrun
    g = torch.Generator().manual_seed(11)
    if dtype == 'uint8':
        x = torch.randint(0, 256, (3, 37, 53), dtype=torch.uint8, generator=g)
    else:
        x = (torch.rand(3, 37, 53, generator=g) * 1.2 - 0.1).to(getattr(torch, dtype))      # (past both ends: the writer clamps)
    y = channels_last(x)
    assert torch.equal(x, y) and not y.is_contiguous() and y.permute(1, 2, 0).is_contiguous()
    assert y.numpy().transpose(1, 2, 0).flags['C_CONTIGUOUS']       # the array the image writer gets is the dense one: no strided copy
    pa, pb = str(tmp_path / ('chw.' + ext)), str(tmp_path / ('hwc.' + ext))
    evalrun.write_frame(pa, x)
    evalrun.write_frame(pb, y)
    a, b = open(pa, 'rb').read(), open(pb, 'rb').read()
    assert len(a) > 100 and a == b


# ------------------------------------------------------------------------------------------------ C-ABI, no GPU
@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def test_header_binding_and_library_agree_on_the_extension(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_RESULT_HWC (0x[0-9a-fA-F]+|\d+)', src)
    assert m and int(m.group(1), 0) == hip.RESULT_HWC == 0x10
    m = re.search(r'#define REFVSR_RESULT_FMT_MASK (0x[0-9a-fA-F]+|\d+)', src)
    assert m and int(m.group(1), 0) & hip.RESULT_HWC == 0 and int(m.group(1), 0) & hip.RESULT_U8 == hip.RESULT_U8
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'int\s+refvsr_convert_result_hwc\s*\(\s*const float\*\s*src,\s*int h,\s*int w,\s*int out_fmt,\s*void\*\s*out,\s*void\*\s*stream\)', code)
    assert 'refvsr_convert_result_hwc' in hip.EXPORTS and len(hip.SIGNATURES['refvsr_convert_result_hwc']) == 6
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), 'refvsr_convert_result_hwc')
    assert L.refvsr_abi_version() == hip.ABI_VERSION == 15          # an added flag and symbol: no ABI bump


def test_unknown_out_fmt_bits_are_refused_before_device_work(L):
    from refvsr_amd import hip
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 65536)()
    at = lambda off: ctypes.cast(ctypes.addressof(buf) + off, P)
    err = lambda: L.refvsr_last_error().decode()
    HWC = hip.RESULT_HWC
    bad = [3, 4, 0x13, 0x20, 0x20 | hip.RESULT_U8, 0x40 | HWC, 0x100, -1]
    for fmt in bad:
        assert L.refvsr_conv_last_fmt(at(0), 24, 8, 8, at(4096), at(8192), 2, 2, at(16384), fmt, None) != 0
        assert 'conv_last: unknown result format' in err(), (fmt, err())
        assert L.refvsr_conv_hr_last_fmt(at(0), 8, 8, at(4096), 0.1, at(8192), 2, 2, at(16384), fmt, None) != 0
        assert 'conv_hr_last: unknown result format' in err(), (fmt, err())
        assert L.refvsr_convert_result_hwc(at(0), 8, 8, fmt, at(16384), None) != 0
        assert 'convert_result_hwc: unknown result format' in err(), (fmt, err())
    # the scorers: the same argument lists as tests/test_score.py / test_score_fov.py, with a bad result format
    a, g = (P * 1)(4096), (P * 1)(8192)
    ws, sc = P(1 << 20), P(1 << 21)
    need = L.refvsr_score_workspace_bytes(1, 40, 52)
    rects = (ctypes.c_int * 4)(0, 8, 0, 8)
    need_r = L.refvsr_score_regions_workspace_bytes(1, 40, 52, 1)
    for fmt in bad:
        assert L.refvsr_score_frames(a, fmt, g, hip.RESULT_F32, hip.INGEST_PLANAR, 1, 40, 52, 7, ws, need, sc, None) != 0
        assert 'score_frames: unknown result format' in err(), (fmt, err())
        assert L.refvsr_score_frames_down(a, fmt, g, hip.RESULT_F32, hip.INGEST_PLANAR, 1, 40, 52, 4, 7, ws, need, sc, None) != 0
        assert 'score_frames_down: unknown result format' in err(), (fmt, err())
        assert L.refvsr_score_regions(a, fmt, g, hip.RESULT_F32, hip.INGEST_PLANAR, 1, 40, 52, rects, 1, ws, need_r, sc, None) != 0
        assert 'score_regions: unknown result format' in err(), (fmt, err())
    # a known format with the layout bit passes the format check: the next check speaks (host-only arguments chosen to fail it)
    for fmt in (HWC, HWC | hip.RESULT_F16, HWC | hip.RESULT_U8):
        assert L.refvsr_score_frames(a, fmt, g, hip.RESULT_F16, hip.INGEST_PLANAR, 1, 40, 52, 7, ws, need, sc, None) != 0
        assert 'ground-truth format' in err(), (fmt, err())
        assert L.refvsr_score_regions(a, fmt, g, hip.RESULT_F16, hip.INGEST_PLANAR, 1, 40, 52, rects, 1, ws, need_r, sc, None) != 0
        assert 'ground-truth format' in err(), (fmt, err())
        assert L.refvsr_conv_last_fmt(at(0), 20, 8, 8, at(4096), at(8192), 2, 2, at(16384), fmt, None) != 0
        assert 'input channels not supported' in err(), (fmt, err())
        assert L.refvsr_conv_hr_last_fmt(at(0), 8, 8, at(4096), 0.1, at(8192), 3, 3, at(16384), fmt, None) != 0
        assert 'does not divide' in err(), (fmt, err())
    assert L.refvsr_convert_result_hwc(None, 8, 8, hip.RESULT_U8, at(0), None) != 0 and 'bad args' in err()
    assert L.refvsr_convert_result_hwc(at(0), 8, 8, hip.RESULT_U8, at(0), None) != 0 and 'bad args' in err()       # in place
    assert L.refvsr_convert_result_hwc(at(2), 8, 8, hip.RESULT_U8, at(4096), None) != 0 and 'aligned' in err()
    assert L.refvsr_convert_result_hwc(at(0), 8, 8, hip.RESULT_F16 | HWC, at(4097), None) != 0 and 'aligned' in err()
    assert L.refvsr_convert_result_hwc(at(0), 1 << 15, 1 << 15, hip.RESULT_U8, at(4096), None) != 0 and 'too large' in err()
