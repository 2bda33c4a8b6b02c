"""Y'CbCr 4:2:0 result frames on a real MI355X: refvsr_result_to_yuv420 returns the bits of the numpy model refvsr_amd/yuv.py for every
format, source form, size class and frame count, touches nothing but its destination, and the engine and evalrun hand the frames
on next to an unchanged 'result'.  Every comparison is array equality: the model is the specification, there is no tolerance."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import yuv_cases as yc
from refvsr_amd import yuv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

FORMATS = ('nv12', 'i420', 'p010', 'i420p10')
MODES = (('bt709', 'limited'), ('bt709', 'full'), ('bt601', 'limited'))
# one block | a single block row | a single block column | ragged vector ends, byte rows of 22 | rows of 70 bytes / 140 fp16 bytes:
# the 16-byte phase changes from row to row | more than one workgroup, float rows of 1032 bytes | ALIGNED.
# The kernel loads a source row as vectors only from 16-byte aligned addresses, and stores a group as vectors only where all of its
# store addresses are aligned.  Every width of the first six is 2 (mod 4): a byte or fp16 row pitch is never a multiple of 8 and almost
# every access goes by element; a float32 pitch is 8 (mod 16), so even rows load wide, odd rows by element, next to element stores
# (vector loads and element stores in one group, and the reverse at the carved offsets below).  ALIGNED is the geometry of real results: rows of
# 80 / 160 / 320 source bytes and of 80 / 160 Y and 40 / 80 planar-chroma bytes, all multiples of their vectors, whole groups only (80
# = 5 x 16 = 10 x 8 pixels), plane and frame sizes multiples of their vectors too (2720-sample planes, 680-sample chroma planes of 8-
# or 16-byte pieces) -- every load and store of every source form and format is a vector.
ALIGNED = (34, 80)
SIZES = ((2, 2), (2, 6), (6, 2), (10, 22), (34, 70), (66, 258), ALIGNED)
DTYPES = (torch.float32, torch.float16, torch.uint8)
CANARY = 0xA5
builtins_range = range         # (tests that take a `range` parameter -- the code range -- loop with this)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def channels_last(x):
    return x.movedim(-3, -1).contiguous().movedim(-1, -3)


_UNIFORM = {}


def uniform(b, h, w):
    """Seeded uniform values in [0, 1], one float64 array per geometry (every frame different), shared by the tests and left unchanged."""
    key = (b, h, w)
    if key not in _UNIFORM:
        _UNIFORM[key] = np.random.RandomState(1000 * h + w + b).rand(b, 3, h, w)
        _UNIFORM[key].setflags(write=False)
    return _UNIFORM[key]


def as_dtype(x64, dt):
    if dt == torch.uint8:
        return np.rint(255.0 * x64).astype(np.uint8)
    return x64.astype(np.float32 if dt == torch.float32 else np.float16)


def np_of(t):
    return t.cpu().numpy()


def check(got, frames_np, fmt, matrix, range, what):
    want = yuv.rgb_to_yuv420(frames_np, fmt, matrix, range)
    got = np_of(got)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got, want), '%s: %d samples differ' % (what, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ kernel against the model
@pytest.mark.parametrize('matrix, range', MODES)
@pytest.mark.parametrize('fmt', FORMATS)
def test_kernel_returns_the_models_bits(dev, fmt, matrix, range):
    from refvsr_amd import hip, ops
    assert hip.YUV420_MAX_FRAMES == 16
    for h, w in SIZES:
        for b in (1, 3, hip.YUV420_MAX_FRAMES + 1):
            x64 = uniform(b, h, w)
            for dt in DTYPES:
                src = as_dtype(x64, dt)
                want = yuv.rgb_to_yuv420(src, fmt, matrix, range)          # the layout moves addresses, never values: one reference
                planar = torch.from_numpy(src).to(dev)
                for lay, t in (('chw', planar), ('hwc', channels_last(planar))):
                    keep = t.clone()
                    frames = t if b != 3 else [t[i].clone() for i in builtins_range(b)]      # separately allocated frames (clone keeps the layout)
                    got = ops.result_to_yuv420(frames, fmt, matrix, range)
                    what = '%s %s %s %dx%d B=%d %s %s' % (fmt, matrix, range, h, w, b, dt, lay)
                    assert got.shape == (b, 3 * h // 2, w) and got.dtype == (torch.uint8 if fmt in ('nv12', 'i420') else torch.uint16), what
                    g = np_of(got)
                    assert np.array_equal(g, want), '%s: %d samples differ' % (what, int((g != want).sum()))
                    assert torch.equal(t, keep), what + ': the source changed'


@pytest.mark.parametrize('fmt', FORMATS)
def test_crafted_cases(dev, fmt):
    """Primaries, extremes, every byte, and the tie cases of tests/yuv_cases.py, in both layouts."""
    from refvsr_amd import ops
    ties = 0
    for name, frame in sorted(yc.cases().items()):
        planar = torch.from_numpy(frame).to(dev)
        for matrix, range in MODES:
            for t in (planar, channels_last(planar)):
                check(ops.result_to_yuv420([t], fmt, matrix, range), frame[None], fmt, matrix, range, '%s %s %s %s' % (name, fmt, matrix, range))
    for case, f, matrix, range, plane in yc.TIES:
        if f == fmt:
            assert yc.tie_mask(yc.cases()[case], f, matrix, range, plane).any()        # (MODES holds every tie's matrix and range)
            assert (matrix, range) in MODES
            ties += 1
    assert ties >= 2


def test_controls_are_visible_on_the_device(dev):
    """The kernel's output on each control's case differs from the wrong model: the GPU comparison can see each mistake."""
    from refvsr_amd import ops
    for control, (case, fmt, matrix, range) in sorted(yc.CONTROLS.items()):
        frame = yc.cases()[case]
        got = np_of(ops.result_to_yuv420([torch.from_numpy(frame).to(dev)], fmt, matrix, range))[0]
        assert np.array_equal(got, yuv.rgb_to_yuv420(frame, fmt, matrix, range)), control
        assert not np.array_equal(got, yc.control_model(control, frame, fmt, matrix, range)), control


@pytest.mark.parametrize('offset', [0, 4, 8])
def test_sources_off_16_byte_alignment(dev, offset):
    """Frames carved from a larger buffer at offset 0 -- every source row loads as vectors -- and at a 4- and an 8-byte offset, where no
    source row does (the destination is aligned in all three: its stores stay vectors next to element loads)."""
    from refvsr_amd import ops
    (h, w), b = ALIGNED, 3                                          # rows of whole vector groups: only the base phase decides
    x64 = uniform(b, h, w)
    for dt in DTYPES:
        src = as_dtype(x64, dt)
        es = src.itemsize
        for lay in ('chw', 'hwc'):
            frames = []
            for i in builtins_range(b):
                big = torch.zeros(src[i].nbytes + 64, dtype=torch.uint8, device=dev)
                dense = src[i] if lay == 'chw' else np.ascontiguousarray(src[i].transpose(1, 2, 0))
                big[offset:offset + dense.nbytes] = torch.from_numpy(dense.reshape(-1).view(np.uint8)).to(dev)
                v = big[offset:offset + dense.nbytes].view(dt).view(dense.shape)
                assert v.data_ptr() % 16 == offset and v.data_ptr() % es == 0
                frames.append(v if lay == 'chw' else v.permute(2, 0, 1))
            for fmt in FORMATS:
                check(ops.result_to_yuv420(frames, fmt, 'bt709', 'limited'), src, fmt, 'bt709', 'limited', '%s %s offset %d' % (dt, lay, offset))


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize('fmt', FORMATS)
def test_nothing_beyond_the_frame_is_written(dev, fmt):
    from refvsr_amd import hip, ops
    P = ctypes.c_void_p
    coef = (ctypes.c_double * 9)(*yuv.coefficients(fmt, 'bt709', 'limited'))
    for h, w in ((2, 2), (10, 22), (34, 70), (66, 258), ALIGNED):
        nbytes = hip.lib().refvsr_yuv420_bytes(h, w, yuv.FORMAT_IDS[fmt])
        assert nbytes == yuv.frame_bytes(h, w, fmt)
        for dt, sfmt in ((torch.float32, hip.RESULT_F32), (torch.float32, hip.RESULT_F32 | hip.RESULT_HWC), (torch.float16, hip.RESULT_F16),
                         (torch.float16, hip.RESULT_F16 | hip.RESULT_HWC), (torch.uint8, hip.RESULT_U8), (torch.uint8, hip.RESULT_U8 | hip.RESULT_HWC)):
            src = as_dtype(uniform(1, h, w), dt)[0]
            t = torch.from_numpy(src).to(dev)
            if sfmt & hip.RESULT_HWC:
                t = channels_last(t)
            keep = t.clone()
            pad = 256                                               # (keeps the destination's 16-byte phase: at ALIGNED every store is a vector)
            buf = torch.full((pad + nbytes + 256,), CANARY, dtype=torch.uint8, device=dev)
            rc = hip.lib().refvsr_result_to_yuv420((P * 1)(t.data_ptr()), sfmt, (P * 1)(buf.data_ptr() + pad), 1, h, w, yuv.FORMAT_IDS[fmt], coef, ops._stream())
            assert rc == 0, hip.lib().refvsr_last_error()
            out = np_of(buf)
            assert (out[:pad] == CANARY).all() and (out[pad + nbytes:] == CANARY).all(), (fmt, h, w, dt)
            want = yuv.rgb_to_yuv420(src, fmt, 'bt709', 'limited')
            assert np.array_equal(out[pad:pad + nbytes].view(want.dtype).reshape(want.shape), want)
            assert torch.equal(t, keep)


def test_ops_refuses_other_strides_and_odd_sizes(dev):
    from refvsr_amd import ops
    x = torch.rand(2, 3, 8, 12, device=dev)
    with pytest.raises(RuntimeError, match='results must be dense and of one layout'):
        ops.result_to_yuv420(x[:, :, :, :10], 'nv12')
    with pytest.raises(RuntimeError, match='results must be dense and of one layout'):
        ops.result_to_yuv420([x[0], channels_last(x[1])], 'nv12')
    with pytest.raises(RuntimeError, match='even h and w'):
        ops.result_to_yuv420(torch.rand(1, 3, 7, 12, device=dev), 'nv12')
    with pytest.raises(ValueError, match='yuv format must be one of'):
        ops.result_to_yuv420(x, 'yv12')
    with pytest.raises(RuntimeError, match='at least one frame'):
        ops.result_to_yuv420([], 'nv12')
    for bad in (x.cpu(), x.double(), x[:, :2], x[0, 0]):
        with pytest.raises(RuntimeError, match=r'cuda float32 \| float16 \| uint8 results \[3,h,w\]'):
            ops.result_to_yuv420(bad, 'nv12')
    import refvsr_amd.torch_ops  # noqa: F401  (registers torch.ops.refvsr.*)
    y = torch.ops.refvsr.result_to_yuv420(x, 'p010', 'bt601', 'full')
    assert np.array_equal(np_of(y), yuv.rgb_to_yuv420(np_of(x), 'p010', 'bt601', 'full'))
    torch.library.opcheck(torch.ops.refvsr.result_to_yuv420, (x, 'nv12', 'bt709', 'limited'), test_utils=('test_schema', 'test_faketensor'))


# ------------------------------------------------------------------------------------------------ through the engine
def make_net(name, t, dev, result_yuv, dtype='float32', layout='chw', pipelined=False, matrix='bt709', range='limited'):
    from refvsr_amd import SRNet, get_config, make_state_dict
    cfg = get_config('p', 'm', name)
    cfg.frame_num, cfg.save_sample = t, False
    cfg.result_dtype, cfg.result_layout = dtype, layout
    cfg.result_yuv, cfg.yuv_matrix, cfg.yuv_range = result_yuv, matrix, range
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234))
    if pipelined:
        net.Network.ensure_engines(1, dev)
        net.Network.set_pipelined(True)
    return net


def clip(nfr, h, w, t, dev, n=1, seed=21):
    from refvsr_amd.synth import make_clip, window_indices
    cl = [make_clip(nfr, h, w, seed=seed + b) for b in builtins_range(n)]
    lr = torch.stack([c[0] for c in cl], 0).to(dev)
    rf = torch.stack([c[1] for c in cl], 0).to(dev)
    return lr, rf, [window_indices(f, nfr, t) for f in builtins_range(nfr)]


def yuv_is_model_of_result(out, fmt, matrix='bt709', range='limited'):
    res, y = out['result'], out['yuv']
    if isinstance(res, tuple):
        assert isinstance(y, tuple) and len(y) == len(res) and all(v.shape[0] == 1 for v in y)
        res, y = torch.cat(list(res)), torch.cat(list(y))
    n, _, sh, sw = res.shape
    assert y.shape == (n, 3 * sh // 2, sw) and y.is_contiguous()
    check(y, np_of(res), fmt, matrix, range, 'engine %s' % fmt)


@pytest.mark.parametrize('layout', ['chw', 'hwc'])
@pytest.mark.parametrize('dtype, fmt', [('float32', 'nv12'), ('float16', 'p010'), ('uint8', 'i420')])
def test_engine_returns_yuv_next_to_an_unchanged_result(dev, dtype, fmt, layout):
    nfr, t = 3, 3
    lr, rf, wins = clip(nfr, 16, 24, t, dev)
    plain = make_net('config_RefVSR_small_L1', t, dev, None, dtype, layout)
    net = make_net('config_RefVSR_small_L1', t, dev, fmt, dtype, layout)
    for f, w in enumerate(wins):
        a = plain(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0)
        b = net(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0)
        assert 'yuv' not in a and list(b.keys()) == ['result', 'yuv']
        assert b['result'].shape == (1, 3, 64, 96) and b['result'].dtype == a['result'].dtype and b['result'].stride() == a['result'].stride()
        assert torch.equal(a['result'], b['result']), 'frame %d: the result moved' % f
        yuv_is_model_of_result(b, fmt)


def test_engine_forward_group_pipelined(dev):
    nfr, t = 4, 3
    lr, rf, wins = clip(nfr, 16, 24, t, dev)
    wl = torch.stack([lr[0, w] for w in wins], 0).contiguous()
    wr = torch.stack([rf[0, w] for w in wins], 0).contiguous()
    outs = {}
    for fmt in (None, 'i420p10'):
        net = make_net('config_RefVSR_small_L1', t, dev, fmt, 'uint8', 'hwc', pipelined=True, matrix='bt601')
        first = net.forward_group(wl[:1], wr[:1], [wins[0]], is_first_frame=True)
        rest = net.forward_group(wl[1:], wr[1:], wins[1:], is_first_frame=False)          # B = 3, steady state
        torch.cuda.synchronize()
        outs[fmt] = (first, rest)
    for a, b in zip(outs[None], outs['i420p10']):
        assert 'yuv' not in a and len(a['result']) == len(b['result']) == len(b['yuv'])
        assert all(torch.equal(x, y) for x, y in zip(a['result'], b['result']))
        assert all(v.shape == (1, 96, 96) and v.dtype == torch.uint16 for v in b['yuv'])
        yuv_is_model_of_result(b, 'i420p10', 'bt601')
    assert len(outs['i420p10'][1]['yuv']) == 3


@pytest.mark.parametrize('pipelined', [True, False])
def test_engine_two_samples_in_one_call(dev, pipelined):
    nfr, t = 3, 3
    lr, rf, wins = clip(nfr, 16, 24, t, dev, n=2)
    outs = {}
    for fmt in (None, 'nv12'):
        net = make_net('config_RefVSR_small_L1', t, dev, fmt, 'float32', 'chw', range='full')
        if pipelined:
            net.Network.ensure_engines(2, dev)
            net.Network.set_pipelined(True)
        kw = (lambda w: {'frame_ids': w}) if pipelined else (lambda w: {})
        outs[fmt] = [net(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0, **kw(w)) for f, w in enumerate(wins)]
        torch.cuda.synchronize()
    for a, b in zip(outs[None], outs['nv12']):
        assert 'yuv' not in a and torch.equal(a['result'], b['result']) and b['yuv'].shape == (2, 96, 96)
        yuv_is_model_of_result(b, 'nv12', range='full')


def test_engine_ir_configuration(dev):
    nfr, t = 2, 5
    lr, rf, wins = clip(nfr, 64, 64, t, dev)
    plain = make_net('config_RefVSR_IR_L1', t, dev, None, 'uint8', 'chw')
    net = make_net('config_RefVSR_IR_L1', t, dev, 'p010', 'uint8', 'chw')
    for f, w in enumerate(wins):
        a = plain(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0)
        b = net(lr[:, w].contiguous(), rf[:, w].contiguous(), f == 0)
        assert 'yuv' not in a and torch.equal(a['result'], b['result']) and b['yuv'].shape == (1, 384, 256)
        yuv_is_model_of_result(b, 'p010')


def test_engine_refuses_bad_names(dev):
    for kw, text in (({'result_yuv': 'yv12'}, 'result_yuv must be None'), ({'result_yuv': None, 'matrix': 'bt2020'}, 'yuv_matrix must be'),
                     ({'result_yuv': 'nv12', 'range': 'pc'}, 'yuv_range must be')):
        net = make_net('config_RefVSR_small_L1', 3, dev, **kw)
        with pytest.raises(ValueError, match=text):
            net.Network.ensure_engines(1, dev)


# ------------------------------------------------------------------------------------------------ evalrun
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    import make_synth_dataset
    root = str(tmp_path_factory.mktemp('ds_yuv'))
    make_synth_dataset.make(root, clips=2, frames=5, h=32, w=48)
    return root


@pytest.mark.parametrize('depth, layout, matrix, range', [(8, 'hwc', 'bt709', 'limited'), (10, 'chw', 'bt601', 'full')])
def test_evalrun_writes_one_y4m_per_clip(dev, dataset, tmp_path, depth, layout, matrix, range):
    """--video_out y4m beside --metrics device --quantitative_only (the RGB frame never leaves the device): every frame of every clip's
    file is the model of the result a second run returns as RGB (uint8 results: its PNG holds the result's bytes), and the score file
    is the second run's apart from the times."""
    from PIL import Image
    from refvsr_amd import evalrun, get_config, make_state_dict
    ck = str(tmp_path / 'RefVSR_small_L1.pytorch')
    torch.save(make_state_dict(get_config('p', 'm', 'config_RefVSR_small_L1'), 1234), ck)
    common = ['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', dataset, '--frame_num', '3', '--ckpt_abs_name', ck,
              '--result_dtype', 'uint8', '--result_layout', layout, '--metrics', 'device', '--frame_group', '4']
    cfg = evalrun.build_config(common + ['--output_offset', str(tmp_path / 'video'), '--quantitative_only', '--video_out', 'y4m', '--video_depth', str(depth),
                                         '--video_fps', '25', '--yuv_matrix', matrix, '--yuv_range', range])
    a = evalrun.evaluate(cfg, log=lambda *_: None)
    b = evalrun.evaluate(evalrun.build_config(common + ['--output_offset', str(tmp_path / 'rgb')]), log=lambda *_: None)
    assert a['frames'] == b['frames'] == 10 and a['psnr'] == b['psnr'] and a['ssim'] == b['ssim']
    strip = lambda text: re.sub(r'\([0-9.]+sec\)', '', text)
    assert strip(open(a['score_file']).read()) == strip(open(b['score_file']).read())
    assert not os.path.exists(os.path.join(a['output_root'], 'png')) and 'videos' not in b
    fmt = 'i420' if depth == 8 else 'i420p10'
    assert sorted(os.listdir(os.path.join(a['output_root'], 'y4m'))) == ['0001.y4m', '0002.y4m'] and len(a['videos']) == 2
    for clip_name in ('0001', '0002'):
        v = yuv.read_y4m(os.path.join(a['output_root'], 'y4m', clip_name + '.y4m'))
        assert (v['h'], v['w'], v['fps'], v['fmt'], v['range']) == (128, 192, (25, 1), fmt, range) and len(v['frames']) == 5
        for f, frame in enumerate(v['frames']):
            png = os.path.join(b['output_root'], 'png', 'output', clip_name, '%04d.png' % f)
            rgb = np.array(Image.open(png).convert('RGB'), dtype=np.uint8).transpose(2, 0, 1)
            assert np.array_equal(frame, yuv.rgb_to_yuv420(rgb, fmt, matrix, range)), (clip_name, f)
