"""Baseline JPEG on a real MI355X: refvsr_jpeg_encode returns the bytes of the numpy model refvsr_amd/jpeg.py -- for the validity matrix
of tests/jpeg_cases.py at 1, 3 and 17 frames (the 16-frame chunking) and for every crafted frame --, touches nothing but its
destinations, reports a frame that does not fit, and videorun writes MJPEG files whose frames are the model's files of the same run's
Y'CbCr frames.  Every comparison is byte equality: the model is the specification, there is no tolerance."""
import ctypes
import io
import warnings

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from refvsr_amd import jpeg, yuv

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def variant(buf, k):
    """Frame k of a batch made from one frame: the samples rotated by 7 k positions inside the buffer (k = 0: the frame itself)."""
    return buf if k == 0 else np.roll(buf.reshape(-1), 7 * k).reshape(buf.shape)


_MODEL = {}


def model(buf, key, h, w, fmt, q, r, k):
    """encode_model of variant k (k < 3) of a case's frame, computed once."""
    key = (key, q, r, k)
    if key not in _MODEL:
        _MODEL[key] = jpeg.encode_model(variant(buf, k), h, w, fmt, q, r)
    return _MODEL[key]


def pillow_reads(data, h, w):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        im = Image.open(io.BytesIO(data))
        im.load()
    assert im.size == (w, h) and im.mode == 'RGB'


def misaligned(frames_np, dev, lead=3):
    """The frames as dense views at odd offsets into one larger device buffer."""
    n = frames_np[0].size
    big = torch.full((lead + len(frames_np) * (n + 1),), CANARY, dtype=torch.uint8, device=dev)
    out = []
    for i, f in enumerate(frames_np):
        v = big[lead + i * (n + 1):lead + i * (n + 1) + n].view(f.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(f)))
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------ kernel against the model
@pytest.mark.parametrize('h,w', jc.SIZES)
@pytest.mark.parametrize('fmt', jc.FORMATS)
def test_matrix_bytes_equal_the_model(dev, fmt, h, w):
    """Every quality and restart interval of the matrix at 1, 3 and 17 frames: frame k of a batch is variant k mod 3 of the case's
    frame, so the model is computed three times per case; Pillow decodes every device-made file of the 3-frame batch."""
    from refvsr_amd import ops
    buf = jc.matrix_frame(h, w, fmt)
    dev_frames = [torch.from_numpy(np.ascontiguousarray(variant(buf, k))).to(dev) for k in range(3)]
    for q in jc.QUALITIES:
        for r in jc.restarts(h, w, fmt):
            for n in (1, 3, 17):
                got = ops.jpeg_encode([dev_frames[k % 3] for k in range(n)], h, w, fmt, q, r)
                assert len(got) == n
                for k, g in enumerate(got):
                    want = model(buf, (fmt, h, w), h, w, fmt, q, r, k % 3)
                    assert g == want, '%s %dx%d q%d R%d: frame %d of %d differs (%d bytes, model %d)' % (fmt, h, w, q, r, k, n, len(g), len(want))
                if n == 3:
                    for g in got:
                        pillow_reads(g, h, w)


@pytest.mark.parametrize('name', sorted(jc.crafted()))
def test_crafted_frames(dev, name):
    from refvsr_amd import ops
    buf, h, w, fmt, q, r = jc.crafted()[name]
    got = ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(buf)).to(dev)[None], h, w, fmt, q, r)
    assert got == [jpeg.encode_model(buf, h, w, fmt, q, r)]
    pillow_reads(got[0], h, w)


def test_default_restart_and_stacked_tensor(dev):
    """restart None is jpeg.DEFAULT_RESTART; a [2, 2, rows, w] tensor is four frames."""
    from refvsr_amd import ops
    h, w, fmt = 30, 50, 'i420'
    buf = jc.matrix_frame(h, w, fmt)
    x = torch.from_numpy(np.stack([variant(buf, k) for k in (0, 1, 2, 0)])).to(dev).view(2, 2, *buf.shape)
    got = ops.jpeg_encode(x, h, w, fmt)
    assert got == [jpeg.encode_model(variant(buf, k), h, w, fmt, 90, jpeg.DEFAULT_RESTART) for k in (0, 1, 2, 0)]


@pytest.mark.parametrize('fmt', jc.FORMATS)
def test_misaligned_sources_and_untouched_surroundings(dev, fmt):
    """Source frames as views at odd addresses of a larger buffer: the model's bytes, and the buffer is left as it was."""
    from refvsr_amd import ops
    h, w = 18, 34
    buf = jc.matrix_frame(h, w, fmt)
    frames_np = [variant(buf, k) for k in range(3)]
    views = misaligned(frames_np, dev)
    assert views[0].data_ptr() % 2 == 1 and len({v.data_ptr() % 4 for v in views}) > 1
    before = views[0]._base.clone() if views[0]._base is not None else None
    got = ops.jpeg_encode(views, h, w, fmt, 90, 2)
    assert got == [jpeg.encode_model(f, h, w, fmt, 90, 2) for f in frames_np]
    if before is not None:
        assert torch.equal(views[0]._base, before)


def raw_call(dev, frames, h, w, fmt, q, r, capacity, stream=None):
    """refvsr_jpeg_encode with canaries around dst, sizes and offsets: (rc, dst bytes [capacity], sizes, offsets, canaries intact)."""
    from refvsr_amd import hip, ops
    lib = hip.lib()
    n, pad = len(frames), 64
    samp = yuv.SAMPLINGS[yuv.sampling_of(fmt)]
    qt, dct, lut = ops._jpeg_tables(dev, q, fmt)
    dst = torch.full((pad + capacity + pad,), CANARY, dtype=torch.uint8, device=dev)
    meta = torch.full((4 + n + 4 + n + 4,), -0x5a5a5a5a5a5a5a5b, dtype=torch.int64, device=dev)       # canary | sizes | canary | offsets | canary
    wsb = lib.refvsr_jpeg_workspace_bytes(n, h, w, samp, r)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    rc = lib.refvsr_jpeg_encode(ops._parr(frames), n, h, w, samp, ops._ptr(qt), ops._ptr(dct), ops._ptr(lut), r,
                                ctypes.c_void_p(dst.data_ptr() + pad), capacity, ctypes.c_void_p(meta.data_ptr() + 8 * 4),
                                ctypes.c_void_p(meta.data_ptr() + 8 * (4 + n + 4)), ops._ptr(ws), wsb, st)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    d, m = dst.cpu().numpy(), meta.cpu().numpy()
    canary = np.int64(-0x5a5a5a5a5a5a5a5b)
    intact = bool((d[:pad] == CANARY).all() and (d[pad + capacity:] == CANARY).all() and (m[:4] == canary).all()
                  and (m[4 + n:8 + n] == canary).all() and (m[8 + 2 * n:] == canary).all())
    return rc, d[pad:pad + capacity], m[4:4 + n].tolist(), m[8 + n:8 + 2 * n].tolist(), intact


@pytest.mark.parametrize('fmt', jc.FORMATS)
def test_exact_capacity_canaries_and_overflow(dev, fmt):
    """dst of exactly the frames' bytes: everything fits, the canaries around dst, sizes and offsets stay.  One byte less: the last frame
    is not written (its bytes keep the canary value), the return code says so, sizes still hold what every frame needs, the canaries
    stay."""
    from refvsr_amd import hip
    h, w, q, r = 30, 50, 90, 3
    buf = jc.matrix_frame(h, w, fmt)
    frames_np = [variant(buf, k) for k in range(3)]
    want = [jpeg.entropy_data(f, h, w, fmt, q, r) for f in frames_np]
    frames = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames_np]
    total = sum(len(d) for d in want)
    rc, data, sizes, offsets, intact = raw_call(dev, frames, h, w, fmt, q, r, total)
    assert rc == 0, hip.lib().refvsr_last_error()
    assert intact and sizes == [len(d) for d in want] and offsets == [0, len(want[0]), len(want[0]) + len(want[1])]
    assert data.tobytes() == b''.join(want)
    rc, data, sizes, offsets, intact = raw_call(dev, frames, h, w, fmt, q, r, total - 1)
    assert rc == hip.JPEG_OVERFLOW and b'does not fit' in hip.lib().refvsr_last_error()
    assert intact and sizes == [len(d) for d in want] and offsets[:2] == [0, len(want[0])]
    assert data[:offsets[2]].tobytes() == want[0] + want[1] and (data[offsets[2]:] == CANARY).all()


def test_side_stream(dev):
    from refvsr_amd import ops
    h, w, fmt = 30, 50, 'i444'
    buf = jc.matrix_frame(h, w, fmt)
    x = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)[None]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with ops.on_stream(side):
        dst, offsets, sizes = ops.jpeg_encode_device(x, h, w, fmt, 75, 2)
    side.synchronize()
    o, s = int(offsets[0]), int(sizes[0])
    assert dst[o:o + s].cpu().numpy().tobytes() == jpeg.entropy_data(buf, h, w, fmt, 75, 2)


def test_custom_op_gives_the_same_bytes(dev):
    import refvsr_amd.torch_ops  # noqa: F401
    h, w, fmt = 18, 34, 'i420'
    buf = jc.matrix_frame(h, w, fmt)
    x = torch.from_numpy(np.stack([variant(buf, k) for k in range(2)])).to(dev)
    dst, offsets, sizes = torch.ops.refvsr.jpeg_encode(x, h, w, fmt, 90, 0)
    assert offsets.dtype == torch.int64 and sizes.dtype == torch.int64 and dst.dtype == torch.uint8
    for k in range(2):
        o, s = int(offsets[k]), int(sizes[k])
        assert dst[o:o + s].cpu().numpy().tobytes() == jpeg.entropy_data(variant(buf, k), h, w, fmt, 90, None)


# ------------------------------------------------------------------------------------------------ videorun
NAME = 'config_RefVSR_small_L1'
T, GROUP = 3, 4


def write_pair(tmp_path, tag, ly, ry, h, w, fmt='i420'):
    paths = []
    for name, x in (('uw', ly), ('w', ry)):
        paths.append(str(tmp_path / ('%s_%s.y4m' % (tag, name))))
        with yuv.Y4MWriter(paths[-1], h, w, fmt, (24, 1), 'limited') as wr:
            for f in x:
                wr.write(f)
    return paths


def run_files(net, paths, out, io_mode, **eval_kw):
    """videorun.run on a pair of files into `out`: (the bytes written, the run's config)."""
    from refvsr_amd import get_config, videorun
    cfg = get_config('p', 'm', NAME)
    cfg.frame_num, cfg.save_sample = T, False
    cfg.EVAL.frame_group = GROUP
    cfg.EVAL.io, cfg.EVAL.io_timeout = io_mode, 10
    for k, v in eval_kw.items():
        setattr(cfg if k.startswith('yuv_') else cfg.EVAL, k, v)
    n, _ = videorun.run(cfg, paths[0], paths[1], out, net=net)
    data = open(out, 'rb').read()
    return data, cfg, n


def mjpeg_against_the_model(dev, tmp_path, tag, ly, ry, h, w, oh, ow, **kw):
    """One clip three ways: --out x.mjpeg by the sync loop, the same by the stream loop, and --out x.y4m with the colour JFIF means, so
    that both make the same planes.  Frame k of the mjpeg file is encode_model of frame k of the y4m file; the two loops agree."""
    import test_gpu_resize as tgr
    paths = write_pair(tmp_path, tag, ly, ry, h, w)
    n = len(ly)
    net = tgr.make_net(NAME, T, dev)
    sync, cfg, got = run_files(net, paths, str(tmp_path / (tag + '_sync.mjpeg')), 'sync', **kw)
    assert got == n and cfg.EVAL.out_format == 'mjpeg' and (cfg.yuv_matrix, cfg.yuv_range, cfg.yuv_siting) == ('bt601', 'full', 'centre')
    stream, cfg2, got = run_files(net, paths, str(tmp_path / (tag + '_stream.mjpeg')), 'stream', **kw)
    assert got == n and stream == sync, 'the stream loop and the sync loop write different files'
    assert cfg2.EVAL.io_stats['frames'] == n and cfg2.EVAL.scene_cuts == cfg.EVAL.scene_cuts
    net_y = tgr.make_net(NAME, T, dev, yuv_matrix='bt601', yuv_range='full')
    y4m, cfg3, _ = run_files(net_y, paths, str(tmp_path / (tag + '.y4m')), 'sync', yuv_matrix='bt601', yuv_range='full', out_siting='centre', **kw)
    assert cfg3.EVAL.out_format == 'y4m' and cfg3.EVAL.scene_cuts == cfg.EVAL.scene_cuts
    frames = yuv.read_y4m(str(tmp_path / (tag + '.y4m')))
    assert (frames['h'], frames['w'], frames['fmt'], frames['range']) == (oh, ow, 'i420', 'full') and len(frames['frames']) == n
    files = jpeg.split_mjpeg(sync)
    assert len(files) == n
    for k, (f, y) in enumerate(zip(files, frames['frames'])):
        assert f == jpeg.encode_model(y, oh, ow, 'i420', 90), 'frame %d is not the model\'s file of the run\'s Y\'CbCr frame' % k
        pillow_reads(f, oh, ow)
    assert len(sync) - n * len(jpeg.header(oh, ow, 'i420')) < len(y4m) // 2          # (the 623-byte headers aside: frames here are tiny)
    return sync, cfg


def test_videorun_mjpeg_frames_are_the_models_files(dev, tmp_path):
    import test_gpu_resize as tgr
    h, w, n = 64, 96, 6
    ly, ry, _, _ = tgr.clip(n, h, w, 'i420')
    mjpeg_against_the_model(dev, tmp_path, 'plain', ly, ry, h, w, 4 * h, 4 * w)


def test_videorun_mjpeg_with_out_size(dev, tmp_path):
    import test_gpu_resize as tgr
    h, w, n = 64, 96, 6
    ly, ry, _, _ = tgr.clip(n, h, w, 'i420')
    _, cfg = mjpeg_against_the_model(dev, tmp_path, 'sized', ly, ry, h, w, 32, 48, in_down=4, out_size='48x32')
    assert cfg.result_yuv is None and cfg.EVAL.out_yuv == 'i420'


def test_videorun_mjpeg_with_scene_cut(dev, tmp_path):
    import test_gpu_scene as tgs
    (la, ra), (lb, rb) = tgs.scenes('i420')
    ly, ry = np.concatenate([la, lb]), np.concatenate([ra, rb])
    _, cfg = mjpeg_against_the_model(dev, tmp_path, 'cut', ly, ry, tgs.H, tgs.W, 4 * tgs.H, 4 * tgs.W, scene_cut=tgs.T_CUT)
    assert cfg.EVAL.scene_cuts == (tgs.NA,)


def test_videorun_mjpeg_444_and_quality(dev, tmp_path):
    """--out_chroma 444 and --jpeg_quality through --out_format on a path without the extension."""
    import test_gpu_resize as tgr
    h, w, n = 64, 96, 3
    ly, ry, _, _ = tgr.clip(n, h, w, 'i420')
    paths = write_pair(tmp_path, 'c444', ly, ry, h, w)
    data, cfg, got = run_files(tgr.make_net(NAME, T, dev), paths, str(tmp_path / 'c444.bin'), 'sync', out_format='mjpeg', out_chroma='444', jpeg_quality=60)
    y4m, _, _ = run_files(tgr.make_net(NAME, T, dev, yuv_matrix='bt601', yuv_range='full'), paths, str(tmp_path / 'c444.y4m'), 'sync',
                          yuv_matrix='bt601', yuv_range='full', out_chroma='444')
    frames = yuv.read_y4m(str(tmp_path / 'c444.y4m'))['frames']
    assert got == n and cfg.result_yuv == 'i444'
    assert jpeg.split_mjpeg(data) == [jpeg.encode_model(y, 4 * h, 4 * w, 'i444', 60) for y in frames]


def test_videorun_without_the_options_is_unchanged(dev, tmp_path):
    """A run without the new options writes the bytes of the run with --out_format y4m given explicitly -- by both loops."""
    import test_gpu_resize as tgr
    import test_gpu_scene as tgs
    h, w, n = 64, 96, 5
    ly, ry, _, _ = tgr.clip(n, h, w, 'i420')
    paths = write_pair(tmp_path, 'same', ly, ry, h, w)
    net = tgs.make_net(NAME, T, dev, ('i420', 'bt709', 'limited', 'bilinear'), result_yuv='i420')
    plain, cfg, _ = run_files(net, paths, str(tmp_path / 'plain.y4m'), 'sync')
    assert cfg.EVAL.out_format == 'y4m' and not hasattr(cfg.EVAL, 'jpeg_quality')
    for io_mode in ('sync', 'stream'):
        named, _, _ = run_files(net, paths, str(tmp_path / ('named_%s.y4m' % io_mode)), io_mode, out_format='y4m')
        assert named == plain
    assert plain.startswith(b'YUV4MPEG2 ') and len(plain) > n * yuv.frame_bytes(4 * h, 4 * w, 'i420')


def test_videorun_command_line_writes_a_readable_mjpeg(dev, tmp_path):
    """`videorun --lr uw.y4m --ref w.y4m --out sr.mjpeg`: split_mjpeg + Pillow read the file back frame for frame."""
    import test_gpu_resize as tgr
    from refvsr_amd import videorun
    h, w, n = 64, 96, 5
    ly, ry, _, _ = tgr.clip(n, h, w, 'i420')
    paths = write_pair(tmp_path, 'cli', ly, ry, h, w)
    out = str(tmp_path / 'sr.mjpeg')
    assert videorun.main(['--config', NAME, '--lr', paths[0], '--ref', paths[1], '--out', out, '--frame_num', '3']) == 0
    files = jpeg.split_mjpeg(open(out, 'rb').read())
    assert len(files) == n
    for f in files:
        pillow_reads(f, 4 * h, 4 * w)
