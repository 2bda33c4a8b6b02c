"""Confidence-map images on the GPU: refvsr_conf_colormap (ops.conf_colormap) against metrics.conf_colormap_model -- itself pinned to
the reference's chain in tests/test_conf_colormap.py -- byte for byte over the shapes, map counts and input families at which the two
kernels can go wrong; the maps of the frame-group path (forward_group(want_conf=True)) against the per-frame forward(is_log=True);
evalrun --eval_mode quan_conf_map end to end.  Every comparison is exact."""
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_conf_colormap import boundary_map, random_map  # noqa: E402
from test_gpu_score import _cfg, _ckpt  # noqa: E402

SHAPES = [(1, 1), (1, 7), (3, 5), (7, 9), (33, 65), (64, 96), (67, 131)]       # 67 x 131 = 8 777: odd, three blocks of pass 1, nine of pass 2
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def paint_guarded(maps, offset=0):
    """refvsr_conf_colormap on cuda float32 maps with every image allocated `offset` bytes past a 0xA5 guard inside a larger 0xA5
    buffer (one launch per 16 maps, ops.conf_colormap's workspace rule): the images as numpy [h, w, 3]; asserts the guards."""
    import ctypes as C
    from refvsr_amd import hip, ops
    h, w = maps[0].shape[-2:]
    nb = 3 * h * w
    bufs = [torch.full((GUARD + offset + nb + GUARD,), FILL, dtype=torch.uint8, device=maps[0].device) for _ in maps]
    ws = torch.empty(hip.lib().refvsr_conf_colormap_workspace_bytes(hip.COLORMAP_MAX_MAPS, h, w) // 4, dtype=torch.float32, device=maps[0].device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for s0 in range(0, len(maps), hip.COLORMAP_MAX_MAPS):
        n = min(hip.COLORMAP_MAX_MAPS, len(maps) - s0)
        pm = (C.c_void_p * n)(*[m.data_ptr() for m in maps[s0:s0 + n]])
        po = (C.c_void_p * n)(*[b.data_ptr() + GUARD + offset for b in bufs[s0:s0 + n]])
        hip.check(hip.lib().refvsr_conf_colormap(pm, n, h, w, po, C.c_void_p(ws.data_ptr()), ws.numel() * 4, st), 'conf_colormap')
    out = []
    for k, b in enumerate(bufs):
        b = b.cpu().numpy()
        lo, hi = GUARD + offset, GUARD + offset + nb
        assert (b[:lo] == FILL).all() and (b[hi:] == FILL).all(), 'map %d: bytes around the image were written' % k
        out.append(b[lo:hi].reshape(h, w, 3))
    return out


def check(maps_host, dev, what, guarded=True):
    from refvsr_amd import metrics, ops
    maps = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps_host]
    got = paint_guarded(maps) if guarded else [g.cpu().numpy() for g in ops.conf_colormap(maps)]
    for k, (m, g) in enumerate(zip(maps_host, got)):
        want = metrics.conf_colormap_model(m)
        bad = int((g != want).any(-1).sum())
        assert np.array_equal(g, want), '%s, map %d of %d (%s): %d pixels differ' % (what, k, len(maps_host), m.shape, bad)
    return got


# ------------------------------------------------------------------------------------------------ 1. kernel bytes against the model
@pytest.mark.parametrize('h,w', SHAPES)
def test_kernel_shapes_and_map_counts(dev, h, w):
    """Scaled and shifted noise at every shape, n = 1, 4, 16 and 17 (the second launch); both ways in: the guarded buffers and
    ops.conf_colormap."""
    maps = [random_map(h, w, 1000 * h + 17 * w + k, 0.5 + 0.37 * k, -1.0 + 0.29 * k) for k in range(17)]
    for n in (1, 4, 16, 17):
        check(maps[:n], dev, 'n = %d' % n)
    check(maps, dev, 'ops.conf_colormap', guarded=False)
    check(maps[:1], dev, 'ops.conf_colormap', guarded=False)


def test_kernel_full_size_once(dev):
    check([random_map(270, 480, 1, 0.83, 0.11), random_map(270, 480, 2, 3.0, -2.0)], dev, '270 x 480')


def test_kernel_bin_edges(dev):
    """k / 256 and both float32 neighbours, plain and under affine maps: the quotient must be the correctly rounded one."""
    from refvsr_amd import ops
    table = np.array(ops.colormap_table(), dtype=np.uint8)
    plain = check([boundary_map()], dev, 'edges')[0][0]
    assert np.array_equal(plain[:257], table[np.minimum(np.arange(257), 255)])
    check([boundary_map(0.37, 0.21), boundary_map(3.0, -1.5), boundary_map(1e-3, 0.5), boundary_map(-2.0, 0.25)], dev, 'edges, affine')
    # the same samples as rows of a taller map (more than one float4 group per lane, a tail of 771 * 5 % 4 = 3 pixels)
    tall = np.ascontiguousarray(np.repeat(boundary_map(0.37, 0.21), 5, axis=0))
    check([tall], dev, 'edges, 5 x 771')


def test_kernel_input_families(dev):
    span = random_map(7, 9, 5, 1e-3, 0.5)
    assert 0 < float(span.max() - span.min()) < 1.1e-3
    check([span], dev, 'span 1e-3')
    neg = random_map(7, 9, 3, 2.0, -3.0)
    assert neg.max() < 0
    check([neg], dev, 'negative')
    for h, w in ((5, 6), (1, 1), (67, 131)):
        got = check([np.full((h, w), 0.625, dtype=np.float32), random_map(h, w, 9)], dev, 'constant')
        assert not got[0].any()                               # span = 0: matplotlib's "bad" colour
    tiny = (random_map(9, 11, 4) * np.float32(1e-40)).astype(np.float32)          # subnormal samples and span: kept, not flushed
    assert tiny.max() > 0
    check([tiny], dev, 'subnormal')


@pytest.mark.parametrize('h,w', [(1, 7), (3, 5), (7, 9), (67, 131)])
def test_kernel_extremes_in_head_and_tail(dev, h, w):
    """The maximum in element 0 and the minimum in the last element (h w % 4 != 0), and the other way round, aligned storage and a
    view that starts one, two and three floats past a 16-byte boundary: the scalar head and tail of the reduction."""
    from refvsr_amd import metrics, ops
    assert (h * w) % 4 != 0
    for flip in (False, True):
        x = random_map(h, w, 11 * h + w).reshape(-1)
        x[0], x[-1] = (5.0, -4.0) if not flip else (-4.0, 5.0)
        x = x.reshape(h, w)
        want = metrics.conf_colormap_model(x)
        check([x], dev, 'extremes')
        for off in (1, 2, 3):
            store = torch.zeros(h * w + 8, dtype=torch.float32, device=dev)
            assert store.data_ptr() % 16 == 0
            view = store[off:off + h * w].view(h, w)
            view.copy_(torch.from_numpy(x))
            assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
            got = paint_guarded([view])[0]
            assert np.array_equal(got, want), 'view %d floats past a 16-byte boundary' % off
            assert np.array_equal(ops.conf_colormap([view])[0].cpu().numpy(), want)


def test_kernel_unaligned_image(dev):
    """An image that starts 1, 2 or 3 bytes past a dword boundary goes out as byte stores: same bytes, nothing around it touched."""
    from refvsr_amd import metrics
    x = random_map(7, 9, 21)
    m = torch.from_numpy(x).to(dev)
    for off in (1, 2, 3):
        assert np.array_equal(paint_guarded([m], offset=off)[0], metrics.conf_colormap_model(x))


def test_kernel_is_deterministic_and_stream_independent(dev):
    from refvsr_amd import ops
    maps = [torch.from_numpy(random_map(67, 131, 40 + k, 1.0 + k, -0.5 * k)).to(dev) for k in range(5)]
    a = [g.cpu() for g in ops.conf_colormap(maps)]
    b = [g.cpu() for g in ops.conf_colormap(maps)]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with ops.on_stream(side):
        c = ops.conf_colormap(maps)
    side.synchronize()
    # a map's bytes do not depend on its position in the launch
    d = [g.cpu() for g in ops.conf_colormap(maps[::-1])][::-1]
    for k in range(5):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k].cpu()) and torch.equal(a[k], d[k])


def test_ops_conf_colormap_shapes_and_refusals(dev):
    from refvsr_amd import metrics, ops
    x = torch.rand(1, 1, 6, 10, device=dev)
    out = ops.conf_colormap([x, x[0], x[0, 0]])
    assert all(o.shape == (6, 10, 3) and o.dtype == torch.uint8 and o.is_cuda for o in out)
    want = metrics.conf_colormap_model(x)
    assert all(np.array_equal(o.cpu().numpy(), want) for o in out)
    with pytest.raises(RuntimeError, match='one geometry'):
        ops.conf_colormap([x, torch.rand(1, 6, 9, device=dev)])
    with pytest.raises(RuntimeError, match='one geometry'):
        ops.conf_colormap([torch.rand(2, 6, 10, device=dev)])
    with pytest.raises(AssertionError):
        ops.conf_colormap([x.half()])


# ------------------------------------------------------------------------------------------------ 2. the maps of the frame-group path
KEYS = ['conf_map', 'conf_map_prop', 'conf_map_prop_backward', 'conf_map_prop_forward']


@pytest.fixture(scope='module')
def group_case(dev):
    """7 frames at 32 x 48, t = 3, reset_branch = 4 (a roll-over inside the first group); the per-frame reference once."""
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    nfr, t = 7, 3
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.reset_branch, cfg.save_sample = t, 4, True
    sd = make_state_dict(cfg, 1234)
    lr, rf, _ = make_clip(nfr, 32, 48, seed=5)
    lr, rf = lr.to(dev), rf.to(dev)
    wins = [window_indices(f, nfr, t) for f in range(nfr)]

    def net():
        n_ = SRNet(cfg).to(dev).eval()
        n_.load_state_dict(sd)
        return n_
    ref = net()
    want = []
    for f, w in enumerate(wins):
        o = ref(lr[w][None], rf[w][None], f == 0, is_log=True, frame_ids=w)
        want.append((o['result'].clone(), dict((k, v.clone()) for k, v in o['eval_vis'].items())))
    torch.cuda.synchronize()
    return {'cfg': cfg, 'net': net, 'lr': lr, 'rf': rf, 'wins': wins, 'want': want}


@pytest.mark.parametrize('cuts', [(0, 4, 7), (0, 1, 5, 7)])
def test_forward_group_returns_the_maps_of_every_window(dev, group_case, cuts):
    """reset_branch = 4: window 4 restarts the forward branch -- as the first window of a group (cuts 0 | 4 | 7) and as the last one
    (0 | 1 | 5 | 7, where the first frame is a call of one window: the single-window path)."""
    g = group_case
    lr, rf, wins, want = g['lr'], g['rf'], g['wins'], g['want']
    assert list(want[0][1].keys()) == KEYS and want[0][1]['conf_map'].shape == (1, 1, 32, 48)
    net = g['net']()
    net.Network.set_pipelined(True)
    got = []
    for f0, f1 in zip(cuts[:-1], cuts[1:]):
        ws = wins[f0:f1]
        o = net.forward_group(torch.stack([lr[w] for w in ws], 0), torch.stack([rf[w] for w in ws], 0), ws, is_first_frame=(f0 == 0), want_conf=True)
        assert len(o['result']) == len(o['eval_vis']) == len(ws)
        got += list(zip(o['result'], o['eval_vis']))
    torch.cuda.synchronize()
    assert len(got) == 7
    for f, ((res, vis), (wres, wvis)) in enumerate(zip(got, want)):
        assert torch.equal(res, wres), 'frame %d: result differs' % f
        assert list(vis.keys()) == KEYS
        for k in KEYS:
            assert vis[k].shape == (1, 1, 32, 48) and vis[k].dtype == torch.float32
            assert torch.equal(vis[k], wvis[k]), 'frame %d: %s differs' % (f, k)


def test_forward_group_without_want_conf_has_no_maps(dev, group_case):
    g = group_case
    lr, rf, wins, want = g['lr'], g['rf'], g['wins'], g['want']
    net = g['net']()
    net.Network.set_pipelined(True)
    calls = []
    from refvsr_amd.engine import Engine
    real = Engine._conf_vis
    try:
        Engine._conf_vis = staticmethod(lambda *a: (calls.append(1), real(*a))[1])
        o = net.forward_group(torch.stack([lr[w] for w in wins[:4]], 0), torch.stack([rf[w] for w in wins[:4]], 0), wins[:4], is_first_frame=True)
        n_plain = len(calls)
        o2 = net.forward_group(torch.stack([lr[w] for w in wins[4:]], 0), torch.stack([rf[w] for w in wins[4:]], 0), wins[4:], want_conf=True)
    finally:
        Engine._conf_vis = staticmethod(real)
    torch.cuda.synchronize()
    assert 'eval_vis' not in o and list(o.keys()) == ['result']
    assert n_plain == 0 and len(calls) == 3                    # the maps (and their max2 launch) are built only when asked for
    assert 'eval_vis' in o2 and len(o2['eval_vis']) == 3
    for f in range(4):
        assert torch.equal(o['result'][f], want[f][0])
    for f in range(3):
        assert torch.equal(o2['result'][f], want[4 + f][0])


# ------------------------------------------------------------------------------------------------ 3. evalrun --eval_mode quan_conf_map
@pytest.fixture(scope='module')
def dataset_long(tmp_path_factory):
    import make_synth_dataset
    root = str(tmp_path_factory.mktemp('ds_conf'))
    make_synth_dataset.make(root, clips=2, frames=7, h=32, w=48)
    return root


FOLDERS = ['input', 'output', 'conf_map_norm', 'conf_map_prop_norm', 'conf_map_prop_b_norm', 'conf_map_prop_f_norm']


def _tree(root, fmt):
    out = {}
    for folder in FOLDERS:
        for clip in sorted(os.listdir(os.path.join(root, fmt, folder))):
            for fn in sorted(os.listdir(os.path.join(root, fmt, folder, clip))):
                out[folder, clip, fn] = open(os.path.join(root, fmt, folder, clip, fn), 'rb').read()
    return out


def test_evalrun_conf_map_end_to_end(dev, dataset_long, tmp_path):
    from PIL import Image
    from refvsr_amd import SRNet, evalrun, metrics
    ck = _ckpt(tmp_path)
    res = {}
    for grp in (1, 4):
        # (--metrics device and -quantitative_only: no effect in this mode)
        extra = ['--metrics', 'device', '-quantitative_only'] if grp == 4 else []
        cfg = _cfg(dataset_long, str(tmp_path / ('conf_%d' % grp)), ['--ckpt_abs_name', ck, '--eval_mode', 'quan_conf_map', '--frame_group', str(grp)] + extra)
        res[grp] = evalrun.evaluate(cfg, log=lambda *_: None)
    sec = r'\(\d+\.\d{5}sec\)'
    for grp, r in res.items():
        assert r['frames'] == 14 and len(r['seconds']) == 14 and r['psnr'] == [] and r['ssim'] == []
        assert os.path.basename(r['score_file']) == 'score_RealMCVSR_quan_conf_map.txt'
        text = open(r['score_file']).read()
        lines = text.split('\n')
        ev = [ln for ln in lines if ln.startswith('[EVAL ')]
        assert len(ev) == 14
        for i, ln in enumerate(ev):
            c, f = divmod(i, 7)
            assert re.fullmatch(r'\[EVAL unit\|RealMCVSR\|%04d\]\[%d/2\]\[%d/7\] %04d\.png %s' % (c + 1, c + 1, f + 1, f, sec), ln), ln
        mean = [i for i, ln in enumerate(lines) if ln.startswith('[MEAN EVAL ')]
        assert len(mean) == 2
        for c, i in enumerate(mean):                           # a clip's line is named for the clip it summarises; a blank line follows
            assert re.fullmatch(r'\[MEAN EVAL unit\|RealMCVSR\|%04d\]\[%d/2\] %s' % (c + 1, c, sec), lines[i]), lines[i]
            assert lines[i + 1] == ''
        assert re.search(r'\n\n\[TOTAL RefVSR_small_L1\.pytorch\|RealMCVSR\] %s\n$' % sec, text)
        assert 'PSNR' not in text and 'SSIM' not in text
    # the twelve PNG trees (six folders, two runs) are byte-identical between --frame_group 1 and 4
    t1, t4 = _tree(res[1]['output_root'], 'png'), _tree(res[4]['output_root'], 'png')
    assert len(t1) == 6 * 14 and sorted(t1) == sorted(t4)
    for k in t1:
        assert t1[k] == t4[k], k
    assert len(_tree(res[1]['output_root'], 'jpg')) == 6 * 14 and len(_tree(res[4]['output_root'], 'jpg')) == 6 * 14
    # output/*.png (and input) are what a qual_quan run writes
    cfg = _cfg(dataset_long, str(tmp_path / 'plain'), ['--ckpt_abs_name', ck])
    plain = evalrun.evaluate(cfg, log=lambda *_: None)
    for folder in ('input', 'output'):
        for clip in ('0001', '0002'):
            for f in range(7):
                p = os.path.join(plain['output_root'], 'png', folder, clip, '%04d.png' % f)
                assert open(p, 'rb').read() == t1[folder, clip, '%04d.png' % f], (folder, clip, f)
    # three (clip, frame) picks: each conf PNG decodes to the model's image of the map an independently driven net returns
    cfg = _cfg(dataset_long, str(tmp_path / 'own'), ['--ckpt_abs_name', ck, '--eval_mode', 'quan_conf_map'])
    net = SRNet(cfg).to(dev).eval()
    evalrun.load_checkpoint(net, ck)
    ds = evalrun.ClipSet(cfg)
    picks = {(0, 0), (0, 5), (1, 6)}
    seen = 0
    with torch.no_grad():
        for i in range(len(ds)):
            it = ds[i]
            if it['is_first']:
                net.Network.reset()
            o = net(it['LR_UW'][None].to(dev), it['LR_REF_W'][None].to(dev), it['is_first'], is_log=True, frame_ids=it['frame_ids'])
            if (it['video_idx'], it['frame_idx']) not in picks:
                continue
            for folder, key in evalrun.CONF_MAP_DIRS:
                want = metrics.conf_colormap_model(o['eval_vis'][key])
                png = np.array(Image.open(os.path.join(res[4]['output_root'], 'png', folder, it['video_name'], it['frame_name'])).convert('RGB'))
                assert want.shape == (32, 48, 3) and np.array_equal(png, want), (folder, it['video_name'], it['frame_name'])
                assert folder != 'conf_map_norm' or want.any()         # (the matching confidence of a frame is never constant)
            seen += 1
    assert seen == 3
