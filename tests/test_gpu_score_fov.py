"""Field-of-view scoring on a real MI355X: refvsr_score_regions with the seven FOV rectangles against metrics.fov_scores_host on every
(result format x ground-truth format / layout) combination, arbitrary rectangles against plain float64 slicing, a full-size pair, the
key 1 pair against refvsr_score_frames, determinism, and `evalrun --eval_mode quan_FOV` with `--metrics device` against `--metrics host`
end to end.  Bars as in tests/test_score_fov.py (they come from the arithmetic): every SSIM mean within 1e-10, every region's
squared-error sum within 1e-12 relative and every PSNR within 1e-9 dB of the float64 host path (which tests/test_score_fov.py holds
against the literal restatement of the reference); the end-to-end per-frame values within 2e-5 dB and 1e-10."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_gpu_score import _cfg, _ckpt, make_gt, make_result  # noqa: E402
from test_score_fov import PSNR_BAR, SSE_REL, SSIM_BAR, check_table, table_sse  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def check_fov(sums, a_host, g_host, what):
    from refvsr_amd.metrics import fov_rects, fov_table, host_region_sums
    sums = sums.cpu().numpy()
    b, _, h, w = a_host.shape
    assert sums.shape == (b, 7, 2) and sums.dtype == np.float64
    for i in range(b):
        want = host_region_sums(a_host[i], g_host[i], fov_rects(h, w))
        check_table(fov_table(sums[i], h, w), fov_table(want, h, w), '%s frame %d' % (what, i), table_sse(sums[i]), table_sse(want))


@pytest.mark.parametrize('gfmt', ['f32', 'u8', 'hwc'])
@pytest.mark.parametrize('afmt', ['f32', 'f16', 'u8'])
def test_kernel_against_the_host_on_every_format(dev, afmt, gfmt):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects
    for h, w in ((20, 20), (33, 65), (70, 134)):
        for b in (1, 3, 17):
            g = torch.Generator().manual_seed(1000 * h + 10 * w + b)
            a, a_host = make_result(afmt, b, h, w, g)
            t, t_host = make_gt(gfmt, a_host, g)
            check_fov(ops.score_regions(a.to(dev), t.to(dev), fov_rects(h, w)), a_host, t_host, '%s/%s %dx%d b%d' % (afmt, gfmt, h, w, b))


def test_kernel_arbitrary_rectangles(dev):
    """Eight non-nested rectangles -- a 1 x 1 rectangle at each corner, one across the corner where four tiles meet, strips along a
    tile boundary in each direction -- against float64 slicing of the host's (a - b)^2 and S arrays."""
    from refvsr_amd import ops
    from refvsr_amd.metrics import host_region_sums
    h, w = 70, 134
    rects = [(0, 1, 0, 1), (0, 1, w - 1, w), (h - 1, h, 0, 1), (h - 1, h, w - 1, w), (30, 36, 60, 68), (5, 66, 2, 9), (0, h, 63, 65), (31, 33, 0, w)]
    g = torch.Generator().manual_seed(70)
    a, a_host = make_result('f32', 3, h, w, g)
    t, t_host = make_gt('hwc', a_host, g)
    got = ops.score_regions(a.to(dev), t.to(dev), rects).cpu().numpy()
    cnt = np.array([3.0 * (r[1] - r[0]) * (r[3] - r[2]) for r in rects])
    for i in range(3):
        want = host_region_sums(a_host[i], t_host[i], rects)
        de = np.abs(got[i, :, 0] - want[:, 0]) / want[:, 0]
        ds = np.abs(got[i, :, 1] - want[:, 1]) / cnt
        print('frame %d: max rel dSSE %.3e, max |dSSIM mean| %.3e' % (i, de.max(), ds.max()))
        assert np.all(de <= SSE_REL) and np.all(ds <= SSIM_BAR)
    one = ops.score_regions(a.to(dev), t.to(dev), rects[4:5]).cpu().numpy()              # a single rectangle, the other sums absent
    assert np.array_equal(one[:, 0], got[:, 4])
    with pytest.raises(RuntimeError, match='1..8 rectangles'):
        ops.score_regions(a.to(dev), t.to(dev), rects + [(0, 2, 0, 2)])
    with pytest.raises(RuntimeError, match='leaves the frame'):
        ops.score_regions(a.to(dev), t.to(dev), [(0, h + 1, 0, w)])


def test_kernel_full_size_pair(dev):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects
    g = torch.Generator().manual_seed(1080)
    a, a_host = make_result('u8', 1, 1080, 1920, g)
    t, t_host = make_gt('hwc', a_host, g)
    check_fov(ops.score_regions(a.to(dev), t.to(dev), fov_rects(1080, 1920)), a_host, t_host, 'u8/hwc 1080x1920')


def test_key_1_pair_equals_score_frames(dev):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects, fov_table, psnr_from_mse
    for h, w in ((33, 65), (70, 134)):
        g = torch.Generator().manual_seed(h)
        a, a_host = make_result('u8', 3, h, w, g)
        t, _ = make_gt('hwc', a_host, g)
        a, t = a.to(dev), t.to(dev)
        sc = ops.score_frames(a, t).cpu().numpy()
        sums = ops.score_regions(a, t, fov_rects(h, w)).cpu().numpy()
        for i in range(3):
            tab = fov_table(sums[i], h, w)
            assert abs(sums[i, 0, 0] / (3.0 * h * w) - sc[i, 0]) <= SSE_REL * sc[i, 0]
            assert abs(tab[0, 0, 0] - psnr_from_mse(sc[i, 0])) <= PSNR_BAR and abs(tab[0, 0, 1] - sc[i, 1]) <= SSIM_BAR


def test_kernel_is_deterministic_and_position_independent(dev):
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects
    g = torch.Generator().manual_seed(5)
    a, a_host = make_result('f32', 16, 33, 65, g)
    t, _ = make_gt('hwc', a_host, g)
    a, t, rects = a.to(dev), t.to(dev), fov_rects(33, 65)
    first = ops.score_regions(a, t, rects).clone()
    assert torch.equal(first, ops.score_regions(a, t, rects))
    for k in (0, 5, 15):
        assert torch.equal(ops.score_regions(a[k:k + 1], t[k:k + 1], rects)[0], first[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.score_regions(a, t, rects)
    side.synchronize()
    assert torch.equal(on_side, first)


def test_kernel_equals_its_numpy_model_bit_for_bit(dev):
    """metrics.score_regions_model restates the tiles, the staging, the accumulation and the reduction order: the same bits."""
    from refvsr_amd import ops
    from refvsr_amd.metrics import fov_rects, score_regions_model
    g = torch.Generator().manual_seed(9)
    a, a_host = make_result('f32', 2, 40, 70, g)
    t, t_host = make_gt('f32', a_host, g)
    got = ops.score_regions(a.to(dev), t.to(dev), fov_rects(40, 70)).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], score_regions_model(a_host[i].numpy(), t_host[i].numpy(), fov_rects(40, 70)))


# ------------------------------------------------------------------------------------------------ evalrun --eval_mode quan_FOV
@pytest.fixture(scope='module')
def dataset_long(tmp_path_factory):
    import make_synth_dataset
    root = str(tmp_path_factory.mktemp('ds_fov'))
    make_synth_dataset.make(root, clips=2, frames=7, h=32, w=48)
    return root


NUMBER = r'\d+\.\d+|inf'


def test_evalrun_fov_device_metrics_equal_the_host_run(dev, dataset_long, tmp_path):
    import re
    from refvsr_amd import evalrun
    ck = _ckpt(tmp_path)
    res = {}
    for mode in ('host', 'device'):
        for grp in (1, 4):
            cfg = _cfg(dataset_long, str(tmp_path / ('out_%s_%d' % (mode, grp))),
                       ['--ckpt_abs_name', ck, '--eval_mode', 'quan_FOV', '--metrics', mode, '--frame_group', str(grp)])
            res[mode, grp] = evalrun.evaluate(cfg, log=lambda *_: None)
    shape = lambda text: re.sub(NUMBER, '#', text)                      # the lines up to the numbers
    texts = {k: open(r['score_file']).read() for k, r in res.items()}
    want = shape(texts['host', 1])
    assert want.count('[EVAL unit|') == 14 and want.count('[MEAN EVAL unit|') == 2 and want.count('[TOTAL RefVSR_small_L1.pytorch|RealMCVSR] \n[PSNR-FOV_in  ] (0-#%: #, ') == 1
    assert want.count('[PSNR-FOV_ring] (#-#%: #, #-#%: #, #-#%: #, #-#%: #, #-#%: #, #-#%: #, )') == 3 and want.endswith('sec)\n\n')
    for k, r in res.items():
        assert shape(texts[k]) == want, k
        assert r['frames'] == 14 and len(r['fov']) == 14 and os.path.basename(r['score_file']) == 'score_RealMCVSR_quan_FOV.txt'
        assert not os.path.exists(os.path.join(r['output_root'], 'png'))             # the FOV evaluation writes no image
        assert [t[0, 0, 0] for t in r['fov']] == r['psnr'] and [t[0, 0, 1] for t in r['fov']] == r['ssim']
    for grp in (1, 4):
        hst, dv = np.array(res['host', grp]['fov']), np.array(res['device', grp]['fov'])
        assert hst.shape == (14, 6, 3, 2)
        dp, ds = np.abs(hst[..., 0] - dv[..., 0]).max(), np.abs(hst[..., 1] - dv[..., 1]).max()
        print('group %d: max |dPSNR| %.3e dB, max |dSSIM| %.3e over 14 x 16 values' % (grp, dp, ds))
        assert dp <= 2e-5 and ds <= 1e-10
        assert np.all(dv[:, 0, 1] == 0.0) and np.all(dv[:, 5, 2] == 0.0) and int((dv != 0.0).sum()) == 14 * 16 * 2
    assert np.array_equal(np.array(res['device', 1]['fov']), np.array(res['device', 4]['fov']))


def test_evalrun_fov_other_flags(dev, dataset_long, tmp_path):
    """--result_dtype, --input_dtype and --vid_name go through the FOV mode as through the plain one."""
    from refvsr_amd import evalrun
    ck = _ckpt(tmp_path)
    res = {}
    for mode in ('host', 'device'):
        cfg = _cfg(dataset_long, str(tmp_path / ('flags_' + mode)), ['--ckpt_abs_name', ck, '--eval_mode', 'quan_FOV', '--metrics', mode, '--frame_group', '4',
                                                                      '--result_dtype', 'uint8', '--input_dtype', 'uint8', '--vid_name', '0002'])
        res[mode] = evalrun.evaluate(cfg, log=lambda *_: None)
        assert res[mode]['frames'] == 7 and open(res[mode]['score_file']).read().count('[MEAN EVAL unit|RealMCVSR|0002]') == 1
    hst, dv = np.array(res['host']['fov']), np.array(res['device']['fov'])
    assert np.abs(hst[..., 0] - dv[..., 0]).max() <= 2e-5 and np.abs(hst[..., 1] - dv[..., 1]).max() <= 1e-10


def test_evalrun_fov_device_metrics_quantitative_only_moves_no_frame(dev, dataset_long, tmp_path, monkeypatch):
    """With --eval_mode quan_FOV --metrics device --quantitative_only no result-sized tensor is copied to the host (counted as
    test_gpu_score.py counts: every device-to-host copy through Tensor.cpu / Tensor.to as (elements, bytes)); the sums cross instead:
    7 rectangles x 16 bytes per frame."""
    from refvsr_amd import evalrun
    ck = _ckpt(tmp_path)
    moved = []
    real_cpu, real_to = torch.Tensor.cpu, torch.Tensor.to

    def cpu(self, *a, **k):
        if self.is_cuda:
            moved.append((self.numel(), self.numel() * self.element_size()))
        return real_cpu(self, *a, **k)

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            moved.append((self.numel(), self.numel() * self.element_size()))
        return out

    monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
    monkeypatch.setattr(torch.Tensor, 'to', to)
    n_res = 3 * 128 * 192
    got = {}
    for mode in ('device', 'host'):
        del moved[:]
        cfg = _cfg(dataset_long, str(tmp_path / ('q_' + mode)),
                   ['--ckpt_abs_name', ck, '--eval_mode', 'quan_FOV', '--metrics', mode, '--quantitative_only', '--frame_group', '4'])
        res = evalrun.evaluate(cfg, log=lambda *_: None)
        assert res['frames'] == 14
        got[mode] = (sum(b for n, b in moved if n == n_res), sum(b for n, b in moved if n % 14 == 0 and n <= 4 * 14), res)
    print('bytes to the host in result-sized copies / in copies of k x 7 x 2 sums: device mode %d / %d, host mode %d / %d'
          % (got['device'][:2] + got['host'][:2]))
    assert got['host'][0] == 14 * n_res * 4
    assert got['device'][0] == 0 and got['device'][1] >= 14 * 7 * 16          # the sums: 7 x 16 bytes per frame
