"""Device scorer on a real MI355X: refvsr_score_frames against the float64 host definitions on every (result format x ground-truth
format / layout) combination, a full-size pair, determinism, the mse-only mode, and `evalrun --metrics device` against `--metrics host`
end to end.  Bars as in tests/test_score.py (they come from the arithmetic): |dSSIM| <= 1e-10 against evalrun.ssim, mse relative 1e-12
and PSNR 1e-9 dB against the float64 restatement, PSNR within 2e-5 dB of evalrun.psnr (float32 mean on the host)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def make_result(fmt, b, h, w, g):
    """(device-side tensor as generated in its format [b,3,h,w], the float32 values the host side is given)."""
    if fmt == 'u8':
        x = torch.randint(0, 256, (b, 3, h, w), dtype=torch.uint8, generator=g)
        return x, x.float() / 255.0
    x = torch.rand(b, 3, h, w, generator=g)
    if fmt == 'f16':
        x = x.half()
    return x, x.float()


def make_gt(fmt, ref, g):
    """A ground truth near `ref` (float32 [b,3,h,w]) generated in its format; 'hwc' is the channels-last view of [b,h,w,3] bytes."""
    noisy = (ref + 0.04 * torch.randn(ref.shape, generator=g)).clamp(0, 1)
    if fmt == 'f32':
        return noisy, noisy
    x = torch.round(noisy * 255.0).to(torch.uint8)
    if fmt == 'hwc':
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x, x.float() / 255.0


def check(scores, a_host, g_host, what):
    from test_score import check_against_host
    scores = scores.cpu()
    assert scores.shape == (a_host.shape[0], 2) and scores.dtype == torch.float64
    for i in range(a_host.shape[0]):
        check_against_host(float(scores[i, 0]), float(scores[i, 1]), a_host[i], g_host[i], '%s frame %d' % (what, i))


@pytest.mark.parametrize('gfmt', ['f32', 'u8', 'hwc'])
@pytest.mark.parametrize('afmt', ['f32', 'f16', 'u8'])
def test_kernel_against_the_host_on_every_format(dev, afmt, gfmt):
    from refvsr_amd import ops
    for h, w in ((40, 52), (33, 65), (64, 96)):
        for b in (1, 3, 16, 17):
            g = torch.Generator().manual_seed(1000 * h + 10 * w + b)
            a, a_host = make_result(afmt, b, h, w, g)
            t, t_host = make_gt(gfmt, a_host, g)
            sc = ops.score_frames(a.to(dev), t.to(dev))
            check(sc, a_host, t_host, '%s/%s %dx%d b%d' % (afmt, gfmt, h, w, b))


def test_kernel_identical_pair_and_smallest_frame(dev):
    from refvsr_amd import ops
    a = torch.rand(2, 3, 7, 7, generator=torch.Generator().manual_seed(3))
    sc = ops.score_frames(a.to(dev), a.clone().to(dev)).cpu()
    assert sc[:, 0].tolist() == [0.0, 0.0] and sc[:, 1].tolist() == [1.0, 1.0]
    b = (a + 0.1).clamp(0, 1)
    check(ops.score_frames(a.to(dev), b.to(dev)), a, b, '7x7')


@pytest.mark.parametrize('afmt', ['f32', 'u8'])
def test_kernel_full_size_pair(dev, afmt):
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(1080)
    a, a_host = make_result(afmt, 1, 1080, 1920, g)
    t, t_host = make_gt('hwc', a_host, g)
    check(ops.score_frames(a.to(dev), t.to(dev)), a_host, t_host, '%s/hwc 1080x1920' % afmt)


def test_kernel_is_deterministic_and_position_independent(dev):
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(5)
    a, a_host = make_result('f32', 16, 33, 65, g)
    t, _ = make_gt('hwc', a_host, g)
    a, t = a.to(dev), t.to(dev)
    first = ops.score_frames(a, t).clone()
    assert torch.equal(first, ops.score_frames(a, t))
    for k in (0, 5, 15):
        assert torch.equal(ops.score_frames(a[k:k + 1], t[k:k + 1])[0], first[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.score_frames(a, t)
    side.synchronize()
    assert torch.equal(on_side, first)


def test_mse_only_mode(dev):
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(6)
    a, a_host = make_result('u8', 3, 40, 52, g)
    t, _ = make_gt('u8', a_host, g)
    a, t = a.to(dev), t.to(dev)
    both, only = ops.score_frames(a, t, win=7).cpu(), ops.score_frames(a, t, win=0).cpu()
    assert torch.equal(both[:, 0], only[:, 0]) and only[:, 1].tolist() == [0.0] * 3 and bool((both[:, 1] > 0).all())
    with pytest.raises(RuntimeError, match='win must be 7'):
        ops.score_frames(a, t, win=5)
    with pytest.raises(RuntimeError, match='must both be'):
        ops.score_frames(a, t[:, :, :-1])


# ------------------------------------------------------------------------------------------------ evalrun --metrics device
@pytest.fixture(scope='module')
def dataset_long(tmp_path_factory):
    import make_synth_dataset
    root = str(tmp_path_factory.mktemp('ds_score'))
    make_synth_dataset.make(root, clips=2, frames=7, h=32, w=48)
    return root


def _cfg(root, out, extra=()):
    from refvsr_amd import evalrun
    return evalrun.build_config(['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', root,
                                 '--output_offset', out, '--frame_num', '3'] + list(extra))


def _ckpt(tmp_path):
    from refvsr_amd import get_config, make_state_dict
    ck = str(tmp_path / 'RefVSR_small_L1.pytorch')
    torch.save(make_state_dict(get_config('p', 'm', 'config_RefVSR_small_L1'), 1234), ck)
    return ck


@pytest.mark.parametrize('rdt', ['float32', 'uint8'])
def test_evalrun_device_metrics_equal_the_host_run(dev, dataset_long, tmp_path, rdt):
    from refvsr_amd import evalrun
    ck = _ckpt(tmp_path)
    res = {}
    for mode in ('host', 'device'):
        for grp in (1, 4):
            cfg = _cfg(dataset_long, str(tmp_path / ('out_%s_%d' % (mode, grp))),
                       ['--ckpt_abs_name', ck, '--result_dtype', rdt, '--metrics', mode, '--frame_group', str(grp)])
            res[mode, grp] = evalrun.evaluate(cfg, log=lambda *_: None)
    prefix = lambda ln: ln.split('PSNR:')[0]
    for grp in (1, 4):
        hst, dv = res['host', grp], res['device', grp]
        assert hst['frames'] == dv['frames'] == 14
        lh, ld = (open(r['score_file']).read().splitlines() for r in (hst, dv))
        assert [prefix(x) for x in lh] == [prefix(x) for x in ld]
        dp = max(abs(p - q) for p, q in zip(hst['psnr'], dv['psnr']))
        ds = max(abs(p - q) for p, q in zip(hst['ssim'], dv['ssim']))
        print('%s group %d: max |dPSNR| %.3e dB, max |dSSIM| %.3e' % (rdt, grp, dp, ds))
        assert dp <= 2e-5 and ds <= 1e-10
        for clip, frame in (('0001', '0000'), ('0001', '0005'), ('0002', '0006')):
            pa, pb = (os.path.join(r['output_root'], 'png', 'output', clip, frame + '.png') for r in (hst, dv))
            assert open(pa, 'rb').read() == open(pb, 'rb').read()
    assert res['device', 1]['psnr'] == res['device', 4]['psnr'] and res['device', 1]['ssim'] == res['device', 4]['ssim']


def test_evalrun_device_metrics_quantitative_only_moves_no_frame(dev, dataset_long, tmp_path, monkeypatch):
    """With --metrics device --quantitative_only no result-sized tensor is copied to the host: every device-to-host copy made through
    Tensor.cpu / Tensor.to is recorded as (elements, bytes) -- the engine's weight packing makes some of its own -- and the bytes of the
    copies that have a result's element count are summed (the host run, counted the same way, moves every frame)."""
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
        cfg = _cfg(dataset_long, str(tmp_path / ('q_' + mode)), ['--ckpt_abs_name', ck, '--metrics', mode, '--quantitative_only', '--frame_group', '4'])
        res = evalrun.evaluate(cfg, log=lambda *_: None)
        assert res['frames'] == 14 and not os.path.exists(os.path.join(res['output_root'], 'png'))
        got[mode] = (sum(b for n, b in moved if n == n_res), sum(b for n, b in moved if n <= 8), res)
    print('bytes to the host in result-sized copies / in copies of at most 8 elements: device mode %d / %d, host mode %d / %d'
          % (got['device'][:2] + got['host'][:2]))
    assert got['host'][0] == 14 * n_res * 4
    assert got['device'][0] == 0 and got['device'][1] >= 14 * 16          # the scores: 16 bytes per frame
    assert max(abs(p - q) for p, q in zip(got['host'][2]['psnr'], got['device'][2]['psnr'])) <= 2e-5
