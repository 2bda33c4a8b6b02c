"""Scores of the flag_HD_in configs on a real MI355X: refvsr_score_frames_down (the bicubic down-scale fused into the scorer's tile
staging) against the two-step path -- metrics.down_bicubic_model on the host, uploaded, scored by refvsr_score_frames -- BIT FOR BIT on
every (factor x size x result format x ground-truth format / layout x batch) combination, a full-size pair against the float64 host
definitions at the bars of tests/test_score.py, determinism, and `evalrun` on an HD config with `--metrics device` against `--metrics
host` end to end (|dPSNR| <= 2e-5 dB: the host's float32 mean, as in tests/test_gpu_score.py; |dSSIM| within the model-against-torch
bar measured in tests/test_score_down.py: the host path's image is torch's float32 one)."""
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

MAX_FRAMES = 16          # REFVSR_SCORE_MAX_FRAMES: a batch of 17 takes two launches


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    assert hip.lib().refvsr_score_max_frames() == MAX_FRAMES
    return torch.device('cuda:0')


def make_result(fmt, b, h, w, g):
    """(the tensor as generated in its format [b,3,h,w], the float32 values it stands for)."""
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
        return noisy
    x = torch.round(noisy * 255.0).to(torch.uint8)
    if fmt == 'hwc':
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x


def down_host(big_host, s):
    """float32 [b,3,h,w]: the definition, frame by frame."""
    from refvsr_amd.metrics import down_bicubic_model
    return torch.from_numpy(np.stack([down_bicubic_model(x.numpy(), s) for x in big_host]))


@pytest.mark.parametrize('afmt', ['f32', 'f16', 'u8'])
@pytest.mark.parametrize('h,w', [(7, 7), (33, 65), (40, 52), (64, 96)])
@pytest.mark.parametrize('s', [2, 4])
def test_fused_equals_two_steps_bit_for_bit(dev, s, h, w, afmt):
    """One wrong tap, one missed clamp or one changed order of summation changes a bit.  (7, 7) at s = 2: every tap of the border
    columns is clamped; batch 17 crosses REFVSR_SCORE_MAX_FRAMES."""
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(10000 * s + 100 * h + w)
    big, big_host = make_result(afmt, MAX_FRAMES + 1, s * h, s * w, g)
    d = down_host(big_host, s)
    assert bool(((d < 0) | (d > 1)).any()), 'no sample leaves [0, 1]: the clamp would go untested'
    big, d_dev, dc_dev = big.to(dev), d.to(dev), d.clamp(0, 1).to(dev)
    for gfmt in ('f32', 'u8', 'hwc'):
        t = make_gt(gfmt, d.clamp(0, 1), g).to(dev)
        for b in (1, 3, MAX_FRAMES + 1):
            fused = ops.score_frames(big[:b], t[:b], down=s)
            ssim2 = ops.score_frames(d_dev[:b], t[:b])[:, 1]
            mse2 = ops.score_frames(dc_dev[:b], t[:b], win=0)[:, 0]
            assert fused.shape == (b, 2) and fused.dtype == torch.float64
            assert torch.equal(fused[:, 1], ssim2), (gfmt, b, (fused[:, 1] - ssim2).abs().max().item())
            assert torch.equal(fused[:, 0], mse2), (gfmt, b, (fused[:, 0] - mse2).abs().max().item())
            assert bool((fused[:, 0] > 0).all()) and bool((fused[:, 1] > 0).all())
            only = ops.score_frames(big[:b], t[:b], win=0, down=s)
            assert torch.equal(only[:, 0], fused[:, 0]) and only[:, 1].tolist() == [0.0] * b


@pytest.mark.parametrize('afmt', ['f32', 'f16', 'u8'])
def test_results_not_aligned_to_four_samples_give_the_same_bits(dev, afmt):
    """At s = 4 a result aligned to four samples is read one tap row per load; a result that starts one sample later takes the
    element-by-element loads.  Same values, same bits."""
    from refvsr_amd import ops
    h, w, s = 33, 65, 4
    g = torch.Generator().manual_seed(44)
    big, big_host = make_result(afmt, 2, s * h, s * w, g)
    t = make_gt('hwc', down_host(big_host, s).clamp(0, 1), g).to(dev)
    big = big.to(dev)
    store = torch.empty(big.numel() + 1, dtype=big.dtype, device=dev)
    shifted = store[1:].view(big.shape)
    shifted.copy_(big)
    assert big.data_ptr() % (4 * big.element_size()) == 0 and shifted.data_ptr() % (4 * big.element_size()) == big.element_size()
    assert shifted.is_contiguous() and torch.equal(ops.score_frames(shifted, t, down=s), ops.score_frames(big, t, down=s))


@pytest.mark.parametrize('afmt', ['f32', 'u8'])
def test_full_size_pair_against_the_host_definitions(dev, afmt):
    """1080 x 1920 -> 270 x 480 at s = 4, at the bars of tests/test_score.py::check_against_host (they come from the arithmetic): the
    SSIM of the unclamped model image, the mse / PSNR of the clamped one."""
    from refvsr_amd import evalrun, ops
    from refvsr_amd.metrics import psnr_from_mse
    from test_score import MSE_REL, PSNR32_BAR, PSNR64_BAR, SSIM_BAR
    g = torch.Generator().manual_seed(270)
    big, big_host = make_result(afmt, 1, 1080, 1920, g)
    d = down_host(big_host, 4)
    t = make_gt('hwc', d.clamp(0, 1), g)
    t_host = t.float() / 255.0
    m, q = ops.score_frames(big.to(dev), t.to(dev), down=4).cpu()[0].tolist()
    want_q = evalrun.ssim(d[0], t_host[0])
    want_m = float(((d[0].clamp(0, 1).double() - t_host[0].double()) ** 2).mean())
    print('%s 1080x1920 / 4: dssim %.3e  mse rel %.3e' % (afmt, abs(q - want_q), abs(m - want_m) / want_m))
    assert abs(q - want_q) <= SSIM_BAR and abs(m - want_m) <= MSE_REL * want_m
    assert abs(psnr_from_mse(m) - 10.0 * np.log10(1.0 / want_m)) <= PSNR64_BAR
    assert abs(psnr_from_mse(m) - evalrun.psnr(d[0].clamp(0, 1), t_host[0])) <= PSNR32_BAR


def test_deterministic_position_independent_and_stream_independent(dev):
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(5)
    big, big_host = make_result('f32', MAX_FRAMES, 2 * 33, 2 * 65, g)
    t = make_gt('hwc', down_host(big_host, 2).clamp(0, 1), g).to(dev)
    big = big.to(dev)
    first = ops.score_frames(big, t, down=2).clone()
    assert torch.equal(first, ops.score_frames(big, t, down=2))
    for k in (0, 5, 15):
        assert torch.equal(ops.score_frames(big[k:k + 1], t[k:k + 1], down=2)[0], first[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.score_frames(big, t, down=2)
    side.synchronize()
    assert torch.equal(on_side, first)


def test_down_1_is_the_call_without_the_argument_and_errors(dev):
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(6)
    a, a_host = make_result('u8', 3, 40, 52, g)
    t = make_gt('u8', a_host, g).to(dev)
    a = a.to(dev)
    for win in (7, 0):
        assert torch.equal(ops.score_frames(a, t, win=win, down=1), ops.score_frames(a, t, win=win))
    assert torch.equal(ops.score_frames(a, t, 7, 1), ops.score_frames(a, t))
    big = torch.zeros(3, 3, 160, 208, dtype=torch.uint8, device=dev)
    for down in (3, 0, 8):
        with pytest.raises(RuntimeError, match='down must be 1, 2 or 4'):
            ops.score_frames(big, t, down=down)
    with pytest.raises(RuntimeError, match='must both be'):
        ops.score_frames(big, t, down=2)                      # four times the ground truth, scored as twice
    with pytest.raises(RuntimeError, match='must both be'):
        ops.score_frames(big[:, :, :-4], t, down=4)
    with pytest.raises(RuntimeError, match='must both be'):
        ops.score_frames(a, t, down=4)                        # a result of the ground truth's own size
    with pytest.raises(RuntimeError, match='must both be'):
        ops.score_frames(big, t)
    assert ops.score_frames(big, t, down=4).shape == (3, 2)


# ------------------------------------------------------------------------------------------------ evalrun on an HD config
LINE = re.compile(r'^\[EVAL unit\|RealMCVSR\|\d{4}\]\[\d+/2\]\[\d+/5\] \d{4}\.png PSNR: \d+\.\d{5} SSIM: \d\.\d{5} \(\d+\.\d{5}sec\)$')


@pytest.fixture(scope='module')
def datasets(tmp_path_factory):
    import make_synth_dataset
    hd, plain = str(tmp_path_factory.mktemp('ds_hd')), str(tmp_path_factory.mktemp('ds_plain'))
    make_synth_dataset.make(hd, hd=True, h=32, w=48, clips=2, frames=5)
    make_synth_dataset.make(plain, h=32, w=48, clips=2, frames=5)
    return {'config_RefVSR_small_MFID_8K': hd, 'config_RefVSR_small_L1': plain}


def _run(name, root, tmp_path, tag, extra):
    from refvsr_amd import evalrun, get_config, make_state_dict
    ck = str(tmp_path / (name + '.pytorch'))
    if not os.path.exists(ck):
        torch.save(make_state_dict(get_config('p', 'm', name), 1234), ck)
    cfg = evalrun.build_config(['--config', name, '--mode', 'unit', '--data_offset', root, '--output_offset', str(tmp_path / tag), '--frame_num', '3',
                                '--quantitative_only', '--ckpt_abs_name', ck] + list(extra))
    res = evalrun.evaluate(cfg, log=lambda *_: None)
    assert res['frames'] == 10 and not os.path.exists(os.path.join(res['output_root'], 'png'))
    lines = open(res['score_file']).read().splitlines()
    frame_lines = [ln for ln in lines if ln.startswith('[EVAL ')]
    assert len(frame_lines) == 10 and all(LINE.match(ln) for ln in frame_lines), frame_lines[:2]
    assert sum(ln.startswith('[MEAN EVAL ') for ln in lines) == 2 and sum(ln.startswith('[TOTAL ') for ln in lines) == 1
    return res


@pytest.fixture(scope='module')
def runs(dev, datasets, tmp_path_factory):
    """evaluate() once per (config, --metrics): the HD config and a config whose result has the ground truth's size, host against
    `--metrics device --frame_group 4`; every ops.score_frames call of each run is recorded as (positional count, keywords)."""
    from refvsr_amd import ops
    tmp = tmp_path_factory.mktemp('runs')
    calls = []
    real = ops.score_frames

    def recorded(*a, **k):
        calls.append((len(a), dict(k)))
        return real(*a, **k)

    got = {}
    ops.score_frames = recorded
    try:
        for name in ('config_RefVSR_small_MFID_8K', 'config_RefVSR_small_L1'):
            for mode, extra in (('host', []), ('device', ['--frame_group', '4'])):
                del calls[:]
                got[name, mode] = _run(name, datasets[name], tmp, '%s_%s' % (name, mode), ['--metrics', mode] + extra)
                got[name, mode]['calls'] = list(calls)
    finally:
        ops.score_frames = real
    return got


def _deltas(runs, name):
    hst, dv = runs[name, 'host'], runs[name, 'device']
    return (max(abs(p - q) for p, q in zip(hst['psnr'], dv['psnr'])), max(abs(p - q) for p, q in zip(hst['ssim'], dv['ssim'])))


def test_evalrun_hd_config_device_metrics_against_the_host_run(runs):
    """PSNR within the host-float32-mean bar, every SSIM > 0 (it was zeroed before), the reference's line format (_run), one fused
    launch per network call."""
    name = 'config_RefVSR_small_MFID_8K'
    hst, dv = runs[name, 'host'], runs[name, 'device']
    assert not hst['calls']
    assert dv['calls'] and all(k == {'win': 7, 'down': 4} for _, k in dv['calls'])
    dp, ds = _deltas(runs, name)
    print('HD: max |dPSNR| %.3e dB, max |dSSIM| %.3e; SSIM %.5f .. %.5f' % (dp, ds, min(dv['ssim']), max(dv['ssim'])))
    assert dp <= 2e-5
    assert all(v > 0 for v in dv['ssim']) and all(v > 0 for v in hst['ssim']) and all(np.isfinite(v) for v in dv['psnr'])


def test_evalrun_hd_config_ssim_within_the_model_against_torch_bar(runs):
    """|dSSIM| between the host run (torch's float32 down-scale) and the device run (the correctly rounded one), largest of the ten
    frames, within the bar tests/test_score_down.py measures on the CPU as the largest of ten frames per case: 2 x 2.145e-09 =
    4.290e-09.  The device scores add nothing to it: the fused kernel equals the two-step path on the definition bit for bit (above),
    and the definition scored by the device is within 2.2e-15 of the float64 host SSIM at full size; what is compared here is torch's
    float32 image against its correct rounding, on the network's results."""
    from test_score_down import SSIM_BAR as SSIM_MODEL_BAR
    dp, ds = _deltas(runs, 'config_RefVSR_small_MFID_8K')
    print('HD: max |dSSIM| %.3e (bar %.3e)' % (ds, SSIM_MODEL_BAR))
    assert ds <= SSIM_MODEL_BAR


def test_evalrun_config_of_ground_truth_size_is_scored_as_before(runs):
    """The call it always was (two positional arguments, win = 7, no `down`), agreeing with the host as it always did."""
    name = 'config_RefVSR_small_L1'
    assert not runs[name, 'host']['calls']
    calls = runs[name, 'device']['calls']
    assert calls and all(n == 2 and k == {'win': 7} for n, k in calls)
    dp, ds = _deltas(runs, name)
    print('plain: max |dPSNR| %.3e dB, max |dSSIM| %.3e' % (dp, ds))
    assert dp <= 2e-5 and ds <= 1e-10


# |dSSIM| that two images up to d apart can have at all: per window |dS| <= d * 2 (49 / 48) (sa + sb) / (sa^2 + sb^2 + c2) <=
# d * 2 (49 / 48) / sqrt(2 c2) = 48.2 d (c2 = 9e-4; the luminance factor moves by less); d = 2.384e-07, two float32 ulp below 1
SSIM_WORST_CASE = 48.2 * 2.384e-07


def test_evalrun_hd_config_with_byte_frames_and_one_frame_per_call(dev, datasets, tmp_path):
    """--result_dtype / --input_dtype / --frame_group combine as for the other configs: the scores are those of the quantised result,
    the same bits with one frame and with four frames per call.  (SSIM against the host run at the worst-case bound of the arithmetic:
    this run is not the one the model-against-torch bar is set for.)"""
    name = 'config_RefVSR_small_MFID_8K'
    extra = ['--result_dtype', 'uint8', '--input_dtype', 'uint8']
    hst = _run(name, datasets[name], tmp_path, 'u8_host', extra + ['--metrics', 'host'])
    dv1 = _run(name, datasets[name], tmp_path, 'u8_dev1', extra + ['--metrics', 'device'])
    dv4 = _run(name, datasets[name], tmp_path, 'u8_dev4', extra + ['--metrics', 'device', '--frame_group', '4'])
    assert dv1['psnr'] == dv4['psnr'] and dv1['ssim'] == dv4['ssim']
    dp = max(abs(p - q) for p, q in zip(hst['psnr'], dv4['psnr']))
    ds = max(abs(p - q) for p, q in zip(hst['ssim'], dv4['ssim']))
    print('HD uint8: max |dPSNR| %.3e dB, max |dSSIM| %.3e' % (dp, ds))
    assert dp <= 2e-5 and ds <= SSIM_WORST_CASE and all(v > 0 for v in dv4['ssim'])
