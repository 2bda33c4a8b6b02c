"""Scores of the flag_HD_in configs, the part that runs without a GPU: the numpy definition of the bicubic down-scale
(refvsr_amd/metrics.py:down_bicubic_model, what refvsr_score_frames_down fuses into its tile staging) against
torch.nn.functional.interpolate on the CPU -- the arithmetic of models/loss/Loss.py:91-92 and, at an exact integer factor, the filter
of cv2.resize(INTER_CUBIC) in evaluation/eval_qual_quan.py:85-92 -- wrong definitions that the same bars must refuse, the composed
model, and the C entry point's declaration, export and argument checks with host integers standing in for device pointers.

Bars.  The model is the correctly rounded float32 image (float64 taps, one rounding); torch evaluates the same sixteen taps in float32
in an order of its own.  On exactly the frames of frames() -- FRAMES_PER_CASE = 10 frames for each of the two factors and four sizes --
the committed model measured
    max |D_model - D_torch|                       = 2.384e-07      (33 x 65 and larger; two float32 ulp of a sample near 1)
    max |PSNR(clip D_model) - PSNR(clip D_torch)| = 1.847e-06 dB   (7 x 7, factor 4; float64 means of both images)
    max |SSIM(D_model) - SSIM(D_torch)|           = 2.145e-09      (7 x 7, factor 2: three windows, nothing averages out)
and the tests assert twice those maxima (the margin is for torch's evaluation order, which may change between its builds).
Why ten frames per case: the maxima of the two scores are set by the 7 x 7 frames, whose SSIM is the mean of three windows, and one
such draw is no measurement of a maximum -- over the twenty 7 x 7 frames |dSSIM| runs from 1.5e-10 to 2.1e-09 and |dPSNR| from
1.3e-07 to 1.8e-06 dB (frame 0 of each case alone gives 5.798e-10 and 4.990e-07 dB).  tests/test_gpu_score_down.py holds the largest
of ten frames of an evaluation run to the SSIM bar, so the bar is the largest of ten frames per case here as well."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEASURED_IMAGE, MEASURED_PSNR_DB, MEASURED_SSIM = 2.384e-07, 1.847e-06, 2.145e-09
IMAGE_BAR, PSNR_BAR, SSIM_BAR = 2 * MEASURED_IMAGE, 2 * MEASURED_PSNR_DB, 2 * MEASURED_SSIM
SIZES = [(7, 7), (33, 65), (64, 96), (270, 480)]
FACTORS = [2, 4]
FRAMES_PER_CASE = 10


def frames(h, w, s, k=0):
    """(big result float32 [3, s h, s w], ground truth float32 [3, h, w]), frame k of the case: the ground truth is image content -- a
    frame of the project's synthetic clips (refvsr_amd.synth.make_clip, the generator of the evaluation tests' datasets) stretched to
    the full range -- and the result its bicubic up-scale + 0.03 randn, clamped: a plausible result whose down-scale overshoots
    [0, 1].  (A 7 x 7 draw whose down-scale happens to stay inside [0, 1] is passed over for the next one: the clamp must matter.)"""
    from refvsr_amd.synth import make_clip
    for j in itertools.count():
        n = k + FRAMES_PER_CASE * j
        g = torch.Generator().manual_seed(1000 * h + 10 * w + s + 100000 * n)
        gt = ((make_clip(1, h, w, seed=h + w + s + 100 * n, want_gt=False)[0][0] - 0.05) / 0.9).clamp(0, 1)
        up = F.interpolate(gt[None], scale_factor=s, mode='bicubic', align_corners=False)[0]
        big = (up + 0.03 * torch.randn(up.shape, generator=g)).clamp(0, 1)
        d = torch_down(big, s)
        if bool(((d < 0) | (d > 1)).any()):
            return big, gt


def torch_down(big, s):
    return F.interpolate(big[None], scale_factor=1.0 / s, mode='bicubic', align_corners=False)[0]


def psnr64(a, b):
    return 10.0 * math.log10(1.0 / float(((a.double() - b.double()) ** 2).mean()))


def deviation(d, big, gt, s, clamp_for_ssim=False):
    """(max |d - torch|, |dPSNR| of the clamped images, |dSSIM| of the unclamped ones) of a candidate down-scale d (numpy float32)."""
    from refvsr_amd import evalrun
    d = torch.from_numpy(np.ascontiguousarray(d))
    want = torch_down(big, s)
    assert want.shape == gt.shape == d.shape
    img = float((d - want).abs().max())
    dp = abs(psnr64(d.clamp(0, 1), gt) - psnr64(want.clamp(0, 1), gt))
    ds = abs(evalrun.ssim(d.clamp(0, 1) if clamp_for_ssim else d, gt) - evalrun.ssim(want, gt))
    return img, dp, ds


@pytest.mark.parametrize('s', FACTORS)
@pytest.mark.parametrize('h,w', SIZES)
def test_model_is_torchs_bicubic_down_scale(h, w, s):
    from refvsr_amd.metrics import down_bicubic_model
    worst = [0.0, 0.0, 0.0]
    for k in range(FRAMES_PER_CASE):
        big, gt = frames(h, w, s, k)
        d = down_bicubic_model(big.numpy(), s)
        assert d.dtype == np.float32 and d.shape == (3, h, w)
        assert ((d < 0.0) | (d > 1.0)).any(), 'no sample leaves [0, 1]: the clamp of the PSNR would go untested'
        worst = [max(a, b) for a, b in zip(worst, deviation(d, big, gt, s))]
    img, dp, ds = worst
    print('%dx%d / %d, %d frames: image %.3e  dPSNR %.3e dB  dSSIM %.3e' % (h, w, s, FRAMES_PER_CASE, img, dp, ds))
    assert img <= IMAGE_BAR and dp <= PSNR_BAR and ds <= SSIM_BAR


def _unclamped_taps(n, s):
    i0 = s * np.arange(n) + s // 2 - 2
    return [(i0 + k) % (s * n) for k in range(4)]          # a tap that leaves the axis wraps round instead of stopping at the border


def _shifted_taps(n, s):
    i0 = s * np.arange(n) + s // 2 - 1
    return [np.clip(i0 + k, 0, s * n - 1) for k in range(4)]


@pytest.mark.parametrize('h,w', [(33, 65), (64, 96)])
def test_wrong_definitions_miss_the_bars(h, w):
    """Controls: each wrong definition must fail the comparison the model passes, or the bars say nothing."""
    from refvsr_amd.metrics import DOWN_W, down_bicubic_model
    for s in FACTORS:
        big, gt = frames(h, w, s)
        typo = down_bicubic_model(big.numpy(), s, weights=(3.0 / 32.0,) + DOWN_W[1:])
        img, dp, ds = deviation(typo, big, gt, s)
        assert img > IMAGE_BAR and dp > PSNR_BAR and ds > SSIM_BAR, ('weight typo', s)
        shifted = down_bicubic_model(big.numpy(), s, taps=_shifted_taps)
        img, dp, ds = deviation(shifted, big, gt, s)
        assert img > IMAGE_BAR and dp > PSNR_BAR and ds > SSIM_BAR, ('shifted taps', s)
        good = down_bicubic_model(big.numpy(), s)
        img, dp, ds = deviation(good, big, gt, s, clamp_for_ssim=True)
        assert ds > SSIM_BAR and dp <= PSNR_BAR, ('clamp before SSIM', s)
    big, gt = frames(h, w, 2)
    img, dp, ds = deviation(down_bicubic_model(big.numpy(), 2, taps=_unclamped_taps), big, gt, 2)
    assert img > IMAGE_BAR and dp > PSNR_BAR and ds > SSIM_BAR, 'no border clamp at s = 2'
    # (at s = 4 no tap leaves the frame: the same replacement changes nothing)
    big4, _ = frames(h, w, 4)
    assert np.array_equal(down_bicubic_model(big4.numpy(), 4, taps=_unclamped_taps), down_bicubic_model(big4.numpy(), 4))


def test_taps_and_weights():
    from refvsr_amd.metrics import DOWN_W, _down_taps
    assert DOWN_W == (-0.09375, 0.59375, 0.59375, -0.09375) and sum(DOWN_W) == 1.0
    assert [t.tolist() for t in _down_taps(3, 4)] == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]]
    assert [t.tolist() for t in _down_taps(3, 2)] == [[0, 1, 3], [0, 2, 4], [1, 3, 5], [2, 4, 5]]
    # a constant frame stays the constant, and a frame of float32 values whose taps need no rounding is reproduced exactly
    from refvsr_amd.metrics import down_bicubic_model
    c = np.full((3, 28, 28), np.float32(0.3))
    assert np.all(down_bicubic_model(c, 4) == np.float32(0.3)) and np.all(down_bicubic_model(c, 2) == np.float32(0.3))


@pytest.mark.parametrize('s', FACTORS)
@pytest.mark.parametrize('h,w', [(7, 7), (33, 65), (40, 52)])
def test_composed_model_is_the_existing_model_on_the_down_scaled_frame(h, w, s):
    from refvsr_amd.metrics import down_bicubic_model, score_frames_down_model, score_frames_model
    big, gt = frames(h, w, s)
    d = down_bicubic_model(big.numpy(), s)
    m, q = score_frames_down_model(big.numpy(), gt.numpy(), s)
    assert m == score_frames_model(np.clip(d, 0, 1), gt.numpy())[0] and q == score_frames_model(d, gt.numpy())[1]
    assert m != score_frames_model(d, gt.numpy())[0]                     # (the clamp matters on these frames)
    m0, q0 = score_frames_down_model(big.numpy(), gt.numpy(), s, win=0)
    assert m0 == m and q0 == 0.0


# ------------------------------------------------------------------------------------------------ C-ABI, no GPU
@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_declared_exported_and_bound(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'int refvsr_score_frames_down\(([^;]*)\);', src)
    assert m and m.group(1).count(',') + 1 == len(hip.SIGNATURES['refvsr_score_frames_down']) == 14
    assert 'int down' in m.group(1) and 'Loss.py:91-92' in src and 'eval_qual_quan.py:85-92' in src
    assert 'refvsr_score_frames_down' in hip.EXPORTS and hasattr(L, 'refvsr_score_frames_down')
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15


def test_score_frames_down_rejects_bad_arguments_without_a_gpu(L):
    """Validation runs before any device work (host integers stand in for device pointers)."""
    from refvsr_amd import hip
    F32, U8, PL, HWC = hip.RESULT_F32, hip.RESULT_U8, hip.INGEST_PLANAR, hip.INGEST_HWC
    a, g, ws, sc = _ptrs(4096), _ptrs(8192), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    need = L.refvsr_score_workspace_bytes(1, 40, 52)
    err = lambda: L.refvsr_last_error().decode()
    call = lambda out=a, of=F32, gt=g, gf=F32, gl=PL, n=1, h=40, w=52, down=4, win=7, wsp=ws, nb=need, scores=sc: \
        L.refvsr_score_frames_down(out, of, gt, gf, gl, n, h, w, down, win, wsp, nb, scores, None)
    assert call(out=None) != 0 and 'score_frames_down: null frame table' in err()
    assert call(gt=None) != 0 and 'null frame table' in err()
    for down in (3, 1, 0, 8, -2):
        assert call(down=down) != 0 and 'down must be 2 or 4' in err()
    for h, w in ((6, 52), (40, 6), (0, 0)):
        assert call(h=h, w=w) != 0 and 'at least 7' in err()
    assert call(nb=need - 1) != 0 and 'workspace too small' in err()
    assert call(down=2, nb=need - 1) != 0 and 'workspace too small' in err()
    assert call(n=17) != 0 and '1..16 frames' in err()
    assert call(win=5) != 0 and 'win must be 7' in err()
    assert call(gf=F32, gl=HWC) != 0 and 'interleaved' in err()
    assert call(gf=U8, gl=2) != 0 and 'layout' in err()
    assert call(out=_ptrs(4098)) != 0 and 'aligned (frame 0)' in err()
    assert call(wsp=None) != 0 and 'null workspace' in err()


def test_ops_score_frames_takes_down():
    import inspect
    from refvsr_amd import ops
    sig = inspect.signature(ops.score_frames)
    assert list(sig.parameters) == ['outs', 'gts', 'win', 'down'] and sig.parameters['down'].default == 1 and sig.parameters['win'].default == 7
    with pytest.raises(RuntimeError, match='down must be 1, 2 or 4'):
        ops.score_frames([torch.zeros(3, 21, 21)], [torch.zeros(3, 7, 7)], down=3)
