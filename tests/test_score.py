"""Device scorer, the part that runs without a GPU: the numpy model of the kernel (refvsr_amd/metrics.py:score_frames_model -- tile
decomposition, direct 7-term sums, reduction order of csrc/score.hip) against the float64 host definitions, the argument validation of
refvsr_score_frames with host memory standing in for device pointers, the CLI switch and the traced op.

Bars (they come from the arithmetic, not from what the code gives): both SSIMs are float64 and differ in summation order only -- a few
ulp of 1 per window over a denominator >= c2 = 9e-4, ~1e-12 -- so |dSSIM| <= 1e-10; mse relative 1e-12 and PSNR 1e-9 dB against the
float64 restatement; PSNR within 2e-5 dB of evalrun.psnr, whose mean is float32 (its own rounding measured up to 4.6e-6 dB)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SSIM_BAR, MSE_REL, PSNR64_BAR, PSNR32_BAR = 1e-10, 1e-12, 1e-9, 2e-5
SIZES = [(7, 7), (8, 130), (33, 65), (40, 52), (64, 96)]


def pairs(h, w, seed):
    """(name, a, b) float32 [3,h,w]: noise, an 8-bit pair, flat + 1/255, an 8-bit-quantised ramp (the worst case for cancellation)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(3, h, w, generator=g)
    yield 'noise', a, (a + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    u = torch.randint(0, 256, (3, h, w), generator=g)
    v = (u + torch.randint(-6, 7, (3, h, w), generator=g)).clamp(0, 255)
    yield '8bit', u.float() / 255.0, v.float() / 255.0
    flat = torch.full((3, h, w), 0.5)
    yield 'flat', flat, flat + 1.0 / 255.0
    ramp = torch.linspace(0, 1, h * w).view(1, h, w).repeat(3, 1, 1)
    q = torch.round(ramp * 255.0) / 255.0
    yield 'ramp', ramp, q


def check_against_host(m, s, a, b, what):
    from refvsr_amd import evalrun
    from refvsr_amd.metrics import psnr_from_mse
    want_s = evalrun.ssim(a, b)
    want_m = float(((a.double() - b.double()) ** 2).mean())
    print('%s: dssim %.3e  mse rel %.3e' % (what, abs(s - want_s), abs(m - want_m) / max(want_m, 1e-300)))
    assert abs(s - want_s) <= SSIM_BAR, what
    assert abs(m - want_m) <= MSE_REL * want_m, what
    if want_m > 0:
        assert abs(psnr_from_mse(m) - 10.0 * math.log10(1.0 / want_m)) <= PSNR64_BAR, what
        assert abs(psnr_from_mse(m) - evalrun.psnr(a, b)) <= PSNR32_BAR, what


@pytest.mark.parametrize('h,w', SIZES)
def test_model_agrees_with_the_host_definitions(h, w):
    from refvsr_amd.metrics import score_frames_model
    for name, a, b in pairs(h, w, 7 * h + w):
        m, s = score_frames_model(a.numpy(), b.numpy())
        check_against_host(m, s, a, b, '%s %dx%d' % (name, h, w))
        m0, s0 = score_frames_model(a.numpy(), b.numpy(), win=0)
        assert m0 == m and s0 == 0.0


@pytest.mark.parametrize('h,w', [(7, 7), (33, 65), (40, 140)])
def test_model_identical_pair_is_exactly_one(h, w):
    from refvsr_amd.metrics import psnr_from_mse, score_frames_model
    a = torch.rand(3, h, w, generator=torch.Generator().manual_seed(h)).numpy()
    m, s = score_frames_model(a, a.copy())
    assert m == 0.0 and s == 1.0 and psnr_from_mse(m) == float('inf')


def test_psnr_from_mse():
    from refvsr_amd.metrics import psnr_from_mse
    assert psnr_from_mse(0.01) == pytest.approx(20.0, abs=1e-12) and psnr_from_mse(0.0) == float('inf')
    assert psnr_from_mse(np.float64(1.0)) == 0.0


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


def test_exports_and_constants(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_SCORE_MAX_FRAMES (\d+)', src)
    assert m and int(m.group(1)) == hip.SCORE_MAX_FRAMES == L.refvsr_score_max_frames() == 16
    assert {'refvsr_score_frames', 'refvsr_score_max_frames', 'refvsr_score_workspace_bytes'} <= set(hip.EXPORTS)
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15


def test_workspace_bytes_is_monotone(L):
    wb = L.refvsr_score_workspace_bytes
    assert wb(1, 7, 7) == 3 * 2 * 8 and wb(0, 40, 40) == 0 and wb(1, 6, 40) == 0 and wb(1, 40, 6) == 0
    for h, w in ((7, 7), (38, 70), (39, 71), (270, 480), (1080, 1920)):
        v = [wb(n, h, w) for n in range(1, 17)]
        assert all(y > x for x, y in zip(v, v[1:])) and v[0] > 0 and v[15] == 16 * v[0]
    assert wb(1, 38, 70) < wb(1, 39, 70) and wb(1, 38, 70) < wb(1, 38, 71)
    seq = [wb(1, s, 2 * s) for s in (7, 40, 100, 270, 540, 1080)]
    assert seq == sorted(seq) and len(set(seq)) == len(seq)
    assert wb(1, 1080, 1920) == 3 * 34 * 30 * 16


def test_score_frames_rejects_bad_arguments_without_a_gpu(L):
    """Validation runs before any device work (the test_capi.py pattern: host integers stand in for device pointers)."""
    from refvsr_amd import hip
    F32, F16, U8, PL, HWC = hip.RESULT_F32, hip.RESULT_F16, hip.RESULT_U8, hip.INGEST_PLANAR, hip.INGEST_HWC
    a, g, ws, sc = _ptrs(4096), _ptrs(8192), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    need = L.refvsr_score_workspace_bytes(1, 40, 52)
    err = lambda: L.refvsr_last_error().decode()
    call = lambda out=a, of=F32, gt=g, gf=F32, gl=PL, n=1, h=40, w=52, win=7, wsp=ws, nb=need, scores=sc: \
        L.refvsr_score_frames(out, of, gt, gf, gl, n, h, w, win, wsp, nb, scores, None)
    assert call(out=None) != 0 and 'null frame table' in err()
    assert call(gt=None) != 0 and 'null frame table' in err()
    for n in (0, -1, 17):
        assert call(n=n) != 0 and '1..16 frames' in err()
    two_a, two_g = _ptrs(4096, 0), _ptrs(8192, 12288)
    assert call(out=two_a, gt=two_g, n=2, nb=2 * need) != 0 and 'null pointer (frame 1)' in err()
    assert call(out=_ptrs(4096, 4096), gt=_ptrs(8192, 0), n=2, nb=2 * need) != 0 and 'null pointer (frame 1)' in err()
    for h, w in ((6, 52), (40, 6), (0, 0), (-7, 52)):
        assert call(h=h, w=w) != 0 and 'at least 7' in err()
    for win in (5, 3, 1, 11, -7):
        assert call(win=win) != 0 and 'win must be 7' in err()
    for of in (-1, 3):
        assert call(of=of) != 0 and 'result format' in err()
    for gf in (-1, F16, 3):
        assert call(gf=gf) != 0 and 'ground-truth format' in err()
    for gl in (-1, 2):
        assert call(gf=U8, gl=gl) != 0 and 'layout' in err()
    assert call(gf=F32, gl=HWC) != 0 and 'interleaved' in err()
    assert call(out=_ptrs(4098)) != 0 and 'aligned (frame 0)' in err()
    assert call(gt=_ptrs(8194)) != 0 and 'aligned (frame 0)' in err()
    assert call(out=_ptrs(4097), of=F16) != 0 and 'aligned' in err()
    assert call(wsp=None) != 0 and 'null workspace' in err()
    assert call(scores=None) != 0 and 'null workspace' in err()
    assert call(wsp=ctypes.c_void_p((1 << 20) + 8)) != 0 and '16-byte' in err()
    assert call(nb=need - 1) != 0 and 'workspace too small' in err()
    assert call(n=2, out=_ptrs(4096, 4096), gt=_ptrs(8192, 8192), nb=need) != 0 and 'workspace too small' in err()


# ------------------------------------------------------------------------------------------------ CLI switch, traced op
def test_cli_metrics_switch(tmp_path):
    from refvsr_amd import evalrun
    base = ['--config', 'config_RefVSR_small_L1', '--mode', 'unit', '--data_offset', str(tmp_path), '--output_offset', str(tmp_path / 'o')]
    assert evalrun.build_config(base).EVAL.metrics == 'host'
    assert evalrun.build_config(base + ['--metrics', 'device']).EVAL.metrics == 'device'
    assert evalrun.build_config(base + ['--metrics', 'host']).EVAL.metrics == 'host'
    with pytest.raises(SystemExit):
        evalrun.build_config(base + ['--metrics', 'gpu'])


def test_fake_op_shape_and_dtype():
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'score_frames' in t.OP_NAMES and hasattr(torch.ops.refvsr, 'score_frames')
    assert str(torch.ops.refvsr.score_frames.default._schema) == 'refvsr::score_frames(Tensor outs, Tensor gts, SymInt win) -> Tensor'
    with FakeTensorMode():
        a = torch.empty((5, 3, 40, 52), dtype=torch.uint8, device='cuda')
        g = torch.empty((5, 40, 52, 3), dtype=torch.uint8, device='cuda').permute(0, 3, 1, 2)
        y = torch.ops.refvsr.score_frames(a, g, 7)
        assert y.shape == (5, 2) and y.dtype == torch.float64
