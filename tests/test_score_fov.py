"""Field-of-view scoring, the part that runs without a GPU: metrics.fov_scores_host and fov_table(score_regions_model(..)) -- the numpy
model of refvsr_score_regions: tiles of pixel centres, symmetric-reflect staging, per-thread accumulation, reduction order -- against a
literal float64 restatement of evaluation/eval_quan_FOV.py:155-192 on evaluation/metrics.py:18-30 written out below (h x w x 3 masks,
np.sum(x * mask) / np.sum(mask), scipy.ndimage.uniform_filter(size=7) for the five moments); the argument validation of
refvsr_score_regions with host memory standing in for device pointers; the CLI switch, the block writer and the traced op.

Bars (they come from the arithmetic, as in tests/test_score.py, and are the same numbers): every SSIM mean within 1e-10, every region's
squared-error sum within 1e-12 relative, every PSNR within 1e-9 dB of the float64 restatement.  A difference of two rectangle sums
amplifies a sum's relative error by at most full / smallest region (< 12 at these sizes: the 50-60 % ring holds 11 % of the frame)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_score import pairs  # noqa: E402

SSIM_BAR, SSE_REL, PSNR_BAR = 1e-10, 1e-12, 1e-9
SIZES = [(20, 20), (21, 27), (33, 65), (40, 52), (70, 134)]
KEYS = [1, 0.9, 0.8, 0.7, 0.6, 0.5]


# ------------------------------------------------------------------------------------------------ the yardstick
def reference_maps(a, b):
    """(a - b)^2 and skimage's full SSIM map (structural_similarity defaults, data range 1) of h x w x 3 float64 images."""
    from scipy.ndimage import uniform_filter
    s = np.empty_like(a)
    c1, c2, norm = 0.01 ** 2, 0.03 ** 2, 49.0 / 48.0
    for c in range(3):
        x, y = a[..., c], b[..., c]
        ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
        uxx, uyy, uxy = uniform_filter(x * x, size=7), uniform_filter(y * y, size=7), uniform_filter(x * y, size=7)
        vx, vy, vxy = norm * (uxx - ux * ux), norm * (uyy - uy * uy), norm * (uxy - ux * uy)
        s[..., c] = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return (a - b) ** 2, s


def reference_fov(a, b):
    """eval_quan_FOV.py:155-192 for one pair a, b [3,h,w]: (table [6][fi, fo, fr][psnr, ssim], the masked squared-error sums
    [6][3], the crop ratios).  PSNR of a zero error is inf (the reference would divide by zero)."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64).transpose(1, 2, 0)
    b = np.asarray(b, dtype=np.float32).astype(np.float64).transpose(1, 2, 0)
    d2, s = reference_maps(a, b)
    h, w, _ = a.shape
    psnr_of = lambda m: float('inf') if m == 0 else 10 * math.log10(1.0 / m)
    masked = lambda mask: (psnr_of(np.sum(d2 * mask) / np.sum(mask)), np.sum(s * mask) / np.sum(mask), np.sum(d2 * mask))
    table, sse, ratios = np.zeros((6, 3, 2)), np.zeros((6, 3)), []
    for k, key in enumerate(KEYS):
        if key == 1.:
            mask_fi = np.ones_like(a)
            fi = (psnr_of(np.mean(d2)), np.mean(s[3:h - 3, 3:w - 3]), np.sum(d2))
            fo = (0, 0, 0)
        else:
            crop_ratio = int(1 / ((1 - key) / 2))
            ratios.append(crop_ratio)
            mask_fi = np.zeros_like(a)
            mask_fi[h // crop_ratio:h - h // crop_ratio, w // crop_ratio:w - w // crop_ratio] = 1.
            fi = masked(mask_fi)
            mask_fo = np.ones_like(a)
            mask_fo[h // crop_ratio:h - h // crop_ratio, w // crop_ratio:w - w // crop_ratio] = 0.
            fo = masked(mask_fo)
        if key > 0.5:
            mask_fr = mask_fi.copy()
            mask_fr[h // 4:h - h // 4, w // 4:w - w // 4] = 0.
            fr = masked(mask_fr)
        else:
            fr = (0, 0, 0)
        for j, v in enumerate((fi, fo, fr)):
            table[k, j] = v[:2]
            sse[k, j] = v[2]
    return table, sse, ratios


def table_sse(sums):
    """The squared-error sums [6][3] that fov_table forms from rectangle sums [7][2] (full, valid, R(0.9) .. R(0.5))."""
    e = np.asarray(sums)[:, 0]
    out = np.zeros((6, 3))
    out[0] = (e[0], 0.0, e[0] - e[6])
    for k in range(1, 6):
        out[k] = (e[k + 1], e[0] - e[k + 1], e[k + 1] - e[6] if k < 5 else 0.0)
    return out


def check_table(got, want, what, got_sse=None, want_sse=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == (6, 3, 2) and got.dtype == np.float64
    assert got[0, 1].tolist() == [0.0, 0.0] and got[5, 2].tolist() == [0.0, 0.0], what          # exact 0.0 where the reference reports 0
    fin = np.isfinite(want[..., 0])
    assert np.array_equal(np.isfinite(got[..., 0]), fin), what
    dp = float(np.max(np.abs(got[..., 0][fin] - want[..., 0][fin]))) if fin.any() else 0.0
    ds = float(np.max(np.abs(got[..., 1] - want[..., 1])))
    de = 0.0
    if got_sse is not None:
        de = float(np.max(np.abs(got_sse - want_sse) / np.maximum(want_sse, 1e-300)))
    print('%s: max |dPSNR| %.3e dB, max |dSSIM| %.3e, max rel dSSE %.3e' % (what, dp, ds, de))
    assert dp <= PSNR_BAR and ds <= SSIM_BAR and de <= SSE_REL, what


# ------------------------------------------------------------------------------------------------ host path and kernel model
@pytest.fixture(scope='module')
def cases():
    """(name, h, w, a, b, reference table, reference sse) computed once for every size and pair kind."""
    pytest.importorskip('scipy')
    out = []
    for h, w in SIZES:
        for name, a, b in pairs(h, w, 7 * h + w):
            table, sse, ratios = reference_fov(a.numpy(), b.numpy())
            assert ratios == [20, 10, 6, 5, 4]
            out.append(('%s %dx%d' % (name, h, w), h, w, a, b, table, sse))
    return out


def test_crop_ratios_and_rectangles():
    from refvsr_amd.metrics import FOV_KEYS, fov_crop_ratio, fov_rects
    assert list(FOV_KEYS) == KEYS
    assert [fov_crop_ratio(k) for k in KEYS[1:]] == [20, 10, 6, 5, 4]
    assert fov_rects(1080, 1920) == [(0, 1080, 0, 1920), (3, 1077, 3, 1917), (54, 1026, 96, 1824), (108, 972, 192, 1728),
                                     (180, 900, 320, 1600), (216, 864, 384, 1536), (270, 810, 480, 1440)]
    assert fov_rects(20, 20)[2] == (1, 19, 1, 19)
    for h, w in ((19, 40), (40, 19), (7, 7)):
        with pytest.raises(ValueError, match='at least 20 x 20'):
            fov_rects(h, w)


def test_host_path_agrees_with_the_reference_restatement(cases):
    from refvsr_amd.metrics import fov_rects, fov_scores_host, host_region_sums
    for what, h, w, a, b, table, sse in cases:
        got = fov_scores_host(a, b)
        check_table(got, table, 'host ' + what, table_sse(host_region_sums(a, b, fov_rects(h, w))), sse)
        assert np.array_equal(got, fov_scores_host(a.numpy(), b.numpy()))          # torch or numpy input


def test_model_agrees_with_the_reference_restatement(cases):
    from refvsr_amd.metrics import fov_rects, fov_table, score_regions_model
    for what, h, w, a, b, table, sse in cases:
        sums = score_regions_model(a.numpy(), b.numpy(), fov_rects(h, w))
        check_table(fov_table(sums, h, w), table, 'model ' + what, table_sse(sums), sse)


def test_key_1_fi_pair_equals_the_frame_scorer(cases):
    from refvsr_amd.metrics import fov_rects, fov_table, psnr_from_mse, score_frames_model, score_regions_model
    for what, h, w, a, b, _, _ in cases:
        if not what.startswith('8bit'):
            continue
        m, s = score_frames_model(a.numpy(), b.numpy())
        sums = score_regions_model(a.numpy(), b.numpy(), fov_rects(h, w))
        t = fov_table(sums, h, w)
        assert abs(sums[0, 0] / (3.0 * h * w) - m) <= SSE_REL * m, what
        assert abs(t[0, 0, 0] - psnr_from_mse(m)) <= PSNR_BAR and abs(t[0, 0, 1] - s) <= SSIM_BAR, what


@pytest.mark.parametrize('h,w', [(20, 20), (33, 65), (70, 134)])
def test_identical_pair_is_inf_and_one_everywhere(h, w):
    from refvsr_amd.metrics import fov_rects, fov_scores_host, fov_table, score_regions_model
    a = torch.rand(3, h, w, generator=torch.Generator().manual_seed(h)).numpy()
    for t in (fov_scores_host(a, a.copy()), fov_table(score_regions_model(a, a.copy(), fov_rects(h, w)), h, w)):
        zero = np.zeros((6, 3), dtype=bool)
        zero[0, 1] = zero[5, 2] = True
        assert np.all(t[..., 0][~zero] == float('inf')) and np.all(t[..., 1][~zero] == 1.0)
        assert np.all(t[zero] == 0.0)


def test_model_sums_of_arbitrary_rectangles():
    """Overlapping, non-nested rectangles, 1 x 1 corners and a rectangle across a tile boundary against plain slicing."""
    from refvsr_amd.metrics import host_region_sums, score_regions_model
    h, w = 40, 70
    _, a, b = list(pairs(h, w, 11))[1]
    rects = [(0, 1, 0, 1), (0, 1, w - 1, w), (h - 1, h, 0, 1), (h - 1, h, w - 1, w), (30, 36, 60, 68), (5, 33, 2, 9), (0, h, 63, 65), (31, 33, 0, w)]
    got, want = score_regions_model(a.numpy(), b.numpy(), rects), host_region_sums(a, b, rects)
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= SSE_REL * want[:, 0])
    cnt = np.array([3.0 * (r[1] - r[0]) * (r[3] - r[2]) for r in rects])
    assert np.all(np.abs(got[:, 1] - want[:, 1]) / cnt <= SSIM_BAR)


def test_host_path_full_size_pair():
    pytest.importorskip('scipy')
    from refvsr_amd.metrics import fov_scores_host
    g = torch.Generator().manual_seed(1080)
    u = torch.randint(0, 256, (3, 1080, 1920), generator=g)
    v = (u + torch.randint(-6, 7, (3, 1080, 1920), generator=g)).clamp(0, 255)
    a, b = u.float() / 255.0, v.float() / 255.0
    table, _, _ = reference_fov(a.numpy(), b.numpy())
    check_table(fov_scores_host(a, b), table, 'host 8bit 1080x1920')


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
    from refvsr_amd import hip, metrics
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_SCORE_MAX_RECTS (\d+)', src)
    assert m and int(m.group(1)) == hip.SCORE_MAX_RECTS == L.refvsr_score_max_rects() == metrics.MAX_RECTS == 8
    assert {'refvsr_score_regions', 'refvsr_score_max_rects', 'refvsr_score_regions_workspace_bytes'} <= set(hip.EXPORTS)
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15
    assert 'eval_quan_FOV.py:155-192' in src and 'evaluation/metrics.py:18-30' in src


def test_workspace_bytes(L):
    wb = L.refvsr_score_regions_workspace_bytes
    assert wb(1, 7, 7, 1) == 3 * 2 * 8 and wb(1, 32, 64, 7) == 3 * 7 * 16 and wb(1, 33, 65, 7) == 4 * 3 * 7 * 16
    assert wb(1, 1080, 1920, 7) == 3 * 34 * 30 * 7 * 16 and wb(16, 1080, 1920, 8) == 16 * 3 * 34 * 30 * 8 * 16
    for bad in ((0, 40, 40, 7), (1, 6, 40, 7), (1, 40, 6, 7), (1, 40, 40, 0), (1, 40, 40, 9)):
        assert wb(*bad) == 0


def test_score_regions_rejects_bad_arguments_without_a_gpu(L):
    """Validation runs before any device work (host integers stand in for device pointers)."""
    from refvsr_amd import hip
    F32, F16, U8, PL, HWC = hip.RESULT_F32, hip.RESULT_F16, hip.RESULT_U8, hip.INGEST_PLANAR, hip.INGEST_HWC
    a, g, ws, sm = _ptrs(4096), _ptrs(8192), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    two = ints(0, 40, 0, 52, 3, 37, 3, 49)
    need = L.refvsr_score_regions_workspace_bytes(1, 40, 52, 2)
    err = lambda: L.refvsr_last_error().decode()
    call = lambda out=a, of=F32, gt=g, gf=F32, gl=PL, n=1, h=40, w=52, rects=two, nr=2, wsp=ws, nb=need, sums=sm: \
        L.refvsr_score_regions(out, of, gt, gf, gl, n, h, w, rects, nr, wsp, nb, sums, None)
    assert call(out=None) != 0 and 'null frame table' in err()
    for n in (0, 17):
        assert call(n=n) != 0 and '1..16 frames' in err()
    for h, w in ((6, 52), (40, 6)):
        assert call(h=h, w=w) != 0 and 'at least 7' in err()
    for nr in (0, 9, -1):
        assert call(nr=nr) != 0 and '1..8 rectangles' in err()
    assert call(rects=None) != 0 and 'null rectangle table' in err()
    for empty in ((5, 5, 0, 52), (0, 40, 9, 9), (8, 4, 0, 52)):
        assert call(rects=ints(0, 40, 0, 52, *empty)) != 0 and 'rectangle 1 is empty' in err()
    for past in ((0, 41, 0, 52), (0, 40, 0, 53), (-1, 40, 0, 52), (0, 40, -2, 52)):
        assert call(rects=ints(*past), nr=1) != 0 and 'rectangle 0 leaves the frame' in err()
    assert call(of=3) != 0 and 'result format' in err()
    assert call(gf=F16) != 0 and 'ground-truth format' in err()
    assert call(gf=U8, gl=2) != 0 and 'layout' in err()
    assert call(gf=F32, gl=HWC) != 0 and 'interleaved' in err()
    assert call(out=_ptrs(4098)) != 0 and 'aligned (frame 0)' in err()
    assert call(out=_ptrs(0)) != 0 and 'null pointer (frame 0)' in err()
    assert call(wsp=None) != 0 and 'null workspace' in err()
    assert call(sums=None) != 0 and 'null workspace' in err()
    assert call(sums=ctypes.c_void_p((1 << 21) + 8)) != 0 and '16-byte' in err()
    assert call(nb=need - 1) != 0 and 'workspace too small' in err()
    assert call(nr=1, nb=need // 2 - 1) != 0 and 'workspace too small' in err()


# ------------------------------------------------------------------------------------------------ CLI, block writer, traced op
def _base(tmp_path):
    return ['--mode', 'unit', '--data_offset', str(tmp_path), '--output_offset', str(tmp_path / 'o')]


def test_cli_selects_the_fov_scorer(tmp_path, monkeypatch):
    from refvsr_amd import evalrun
    cfg = evalrun.build_config(_base(tmp_path) + ['--config', 'config_RefVSR_small_L1', '--eval_mode', 'quan_FOV'])
    assert cfg.EVAL.eval_mode == 'quan_FOV' and evalrun.build_config(_base(tmp_path)).EVAL.eval_mode == 'qual_quan'
    # the dispatch is evaluate()'s first step: stop it at the data set and look at what it chose
    seen = {}

    class Stop(Exception):
        pass

    class Net(object):
        pass

    def clipset(config):
        seen['root'] = config.EVAL.LOG_DIR.save
        raise Stop()

    monkeypatch.setattr(evalrun, 'ClipSet', clipset)
    with pytest.raises(Stop):
        evalrun.evaluate(cfg, net=Net(), log=lambda *_: None)
    assert os.path.isdir(os.path.join(seen['root'], 'quan_FOV', 'seeded'))
    cfg.flag_HD_in = True
    with pytest.raises(RuntimeError, match='flag_HD_in configs are not supported'):
        evalrun.evaluate(cfg, net=Net(), log=lambda *_: None)
    cfg.EVAL.eval_mode = 'qual_quan'                                   # (the existing mode still takes such a config)
    with pytest.raises(Stop):
        evalrun.evaluate(cfg, net=Net(), log=lambda *_: None)


def test_block_writer_reproduces_the_reference_blocks():
    from refvsr_amd import evalrun
    t = np.zeros((6, 3, 2))
    t[:, 0, 0] = [30.5, 31.25, 32, 33, 34, 35.123456]
    t[:, 1, 0] = [0, 29.5, 29, 28.5, 28, 27.5]
    t[:, 2, 0] = [30.1, 30.2, 30.3, 30.4, 30.5, 0]
    t[:, 0, 1] = [0.9, 0.91, 0.92, 0.93, 0.94, 0.95]
    t[:, 1, 1] = [0, 0.89, 0.88, 0.87, 0.86, 0.85]
    t[:, 2, 1] = [0.901, 0.902, 0.903, 0.904, 0.905, 0]
    rows = ('[PSNR-FOV_in  ] (0-100.0%: 30.50000, 0-90.0%: 31.25000, 0-80.0%: 32.00000, 0-70.0%: 33.00000, 0-60.0%: 34.00000, 0-50.0%: 35.12346, )\n'
            '[PSNR-FOV_out ] (100.0-100%: 0.00000, 90.0-100%: 29.50000, 80.0-100%: 29.00000, 70.0-100%: 28.50000, 60.0-100%: 28.00000, 50.0-100%: 27.50000, )\n'
            '[PSNR-FOV_ring] (50.0-100.0%: 30.10000, 50.0-90.0%: 30.20000, 50.0-80.0%: 30.30000, 50.0-70.0%: 30.40000, 50.0-60.0%: 30.50000, 50.0-50.0%: 0.00000, )\n'
            '[SSIM-FOV_in  ] (0-100.0%: 0.90000, 0-90.0%: 0.91000, 0-80.0%: 0.92000, 0-70.0%: 0.93000, 0-60.0%: 0.94000, 0-50.0%: 0.95000, )\n'
            '[SSIM-FOV_out ] (100.0-100%: 0.00000, 90.0-100%: 0.89000, 80.0-100%: 0.88000, 70.0-100%: 0.87000, 60.0-100%: 0.86000, 50.0-100%: 0.85000, )\n'
            '[SSIM-FOV_ring] (50.0-100.0%: 0.90100, 50.0-90.0%: 0.90200, 50.0-80.0%: 0.90300, 50.0-70.0%: 0.90400, 50.0-60.0%: 0.90500, 50.0-50.0%: 0.00000, ')
    mean = evalrun.fov_block('[MEAN EVAL {}|{}|{}][{}/{}] ({:.5f}sec) \n'.format('unit', 'RealMCVSR', '0001', 0, 2, 0.25), t, ') \n\n')
    assert mean == '[MEAN EVAL unit|RealMCVSR|0001][0/2] (0.25000sec) \n' + rows + ') \n\n'
    total = evalrun.fov_block('\n[TOTAL {}|{}] \n'.format('RefVSR_small_L1', 'RealMCVSR'), t, ') ({:.5f}sec)\n\n'.format(0.5))
    assert total == '\n[TOTAL RefVSR_small_L1|RealMCVSR] \n' + rows + ') (0.50000sec)\n\n'


def test_fake_op_shape_and_dtype():
    import refvsr_amd.torch_ops as t
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'score_regions' in t.OP_NAMES and hasattr(torch.ops.refvsr, 'score_regions')
    assert str(torch.ops.refvsr.score_regions.default._schema) == 'refvsr::score_regions(Tensor outs, Tensor gts, SymInt[] rects) -> Tensor'
    with FakeTensorMode():
        a = torch.empty((5, 3, 40, 52), dtype=torch.uint8, device='cuda')
        g = torch.empty((5, 40, 52, 3), dtype=torch.uint8, device='cuda').permute(0, 3, 1, 2)
        y = torch.ops.refvsr.score_regions(a, g, [0, 40, 0, 52, 3, 37, 3, 49])
        assert y.shape == (5, 2, 2) and y.dtype == torch.float64
