"""Bit-exact parity of the per-frame preparation's fused / re-tiled kernels with the launches they replace: the LDS-tile patch-row
kernel vs the gather kernel (refvsr_set_match_patches_kernel), the flagged-only LR lo rows vs the full array, the one-launch
SPyNet pyramid vs five avgpool2 calls, the one-launch frame preparation vs its seven launches, and a whole stream with and without
REFVSR_LEGACY_PREP.  Every comparison is torch.equal."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from refvsr_amd import hip
    hip.lib()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def weights(dev, small_cfg, small_sd):
    from refvsr_amd.engine import Weights
    return Weights(small_cfg, small_sd, dev)


def _patches(feat, want_lo, kernel):
    from refvsr_amd import ops
    ops.set_match_patches_kernel(kernel)
    try:
        return ops.match_patches(feat, 256, want_lo=want_lo)
    finally:
        ops.set_match_patches_kernel(1)


MAPS = ['normal', 'zero', 'large']


def _feature_map(kind, h, w, dev):
    g = torch.Generator().manual_seed(1000 * h + w)
    if kind == 'zero':
        return torch.zeros(16, h, w, device=dev)
    f = torch.randn(16, h, w, generator=g)
    return (f * 1e4 if kind == 'large' else f).to(dev)


@pytest.mark.parametrize('want_lo', [False, True])
@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (9, 15), (17, 33), (34, 70)])
def test_match_patches_lds_tile_equals_gather_kernel(dev, h, w, want_lo):
    """Fewer pixels than a workgroup (2x2, 3x5, 9x15), strips that cross rows (every size: w < 256), reflection on all four sides,
    pixel counts that are no multiple of 128 or of the 256-pixel strip (561, 2380: the last strip is partial)."""
    n = h * w
    for kind in MAPS:
        f = _feature_map(kind, h, w, dev)
        old = _patches(f, want_lo, 0)
        new = _patches(f, want_lo, 1)
        assert len(old) == len(new) == (3 if want_lo else 2)
        assert torch.equal(old[0], new[0]), (kind, 'rows')            # incl. the zero pad rows and the zero slot of every row
        assert torch.equal(old[1], new[1]), (kind, 'inv_norm')
        if want_lo:
            assert torch.equal(old[2], new[2]), (kind, 'rows_lo')
        if kind == 'zero':
            assert float(new[1].min()) == float(new[1].max()) > 9e11 and float(new[0].abs().max()) == 0.0      # the 1e-12 clamp
        else:
            assert float(new[0][:n, :144].abs().max()) > 0.0


def _match_chain(lr_f, ref_f, legacy):
    """The matching of Engine.feature_match on given feature maps: legacy = gather kernel + full LR lo rows."""
    from refvsr_amd import ops
    ops.set_match_patches_kernel(0 if legacy else 1)
    try:
        if legacy:
            lr_rows, inv_lr, lr_lo = ops.match_patches(lr_f, ops.hip.MATCH_COLBLOCK, want_lo=True)
        else:
            (lr_rows, inv_lr), lr_lo = ops.match_patches(lr_f, ops.hip.MATCH_COLBLOCK), None
        ref_rows, inv_ref, ref_lo = ops.match_patches(ref_f, ops.hip.MATCH_ROWCHUNK, want_lo=True)
    finally:
        ops.set_match_patches_kernel(1)
    n_lr, n_ref = lr_f.shape[1] * lr_f.shape[2], ref_f.shape[1] * ref_f.shape[2]
    cand, cval = ops.match_top2(ref_rows, n_ref, lr_rows, n_lr, 1)
    return ops.match_refine(lr_f, ref_f, inv_lr, inv_ref, cand, cval, ops.MATCH_EXACT_MARGIN, (lr_rows, lr_lo), (ref_rows, ref_lo))


def _periodic(c, h, w, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    cell = torch.rand(c, 4, 4, generator=g) * scale
    return cell.repeat(1, (h + 3) // 4, (w + 3) // 4)[:, :h, :w].contiguous()


@pytest.mark.parametrize('h,w', [(16, 24), (34, 70)])
def test_flagged_lo_rows_periodic_feature_map(dev, h, w):
    """Feature maps of period 4 in both directions: an interior LR patch equals several reference patches exactly, so the two best
    fp16 scores tie and the column goes to the exhaustive search, which reads its LR lo row."""
    lr_f = _periodic(16, h, w, 7).to(dev)
    ref_f = _periodic(16, h // 2, w // 2, 7).to(dev)
    conf_o, idx_o, fl_o = _match_chain(lr_f, ref_f, True)
    conf_n, idx_n, fl_n = _match_chain(lr_f, ref_f, False)
    count = int(fl_n[0])
    print('flagged %d of %d columns (%dx%d periodic feature map)' % (count, h * w, h, w))
    assert count >= 1 and count == int(fl_o[0])
    assert torch.equal(conf_o, conf_n) and torch.equal(idx_o, idx_n)
    assert torch.equal(fl_o[1:1 + count].sort()[0], fl_n[1:1 + count].sort()[0])


@pytest.mark.parametrize('h,w', [(16, 24), (34, 70)])
def test_flagged_lo_rows_feature_match(dev, small_cfg, weights, h, w):
    """Engine.feature_match on frames of period 4 (the pooled reference frame has period 2: interior reference patches of one
    phase are identical, every LR column ties) and on random frames (few or no flagged columns): new launch list vs the old one."""
    from refvsr_amd.engine import Engine, FrameCtx
    new, old = Engine(small_cfg, weights), Engine(small_cfg, weights)
    old.legacy_prep = True
    g = torch.Generator().manual_seed(3)
    for kind, lr, ref in (('periodic', _periodic(3, h, w, 11), _periodic(3, h, w, 12)),
                          ('random', torch.rand(3, h, w, generator=g), torch.rand(3, h, w, generator=g))):
        conf_o, idx_o, grid_o = old.feature_match(FrameCtx(lr.to(dev), ref.to(dev)))
        conf_n, idx_n, grid_n = new.feature_match(FrameCtx(lr.to(dev), ref.to(dev)))
        count = int(new.last_flagged[0])
        print('flagged %d of %d columns (%dx%d %s frames)' % (count, h * w, h, w, kind))
        assert count == int(old.last_flagged[0])
        if kind == 'periodic':
            assert count >= 1
        assert grid_o == grid_n and torch.equal(conf_o, conf_n) and torch.equal(idx_o, idx_n)


@pytest.mark.parametrize('h,w', [(32, 32), (64, 96), (96, 160)])
def test_avgpool_pyramid_equals_five_pools(dev, h, w):
    from refvsr_amd import ops
    x = torch.randn(3, h, w, generator=torch.Generator().manual_seed(h + w)).to(dev)
    want = [x]
    for _ in range(5):
        want.append(ops.avgpool2(want[-1]))
    got = ops.avgpool_pyramid(x)
    assert len(got) == 5
    for k in range(5):
        assert got[k].shape == want[k + 1].shape and got[k].is_contiguous()
        assert torch.equal(got[k], want[k + 1]), 'level %d' % (k + 1)
    # the fenced second run (tests/footprint.py): NaN around the frame, 0xA5 around the one allocation that holds the five levels
    import footprint as fp
    fp.reset_inputs()
    xf = fp.fenced_input(x.cpu(), dev, 'nan')
    with fp.fenced_outputs(ops) as fo:
        got2 = ops.avgpool_pyramid(xf)
        bad = fp.judge(fo, got2, got)
    fp.reset_inputs()
    assert not bad, 'fenced run: ' + bad


@pytest.mark.parametrize('h,w,hr,wr', [(2, 2, 2, 2), (6, 10, 6, 10), (34, 70, 34, 70), (6, 10, 7, 11)])
def test_frame_prep_equals_seven_launches(dev, weights, h, w, hr, wr):
    """(7, 11): a reference frame with odd sides -- its last row and column reach ref8 but no 2x2 average."""
    from refvsr_amd import ops
    g = torch.Generator().manual_seed(17 * h + w + hr)
    lr, ref = torch.rand(3, h, w, generator=g).to(dev), torch.rand(3, hr, wr, generator=g).to(dev)
    ms = weights.raw['feature_match.sub_mean']
    lr8, ref8, lr_n, ref_n = ops.frame_prep(lr, ref, *ms)
    assert torch.equal(lr8, ops.pack_nhwc16(lr, 8))
    assert torch.equal(ref8, ops.pack_nhwc16(ref, 8))
    assert torch.equal(lr_n, ops.pack_nhwc32(ops.conv_direct(lr, *ms), 4))
    assert torch.equal(ref_n, ops.pack_nhwc32(ops.avgpool2(ops.conv_direct(ref, *ms)), 4))


def _run_stream(dev, monkeypatch, legacy):
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import window_indices
    if legacy:
        monkeypatch.setenv('REFVSR_LEGACY_PREP', '1')
    else:
        monkeypatch.delenv('REFVSR_LEGACY_PREP', raising=False)
    g = load_golden('e2e_S_16x24_t7')
    t = int(g['t'])
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    cfg.frame_num, cfg.cache_windows = t, True
    rb = int(g['reset_branch'])
    cfg.reset_branch = None if rb < 0 else rb
    net = SRNet(cfg).to(dev).eval()
    net.load_state_dict(make_state_dict(cfg, 1234))
    lr, rf = g['lr'], g['ref']
    outs = []
    for f in range(lr.shape[1]):
        wi = window_indices(f, lr.shape[1], t)
        outs.append(net(lr[:, wi].to(dev), rf[:, wi].to(dev), f == 0)['result'].clone())
    eng = net.Network.engine(0)
    assert eng.legacy_prep == legacy
    st = eng.export_state()
    return outs, {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}


def test_legacy_prep_knob_gives_equal_stream(dev, monkeypatch):
    """REFVSR_LEGACY_PREP=1 restores the old launch list; results and the carried state of a stream are the same bits."""
    new, st_new = _run_stream(dev, monkeypatch, False)
    old, st_old = _run_stream(dev, monkeypatch, True)
    assert len(new) == len(old) > 0
    for a, b in zip(new, old):
        assert torch.equal(a, b)
    assert sorted(st_new) == sorted(st_old) and len(st_new) > 0
    for k in st_new:
        assert torch.equal(st_new[k], st_old[k]), k
