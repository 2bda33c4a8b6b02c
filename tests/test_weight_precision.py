"""config.weight_precision (CPU): the config surface, the round16 set against the packers' calls, the fp16-format packers against a
numpy lane model built on the library's own K-block tables, and the ABI 15 surface.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ config
def test_default_is_hi_lo_on_every_config():
    from refvsr_amd.config import CONFIG_NAMES, get_config, resolve_weight_precision
    for name in CONFIG_NAMES:
        cfg = get_config('p', 'm', name)
        assert cfg.weight_precision == 'hi_lo'
        assert resolve_weight_precision(cfg) == 'hi_lo'


def test_amp_resolves_by_is_amp_and_bad_values_raise():
    from refvsr_amd.config import CONFIG_NAMES, get_config, resolve_weight_precision
    for name in CONFIG_NAMES:
        cfg = get_config('p', 'm', name)
        cfg.weight_precision = 'amp'
        want = 'fp16' if cfg.is_amp else 'hi_lo'
        assert resolve_weight_precision(cfg) == want, name
        small = cfg.mid_channels == 24 and cfg.network == 'RefVSR'
        assert cfg.is_amp == small, name                 # the reference's AMP configs are exactly the mid_channels = 24 RefVSR ones
        cfg.weight_precision = 'fp16'
        if small:
            assert resolve_weight_precision(cfg) == 'fp16'
        else:
            with pytest.raises(ValueError, match='fp16'):
                resolve_weight_precision(cfg)
        for bad in ('bf16', 'FP16', 'hi-lo', 16):
            cfg.weight_precision = bad
            with pytest.raises(ValueError, match='weight_precision'):
                resolve_weight_precision(cfg)
    cfg = get_config('p', 'm', 'config_RefVSR_IR_L1')       # an IR config with 24 channels is still not supported
    cfg.mid_channels, cfg.weight_precision = 24, 'fp16'
    with pytest.raises(ValueError):
        resolve_weight_precision(cfg)


def test_fp16_on_unsupported_family_raises_at_packing():
    from refvsr_amd import get_config, make_state_dict
    from refvsr_amd.engine import Weights
    cfg = get_config('p', 'm', 'config_RefVSR_MFID')
    cfg.weight_precision = 'fp16'
    with pytest.raises(ValueError, match='mid_channels = 24'):
        Weights(cfg, make_state_dict(cfg, 1), 'cpu')


# ---------------------------------------------------------------------------------------------------------- the round16 set
def _packed_fp16_names(cfg, monkeypatch):
    """Names of the conv weights engine.Weights hands to pack_conv with fp16 operands (hi + lo, or hi only), read from the calls."""
    from refvsr_amd import engine, make_state_dict
    sd = make_state_dict(cfg, 7)
    by_id = {id(v): k for k, v in sd.items() if k.endswith('.weight')}
    seen, fp32 = set(), set()
    real = engine.pack_conv

    def spy(w, b, srcs, *a, **k):
        name = by_id.get(id(w))
        if name is not None:
            (fp32 if k.get('f32') else seen).add(name)
        return real(w, b, srcs, *a, **k)
    monkeypatch.setattr(engine, 'pack_conv', spy)
    W = engine.Weights(cfg, sd, 'cpu')
    raw = {'Network.%s.weight' % n for n in W.raw if not n.endswith('map64.0') and not n.endswith('map128.0')}
    return sd, seen, fp32, raw


@pytest.mark.parametrize('name,scale', [('config_RefVSR_small_L1', 4), ('config_RefVSR_small_MFID_8K', 4), ('config_RefVSR_small_L1', 2)])
def test_round16_set_is_the_set_packed_with_fp16_operands(name, scale, monkeypatch):
    """round16 rounds exactly the conv weights that engine.Weights packs with fp16 MFMA operands today; the exclusions (matching
    features, the 2 -> 16 confidence convs) are the fp32-packed and raw ones."""
    from refvsr_amd import get_config, set_scale
    from refvsr_amd.weights import round16, round16_excluded
    cfg = get_config('p', 'm', name)
    if scale != 4:
        set_scale(cfg, scale)
    sd, fp16_names, fp32_names, raw_names = _packed_fp16_names(cfg, monkeypatch)
    r = round16(sd)
    rounded = {k for k in sd if not torch.equal(r[k], sd[k])}
    conv_w = {k for k, v in sd.items() if k.endswith('.weight') and v.dim() == 4}
    assert rounded == {k for k in conv_w if not round16_excluded(k)}
    assert rounded == fp16_names, (sorted(rounded ^ fp16_names)[:8])
    assert {k for k in conv_w if round16_excluded(k)} == fp32_names | raw_names
    assert all(r[k].dtype == torch.float32 for k in r)
    assert all(torch.equal(r[k], sd[k]) for k in sd if k.endswith('.bias'))
    assert all(torch.equal(r[k], sd[k].half().float()) for k in rounded)


def test_weights_fp16_mode_packs_round16_and_f16w_blobs():
    """Weights in fp16 mode == Weights on round16(sd) for every generic pack; every specialised blob of the C = 24 engine is in the
    fp16 format."""
    from refvsr_amd import get_config, make_state_dict
    from refvsr_amd.engine import Weights
    from refvsr_amd.weights import round16
    cfg = get_config('p', 'm', 'config_RefVSR_small_L1')
    sd = make_state_dict(cfg, 3)
    cfg.weight_precision = 'fp16'
    Wf = Weights(cfg, sd, 'cpu')
    cfg.weight_precision = 'hi_lo'
    Wh = Weights(cfg, round16(sd), 'cpu')
    assert Wf.wfmt == 'fp16' and Wh.wfmt == 'hi_lo' and Wf.conv.keys() == Wh.conv.keys()
    n_f16w = 0
    for k in Wf.conv:
        a, b = Wf.conv[k], Wh.conv[k]
        assert torch.equal(a.wpack, b.wpack) and torch.equal(a.bias, b.bias), k
        if a.blob24 is not None:
            assert a.blob_wfmt == 'fp16' and b.blob_wfmt == 'hi_lo', k
            n_f16w += 1
    assert n_f16w > 100
    for k in Wf.raw:
        assert all(torch.equal(x, y) for x, y in zip(Wf.raw[k], Wh.raw[k])), k


# ------------------------------------------------------------------------------------------------------------ the packers
@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    return hip.lib()


def _kb(v):
    return None if v == -1 else (v >> 16, (v >> 8) & 0xff, v & 0xff)


def _unpack_rows(frag16, kblock, nsteps, ncg):
    """fp16 fragments [S][16 rows][4 quarters][8] of one fragment slot -> W [16][9 taps * ncg * 8] (numpy lane model)."""
    W = np.zeros((16, 9 * ncg * 8), np.float16)
    zero_ok = True
    for s in range(nsteps):
        for q in range(4):
            kb = kblock(s, q)
            if kb is None:
                zero_ok &= not frag16[s, :, q].any()
                continue
            ty, tx, cg = kb
            g = (ty * 3 + tx) * ncg + cg
            W[:, g * 8:g * 8 + 8] = frag16[s, :, q]
    return W, zero_ok


def _kmat(w):
    """[cout, cin, 3, 3] -> fp16 [cout, 9 taps * ncg * 8] in the (tap, channel group) order of packing.kmatrix (cin padded to 8)."""
    from refvsr_amd.packing import kmatrix
    Wk, _, ncg = kmatrix(w.numpy(), [w.shape[1]])
    return Wk.astype(np.float16), ncg


def test_pack_resblock24_f16w_against_lane_model(L):
    from refvsr_amd import hip
    from refvsr_amd.packing import pack_resblock24_f16w
    g = torch.Generator().manual_seed(0)
    w1, w2 = torch.randn(24, 24, 3, 3, generator=g), torch.randn(24, 24, 3, 3, generator=g)
    b1, b2 = torch.randn(24, generator=g), torch.randn(24, generator=g)
    blob = pack_resblock24_f16w(w1, b1, w2, b2).numpy()
    assert blob.size == hip.RESBLOCK24_F16W_BLOB_BYTES == L.refvsr_resblock24_f16w_blob_bytes() == 28928
    kblock = lambda s, q: _kb(L.refvsr_resblock24_kblock(s, q))
    wb = 7 * 2 * 1024
    for i, w in enumerate((w1, w2)):
        frag = blob[i * wb:(i + 1) * wb].view(np.float16).reshape(7, 2, 4, 16, 8).transpose(0, 1, 3, 2, 4)   # [s][f][r][q][8]
        want, _ = _kmat(w)
        for f in range(2):
            got, zero_ok = _unpack_rows(frag[:, f], kblock, 7, 3)
            assert zero_ok
            rows = want[16 * f:16 * f + 16]
            assert np.array_equal(got[:rows.shape[0]].view(np.uint16), rows.view(np.uint16)), (i, f)
            assert not got[rows.shape[0]:].any(), 'padding rows must be zero'
    bias = blob[2 * wb:].view(np.float32)
    assert np.array_equal(bias[:24], b1.numpy()) and not bias[24:32].any()
    assert np.array_equal(bias[32:56], b2.numpy()) and not bias[56:].any()


@pytest.mark.parametrize('cout,srcs,c0,c1,size_fn', [
    (24, [24], 24, 0, 'refvsr_conv24_f16w_blob_bytes'), (24, [16], 16, 0, 'refvsr_conv24_f16w_blob_bytes'),
    (24, [3, 24], 8, 24, 'refvsr_conv24_f16w_blob_bytes'), (24, [24, 24], 24, 24, 'refvsr_conv24_f16w_blob_bytes'),
    (32, [32], 32, 0, 'refvsr_conv32_f16w_blob_bytes'), (32, [3], 8, 0, 'refvsr_conv32_f16w_blob_bytes')])
def test_pack_conv24_f16w_against_lane_model(L, cout, srcs, c0, c1, size_fn):
    from refvsr_amd.packing import c24_steps, kmatrix, pack_conv24
    g = torch.Generator().manual_seed(cout + c0 + c1)
    w, b = torch.randn(cout, sum(srcs), 3, 3, generator=g), torch.randn(cout, generator=g)
    blob = pack_conv24(w, b, srcs, wfmt='fp16').numpy()
    assert blob.size == getattr(L, size_fn)(c0, c1)
    Wk, _, ncg = kmatrix(w.numpy(), srcs)
    S, nf = c24_steps(ncg), 2
    kblock = lambda s, q: _kb(L.refvsr_conv24_kblock(ncg, s, q))
    frag = blob[:S * nf * 1024].view(np.float16).reshape(S, nf, 4, 16, 8).transpose(0, 1, 3, 2, 4)
    want = Wk.astype(np.float16)
    for f in range(nf):
        got, zero_ok = _unpack_rows(frag[:, f], kblock, S, ncg)
        assert zero_ok
        rows = want[16 * f:16 * f + 16]
        assert np.array_equal(got[:rows.shape[0]].view(np.uint16), rows.view(np.uint16)), f
        assert not got[rows.shape[0]:].any()
    bias = blob[S * nf * 1024:].view(np.float32)
    assert np.array_equal(bias[:cout], b.numpy()) and not bias[cout:].any()


def test_pack_conv_shuffle2_f16w_layout(L):
    """The pixel-shuffle blobs: two 48-row groups in the 3-fragment fp16 format, each equal to pack_conv24(rows of group z)."""
    from refvsr_amd.packing import pack_conv24, pack_conv_shuffle2
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(96, 24, 3, 3, generator=g), torch.randn(96, generator=g)
    blob = pack_conv_shuffle2(w, b, wfmt='fp16')
    assert blob.numel() == L.refvsr_conv_shuffle2_f16w_blob_bytes(24) == 2 * (7 * 3 * 1024 + 256)
    assert L.refvsr_conv_shuffle2_f16w_blob_bytes(48) == -1
    half = blob.numel() // 2
    for z in range(2):
        R = np.arange(48)
        rows = 4 * (R % 24) + 2 * z + R // 24
        assert torch.equal(blob[z * half:(z + 1) * half], pack_conv24(w[rows], b[rows], [24], shuffle_group=True, wfmt='fp16'))


def test_f16w_blob_equals_hi_lo_blob_on_round16_weights_hi_rows():
    """On fp16-representable weights the hi + lo blob's lo fragments are all zero and its hi rows are the fp16 blob's rows."""
    from refvsr_amd.packing import pack_resblock24, pack_resblock24_f16w
    g = torch.Generator().manual_seed(2)
    w = torch.randn(24, 24, 3, 3, generator=g).half().float()
    b = torch.randn(24, generator=g)
    hl = pack_resblock24(w, b, w, b).numpy()[:2 * 21504].view(np.float16).reshape(2, 7, 3, 4, 16, 8)
    f16 = pack_resblock24_f16w(w, b, w, b).numpy()[:2 * 14336].view(np.float16).reshape(2, 7, 2, 4, 16, 8)
    assert not hl[:, :, 1].any() and not hl[:, :, 2, :, 8:].any()
    assert np.array_equal(hl[:, :, 0].view(np.uint16), f16[:, :, 0].view(np.uint16))
    assert np.array_equal(hl[:, :, 2, :, :8].view(np.uint16), f16[:, :, 1, :, :8].view(np.uint16))


# ------------------------------------------------------------------------------------------------------------------ ABI 15
def test_abi15_header_exports_and_binding_agree():
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    assert re.search(r'#define REFVSR_ABI_VERSION 15\b', src)
    assert re.search(r'#define REFVSR_RESBLOCK24_F16W_BLOB_BYTES 28928\b', src)
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', body))
    assert declared == set(hip.EXPORTS)
    twins = {n for n in declared if n.endswith('_f16w')}
    assert twins == {'refvsr_resblock24_chain_f16w', 'refvsr_resblock24_chain_batch_f16w', 'refvsr_conv24_f16w', 'refvsr_conv24_batch_f16w',
                     'refvsr_conv32_f16w', 'refvsr_conv_shuffle2_f16w', 'refvsr_conv_shuffle2_batch_f16w', 'refvsr_conf_alpha_f16w',
                     'refvsr_conf_alpha_batch_f16w'}
    for t in twins:                                  # same signature as the function each twin is named after
        assert hip.SIGNATURES[t] == hip.SIGNATURES[t[:-len('_f16w')]], t
    h = ctypes.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(h, name), name
    assert hip.ABI_VERSION == 15 and hip.lib().refvsr_abi_version() == 15


def test_f16w_entry_points_reject_bad_arguments_without_a_gpu(L):
    from refvsr_amd import hip
    assert L.refvsr_resblock24_chain_f16w(None, 8, 32, 1, None, 28928, 0.0, None, None, None, None) != 0
    assert L.refvsr_conv24_f16w_blob_bytes(48, 0) == -1 and L.refvsr_conv32_f16w_blob_bytes(24, 0) == -1
    assert L.refvsr_conv24_f16w_blob_bytes(24, 0) == 7 * 2 * 1024 + 128
    rc = L.refvsr_conf_alpha_f16w(None, None, 8, 8, 1, None, None, 0.2, None, 24, 0.2, None, None, None)
    assert rc != 0 and b'null' in L.refvsr_last_error()
    with pytest.raises(RuntimeError):
        hip.check(rc, 'conf_alpha_f16w')


def test_evalrun_weight_precision_flag():
    from refvsr_amd.config import resolve_weight_precision
    from refvsr_amd.evalrun import build_config
    assert build_config(['-c', 'config_RefVSR_small_L1']).weight_precision == 'hi_lo'
    cfg = build_config(['-c', 'config_RefVSR_small_MFID', '--weight_precision', 'amp'])
    assert cfg.weight_precision == 'amp' and resolve_weight_precision(cfg) == 'fp16'
    cfg = build_config(['-c', 'config_RefVSR_MFID', '--weight_precision', 'amp'])
    assert resolve_weight_precision(cfg) == 'hi_lo'
    with pytest.raises(SystemExit):
        build_config(['--weight_precision', 'bf16'])
