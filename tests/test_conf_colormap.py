"""Confidence-map images, the part that runs without a GPU: the colour table of refvsr_colormap_table (its digest, pinned entries and,
where matplotlib is installed, its rebuild from get_cmap('inferno')); metrics.conf_colormap_model -- the numpy restatement of
refvsr_conf_colormap's steps -- against a literal restatement of evaluation/eval_quan_conf_map.py:79-84,126,150 written out below
(torch min / max normalisation, colormap(x)[:, :, :3], torch.Tensor, * 255, the rounding cast of cv2.imwrite); the argument validation
of refvsr_conf_colormap with host memory standing in for device pointers; the CLI switch and the refusal of RefVSR_IR.

Every comparison is bit-exact (np.array_equal): the model and the reference's chain are the same float32 operations."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHA256 = 'e24e8bd38b972989f64c42856b2b274df5ada3a62bc01bf8e83500a2ea938ad4'
PINNED = {0: (0, 0, 4), 1: (1, 0, 5), 127: (186, 54, 85), 128: (188, 55, 84), 255: (252, 255, 164)}


@pytest.fixture(scope='module')
def L():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the inputs (shared with the GPU file)
def boundary_map(scale=1.0, shift=0.0):
    """k / 256 (k = 0 .. 256) and both float32 neighbours of each, clipped to [0, 1], under x -> scale x + shift in float32: after the
    normalisation the samples sit on and one ulp around the colour table's bin edges.  [1, 771] float32."""
    k = np.arange(257, dtype=np.float32) / np.float32(256)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))]).astype(np.float32)
    v = np.clip(v, np.float32(0), np.float32(1))
    return (np.float32(scale) * v + np.float32(shift)).astype(np.float32)[None, :]


def random_map(h, w, seed, scale=1.0, shift=0.0):
    g = np.random.RandomState(seed)
    return (np.float32(scale) * g.rand(h, w).astype(np.float32) + np.float32(shift)).astype(np.float32)


def input_families():
    """name -> float32 [h, w] map: the families both test files walk."""
    fam = {}
    for h, w in ((1, 1), (3, 5), (33, 65), (270, 480)):
        fam['random %dx%d' % (h, w)] = random_map(h, w, 7 * h + w, 0.83, 0.11)
    fam['boundaries'] = boundary_map()
    fam['boundaries 0.37 x + 0.21'] = boundary_map(0.37, 0.21)
    fam['boundaries 3 x - 1.5'] = boundary_map(3.0, -1.5)
    fam['negative'] = random_map(7, 9, 3, 2.0, -3.0)
    fam['span 1e-3'] = random_map(7, 9, 5, 1e-3, 0.5)
    fam['constant'] = np.full((5, 6), 0.625, dtype=np.float32)
    return fam


# ------------------------------------------------------------------------------------------------ the yardstick
def reference_image(x):
    """eval_quan_conf_map.py:79-84,126,150 for one map x [h, w] (float32), statement by statement; cv2.imwrite's float -> uint8
    conversion is saturate_cast<uchar>(rint(v)).  uint8 [h, w, 3], RGB (the reference's cvtColor only reorders for the BGR writer)."""
    import matplotlib.pyplot as plt
    colormap = plt.get_cmap('inferno')
    conf_map_norm = torch.from_numpy(np.ascontiguousarray(x))[None, None]            # vis['conf_map']: [1, 1, h, w]
    conf_map_norm = conf_map_norm - conf_map_norm.min()
    conf_map_norm = conf_map_norm / conf_map_norm.max()
    conf_map_norm_cpu = conf_map_norm.cpu().numpy()[0].transpose(1, 2, 0)[:, :, 0]
    conf_map_norm_cpu = colormap(conf_map_norm_cpu)[:, :, :3]
    conf_map_norm = torch.Tensor(conf_map_norm_cpu)[None, :].permute(0, 3, 1, 2)
    conf_map_norm_cpu = conf_map_norm.cpu().numpy()[0].transpose(1, 2, 0)
    img = conf_map_norm_cpu * 255
    assert img.dtype == np.float32
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the table
def _table(L):
    buf = (ctypes.c_ubyte * 768)()
    assert L.refvsr_colormap_table(buf) == 0
    return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(256, 3)


def test_table_digest_and_pinned_entries(L):
    from refvsr_amd import ops
    t = _table(L)
    assert hashlib.sha256(t.tobytes()).hexdigest() == SHA256
    for i, rgb in PINNED.items():
        assert tuple(int(v) for v in t[i]) == rgb, i
    assert np.array_equal(np.array(ops.colormap_table(), dtype=np.uint8), t)
    assert L.refvsr_colormap_table(None) != 0 and 'null output' in L.refvsr_last_error().decode()


def test_table_is_matplotlibs_inferno(L):
    pytest.importorskip('matplotlib')
    import matplotlib.pyplot as plt
    lut64 = np.asarray(plt.get_cmap('inferno')(np.arange(256)), dtype=np.float64)[:, :3]
    prod = lut64.astype(np.float32) * np.float32(255)
    assert prod.dtype == np.float32
    assert np.array_equal(np.rint(prod).astype(np.uint8), _table(L))
    # the committed header is what the generator writes from the same table
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_colormap_table', os.path.join(ROOT, 'tools', 'gen_colormap_table.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert np.array_equal(gen.header_bytes(), _table(L))


def test_exports_and_constants(L):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    m = re.search(r'#define REFVSR_COLORMAP_MAX_MAPS (\d+)', src)
    assert m and int(m.group(1)) == hip.COLORMAP_MAX_MAPS == 16
    names = {'refvsr_conf_colormap', 'refvsr_conf_colormap_workspace_bytes', 'refvsr_colormap_table'}
    assert names <= set(hip.EXPORTS)
    for name in names:
        assert hasattr(L, name) and re.search(r'\b%s\s*\(' % name, src)
    assert hip.ABI_VERSION == L.refvsr_abi_version() == 15
    assert 'eval_quan_conf_map.py:64-100' in src and '148-165' in src
    mk = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'Makefile')).read()
    assert 'colormap.hip' in mk and 'fast-math' not in mk


def test_workspace_bytes(L):
    wb = L.refvsr_conf_colormap_workspace_bytes
    assert wb(1, 1, 1) == 8 and wb(16, 1, 1) == 16 * 8 and wb(4, 32, 48) == 4 * 8
    assert wb(1, 270, 480) == 32 * 8                        # 32 400 float4s: 32 blocks of 1024
    assert wb(16, 1080, 1920) == 16 * 64 * 8                # capped at 64 partial pairs per map
    for bad in ((0, 4, 4), (17, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 32768), (1, -1, 4)):
        assert wb(*bad) == 0


# ------------------------------------------------------------------------------------------------ 2. the model against the reference
def test_model_equals_the_reference_chain():
    pytest.importorskip('matplotlib')
    from refvsr_amd import metrics
    for name, x in input_families().items():
        got = metrics.conf_colormap_model(x)
        assert got.dtype == np.uint8 and got.shape == x.shape + (3,)
        with np.errstate(invalid='ignore'):
            want = reference_image(x)
        assert np.array_equal(got, want), name
        if x.min() == x.max():                               # ('constant', and the single sample of 1 x 1)
            assert not got.any(), name
        else:
            assert got.any(), name


def test_model_pins_without_matplotlib(L):
    """What holds with the library's table alone: the ends of the range, the bin edges and the constant map."""
    from refvsr_amd import metrics
    t = _table(L)
    x = boundary_map()                                       # already normalised: min 0, max 1
    got = metrics.conf_colormap_model(x)[0]
    k = np.arange(257)
    assert np.array_equal(got[:257], t[np.minimum(k, 255)])                  # k / 256 opens bin k; 1.0 belongs to the last bin
    assert np.array_equal(got[257 + 1:257 + 257], t[k[1:] - 1])              # one ulp below an edge: the bin before
    assert np.array_equal(got[514:514 + 256], t[k[:256]])                    # one ulp above: the same bin
    assert not metrics.conf_colormap_model(np.full((3, 4), -2.5, dtype=np.float32)).any()
    assert metrics.conf_colormap_model(torch.rand(1, 1, 6, 7)).shape == (6, 7, 3)
    one = metrics.conf_colormap_model(np.array([[1.0, 3.0]], dtype=np.float32))
    assert np.array_equal(one[0], t[[0, 255]])


# ------------------------------------------------------------------------------------------------ 3. argument validation
def test_conf_colormap_rejects_bad_arguments_without_a_gpu(L):
    """Validation runs before any device work (host memory stands in for device pointers: never dereferenced)."""
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 65536)()
    base = (ctypes.addressof(buf) + 15) & ~15
    arr = lambda *vals: (P * len(vals))(*vals)
    maps, rgb, ws = arr(base, base + 1024), arr(base + 4096, base + 8192), P(base + 16384)
    need = L.refvsr_conf_colormap_workspace_bytes(2, 8, 8)
    assert need == 2 * 8
    err = lambda: L.refvsr_last_error().decode()
    call = lambda m=maps, n=2, h=8, w=8, o=rgb, wsp=ws, nb=need: L.refvsr_conf_colormap(m, n, h, w, o, wsp, nb, None)
    assert call(m=None) != 0 and 'null map / image table' in err()
    assert call(o=None) != 0 and 'null map / image table' in err()
    for n in (0, 17, -1):
        assert call(n=n) != 0 and '1..16 maps per launch' in err()
    for h, w in ((0, 8), (8, 0), (-3, 8)):
        assert call(h=h, w=w) != 0 and 'at least 1' in err()
    for h, w in ((65536, 32768), (46341, 46341)):
        assert call(h=h, w=w) != 0 and 'below 2^31' in err()
    assert call(wsp=None) != 0 and 'null workspace' in err()
    assert call(nb=need - 1) != 0 and 'workspace too small (15 bytes, 16 needed)' in err()
    assert call(nb=0) != 0 and 'workspace too small' in err()
    assert call(m=arr(base, 0)) != 0 and 'null pointer (map 1)' in err()
    assert call(o=arr(0, base + 8192)) != 0 and 'null pointer (map 0)' in err()
    assert call(m=arr(base, base + 1026)) != 0 and '4-byte aligned (map 1)' in err()
    assert call(m=arr(base + 1, base + 1024)) != 0 and '4-byte aligned (map 0)' in err()
    from refvsr_amd import hip
    with pytest.raises(RuntimeError, match='1..16 maps per launch'):
        hip.check(call(n=17), 'conf_colormap')


# ------------------------------------------------------------------------------------------------ 4. the CLI switch, the IR refusal
def _base(tmp_path):
    return ['--mode', 'unit', '--data_offset', str(tmp_path), '--output_offset', str(tmp_path / 'o')]


def test_cli_selects_the_mode(tmp_path):
    from refvsr_amd import evalrun
    cfg = evalrun.build_config(_base(tmp_path) + ['--config', 'config_RefVSR_small_L1', '--eval_mode', 'quan_conf_map'])
    assert cfg.EVAL.eval_mode == 'quan_conf_map' and cfg.save_sample is True
    plain = evalrun.build_config(_base(tmp_path))
    assert plain.EVAL.eval_mode == 'qual_quan' and plain.save_sample is False
    assert [d for d, _ in evalrun.CONF_MAP_DIRS] == ['conf_map_norm', 'conf_map_prop_norm', 'conf_map_prop_b_norm', 'conf_map_prop_f_norm']
    assert [k for _, k in evalrun.CONF_MAP_DIRS] == ['conf_map', 'conf_map_prop', 'conf_map_prop_backward', 'conf_map_prop_forward']


def test_ir_network_is_refused_before_data_or_device(tmp_path, monkeypatch):
    from refvsr_amd import evalrun

    def boom(*a, **k):
        raise AssertionError('evaluate() went past the refusal')
    monkeypatch.setattr(evalrun, 'ClipSet', boom)
    monkeypatch.setattr(evalrun, 'load_checkpoint', boom)
    monkeypatch.setattr(torch.cuda, 'synchronize', boom)
    cfg = evalrun.build_config(_base(tmp_path) + ['--config', 'config_RefVSR_IR_MFID', '--eval_mode', 'quan_conf_map'])
    with pytest.raises(RuntimeError, match='RefVSR_IR returns no confidence maps'):
        evalrun.evaluate(cfg)
    assert not (tmp_path / 'o').exists()                      # nothing was created on the way
