"""The C-ABI shared library: builds for gfx950 (hipcc cross-compiles without a GPU), loads, and
exports every symbol that include/refvsr_hip.h declares and refvsr_amd/hip.py binds.  No compute
calls here (no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def libpath():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.LIB_PATH


def _declared():
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', src)))


def test_header_binding_and_library_agree(libpath):
    from refvsr_amd import hip
    declared = _declared()
    assert declared == sorted(hip.EXPORTS), set(declared) ^ set(hip.EXPORTS)
    h = ctypes.CDLL(libpath)
    for name in declared:
        assert hasattr(h, name), 'library does not export ' + name


def test_abi_version_and_error_channel(libpath):
    from refvsr_amd import hip
    h = hip.lib()
    assert h.refvsr_abi_version() == hip.ABI_VERSION
    # argument validation runs before any device work: a null descriptor is rejected with a message
    rc = h.refvsr_conv_mfma(None, None)
    assert rc != 0 and b'null descriptor' in h.refvsr_last_error()
    with pytest.raises(RuntimeError, match='null descriptor'):
        hip.check(rc, 'conv_mfma')


def test_conv_descriptor_layout_matches_header():
    """Field order / types of the ctypes mirror follow `struct RefvsrConv` in the header."""
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    body = src[src.index('typedef struct RefvsrConv {'):src.index('} RefvsrConv;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S).split('{', 1)[1]
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(','):
            names.append(part.replace('*', ' ').split()[-1])
    assert names == [f[0] for f in hip.RefvsrConv._fields_]


def test_packing_contract_matches_the_library(libpath):
    """The K-block order is computed twice -- packing.py on the host side of the boundary, rv_kslot inside the kernels.
    The library exports its closed form as host functions so that the two are pinned against each other without a GPU."""
    from refvsr_amd import hip
    from refvsr_amd.packing import kslot, ksteps
    h = hip.lib()
    for ks in (1, 3, 5, 7):
        for ncg in range(1, 18):
            assert h.refvsr_ksteps(ks, ncg) == ksteps(ks, ncg)
            slots = set()
            for ty in range(ks):
                for tx in range(ks):
                    for cg in range(ncg):
                        j = h.refvsr_kslot(ty, tx, cg, ks, ncg)
                        assert j == kslot(ty, tx, cg, ks, ncg)
                        slots.add(j)
            assert len(slots) == ks * ks * ncg and max(slots) < 4 * ksteps(ks, ncg)


def test_argument_validation_precedes_device_work(libpath):
    """Error behaviour of the boundary: every entry point validates its arguments before touching the device and
    reports through refvsr_last_error() -- so the checks run (and are pinned) in the GPU-less container too."""
    from refvsr_amd import hip
    h = hip.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 4096)()                    # host memory standing in for device pointers: never dereferenced
    p = ctypes.cast(buf, P)

    def expect(rc, text):
        assert rc != 0 and text in h.refvsr_last_error().decode(), h.refvsr_last_error()

    d = hip.RefvsrConv()
    d.src0, d.c0, d.h_in, d.w_in, d.h_out, d.w_out = p, 12, 8, 8, 8, 8       # 12 channels: not a 16-byte multiple
    expect(h.refvsr_conv_mfma(ctypes.byref(d), None), 'src0/c0 invalid (c0=12)')
    d.c0, d.ksize, d.stride, d.pad = 24, 9, 1, 4
    expect(h.refvsr_conv_mfma(ctypes.byref(d), None), 'bad geometry')
    d.ksize, d.pad, d.wpack, d.bias, d.out, d.mt_per_block, d.cout, d.out_c = 3, 1, p, p, p, 4, 24, 24
    expect(h.refvsr_conv_mfma(ctypes.byref(d), None), 'mt_per_block must be 1..3')
    d.mt_per_block, d.cout = 2, 22
    expect(h.refvsr_conv_mfma(ctypes.byref(d), None), 'nhwc16 output needs cout % 4 == 0')
    d.cout, d.out_mode, d.res = 24, 1, p                                      # pixel shuffle with a residual
    expect(h.refvsr_conv_mfma(ctypes.byref(d), None), 'pixel-shuffle output constraints')

    assert h.refvsr_resblock_lean_fits(24) == 1 and h.refvsr_resblock_lean_fits(16) == 1
    assert h.refvsr_resblock_lean_fits(48) == 0 and h.refvsr_resblock_lean_fits(20) == 0
    expect(h.refvsr_resblock_lean(p, 24, 8, 8, p, p, p, p, 7, 0.0, 1.0, p, None), 'in-place')
    q = ctypes.cast(ctypes.addressof(buf) + 2048, P)
    expect(h.refvsr_resblock_lean(p, 48, 8, 8, p, p, p, p, 14, 0.0, 1.0, q, None), '48')

    expect(h.refvsr_pack_nhwc16(p, 3, 8, 8, q, 12, None), 'pack_nhwc16: bad args')
    expect(h.refvsr_resize(p, 3, 8, 8, q, 16, 16, 7, 0.0, 1.0, None, None, None, 0, 0, 0, None), 'resize: bad mode 7')
    expect(h.refvsr_warp_nhwc16(p, 1, 8, 24, q, 8, 8, q, None), 'warp_nhwc16: bad args')
    expect(h.refvsr_match_top2(p, 1, q, 512, 1, q, q, None), 'match_top2')
    expect(h.refvsr_aligned_sample(p, 1, 1, 1, 24, q, q, None), 'map too small for reflection padding')
    expect(h.refvsr_block_gather_nhwc16(p, 8, 8, 20, q, 4, 4, 2, q, None), 'block_gather')
    flags = (ctypes.c_void_p * 1)(p)
    expect(h.refvsr_buffers_equal(flags, flags, 1, 24, q, None), 'multiple of 16 bytes')


def test_conv_variant_query_is_the_launchers_plan(libpath):
    """refvsr_conv_variant (added symbol, ABI 15 unchanged): host only -- it answers here, where no device exists -- with the packed
    key of the planned conv_mfma_kernel instantiation, and rejects what refvsr_conv_mfma rejects, with the same message."""
    from refvsr_amd import hip
    h = hip.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    key = ctypes.c_int(-1)
    assert h.refvsr_conv_variant(None, ctypes.byref(key)) != 0 and b'null descriptor' in h.refvsr_last_error()
    d = hip.RefvsrConv()
    d.src0, d.c0, d.h_in, d.w_in, d.h_out, d.w_out = p, 24, 19, 45, 19, 45
    d.ksize, d.stride, d.pad, d.wpack, d.bias, d.out = 3, 1, 1, p, p, p
    d.cout, d.mt_per_block, d.ksteps, d.out_c, d.act_slope, d.post_slope = 24, 2, h.refvsr_ksteps(3, 3), 24, 1.0, 1.0
    assert h.refvsr_conv_variant(ctypes.byref(d), None) != 0 and b'null key' in h.refvsr_last_error()
    if not [k for k in os.environ if k.startswith('REFVSR_CONV_')]:
        assert h.refvsr_conv_variant(ctypes.byref(d), ctypes.byref(key)) == 0
        # MT | TILES << 2 | NW << 6 | EPI << 11 | F32 << 12 | GATHER << 13 | RESIDENT << 14 | HI1 << 15: resident, lean, 8 waves, 2 tiles
        assert key.value == (2 | 2 << 2 | 8 << 6 | 1 << 11 | 1 << 14), key.value
    d.ksteps += 1
    key.value = -1
    assert h.refvsr_conv_variant(ctypes.byref(d), ctypes.byref(key)) != 0 and b'ksteps mismatch' in h.refvsr_last_error() and key.value == -1
    assert h.refvsr_conv_mfma(ctypes.byref(d), None) != 0 and b'ksteps mismatch' in h.refvsr_last_error()


def test_fixed_variant_queries_are_the_launchers_plans(libpath):
    """refvsr_conv24_variant / refvsr_resblock24_variant (added symbols, ABI 15 unchanged): host only -- they answer here, where no
    device exists -- with the packed key, tile count and LDS bytes of the planned conv24_kernel / resblock24_kernel instantiation, and
    reject what the entry points reject, with the same message."""
    from refvsr_amd import hip
    h = hip.lib()
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    ops = [n for n, _ in sorted(re.findall(r'REFVSR_C24_([A-Z0-9_]+) = (\d)', src), key=lambda t: int(t[1]))]
    assert ops == ['CONV24', 'CONV32', 'CONV48', 'SHUFFLE2', 'CONF_ALPHA', 'CONV_LAST']
    assert [getattr(hip, 'C24_' + n) for n in ops] == list(range(6))
    key, n, lds = ctypes.c_longlong(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    c24 = lambda *a: h.refvsr_conv24_variant(*a, ctypes.byref(key), ctypes.byref(n), ctypes.byref(lds))
    k = lambda COUT, NCG0, NCG1, NWV, TH, WPS, SHUF=0, CONF=0, HALF=0, MM=0, WF=0: (
        COUT | NCG0 << 6 | NCG1 << 10 | NWV << 14 | TH << 19 | WPS << 24 | SHUF << 27 | CONF << 33 | HALF << 35 | MM << 36 | WF << 37)
    # (op, x0, x1, mm, wf, batch, h, w) -> (key, tiles, LDS bytes); none of these depends on REFVSR_CONV48_WAVES
    for args, want in (((hip.C24_CONV24, 24, 0, 0, 0, 1, 19, 45), (k(24, 3, 0, 8, 8, 4), 6, 37952)),
                       ((hip.C24_CONV24, 8, 24, 1, 1, 3, 19, 45), (k(24, 1, 3, 8, 8, 4, MM=1, WF=1), 18, 45760)),
                       ((hip.C24_CONV24, 24, 0, 0, 0, 7, 19, 45), (k(24, 3, 0, 8, 8, 4), 6, 37952)),      # a single-map entry has no batch
                       ((hip.C24_CONV32, 8, 0, 0, 1, 1, 8, 32), (k(32, 1, 0, 8, 8, 4, WF=1), 1, 11712)),
                       ((hip.C24_CONV48, 48, 48, 0, 0, 1, 19, 45), (k(24, 6, 6, 16, 8, 4, HALF=1), 6, 153792)),
                       ((hip.C24_SHUFFLE2, 48, 0, 0, 0, 1, 33, 70), (k(48, 6, 0, 16, 16, 4, SHUF=48), 9, 154816)),
                       ((hip.C24_CONF_ALPHA, 24, 2, 1, 0, 3, 19, 45), (k(24, 2, 0, 8, 8, 4, CONF=2, MM=1), 45, 36480)),      # 38 x 90: the doubled grid
                       ((hip.C24_CONV_LAST, 24, 0, 0, 0, 1, 75, 301), (k(3, 3, 0, 8, 8, 4), 100, 23616))):
        assert c24(*args) == 0, h.refvsr_last_error()
        assert (key.value, n.value, lds.value) == want, args
    assert h.refvsr_conv24_variant(hip.C24_CONV24, 24, 0, 0, 0, 1, 19, 45, ctypes.byref(key), None, None) == 0      # tile count and LDS bytes are optional
    if not os.environ.get('REFVSR_CONV48_WAVES'):
        assert c24(hip.C24_CONV48, 48, 0, 0, 0, 1, 33, 70) == 0 and key.value == k(48, 6, 0, 16, 16, 4)

    P = ctypes.c_void_p
    buf = (ctypes.c_char * 65536)()
    at = lambda off: ctypes.cast(ctypes.addressof(buf) + off, P)
    arr = lambda *ps: (P * len(ps))(*[p.value for p in ps])

    def expect(query, entry, text):
        """the query's message, then the entry point's: both `text`"""
        assert query() != 0
        got = h.refvsr_last_error().decode()
        assert got == text, got
        if entry is not None:
            assert entry() != 0 and h.refvsr_last_error().decode() == text, h.refvsr_last_error()

    s2, o2 = arr(at(0), at(4096)), arr(at(8192), at(12288))
    conv = lambda f, c0, c1: f(at(0), c0, None, c1, 8, 8, at(1024), 1.0, None, None, 1.0, at(4096), None)
    expect(lambda: c24(hip.C24_CONV24, 20, 0, 0, 0, 1, 8, 8), lambda: conv(h.refvsr_conv24, 20, 0), 'conv24: 20 + 0 input channels not supported')
    expect(lambda: c24(hip.C24_CONV24, 24, 0, 1, 0, 5, 8, 8), lambda: h.refvsr_conv24_batch(s2, 24, None, 0, 5, 8, 8, at(1024), 1.0, None, None, 1.0, o2, None),
           'conv24_batch: 1..4 maps per launch')
    expect(lambda: c24(hip.C24_CONV32, 24, 0, 0, 1, 1, 8, 8), lambda: conv(h.refvsr_conv32_f16w, 24, 0), 'conv32: 24 + 0 input channels not supported')
    expect(lambda: c24(hip.C24_CONV48, 24, 24, 0, 0, 1, 8, 8), lambda: conv(h.refvsr_conv48, 24, 24), 'conv48: 24 + 24 input channels not supported')
    expect(lambda: c24(hip.C24_SHUFFLE2, 48, 0, 1, 0, 2, 8, 8), lambda: h.refvsr_conv_shuffle2_batch(s2, 2, 48, 8, 8, at(1024), 1.0, o2, None),
           'conv_shuffle2_batch: 48 channels not supported (24)')
    expect(lambda: c24(hip.C24_SHUFFLE2, 48, 0, 0, 1, 1, 8, 8), None,
           'conv_shuffle2_f16w: 24 channels only (the mid_channels = 24 family)')      # a shape without a twin: the dispatch's message (the entry
    #                                                                                    point gives it behind refvsr_init, which needs a device)
    conf = lambda f, cout, up: f(at(0), at(512), 8, 8, up, at(1024), at(2048), 0.2, at(3072), cout, 0.2, at(8192), None, None)
    expect(lambda: c24(hip.C24_CONF_ALPHA, 24, 3, 0, 0, 1, 8, 8), lambda: conf(h.refvsr_conf_alpha, 24, 3), 'conf_alpha: up must be 1 or 2')
    expect(lambda: c24(hip.C24_CONF_ALPHA, 32, 1, 0, 0, 1, 8, 8), lambda: conf(h.refvsr_conf_alpha, 32, 1), 'conf_alpha: 32 output channels not supported (24 | 48)')
    expect(lambda: c24(hip.C24_CONF_ALPHA, 48, 1, 0, 1, 1, 8, 8), None,
           'conf_alpha_f16w: 24 output channels only (the mid_channels = 24 family)')
    expect(lambda: c24(hip.C24_CONF_ALPHA, 48, 1, 1, 0, 2, 8, 8),
           lambda: h.refvsr_conf_alpha_batch(s2, s2, 2, 8, 8, 1, at(1024), at(2048), 0.2, at(3072), 48, 0.2, o2, None, None), 'conf_alpha_batch: 48 output channels not supported (24)')
    expect(lambda: c24(hip.C24_CONV_LAST, 16, 0, 0, 0, 1, 8, 8), lambda: h.refvsr_conv_last(at(0), 16, 8, 8, at(1024), at(2048), 8, 8, at(4096), None),
           'conv_last: 16 input channels not supported (24 | 48)')
    # the query's own arguments
    key.value = -1
    assert h.refvsr_conv24_variant(hip.C24_CONV24, 24, 0, 0, 0, 1, 8, 8, None, None, None) != 0 and b'null key' in h.refvsr_last_error()
    for bad in ((6, 24, 0, 0, 0, 1, 8, 8), (-1, 24, 0, 0, 0, 1, 8, 8), (0, 24, 0, 2, 0, 1, 8, 8), (0, 24, 0, 0, 2, 1, 8, 8), (0, 24, 0, 0, 0, 1, 0, 8)):
        assert c24(*bad) != 0 and h.refvsr_last_error() == b'conv24_variant: bad args' and key.value == -1
    assert c24(hip.C24_CONV32, 32, 0, 1, 0, 2, 8, 8) != 0 and h.refvsr_last_error() == b'conv24: no kernel for this plan'      # conv32 has no `_batch` form

    # resblock24: the setters and the probe buffer are the process's state (restored); no stream budget registered: by-size uses the device's CUs
    rkey = ctypes.c_int(-1)
    rb = lambda *a: h.refvsr_resblock24_variant(*a, None, ctypes.byref(rkey), ctypes.byref(n), ctypes.byref(lds))
    rk = lambda RELU, NWV, PROBE, TH, STORE, HEAD, WF: RELU | NWV << 1 | PROBE << 6 | TH << 7 | STORE << 12 | HEAD << 13 | WF << 14
    try:
        for waves, store, probe, args, want in ((8, 1, 0, (0, 0, 1, 3, 19, 45), (rk(1, 8, 0, 8, 1, 0, 0), 18, 64000)),
                                                (16, 0, 0, (0, 1, 0, 1, 33, 70), (rk(0, 16, 0, 16, 0, 0, 1), 9, 63488)),
                                                (4, 1, 0, (0, 0, 1, 1, 19, 45), (rk(1, 4, 0, 8, 0, 0, 0), 6, 64000)),
                                                (4, 1, 0, (1, 0, 0, 1, 19, 45), (rk(0, 8, 0, 8, 0, 1, 0), 6, 64000)),      # the head has no four-wave kernel: by size
                                                (16, 1, 1, (0, 0, 1, 1, 33, 70), (rk(1, 16, 1, 16, 0, 0, 0), 9, 77824)),
                                                (16, 1, 1, (0, 1, 1, 1, 33, 70), (rk(1, 16, 0, 16, 1, 0, 1), 9, 63488))):     # no probe kernel in the fp16 format
            assert h.refvsr_set_resblock24_waves(waves) == 0 and h.refvsr_set_resblock24_store(store) == 0
            h.refvsr_set_probe(at(0) if probe else None, 0)                  # (never written: nothing is launched)
            assert rb(*args) == 0, h.refvsr_last_error()
            assert (rkey.value, n.value, lds.value) == want, (waves, store, probe, args)
    finally:
        h.refvsr_set_probe(None, 0)
        h.refvsr_set_resblock24_waves(0)
        h.refvsr_set_resblock24_store(1)
    assert h.refvsr_resblock24_variant(0, 0, 1, 1, 8, 8, None, None, None, None) != 0 and b'null key' in h.refvsr_last_error()
    for bad in ((2, 0, 1, 1, 8, 8), (1, 1, 0, 1, 8, 8), (0, 2, 1, 1, 8, 8), (0, 0, 1, 5, 8, 8), (0, 0, 1, 0, 8, 8), (0, 0, 1, 1, 0, 8)):
        assert rb(*bad) != 0 and h.refvsr_last_error() == b'resblock24_variant: bad args'


def test_block_variant_queries_are_the_launchers_plans(libpath):
    """refvsr_resblock48_variant / refvsr_resblock_lean_variant (added symbols, ABI 15 unchanged): with a null grid pointer they are host
    only -- they answer here -- with the key, tile count and LDS bytes of the planned resblock48_kernel / resblock_lean_kernel
    instantiation under the process's probe buffer and wave setter (restored), and reject bad arguments with a message."""
    from refvsr_amd import hip
    h = hip.lib()
    buf = (ctypes.c_char * 64)()
    key, n, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    r48 = lambda *a: h.refvsr_resblock48_variant(*a, None, ctypes.byref(key), ctypes.byref(n), None, ctypes.byref(lds))
    rl = lambda *a: h.refvsr_resblock_lean_variant(*a, None, ctypes.byref(key), ctypes.byref(n), None, ctypes.byref(lds))
    try:
        for probe, args, want in ((0, (0.25, 1, 43, 77), (0, 18, 134912)), (0, (0.0, 3, 43, 77), (1, 54, 134912)),
                                  (1, (0.0, 1, 7, 5), (3, 1, 134912)), (1, (0.25, 1, 19, 45), (0, 6, 134912))):      # the leaky kernel has no probe form
            h.refvsr_set_probe(ctypes.cast(buf, ctypes.c_void_p) if probe else None, 0)      # (never written: nothing is launched)
            assert r48(*args) == 0, h.refvsr_last_error()
            assert (key.value, n.value, lds.value) == want, (probe, args)
        h.refvsr_set_probe(None, 0)
        for waves, args, want in ((8, (24, 19, 45), (2 | 8 << 3, 6, 78560)), (4, (8, 43, 77), (1 | 4 << 3, 18, 19552)),
                                  (4, (32, 7, 5), (2 | 1 << 2 | 4 << 3, 1, 108832))):
            assert h.refvsr_set_resblock_waves(waves) == 0
            assert rl(*args) == 0, h.refvsr_last_error()
            assert (key.value, n.value, lds.value) == want, (waves, args)
    finally:
        h.refvsr_set_probe(None, 0)
        h.refvsr_set_resblock_waves(8)
    assert h.refvsr_resblock48_variant(0.0, 1, 8, 8, None, ctypes.byref(key), None, None, None) == 0       # tile count, grid and LDS bytes are optional
    assert h.refvsr_resblock48_variant(0.0, 1, 8, 8, None, None, None, None, None) != 0 and b'null key' in h.refvsr_last_error()
    for bad in ((-0.5, 1, 8, 8), (1.5, 1, 8, 8), (0.0, 0, 8, 8), (0.0, 5, 8, 8), (0.0, 1, 0, 8), (0.0, 1, 8, 0)):
        assert r48(*bad) != 0 and h.refvsr_last_error() == b'resblock48_variant: bad args'
    assert h.refvsr_resblock_lean_variant(24, 8, 8, None, None, None, None, None) != 0 and b'null key' in h.refvsr_last_error()
    for bad in ((24, 0, 8), (24, 8, 0)):
        assert rl(*bad) != 0 and h.refvsr_last_error() == b'resblock_lean_variant: bad args'
    for c in (48, 20, 0):
        assert rl(c, 8, 8) != 0 and h.refvsr_last_error() == b'resblock_lean: channel count %d not supported by the fused kernel' % c


def test_multimap_entry_points_validate_before_device_work(libpath):
    """The ABI 11 entry points (host arrays of per-map device pointers): batch bounds, null table entries, shape support and aliasing are
    rejected with a message before anything touches the device."""
    from refvsr_amd import hip
    h = hip.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 65536)()
    at = lambda off: ctypes.cast(ctypes.addressof(buf) + off, P)
    arr = lambda *ps: (P * len(ps))(*[p.value for p in ps])

    def expect(rc, text):
        assert rc != 0 and text in h.refvsr_last_error().decode(), h.refvsr_last_error()

    assert hip.MAX_MAPS == 4
    s2, o2 = arr(at(0), at(4096)), arr(at(8192), at(12288))
    five = arr(at(0), at(64), at(128), at(192), at(256))
    expect(h.refvsr_resblock24_chain_batch(five, 5, 8, 8, 1, at(1024), 43264, 0.0, None, None, five, None), 'resblock24_chain: bad args')
    expect(h.refvsr_resblock24_chain_batch(s2, 2, 8, 8, 2, at(1024), 43264, 0.0, None, None, o2, None), 'n >= 2 needs scratch0')
    expect(h.refvsr_resblock24_chain_batch(s2, 2, 8, 8, 1, at(1024), 43264, 0.0, None, None, s2, None), 'buffers must be distinct')
    expect(h.refvsr_resblock24_chain_batch(arr(at(0), P(0)), 2, 8, 8, 1, at(1024), 43264, 0.0, None, None, o2, None), 'null map pointer (map 1)')
    expect(h.refvsr_resblock48_chain_batch(five, 5, 8, 8, 1, at(1024), 172544, 0.0, None, None, five, None), 'resblock48_chain: bad args')
    expect(h.refvsr_resblock48_chain_batch(s2, 2, 8, 8, 3, at(1024), 172544, 0.0, at(16384), None, o2, None), 'n >= 3 needs scratch1')
    expect(h.refvsr_resblock48_chain_batch(s2, 2, 8, 8, 1, at(1024), 172544, 0.0, None, None, arr(at(8192), at(8192)), None), 'buffers must be distinct')
    expect(h.refvsr_resblock48_chain_batch(s2, 2, 8, 8, 1, at(1024), 1024, 0.0, None, None, o2, None), 'stride >= 172544')
    expect(h.refvsr_conv24_batch(s2, 24, None, 0, 5, 8, 8, at(1024), 1.0, None, None, 1.0, o2, None), '1..4 maps per launch')
    expect(h.refvsr_conv24_batch(s2, 20, None, 0, 2, 8, 8, at(1024), 1.0, None, None, 1.0, o2, None), 'input channels not supported')
    expect(h.refvsr_conv24_batch(s2, 24, None, 24, 2, 8, 8, at(1024), 1.0, None, None, 1.0, o2, None), 'src1 / c1 mismatch')
    expect(h.refvsr_conv24_batch(s2, 24, None, 0, 2, 8, 8, at(1024), 1.0, None, None, 1.0, s2, None), 'in-place operation is not supported')
    expect(h.refvsr_conv_shuffle2_batch(s2, 2, 48, 8, 8, at(1024), 1.0, o2, None), '48 channels not supported (24)')
    expect(h.refvsr_conf_alpha_batch(s2, s2, 2, 8, 8, 3, at(1024), at(2048), 0.2, at(3072), 24, 0.2, o2, None, None), 'up must be 1 or 2')
    expect(h.refvsr_conf_alpha_batch(s2, s2, 2, 8, 8, 2, at(1024), at(2048), 0.2, at(3072), 24, 0.2, o2, o2, None), 'max by-product exists at up = 1 only')
    expect(h.refvsr_conf_alpha_batch(s2, s2, 2, 8, 8, 1, at(1024), at(2048), 0.2, at(3072), 48, 0.2, o2, None, None), '48 output channels not supported (24)')
    expect(h.refvsr_warp_nhwc16_batch(s2, 2, 8, 8, 20, s2, 8, 8, o2, None), 'warp_nhwc16: bad args')
    expect(h.refvsr_warp_nhwc16_up2_batch(five, 5, 8, 8, 24, five, 8, 8, five, None), '(map, flow) pairs per launch')
    expect(h.refvsr_warp_planar_batch(arr(at(0), P(0)), 2, 1, 8, 8, s2, 8, 8, o2, None), 'null pointer (pair 1)')


def test_fixed_channel_entry_points_validate_before_device_work(libpath):
    """conv32 / conv48 / conv_last / conv_hr_last: shape support comes first (fixed_plan.h:c24_plan), then the argument checks, all
    before anything touches the device; refvsr_resblock24_kblock is the NCG = 3 K plan behind a range check."""
    from refvsr_amd import hip
    h = hip.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 65536)()
    at = lambda off: ctypes.cast(ctypes.addressof(buf) + off, P)

    def expect(rc, text):
        assert rc != 0 and h.refvsr_last_error().decode() == text, h.refvsr_last_error()

    conv = lambda f, c0, src1, c1, h_, blob, act, out: f(at(0), c0, src1, c1, h_, 8, blob, act, None, None, 1.0, out, None)
    for name, f, bad in (('conv32', h.refvsr_conv32, (24, 0)), ('conv32', h.refvsr_conv32_f16w, (32, 8)), ('conv48', h.refvsr_conv48, (24, 24))):
        ok = (8, 0) if name == 'conv32' else (16, 0)
        expect(conv(f, bad[0], None, bad[1], 0, None, 2.0, at(0)), '%s: %d + %d input channels not supported' % (name, bad[0], bad[1]))   # before every other check
        expect(conv(f, ok[0], None, 0, 0, at(1024), 1.0, at(4096)), name + ': bad args')
        expect(conv(f, ok[0], at(2048), 0, 8, at(1024), 1.0, at(4096)), name + ': src1 / c1 mismatch')
        expect(conv(f, ok[0], None, 0, 8, at(1032), 1.0, at(4096)), name + ': blob must be 16-byte aligned')
        expect(conv(f, ok[0], None, 0, 8, at(1024), 2.0, at(4096)), name + ': activation slopes must lie in [0, 1]')
        expect(conv(f, ok[0], None, 0, 8, at(1024), 1.0, at(0)), name + ': in-place operation is not supported')
        expect(conv(f, ok[0], None, 0, 1 << 24, at(1024), 1.0, at(4096)), name + ': map too large for 32-bit offsets')
    expect(conv(h.refvsr_conv48, 8, None, 48, 8, at(1024), 1.0, at(4096)), 'conv48: src1 / c1 mismatch')

    last = lambda c, h_, blob, base, bh, out, fmt: h.refvsr_conv_last_fmt(at(0), c, h_, 8, blob, base, bh, 8, out, fmt, None)
    expect(last(16, 8, at(1024), at(2048), 8, at(4096), 7), 'conv_last: unknown result format 7')
    expect(last(16, 8, None, None, 0, None, 0), 'conv_last: 16 input channels not supported (24 | 48)')
    expect(last(24, 8, at(1024), at(2048), 3, at(4096), 0), 'conv_last: base frame 3x8 does not divide the output 8x8')
    expect(last(24, 8, None, at(2048), 8, at(4096), 0), 'conv_last: bad args')
    expect(last(48, 8, at(1032), at(2048), 8, at(4096), 0), 'conv_last: blob must be 16-byte aligned')
    expect(last(48, 8, at(1024), at(2048), 8, at(0), 0), 'conv_last: in-place operation is not supported')
    expect(h.refvsr_conv_last(at(0), 20, 8, 8, at(1024), at(2048), 8, 8, at(4096), None), 'conv_last: 20 input channels not supported (24 | 48)')

    hr = lambda h_, blob, act, base, bh, out, fmt: h.refvsr_conv_hr_last_fmt(at(0), h_, 8, blob, act, base, bh, 8, out, fmt, None)
    expect(hr(8, at(1024), 0.1, None, 8, at(4096), 0), 'conv_hr_last: bad args')
    expect(hr(0, at(1024), 0.1, at(2048), 8, at(4096), 0), 'conv_hr_last: bad args')
    expect(hr(8, at(1024), 0.1, at(2048), 8, at(4096), 3), 'conv_hr_last: unknown result format 3')
    expect(hr(8, at(1032), 0.1, at(2048), 8, at(4096), 0), 'conv_hr_last: blob must be 16-byte aligned')
    expect(hr(8, at(1024), 0.0, at(2048), 8, at(4096), 0), 'conv_hr_last: activation slope must lie in (0, 1]')
    expect(hr(8, at(1024), 0.1, at(2048), 3, at(4096), 0), 'conv_hr_last: base frame 3x8 does not divide the output 8x8')
    expect(hr(1 << 24, at(1024), 0.1, at(2048), 1 << 24, at(4096), 0), 'conv_hr_last: map too large for 32-bit offsets')
    expect(h.refvsr_conv_hr_last(at(0), 8, 8, None, 0.1, at(2048), 8, 8, at(4096), None), 'conv_hr_last: bad args')

    for s, q in ((-1, 0), (7, 0), (0, -1), (0, 4), (7, 4)):
        assert h.refvsr_resblock24_kblock(s, q) == -2
    assert [h.refvsr_resblock24_kblock(6, q) for q in range(4)] == [514, 66050, 131586, -1]     # u = 8 of rows 0..2, then the zero block
    assert [h.refvsr_resblock24_kblock(s, q) for s in range(7) for q in range(4)] == [h.refvsr_conv24_kblock(3, s, q) for s in range(7) for q in range(4)]


def test_blob_sizes_are_the_recorded_ones(libpath):
    """Every *_blob_bytes export for every (c0, c1) of {8, 16, 20, 24, 32, 48} x {0, 8, 24, 48} (c of {8, 16, 24, 32, 48, 96}): the sizes the
    library reported before they were expressed through fixed_plan.h:c24_blob_bytes, -1 for every other shape."""
    from refvsr_amd import hip
    h = hip.lib()
    pairs = {'conv24': {(8, 24): 27776, (16, 0): 15488, (24, 0): 21632, (24, 24): 43136},
             'conv32': {(8, 0): 12416, (32, 0): 36992},
             'conv48': {(8, 48): 110848, (16, 0): 30976, (48, 0): 86272, (48, 48): 166144},
             'conv24_f16w': {(8, 24): 18560, (16, 0): 10368, (24, 0): 14464, (24, 24): 28800},
             'conv32_f16w': {(8, 0): 6272, (32, 0): 18560}}
    for name, want in pairs.items():
        f = getattr(h, 'refvsr_%s_blob_bytes' % name)
        for c0 in (8, 16, 20, 24, 32, 48):
            for c1 in (0, 8, 24, 48):
                assert f(c0, c1) == want.get((c0, c1), -1), (name, c0, c1)
    single = {'conv_shuffle2': {24: 86528, 48: 345088}, 'conv_shuffle2_f16w': {24: 43520}, 'conv_last': {24: 7296, 48: 14464}}
    for name, want in single.items():
        f = getattr(h, 'refvsr_%s_blob_bytes' % name)
        for c in (8, 16, 24, 32, 48, 96):
            assert f(c) == want.get(c, -1), (name, c)
    assert h.refvsr_resblock24_f16w_blob_bytes() == 28928



def test_cu_budget_argument_checks_and_constants(libpath):
    """ABI 13 / 14 host-side contracts that need no GPU: REFVSR_MAX_MAPS of the library equals the binding's copy (checked at load
    time too), the CU-budget setter validates before any device work, the result-format enum of the header equals the binding's."""
    from refvsr_amd import hip
    h = hip.lib()
    assert h.refvsr_max_maps() == hip.MAX_MAPS == 4
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    assert re.search(r'REFVSR_RESULT_F32 = 0, REFVSR_RESULT_F16 = 1, REFVSR_RESULT_U8 = 2', src)
    assert (hip.RESULT_F32, hip.RESULT_F16, hip.RESULT_U8) == (0, 1, 2)
    assert h.refvsr_stream_set_cu_budget(ctypes.c_void_p(0x1000), 12) != 0 and b'multiple of 8' in h.refvsr_last_error()
    assert h.refvsr_stream_set_cu_budget(ctypes.c_void_p(0x1000), -8) != 0
    assert h.refvsr_stream_set_cu_budget(ctypes.c_void_p(0x1000), 0) == 0        # forgetting an unknown stream is not an error
    assert h.refvsr_convert_result(None, 16, hip.RESULT_U8, None, None) != 0 and b'bad args' in h.refvsr_last_error()
    assert h.refvsr_stream_destroy(None) != 0
