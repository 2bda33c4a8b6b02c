"""The parameter fingerprint without a GPU: the numpy model's properties (refvsr_amd/fingerprint.py), the chunk-table builder, the
weight-check policy's truth table, and the library boundary (refvsr_param_fingerprint validates before any launch)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from refvsr_amd import fingerprint as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 255, 256, 257, 1023, 1025, 100352)


def _bits(rs, n):
    return rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope='module')
def table():
    rs = np.random.RandomState(7)
    return [_bits(rs, n).view(np.float32) for n in (5, 1, 300, 300, 4097)]


# ------------------------------------------------------------------------------------------------ model
def test_mix64_is_splitmix64s_finaliser():
    # splitmix64 seeded with 0: its first outputs are mix64 of the multiples of the golden-ratio increment (Vigna's reference values)
    g = 0x9e3779b97f4a7c15
    got = fp.mix64(np.array([g, (2 * g) % 2 ** 64, (3 * g) % 2 ** 64], dtype=np.uint64))
    assert [int(v) for v in got] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]
    assert (fp.MIX_MUL1, fp.MIX_MUL2) == (0xbf58476d1ce4e5b9, 0x94d049bb133111eb) and fp.MIX_MUL1 % 2 == fp.MIX_MUL2 % 2 == 1
    src = open(os.path.join(ROOT, 'refvsr_amd', 'csrc', 'fingerprint.hip')).read()
    assert '0xbf58476d1ce4e5b9ull' in src and '0x94d049bb133111ebull' in src        # the kernel's constants are the model's


def test_one_bit_flip_changes_the_fingerprint(table):
    f0 = fp.param_fingerprint_model(table)
    for t in (0, 2, 4):
        n = table[t].size
        for pos in (0, n // 2, n - 1):
            for bit in (0, 17, 31):
                mod = [a.copy() for a in table]
                mod[t].view(np.uint32)[pos] ^= np.uint32(1 << bit)
                assert fp.param_fingerprint_model(mod) != f0, (t, pos, bit)
    # patterns, not values: -0 for +0, another NaN payload
    z = [np.zeros(4, np.float32)]
    assert fp.param_fingerprint_model(z) != fp.param_fingerprint_model([np.array([0, -0.0, 0, 0], np.float32)])
    nan = np.array([0x7fc00000, 0x7fc00001], dtype=np.uint32)
    assert fp.param_fingerprint_model([nan[:1].view(np.float32)]) != fp.param_fingerprint_model([nan[1:].view(np.float32)])


def test_swapped_contents_change_the_fingerprint(table):
    assert table[2].size == table[3].size and not np.array_equal(table[2].view(np.uint32), table[3].view(np.uint32))
    sw = [table[0], table[1], table[3], table[2], table[4]]
    assert fp.param_fingerprint_model(sw) != fp.param_fingerprint_model(table)


def test_any_order_of_partial_sums_gives_the_same_bits(table):
    words = np.concatenate([fp.words_of(a) for a in table])
    t = fp.terms(words)
    want = fp.param_fingerprint_model(table)
    rs = np.random.RandomState(3)
    with np.errstate(over='ignore'):
        for parts in (1, 7, 64, 1000):
            cuts = np.sort(rs.choice(np.arange(1, t.size), size=parts - 1, replace=False)) if parts > 1 else []
            partial = [p.sum(dtype=np.uint64) for p in np.split(t, cuts)]
            for _ in range(3):
                rs.shuffle(partial)
                total = np.uint64(0)
                for p in partial:
                    total = total + p
                assert int(total) == want
        assert int(t[rs.permutation(t.size)].sum(dtype=np.uint64)) == want


def test_split_into_other_tensors_at_the_same_global_indices(table):
    words = np.concatenate([fp.words_of(a) for a in table])
    want = fp.param_fingerprint_model(table)
    assert fp.param_fingerprint_model([words.view(np.float32)]) == want
    for cuts in ([1], [2, 3, 4], [100, 4096, 4097]):
        assert fp.param_fingerprint_model([w.view(np.float32) for w in np.split(words, cuts)]) == want
    # .. and as the chunks the kernel walks
    with np.errstate(over='ignore'):
        total = np.uint64(0)
        for t_, off, g, m in fp.chunk_table([a.size for a in table], 256):
            total = total + fp.terms(fp.words_of(table[t_])[off:off + m], g).sum(dtype=np.uint64)
    assert int(total) == want
    assert fp.as_int64(2 ** 64 - 1) == -1 and fp.as_int64(5) == 5 and fp.as_int64(2 ** 63) == -2 ** 63


# ------------------------------------------------------------------------------------------------ chunk table
@pytest.mark.parametrize('chunk_words', [fp.CHUNK_WORDS, 256, 1])
def test_chunk_table_covers_every_word_once(chunk_words):
    if chunk_words == 1:
        sizes = SIZES[:-1]
    else:
        sizes = SIZES
    ch = fp.chunk_table(sizes, chunk_words)
    seen = [np.zeros(n, np.int32) for n in sizes]
    g_next, last = 0, (0, 0)
    for t, off, g, m in ch:
        assert 1 <= m <= chunk_words and off + m <= sizes[t]
        assert g == g_next, 'global indices are consecutive'
        assert g == sum(sizes[:t]) + off
        assert (t, off) >= last
        last = (t, off)
        seen[t][off:off + m] += 1
        g_next += m
    assert g_next == sum(sizes) and all((s == 1).all() for s in seen)
    if chunk_words == fp.CHUNK_WORDS:
        assert len(ch) == 8 + 25                      # 100 352 = 24.5 x 4 096
        ent = fp.chunk_entries([4096 * (i + 1) + 4 * i for i in range(len(sizes))], sizes)
        assert ent.dtype.itemsize == 16 and len(ent) == len(ch)
        assert [int(e['base']) for e in ent[:3]] == [4096, 8196, 12296] and int(ent[-1]['base']) == 9 * 4096 + 32 + 4 * 24 * 4096
        assert int(ent['n'].sum()) == sum(sizes) and int(ent[-1]['g0']) + int(ent[-1]['n']) == sum(sizes)


def test_chunk_table_refuses_empty_and_oversized_tables():
    for bad in ([], [0], [0, 0]):
        with pytest.raises(ValueError, match='empty tensor list'):
            fp.chunk_table(bad)
    with pytest.raises(ValueError, match='empty tensor list'):
        fp.param_fingerprint_model([])
    with pytest.raises(ValueError, match='32-bit global index'):
        fp.chunk_table([2 ** 31, 2 ** 31])
    with pytest.raises(ValueError, match='4-byte aligned'):
        fp.chunk_entries([4098], [3])
    assert [c[1:] for c in fp.chunk_table([0, 3, 0, 2])] == [(0, 0, 3), (0, 3, 2)]      # tensors without words get no chunk


# ------------------------------------------------------------------------------------------------ policy
def test_policy_truth_table():
    for ids, first, reset in itertools.product((False, True), repeat=3):
        assert fp.weight_check_policy('off', ids, first, reset) == 'none'
        assert fp.weight_check_policy('sync', ids, first, reset) == 'sync'
    # (has frame_ids, first frame, just reset) -> 'auto'.  Steady calls without frame_ids are asynchronous as well: the synchronous
    # read cost the plain call surface 3.3 % against the parent commit (profiles/weight_check_ab.txt), past the 1 % bar
    auto = {(ids, first, reset): fp.weight_check_policy('auto', ids, first, reset)
            for ids, first, reset in itertools.product((False, True), repeat=3)}
    assert auto == {(False, False, False): 'async', (False, False, True): 'sync', (False, True, False): 'sync', (False, True, True): 'sync',
                    (True, False, False): 'async', (True, False, True): 'sync', (True, True, False): 'sync', (True, True, True): 'sync'}
    with pytest.raises(ValueError, match='weight_check must be one of auto, sync, off'):
        fp.weight_check_policy('always', True, False, False)


def test_config_field_and_cli_flag():
    from refvsr_amd import evalrun, get_config
    assert get_config('p', 'm', 'config_RefVSR_small_L1').weight_check == 'auto'
    base = ['--config', 'config_RefVSR_small_L1']
    assert evalrun.build_config(base).weight_check == 'auto'
    assert evalrun.build_config(base + ['--weight_check', 'sync']).weight_check == 'sync'
    assert evalrun.build_config(base + ['--weight_check', 'off']).weight_check == 'off'
    with pytest.raises(SystemExit):
        evalrun.build_config(base + ['--weight_check', 'never'])


def test_network_host_detector_sees_every_pointer(small_cfg):
    """The host-side key holds the address of every parameter: `p.data = w` on a middle parameter changes it (the first / last
    pointer test of before did not); no GPU, no library."""
    import torch
    from refvsr_amd import SRNet
    net = SRNet(small_cfg).Network
    k0 = net._weights_key()
    params = list(net.parameters())
    assert len(k0[2]) == len(params) > 100
    mid = params[len(params) // 2]
    mid.data = torch.ones_like(mid)
    k1 = net._weights_key()
    assert k1 != k0 and k1[0] == k0[0] and k1[1] == k0[1] and k1[2][0] == k0[2][0] and k1[2][-1] == k0[2][-1]
    assert hasattr(SRNet, 'invalidate') and net.weight_check_mode() == 'auto'


# ------------------------------------------------------------------------------------------------ library and binding
@pytest.fixture(scope='module')
def lib():
    from refvsr_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    h = lib
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 8192)()                    # host memory standing in for device pointers: never dereferenced
    base = (ctypes.addressof(buf) + 255) & ~255
    at = lambda off: P(base + off)

    def expect(rc, text):
        assert rc != 0 and h.refvsr_last_error().decode() == text, h.refvsr_last_error()

    f = h.refvsr_param_fingerprint
    expect(f(None, 1, at(1024), 64, at(2048), None), 'param_fingerprint: null chunk table')
    expect(f(at(0), 0, at(1024), 64, at(2048), None), 'param_fingerprint: 1..4194304 chunks (got 0)')
    expect(f(at(0), -3, at(1024), 64, at(2048), None), 'param_fingerprint: 1..4194304 chunks (got -3)')
    expect(f(at(8), 1, at(1024), 64, at(2048), None), 'param_fingerprint: chunk table must be 16-byte aligned')
    expect(f(at(0), 1, None, 64, at(2048), None), 'param_fingerprint: null workspace / out')
    expect(f(at(0), 1, at(1024), 64, None, None), 'param_fingerprint: null workspace / out')
    expect(f(at(0), 1, at(1032), 64, at(2048), None), 'param_fingerprint: workspace must be 16-byte aligned')
    expect(f(at(0), 1, at(1024), 64, at(2052), None), 'param_fingerprint: out must be 8-byte aligned')
    expect(f(at(0), 9, at(1024), 64, at(2048), None), 'param_fingerprint: workspace too small (64 bytes, 72 needed)')
    expect(f(at(0), 1, at(1024), 0, at(2048), None), 'param_fingerprint: workspace too small (0 bytes, 8 needed)')
    ws = h.refvsr_param_fingerprint_workspace_bytes
    assert [ws(n) for n in (-1, 0, 1, 9, 1 << 22, (1 << 22) + 1)] == [0, 0, 8, 72, 8 << 22, 0]


def test_header_binding_and_library_agree(lib):
    from refvsr_amd import hip
    src = open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
    assert 'ckpt_manager.py:50-60' in src
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(refvsr_[a-z0-9_]+)\s*\(', src))
    new = {'refvsr_param_fingerprint', 'refvsr_param_fingerprint_workspace_bytes'}
    assert new <= declared and declared == set(hip.EXPORTS)
    assert len(hip.SIGNATURES['refvsr_param_fingerprint']) == 6
    for name in new:
        assert hasattr(lib, name)
    assert re.search(r'#define REFVSR_FINGERPRINT_CHUNK_WORDS %d\b' % hip.FINGERPRINT_CHUNK_WORDS, src) and hip.FINGERPRINT_CHUNK_WORDS == fp.CHUNK_WORDS
    assert not [n for n in new if n.endswith('_f16w')]
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert '%d entry points' % len(hip.EXPORTS) in readme


def test_abi_version_is_still_15(lib):
    from refvsr_amd import hip
    assert hip.ABI_VERSION == 15 and lib.refvsr_abi_version() == 15
    assert '#define REFVSR_ABI_VERSION 15' in open(os.path.join(ROOT, 'include', 'refvsr_hip.h')).read()
