"""CPU side of the exact-fp32 parity tests (tests/f32_cases.py, tests/test_gpu_f32_exact.py): for every case the GPU file runs,
  * the exactness condition holds (fewer than 2^24 granules at every stage, no subnormal) and the case's controls show that it
    would see what it is meant to see: a dropped 4-channel K-block of one tap (dense: >= 1 % and >= 8 outputs), fp16 or hi + lo
    (22-bit) weights (wfull: >= 5 %), fp16 activations (xfull: >= 5 %);
  * a float32 evaluation (F.conv2d in float32, MKL-DNN's summation order) equals the float64 reference exactly;
  * packing.pack_conv(f32=True) accepts the weights and its [nz, S, MT, 64, 4] fragments decode back to them exactly: every
    K-block once, zeros in the padding."""
import pytest
import torch

import exact_cases as ec
import f32_cases as fc
from f32_cases import get_case


def test_table_is_sound():
    assert fc.PREMISE.startswith('premise') and len(set(fc.NAMES)) == len(fc.NAMES) > 50
    v = fc.full24(ec.rng(3), (64,))
    n = (v.abs() * 2.0 ** 24)
    assert torch.equal(n, n.round()) and bool((n % 2 == 1).all()) and float(n.min()) >= 2 ** 23 and float(n.max()) < 2 ** 24
    assert torch.equal(v.float().double(), v) and not torch.equal(v.float().half().double(), v)
    hi = v.float().half().double()
    assert not torch.equal(hi + (v - hi).float().half().double(), v), '24-bit values must not fit the 22-bit hi + lo split'
    kinds = set((get_case(n).run['entry'], get_case(n).strength) for n in fc.NAMES if get_case(n).kind == 'conv')
    assert kinds == set((e, s) for e in ('conv_mfma', 'conv_direct', 'conv1x1') for s in ('dense', 'wfull', 'xfull'))


@pytest.mark.parametrize('name', fc.NAMES)
def test_case_is_exact_and_strong(name):
    c = get_case(name)
    print('%-60s %s' % (name, c.line()))
    c.assert_strong()
    if c.strength == 'dense' and c.kind == 'conv':
        n = (c.p['w'].abs() * 2.0 ** 17)
        assert float(n.max()) >= 2 ** 11, 'dense weights must need more bits than fp16 holds (12 to 14)'
        assert not torch.equal(c.p['w'].float().half().double(), c.p['w'])


@pytest.mark.parametrize('name', fc.NAMES)
def test_float32_emulation_equals_reference(name):
    c = get_case(name)
    p32 = c.evaluate('f32')[0]
    for k, v in c.want.items():
        assert torch.equal(p32[k].double(), v), '%s: float32 arithmetic is not exact on this case (%s)' % (name, k)


@pytest.mark.parametrize('name', [n for n in fc.NAMES if 'conv_mfma' in n])
def test_f32_packing_decodes_to_the_weights(name):
    from refvsr_amd import packing as pk
    c = get_case(name)
    p = c.p
    cins = [s.shape[0] for s in p['srcs']]
    packed = pk.pack_conv(p['w'].float(), p['b'].float(), cins, mt=c.run['mt'], f32=True)
    assert tuple(packed['wpack'].shape[2:]) == (packed['mt'], 64, 4) and packed['cpads'] == [fc.pad4(x) for x in cins]
    gw, gb = fc.decode_pack_conv_f32(packed, pk.kslot)
    assert torch.equal(gw, p['w']) and torch.equal(gb, p['b']), 'pack_conv(f32=True) fragments do not decode to w'


def test_decoder_sees_a_misplaced_fragment():
    from refvsr_amd import packing as pk
    c = get_case(fc.PREMISE)
    packed = pk.pack_conv(c.p['w'].float(), c.p['b'].float(), [24], f32=True)
    wp = packed['wpack'].clone()
    wp[0, 1, 0, 5], wp[0, 1, 0, 21] = packed['wpack'][0, 1, 0, 21], packed['wpack'][0, 1, 0, 5]      # two K-slots of one row swapped
    gw, _ = fc.decode_pack_conv_f32(dict(packed, wpack=wp), pk.kslot)
    assert not torch.equal(gw, c.p['w'])
