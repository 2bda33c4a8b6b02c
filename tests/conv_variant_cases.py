"""One exact case for EVERY instantiation of conv_mfma_kernel: the table behind tests/test_conv_variant_cases.py (CPU) and
tests/test_gpu_conv_variants.py (the kernels).

refvsr_conv_mfma dispatches to one of the 56 entries of RV_CONV_VARIANTS (refvsr_amd/csrc/conv_plan.h).  Row i of ROWS is a conv
descriptor that the planner sends to entry i, the REFVSR_CONV_* knob set under which it does so, and an exact-arithmetic case for it:
hi + lo weights (exact_cases), plain fp16 weights (`hi_only`, the HI1 variants) or fp32 operands (f32_cases, the F32 variants).  The
knobs are read once per process, so rows with a knob run in a child process (tests/conv_variant_child.py).

How a row's descriptor was chosen (asserted by the CPU test): ksize >= 3; at least 5 K-steps; a streamed variant has more weight
chunks (of CONV_CH = 8 K-steps) than ring slots, so the ring wraps; the 19 x 45 input leaves partial tiles in both directions for 4-,
8- and 16-row tiles (with a stride, the output is smaller than one tile both ways: still partial, and the variant is not reachable at
stride 1 where the row has one); packing.pack_conv accepts it.  No row needs an exception.  Resident variants run a second time on
33 x 70 with refvsr_set_conv_workgroup_cap(2): every workgroup then walks several tiles through the prefetch path.

Epilogues: EPI = 1 (lean) rows store fp16 HWC with slopes in [0, 1]; resident fp16 rows with EPI = 0 get there by a planar fp32
output; everything else alternates between the two stores.  Each family (gather, single-fp16, resident, streamed, fp32) holds two
sources, mt 1 to 3 (single-fp16: 1 and 2, all it is built for), nz > 1, both stores and mul / res / post operands.
"""
import collections

import exact_cases as ec
import f32_cases as fc

FIELDS = ('MT', 'TILES', 'F32', 'GATHER', 'RESIDENT', 'EPI', 'NW', 'HI1')
KNOBS = collections.OrderedDict((('', {}), ('NO_NW8', {'REFVSR_CONV_NO_NW8': '1'}), ('TILES4', {'REFVSR_CONV_TILES': '4'})))
WALK_HW, WALK_CAP = (33, 70), 2
EPILOGUES = {
    # fp16 / fp32 HWC or planar
    'plain': dict(),
    'relu': dict(act=0.0),
    'res_relu': dict(res=True, post=0.0),
    'lrelu_mul': dict(act=0.25, mul=True),
    'res_post': dict(res=True, post=0.25),
    'all': dict(act=0.25, mul=True, res=True, post=0.5),
    'mul_res_relu': dict(mul=True, res=True, post=0.0),
    # planar only
    'relu_resp': dict(act=0.0, res_planar=True),
    'const_clamp': dict(add_const=1.0, clamp=(0.5, 1.5)),
    'all_planar': dict(act=0.0, mul=True, res=True, post=0.0, res_planar=True, add_const=0.25, clamp=(-1.0, 1.0)),
}
PLANAR_ONLY = ('relu_resp', 'const_clamp', 'all_planar')

Row = collections.namedtuple('Row', 'variant knob cins cout ks stride mt out epi')


def variant_key(v):
    """conv_variant_key of conv_plan.h."""
    MT, TILES, F32, GATHER, RESIDENT, EPI, NW, HI1 = v
    return MT | TILES << 2 | NW << 6 | EPI << 11 | F32 << 12 | GATHER << 13 | RESIDENT << 14 | HI1 << 15


def mode(row):
    return 'f32' if row.variant[2] else 'hi_only' if row.variant[7] else 'hi_lo'


def geometry(row, hw):
    """(padded channel counts, (h_out, w_out), K-steps) of a row's descriptor at input size hw."""
    from refvsr_amd.packing import ksteps
    grp = 4 if mode(row) == 'f32' else 8
    cp = [(c + grp - 1) // grp * grp for c in row.cins]
    return cp, fc.out_hw(hw, row.ks, row.stride), ksteps(row.ks, sum(cp) // grp)


def descriptor(row, hw):
    """The fields that ops.conv puts into the RefvsrConv descriptor of a row at input size hw (pointers as 0 | 1: absent | present)."""
    cp, (ho, wo), S = geometry(row, hw)
    grp = 4 if mode(row) == 'f32' else 8
    e = EPILOGUES[row.epi]
    planar = row.out == 'planar'
    co_s = (row.cout + grp - 1) // grp * grp
    return collections.OrderedDict((
        ('c0', cp[0]), ('c1', cp[1] if len(cp) > 1 else 0), ('h_in', hw[0]), ('w_in', hw[1]), ('h_out', ho), ('w_out', wo), ('ksize', row.ks),
        ('stride', row.stride), ('pad', row.ks // 2), ('cout', row.cout), ('mt', row.mt), ('ksteps', S), ('act', e.get('act', 1.0)),
        ('post', e.get('post', 1.0)), ('mul', int(bool(e.get('mul')))), ('mul_c', co_s if e.get('mul') else 0), ('res', int(bool(e.get('res')))),
        ('res_c', co_s if e.get('res') else 0), ('out_mode', 2 if planar else 0), ('out_c', 0 if planar else co_s),
        ('res_planar', int(bool(e.get('res_planar')))), ('f32', {'hi_lo': 0, 'f32': 1, 'hi_only': 2}[mode(row)])))


def dump_line(row, hw):
    """The row as a line of tools/conv_plan_dump, knob included."""
    knob = {'': '', 'NO_NW8': ' NO_NW8=1', 'TILES4': ' TILES=4'}[row.knob]
    return ' '.join('%s=%g' % kv for kv in descriptor(row, hw).items()) + knob


def row_name(i, row, hw):
    return 'variant %02d %s %s %s->%d %dx%d s%d mt%d %s %s %dx%d' % ((i, ''.join(str(x) + '.' for x in row.variant)[:-1], mode(row), row.cins, row.cout, row.ks,
                                                                   row.ks, row.stride, row.mt, row.out, row.epi) + tuple(hw))


def build_case(i, row, walk=False):
    """The exact case of row i at 19 x 45, or its walk twin at 33 x 70 (resident variants)."""
    hw = WALK_HW if walk else ec.L19
    e = dict(EPILOGUES[row.epi])
    seed = 7000 + 2 * i + int(walk)
    name = row_name(i, row, hw)
    cap = WALK_CAP if walk else 0
    if mode(row) == 'f32':
        return fc._mfma(name, seed, 'dense', row.cout, list(row.cins), row.ks, hw, mt=row.mt, cap=cap, stride=row.stride, out=row.out, **e)
    hi_only = mode(row) == 'hi_only'
    for mag_exp in (-3, -4, -5):                            # the most significant bits (14, 13, 12) with which the bound holds
        c = ec._conv_case(name, seed, row.cout, list(row.cins), row.ks, hw, stride=row.stride, out=row.out, mag_exp=mag_exp,
                          run=dict(mt=row.mt, hi_only=hi_only, cap=cap), primary='hi' if hi_only else 'f64', **e)
        if c.bound < ec.LIMIT:
            break
    return c


def R(variant, knob, cins, cout, ks, stride, mt, out, epi):
    return Row(tuple(variant), knob, tuple(cins), cout, ks, stride, mt, out, epi)


# variant (MT, TILES, F32, GATHER, RESIDENT, EPI, NW, HI1) in the order of RV_CONV_VARIANTS, knob set, sources, cout, ksize, stride, mt, store, epilogue
ROWS = [
    R((1, 4, 0, 1, 0, 0, 4, 0), '', [3, 24], 32, 3, 4, 1, 'nhwc', 'relu'),    #  0: S=9, 2 chunks on 1 slots
    R((2, 4, 0, 1, 0, 0, 4, 0), '', [16], 32, 5, 4, 2, 'planar', 'relu_resp'),    #  1: S=13, 2 chunks on 1 slots
    R((3, 4, 0, 1, 0, 0, 4, 0), '', [32], 96, 3, 4, 3, 'nhwc', 'mul_res_relu'),    #  2: S=9, 2 chunks on 1 slots
    R((1, 2, 0, 0, 0, 0, 8, 1), '', [24, 24], 16, 5, 1, 1, 'planar', 'mul_res_relu'),    #  3: S=38, 5 chunks on 4 slots
    R((2, 2, 0, 0, 0, 0, 8, 1), '', [24], 64, 7, 1, 2, 'nhwc', 'relu'),    #  4: S=37, 5 chunks on 4 slots
    R((1, 4, 0, 0, 0, 0, 4, 1), 'NO_NW8', [24], 16, 7, 1, 1, 'planar', 'plain'),    #  5: S=37, 5 chunks on 4 slots
    R((2, 4, 0, 0, 0, 0, 4, 1), 'NO_NW8', [24, 24], 64, 5, 1, 2, 'nhwc', 'mul_res_relu'),    #  6: S=38, 5 chunks on 4 slots
    R((1, 2, 0, 0, 0, 0, 4, 1), '', [24], 16, 7, 4, 1, 'planar', 'const_clamp'),    #  7: S=37, 5 chunks on 4 slots
    R((2, 2, 0, 0, 0, 0, 4, 1), '', [16], 64, 7, 4, 2, 'nhwc', 'res_relu'),    #  8: S=25, 4 chunks on 2 slots
    R((3, 2, 0, 0, 1, 1, 16, 0), '', [24, 24], 48, 3, 1, 3, 'nhwc', 'res_post'),    #  9: S=14
    R((3, 2, 0, 0, 1, 0, 16, 0), '', [40], 96, 3, 1, 3, 'planar', 'plain'),    # 10: S=12
    R((2, 2, 0, 0, 1, 1, 16, 0), 'TILES4', [48], 32, 3, 1, 2, 'nhwc', 'plain'),    # 11: S=14
    R((2, 2, 0, 0, 1, 0, 16, 0), 'TILES4', [24, 24], 64, 3, 1, 2, 'planar', 'const_clamp'),    # 12: S=14
    R((1, 2, 0, 0, 1, 1, 8, 0), '', [8], 16, 5, 1, 1, 'nhwc', 'res_relu'),    # 13: S=7
    R((1, 2, 0, 0, 1, 0, 8, 0), '', [16], 32, 3, 1, 1, 'planar', 'all_planar'),    # 14: S=5
    R((1, 2, 0, 0, 0, 0, 8, 0), '', [24, 24], 16, 5, 1, 1, 'planar', 'plain'),    # 15: S=38, 5 chunks on 4 slots
    R((2, 2, 0, 0, 1, 1, 8, 0), '', [16], 64, 3, 1, 2, 'nhwc', 'all'),    # 16: S=5
    R((2, 2, 0, 0, 1, 0, 8, 0), '', [8], 32, 5, 1, 2, 'planar', 'const_clamp'),    # 17: S=7
    R((2, 2, 0, 0, 0, 0, 8, 0), '', [48, 48], 64, 3, 1, 2, 'nhwc', 'res_relu'),    # 18: S=27, 4 chunks on 2 slots
    R((3, 2, 0, 0, 1, 1, 8, 0), '', [16], 48, 3, 1, 3, 'nhwc', 'res_relu'),    # 19: S=5
    R((3, 2, 0, 0, 1, 0, 8, 0), '', [16], 96, 3, 1, 3, 'planar', 'plain'),    # 20: S=5
    R((3, 2, 0, 0, 0, 0, 8, 0), '', [3, 24], 48, 5, 1, 3, 'planar', 'relu_resp'),    # 21: S=25, 4 chunks on 2 slots
    R((1, 1, 1, 0, 1, 0, 8, 0), '', [28], 32, 3, 1, 1, 'nhwc', 'plain'),    # 22: S=16
    R((1, 1, 1, 0, 0, 0, 8, 0), '', [12], 16, 7, 4, 1, 'planar', 'mul_res_relu'),    # 23: S=37, 5 chunks on 4 slots
    R((2, 1, 1, 0, 1, 0, 8, 0), '', [12, 16], 64, 3, 1, 2, 'nhwc', 'lrelu_mul'),    # 24: S=16
    R((2, 1, 1, 0, 0, 0, 8, 0), '', [8], 32, 7, 4, 2, 'planar', 'plain'),    # 25: S=25, 4 chunks on 2 slots
    R((1, 2, 1, 0, 1, 0, 4, 0), 'NO_NW8', [28], 32, 3, 1, 1, 'nhwc', 'mul_res_relu'),    # 26: S=16
    R((1, 2, 1, 0, 0, 0, 4, 0), 'NO_NW8', [3, 28], 16, 5, 2, 1, 'planar', 'const_clamp'),    # 27: S=50, 7 chunks on 4 slots
    R((1, 2, 0, 0, 1, 1, 4, 0), '', [8, 48], 32, 3, 1, 1, 'nhwc', 'plain'),    # 28: S=16
    R((1, 2, 0, 0, 1, 0, 4, 0), '', [8, 48], 16, 3, 1, 1, 'planar', 'all_planar'),    # 29: S=16
    R((1, 2, 0, 0, 0, 0, 4, 0), '', [48, 48], 32, 3, 2, 1, 'nhwc', 'relu'),    # 30: S=27, 4 chunks on 2 slots
    R((1, 4, 1, 0, 1, 0, 4, 0), '', [8], 16, 3, 1, 1, 'planar', 'relu_resp'),    # 31: S=5
    R((1, 4, 1, 0, 0, 0, 4, 0), '', [64], 32, 3, 1, 1, 'nhwc', 'plain'),    # 32: S=36, 5 chunks on 4 slots
    R((1, 4, 0, 0, 1, 1, 4, 0), 'NO_NW8', [3, 24], 16, 3, 1, 1, 'nhwc', 'res_post'),    # 33: S=9
    R((1, 4, 0, 0, 1, 0, 4, 0), 'NO_NW8', [16], 32, 3, 1, 1, 'planar', 'all_planar'),    # 34: S=5
    R((1, 4, 0, 0, 0, 0, 4, 0), 'NO_NW8', [24], 16, 7, 1, 1, 'planar', 'plain'),    # 35: S=37, 5 chunks on 4 slots
    R((2, 2, 1, 0, 1, 0, 4, 0), 'NO_NW8', [12, 16], 64, 3, 1, 2, 'nhwc', 'mul_res_relu'),    # 36: S=16
    R((2, 2, 1, 0, 0, 0, 4, 0), 'NO_NW8', [8], 32, 7, 4, 2, 'planar', 'const_clamp'),    # 37: S=25, 4 chunks on 2 slots
    R((2, 2, 0, 0, 1, 1, 4, 0), '', [48], 64, 3, 1, 2, 'nhwc', 'lrelu_mul'),    # 38: S=14
    R((2, 2, 0, 0, 1, 0, 4, 0), '', [24, 24], 32, 3, 1, 2, 'planar', 'all_planar'),    # 39: S=14
    R((2, 2, 0, 0, 0, 0, 4, 0), '', [64], 64, 3, 2, 2, 'nhwc', 'relu'),    # 40: S=18, 3 chunks on 2 slots
    R((2, 4, 1, 0, 1, 0, 4, 0), '', [3], 32, 5, 1, 2, 'planar', 'relu_resp'),    # 41: S=7
    R((2, 4, 1, 0, 0, 0, 4, 0), '', [12, 16], 64, 5, 1, 2, 'nhwc', 'plain'),    # 42: S=44, 6 chunks on 4 slots
    R((2, 4, 0, 0, 1, 1, 4, 0), 'NO_NW8', [16], 32, 3, 1, 2, 'nhwc', 'res_relu'),    # 43: S=5
    R((2, 4, 0, 0, 1, 0, 4, 0), 'NO_NW8', [16], 64, 3, 1, 2, 'planar', 'all_planar'),    # 44: S=5
    R((2, 4, 0, 0, 0, 0, 4, 0), 'NO_NW8', [3, 24], 32, 5, 1, 2, 'planar', 'plain'),    # 45: S=25, 4 chunks on 3 slots
    R((3, 2, 1, 0, 1, 0, 4, 0), '', [28], 96, 3, 1, 3, 'nhwc', 'mul_res_relu'),    # 46: S=16
    R((3, 2, 1, 0, 0, 0, 4, 0), '', [12], 48, 5, 4, 3, 'planar', 'const_clamp'),    # 47: S=19, 3 chunks on 2 slots
    R((3, 2, 0, 0, 1, 1, 4, 0), '', [3, 24], 96, 3, 1, 3, 'nhwc', 'relu'),    # 48: S=9
    R((3, 2, 0, 0, 1, 0, 4, 0), '', [32], 48, 3, 1, 3, 'planar', 'all_planar'),    # 49: S=9
    R((3, 2, 0, 0, 0, 0, 4, 0), '', [48, 48], 96, 3, 1, 3, 'nhwc', 'relu'),    # 50: S=27, 4 chunks on 2 slots
    R((3, 4, 1, 0, 1, 0, 4, 0), '', [8], 48, 3, 1, 3, 'planar', 'relu_resp'),    # 51: S=5
    R((3, 4, 1, 0, 0, 0, 4, 0), '', [48], 96, 3, 1, 3, 'nhwc', 'plain'),    # 52: S=27, 4 chunks on 3 slots
    R((3, 4, 0, 0, 1, 1, 4, 0), 'NO_NW8', [8], 48, 5, 1, 3, 'nhwc', 'plain'),    # 53: S=7
    R((3, 4, 0, 0, 1, 0, 4, 0), 'NO_NW8', [16], 96, 3, 1, 3, 'planar', 'all_planar'),    # 54: S=5
    R((3, 4, 0, 0, 0, 0, 4, 0), 'NO_NW8', [64], 48, 3, 1, 3, 'planar', 'mul_res_relu'),    # 55: S=18, 3 chunks on 2 slots
]

_CACHE = {}


def get_case(i, walk=False):
    if (i, walk) not in _CACHE:
        _CACHE[(i, walk)] = build_case(i, ROWS[i], walk)
    return _CACHE[(i, walk)]


def is_resident(row):
    return bool(row.variant[4])
