"""Which entry point a conv call takes, and which specialised blob a conv carries, pinned on the CPU against
tests/golden/conv_routes.json: recorded from ops.conv / ops.conv_b / ops.ConvWeights as they stood when each of the two wrappers
carried its own copy of the conditions and the blob choice lived in the constructor (the case list of tests/packing_cases.py, run on a
copy of those files).  A recording library stands in for librefvsr_hip.so; the tensors are CPU tensors, the 2 GiB maps views of one
element."""
import json
import os

import pytest

import packing_cases as pc
import refvsr_amd
from refvsr_amd import engine, hip, ops
from refvsr_amd import packing as pk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_routes.json')
ROUTES = ('refvsr_conv_shuffle2', 'refvsr_conv24', 'refvsr_conv32', 'refvsr_conv48', 'refvsr_conv_shuffle2_batch', 'refvsr_conv24_batch',
          'refvsr_conv_mfma')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def shapes(golden):
    got = pc.conv_shapes(refvsr_amd, engine)
    assert sorted('%s | %s' % (pc.shape_name(s), f) for s in got for f in ('hi_lo', 'fp16')) == sorted(golden['blobs']) and len(got) == 39
    return got


def test_conv_calls_take_the_recorded_entry_points(golden, shapes, monkeypatch):
    with monkeypatch.context() as m:
        got = pc.route_table(ops, hip, pk, shapes, m.setattr)
    want = pc.unpack_table(golden['routes'], list(got))
    assert len(got) > 1500
    wrong = ['%s | act=%g post=%g: %s, recorded %s' % ((k,) + ap + (g, w))
             for k in got for ap, g, w in zip(pc.ACT_POST, got[k], want[k]) if g != w]
    assert not wrong, '%d of %d calls differ from the recorded routes:\n%s' % (len(wrong), 9 * len(got), '\n'.join(wrong[:20]))


def test_every_route_is_in_the_table(golden):
    used = set(golden['routes']['outcomes'][o] for p in golden['routes']['patterns'] for o in p)
    first = set(o.split()[0] for o in used)
    assert not set(ROUTES) - first
    assert not set(r + '_f16w' for r in ROUTES if 'conv24' in r or 'shuffle2' in r or 'conv32' in r) - first       # the fp16-format twins
    # the map-by-map fallback of conv_b: B > 1 launches of a single-map entry, behind the library query or without it
    assert any(int(o.split()[1]) > 1 and o.split()[2] == '1' for o in used) and any(int(o.split()[1]) > 1 and o.split()[2] == '0' for o in used)
    assert not [o for o in used if ' ' not in o], 'a call of the table raises'


def _flags(knob):
    return pk.BlobFlags(*[knob == k for k in pc.KNOBS[1:]])


def test_blob_plan_equals_the_recorded_choice(golden, shapes):
    want = golden['blobs']
    wrong, kinds = [], set()
    for shape in shapes:
        w_shape, srcs, shuffle, f32, hi_only = shape
        for wfmt in ('hi_lo', 'fp16'):
            plans = [pk.blob_plan(w_shape, list(srcs), shuffle, f32, hi_only, wfmt, _flags(knob)) for knob in pc.KNOBS]
            kinds.update(kind for kind, _ in plans)
            assert all(blob_wfmt == 'hi_lo' for kind, blob_wfmt in plans if kind is None)
            got, key = ''.join(pc.blob_code(kind is not None, blob_wfmt) for kind, blob_wfmt in plans), '%s | %s' % (pc.shape_name(shape), wfmt)
            if got != want[key]:
                wrong.append('%s: %s, recorded %s' % (key, got, want[key]))
    assert not wrong, '%d of %d rows of %d plans differ from the recorded ones:\n%s' % (len(wrong), len(want), len(pc.KNOBS), '\n'.join(wrong[:20]))
    assert kinds == {None, 'conv24', 'shuffle2'}
    # every knob and both formats decide something in the table
    for i in range(1, len(pc.KNOBS)):
        assert any(v[i] != v[0] for v in want.values()), pc.KNOBS[i]
    assert any('f' in v for v in want.values()) and any('h' in v for v in want.values())


def test_conv_weights_read_the_knobs_and_follow_the_plan(golden, shapes, monkeypatch):
    """ops.ConvWeights under each knob (REFVSR_NO_CONV24 is read when ops is imported: ops.CONV24; the other three at construction)."""
    def set_knob(name):
        for k in pc.KNOBS[1:]:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setattr(ops, 'CONV24', name != 'REFVSR_NO_CONV24')
        if name and name != 'REFVSR_NO_CONV24':
            monkeypatch.setenv(name, '1')
    assert pc.blob_table(ops, pk, shapes, set_knob) == golden['blobs']
    cw = ops.ConvWeights(pc.packed(pk, shapes[[pc.shape_name(s) for s in shapes].index('96<-24 k3 shuffle')]), 'cpu', wfmt='fp16')
    assert (cw.blob_kind, cw.blob_wfmt) == ('shuffle2', 'fp16') and cw.blob24 is not None
