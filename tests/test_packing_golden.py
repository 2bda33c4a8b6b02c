"""The bytes the kernels read, pinned on the CPU: sha256 digests of every blob packer's output and of every packed conv of every model,
against tests/golden/packing_digests.json -- recorded from packing.py / ops.py as they stood before the fragment packers became one
filler and a table of row layouts (the case list of tests/packing_cases.py, run on a copy of those files).  Then the identities that
let one packer stand for five."""
import json
import os

import numpy as np
import pytest
import torch

import packing_cases as pc
import refvsr_amd
from refvsr_amd import engine
from refvsr_amd import packing as pk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'packing_digests.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_packers_produce_the_recorded_bytes(golden):
    got = pc.packer_digests(pk)
    assert sorted(got) == sorted(golden['packers']) and len(got) == 33
    wrong = [k for k in sorted(got) if got[k] != golden['packers'][k]]
    assert not wrong, '%d of %d packer cases differ from the recorded bytes: %s' % (len(wrong), len(got), wrong)


@pytest.mark.parametrize('config,weight_precision', pc.model_cases())
def test_model_weights_produce_the_recorded_bytes(golden, config, weight_precision):
    assert pc.model_digest(refvsr_amd, engine, config, weight_precision) == golden['models']['%s %s' % (config, weight_precision or 'hi_lo')]


def test_rb24_kblock_is_the_three_group_table():
    assert all(pk.rb24_kblock(s, q) == pk.c24_kblock(3, s, q) for s in range(pk.RB24_S) for q in range(4))
    assert pk.RB24_S * 4 == 28 and pk.c24_steps(3) == pk.RB24_S


def _block(c, fp16):
    return pc.weights(1, c, c, fp16) + pc.weights(2, c, c, fp16)


@pytest.mark.parametrize('name,c,wfmt', [('pack_resblock24', 24, 'hi_lo'), ('pack_resblock24_f16w', 24, 'fp16'), ('pack_resblock48', 48, 'hi_lo')])
def test_block_blob_is_two_conv_blobs_and_two_bias_tails(name, c, wfmt):
    w1, b1, w2, b2 = _block(c, wfmt == 'fp16')
    blob = getattr(pk, name)(w1, b1, w2, b2)
    tail = 256 if c == 48 else 128
    c1, c2 = pk.pack_conv24(w1, b1, [c], wfmt=wfmt), pk.pack_conv24(w2, b2, [c], wfmt=wfmt)
    assert blob.dtype == torch.uint8 and blob.is_contiguous()
    assert blob.numel() == {'pack_resblock24': pk.RB24_BLOB, 'pack_resblock24_f16w': pk.RB24_F16W_BLOB, 'pack_resblock48': pk.RB48_BLOB}[name]
    assert torch.equal(blob, torch.cat([c1[:-tail], c2[:-tail], c1[-tail:], c2[-tail:]]))


def test_hr_last_blob_is_conv_hr_then_the_head_in_slot_0():
    (w_hr, b_hr), (w_last, b_last) = pc.weights(3, 24, 24), pc.weights(4, 3, 24)
    blob = pk.pack_conv_hr_last(w_hr, b_hr, w_last, b_last)
    hr, last = pk.pack_conv24(w_hr, b_hr, [24]), pk.pack_conv_last(w_last, b_last)
    wb = pk.RB24_S * pk.RB24_NF * 1024
    assert blob.numel() == pk.RB24_BLOB == 2 * wb + 256 and last.numel() == pk.RB24_S * 1024 + 128
    assert torch.equal(blob[:wb], hr[:wb]) and torch.equal(blob[2 * wb:2 * wb + 128], hr[wb:])
    conv2 = blob[wb:2 * wb].view(pk.RB24_S, pk.RB24_NF, 1024)
    assert torch.equal(conv2[:, 0].reshape(-1), last[:-128]) and not conv2[:, 1:].any()
    assert torch.equal(blob[2 * wb + 128:], last[-128:])
    assert np.array_equal(blob[2 * wb + 128:].numpy().view(np.float32)[:4], np.append(b_last.numpy(), 0))
