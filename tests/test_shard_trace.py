"""The multi-GPU host protocol, pinned event by event (CPU, gloo): what run_wavefront / run_sharded call on the executor, fetch
and send -- per rank, in order, with lanes, flags, peers, sizes and groups -- must equal the traces recorded from the runner
before it was rebuilt on the two pure per-rank programs (tests/golden/shard_traces.json, recorded with tests/shard_trace.py);
the programs themselves (shard_plan.chain_steps / lane_program) and the makespan model (tests/golden/shard_model.json) are checked
alongside."""
import json
import os
import re

import pytest

import shard_trace as st
from refvsr_amd import shard, shard_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STEP = re.compile(r'^.(?:b1|b|call)(\d+),([01])')            # a forward-branch step: frame, is_first_frame
IMPORT = re.compile(r'^.imp[ps]?$')
EXPORT = re.compile(r'^.exp[ps]?$')


@pytest.fixture(scope='module')
def golden_traces():
    return st.load_traces(os.path.join(GOLDEN, 'shard_traces.json'))


@pytest.fixture(scope='module')
def golden_model():
    with open(os.path.join(GOLDEN, 'shard_model.json')) as fh:
        return json.load(fh)


def _combos(trace):
    """(state received?, first, state sent?) of every forward-branch step of a trace: an import since the previous step, the flag,
    an export before the next step."""
    out, recv, cur = [], False, None
    for tok in trace.split():
        m = STEP.match(tok)
        if m:
            if cur is not None:
                out.append(tuple(cur))
            cur, recv = [recv, m.group(2) == '1', False], False
        elif IMPORT.match(tok):
            recv = True
        elif EXPORT.match(tok) and cur is not None:
            cur[2] = True
    if cur is not None:
        out.append(tuple(cur))
    return out


def test_recorded_traces_reach_every_branch(golden_traces):
    """The cap of the recording: every op kind of the lane program and every (received, first, sent) combination a chain step can
    have occurs in the recorded traces (received and first exclude each other)."""
    toks = set(re.sub(r'[\d.,]+.*$', '', t[1:]) for tr in golden_traces.values() for t in tr.split())
    for name, why in (('pg', "('ag', frames)"), ('pa', "('a1', f)"), ('prep', "('prep', i)"), ('irecv', "('post_recv', i, peer)"),
                      ('isend', "('send', i, peer)"), ('impc', "('wait_recv', i, peer)")):
        assert name in toks, 'no recorded trace runs a %s op' % why
    assert any(t[1:].startswith('isend') and t.endswith('ctx') for tr in golden_traces.values() for t in tr.split())
    seen = set(c for tr in golden_traces.values() for c in _combos(tr))
    want = set((r, f, s) for r in (False, True) for f in (False, True) for s in (False, True) if not (r and f))
    assert seen == want, 'missing: %s' % sorted(want - seen)
    kinds = set(k.split('@')[0].split('/')[-2] for k in golden_traces if '/sharded' not in k)
    assert kinds == set(k[0] for k in st.KINDS)


@pytest.mark.parametrize('world', [1, 2, 3])
def test_runner_traces_match_the_recorded_ones(world, golden_traces):
    """Every rank of every case: the same events in the same order; and the ranks' results together are the sequential walk of
    the recurrence (a misplaced hand-off or `first` flag changes them)."""
    got = st.run_world(world)
    specs = dict(st.cases(world))
    bad = [k for k in sorted(got) if got[k][0] != golden_traces['%s@%d' % k]]
    for cid, rank in bad[:3]:
        a, b = got[(cid, rank)][0].split(), golden_traces['%s@%d' % (cid, rank)].split()
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print('%s rank %d, event %d: got %s, recorded %s' % (cid, rank, i, a[i:i + 6], b[i:i + 6]))
    assert not bad, '%d of %d rank traces differ from the recorded ones (first: %s)' % (len(bad), len(got), bad[0])
    missing = sorted((c, r) for c in specs for r in range(world) if (c, r) not in got)
    assert not missing, '%d rank traces never arrived (a rank died or stalled), first: %s' % (len(missing), missing[0])
    assert len([k for k in golden_traces if k.startswith('w%d/' % world)]) == len(got)
    for cid, spec in specs.items():
        res = {}
        for r in range(world):
            assert not set(res) & set(got[(cid, r)][1]), 'a frame computed twice'
            res.update(got[(cid, r)][1])
        assert res == st.sequential(spec['nframes'], spec['reset']), cid


def _partitions():
    """(name, nframes, world, reset, parts): every wavefront case of the traces + all families at world 8, 64 frames."""
    out = []
    for world in (1, 2, 3):
        seen = set()
        for cid, spec in st.cases(world):
            if spec['run'] == 'wavefront' and (spec['nframes'], spec['reset'], spec['fam']) not in seen:
                seen.add((spec['nframes'], spec['reset'], spec['fam']))
                out.append((cid, spec['nframes'], world, spec['reset'], st.family_parts(shard, spec['fam'], spec['nframes'], world, spec['reset'])))
    for reset in (9, None):
        for fam in st.FAMILIES:
            parts = st.family_parts(shard, fam, 64, 8, reset)
            if parts is not None:
                out.append(('w8/n64/r%s/%s' % (reset or 0, fam), 64, 8, reset, parts))
    return out


def test_chain_steps_of_all_ranks_form_one_chain():
    for name, nframes, world, reset, parts in _partitions():
        blocks = shard.as_blocks(parts, world)
        starts = set(a for a, _, _ in blocks)
        steps = {}
        for r in range(world):
            for f, recv_from, first, send_to in shard_plan.chain_steps(blocks, r, reset):
                assert f not in steps, '%s: frame %d twice' % (name, f)
                assert recv_from != r and send_to != r
                steps[f] = (r, recv_from, first, send_to)
            assert [s[0] for s in shard_plan.chain_steps(blocks, r, reset)] == [f for a, b, q in blocks if q == r for f in range(a, b)]
        assert sorted(steps) == list(range(nframes)), name
        for f in range(nframes):
            r, recv_from, first, send_to = steps[f]
            if send_to is not None:
                assert f + 1 in steps and steps[f + 1][:2] == (send_to, r), '%s: the send after frame %d meets no receive' % (name, f)
            if recv_from is not None:
                assert steps[f - 1][0] == recv_from and steps[f - 1][3] == r, '%s: the receive before frame %d meets no send' % (name, f)
            assert first == (f in starts and (f == 0 or bool(reset and f % reset == 0))), (name, f)
            assert not (first and recv_from is not None), (name, f)


def test_lane_program_is_the_grouped_plan_or_the_plain_window_list():
    for name, nframes, world, reset, parts in _partitions():
        blocks = shard.as_blocks(parts, world)
        plan = shard.ContextPlan(nframes, world, blocks, reset, st.FRAME_NUM)
        assert shard_plan.owner_map(blocks) == plan.owner
        for r in range(world):
            plain = [('a1', f) for a, b, q in blocks if q == r for f in range(a, b)]
            for g in (0, 1):
                assert shard_plan.lane_program(blocks, r, g) == plain
            for g in (1, 2, 3, 4):
                assert shard_plan.lane_program(blocks, r, g) == shard.group_lane_ops(plain, g)
                assert shard_plan.lane_program(blocks, r, g, plan) == shard.group_lane_ops(plan.program(r), g)


@pytest.mark.parametrize('point', st.model_grid(), ids=lambda pt: st.model_key(*pt))
def test_makespan_model_reproduces_the_recorded_floats(point, golden_model):
    """predicted_speedup (speedup, makespan) per partition family and choose_partition (blocks, speedup, name), as repr of the
    floats: makespans are whole multiples of dt, so any difference means the simulated order changed."""
    assert st.model_point(shard, *point) == golden_model[st.model_key(*point)]


def test_shard_plan_needs_no_torch():
    """The planning module is pure: a child interpreter that cannot import torch imports it and plans a clip."""
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, %r)\n"
            "import importlib.util as u\n"
            "s = u.spec_from_file_location('shard_plan', %r); m = u.module_from_spec(s); s.loader.exec_module(m)\n"
            "assert m.chain_steps(m.as_blocks(m.partition(5, 2)), 1, None) == [(3, 0, False, None), (4, None, False, None)]\n"
            % (st.ROOT, os.path.join(st.ROOT, 'refvsr_amd', 'shard_plan.py')))
    subprocess.run([sys.executable, '-c', code], check=True)
