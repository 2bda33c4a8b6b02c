"""Pure planning for the multi-GPU run of one clip (no torch): who owns which frames, what every rank issues, what it costs.

  * partitions of a clip over the ranks (`partition*`, `as_blocks`, `owner_map`);
  * the two programs of a rank, which the runner (shard.run_wavefront / run_sharded) executes and the makespan model
    (`simulate_wavefront`) replays -- nothing else decides the order of calls or messages:
      - `lane_program`: lane a -- phase A of the local windows, single or in groups, with the context exchange (`ContextPlan`)
        also the preparation of contexts and their messages;
      - `chain_steps`: the forward-branch chain -- per local frame whether it starts behind a received state, runs as
        is_first_frame, and ends with a send;
  * the makespan model and `choose_partition`.
"""
import math

STATE_KEYS = ('feat', 'flow', 'feat_up', 'conf')
MAX_KEYFRAMES = 11


def partition(nframes, world, reset_branch=None, aligned=False):
    """Contiguous [start, end) frame ranges per rank.  aligned=True snaps boundaries to multiples of
    reset_branch (exchange-free, possibly unbalanced)."""
    if aligned:
        assert reset_branch, 'aligned partition needs reset_branch'
        units = list(range(0, nframes, reset_branch)) + [nframes]
        nunits = len(units) - 1
        per = [nunits // world + (1 if r < nunits % world else 0) for r in range(world)]
        out, u = [], 0
        for r in range(world):
            out.append((units[u], units[u + per[r]]))
            u += per[r]
        return out
    base, rem = divmod(nframes, world)
    out, s = [], 0
    for r in range(world):
        e = s + base + (1 if r < rem else 0)
        out.append((s, e))
        s = e
    return out


def needs_handoff(start, reset_branch):
    return start != 0 and not (reset_branch and start % reset_branch == 0)

def partition_hybrid(nframes, world, reset_branch):
    """The partition the wavefront uses when the forward branch restarts every reset_branch frames: boundaries snapped to
    multiples of reset_branch (those shards need no hand-off and start immediately), except that a short last shard is
    re-balanced with its predecessor -- ONE boundary then lies inside a restart unit and is served by the hand-off.
    64 frames, reset 9, 8 ranks: (0,9) (9,18) ... (45,54) (54,59) (59,64): seven exchange-free starts, one hand-off, the longest
    shard has 9 frames (64 / 9 = 7.1 x over one rank; the balanced partition needs a hand-off at every boundary)."""
    parts = partition(nframes, world, reset_branch, aligned=True)
    nz = [i for i, (a, b) in enumerate(parts) if b > a]
    if len(nz) >= 2:
        i, j = nz[-2], nz[-1]
        (a0, a1), (b0, b1) = parts[i], parts[j]
        if (a1 - a0) - (b1 - b0) >= 2:
            mid = a0 + (b1 - a0 + 1) // 2
            parts[i], parts[j] = (a0, mid), (mid, b1)
    return parts


def partition_chain(nframes, world, ratio=0.165):
    """Partition for a clip WITHOUT forward-branch restarts (reset_branch = None, BASELINE configs[4]): every boundary needs
    the hand-off, so the B1 steps of all frames form one serial chain over the ranks.  A rank can start its chain when its own
    phase A is done AND the state has arrived; equal shards make rank r wait for r whole shards of B1 (4.1 x at 8 ranks with
    the measured phase times).  Shards growing by (1 + ratio) per rank (ratio = t_B1 / t_A, 0.165 measured for RefVSR_small
    at 270p: profiles/r03_bench.json `wavefront_model`) let the chain arrive exactly when phase A ends: n_0 = x,
    n_r = x (1 + ratio)^r.  64 frames over 8 ranks: 4 5 6 7 8 10 11 13 -> 4.8 x predicted (equal shards: 4.1 x)."""
    if nframes < world:
        return partition(nframes, world)
    w = [(1.0 + ratio) ** r for r in range(world)]
    tot = sum(w)
    ideal = [nframes * v / tot for v in w]
    n = [max(1, int(v)) for v in ideal]          # every rank owns at least one frame (nframes >= world)
    # largest remainders first ...
    while sum(n) < nframes:
        r = max(range(world), key=lambda i: (ideal[i] - n[i], i))
        n[r] += 1
    # ... and when the floor-to-one bump overshot: take from the largest shard (ties -> highest rank), never below 1
    while sum(n) > nframes:
        r = max(range(world), key=lambda i: (n[i], i))
        assert n[r] > 1
        n[r] -= 1
    n.sort()                                      # non-decreasing sizes along the chain
    out, s0 = [], 0
    for v in n:
        out.append((s0, s0 + v))
        s0 += v
    return out


def as_blocks(parts, world=None):
    """Normalise a partition to chain order: [(start, end, rank), ...] sorted by start, empty ranges dropped.  Accepts the
    per-rank form [(start, end)] * world (contiguous shards: rank = position) or a block list [(start, end, rank), ...]
    (a rank may own several blocks -- `partition_cyclic`)."""
    parts = list(parts)
    if parts and len(parts[0]) == 2:
        blocks = [(a, b, r) for r, (a, b) in enumerate(parts) if b > a]
    else:
        blocks = [(a, b, r) for a, b, r in parts if b > a]
    blocks.sort()
    for (a0, b0, _), (a1, _, _) in zip(blocks, blocks[1:]):
        assert b0 == a1, 'partition must cover the clip contiguously'
    return blocks


def partition_cyclic(nframes, world, size):
    """Block-cyclic partition: blocks of `size` consecutive frames dealt to the ranks round-robin (the last block may be
    shorter).  For a clip WITHOUT forward-branch restarts every rank then has part of the EARLY frames: the B1 chain does not
    wait for one rank to walk a whole shard at the rate of its phase A (the start-up that bounds contiguous shards), at the price
    of one cold window (two frames prepared twice) and one hand-off per block."""
    assert size >= 1
    return [(s0, min(s0 + size, nframes), (i % world)) for i, s0 in enumerate(range(0, nframes, size))]


def partition_cyclic_growing(nframes, world, t_window, t_chain_step, t_start, scale=1.0, cap=8):
    """Block-cyclic partition whose blocks GROW along the clip, for clips without forward-branch restarts.  The B1 chain reaches
    frame f about t_start + f * t_chain_step after the start; the owner of the block that starts there must have finished phase A
    of all its earlier frames (f / world of them) and of this block by then: n <= (t_start + f t_chain_step) / t_window - f / world.
    One-frame blocks get the chain going (its first step waits for ONE window, not a block of them), larger blocks later save
    hand-offs -- the chain is what bounds such a clip.  scale: safety factor on n (choose_partition tries several)."""
    assert t_window > 0 and cap >= 1
    out, f0, k = [], 0, 0
    while f0 < nframes:
        n = int(math.floor(scale * ((t_start + f0 * t_chain_step) / t_window - f0 / float(world))))
        n = max(1, min(n, cap, nframes - f0))
        out.append((f0, f0 + n, k % world))
        f0 += n
        k += 1
    return out


def owner_map(blocks):
    """{frame: rank} of a block list (as_blocks)."""
    return {f: r for a, b, r in blocks for f in range(a, b)}


def window_ids(f, nframes, frame_num):
    """Frame indices of the window whose output frame is f (clip edges replicate frames, datasets.py:233-234)."""
    return [min(max(f - frame_num // 2 + k, 0), nframes - 1) for k in range(frame_num)]


def window_is_hinted(f, reset_branch):
    """Phase A of window f prepares ALL its frames (not only centre .. last): the forward branch restarts there (clip start or a
    multiple of reset_branch, RefVSR.py:168-176) and walks frames 0 .. centre itself."""
    return f == 0 or bool(reset_branch and f % reset_branch == 0)


class ContextPlan(object):
    """Who prepares which per-frame context and who needs it, for run_wavefront(exchange_contexts=True).

    A per-frame context is everything that is a function of ONE (lr_i, ref_i) pair -- matching, reference encoders, both
    aligned-attention outputs (Engine.prepare_frame, RefVSR.py:196-204,233-234,127,136): ~35 % of a frame's phase A.  Window f
    needs the contexts of its frames centre .. last (all of them when the forward branch restarts at f).  Without the exchange a
    rank prepares every context its windows need -- the first window of every block pays for two (four at a restart) contexts
    that the neighbouring block's owner prepares as well.  With it, context i is prepared ONCE, by the owner of output frame i,
    and sent to the other ranks whose windows need it (one message of ~32 MB at 270p, point to point, off the B1 chain).

    tasks[r]     lane-a order of rank r: ('prep', i) | ('a1', f): windows in block order, a context right before its first own use
                 or earlier when another rank's window needs it earlier on the B1 chain (see __init__)
    consumers[i] ranks other than the owner that need context i (sorted)
    imports[r][f] contexts rank r must have received before phase A of window f (first use only)
    Every rank issues its messages in increasing frame order (`messages`, `program`): one global order = no deadlock on in-order
    transports."""

    def __init__(self, nframes, world, parts, reset_branch, frame_num, lead=3):
        blocks = as_blocks(parts, world)
        t, ctr = frame_num, frame_num // 2
        self.blocks, self.nframes, self.world, self.t = blocks, nframes, world, t
        self.owner = owner_map(blocks)
        assert sorted(self.owner) == list(range(nframes)), 'partition must cover every frame once'
        self.windows = {r: [f for a, b, q in blocks if q == r for f in range(a, b)] for r in range(world)}
        self.needed = {}
        for f in range(nframes):
            ids = window_ids(f, nframes, t)
            self.needed[f] = sorted(set(ids[0 if window_is_hinted(f, reset_branch) else ctr:]))
        # first use of every context per rank: (window position, window)
        first_use = {r: {} for r in range(world)}
        for r in range(world):
            for pos, f in enumerate(self.windows[r]):
                for i in self.needed[f]:
                    first_use[r].setdefault(i, (pos, f))
        self.consumers = {i: sorted(r for r in range(world) if r != self.owner[i] and i in first_use[r]) for i in range(nframes)}
        self.imports = {r: {} for r in range(world)}
        for r in range(world):
            for i, (pos, f) in first_use[r].items():
                if self.owner[i] != r:
                    self.imports[r].setdefault(f, []).append(i)
            for f in self.imports[r]:
                self.imports[r][f].sort()
        # Lane-a order.  The windows of a rank keep their block order (the window cache follows the sliding window); a context is
        # prepared right before the first OWN window that needs it -- or earlier, when another rank needs it earlier.  "Earlier" is
        # measured on the B1 chain, which paces everything: window f's phase A is needed when the chain gets there, ct(f) = f - (the
        # last restart <= f) steps after its chain started (restart units are independent chains that start together); a context
        # for a foreign window f' has to be on its way `lead` steps before that (its transfer + the consumer's phase A).
        ct = {}
        for f in range(nframes):
            ct[f] = 0 if window_is_hinted(f, reset_branch) else ct[f - 1] + 1
        self.tasks = {}
        for r in range(world):
            own = [i for i in range(nframes) if self.owner[i] == r]
            seq = self.windows[r]
            due = {}
            for i in own:
                pos = first_use[r][i][0] if i in first_use[r] else len(seq)
                when = float(ct[seq[pos]]) if pos < len(seq) else float('inf')
                for q in self.consumers[i]:
                    dl = ct[first_use[q][i][1]] - lead
                    p2 = next((p for p, f in enumerate(seq) if ct[f] > dl), len(seq))
                    if p2 < pos or (p2 == pos and dl < when):
                        pos, when = min(pos, p2), min(when, float(dl))
                due[i] = (pos, when, i)
            todo = sorted(own, key=lambda i: due[i])
            out, k = [], 0
            for pos, f in enumerate(seq):
                while k < len(todo) and due[todo[k]][0] <= pos:
                    out.append(('prep', todo[k]))
                    k += 1
                out.append(('a1', f))
            assert k == len(todo), 'a context nobody needs'
            self.tasks[r] = out

    def program(self, r):
        """The host program of rank r's lane a: ('prep', i) | ('post_recv', i, peer) | ('send', i, peer) | ('wait_recv', i, peer) |
        ('a1', f), in issue order.  tasks[r] with the messages put in: a context is sent right after its preparation, a receive is
        posted (and waited for) right before the first window that needs it -- and EVERY rank issues its messages in increasing
        frame order (`messages`): whatever that order puts before a message is issued first (a receive is just posted early; a send
        whose context is not prepared yet prepares it on the spot).  One global order on all ranks = no deadlock on any in-order
        transport: per rank pair (lazily initialised ProcessGroupNCCL: a communicator and a stream per pair) and even when all
        operations of a rank share ONE stream (eagerly initialised groups serialise unbatched send / recv with everything else)."""
        msgs = self.messages(r)
        state = {'ptr': 0}
        prepared, out = set(), []

        def prepare(i):
            if i not in prepared:
                out.append(('prep', i))
                prepared.add(i)

        def issue_until(upto):
            while state['ptr'] < len(msgs) and msgs[state['ptr']][0] <= upto:
                i, kind, p = msgs[state['ptr']]
                state['ptr'] += 1
                if kind == 'recv':
                    out.append(('post_recv', i, p))
                else:
                    prepare(i)
                    out.append(('send', i, p))

        for kind, x in self.tasks[r]:
            if kind == 'prep':
                prepare(x)
                if self.consumers[x]:
                    issue_until(x)
            else:
                for i in self.imports[r].get(x, ()):
                    issue_until(i)
                    out.append(('wait_recv', i, self.owner[i]))
                out.append(('a1', x))
        issue_until(self.nframes)
        return out

    def messages(self, r):
        """All context messages of rank r in the order it issues them: [(frame, 'send' | 'recv', peer)] by frame, then peer."""
        out = []
        for i in range(self.nframes):
            if self.owner[i] == r:
                out += [(i, 'send', q) for q in self.consumers[i]]
            elif r in self.consumers[i]:
                out.append((i, 'recv', self.owner[i]))
        return out

    def pair_order(self, r, peer):
        """All context messages between r and peer, in the order both ends issue them: [(frame, 'send' | 'recv')] from r's view."""
        out = []
        for i in range(self.nframes):
            if self.owner[i] == r and peer in self.consumers[i]:
                out.append((i, 'send'))
            elif self.owner[i] == peer and r in self.consumers[i]:
                out.append((i, 'recv'))
        return out


def group_lane_ops(program, group):
    """Phase-A groups (round 6): the lane-a program of a rank -- ('a1', f) ops, with the context exchange also ('prep', i),
    ('send', i, peer), ('post_recv', i, peer), ('wait_recv', i, peer) -- with runs of up to `group` windows turned into ONE
    ('ag', (f1, ..., fk)) op: their backward branches are independent chains over identical weights and run as multi-map launches
    (Engine.phase_a_group), whether the windows are consecutive or not.  Everything that stood between the windows of a group is
    issued BEFORE the group (a window computes nothing another op waits for: deferring it reorders no message -- every rank still
    issues its sends and receives in the one global order of ContextPlan.program -- and cannot close a cycle).  group <= 1: unchanged."""
    if group <= 1:
        return list(program)
    out, cur = [], []
    for op in program:
        if op[0] == 'a1':
            cur.append(op[1])
            if len(cur) == group:
                out.append(('ag', tuple(cur)))
                cur = []
        else:
            out.append(op)
    if cur:
        out.append(('ag', tuple(cur)))
    return out


def lane_program(blocks, rank, group, plan=None):
    """The lane-a program run_wavefront executes on `rank`: its windows in block order -- with a ContextPlan, plan.program(rank) --
    in phase-A groups of up to `group` windows."""
    if plan is not None:
        return group_lane_ops(plan.program(rank), group)
    return group_lane_ops([('a1', f) for a, b, r in blocks if r == rank for f in range(a, b)], group)


def chain_steps(blocks, rank, reset_branch):
    """The forward-branch chain of `rank`: its frames in chain order, [(f, recv_from, first, send_to)] --
    recv_from  the rank whose state frame f starts from: f opens a block behind a hand-off and another rank owns f - 1, else None
               (a block that continues a block of the same rank just goes on: neither received nor first);
    first      f runs as is_first_frame: it opens a block that needs no hand-off (the clip start or a multiple of reset_branch; a
               restart INSIDE a block is not flagged -- the executor restarts there from its own frame counter);
    send_to    the rank the state goes to after f: f ends a block, another rank owns the next one and that one needs a hand-off.
    The ONLY place that decides these three things, for the runners and for the model."""
    owner = owner_map(blocks)
    out = []
    for a, b, r in blocks:
        if r != rank:
            continue
        handoff, nxt = needs_handoff(a, reset_branch), owner.get(b)
        send_to = nxt if nxt is not None and nxt != rank and needs_handoff(b, reset_branch) else None
        for f in range(a, b):
            recv_from = owner[a - 1] if f == a and handoff and owner[a - 1] != rank else None
            out.append((f, recv_from, f == a and not handoff, send_to if f == b - 1 else None))
    return out


def group_time(k, group, t_a, t_a_single):
    """Phase-A time PER FRAME of a group of k windows when a full group of `group` costs t_a per frame and a lone window t_a_single:
    linear in between (the multi-map launches share one weight fill and one launch among k tiles)."""
    if group <= 1 or t_a_single is None or k >= group:
        return t_a
    return t_a_single - (t_a_single - t_a) * (k - 1) / float(group - 1)


def simulate_wavefront(nframes, world, parts, reset_branch, t_a, t_b1, t_b2, t_handoff=0.0, t_cold=0.0, interleaved=True, dt=0.01,
                       exchange=None, frame_num=5, group=1, t_a_single=None):
    """Makespan of run_wavefront from per-frame phase times (any time unit): every rank executes ONE task at a time with
    priorities  B1 (its phase A done, the previous frame's B1 done and -- across ranks -- handed over) > phase A (lane-a order)
    > B2, pre-emptively (the kernels of the two streams interleave at ~10 us granularity).
    t_cold: extra phase-A time of the first frame of a block that does not start the clip (its window is not in the cache: TWO more
    contexts to prepare; FOUR when the forward branch restarts at that frame -- a reset-aligned block start prepares the whole
    window -- i.e. 2 t_cold).
    interleaved=False: the round-3 order (B1 of a rank only after ALL its phase A).
    exchange: None | dict(t_prep, t_ctx, t_cold_x=0, lookahead=1) -- run_wavefront(exchange_contexts=True): every context is
    prepared once, by the owner of its frame (t_prep of the t_a), and sent to the ranks that need it (t_ctx after its preparation
    it is usable there); lane a follows ContextPlan.tasks (in order: a window waiting for an import blocks the lane), a block start
    costs t_cold_x (the flows of a cold window) instead of t_cold.
    group > 1 (round 6): lane a runs phase A in groups of up to `group` windows (group_lane_ops: what run_wavefront(group=) executes);
    t_a is then the per-frame phase-A time INSIDE a full group, t_a_single that of a lone window (group_time), a group is ready when
    every import of every member is there and all its windows are done at its end.  Returns the makespan."""
    blocks = as_blocks(parts)
    owner, first = owner_map(blocks), set(a for a, _, _ in blocks)
    assert sorted(owner) == list(range(nframes)), 'partition must cover every frame once'
    steps = {r: chain_steps(blocks, r, reset_branch) for r in range(world)}
    frames_of = {r: [s[0] for s in steps[r]] for r in range(world)}
    recv_from = {s[0]: s[1] for r in range(world) for s in steps[r]}
    if exchange is None:
        plan, imports, t_prep, t_ctx, t_win = None, {r: {} for r in range(world)}, 0.0, 0.0, t_a
        extra = lambda f: 0.0 if (f not in first or f == 0) else (2.0 * t_cold if window_is_hinted(f, reset_branch) else t_cold)
    else:
        plan = ContextPlan(nframes, world, blocks, reset_branch, frame_num) if exchange.get('plan') is None else exchange['plan']
        t_prep, t_ctx, t_cold_x = exchange['t_prep'], exchange.get('t_ctx', 0.0), exchange.get('t_cold_x', 0.0)
        assert 0.0 <= t_prep <= t_a
        imports, t_win = plan.imports, t_a - t_prep
        extra = lambda f: t_cold_x if (f in first and f != 0) else 0.0
    # the lanes: what run_wavefront executes (lane_program) without the messages, every op with its duration -- a window: its share
    # of t_a + its cold terms; a group ('ag', members): the members' times at the group's per-frame rate
    dur = {('a1', f): t_win + extra(f) for f in range(nframes)}
    dur.update((('prep', i), t_prep) for i in range(nframes))
    lane = {}
    for r in range(world):
        lane[r] = []
        for op in lane_program(blocks, r, group, plan):
            if op[0] == 'ag':
                per = group_time(len(op[1]), group, t_a, t_a_single) - t_prep
                lane[r].append(('ag', op[1], sum(per + (dur[('a1', f)] - t_win) for f in op[1])))
            elif op[0] in ('a1', 'prep'):
                lane[r].append((op[0], op[1], dur[op]))
    rem_lane = {r: [d for _, _, d in lane[r]] for r in range(world)}
    rem_b1 = {f: t_b1 for f in range(nframes)}
    rem_b2 = {f: t_b2 for f in range(nframes)}
    done_a, done_b1, done_b2, done_prep = {}, {}, {}, {}
    nxt_l = {r: 0 for r in range(world)}
    nxt_b1 = {r: 0 for r in range(world)}
    nxt_b2 = {r: 0 for r in range(world)}
    n_steps = 0
    t = 0.0
    limit = 100.0 * nframes * (t_a + t_b1 + t_b2 + 2.0 * t_cold + t_handoff + t_ctx) + 1.0
    while len(done_b2) < nframes:
        assert t < limit, 'schedule does not terminate'
        for r in range(world):
            fs = frames_of[r]
            ran = False
            if nxt_b1[r] < len(fs):
                f = fs[nxt_b1[r]]
                ok = f in done_a
                if ok and needs_handoff(f, reset_branch):
                    ok = f - 1 in done_b1 and t >= done_b1[f - 1] + (t_handoff if recv_from[f] is not None else 0.0)
                if ok and not interleaved:
                    ok = nxt_l[r] >= len(lane[r])
                if ok:
                    rem_b1[f] -= dt
                    if rem_b1[f] <= 1e-9:
                        done_b1[f] = t + dt
                        nxt_b1[r] += 1
                    ran = True
            if not ran and nxt_l[r] < len(lane[r]):
                kind, x, _ = lane[r][nxt_l[r]]
                ready = True
                members = (x,) if kind == 'a1' else (x if kind == 'ag' else ())
                for f_ in members:
                    for i in imports[r].get(f_, ()):
                        ready = ready and i in done_prep and t >= done_prep[i] + t_ctx
                if ready:
                    j = nxt_l[r]
                    rem_lane[r][j] -= dt
                    if rem_lane[r][j] <= 1e-9:
                        if kind == 'prep':
                            done_prep[x] = t + dt
                        for f_ in members:
                            done_a[f_] = t + dt
                        nxt_l[r] += 1
                    ran = True
            if not ran and nxt_b2[r] < nxt_b1[r]:
                f = fs[nxt_b2[r]]
                rem_b2[f] -= dt
                if rem_b2[f] <= 1e-9:
                    done_b2[f] = t + dt
                    nxt_b2[r] += 1
        n_steps += 1
        t = n_steps * dt
    return t


def predicted_speedup(nframes, world, parts, reset_branch, t_a, t_b1, t_b2, t_handoff=0.0, t_cold=0.0, interleaved=True, exchange=None,
                      frame_num=5, steps_per_frame=2000.0, group=1, t_a_single=None):
    """(speedup over one rank, makespan) of run_wavefront for a partition (per-rank ranges or a block list) from per-frame
    phase times: simulate_wavefront against nframes * (t_a + t_b1 + t_b2) -- one rank walking the clip phase by phase at the same
    per-frame times (with group > 1: in full groups).  bench.py quotes the makespan against the N = 1 HEADLINE rate as well."""
    dt = max(1e-6, (t_a + t_b1 + t_b2) / steps_per_frame)
    span = simulate_wavefront(nframes, world, parts, reset_branch, t_a, t_b1, t_b2, t_handoff, t_cold, interleaved, dt, exchange, frame_num,
                              group, t_a_single)
    seq = nframes * (t_a + t_b1 + t_b2)
    return (seq / span if span > 0 else 0.0), span


def choose_partition(nframes, world, reset_branch, t_a, t_b1, t_b2, t_handoff=0.3, t_cold=None, exchange=None, frame_num=5, group=1,
                     t_a_single=None):
    """The partition run_wavefront should use for these phase times: the best of the reset-aligned hybrid (when the forward
    branch restarts), the balanced and the growing contiguous shards and the block-cyclic partitions with 1..8 frames per
    block, by simulated makespan.  t_cold defaults to 0.85 t_a (two more frames to prepare: ~5.0 of 5.8 ms for RefVSR_small
    at 270p).  exchange: see simulate_wavefront (the context exchange of run_wavefront).  Returns (block list, predicted speedup,
    name)."""
    if t_cold is None:
        t_cold = 0.85 * t_a
    cands = []
    if reset_branch:
        cands.append(('hybrid_reset_aligned', partition_hybrid(nframes, world, reset_branch)))
    cands.append(('balanced', partition(nframes, world)))
    if nframes >= world:
        cands.append(('growing_shards', partition_chain(nframes, world, t_b1 / t_a if t_a > 0 else 0.165)))
    for size in range(1, 9):
        if size * world < nframes:
            cands.append(('block_cyclic_%d' % size, partition_cyclic(nframes, world, size)))
    if nframes > world:
        # growing blocks: phase-A time of a window and of the chain's first step with / without the context exchange
        t_w = t_a if exchange is not None else t_a + 0.5 * t_cold
        t_0 = (t_a + exchange['t_prep']) if exchange is not None else t_a
        for sc in (0.8, 1.0, 1.2):
            cands.append(('block_cyclic_growing_%.1f' % sc, partition_cyclic_growing(nframes, world, t_w, t_b1 + 0.5 * t_handoff, t_0, sc)))
    # rank the candidates at a quarter of the time resolution, re-simulate the best three at the full one
    rough = []
    for name, parts in cands:
        sp, _ = predicted_speedup(nframes, world, parts, reset_branch, t_a, t_b1, t_b2, t_handoff, t_cold, True, exchange, frame_num, 500.0,
                                  group, t_a_single)
        rough.append((sp, name, parts))
    rough.sort(key=lambda v: -v[0])
    fine = []
    for _, name, parts in rough[:3]:
        sp, _ = predicted_speedup(nframes, world, parts, reset_branch, t_a, t_b1, t_b2, t_handoff, t_cold, True, exchange, frame_num,
                                  group=group, t_a_single=t_a_single)
        fine.append((as_blocks(parts), sp, name))
    top = max(v[1] for v in fine)
    # within 1 % of the best: the partition with the fewest blocks (fewest hand-offs and messages: the model's terms for those are
    # the assumed ones)
    return min((v for v in fine if v[1] >= 0.99 * top), key=lambda v: (len(v[0]), -v[1]))
