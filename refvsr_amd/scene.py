"""Pure planning for a video file with scene cuts (no torch, no numpy): where the cuts are, and what videorun runs between them.

The reference never meets a cut: its loader serves one folder per clip, replicates frames at the clip's edges
(data_loader/datasets.py:222-234) and starts every clip with is_first = True.  A file with cuts is therefore run as the reference
would run its scenes as separate clips: the windows are clamped at the cuts, no group of frames straddles one, and the group that
opens a scene is an is_first_frame call behind a Network.reset().

  * the detector: `scene_scores` (the widely used scene score on the sums of absolute luma differences of consecutive frames, which
    ops.luma_sad computes on the device and yuv.luma_sad models), `cuts_from_scores`, and `SceneDetector`, the same frame by frame;
  * the plan: `clips`, `plan_groups` (the whole file at once) and `GroupPlanner` (the same plan emitted group by group, as soon as
    the cuts up to the last frame of a group's windows are known) -- nothing else in videorun decides windows, groups or resets.

A cut is the index of a frame that starts a new scene, in (0, n); frame 0 always starts one and is never listed.
"""


def window_indices(f, nframes, t):
    """synth.window_indices (restated: this module imports nothing): the window centred on frame f, edge frames repeated."""
    return [min(max(f - t // 2 + k, 0), nframes - 1) for k in range(t)]


def check_threshold(threshold):
    """A scene-score threshold: a number in (0, 1]."""
    try:
        th = float(threshold)
    except (TypeError, ValueError):
        th = float('nan')
    if not 0.0 < th <= 1.0:
        raise ValueError('scene_cut must lie in (0, 1] (got %r)' % (threshold,))
    return th


def check_cuts(cuts, n=None):
    """A cut list as a tuple of ints: strictly increasing, every cut in (0, n) (n = None: positive)."""
    cuts = tuple(int(c) for c in cuts)
    for i, c in enumerate(cuts):
        if c <= 0 or (n is not None and c >= n):
            raise ValueError('cuts must lie in (0, %s) -- frame 0 always starts a scene (got %d)' % ('n' if n is None else n, c))
        if i and c <= cuts[i - 1]:
            raise ValueError('cuts must be strictly increasing (got %d behind %d)' % (c, cuts[i - 1]))
    return cuts


# ------------------------------------------------------------------------------------------------ detector
def mafd(sad, h, w, depth):
    """The mean absolute luma difference of a frame pair on the 8-bit scale (float64): sad / (h w 2^(depth - 8))."""
    return float(sad) / (float(h * w) * float(2 ** (depth - 8)))


def score_of(m, m_prev):
    """The scene score of a frame with mean difference m behind a frame with m_prev: clip(min(m, |m - m_prev|) / 100, 0, 1).  The
    second term keeps a run of steadily large differences (a pan) from firing on every frame: a cut scores high once."""
    return min(max(min(m, abs(m - m_prev)) / 100.0, 0.0), 1.0)


def scene_scores(sads, h, w, depth):
    """sads: the sums of absolute luma differences of frames 1, 2, ... against their predecessors (n - 1 integers for n frames).
    Returns the n scene scores, score[0] = 0 (mafd_0 = 0: frame 1 is scored against a still picture)."""
    scores, prev = [0.0], 0.0
    for s in sads:
        m = mafd(s, h, w, depth)
        scores.append(score_of(m, prev))
        prev = m
    return scores


def cuts_from_scores(scores, threshold):
    """The cuts of a file with these scores (scores[k]: frame k): every k >= 1 with scores[k] >= threshold."""
    th = check_threshold(threshold)
    return tuple(k for k, s in enumerate(scores) if k >= 1 and s >= th)


class SceneDetector(object):
    """scene_scores + cuts_from_scores frame by frame: push(sad) takes the SAD of the next frame (1, 2, ...) against its
    predecessor and says whether that frame starts a scene.  `scores` and `cuts` grow as the whole-file forms would give them."""

    def __init__(self, h, w, depth, threshold):
        self.h, self.w, self.depth, self.threshold = int(h), int(w), int(depth), check_threshold(threshold)
        self.scores, self.cuts, self._prev = [0.0], [], 0.0

    def push(self, sad):
        m = mafd(sad, self.h, self.w, self.depth)
        s = score_of(m, self._prev)
        self._prev = m
        k = len(self.scores)
        self.scores.append(s)
        if s >= self.threshold:
            self.cuts.append(k)
        return s >= self.threshold


# ------------------------------------------------------------------------------------------------ plan
def clips(n, cuts=()):
    """The scenes [s, e) of n frames with these cuts."""
    edges = (0,) + check_cuts(cuts, n) + (n,)
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def clip_groups(s, e, t, G):
    """The groups of one scene [s, e): (frames, windows, is_first) per G frames -- file-global frame ids, the windows those of the
    scene alone (window_indices inside it) offset by s; the first group opens the scene."""
    out = []
    for f0 in range(s, e, G):
        fs = list(range(f0, min(f0 + G, e)))
        out.append((fs, [[s + i for i in window_indices(f - s, e - s, t)] for f in fs], f0 == s))
    return out


def plan_groups(n, t, G, cuts=()):
    """What videorun runs: [(frames, windows, is_first)] over the scenes of the file, in order.  cuts = (): the plan of a file that is
    one clip -- groups of G frames from 0, windows clamped at the two ends of the file, is_first on the first group alone."""
    return [g for s, e in clips(n, cuts) for g in clip_groups(s, e, t, G)]


class GroupPlanner(object):
    """plan_groups, group by group.  push(is_cut) classifies the next frame (0, 1, ...; frame 0's answer is ignored: it always starts
    a scene); pop() returns the next group once `need()` frames are classified -- the frames up to the last one its windows can
    read, min(f0 + G + t // 2, n): exactly the frames the run has to have read for that group anyway -- and None before that or
    behind the last group (done()).
    n = None: the length is not known (a pipe).  need() is f0 + G + t // 2 and pop() returns a group as soon as that many frames are
    classified; finish() says that the frames pushed so far are all there are (n = known): pop() then drains the remaining groups and
    done() becomes true behind the last one.  The pops are those of plan_groups(n, t, G, cuts) either way."""

    def __init__(self, n, t, G):
        self.n, self.t, self.G = None if n is None else int(n), int(t), int(G)
        self.known = 0                     # frames classified so far
        self.cuts = []
        self._f0, self._s = 0, 0           # first frame of the next group, first frame of its scene

    def finish(self):
        if self.n is None:
            self.n = self.known

    def done(self):
        return self.n is not None and self._f0 >= self.n

    def need(self):
        return self._f0 + self.G + self.t // 2 if self.n is None else min(self._f0 + self.G + self.t // 2, self.n)

    def push(self, is_cut):
        if self.n is not None and self.known >= self.n:
            raise ValueError('GroupPlanner: all %d frames are classified' % self.n)
        if is_cut and self.known > 0:
            self.cuts.append(self.known)
        self.known += 1

    def pop(self):
        if self.done() or self.known < self.need():
            return None
        f0, s = self._f0, self._s
        # (a length not known yet lies beyond the known frames, as a scene's end there does)
        e = min([c for c in self.cuts if c > f0] + [self.known + 1 if self.n is None else self.n])      # the scene's end, if it lies inside the frames known
        hi = min(f0 + self.G, e)
        # a window reads frames below min(f + t // 2 + 1, e): an end beyond the known frames is beyond every window of the group, and
        # the clamp at any such end gives the same indices
        e_w = e if e <= self.known else max(self.known, hi)
        fs = list(range(f0, hi))
        wins = [[s + i for i in window_indices(f - s, e_w - s, self.t)] for f in fs]
        self._f0 = hi
        if hi == e:
            self._s = e
        return fs, wins, f0 == s
