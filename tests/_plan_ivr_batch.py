"""The shared reference of the batched, quota-constrained greedy planner's tests
(tests/test_plan_ivr_batch_host.py, tests/test_gpu_plan_ivr_batch.py),
in numpy on the oracle's dense covariance; built on tests/_plan_ivr.py and tests/_ivr.py.

A candidate list is a sequence of positions; position j holds cell cand[j] and belongs to
group[j]. At a pick, position j is allowed iff the run has made fewer than quota[group[j]]
picks in that group so far; the pick is the first allowed position of maximal score. The
scores are _plan_ivr's: S(c) / (diag C(c) + sigma_H + jitter) after the rank-one updates of
the picks before.

Picks of two device runs are compared only on fixtures whose oracle scores are not tied:
gap_of() is the relative distance between the best allowed score and the best allowed score
of another cell, and GAP is what it has to exceed at every pick (test_plan_ivr_batch_host.py
asserts it for every fixture listed in EXACT and RAGGED below). Symmetric grids with N = 0
tie exactly and are only ever compared with the oracle's maximum.
"""
import numpy as np

from tests import _ivr as I
from tests import _plan_ivr as P

GAP = 1e-6          # relative to max(top score, the metric's floor)
NPICK = 40          # crosses the 32-iteration chunk

# (kind, grid, N): the members of the GPU tests' batches. Data: _plan_ivr's seeds per case.
MEMBERS8 = (("mf", "13x11", 65), ("sf", "9x7", 197), ("mf", "40x33", 197), ("sf", "13x11", 0),
            ("mf", "9x7", 0), ("sf", "16x40_yo", 65), ("mf", "scatter150", 65), ("sf", "13x11", 197))
MEMBERS3 = MEMBERS8[:3]
# the fixtures on which the picks of two runs are compared cell for cell: (members, weights)
EXACT = ((MEMBERS3, "mask"), (MEMBERS3, "ones"))
# three members (weights ones) whose gains cross RAGGED_GAIN at different picks, one before
# its first: the oracle's runs make RAGGED_COUNTS picks, and none of their gains up to the
# stop lies within RAGGED_MARGIN (relative) of RAGGED_GAIN (test_plan_ivr_batch_host.py)
RAGGED = (("mf", "13x11", 65), ("sf", "13x11", 65), ("sf", "9x7", 197))
RAGGED_PICKS = 12
RAGGED_GAIN = 0.02
RAGGED_COUNTS = (9, 2, 0)
RAGGED_MARGIN = 1e-2


def case_data(kind, gname, N):
    """(Xs, X, y, NL) of a member: the grid and the rows tests/test_gpu_plan_ivr.py uses."""
    Xs = P.extra_grid(gname)
    X, y, NL = I.data(kind, Xs, N, seed=7 + N + len(gname) + len(kind))
    return Xs, X, y, NL


def quadrants(Xs):
    """[M] the quadrant 0..3 of every cell about the grid's midpoint."""
    mid = 0.5 * (Xs.min(0) + Xs.max(0))
    return (2 * (Xs[:, 0] > mid[0]) + (Xs[:, 1] > mid[1])).astype(np.int64)


def _lists(M, cand, group, quota):
    cand = np.arange(M) if cand is None else np.asarray(cand, dtype=np.int64)
    if group is None:
        return cand, None, None
    group = np.asarray(group, dtype=np.int64)
    assert group.shape == cand.shape
    quota = np.ones(int(group.max()) + 1, dtype=np.int64) if quota is None else np.asarray(quota, dtype=np.int64)
    return cand, group, quota


def allowed(cand, group, quota, counts):
    """The mask over the positions allowed now."""
    if group is None:
        return np.ones(cand.shape[0], dtype=bool)
    return counts[group] < quota[group]


def gap_of(sc_pos, cand, ok, fl):
    """The relative distance between the best allowed score and the best allowed score of
    another cell (inf: no other cell is allowed)."""
    j = int(np.argmax(np.where(ok, sc_pos, -np.inf)))
    other = ok & (cand != cand[j])
    if not other.any():
        return np.inf
    return float((sc_pos[j] - sc_pos[other].max()) / max(sc_pos[j], fl))


def greedy_quota(C0, hyp, w, n_points, cand=None, group=None, quota=None, min_gain=-np.inf):
    """The quota-constrained greedy by the rank-one recurrence on the dense covariance C0
    (P.recurrence with the allowed set recomputed per pick) -> (cells, pos, gains, gaps,
    scores): gaps[t] is gap_of at pick t, scores[t] the [M] score vector pick t saw."""
    M = C0.shape[0]
    wv = P.wvec(w, M)
    cand, group, quota = _lists(M, cand, group, quota)
    counts = None if group is None else np.zeros(quota.shape[0], dtype=np.int64)
    fl = P.pick_floor(hyp, w, M)
    nz = P.noise_of(hyp)
    C = C0.copy()
    S = (wv[:, None] * C ** 2).sum(0)
    cells, pos, gains, gaps, scores = [], [], [], [], []
    for _ in range(n_points):
        var = np.diag(C)
        sc = S / (var + nz)
        ok = allowed(cand, group, quota, counts)
        if not ok.any():
            break
        sp = sc[cand]
        j = int(np.argmax(np.where(ok, sp, -np.inf)))      # the first allowed position of the maximum
        if not sp[j] >= min_gain:
            break
        c = int(cand[j])
        gaps.append(gap_of(sp, cand, ok, fl))
        cells.append(c)
        pos.append(j)
        gains.append(sp[j])
        scores.append(sc)
        if group is not None:
            counts[group[j]] += 1
        g = C[:, c] / np.sqrt(var[c] + nz)
        C = C - np.outer(g, g)
        x = wv * g
        tau = wv @ (g * g)
        u = C @ x
        S = S - 2.0 * g * u - g * g * tau
    return (np.asarray(cells, dtype=np.int64), np.asarray(pos, dtype=np.int64), np.asarray(gains), np.asarray(gaps),
            scores)


def check_quota_run(kind, X, y, NL, Xs, hyp, w, cells, pos, gains, cand=None, group=None, quota=None):
    """A device run against the from-scratch scores given its own picks -> (worst gain error,
    worst shortfall from the maximum over the positions allowed at the pick, both in units of
    max(|ref|, floor), the gaps per pick). Asserts what is exact: pos indexes the list,
    cells == cand[pos], and every chosen position was allowed when it was chosen."""
    M = Xs.shape[0]
    cand, group, quota = _lists(M, cand, group, quota)
    counts = None if group is None else np.zeros(quota.shape[0], dtype=np.int64)
    fl = P.pick_floor(hyp, w, M)
    cells, pos = np.asarray(cells), np.asarray(pos)
    assert cells.shape == pos.shape == np.asarray(gains).shape
    assert np.all((pos >= 0) & (pos < cand.shape[0])) and np.array_equal(cells, cand[pos])
    e_gain = e_max = 0.0
    gaps = []
    for t, c in enumerate(cells):
        ref = P.scratch_scores(kind, X, y, NL, Xs, hyp, w, cells[:t])
        ok = allowed(cand, group, quota, counts)
        assert ok[pos[t]], (t, int(pos[t]))
        e_gain = max(e_gain, abs(gains[t] - ref[c]) / max(abs(ref[c]), fl))
        best = ref[cand[ok]].max()
        e_max = max(e_max, (best - ref[c]) / max(best, fl))
        gaps.append(gap_of(ref[cand], cand, ok, fl))
        if group is not None:
            counts[group[pos[t]]] += 1
    return e_gain, e_max, np.asarray(gaps)


def left_allowed(M, cand, group, quota, pos):
    """Whether any position is still allowed after the picks at `pos`."""
    cand, group, quota = _lists(M, cand, group, quota)
    if group is None:
        return cand.shape[0] > 0
    counts = np.bincount(group[np.asarray(pos, dtype=np.int64)], minlength=quota.shape[0])
    return bool(allowed(cand, group, quota, counts).any())


def oracle_run(member, wname, n_points, **kw):
    """greedy_quota on a member's oracle covariance."""
    kind, gname, N = member
    Xs, X, y, NL = case_data(kind, gname, N)
    hyp = I.hyp_of(kind)
    C0 = I.dense_cov(kind, X, y, NL, Xs, hyp)
    return greedy_quota(C0, hyp, P.weights(wname, Xs.shape[0]), n_points, **kw)
