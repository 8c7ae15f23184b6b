"""The batched, quota-constrained greedy planner on the oracle alone,
and what the GPU tests rely on: the reference greedy agrees with the from-scratch closed
form, the fixtures on which two device runs' picks are compared have no near ties, the
ragged fixture's gains keep their distance from its min_gain, and the built library
exports the entry point.

The bound of the recurrence, 1e-9, is tests/test_plan_ivr_host.py's: a margin over the
reference's own drift, never over a device's result.
"""
import os

import numpy as np
import pytest

from tests import _ivr as I
from tests import _plan_ivr as P
from tests import _plan_ivr_batch as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIFT_BOUND = 1e-9


def _quota_cases():
    """(name, cand, group, quota, n_points, expected picks) on the 13 x 11 grid."""
    Xs = P.extra_grid("13x11")
    M = Xs.shape[0]
    quad = Q.quadrants(Xs)
    twice = np.concatenate((np.arange(M), [71]))              # cell 71 again, under another group
    g2 = np.concatenate((quad, [(quad[71] + 1) % 4]))
    return Xs, [("quota1", None, quad, None, 10, 4), ("quota2103", None, quad, [2, 1, 0, 3], 10, 6),
                ("listed_twice", twice, g2, None, 10, 4), ("only_twice", [71, 71], [0, 1], None, 10, 2),
                ("free", None, None, None, 10, 10)]


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("N", P.NS)
def test_quota_greedy_equals_the_from_scratch_closed_form(kind, N):
    """Every pick of the reference greedy saw the from-scratch scores (within the drift
    bound), is allowed, and is the maximum over the allowed positions within PARITY_TOL."""
    Xs, cases = _quota_cases()
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    _, X, y, NL = Q.case_data(kind, "13x11", N)
    C0 = I.dense_cov(kind, X, y, NL, Xs, hyp)
    for wname in ("ones", "mask"):
        w = P.weights(wname, M)
        for name, cand, group, quota, n, want in cases:
            cells, pos, gains, _, scores = Q.greedy_quota(C0, hyp, w, n, cand, group, quota)
            assert cells.shape[0] == want, (name, cells)
            for t in range(cells.shape[0]):
                ref = P.scratch_scores(kind, X, y, NL, Xs, hyp, w, cells[:t])
                assert P.score_err(scores[t], ref, hyp, w, M) <= DRIFT_BOUND, (name, t)
            eg, em, _ = Q.check_quota_run(kind, X, y, NL, Xs, hyp, w, cells, pos, gains, cand, group, quota)
            assert eg <= P.TOL and em <= P.TOL, (name, eg, em)
            if group is not None:
                counts = np.bincount(np.asarray(group)[pos], minlength=4)
                q = np.ones(4, dtype=np.int64) if quota is None else np.asarray(quota)
                assert np.all(counts <= q) and not Q.left_allowed(M, cand, group, quota, pos), name
            else:                                               # the unconstrained run is P.recurrence's
                c2, g2, _ = P.recurrence(C0, hyp, w, n)
                assert np.array_equal(cells, c2) and np.array_equal(gains, g2)


def test_a_cell_listed_twice_is_taken_once_for_each_group():
    """Two positions of one cell under two groups: both are taken, the first position first
    (equal scores: the first allowed position wins)."""
    Xs, cases = _quota_cases()
    _, cand, group, quota, n, _ = cases[3]
    for kind in P.KINDS:
        _, X, y, NL = Q.case_data(kind, "13x11", 65)
        hyp = I.hyp_of(kind)
        cells, pos, gains, _, _ = Q.greedy_quota(I.dense_cov(kind, X, y, NL, Xs, hyp), hyp, None, n, cand, group, quota)
        assert cells.tolist() == [71, 71] and pos.tolist() == [0, 1] and gains[1] < gains[0]


def test_the_checker_flags_a_pick_outside_its_quota():
    kind, Xs = "mf", P.extra_grid("13x11")
    hyp = I.hyp_of(kind)
    _, X, y, NL = Q.case_data(kind, "13x11", 65)
    quad = Q.quadrants(Xs)
    C0 = I.dense_cov(kind, X, y, NL, Xs, hyp)
    cells, pos, gains, _, _ = Q.greedy_quota(C0, hyp, None, 4, None, quad, None)
    bad_pos = pos.copy()
    bad_pos[3] = pos[0]                                       # group of pick 0 again: quota 1 is spent
    with pytest.raises(AssertionError):
        Q.check_quota_run(kind, X, y, NL, Xs, hyp, None, cells[[0, 1, 2, 0]], bad_pos, gains, None, quad, None)
    free, fpos, fg, _, _ = Q.greedy_quota(C0, hyp, None, 4)
    if len(set(quad[free].tolist())) < 4:                     # the free run is no answer under quota 1
        with pytest.raises(AssertionError):
            Q.check_quota_run(kind, X, y, NL, Xs, hyp, None, free, fpos, fg, None, quad, None)


@pytest.mark.parametrize("members,wname", Q.EXACT, ids=["mask", "ones"])
def test_precondition_no_near_ties_where_picks_are_compared(members, wname):
    """The condition of every GPU comparison of picks between two runs: at every pick the
    oracle's top two allowed scores (of different cells) differ by more than
    GAP max(top, floor). Also under refresh (the same scores) and for 8 picks from N = 60."""
    for member in members:
        cells, _, gains, gaps, _ = Q.oracle_run(member, wname, Q.NPICK)
        assert cells.shape[0] == Q.NPICK
        print(f"{member} {wname}: smallest gap {gaps.min():.3e}")
        assert gaps.min() > Q.GAP, (member, gaps.min())


def test_precondition_of_the_ragged_batch():
    """RAGGED's oracle runs under RAGGED_GAIN make RAGGED_COUNTS picks, no gain up to the
    stop (the first gain below included) is within RAGGED_MARGIN of RAGGED_GAIN, and the
    picks made have no near ties."""
    for member, want in zip(Q.RAGGED, Q.RAGGED_COUNTS):
        cells, _, gains, gaps, _ = Q.oracle_run(member, "ones", Q.RAGGED_PICKS)
        below = np.nonzero(gains < Q.RAGGED_GAIN)[0]
        n = int(below[0]) if below.size else Q.RAGGED_PICKS
        assert n == want, (member, gains)
        upto = gains[:min(n + 1, Q.RAGGED_PICKS)]
        assert np.all(np.abs(upto - Q.RAGGED_GAIN) > Q.RAGGED_MARGIN * Q.RAGGED_GAIN), (member, upto)
        assert gaps[:n + 1].min() > Q.GAP
        stopped = Q.oracle_run(member, "ones", Q.RAGGED_PICKS, min_gain=Q.RAGGED_GAIN)
        assert stopped[0].shape[0] == want and np.array_equal(stopped[0], cells[:want])
    assert len(set(Q.RAGGED_COUNTS)) == 3 and 0 in Q.RAGGED_COUNTS


def test_precondition_rows_crossing_64():
    for kind in P.KINDS:
        _, _, _, gaps, _ = Q.oracle_run((kind, "13x11", 60), "ones", 8)
        assert gaps.min() > Q.GAP, (kind, gaps.min())


def test_symmetric_prior_grids_tie_exactly():
    """Why members without rows are only ever compared with the oracle's maximum."""
    _, _, _, gaps, _ = Q.oracle_run(("sf", "13x11", 0), "ones", 4)
    assert gaps.min() <= Q.GAP


def test_library_exports_the_batched_planner():
    import __graft_entry__ as ge
    ge.build()
    from mfgp_coverage_amd import _lib
    assert "mfgp_batch_plan_ivr" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mfgp_batch_plan_ivr"][1]) == 17
    assert hasattr(_lib.lib(), "mfgp_batch_plan_ivr")
    data = open(_lib.LIB_PATH, "rb").read()
    for k in (b"k_ivr_pick_batch", b"k_plan_x_batch", b"k_cov_dot_batch", b"k_cov_psum_batch", b"k_kss_t_batch",
              b"k_kss_out_batch", b"k_cov_apply_batch", b"k_plan_scatter"):
        assert k in data, k
    hdr = open(os.path.join(ROOT, "include", "mfgp_hip.h")).read()
    assert "MFGP_PLAN_MAXGROUPS 64" in hdr


def test_per_member_arguments():
    from mfgp_coverage_amd._lib import _per_member
    assert _per_member(None, 3) is None
    assert _per_member([1, 2, 3], 3) == [[1, 2, 3]] * 3                      # one list of cells for all
    assert _per_member([[1], [2, 3], []], 3) == [[1], [2, 3], []]            # one per member
    rows = _per_member(np.arange(6).reshape(2, 3), 2)
    assert len(rows) == 2 and rows[1].tolist() == [3, 4, 5]
    assert len(_per_member(np.arange(4), 2)) == 2
    with pytest.raises(ValueError):
        _per_member([[1], [2]], 3)
    with pytest.raises(ValueError):
        _per_member(np.zeros((2, 3)), 3)
