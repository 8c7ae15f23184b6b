"""The mathematics of the covariance products and the greedy integrated-variance planner
(DESIGN.md section 21), on the oracle alone: no device involved.

The bound of the recurrence test, 1e-9, is a margin over the reference's own drift (the
rank-one recurrence in fp64 numpy against the from-scratch closed form), never over a
device's result; the device's gate is O.PARITY_TOL = 1e-6 (tests/test_gpu_plan_ivr.py).
"""
import numpy as np
import pytest

from tests import _ivr as I
from tests import _plan_ivr as P
from tests._lattice_grids import axis, make_grid

PICKS = 48
DRIFT_BOUND = 1e-9


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("gname", sorted(I.GRIDS))
@pytest.mark.parametrize("N", P.NS)
def test_recurrence_equals_the_from_scratch_closed_form(kind, gname, N):
    """48 greedy picks by the recurrence (revisited cells included), each pick's score vector
    against I.ivr_closed on the oracle with the picks stacked under the hifi rows, weights
    ones and `mask`. Measured maximum over all cases, in _ivr.err's metric: 6.1e-11 (SF 9x7,
    mask weights, N = 65, where one live cell is picked 48 times); every other case
    <= 3.5e-11. Every recurrence pick lies within PARITY_TOL max(best, floor) of the
    from-scratch maximum."""
    Xs = I.grid(gname)
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    X, y, NL = I.data(kind, Xs, N, seed=7 + N + len(gname) + len(kind))
    C0 = I.dense_cov(kind, X, y, NL, Xs, hyp)
    worst = {}
    for wname in ("ones", "mask"):
        w = P.weights(wname, M)
        cells, gains, scores = P.recurrence(C0, hyp, w, PICKS)
        fl = P.pick_floor(hyp, w, M)
        e = 0.0
        for t in range(PICKS):
            ref = P.scratch_scores(kind, X, y, NL, Xs, hyp, w, cells[:t])
            e = max(e, P.score_err(scores[t], ref, hyp, w, M))
            best = ref.max()
            assert ref[cells[t]] >= best - P.TOL * max(best, fl), (wname, t)
        worst[wname] = e
    print(f"recurrence {kind} {gname} N = {N}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert max(worst.values()) <= DRIFT_BOUND, worst


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("N", (0, 1, 65, 197))
def test_two_pass_product_equals_the_dense_product(kind, N):
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    X, y, NL = I.data(kind, Xs, N, seed=31 + N)
    C = I.dense_cov(kind, X, y, NL, Xs, hyp)
    rng = np.random.default_rng(32)
    x = np.stack([rng.standard_normal(M), np.eye(M)[77], I.weight_sets(M, 33)["mask"]], axis=1)
    got = P.cov_apply_from_v(kind, X, NL, Xs, hyp, x)
    e = P.apply_err(got.T, (C @ x).T, hyp, x.T)
    print(f"two-pass product {kind} N = {N}: {e:.3e}")
    assert e <= 1e-9


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", [(16, 40, "x_outer", False), (16, 40, "y_outer", False), (13, 11, "x_outer", True),
                                   (40, 16, "y_outer", True)])
def test_separable_prior_product_equals_the_dense_prior(kind, shape):
    nx, ny, order, rev = shape
    gx, gy = axis(nx, reverse=rev), axis(ny, -0.5, 0.7)
    Xs = make_grid(gx, gy, order)
    hyp = I.hyp_of(kind)
    rng = np.random.default_rng(nx + ny)
    # both sides are sums of M products bounded by k** |x_j|: each is within M eps k** sum|x| of
    # the exact value, the metric's floor is 1e-6 k** sum|x|, so the two differ by at most
    # 2 M eps / 1e-6 in the metric (M = 640: 2.8e-7, M = 143: 6.4e-8). The bound is a tenth of
    # that worst case: rounding errors do not all align (measured: 6.1e-12 at M = 640).
    bound = 0.1 * 2 * nx * ny * np.finfo(np.float64).eps / 1e-6
    for x in (rng.standard_normal(nx * ny), np.eye(nx * ny)[nx + 3]):
        ref = I.prior_cov(kind, Xs, hyp) @ x
        got = P.kss_separable(kind, gx, gy, order, hyp, x)
        assert P.apply_err(got, ref, hyp, x) <= bound


def test_the_run_checker_flags_a_wrong_pick_and_a_wrong_gain():
    """check_run itself: a run that is right passes, a swapped pick or a perturbed gain fails."""
    kind, Xs = "mf", I.grid("9x7")
    hyp = I.hyp_of(kind)
    X, y, NL = I.data(kind, Xs, 65, seed=41)
    w = None
    cells, gains, _ = P.recurrence(I.dense_cov(kind, X, y, NL, Xs, hyp), hyp, w, 6)
    eg, em, _ = P.check_run(kind, X, y, NL, Xs, hyp, w, cells, gains)
    assert eg <= P.TOL and em <= P.TOL
    bad = cells.copy()
    bad[3] = (bad[3] + 17) % Xs.shape[0]
    assert P.check_run(kind, X, y, NL, Xs, hyp, w, bad, gains)[1] > P.TOL
    g2 = gains.copy()
    g2[2] *= 1.0 + 1e-4
    assert P.check_run(kind, X, y, NL, Xs, hyp, w, cells, g2)[0] > P.TOL
