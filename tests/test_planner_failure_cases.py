"""The failing planner cases of tests/_planner_cases.py, proven on the CPU oracle
alone (no GPU): each fails where the GPU tests (test_gpu_planner_failures.py) rely
on it failing, with a margin that rounding cannot cross.

Margins: a pivot is vmax - d * kss, compared against 1e-3 * kss = a thousand
PARITY_TOLs (the device's variances agree with the oracle's to PARITY_TOL * kss at
worst), so rounding cannot move the failing step along one path of chosen cells.
Near ties between cells can change the path: the tie-break tests below replay the
loop with other choices and show what the GPU tests may assert about the step (the
exact one for A and C, the second chunk short of its last iteration for B).
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _planner_cases as P

MARGIN = 1e-3   # of kss


def test_margin_is_a_thousand_parity_tolerances():
    assert MARGIN == 1000 * O.PARITY_TOL


@pytest.mark.parametrize("name,i_fail", [("A", 19), ("B", 52), ("C", 16)])
def test_case_fails_where_intended(name, i_fail):
    c = P.build(name)
    # the initial rows are positive definite under the negative jitter
    if c.kind == "sf":
        K = O.se_kernel(c.XH, c.XH, c.hyp[1], c.hyp[2]) + np.eye(c.XH.shape[0]) * (np.exp(c.hyp[-1]) + c.jitter)
    else:
        K = O.mf_K(c.XL, c.XH, c.hyp, c.jitter)
    np.linalg.cholesky(K)
    assert c.jitter < 0
    # the oracle's loop fails at the intended step, by a clear margin on both sides
    assert c.i_fail == i_fail
    assert c.pivots.shape[0] == i_fail + 1
    assert c.pivots[i_fail - 1] >= MARGIN * c.kss, c.pivots[i_fail - 1] / c.kss
    assert c.pivots[i_fail] <= -MARGIN * c.kss, c.pivots[i_fail] / c.kss
    assert (c.pivots[:i_fail] > 0).all()
    # the sizes stay small: a 24 x 24 grid, at most 120 rows, at most 200 iterations
    assert c.xs.shape == (24 * 24, 2)
    assert c.XL.shape[0] + c.XH.shape[0] + i_fail + 1 <= 120 and i_fail < P.MAX_ITERS


def test_case_b_fails_in_the_second_chunk():
    """The loops read the status once per 32 iterations: case B's failure cannot move
    into the first chunk (every pivot there is >= 1e-2 kss) and lies well inside the
    second (iterations 32 .. 63)."""
    c = P.build("B")
    assert (c.pivots[:33] >= 1e-2 * c.kss).all(), c.pivots[:33].min() / c.kss
    assert 32 < c.i_fail < 63


def _tie_breaks():
    """Other ways a device may break near ties: cells within PARITY_TOL (and 10 x
    that) of the maximum, the last of them or a random one."""
    out = []
    for tol in (O.PARITY_TOL, 10 * O.PARITY_TOL):
        out.append((tol, "last"))
        out += [(tol, np.random.default_rng(s)) for s in range(4)]
    return out


@pytest.mark.parametrize("name", ["A", "C"])
def test_failing_step_does_not_move_under_tie_breaks(name):
    """Cases A and C fail at the same step however near ties are broken: the GPU tests
    assert the exact row the error names for them."""
    c = P.build(name)
    for tie in _tie_breaks():
        _, vmaxs, i_fail = P.oracle_loop(c, 0.0, tie=tie)
        assert i_fail == c.i_fail, (tie[0], i_fail)
        piv = vmaxs - c.d * c.kss
        assert piv[i_fail - 1] >= MARGIN * c.kss and piv[i_fail] <= -MARGIN * c.kss


def test_case_b_stays_inside_the_second_chunk_under_tie_breaks():
    """Case B has near ties from its first step on (top-two gap below PARITY_TOL * kss),
    and its failing step moves with the tie-break (48 .. 53 here). It stays in the
    second chunk and before that chunk's last iteration (32 <= i_fail <= 62), which is
    all the GPU tests assert for it: the named row is neither in the first chunk nor
    the chunk's last row (what a lost status word would report)."""
    c = P.build("B")
    _, var = c.oracle()
    top = np.sort(var)[-2:]
    assert top[1] - top[0] < O.PARITY_TOL * c.kss   # (the near tie is there)
    seen = set()
    for tie in _tie_breaks():
        _, vmaxs, i_fail = P.oracle_loop(c, 0.0, tie=tie)
        seen.add(i_fail)
        assert 40 <= i_fail <= 58, (tie[0], i_fail)   # well inside 32 .. 62
        assert ((vmaxs - c.d * c.kss)[:33] >= 1e-2 * c.kss).all()
    print("case B failing steps under tie-breaks:", sorted(seen))


def test_case_a_fails_mid_first_chunk():
    c = P.build("A")
    assert 1 < c.i_fail < 31   # other iterations of the same chunk follow the failing one


@pytest.mark.parametrize("name", ["A", "B", "C", "B2", "H0", "H1"])
def test_append_rows_stay_positive_definite(name):
    """The rows the GPU tests append after a failed loop: on the grid, none of them an
    existing row, and the step itself positive definite by a margin under the case's
    jitter (4 rows for the single-model tests, their first for the batch step)."""
    c = P.build(name)
    X, y = P.append_rows(c, 4)
    have = {tuple(r) for r in np.vstack([c.XL, c.XH])}
    assert len({tuple(r) for r in X}) == 4 and not have & {tuple(r) for r in X}
    assert all((c.xs == r).all(1).sum() == 1 for r in X)
    c.oracle(np.vstack([c.XH, X]), np.append(c.yH, y))   # (np.linalg.cholesky accepts it)
    if c.d > 0:
        assert (c.pivots[:4] >= 10 * MARGIN * c.kss).all(), c.pivots[:4] / c.kss


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_variance_stays_away_from_zero_after_the_checked_step(name):
    """The step the GPU tests compare with the oracle (the case's rows + append_rows'
    4): under the negative nugget the variance changes sign, and the fp32 metric is
    relative to |var_ref| with an absolute fp32-V error of ~2 * 2^-24 * kss = 1.2e-7 kss;
    F32_TOL = 1e-4 therefore needs |var_ref| >= 1.2e-3 kss on every cell. The cases
    keep 1e-2 kss (8 times that)."""
    c = P.build(name)
    X, y = P.append_rows(c, 4)
    _, var = c.oracle(np.vstack([c.XH, X]), np.append(c.yH, y))
    assert (var < 0).any()   # (the sign change is there)
    assert np.abs(var).min() >= 1e-2 * c.kss, np.abs(var).min() / c.kss
    assert 2 * 2.0 ** -24 / 1e-2 < O.F32_TOL / 8


def test_healthy_second_chunk_member_runs_past_one_chunk():
    """Case (d)'s healthy member (B2, threshold 0.3 x its initial max variance) reaches
    its threshold after more than 32 points, so it is still live when B fails."""
    c = P.build("B2")
    _, var = c.oracle()
    pts, _, i_fail = P.oracle_loop(c, 0.3 * float(var.max()))
    assert i_fail == -1 and 32 < pts.shape[0] < P.MAX_ITERS, pts.shape
    assert pts.shape[0] > P.build("B").i_fail   # ... and past B's failing step


def test_cap_case_visits_every_free_cell_first():
    """The point-cap case (6 x 6 grid, 5 rows on cells, threshold 0): 4 * 36 + 1 = 145
    points revisit every cell several times. Its first 31 points are the 31 cells that
    hold no row, each once -- until then a free cell's variance exceeds every taken
    cell's by more than 1e-3 kss, so rounding cannot change that on the device (the
    32nd point is the first revisit)."""
    c = P.build("CAP")
    pts, _, i_fail = P.oracle_loop(c, 0.0, 145)
    assert i_fail == -1 and pts.shape == (145, 2)
    free = {tuple(r) for r in c.xs} - {tuple(r) for r in c.XH}
    assert len(free) == 31 and {tuple(p) for p in pts[:31]} == free
    assert tuple(pts[31]) in {tuple(p) for p in pts[:31]} | {tuple(r) for r in c.XH}
    XH, yH = c.XH.copy(), c.yH.copy()
    for k in range(31):
        mu, var = c.oracle(XH, yH)
        taken = np.array([tuple(r) in {tuple(q) for q in XH} for r in c.xs])
        assert var[~taken].max() - var[taken].max() >= MARGIN * c.kss, k
        j = int(np.argmax(var))
        assert not taken[j]
        XH, yH = np.vstack([XH, c.xs[j]]), np.append(yH, mu[j])
    cnt = np.array([(pts == r).all(1).sum() for r in c.xs])
    assert cnt.min() >= 2   # every cell is revisited
