"""The cases of tests/test_gpu_lattice_grids.py, checked on the CPU (no GPU needed).

* The oracle's two formulations (the reference's dense-covariance op sequence,
  O.*_faithful, and the diag-only Cholesky form the GPU tests compare with,
  O.*_diag) agree within PARITY_TOL / 10 at every cell of every case, base rows
  and all appended rows: the reference is well inside the tolerance on these
  grids before a kernel is judged by it.
* The grid builder against a NumPy restatement of the lattice detection's
  contract: the (nx, ny) the GPU tests expect from stats(), the cell strides,
  and the rows the device's cell lookup finds (uniform axes: every grid row;
  warped axes: only some; rows shifted along one coordinate: none).
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _lattice_grids as G


def _hyp(name):
    from mfgp_coverage_amd.synthetic import HYP
    return HYP[name].copy()


@pytest.mark.parametrize("hypname", ["australia3_sf", "australia8_mf"])
@pytest.mark.parametrize("case", G.ALL_CASES, ids=lambda c: c.name)
def test_oracle_formulations_agree(case, hypname):
    hyp = _hyp(hypname)
    mf = hyp.shape[0] == 9
    Xs, X, y, NL = case.data(mf)
    kss = O.prior_variance(hyp)
    worst = 0.0
    for lo in range(0, Xs.shape[0], 512):   # (the dense form holds [m, m] covariances: by blocks of cells)
        xs = Xs[lo:lo + 512]
        if mf:
            a = O.mf_faithful(X[:NL], y[:NL], X[NL:], y[NL:], hyp, xs)
            b = O.mf_diag(X[:NL], y[:NL], X[NL:], y[NL:], hyp, xs)
        else:
            a = O.sf_faithful(X, y, hyp, xs)
            b = O.sf_diag(X, y, hyp, xs)
        worst = max(worst, *O.parity_errors(b[0], b[1], a[0], a[1], kss))
    assert worst < O.PARITY_TOL / 10, worst


@pytest.mark.parametrize("case", G.ALL_CASES, ids=lambda c: c.name)
def test_case_grid_is_the_expected_lattice(case):
    Xs = case.grid()
    nx, ny, sx, sy = G.expected_lattice(Xs)
    assert (nx, ny) == (case.nx, case.ny)
    assert Xs.shape[0] == nx * ny
    if case.order == "x_outer":
        assert (sx, sy) == (ny, 1)
    else:
        assert (sx, sy) == (1, nx)
    # cell (ix, iy) sits at ix sx + iy sy
    gx, gy = G.axes_of(Xs)
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    c = ix * sx + iy * sy
    assert np.array_equal(np.sort(c.reshape(-1)), np.arange(nx * ny))
    assert np.array_equal(Xs[c, 0], gx[ix]) and np.array_equal(Xs[c, 1], gy[iy])
    assert gx.shape[0] == 1 or (gx[1] < gx[0]) == case.xrev
    assert gy.shape[0] == 1 or (gy[1] < gy[0]) == case.yrev


def test_expected_lattice_rejects_non_lattices():
    Xs = G.make_grid(G.axis(6), G.axis(5))
    assert G.expected_lattice(Xs) == (6, 5, 5, 1)
    assert G.expected_lattice(Xs[:-1]) == (0, 0, 0, 0)           # a ragged last row
    bent = Xs.copy()
    bent[7, 1] += 1e-3                                            # one cell off its axis value
    assert G.expected_lattice(bent) == (0, 0, 0, 0)
    flat = G.make_grid(np.array([0.0, 0.5, 0.5, 1.0]), G.axis(5))   # not strictly monotone
    assert G.expected_lattice(flat) == (0, 0, 0, 0)
    assert G.expected_lattice(Xs[np.random.default_rng(0).permutation(30)]) == (0, 0, 0, 0)


@pytest.mark.parametrize("mf", [False, True])
@pytest.mark.parametrize("case", G.ALL_CASES, ids=lambda c: c.name)
def test_case_rows(case, mf):
    """All rows come from one permutation (no append repeats a base row unless the
    case revisits), and the device's lookup finds the rows it should."""
    Xs, X, y, NL = case.data(mf)
    n = case.n0 + sum(G.KS)
    assert X.shape == (n, 2) and y.shape == (n,) and np.all(np.isfinite(y))
    rows = {tuple(r) for r in X}
    if case.kind == "cells":
        assert len(rows) == n
    else:
        assert n > Xs.shape[0] and len(rows) == Xs.shape[0]     # every cell, some twice
    on = G.on_lattice(Xs, X)
    cells = {tuple(r) for r in Xs}
    is_cell = np.array([tuple(r) in cells for r in X])
    assert not np.any(on & ~is_cell)
    if case.warp is None:
        assert np.array_equal(on, is_cell)       # uniform axes: the estimate is the index
    else:
        assert 0 < on.sum() < n                  # warped: some rows within one index, most not
    if case.shift is not None:
        moved = ~is_cell
        assert moved[3:9].all() and moved[case.n0 + 2:case.n0 + 6].all() and moved.sum() == 19
        other = 1 - case.shift
        g = G.axes_of(Xs)[other]
        assert np.isin(X[moved, other], g).all()                  # still an axis value the other way
        assert G.expected_virtual(Xs, X, NL, case.n0, mf) == 11 + (5 if mf else 0)


def test_greedy_variance_is_the_oracle():
    """The point-by-point form of the oracle's variance the planner test walks
    (G.GreedyVariance) against O.mf_diag rebuilt from scratch, on that test's grid,
    over a greedy argmax sequence with a revisited cell."""
    hyp = _hyp("australia8_mf")
    Xs = G.make_grid(G.axis(24), G.axis(70, -0.5, 0.7))
    X, y, _ = G.make_data(Xs, 158, 600)
    gv = G.GreedyVariance(hyp, X[:60], X[60:], Xs, room=41)
    kss = O.prior_variance(hyp)
    for i in range(41):
        ref = gv.from_scratch() if i % 20 == 0 else None
        if ref is not None:
            assert np.max(np.abs(gv.var - ref) / np.maximum(np.abs(ref), 1e-6 * kss)) < 1e-10, i
        gv.append(Xs[np.argmax(gv.var)] if i != 7 else X[100])
