"""Integrated variance reduction, host side (CPU; no GPU needed).

1. The yardstick of tests/test_gpu_ivr.py (tests/_ivr.py: the closed form on the oracle's
   dense covariance) equals the append form -- the weighted fall of the diagonal when the
   candidate joins the hifi rows -- on the oracle alone, to 1e-9 in the floored-relative
   metric (measured: <= 2.5e-12), and the metric's floor stays far below the smallest
   score, so it hides no error.
2. Code-object budgets of k_ivr_partial / k_ivr_finish / k_ivr_best on the cross-compiled
   library: call-free, no scratch, vgpr + agpr <= 256 and LDS <= 80 KB (two workgroups of
   256 threads per CU, the occupancy DESIGN.md section 20 states for k_ivr_partial).
"""
import os
import sys

import numpy as np
import pytest

from tests import _ivr as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_TOL = 1e-9


@pytest.mark.parametrize("kind", ["sf", "mf"])
@pytest.mark.parametrize("gname,N", [("9x7", 65), ("13x11", 129), ("24x24", 197)])
def test_closed_form_equals_append_form(kind, gname, N):
    Xs = I.grid(gname)
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    X, y, NL = I.data(kind, Xs, N, seed=3 + N)
    rng = np.random.default_rng(N)
    cand = np.unique(np.concatenate(([0, M - 1], rng.integers(0, M, 6))))
    ws = I.weight_sets(M, seed=N)
    w = np.vstack((np.ones((1, M)), ws["w3"][:2]))
    C = I.dense_cov(kind, X, y, NL, Xs, hyp)
    closed = I.ivr_closed(C, hyp, w, cand)
    appended = I.ivr_append(kind, X, y, NL, Xs, hyp, cand, w)
    e = I.err(closed, appended, hyp, w, M)
    # ones and the positive weights (rows 0, 1): every score an order above the floor, so the
    # metric is a relative one there; under the region mask (row 2) candidates far from the
    # region score next to nothing and the floor is what bounds them, as it does for variances
    margin = float(np.min((np.abs(appended) / I.floor(hyp, w, M))[:2]))
    print(f"ivr forms {kind} {gname} N = {N}: error {e:.3e}, smallest score / floor {margin:.1f}")
    assert e <= FORM_TOL
    assert margin >= 10.0


def test_prior_score_without_rows():
    """No training rows: the score of the prior covariance, finite and positive."""
    Xs = I.grid("9x7")
    hyp = I.hyp_of("mf")
    C = I.dense_cov("mf", np.empty((0, 2)), np.empty(0), 0, Xs, hyp)
    s = I.ivr_closed(C, hyp)
    assert s.shape == (1, 63) and np.all(np.isfinite(s)) and np.all(s > 0)
    a = I.ivr_append("mf", np.empty((0, 2)), np.empty(0), 0, Xs, hyp, [0, 31, 62])
    assert I.err(s[:, [0, 31, 62]], a, hyp, None, 63) <= FORM_TOL


@pytest.fixture(scope="module")
def report():
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    return check_codeobj.kernel_report(os.path.join(ROOT, "mfgp_coverage_amd", "libmfgp_hip.so"), all_units=True)


@pytest.mark.parametrize("kernel", ["k_ivr_partial", "k_ivr_finish", "k_ivr_best"])
def test_ivr_kernels_are_call_free_and_fit_two_workgroups_per_cu(report, kernel):
    ks = {n: r for n, r in report.items() if kernel in n}
    assert len(ks) == 1, sorted(report)
    for n, r in ks.items():
        assert r["calls"] == 0, (n, r)
        assert r["scratch"] == 0, (n, r)
        assert r["vgpr"] + r["agpr"] <= 256, (n, r)
        assert r["lds"] <= 80 * 1024, (n, r)
