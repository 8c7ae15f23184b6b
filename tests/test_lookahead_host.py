"""Look-ahead variance, host side (CPU; no GPU needed).

1. The yardstick of tests/test_gpu_lookahead.py -- O.mf_faithful on the stacked sets
   with zero values for the look-ahead covariance, O.mf_diag for the current mean and
   variance (tests/_lookahead.py) -- equals the outputs of the reference's own
   MFGP.pred_var / get_neg_var (tests/golden/lookahead_reference.npz, written by
   make_lookahead_golden.py) to 1e-9 in the floored-relative metric.
2. The fixed scenarios of the GPU tests keep the properties those tests rely on, on
   the oracle alone: the get_neg_var sample leaves at most 1 % of its points within
   the rounding band of the mask, and get_max_var's scenario ends on a local maximum
   for seeds 0-7 of the same scipy call.
3. Code-object budgets of k_look_border / k_look_query on the cross-compiled library:
   vgpr + agpr <= 256, LDS <= 80 KB, no scratch (two workgroups per CU, as declared).
"""
import os
import sys

import numpy as np
import pytest

from tests import _lookahead as LA
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_TOL = 1e-9


@pytest.fixture(scope="module")
def gold():
    with np.load(LA.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case,shape", [("a", (3, 5, 70)), ("b", (0, 1, 1)), ("c", (7, 0, 33))])
def test_oracle_composition_equals_reference_pred_var(gold, case, shape):
    g = {k[2:]: v for k, v in gold.items() if k.startswith(case + "_")}
    assert (g["XLn"].shape[0], g["XHn"].shape[0], g["x"].shape[0]) == shape
    assert (g["XL"].shape[0], g["XH"].shape[0]) == (60, 137)
    C = LA.oracle_look_cov("mf", g["XL"], g["XH"], gold["hyp"], g["XLn"], g["XHn"], g["x"])
    assert LA.floored_rel(C, g["pred_var"], gold["hyp"]) <= GOLD_TOL


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_oracle_neg_var_equals_reference_get_neg_var(gold, case):
    g = {k[2:]: v for k, v in gold.items() if k.startswith(case + "_")}
    masked = 0
    for (thrd, c), ref in zip(g["tc"], g["neg"]):
        val, margin = LA.oracle_neg_var("mf", g["XL"], g["yL"], g["XH"], g["yH"], gold["hyp"], g["XLn"], g["XHn"],
                                        g["xn"], thrd, c)
        # (the second threshold is the median of the reference's own mean + c var: one
        # point sits on it, where restatement and reference may round to either side)
        clear = np.abs(margin) > 1e-6 * O.prior_variance(gold["hyp"])
        assert np.count_nonzero(~clear) <= 1
        assert np.array_equal(val[clear] == 0, ref[clear] == 0)
        assert LA.floored_rel(val[clear], ref[clear], gold["hyp"]) <= GOLD_TOL
        masked += np.count_nonzero(ref == 0)
    assert 0 < masked < 40   # one pair masks part of the points


def test_neg_var_sample_stays_clear_of_the_mask_edge():
    s, X, thrd, c = LA.neg_var_sample()
    val, margin = LA.oracle_neg_var(s["kind"], s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], s["XLn"], s["XHn"], X,
                                    thrd, c)
    near = np.abs(margin) < 1e-6 * O.prior_variance(s["hyp"])
    assert np.count_nonzero(near) <= 0.01 * X.shape[0]
    assert 20 <= np.count_nonzero(val == 0) <= 180   # masked and unmasked points, both well represented


def test_max_var_scenario_ends_on_a_local_maximum_for_seeds_0_to_7():
    from scipy.optimize import differential_evolution
    s = LA.hole_scenario()
    thrd, c = LA.hole_threshold(s)
    probe, pval = LA.hole_probe(s, thrd, c)
    b = s["bounds"]

    def f(x):   # a generation [2, S], or the polish step's point [2]
        x = np.asarray(x, dtype=np.float64)
        v = LA.oracle_neg_var("mf", s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], s["XLn"], s["XHn"],
                              x[None, :] if x.ndim == 1 else x.T, thrd, c)[0]
        return v[0] if x.ndim == 1 else v
    assert 0.1 < np.mean(pval == 0) < 0.9   # the threshold masks part of the box
    for seed in range(8):
        np.random.seed(seed)
        r = differential_evolution(f, ([b[0][0], b[1][0]], [b[0][1], b[1][1]]), init="random", vectorized=True,
                                   updating="deferred")
        LA.check_local_max(r.x, -r.fun, probe, pval, b)


@pytest.fixture(scope="module")
def report():
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    # (every translation unit's kernels: the look-ahead kernels are not in the first)
    return check_codeobj.kernel_report(os.path.join(ROOT, "mfgp_coverage_amd", "libmfgp_hip.so"), all_units=True)


@pytest.mark.parametrize("kernel", ["k_look_border", "k_look_query"])
def test_look_kernels_fit_two_workgroups_per_cu(report, kernel):
    ks = {n: r for n, r in report.items() if kernel in n}
    assert len(ks) == 1, sorted(report)
    for n, r in ks.items():
        assert r["vgpr"] + r["agpr"] <= 256, (n, r)
        assert r["lds"] <= 80 * 1024, (n, r)
        assert r["scratch"] == 0, (n, r)
        assert r["calls"] == 0, (n, r)
