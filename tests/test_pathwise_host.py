"""Pathwise (Matheron) sampling, host side (CPU; no GPU needed).

1. mfgp_sample_axis_factor, the library's host routine (diagonally pivoted Cholesky of
   the unit-diagonal axis Gram, stopped at a largest remaining diagonal entry <= 2^-50):
   |A A^T - K|max <= 1e-12 -- the stop threshold (8.9e-16) plus rounding, with a wide
   margin; the remainder is positive semi-definite, so its largest entry lies on the
   diagonal -- the ranks, and its argument errors.
2. The formula itself in numpy (tests/_pathwise.py: pchol, the pathwise map, the basis
   trick): sum_i a_i a_i^T equals the oracle's dense posterior covariance
   (O.sf_faithful / O.mf_faithful) within O.PARITY_TOL in the floored-relative metric,
   and the zero-normal sample is the oracle's mean. Measured maxima over the cases
   below: covariance 2.2e-9, mean 1.4e-10 -- the GPU test's bound is reachable.
3. Code-object budgets of the new kernels on the cross-compiled library: no scratch,
   vgpr + agpr <= 256, no calls.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _pathwise as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfgp_coverage_amd import _lib
    return _lib


@pytest.mark.parametrize("l", [0.73, 0.268, 0.05, 0.01])
@pytest.mark.parametrize("n", [1, 13, 51, 128, 256])
def test_axis_factor(lib, n, l):
    a = np.linspace(0.0, 1.0, n)
    A, r = lib.sample_axis_factor(a, l)
    K = PW.axis_gram(a, l)
    assert A.shape == (n, r) and 1 <= r <= n
    e = float(np.max(np.abs(A @ A.T - K)))
    print(f"axis factor n = {n}, l = {l}: rank {r}, |A A^T - K|max = {e:.2e}")
    assert e <= 1e-12
    if l >= 0.268:
        assert r <= 25
    if l == 0.01 and n == 128:
        assert r == n
    # the numpy restatement meets the same bound (its rank may differ by the pivots that
    # rounding leaves just above or just below the stop threshold)
    B = PW.pchol(K)
    assert float(np.max(np.abs(B @ B.T - K))) <= 1e-12


def test_axis_factor_full_output_and_errors(lib):
    L = lib.lib()
    a = np.linspace(0.0, 1.0, 40)
    A = np.full((40, 40), 7.0)
    r = ctypes.c_int(-1)
    rc = L.mfgp_sample_axis_factor(ctypes.c_void_p(a.ctypes.data), 40, 0.73, ctypes.c_void_p(A.ctypes.data),
                                   ctypes.byref(r))
    assert rc == 0 and 1 <= r.value < 40
    assert np.all(A[:, r.value:] == 0.0)         # columns >= rank are zero
    assert np.array_equal(A[:, :r.value], lib.sample_axis_factor(a, 0.73)[0])
    ap, Ap = ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(A.ctypes.data)
    assert L.mfgp_sample_axis_factor(None, 40, 0.73, Ap, ctypes.byref(r)) == lib.ERR_ARG
    assert L.mfgp_sample_axis_factor(ap, 40, 0.73, None, ctypes.byref(r)) == lib.ERR_ARG
    assert L.mfgp_sample_axis_factor(ap, 40, 0.73, Ap, None) == lib.ERR_ARG
    assert L.mfgp_sample_axis_factor(ap, -1, 0.73, Ap, ctypes.byref(r)) == lib.ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="length scale"):
            lib.sample_axis_factor(a, bad)
    b = a.copy()
    b[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        lib.sample_axis_factor(b, 0.73)
    assert L.mfgp_sample_axis_factor(None, 0, 0.73, None, ctypes.byref(r)) == 0 and r.value == 0


def test_headline_ranks(lib):
    """HYP_MF's length scales (0.27 and 0.73) on 128 points: numerical ranks of about 19
    and 11, far below 128 -- a plain Cholesky fails on these Gram matrices."""
    a = np.linspace(0.0, 1.0, 128)
    r_h = lib.sample_axis_factor(a, np.exp(PW.HYP_MF[5]))[1]
    r_l = lib.sample_axis_factor(a, np.exp(PW.HYP_MF[2]))[1]
    print(f"headline ranks: l = {np.exp(PW.HYP_MF[5]):.3f}: {r_h}, l = {np.exp(PW.HYP_MF[2]):.3f}: {r_l}")
    assert 15 <= r_h <= 25 and 8 <= r_l <= 15
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(PW.axis_gram(a, 0.73))


HOST_CASES = [("sf", (13, 11), 0), ("mf", (13, 11), 1), ("mf", (13, 11), 129), ("sf", (17, 19), 257),
              ("mf", (17, 19), 257), ("mf", (8, 8), 65), ("sf", (5, 13), 64)]


@pytest.mark.parametrize("kind,shape,N", HOST_CASES)
def test_formula_in_numpy(kind, shape, N):
    c = PW.case(kind, shape, N)
    nz, _ = PW.dims(c)
    mu_r, cov_r = PW.oracle_mean_cov(c)
    f0, C = PW.basis_cov(lambda Z: PW.pathwise(c, Z), nz)
    e_cov = PW.floored_rel(C, cov_r, c["hyp"])
    e_mu = O.parity_errors(f0, np.diag(cov_r), mu_r, np.diag(cov_r), O.prior_variance(c["hyp"]))[0]
    print(f"pathwise numpy {kind} {shape} N = {N}: nz = {nz}, cov {e_cov:.2e}, mu {e_mu:.2e}")
    assert e_cov <= O.PARITY_TOL and e_mu <= O.PARITY_TOL
    # the prior alone
    nzp, _ = PW.dims(c, prior=True)
    p0, P = PW.basis_cov(lambda Z: PW.pathwise(c, Z, prior=True), nzp)
    assert np.all(p0 == 0.0)
    assert PW.floored_rel(P, PW.prior_cov(c), c["hyp"]) <= O.PARITY_TOL


@pytest.fixture(scope="module")
def report(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    return check_codeobj.kernel_report(os.path.join(ROOT, "mfgp_coverage_amd", "libmfgp_hip.so"), all_units=True)


@pytest.mark.parametrize("kernel", ["k_sample_t", "k_sample_field", "k_sample_resid", "k_sample_solve",
                                    "k_sample_gemm"])
def test_sample_kernels_fit_their_budget(report, kernel):
    ks = {n: r for n, r in report.items() if kernel in n}
    assert len(ks) == 1, sorted(report)
    for n, r in ks.items():
        assert r["vgpr"] + r["agpr"] <= 256, (n, r)
        assert r["lds"] <= 80 * 1024, (n, r)
        assert r["scratch"] == 0, (n, r)
        assert r["calls"] == 0, (n, r)
