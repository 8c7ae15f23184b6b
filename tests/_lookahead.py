"""Shared pieces of the look-ahead tests (test_lookahead_host.py, test_gpu_lookahead.py):
the oracle composition both use as the yardstick, and the fixed scenarios.

The oracle's look-ahead covariance is the reference's own computation restated by
oracle/gp_oracle.py: O.mf_faithful / O.sf_faithful on the stacked sets (training rows
plus prospective rows, zero values: pred_var ignores y, gp:440-481) with
return_cov=True; the current model's mean and variance are O.mf_diag / O.sf_diag.
test_lookahead_host.py pins this composition to outputs of the reference itself
(tests/golden/lookahead_reference.npz).
"""
import os

import numpy as np

from oracle import gp_oracle as O

HYP_SF = np.array([0.001, -2.368468757, -1.353149618, -4.596652374])        # tests/test_gpu_cov_block.py
HYP_MF = np.array([-1.700903132, -1.947362545, -0.309197345, -14.9598621, -3.655273338,
                   -1.317607182, -0.721748367, -5.926942955, -1.371689752])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookahead_reference.npz")
E2 = np.empty((0, 2))


def field(X, rng):
    c = rng.random((3, 2))
    f = sum(np.exp(-np.sum((X - ci) ** 2, 1) / 0.05) for ci in c)
    return f / f.max() + 0.1 * rng.standard_normal(X.shape[0])


def oracle_current(kind, XL, yL, XH, yH, hyp, x):
    """(mean, variance) of the current model at x."""
    if kind == "sf":
        return O.sf_diag(XH, yH, hyp, x)
    return O.mf_diag(XL, yL, XH, yH, hyp, x)


def oracle_look_cov(kind, XL, XH, hyp, XLn, XHn, x):
    """The dense look-ahead covariance at x: the reference's predict covariance of the
    stacked sets with zero values."""
    XLs, XHs = np.vstack((XL, XLn)), np.vstack((XH, XHn))
    if kind == "sf":
        return O.sf_faithful(XHs, np.zeros(XHs.shape[0]), hyp, x, return_cov=True)[1]
    return O.mf_faithful(XLs, np.zeros(XLs.shape[0]), XHs, np.zeros(XHs.shape[0]), hyp, x, return_cov=True)[1]


def oracle_neg_var(kind, XL, yL, XH, yH, hyp, XLn, XHn, x, thrd, c):
    """get_neg_var (gp:555-563) at every row of x -> ([n] values, [n] margins
    mean + c var_old - thrd)."""
    mean, var_old = oracle_current(kind, XL, yL, XH, yH, hyp, x)
    var = np.diag(oracle_look_cov(kind, XL, XH, hyp, XLn, XHn, x))
    margin = mean + c * var_old - thrd
    return np.where(margin <= 0, 0.0, -var), margin


def floored_rel(a, ref, hyp):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref), 1e-6 * O.prior_variance(hyp))))


def scenario(kind, N, PL, PH, Q, seed):
    """Training rows (NL ~ N / 3 for MF), prospective rows and query points in the unit
    square. Where the counts allow: prospective point 0 (of the hifi ones, or of the lofi
    ones without any) equals a training row, the last doubles the second, query 0 equals
    a prospective point, the last query lies far outside the data."""
    rng = np.random.default_rng(seed)
    NL = 0 if kind == "sf" else N // 3
    X = rng.random((N, 2))
    y = field(X, rng) if N else np.empty(0)
    XLn, XHn = rng.random((PL, 2)), rng.random((PH, 2))
    P = PL + PH
    Pn = XHn if PH else XLn
    if P and N:
        Pn[0] = X[N - 1]
    if Pn.shape[0] > 2:
        Pn[-1] = Pn[1]
    x = rng.random((Q, 2))
    if P and Q > 2:
        x[0] = Pn[min(1, Pn.shape[0] - 1)]
    if Q > 1:
        x[-1] = (7.5, -6.0)
    return dict(kind=kind, hyp=HYP_SF if kind == "sf" else HYP_MF, XL=X[:NL], yL=y[:NL], XH=X[NL:], yH=y[NL:],
                XLn=XLn, XHn=XHn, x=x)


def hole_scenario():
    """get_max_var: hifi data on a jittered lattice with a hole around (0.62, 0.4), lofi
    data everywhere; the box around the hole; two prospective hifi points at its rim."""
    rng = np.random.default_rng(11)
    g = np.linspace(0.0, 1.0, 12)
    XH = np.array([(a, b) for a in g for b in g]) + 0.01 * rng.standard_normal((144, 2))
    XH = XH[np.hypot(XH[:, 0] - 0.62, XH[:, 1] - 0.4) > 0.2]
    gl = np.linspace(0.0, 1.0, 7)
    XL = np.array([(a, b) for a in gl for b in gl])
    f = lambda X: np.exp(-((X[:, 0] - 0.62) ** 2 + (X[:, 1] - 0.4) ** 2) / 0.08)   # noqa: E731
    yL, yH = 0.8 * f(XL), f(XH)
    bounds = np.array([[0.42, 0.2], [0.82, 0.6]])   # [[x_lo, y_lo], [x_hi, y_hi]] as gp:576 reads it
    XHn = np.array([[0.5, 0.3], [0.74, 0.52]])
    return dict(kind="mf", hyp=HYP_MF, XL=XL, yL=yL, XH=XH, yH=yH, XLn=E2, XHn=XHn, bounds=bounds)


def hole_probe(s, thrd, c, n=61):
    """The oracle's get_neg_var on an n x n probe of the scenario's box -> (points, values)."""
    b = s["bounds"]
    gx, gy = np.linspace(b[0][0], b[1][0], n), np.linspace(b[0][1], b[1][1], n)
    probe = np.array([(a, bb) for a in gx for bb in gy])
    val, _ = oracle_neg_var(s["kind"], s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], s["XLn"], s["XHn"], probe, thrd, c)
    return probe, val


def check_local_max(x, value, probe, pval, bounds=None):
    """get_max_var's result (x, value) against the oracle's probe: x unmasked territory's
    local maximum -- no unmasked probe point within 0.05 of x exceeds value by more than
    1e-6 relative."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if bounds is not None:
        assert np.all(x >= np.asarray(bounds[0]) - 1e-12) and np.all(x <= np.asarray(bounds[1]) + 1e-12), (x, bounds)
    assert value > 0, (x, value)   # (a masked point returns 0)
    near = (np.hypot(probe[:, 0] - x[0], probe[:, 1] - x[1]) < 0.05) & (pval < 0)
    assert np.any(near), x
    assert np.max(-pval[near]) <= value * (1 + 1e-6), (x, value, float(np.max(-pval[near])))


def hole_threshold(s):
    """(Thrd, c) of the get_max_var scenario: mean + c var_old over the box spans about
    0.42 .. 0.56 (61 x 61 probe of the oracle), 0.554 at the look-ahead variance's peak
    near (0.627, 0.413): this threshold masks about half of the box and leaves the peak."""
    return 0.49, 10.0


def neg_var_sample():
    """get_neg_var's sample: the N = 197 MF scenario with 3 + 5 prospective points, 200
    fixed points, and a threshold near the median of mean + c var_old over them."""
    s = scenario("mf", 197, 3, 5, 4, seed=23)
    X = np.random.default_rng(29).random((200, 2))
    return s, X, NEG_THRD, 4.0


NEG_THRD = 0.147   # (the oracle's median is 0.1475; the nearest point of the sample lies 2.7e-4 away)
