"""Look-ahead variance and off-grid queries on the device (k_look_border, k_look_query,
mfgp_query) and the drop-in methods built on them: predict_at, MFGP.pred_var /
pred_var_diag / get_neg_var / get_max_var, SFGP.ExpectedImprovement.

The yardstick is the oracle composition of tests/_lookahead.py (the reference's own
predict covariance of the stacked sets; pinned to the reference's pred_var / get_neg_var
outputs by tests/test_lookahead_host.py), in the project's metrics (O.parity_errors for
mu / var0, the same floored-relative metric over every entry of var and cov), bound
O.PARITY_TOL. Measured maxima on an MI355X: mu 2.1e-11, var0 2.3e-13, var 2.8e-13,
cov 4.7e-10; against a real append (test 3) 3.6e-15.
"""
import copy

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _lookahead as LA

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL
LOOK_KEYS = ("look_border", "look_query")
PATH_COUNTERS = ("full_factor", "inc_factor", "full_predict", "vstream", "lattice", "lattice_arg", "lattice_g2",
                 "post_copy")


def _model(s, dtype=None, jitter=1e-8, hyp=None):
    from mfgp_coverage_amd import _lib
    m = _lib.Model(_lib.context(), _lib.SF if s["kind"] == "sf" else _lib.MF, s["hyp"] if hyp is None else hyp, jitter,
                   dtype=_lib.F64 if dtype is None else dtype)
    m.set_data(s["XL"], s["yL"], s["XH"], s["yH"])
    return m


def _errors(s, q, x=None, XLn=None, XHn=None):
    """(mu, var0, var, cov) errors of a QueryResult against the oracle."""
    x = s["x"] if x is None else x
    XLn = s["XLn"] if XLn is None else XLn
    XHn = s["XHn"] if XHn is None else XHn
    mu0, v0 = LA.oracle_current(s["kind"], s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], x)
    C = LA.oracle_look_cov(s["kind"], s["XL"], s["XH"], s["hyp"], XLn, XHn, x)
    e_mu, e_v0 = O.parity_errors(q.mu, q.var0, mu0, v0, O.prior_variance(s["hyp"]))
    return e_mu, e_v0, LA.floored_rel(q.var, np.diag(C), s["hyp"]), LA.floored_rel(q.cov, C, s["hyp"])


def _split(kind, P, lofi_only):
    """(P_L, P_H) of P prospective points: mixed fidelities, or lofi only (SF: its one)."""
    if kind == "sf":
        return 0, P
    return (P, 0) if lofi_only else (P // 3, P - P // 3)


# ---- 1. against the oracle ------------------------------------------------------

# every N over the block edges with one (P, Q); every P (mixed fidelities, and lofi only
# on MF: an SF model has one fidelity) and every Q at N = 197
_SHAPES = [(k, N, 8, False, 70) for k in ("sf", "mf") for N in (0, 1, 63, 64, 65, 127, 128, 129, 197, 257)]
_SHAPES += [(k, 197, P, False, 65) for k in ("sf", "mf") for P in (0, 1, 8, 63, 64)]
_SHAPES += [("mf", 197, P, True, 65) for P in (1, 8, 63, 64)]
_SHAPES += [(k, 197, 8, False, Q) for k in ("sf", "mf") for Q in (1, 63, 64, 65, 130)]


@pytest.mark.parametrize("kind,N,P,lofi_only,Q", _SHAPES)
def test_query_matches_the_oracle(kind, N, P, lofi_only, Q):
    PL, PH = _split(kind, P, lofi_only)
    s = LA.scenario(kind, N, PL, PH, Q, seed=1000 + N + 3 * P + Q)
    q = _model(s).query(s["x"], s["XLn"], s["XHn"], mu=True, var0=True, var=True, cov=True)
    e = _errors(s, q)
    print("errors mu %.2e var0 %.2e var %.2e cov %.2e" % e)
    assert max(e) <= TOL, e
    if P == 0:
        assert np.array_equal(q.var, q.var0)


# ---- 2. position independence, bit for bit --------------------------------------

@pytest.mark.parametrize("kind", ["sf", "mf"])
def test_a_query_does_not_depend_on_its_place_or_its_batch(kind):
    s = LA.scenario(kind, 197, *_split(kind, 8, False), 130, seed=77)
    m = _model(s)
    want = dict(mu=True, var0=True, var=True)
    a = m.query(s["x"], s["XLn"], s["XHn"], **want)
    perm = np.random.default_rng(3).permutation(130)
    b = m.query(s["x"][perm], s["XLn"], s["XHn"], **want)
    for f in ("mu", "var0", "var"):
        assert np.array_equal(getattr(b, f), getattr(a, f)[perm]), f
    for i in (0, 5, 63, 64, 100, 129):
        c = m.query(s["x"][i:i + 1], s["XLn"], s["XHn"], **want)
        for f in ("mu", "var0", "var"):
            assert getattr(c, f)[0] == getattr(a, f)[i], (f, i)


# ---- 3. against a real append ---------------------------------------------------

def _grid(nx, ny):
    gx, gy = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
    return np.array([(a, b) for a in gx for b in gy])


def _mfgp(s):
    from mfgp_coverage_amd.gaussian_process import MFGP
    mf = MFGP(s["XL"], s["yL"][:, None], s["XH"], s["yH"][:, None], 1, 1)
    mf.hyp = s["hyp"].copy()
    mf.updt_info(mf.X_L, mf.y_L, mf.X_H, mf.y_H)
    return mf


def test_pred_var_diag_equals_the_variance_after_a_real_append():
    s = LA.scenario("mf", 197, 0, 0, 1, seed=5)
    mf = _mfgp(s)
    Xs = _grid(13, 11)
    mu0, cov0 = mf.predict(Xs)
    mu0, var0 = np.array(mu0), np.array(np.diag(cov0))
    cells = [5, 17, 17, 40, 77, 5, 100, 142]   # (some revisited)
    Xn = Xs[cells]
    d = mf.pred_var_diag(Xs, [], Xn)
    cp = copy.deepcopy(mf)
    cp.updt_hifi(Xn, np.linspace(-1.0, 2.0, 8)[:, None])   # (arbitrary values: the variance ignores them)
    var1 = np.array(np.diag(cp.predict(Xs)[1]))
    e = LA.floored_rel(d, var1, s["hyp"])
    print("look-ahead against a real append: %.2e" % e)
    assert e <= TOL
    mu2, cov2 = mf.predict(Xs)
    assert np.array_equal(np.array(mu2), mu0) and np.array_equal(np.array(np.diag(cov2)), var0)


# ---- 4. non-mutation ------------------------------------------------------------

def _path(st):
    return {k: v for k, v in st.items() if k not in LOOK_KEYS}


def test_queries_leave_the_model_and_its_step_path_as_they_were():
    Xs = _grid(24, 24)
    rng = np.random.default_rng(8)
    idx = rng.choice(Xs.shape[0], 90, replace=False)
    X, y = Xs[idx[:80]], LA.field(Xs[idx[:80]], rng)
    s = dict(kind="mf", hyp=LA.HYP_MF, XL=X[:25], yL=y[:25], XH=X[25:], yH=y[25:])
    mf = _mfgp(s)
    m = mf._dev()
    mf.predict(Xs)
    steps = Xs[idx[80:]]

    def step(i):   # one hifi append and its predict: the path counters it moved
        st = m.stats()
        mf.updt_hifi(steps[i:i + 1], np.array([[0.3]]))
        mf.predict(Xs)
        return {k: m.stats()[k] - st[k] for k in PATH_COUNTERS}

    def pred():   # a predict of the unchanged model: its bits and the path counters it moved
        st = m.stats()
        mu, cov = mf.predict(Xs)
        return np.array(mu), np.array(np.diag(cov)), {k: m.stats()[k] - st[k] for k in PATH_COUNTERS}
    step(0)
    before = step(1)
    mu0, var0, pred_before = pred()
    st0, ser0 = m.stats(), m.serial()
    x = rng.random((70, 2))
    m.query(x, None, x[:3], mu=True, var0=True, var=True, cov=True)
    mf.pred_var(x, x[3:5], x[5:9])
    np.random.seed(0)
    mf.get_max_var(np.array([[0.3, 0.3], [0.6, 0.6]]), -1.0, 1.0, LA.E2, x[:2])
    st1 = m.stats()
    assert _path(st1) == _path(st0) and m.serial() == ser0
    assert st1["look_border"] > st0["look_border"] and st1["look_query"] > st0["look_query"]
    mu1, var1, pred_after = pred()
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0)
    assert pred_after == pred_before, (pred_before, pred_after)   # the same bits by the same path
    assert step(2) == before, (before, m.stats())


@pytest.mark.parametrize("kind", ["sf", "mf"])
def test_a_model_without_a_grid_answers_predict_at(kind):
    from mfgp_coverage_amd.gaussian_process import SFGP
    s = LA.scenario(kind, 129, 0, 0, 65, seed=31)
    if kind == "sf":
        gpm = SFGP(s["XH"], s["yH"][:, None], 1)
        gpm.hyp = s["hyp"].copy()
        gpm.updt_info(gpm.X, gpm.y)
    else:
        gpm = _mfgp(s)
    mu, var = gpm.predict_at(s["x"])
    assert mu.shape == (65, 1) and var.shape == (65,)
    mu0, v0 = LA.oracle_current(kind, s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], s["x"])
    assert max(O.parity_errors(mu[:, 0], var, mu0, v0, O.prior_variance(s["hyp"]))) <= TOL
    st = gpm._dev().stats()
    assert st["v_rows"] == 0 and st["full_predict"] == 0 and st["look_query"] == 1


# ---- 5. border cache ------------------------------------------------------------

def test_the_border_is_kept_per_prospective_set_and_model_state():
    s = LA.scenario("mf", 129, 3, 5, 64, seed=41)
    m = _model(s)

    def counts():
        st = m.stats()
        return st["look_border"], st["look_query"]
    a = m.query(s["x"], s["XLn"], s["XHn"])
    b = m.query(s["x"], s["XLn"], s["XHn"])
    assert counts() == (1, 2)
    assert np.array_equal(a.var, b.var) and np.array_equal(a.mu, b.mu)
    m.query(s["x"], s["XLn"], s["XHn"][:4])            # another set
    assert counts() == (2, 3)
    m.query(s["x"], s["XHn"][:3], s["XHn"])            # the same bytes, other fidelities
    assert counts() == (3, 4)
    m.append(np.array([[0.25, 0.75]]), np.array([0.1]))   # the model moved on
    m.query(s["x"], s["XHn"][:3], s["XHn"])
    assert counts() == (4, 5)
    m.query(s["x"])                                     # no prospective points: no border
    assert counts() == (4, 6)


# ---- 6. errors ------------------------------------------------------------------

def test_argument_errors_are_raised_before_anything_runs():
    s = LA.scenario("mf", 65, 3, 5, 10, seed=51)
    m = _model(s)
    st0 = m.stats()
    P65 = np.random.default_rng(1).random((65, 2))
    with pytest.raises(ValueError):
        m.query(s["x"], P65[:30], P65[30:])
    with pytest.raises(ValueError):
        m.query(s["x"], s["XLn"], s["XHn"], cov=True, ldc=9)
    bad = s["x"].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        m.query(bad, s["XLn"], s["XHn"])
    ssf = LA.scenario("sf", 65, 0, 5, 10, seed=52)
    msf = _model(ssf)
    with pytest.raises(ValueError):
        msf.query(ssf["x"], ssf["XHn"][:1], ssf["XHn"])
    assert m.stats() == st0 and msf.stats()["look_query"] == 0


def test_a_border_that_is_not_positive_definite_raises_linalgerror():
    # Five rows far apart (K close to s I) factor with a slightly negative net diagonal
    # shift noise + jitter = -1e-4; a doubled prospective point far from them then gives
    # the 2 x 2 border [[s - 1e-4, s], [s, s - 1e-4]], whose second pivot is negative.
    hyp = LA.HYP_SF
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, 2.0]])
    s = dict(kind="sf", hyp=hyp, XL=LA.E2, yL=np.empty(0), XH=X, yH=np.linspace(0.0, 1.0, 5))
    m = _model(s, jitter=-(np.exp(hyp[3]) + 1e-4))
    x = np.array([[0.5, 0.5], [3.0, 3.0]])
    ok = m.query(x, None, np.array([[3.0, 3.0]]))
    assert np.all(np.isfinite(ok.var))
    with pytest.raises(np.linalg.LinAlgError):
        m.query(x, None, np.array([[3.0, 3.0], [3.0, 3.0]]))
    again = m.query(x, None, np.array([[3.0, 3.0]]))
    assert np.array_equal(again.var, ok.var) and np.array_equal(again.mu, ok.mu)
    m.set_grid(x)
    mu, var = m.predict()
    assert np.allclose(mu, ok.mu, rtol=1e-9, atol=0) and np.all(np.isfinite(var))


def test_an_f32_model_is_served_in_fp64():
    from mfgp_coverage_amd import _lib
    s = LA.scenario("mf", 197, 3, 5, 70, seed=61)
    q = _model(s, dtype=_lib.F32).query(s["x"], s["XLn"], s["XHn"], mu=True, var0=True, var=True, cov=True)
    assert max(_errors(s, q)) <= TOL


# ---- 7. get_neg_var / _neg_var_many ---------------------------------------------

def test_neg_var_matches_the_oracle_objective():
    s, X, thrd, c = LA.neg_var_sample()
    mf = _mfgp(s)
    ref, margin = LA.oracle_neg_var("mf", s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], s["XLn"], s["XHn"], X, thrd, c)
    clear = np.abs(margin) >= 1e-6 * O.prior_variance(s["hyp"])
    assert np.count_nonzero(~clear) <= 0.01 * X.shape[0]
    st0 = mf._dev().stats()
    val = mf._neg_var_many(X, thrd, c, s["XLn"], s["XHn"])
    assert mf._dev().stats()["look_query"] == st0["look_query"] + 1
    assert val.shape == (200,)
    assert np.array_equal(val[clear] == 0, ref[clear] == 0)
    assert 20 <= np.count_nonzero(val == 0) <= 180
    assert LA.floored_rel(val[clear], ref[clear], s["hyp"]) <= TOL
    i_masked, i_open = int(np.flatnonzero(val == 0)[0]), int(np.flatnonzero(val < 0)[0])
    assert mf.get_neg_var(X[i_masked], thrd, c, s["XLn"], s["XHn"]) == 0
    one = mf.get_neg_var(X[i_open], thrd, c, s["XLn"], s["XHn"])
    assert one.shape == (1, 1) and one[0, 0] == val[i_open]


# ---- 8. get_max_var -------------------------------------------------------------

def test_get_max_var_finds_a_local_maximum_with_one_launch_per_generation(monkeypatch):
    import scipy.optimize
    s = LA.hole_scenario()
    thrd, c = LA.hole_threshold(s)
    probe, pval = LA.hole_probe(s, thrd, c)
    mf = _mfgp(s)
    m = mf._dev()
    seen, sizes = {}, []
    de = scipy.optimize.differential_evolution

    def recording_de(*a, **k):
        seen["result"] = de(*a, **k)
        return seen["result"]
    many = mf._neg_var_many

    def recording_many(X, *a):
        sizes.append(np.shape(X)[0])
        return many(X, *a)
    monkeypatch.setattr(scipy.optimize, "differential_evolution", recording_de)
    monkeypatch.setattr(mf, "_neg_var_many", recording_many)
    st0 = m.stats()
    np.random.seed(0)
    x, value = mf.get_max_var(s["bounds"], thrd, c, s["XLn"], s["XHn"])
    st1 = m.stats()
    assert x.shape == (1, 2)
    LA.check_local_max(x, value, probe, pval, s["bounds"])
    ref = LA.oracle_neg_var("mf", s["XL"], s["yL"], s["XH"], s["yH"], s["hyp"], s["XLn"], s["XHn"], x, thrd, c)[0]
    assert ref[0] < 0                                                  # x is unmasked
    assert LA.floored_rel(np.array([value]), -ref, s["hyp"]) <= TOL
    nit = seen["result"].nit
    generations = [n for n in sizes if n > 1]
    polish = [n for n in sizes if n == 1]
    assert st1["look_border"] == st0["look_border"] + 1
    assert len(generations) == nit + 1, (len(generations), nit)        # the initial population, then one per iteration
    assert st1["look_query"] - st0["look_query"] == len(sizes) <= nit + 1 + len(polish)


# ---- 9. ExpectedImprovement -----------------------------------------------------

def test_expected_improvement_applies_the_reference_formula_to_the_posterior():
    from scipy.stats import norm

    from mfgp_coverage_amd.gaussian_process import SFGP
    s = LA.scenario("sf", 129, 0, 0, 130, seed=71)
    sf = SFGP(s["XH"], s["yH"][:, None], 1)
    sf.hyp = s["hyp"].copy()
    sf.updt_info(sf.X, sf.y)
    ei = sf.ExpectedImprovement(s["x"])
    assert ei.shape == (130, 1)
    mu, var = O.sf_diag(s["XH"], s["yH"], s["hyp"], s["x"])
    var = np.abs(var)[:, None]                        # gp:171
    best = np.min(s["yH"])                            # gp:174
    Z = (best - mu[:, None]) / var                    # gp:175
    ref = (best - mu[:, None]) * norm.cdf(Z) + var * norm.pdf(Z)   # gp:176
    assert LA.floored_rel(ei, ref, s["hyp"]) <= TOL
