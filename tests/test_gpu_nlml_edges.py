"""mfgp_nlml (k_nlml_value, k_trinv, k_kinv, k_alpha, k_nlml_grad and the host-side mean
terms) at the edges of its 64 x 64 tiles, against extended-precision values
(tests/golden/nlml_edges_reference.npz, made by oracle.gp_oracle.nlml_extended in 80-bit
long double; tests/_nlml_edges.py lists the cases), and the promises around it: the
likelihood sees the rows the model holds whatever route put them there, the caller's
model is untouched, an MFGP_F32 model gives the fp64 bits, the error paths, train on MF.

Bound per case, for the value and for the gradient (tests/_nlml_edges.bounds):
    16 * max(e_oracle, eps64 * cond(K) * max(N, 64))
with e_oracle the fp64 NumPy oracle's own error against the extended values: a margin
over the reference's error, never over the code under test.

Measured on an MI355X: the largest error over the cases of a hyperparameter set, as
device / fp64 oracle / bound of the case that gave it:
    set                                  value                        gradient
    australia3_sf (9 cases)              5.4e-15 / 5.5e-15 / 3.7e-11  4.9e-14 / 7.5e-14 / 3.5e-10
    australia9_mf (12 cases)             8.6e-16 / 2.6e-16 / 5.1e-12  1.4e-14 / 4.8e-15 / 1.8e-10
    australia8_mf (12 cases)             1.1e-12 / 2.6e-13 / 5.8e-10  5.4e-14 / 1.2e-13 / 3.9e-9
    anti_two_corners_sf N = 65           4.1e-11 / 3.6e-10 / 9.3e-6   7.6e-11 / 8.1e-10 / 9.3e-6
    anti_two_corners_sf N = 129          1.9e-9  / 8.3e-10 / 8.0e-5   7.5e-9  / 5.2e-9  / 8.0e-5
    australia9_mf perturbed, jitter 1e-6 1.5e-15 / 7.5e-16 / 1.7e-10  8.3e-15 / 1.6e-14 / 1.7e-10
No case exceeded its bound; the closest came to about 1/500 of it. Each test prints its
figures (NLML_EDGE lines, pytest -s).
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _fixtures as F
from tests import _nlml_edges as E

pytestmark = pytest.mark.gpu

E2, E1 = np.empty((0, 2)), np.empty(0)


@pytest.fixture(scope="module")
def fx():
    return F.load("nlml_edges_reference.npz")


def _model(ctx, XL, yL, XH, yH, hyp, jitter, dtype=None):
    from mfgp_coverage_amd import _lib
    kind = _lib.SF if hyp.shape[0] == 4 else _lib.MF
    m = _lib.Model(ctx, kind, hyp, jitter, dtype=_lib.F64 if dtype is None else dtype)
    m.set_data(XL, yL, XH, yH)
    return m


def _same_bits(a, b):
    va, ga = a
    vb, gb = b
    return np.float64(va).tobytes() == np.float64(vb).tobytes() and ga.tobytes() == gb.tobytes()


def _meets(fx, name, v, g):
    ev, eg = E.errors(v, g, float(fx[f"{name}_nlml"]), fx[f"{name}_grad"])
    bv, bg = E.bounds(fx, name)
    print(f"NLML_EDGE {name} val {ev:.3e} bound {bv:.3e} grad {eg:.3e} bound {bg:.3e}")
    assert ev <= bv and eg <= bg, (name, ev, bv, eg, bg)


# ---------------------------------------------------------------------------
# 1. every edge case against the extended-precision fixture
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.NAMES)
def test_edges_vs_fixture(fx, name):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    m = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
    v, g = m.nlml(hyp, grad=True)
    _meets(fx, name, v, g)
    # no atomics, host sums in a fixed order: the value alone and a second call give the same bits
    assert np.float64(m.nlml(hyp)).tobytes() == np.float64(v).tobytes()
    assert _same_bits(m.nlml(hyp, grad=True), (v, g))


# ---------------------------------------------------------------------------
# 2. the data the model holds is the data the likelihood sees
# ---------------------------------------------------------------------------

ROUTE_CASES = ["mf_australia9_mf_n129_nl64", "sf_australia3_sf_n129"]


def _route_appends(ctx, XL, yL, XH, yH, hyp, jitter, first, steps):
    """set_data of the first `first` rows (all lofi rows and the leading hifi rows), then
    one append per entry of `steps`."""
    at = first - XL.shape[0]
    m = _model(ctx, XL, yL, XH[:at], yH[:at], hyp, jitter)
    for k in steps:
        m.append(XH[at:at + k], yH[at:at + k])
        at += k
    assert at == XH.shape[0]
    return m


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_rows_reached_by_other_routes(fx, name):
    """The scratch model copies rows [0, N) and factors from scratch: appends across a tile
    edge (1 + 1 rows across 64, 16 rows across 128), 20 rows in one call (more than the
    bordered append takes: a refactor) and a truncate back from 140 rows all give the
    bits of the set_data route."""
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    ctx = _lib.context()
    base = _model(ctx, XL, yL, XH, yH, hyp, jitter).nlml(hyp, grad=True)
    _meets(fx, name, *base)
    n0 = max(63, XL.shape[0])          # (the MF case holds 64 lofi rows: it starts on the edge)
    mid = 113 - n0 - 2                 # bordered appends of at most 16 rows up to row 113
    routes = {"across_64_and_128": _route_appends(ctx, XL, yL, XH, yH, hyp, jitter, n0,
                                                  [1, 1] + [16] * (mid // 16) + [mid % 16] * (mid % 16 > 0) + [16]),
              "twenty_rows": _route_appends(ctx, XL, yL, XH, yH, hyp, jitter, 109, [20])}
    rng = np.random.default_rng(140)
    more = _model(ctx, XL, yL, np.vstack([XH, rng.random((11, 2))]), np.concatenate([yH, rng.random(11)]),
                  hyp, jitter)
    assert more.n == 140
    more.truncate(XH.shape[0])
    routes["truncated_from_140"] = more
    st = routes["across_64_and_128"].stats()
    assert st["inc_factor"] == 6 and st["full_factor"] == 1, st
    st = routes["twenty_rows"].stats()
    assert st["inc_factor"] == 0 and st["full_factor"] == 2, st
    for rname, m in routes.items():
        assert m.n == 129
        got = m.nlml(hyp, grad=True)
        assert _same_bits(got, base), rname
        _meets(fx, name, *got)
        assert np.float64(m.nlml(hyp)).tobytes() == np.float64(base[0]).tobytes(), rname


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_rows_staged_by_a_deferred_append(fx, name):
    """Deferred appends on: the rows are staged, not yet factored, when nlml is called."""
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    base = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter).nlml(hyp, grad=True)
    ctx = _lib.Context(0)
    ctx.set_deferred_appends(True)
    m = _route_appends(ctx, XL, yL, XH, yH, hyp, jitter, 120, [1, 8])
    assert m.n == 129 and m.stats()["factor_rows"] == 120, m.stats()
    got = m.nlml(hyp, grad=True)
    st = m.stats()
    assert st["factor_rows"] == 120 and st["inc_factor"] == 0 and st["full_factor"] == 1, st   # still staged
    assert _same_bits(got, base)
    _meets(fx, name, *got)
    L = m.factor()                              # runs the staged append: the rows were all there
    st = m.stats()
    assert L.shape == (129, 129) and st["factor_rows"] == 129 and st["inc_factor"] == 1, st
    assert _same_bits(m.nlml(hyp, grad=True), base)


# ---------------------------------------------------------------------------
# 3. the caller's model is untouched
# ---------------------------------------------------------------------------

PATHS = ("full_factor", "inc_factor", "full_predict", "vstream", "lattice")


def _twin(with_nlml, wl, hyp, h2):
    """One MF model (N = 120, NL = 40, a 16 x 16 lattice grid) on a context of its own,
    stepped by append + predict; with_nlml: nlml(h2, grad) is called in between."""
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    m = _lib.Model(ctx, _lib.MF, hyp, 1e-8)
    m.set_grid(wl.xs)
    m.set_data(wl.XL, wl.yL, wl.XH, wl.yH)
    probes, outs = [], []

    def probe():
        if not with_nlml:
            return
        s = m.serial()            # (serial() waits for nothing: a running launch keeps running)
        probes.append(m.nlml(h2, grad=True))
        assert m.serial() == s

    def step(i, between=False):
        m.append(wl.Xnew[i], wl.ynew[i])
        if between:
            probe()
        outs.append(m.predict())

    probe()                                   # after set_data, before the first predict
    outs.append(m.predict())
    step(0, between=True)                     # an eager append that returned at its early verdict
    ctx.set_deferred_appends(True)
    m.append(wl.Xnew[1], wl.ynew[1])          # a deferred append: staged
    assert m.stats()["factor_rows"] == 124
    probe()
    assert m.stats()["factor_rows"] == 124
    outs.append(m.predict())
    ctx.set_deferred_appends(False)
    probe()                                   # after a predict: the next append is the speculative fused one
    step(2)
    ctx.set_lattice("force")
    step(3)
    probe()                                   # between two lattice steps
    step(4)
    c = m.clone()
    if with_nlml:
        assert _same_bits(c.nlml(h2, grad=True), m.nlml(h2, grad=True))
    return m, outs, probes


def test_model_is_untouched():
    """mfgp_nlml builds a scratch model on the caller's context (its descriptor slots,
    workspace, stream): a twin that never calls it gives the same posterior bits, factor
    and path counters, and the serial does not move across the call."""
    from mfgp_coverage_amd import synthetic
    wl = synthetic.Workload(16, 40, 80, 4, 5, seed=120)
    hyp = synthetic.HYP["australia9_mf"]
    h2 = hyp + 0.05 * np.random.default_rng(120).standard_normal(9)
    a, outs_a, probes = _twin(True, wl, hyp, h2)
    b, outs_b, _ = _twin(False, wl, hyp, h2)
    assert len(outs_a) == len(outs_b) == 6 and len(probes) == 5
    for i, ((mu_a, var_a), (mu_b, var_b)) in enumerate(zip(outs_a, outs_b)):
        assert mu_a.tobytes() == mu_b.tobytes() and var_a.tobytes() == var_b.tobytes(), i
    assert a.factor().tobytes() == b.factor().tobytes()
    sa, sb = a.stats(), b.stats()
    assert {k: sa[k] for k in PATHS} == {k: sb[k] for k in PATHS}, (sa, sb)
    assert sa["lattice"] == 2 and sa["inc_factor"] == 5 and sa["full_factor"] == 1 and sa["full_predict"] == 1, sa
    assert sa["early_pd"] >= 1, sa
    # the last predict is the model's own posterior, and every probe the likelihood of its rows then
    X = np.vstack([wl.XH, wl.Xnew.reshape(-1, 2)])
    y = np.concatenate([wl.yH, wl.ynew.reshape(-1)])
    mu_r, var_r = O.mf_diag(wl.XL, wl.yL, X, y, hyp, wl.xs)
    assert max(O.parity_errors(*outs_a[-1], mu_r, var_r, O.prior_variance(hyp))) < O.PARITY_TOL
    for (v, g), nh in zip(probes, (80, 84, 88, 88, 96)):
        vo, go = O.nlml(X[:nh], y[:nh], h2, XL=wl.XL, yL=wl.yL, grad=True)
        np.testing.assert_allclose(v, vo, rtol=1e-10)
        assert np.all(np.abs(g - go) <= 1e-8 * np.maximum(np.abs(go), 1.0)), (nh, g, go)


# ---------------------------------------------------------------------------
# 4. an MFGP_F32 model: the scratch model is always fp64
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ROUTE_CASES)
def test_f32_model_gives_the_f64_bits(fx, name):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    m64 = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
    m32 = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter, dtype=_lib.F32)
    assert _same_bits(m32.nlml(hyp, grad=True), m64.nlml(hyp, grad=True))
    assert np.float64(m32.nlml(hyp)).tobytes() == np.float64(m64.nlml(hyp)).tobytes()


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------

def test_wrong_nhyp_raises(fx):
    from mfgp_coverage_amd import _lib, gaussian_process as gp
    msg = "Hyperparameters must be of length 4 \\(single-fidelity\\) or 9 \\(multi-fidelity\\)"
    for name, wrong in (("mf_australia9_mf_n65_nl64", 4), ("sf_australia3_sf_n65", 9)):
        XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
        m = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
        for grad in (False, True):
            with pytest.raises(TypeError, match=msg):      # _lib.check: MFGP_ERR_ARG with this message
                m.nlml(np.zeros(wrong), grad=grad)
        _meets(fx, name, *m.nlml(hyp, grad=True))           # and the model still answers
        d = gp.SFGP(XH, yH[:, None], 1) if hyp.shape[0] == 4 else gp.MFGP(XL, yL[:, None], XH, yH[:, None], 1, 1)
        with pytest.raises(TypeError, match=msg):
            d.likelihood(np.zeros(wrong))
        with pytest.raises(TypeError, match=msg):
            d.likelihood_and_grad(np.zeros(wrong))


@pytest.mark.parametrize("key", ["australia3_sf", "australia9_mf"])
def test_empty_model_is_the_empty_sum(key):
    from mfgp_coverage_amd import _lib, synthetic
    hyp = synthetic.HYP[key]
    m = _lib.Model(_lib.context(), _lib.SF if hyp.shape[0] == 4 else _lib.MF, hyp, 1e-8)
    assert m.nlml(hyp) == 0.0                               # before any data
    m.set_data(E2, E1, E2, E1)
    v, g = m.nlml(hyp, grad=True)
    assert v == 0.0 and g.shape == hyp.shape and not np.any(g)
    assert m.nlml(hyp) == 0.0


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_not_positive_definite_raises_and_recovers(fx, name):
    """jitter = -1 makes K indefinite by construction. set_hyp takes effect at the next
    factorisation only, mfgp_nlml reads the model's jitter at once: it raises, with and
    without the gradient, and leaves the model and its context usable."""
    from mfgp_coverage_amd import _lib, synthetic
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    Xs = synthetic.grid(16)
    m = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
    m.set_grid(Xs)
    m.predict()
    m.set_hyp(hyp, -1.0)
    for grad in (False, True, False):
        with pytest.raises(np.linalg.LinAlgError):
            m.nlml(hyp, grad=grad)
    m.set_hyp(hyp, 1e-8)
    mu, var = m.predict()
    if hyp.shape[0] == 4:
        mu_r, var_r = O.sf_diag(XH, yH, hyp, Xs)
    else:
        mu_r, var_r = O.mf_diag(XL, yL, XH, yH, hyp, Xs)
    assert max(O.parity_errors(mu, var, mu_r, var_r, O.prior_variance(hyp))) < O.PARITY_TOL
    _meets(fx, name, *m.nlml(hyp, grad=True))


# ---------------------------------------------------------------------------
# 6. train on an MF model
# ---------------------------------------------------------------------------

def test_train_mf_lowers_nlml(capsys):
    """train (gp:388-399) on MFGP: L-BFGS-B with the device gradient lowers the NLML, the
    oracle agrees on the trained point, and a predict afterwards runs with the trained hyp."""
    from mfgp_coverage_amd import gaussian_process as gp, synthetic
    wl = synthetic.Workload(32, 40, 30, 1, 1, seed=2)
    m = gp.MFGP(wl.XL.copy(), wl.yL.reshape(-1, 1).copy(), wl.XH.copy(), wl.yH.reshape(-1, 1).copy(), 1, 1)
    h0 = synthetic.HYP["australia9_mf"].copy()
    m.hyp = h0.copy()
    before = m.likelihood(m.hyp)
    np.testing.assert_allclose(before, O.nlml(wl.XH, wl.yH, h0, XL=wl.XL, yL=wl.yL), rtol=1e-10)
    m.train()
    assert "Log likelihood" in capsys.readouterr().out      # the reference's callback (gp:483-491)
    assert m.hyp.shape == (9,) and not np.array_equal(m.hyp, h0)
    after = m.likelihood(m.hyp)
    assert after < before
    np.testing.assert_allclose(after, O.nlml(wl.XH, wl.yH, m.hyp, XL=wl.XL, yL=wl.yL), rtol=1e-8)
    Xs = synthetic.grid(16)
    mu, cov = m.predict(Xs)
    mu_r, var_r = O.mf_diag(wl.XL, wl.yL, wl.XH, wl.yH, m.hyp, Xs)
    e = O.parity_errors(mu[:, 0], np.diag(cov), mu_r, var_r, O.prior_variance(m.hyp))
    assert max(e) < O.PARITY_TOL, e
