"""mfgp_nlml_batch (the NLML and its gradient for S hyperparameter vectors over one
model's data, in one set of launches per chunk) and train with restarts on it.

The central promise is bit equality: member s's value and gradient are what
mfgp_nlml(m, hyps[s]) returns, whatever S, the member's position, the other members,
the chunking, or whether the gradient was asked for. Everything here is that equality,
except where member 0 of an edge case also meets the existing bound of
tests/_nlml_edges.bounds against the extended-precision values
(tests/golden/nlml_edges_reference.npz), and the two oracle checks that
test_gpu_nlml_edges.py already makes after a recovery and after train (O.PARITY_TOL,
rtol 1e-8). No new tolerance is introduced.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _fixtures as F
from tests import _nlml_edges as E

pytestmark = pytest.mark.gpu

E2, E1 = np.empty((0, 2)), np.empty(0)
ROUTE_CASES = ["mf_australia9_mf_n129_nl64", "sf_australia3_sf_n129"]
PATHS = ("full_factor", "inc_factor", "full_predict", "vstream", "lattice")
NHYP_MSG = "Hyperparameters must be of length 4 \\(single-fidelity\\) or 9 \\(multi-fidelity\\)"


@pytest.fixture(scope="module")
def fx():
    return F.load("nlml_edges_reference.npz")


def _model(ctx, XL, yL, XH, yH, hyp, jitter, dtype=None):
    from mfgp_coverage_amd import _lib
    kind = _lib.SF if hyp.shape[0] == 4 else _lib.MF
    m = _lib.Model(ctx, kind, hyp, jitter, dtype=_lib.F64 if dtype is None else dtype)
    m.set_data(XL, yL, XH, yH)
    return m


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def _meets(fx, name, v, g):
    ev, eg = E.errors(v, g, float(fx[f"{name}_nlml"]), fx[f"{name}_grad"])
    bv, bg = E.bounds(fx, name)
    print(f"NLML_BATCH {name} val {ev:.3e} bound {bv:.3e} grad {eg:.3e} bound {bg:.3e}")
    assert ev <= bv and eg <= bg, (name, ev, bv, eg, bg)


def _assert_rows_are_single_calls(m, H, tag=""):
    """Every row of nlml_batch(H), with and without the gradient, has the bits of
    m.nlml(H[s]); a row the single call raises LinAlgError for has status > 0 and NaNs."""
    v1, st1 = m.nlml_batch(H, status=True)
    v2, g2, st2 = m.nlml_batch(H, grad=True, status=True)
    assert v1.shape == (len(H),) and g2.shape == H.shape and st1.dtype.kind == "i"
    assert np.array_equal(st1, st2)
    for s, h in enumerate(H):
        try:
            v, g = m.nlml(h, grad=True)
            v0 = m.nlml(h)
        except np.linalg.LinAlgError:
            assert st1[s] > 0 and np.isnan(v1[s]) and np.isnan(v2[s]) and np.all(np.isnan(g2[s])), (tag, s)
            continue
        assert st1[s] == 0, (tag, s, st1)
        assert _bits(v1[s]) == _bits(v0), (tag, s, "value alone")
        assert _bits(v2[s]) == _bits(v) and _bits(g2[s]) == _bits(g), (tag, s, "value and gradient")
    return v2, g2, st2


# ---------------------------------------------------------------------------
# 1. equals the single path, at every tile edge
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.NAMES)
def test_equals_the_single_path(fx, name):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    m = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
    rng = np.random.default_rng(E.NAMES.index(name))
    H = np.vstack([hyp, hyp + 0.05 * rng.standard_normal(hyp.shape[0]),
                   hyp + 0.05 * rng.standard_normal(hyp.shape[0])])
    v, g, st = _assert_rows_are_single_calls(m, H, name)
    assert st[0] == 0
    _meets(fx, name, v[0], g[0])


# ---------------------------------------------------------------------------
# 2. a member's bits are its own
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ROUTE_CASES)
def test_a_members_bits_are_its_own(fx, name):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    ctx = _lib.Context(0)
    m = _model(ctx, XL, yL, XH, yH, hyp, jitter)
    rng = np.random.default_rng(5)
    P = np.vstack([hyp] + [hyp + 0.05 * rng.standard_normal(hyp.shape[0]) for _ in range(3)])
    ref = {}
    for p in range(len(P)):                       # S = 1
        v, g = m.nlml_batch(P[p:p + 1], grad=True)
        assert _bits(v[0]) == _bits(m.nlml(P[p], grad=True)[0]) and _bits(g[0]) == _bits(m.nlml(P[p], grad=True)[1])
        assert _bits(m.nlml_batch(P[p:p + 1])[0]) == _bits(v[0])
        ref[p] = (_bits(v[0]), _bits(g[0]))
    orders = ([0, 1, 2, 3, 1], [3, 1, 1, 0, 2])   # S = 5, one vector twice
    for chunk in (0, 1, 2, 0):
        ctx.set_nlml_chunk(chunk)
        for order in orders:
            v, g = m.nlml_batch(P[order], grad=True)
            v0 = m.nlml_batch(P[order])
            for s, p in enumerate(order):
                assert (_bits(v[s]), _bits(g[s])) == ref[p], (chunk, order, s)
                assert _bits(v0[s]) == ref[p][0], (chunk, order, s)


def test_eleven_tile_rows_and_a_short_last_chunk():
    """N = 700 (300 lofi + 400 hifi rows: 11 tile rows), S = 3 in chunks of 2."""
    from mfgp_coverage_amd import _lib, synthetic
    wl = synthetic.Workload(32, 300, 400, 1, 1, seed=700)
    hyp = synthetic.HYP["australia9_mf"]
    ctx = _lib.Context(0)
    m = _model(ctx, wl.XL, wl.yL, wl.XH, wl.yH, hyp, 1e-8)
    assert m.n == 700
    rng = np.random.default_rng(700)
    H = np.vstack([hyp, hyp + 0.05 * rng.standard_normal(9), hyp + 0.05 * rng.standard_normal(9)])
    ctx.set_nlml_chunk(2)
    v, g, st = _assert_rows_are_single_calls(m, H, "n700 chunk 2")
    assert not np.any(st)
    ctx.set_nlml_chunk(0)
    v0, g0 = m.nlml_batch(H, grad=True)
    assert _bits(v0) == _bits(v) and _bits(g0) == _bits(g)


# ---------------------------------------------------------------------------
# 3. a member that is not positive definite
# ---------------------------------------------------------------------------

NOT_PD_CASES = ["sf_australia3_sf_n65", "sf_australia3_sf_n129", "mf_australia9_mf_n65_nl64",
                "mf_australia9_mf_n129_nl64"]


@pytest.mark.parametrize("name", NOT_PD_CASES)
def test_a_member_that_is_not_positive_definite(fx, name):
    """Jitter -0.25: noise 1.0 keeps K positive definite, noise 1e-4 makes its diagonal
    negative. The failing member gets its status and NaNs, the others their bits."""
    from mfgp_coverage_amd import _lib, synthetic
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    assert jitter == 1e-8
    Xs = synthetic.grid(16)
    ctx = _lib.Context(0)
    m = _model(ctx, XL, yL, XH, yH, hyp, jitter)
    m.set_grid(Xs)
    m.predict()
    m.set_hyp(hyp, -0.25)
    noise = (3,) if hyp.shape[0] == 4 else (7, 8)
    H = np.vstack([hyp, hyp, hyp])
    for p in noise:
        H[:, p] = np.log([1.0, 1e-4, 1.0])
    singles = [m.nlml(H[s], grad=True) for s in (0, 2)]
    with pytest.raises(np.linalg.LinAlgError):
        m.nlml(H[1], grad=True)
    for chunk in (0, 1):
        ctx.set_nlml_chunk(chunk)
        for grad in (True, False):
            out = m.nlml_batch(H, grad=grad, status=True)
            v, st = out[0], out[-1]
            assert st[0] == 0 and st[1] > 0 and st[2] == 0, st
            assert np.isnan(v[1])
            if grad:
                assert np.all(np.isnan(out[1][1]))
            for s, (v1, g1) in zip((0, 2), singles):
                assert _bits(v[s]) == _bits(v1), (chunk, grad, s)
                if grad:
                    assert _bits(out[1][s]) == _bits(g1), (chunk, s)
            with pytest.raises(np.linalg.LinAlgError):
                m.nlml_batch(H, grad=grad)
    ctx.set_nlml_chunk(0)
    m.set_hyp(hyp, 1e-8)
    mu, var = m.predict()
    if hyp.shape[0] == 4:
        mu_r, var_r = O.sf_diag(XH, yH, hyp, Xs)
    else:
        mu_r, var_r = O.mf_diag(XL, yL, XH, yH, hyp, Xs)
    assert max(O.parity_errors(mu, var, mu_r, var_r, O.prior_variance(hyp))) < O.PARITY_TOL
    _meets(fx, name, *m.nlml(hyp, grad=True))
    v, g = m.nlml_batch(hyp[None, :], grad=True)
    _meets(fx, name, v[0], g[0])


# ---------------------------------------------------------------------------
# 4. the caller's model is untouched
# ---------------------------------------------------------------------------

def _twin(mode, wl, hyp, H):
    """test_gpu_nlml_edges._twin's walk: one MF model (N = 120, NL = 40, a 16 x 16 lattice
    grid) on a context of its own, stepped by append + predict. mode "batch": nlml_batch(H)
    is called in between; "single": nlml of each row of H instead; None: neither."""
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    m = _lib.Model(ctx, _lib.MF, hyp, 1e-8)
    m.set_grid(wl.xs)
    m.set_data(wl.XL, wl.yL, wl.XH, wl.yH)
    probes, outs = [], []

    def probe():
        if mode is None:
            return
        s = m.serial()
        if mode == "batch":
            v, g, st = m.nlml_batch(H, grad=True, status=True)
            assert not np.any(st)
            probes.append((v, g, m.nlml_batch(H)))
        else:
            rows = [m.nlml(h, grad=True) for h in H]
            probes.append((np.array([r[0] for r in rows]), np.vstack([r[1] for r in rows]),
                           np.array([m.nlml(h) for h in H])))
        assert m.serial() == s

    def step(i, between=False):
        m.append(wl.Xnew[i], wl.ynew[i])
        if between:
            probe()
        outs.append(m.predict())

    probe()                                   # after set_data, before the first predict
    outs.append(m.predict())
    step(0, between=True)                     # after an eager append
    ctx.set_deferred_appends(True)
    m.append(wl.Xnew[1], wl.ynew[1])          # a deferred append: staged
    assert m.stats()["factor_rows"] == 124
    probe()
    assert m.stats()["factor_rows"] == 124    # still staged
    outs.append(m.predict())
    ctx.set_deferred_appends(False)
    probe()
    step(2)
    ctx.set_lattice("force")
    step(3)
    probe()                                   # between two lattice steps
    step(4)
    return m, outs, probes


def test_model_is_untouched():
    from mfgp_coverage_amd import synthetic
    wl = synthetic.Workload(16, 40, 80, 4, 5, seed=120)
    hyp = synthetic.HYP["australia9_mf"]
    H = np.vstack([hyp + 0.05 * np.random.default_rng(120).standard_normal(9), hyp])
    a, outs_a, probes_a = _twin("batch", wl, hyp, H)
    b, outs_b, _ = _twin(None, wl, hyp, H)
    _, _, probes_c = _twin("single", wl, hyp, H)
    assert len(outs_a) == len(outs_b) == 6 and len(probes_a) == len(probes_c) == 5
    for i, ((mu_a, var_a), (mu_b, var_b)) in enumerate(zip(outs_a, outs_b)):
        assert mu_a.tobytes() == mu_b.tobytes() and var_a.tobytes() == var_b.tobytes(), i
    assert a.factor().tobytes() == b.factor().tobytes()
    sa, sb = a.stats(), b.stats()
    assert {k: sa[k] for k in PATHS} == {k: sb[k] for k in PATHS}, (sa, sb)
    assert sa["lattice"] == 2 and sa["inc_factor"] == 5 and sa["full_factor"] == 1 and sa["full_predict"] == 1, sa
    # every probe is the single path's likelihood of the rows the model held then (80, 84,
    # 88 with the staged rows, 88, 96), which test_gpu_nlml_edges ties to the oracle
    for i, (pa, pc) in enumerate(zip(probes_a, probes_c)):
        assert all(_bits(x) == _bits(y) for x, y in zip(pa, pc)), i
    vals = [_bits(p[0]) for p in probes_a]
    assert vals[1] != vals[2] and vals[2] == vals[3]      # the staged rows count, and are the rows then factored


# ---------------------------------------------------------------------------
# 5. edges of the interface
# ---------------------------------------------------------------------------

def test_no_members(fx):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, "mf_australia9_mf_n65_nl64")
    m = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
    v, g, st = m.nlml_batch(np.empty((0, 9)), grad=True, status=True)
    assert v.shape == (0,) and g.shape == (0, 9) and st.shape == (0,)
    assert m.nlml_batch(np.empty((0, 9))).shape == (0,)
    assert _bits(m.nlml_batch(hyp[None, :])[0]) == _bits(m.nlml(hyp))   # and the model still answers


@pytest.mark.parametrize("key", ["australia3_sf", "australia9_mf"])
def test_empty_model_is_the_empty_sum(key):
    from mfgp_coverage_amd import _lib, synthetic
    hyp = synthetic.HYP[key]
    m = _lib.Model(_lib.context(), _lib.SF if hyp.shape[0] == 4 else _lib.MF, hyp, 1e-8)
    H = np.vstack([hyp, hyp + 0.1])
    for data in (False, True):
        if data:
            m.set_data(E2, E1, E2, E1)
        v, g, st = m.nlml_batch(H, grad=True, status=True)
        assert not np.any(v) and not np.any(g) and not np.any(st) and g.shape == H.shape
        assert not np.any(m.nlml_batch(H))


def test_wrong_nhyp_raises(fx):
    from mfgp_coverage_amd import _lib, gaussian_process as gp
    for name, wrong in (("mf_australia9_mf_n65_nl64", 4), ("sf_australia3_sf_n65", 9)):
        XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
        m = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
        for grad in (False, True):
            with pytest.raises(TypeError, match=NHYP_MSG):     # _lib.check: MFGP_ERR_ARG with this message
                m.nlml_batch(np.zeros((2, wrong)), grad=grad, status=True)
        v, g = m.nlml_batch(hyp[None, :], grad=True)
        _meets(fx, name, v[0], g[0])                            # and the model still answers
        d = gp.SFGP(XH, yH[:, None], 1) if hyp.shape[0] == 4 else gp.MFGP(XL, yL[:, None], XH, yH[:, None], 1, 1)
        with pytest.raises(TypeError, match=NHYP_MSG):
            d.likelihood_batch(np.zeros((2, wrong)))
        with pytest.raises(TypeError, match=NHYP_MSG):
            d.likelihood_and_grad_batch(np.zeros((2, wrong)))
        with pytest.raises(TypeError, match=NHYP_MSG):
            d.train(starts=np.zeros((2, wrong)))


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_f32_model_gives_the_f64_bits(fx, name):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    H = np.vstack([hyp, hyp + 0.05 * np.random.default_rng(32).standard_normal(hyp.shape[0])])
    m64 = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter)
    m32 = _model(_lib.context(), XL, yL, XH, yH, hyp, jitter, dtype=_lib.F32)
    v64, g64 = m64.nlml_batch(H, grad=True)
    v32, g32 = m32.nlml_batch(H, grad=True)
    assert _bits(v32) == _bits(v64) and _bits(g32) == _bits(g64)
    assert _bits(m32.nlml_batch(H)) == _bits(v64)
    _assert_rows_are_single_calls(m32, H, name)


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_repeated_calls_and_a_trim_in_between(fx, name):
    from mfgp_coverage_amd import _lib
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    ctx = _lib.Context(0)
    m = _model(ctx, XL, yL, XH, yH, hyp, jitter)
    H = np.vstack([hyp, hyp + 0.05 * np.random.default_rng(9).standard_normal(hyp.shape[0])])
    first = m.nlml_batch(H, grad=True)
    second = m.nlml_batch(H, grad=True)
    ctx.trim()
    third = m.nlml_batch(H, grad=True)
    smaller = m.nlml_batch(H[:1])                               # scratch kept from a larger call
    for other in (second, third):
        assert _bits(other[0]) == _bits(first[0]) and _bits(other[1]) == _bits(first[1])
    assert _bits(smaller[0]) == _bits(first[0][0])


# ---------------------------------------------------------------------------
# 6. the drop-in classes: likelihood_batch and train with restarts
# ---------------------------------------------------------------------------

def _mfgp(wl, h0):
    from mfgp_coverage_amd import gaussian_process as gp
    m = gp.MFGP(wl.XL.copy(), wl.yL.reshape(-1, 1).copy(), wl.XH.copy(), wl.yH.reshape(-1, 1).copy(), 1, 1)
    m.hyp = h0.copy()
    return m


def test_likelihood_batch_rows():
    from mfgp_coverage_amd import synthetic
    wl = synthetic.Workload(32, 40, 30, 1, 1, seed=2)
    h0 = synthetic.HYP["australia9_mf"]
    m = _mfgp(wl, h0)
    H = np.vstack([h0, h0 + 0.1, h0 - 0.1])
    v = m.likelihood_batch(H)
    v2, g2 = m.likelihood_and_grad_batch(H)
    for s, h in enumerate(H):
        v1, g1 = m.likelihood_and_grad(h)
        assert _bits(v[s]) == _bits(m.likelihood(h)) and _bits(v2[s]) == _bits(v1) and _bits(g2[s]) == _bits(g1)
    m.jitter = -0.25
    m._push_hyp()
    H[1, 7:] = np.log(1e-4)
    with pytest.raises(np.linalg.LinAlgError):
        m.likelihood_batch(H)
    with pytest.raises(np.linalg.LinAlgError):
        m.likelihood_and_grad_batch(H)


def test_train_with_restarts(capsys):
    """Four explicit starts around australia9_mf: every start's run is the solo L-BFGS-B
    run from it, m.hyp the best of them; train() alone is still the reference's."""
    from scipy.optimize import minimize
    from mfgp_coverage_amd import synthetic
    wl = synthetic.Workload(32, 40, 30, 1, 1, seed=2)
    h0 = synthetic.HYP["australia9_mf"].copy()
    rng = np.random.default_rng(4)
    starts = np.vstack([h0] + [h0 + 0.1 * rng.standard_normal(9) for _ in range(3)])
    m = _mfgp(wl, h0)
    before = m.likelihood(m.hyp)
    solo = [minimize(m.likelihood_and_grad, x0, jac=True, method="L-BFGS-B") for x0 in starts]
    m.train(starts=starts)
    assert "Log likelihood" not in capsys.readouterr().out      # no callback with restarts
    assert len(m.train_runs) == 4
    for rec, s, x0 in zip(m.train_runs, solo, starts):
        assert set(rec) == {"x0", "x", "fun", "nit", "nfev", "success", "message"}
        assert _bits(rec["x0"]) == _bits(x0)
        assert _bits(rec["x"]) == _bits(s.x) and _bits(rec["fun"]) == _bits(s.fun)
        assert rec["nfev"] == s.nfev and rec["nit"] == s.nit and rec["success"] == s.success
    best = min(range(4), key=lambda i: (solo[i].fun, i))
    assert _bits(m.hyp) == _bits(solo[best].x)
    after = m.likelihood(m.hyp)
    assert after < before
    np.testing.assert_allclose(after, O.nlml(wl.XH, wl.yH, m.hyp, XL=wl.XL, yL=wl.yL), rtol=1e-8)
    Xs = synthetic.grid(16)
    mu, cov = m.predict(Xs)
    mu_r, var_r = O.mf_diag(wl.XL, wl.yL, wl.XH, wl.yH, m.hyp, Xs)
    e = O.parity_errors(mu[:, 0], np.diag(cov), mu_r, var_r, O.prior_variance(m.hyp))
    assert max(e) < O.PARITY_TOL, e
    # drawn restarts: self.hyp first, then seeded draws; the same seed gives the same runs
    m2 = _mfgp(wl, h0)
    m2.train(n_restarts=2, scale=0.1, seed=4)
    assert len(m2.train_runs) == 3 and _bits(m2.train_runs[0]["x0"]) == _bits(h0)
    assert _bits(m2.train_runs[0]["x"]) == _bits(solo[0].x)
    assert _bits(m2.train_runs[1]["x0"]) == _bits(starts[1]) and _bits(m2.train_runs[1]["x"]) == _bits(solo[1].x)
    # train() with no arguments: the reference's body, callback lines included
    capsys.readouterr()
    m3 = _mfgp(wl, h0)
    m3.train()
    assert "Log likelihood" in capsys.readouterr().out
    assert _bits(m3.hyp) == _bits(solo[0].x)


def test_train_when_every_start_fails():
    from mfgp_coverage_amd import synthetic
    wl = synthetic.Workload(32, 40, 30, 1, 1, seed=2)
    h0 = synthetic.HYP["australia9_mf"].copy()
    m = _mfgp(wl, h0)
    m.likelihood(h0)                      # the data reach the device under the good jitter
    m.jitter = -0.25
    m._push_hyp()                         # (takes effect at the next factorisation: the members')
    bad = h0.copy()
    bad[7:] = np.log(1e-4)
    with pytest.raises(np.linalg.LinAlgError):
        m.train(starts=np.vstack([bad, bad + 0.01]))
    assert _bits(m.hyp) == _bits(h0)
    assert [r["success"] for r in m.train_runs] == [False, False]
