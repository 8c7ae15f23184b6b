"""oracle.gp_oracle.posterior_extended (the posterior mean and variance wholly in 80-bit
long double) against the committed tile-edge fixture tests/golden/
posterior_edges_reference.npz, the fp64 oracle, and the reference's own recorded
posteriors; and the gate built on it against two planted errors that PARITY_TOL lets
through. No GPU."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gp_oracle as O
from tests import _fixtures as F
from tests import _posterior_edges as E

EXTENDED = np.finfo(np.longdouble).eps < 1e-18
needs_extended = pytest.mark.skipif(not EXTENDED, reason="np.longdouble is not the 80-bit extended format here")


@pytest.fixture(scope="module")
def fx():
    return F.load("posterior_edges_reference.npz")


def test_fixture_holds_every_case(fx):
    want = [f"{n}_{k}" for n in E.NAMES for k in E.INPUT_KEYS]
    want += [f"{n}_s{s}_{k}" for n, s in E.STAGE_IDS for k in E.STAGE_KEYS]
    assert sorted(fx) == sorted(want)
    assert len(E.CASES) == 22 and {nx * ny for nx, ny in E.GRIDS} == {63, 64, 65, 129, 143, 144, 195}
    for name, kind, key, n, nl, nx, ny, offgrid in E.CASES:
        XL, yL, XH, yH, hyp, jitter, Xs = E.case_inputs(fx, name)
        M = nx * ny
        assert (nx, ny) in E.GRIDS and n <= 193 and M <= 200
        assert XL.shape == (nl, 2) and yL.shape == (nl,) and XH.shape == (n - nl, 2) and yH.shape == (n - nl,)
        assert Xs.shape == (M, 2) and np.array_equal(Xs, E.make_grid(nx, ny))
        assert hyp.shape == ((4,) if kind == "sf" else (9,)) and jitter == O.JITTER
        assert all(a.dtype == np.float64 for a in (XL, yL, XH, yH, hyp, Xs))
        # distinct rows, at grid cells except for the off-grid tail
        X = np.vstack([XL, XH])
        assert np.unique(X, axis=0).shape[0] == n
        at_cell = np.array([np.any(np.all(Xs == x, axis=1)) for x in X])
        assert np.all(at_cell[:n - E.TAIL]) and np.all(at_cell[n - E.TAIL:] != offgrid)
        for s in E.stages(n, nl):
            mu, var, kss = E.stage_ref(fx, name, s)
            assert mu.shape == (M,) and var.shape == (M,) and mu.dtype == np.float64 and var.dtype == np.float64
            assert np.all(np.isfinite(mu)) and np.all(var > 0) and np.all(var <= kss)
            assert abs(kss - O.prior_variance(hyp)) <= 2 * np.spacing(kss)      # (libm's exp: an ulp off)
            assert fx[f"{name}_s{s}_cond"] >= 1.0
            assert 0 <= fx[f"{name}_s{s}_e_oracle_mu"] < 1e-8 and 0 <= fx[f"{name}_s{s}_e_oracle_var"] < 1e-12


@pytest.mark.parametrize("name", E.NAMES)
def test_oracle_meets_fixture(fx, name):
    """The fp64 oracle against the extended values, within the bound the device is held to."""
    _, _, _, _, hyp, jitter, Xs = E.case_inputs(fx, name)
    for s in E.case_stages(name):
        mu, var = E.oracle(*E.stage_rows(fx, name, s), hyp, Xs, jitter)
        e_mu, e_var = E.errors(mu, var, *E.stage_ref(fx, name, s))
        b_mu, b_var = E.bounds(fx, name, s)
        assert e_mu <= b_mu and e_var <= b_var, (s, e_mu, b_mu, e_var, b_var)


@needs_extended
@pytest.mark.parametrize("name", E.NAMES)
def test_extended_reproduces_fixture(fx, name):
    """Maker and fixture cannot drift apart: recomputed now, the extended values round to
    the stored float64 (2 ulp of slack; posterior_extended calls no libm function)."""
    _, _, _, _, hyp, jitter, Xs = E.case_inputs(fx, name)
    for s in E.case_stages(name):
        mu, var, kss = O.posterior_extended(*E.stage_rows(fx, name, s), hyp, Xs, jitter)
        assert mu.dtype == np.longdouble and var.dtype == np.longdouble and kss.dtype == np.longdouble
        mu_r, var_r, kss_r = E.stage_ref(fx, name, s)
        got = np.concatenate([mu.astype(np.float64), var.astype(np.float64), [np.float64(kss)]])
        ref = np.concatenate([mu_r, var_r, [kss_r]])
        assert np.all(np.abs(got - ref) <= 2 * np.spacing(np.abs(ref))), (s, np.max(np.abs(got - ref)))


@needs_extended
@pytest.mark.parametrize("kind", ["sf", "mf"])
@pytest.mark.parametrize("N", [0, 9, 50, 130])
def test_extended_vs_reference_posterior(kind, N):
    """The restatement against the reference's own recorded posterior on its 32 x 32 grid
    (tests/golden/atc_reference.npz), within the bound formula of that case: 16 times the
    larger of the fp64 diag oracle's error against the extended values and
    eps64 cond(K) max(N, 64)."""
    atc = F.atc()
    X, y, Xs = atc["train"][:N, :2], atc["train"][:N, 2], atc["grid_g32"]
    e2, e1 = np.empty((0, 2)), np.empty(0)
    if kind == "sf":
        XL, yL, hyp = e2, e1, atc["hyp_sf"]
        K = O.se_kernel(X, X, hyp[1], hyp[2]) + np.eye(N) * (np.exp(hyp[-1]) + O.JITTER)
    else:
        XL, yL, hyp = atc["prior"][:, :2], atc["prior"][:, 2], atc["hyp_mf"]
        K = O.mf_K(XL, X, hyp)
    mu, var, kss = O.posterior_extended(XL, yL, X, y, hyp, Xs)
    mu64, var64, kss = mu.astype(np.float64), var.astype(np.float64), float(kss)
    n = XL.shape[0] + N
    cond = np.linalg.cond(K, 2) if n else 1.0
    e_or = E.errors(*E.oracle(XL, yL, X, y, hyp, Xs, O.JITTER), mu64, var64, kss)
    e = E.errors(atc[f"{kind}_g32_n{N}_mu"], atc[f"{kind}_g32_n{N}_var"], mu64, var64, kss)
    b = [E.bound_of(eo, cond, n) for eo in e_or]
    assert e[0] <= b[0] and e[1] <= b[1], (e, b, cond)


@needs_extended
def test_extended_edge_inputs():
    """N = 0 is the prior, a non-PD K raises as np.linalg.cholesky does."""
    from mfgp_coverage_amd import synthetic
    e2, e1, Xs = np.empty((0, 2)), np.empty(0), E.make_grid(3, 2)
    for key in ("australia3_sf", "australia9_mf"):
        hyp = synthetic.HYP[key]
        mu, var, kss = O.posterior_extended(e2, e1, e2, e1, hyp, Xs)
        assert mu.shape == var.shape == (6,) and mu.dtype == var.dtype == np.longdouble
        assert np.all(var == kss) and np.all(mu == mu[0])
        assert abs(np.float64(kss) - O.prior_variance(hyp)) <= 2 * np.spacing(O.prior_variance(hyp))
        assert abs(np.float64(mu[0]) - O.prior_mean(hyp)) <= 2 * np.spacing(O.prior_mean(hyp))
    X = np.array([[0.1, 0.2], [0.1, 0.2]])
    with pytest.raises(np.linalg.LinAlgError):
        O.posterior_extended(e2, e1, X, np.zeros(2), synthetic.HYP["australia3_sf"], Xs, jitter=-1.0)


def test_extended_refuses_a_64bit_long_double(monkeypatch):
    monkeypatch.setattr(O, "LD", np.float64)
    with pytest.raises(RuntimeError, match="extended"):
        O.posterior_extended(np.empty((0, 2)), np.empty(0), np.zeros((1, 2)), np.zeros(1), np.zeros(4), np.zeros((1, 2)))


# (a stage whose mean stays 5e-3 away from zero: parity_errors divides mu's error by |mu| cell by
# cell, and a zero crossing would inflate a float32 rounding of z past even PARITY_TOL)
TEETH = ("mf_australia8_mf_n64_nl0_8x8", 63)


def test_the_gate_has_teeth(fx):
    """Two planted errors on an australia8_mf stage, applied to the fp64 oracle's result:
    1e-9 k** added to one cell's variance, and z = L^-1 r rounded to float32 before
    mu = m + V^T z. Both exceed the bound of that stage, and both pass
    parity_errors < PARITY_TOL: the gate every other posterior test uses misses them."""
    name, s = TEETH
    _, _, _, _, hyp, jitter, Xs = E.case_inputs(fx, name)
    XL, yL, XH, yH = E.stage_rows(fx, name, s)
    mu_r, var_r, kss = E.stage_ref(fx, name, s)
    b_mu, b_var = E.bounds(fx, name, s)
    mu, var = O.mf_diag(XL, yL, XH, yH, hyp, Xs, jitter)
    e_mu, e_var = E.errors(mu, var, mu_r, var_r, kss)
    assert e_mu <= b_mu and e_var <= b_var

    var_bad = var.copy()
    var_bad[Xs.shape[0] // 2] += 1e-9 * kss
    e = E.errors(mu, var_bad, mu_r, var_r, kss)
    assert e[1] > b_var and e[0] <= b_mu, (e, b_var)
    assert max(O.parity_errors(mu, var_bad, mu_r, var_r, kss)) < O.PARITY_TOL

    _, _, _, mean_L, mean_H = O._mf_parts(hyp)
    L = np.linalg.cholesky(O.mf_K(XL, XH, hyp, jitter))
    V = sla.solve_triangular(L, O.mf_psi(Xs, XL, XH, hyp).T, lower=True, check_finite=False)
    z = sla.solve_triangular(L, np.concatenate((yL - mean_L, yH - mean_H)), lower=True, check_finite=False)
    assert np.array_equal(mean_H + V.T @ z, mu)                       # the oracle's own steps
    mu_bad = mean_H + V.T @ z.astype(np.float32).astype(np.float64)
    e = E.errors(mu_bad, var, mu_r, var_r, kss)
    assert e[0] > b_mu and e[1] <= b_var, (e, b_mu)
    assert max(O.parity_errors(mu_bad, var, mu_r, var_r, kss)) < O.PARITY_TOL
