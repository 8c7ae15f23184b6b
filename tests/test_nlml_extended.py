"""oracle.gp_oracle.nlml_extended (the NLML and its gradient wholly in 80-bit long
double) against the committed block-edge fixture tests/golden/nlml_edges_reference.npz,
the fp64 oracle, and the reference's own recorded likelihood values. No GPU."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _fixtures as F
from tests import _nlml_edges as E

EXTENDED = np.finfo(np.longdouble).eps < 1e-18
needs_extended = pytest.mark.skipif(not EXTENDED, reason="np.longdouble is not the 80-bit extended format here")


@pytest.fixture(scope="module")
def fx():
    return F.load("nlml_edges_reference.npz")


def test_fixture_holds_every_case(fx):
    keys = ("XL", "yL", "XH", "yH", "hyp", "jitter", "nlml", "grad", "cond", "e_oracle_val", "e_oracle_grad")
    assert sorted(fx) == sorted(f"{n}_{k}" for n in E.NAMES for k in keys)
    for name, kind, n, nl, key, perturbed in E.CASES:
        XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
        assert XL.shape == (nl, 2) and yL.shape == (nl,) and XH.shape == (n - nl, 2) and yH.shape == (n - nl,)
        assert hyp.shape == ((4,) if kind == "sf" else (9,)) and fx[f"{name}_grad"].shape == hyp.shape
        assert jitter == (1e-6 if perturbed else O.JITTER)
        assert all(a.dtype == np.float64 for a in (XL, yL, XH, yH, hyp, fx[f"{name}_nlml"], fx[f"{name}_grad"]))
        assert np.isfinite(fx[f"{name}_nlml"]) and np.all(np.isfinite(fx[f"{name}_grad"]))
        assert fx[f"{name}_cond"] >= 1.0


@pytest.mark.parametrize("name", E.NAMES)
def test_oracle_meets_fixture(fx, name):
    """The fp64 oracle against the extended values, within the bound the device is held to."""
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    v, g = O.nlml(XH, yH, hyp, jitter=jitter, grad=True, **E.oracle_kwargs(XL, yL, hyp))
    ev, eg = E.errors(v, g, float(fx[f"{name}_nlml"]), fx[f"{name}_grad"])
    bv, bg = E.bounds(fx, name)
    assert ev <= bv and eg <= bg, (ev, bv, eg, bg)
    assert O.nlml(XH, yH, hyp, jitter=jitter, **E.oracle_kwargs(XL, yL, hyp)) == v


@needs_extended
@pytest.mark.parametrize("name", E.NAMES)
def test_extended_reproduces_fixture(fx, name):
    """Maker and fixture cannot drift apart: recomputed now, the extended values round to
    the stored float64 (2 ulp of slack; nlml_extended calls no libm function, whose x87
    instructions differ between CPU vendors, so it has been the same bits on two hosts)."""
    XL, yL, XH, yH, hyp, jitter = E.case_inputs(fx, name)
    v, g = O.nlml_extended(XH, yH, hyp, jitter=jitter, **E.oracle_kwargs(XL, yL, hyp))
    assert v.dtype == np.longdouble and g.dtype == np.longdouble
    got = np.concatenate([[np.float64(v)], g.astype(np.float64)])
    ref = np.concatenate([[fx[f"{name}_nlml"]], fx[f"{name}_grad"]])
    assert np.all(np.abs(got - ref) <= 2 * np.spacing(np.abs(ref))), (got, ref)


@needs_extended
@pytest.mark.parametrize("c", ["sf_n50_h1", "sf_n130_h1", "mf_n30_h1", "mf_n90_h1"])
def test_extended_vs_reference_likelihood(c):
    """The restatement against the reference's own recorded likelihood, as
    test_oracle_nlml_vs_reference holds the fp64 oracle to it."""
    nl = F.load("nlml_reference.npz")
    n = int(nl[c + "_n"])
    X, y = nl["train"][:n, :2], nl["train"][:n, 2]
    kw = {} if c.startswith("sf") else {"XL": nl["prior"][:, :2], "yL": nl["prior"][:, 2]}
    v, g = O.nlml_extended(X, y, nl[c + "_hyp"], **kw)
    np.testing.assert_allclose(float(v), nl[c + "_nlml"], rtol=1e-12)
    _, go = O.nlml(X, y, nl[c + "_hyp"], grad=True, **kw)
    assert np.all(np.abs(g.astype(np.float64) - go) <= 1e-10 * np.maximum(np.abs(go), 1.0))


@needs_extended
def test_own_exp_and_log_against_libm():
    """_exp_ld / _log_ld (basic operations only) against the host's expl / logl, which are
    good to an ulp or so whatever the vendor: a few eps (1.08e-19) apart, exact at 0 / 1."""
    LD = np.longdouble
    eps = np.finfo(LD).eps
    x = np.concatenate([np.linspace(-60.0, 5.0, 4001), [-37.82682938, -15.98930639, 1e-5, -1e-5]]).astype(LD)
    assert np.max(np.abs(O._exp_ld(x) / np.exp(x) - 1)) <= 4 * eps
    p = np.concatenate([np.logspace(-12, 6, 2001), [2 * np.pi]]).astype(LD)
    assert np.max(np.abs(O._log_ld(p) - np.log(p)) / np.maximum(np.abs(np.log(p)), 1)) <= 4 * eps
    assert O._exp_ld(LD(0)) == 1 and O._log_ld(LD(1)) == 0 and O._exp_ld(LD(-20000)) == 0
    assert abs(O._PI - 4 * np.arctan(LD(1))) <= 4 * eps and abs(O._LN2 - np.log(LD(2))) <= eps


@needs_extended
def test_extended_edge_inputs():
    """N = 0 is the empty sum, a non-PD K raises as np.linalg.cholesky does."""
    from mfgp_coverage_amd import synthetic
    e2, e1 = np.empty((0, 2)), np.empty(0)
    for hyp in (synthetic.HYP["australia3_sf"], synthetic.HYP["australia9_mf"]):
        v, g = O.nlml_extended(e2, e1, hyp, **E.oracle_kwargs(e2, e1, hyp))
        assert v == 0 and g.shape == hyp.shape and not np.any(g)
    X = np.array([[0.1, 0.2], [0.1, 0.2]])
    with pytest.raises(np.linalg.LinAlgError):
        O.nlml_extended(X, np.zeros(2), synthetic.HYP["australia3_sf"], jitter=-1.0)


def test_extended_refuses_a_64bit_long_double(monkeypatch):
    monkeypatch.setattr(O, "LD", np.float64)
    with pytest.raises(RuntimeError, match="extended"):
        O.nlml_extended(np.zeros((1, 2)), np.zeros(1), np.zeros(4))
