"""Pathwise (Matheron) samples of the prior and the posterior on the whole lattice grid
from the resident V (mfgp_sample_posterior: k_sample_t, k_sample_field, k_sample_resid,
k_sample_solve, k_sample_gemm), and the drop-in classes' sample_posterior / sample_prior.

No statistics are involved: a sample is affine in its normals, f = f(0) + J z, so
  * the zero-normal sample is the posterior mean: against the oracle's mu, O.parity_errors
    <= O.PARITY_TOL;
  * sum_i a_i a_i^T with a_i = f(e_i) - f(0) over the nz unit vectors is the sampler's
    covariance J J^T: against the oracle's dense posterior covariance (O.sf_faithful /
    O.mf_faithful, return_cov=True), and with MFGP_SAMPLE_PRIOR against
    cov_block(prior=True)'s k**, in the floored-relative metric
    max |d| / max(|ref|, 1e-6 k**) <= O.PARITY_TOL.
Measured maxima over the cases of tests/_pathwise.py (13x11 with N = 0, 1, 63, 64, 65,
129; 17x19 with N = 197, 257; 8x8 with N = 65; 5x13 with N = 64; SF and MF) on an
MI355X: mean 6.6e-11, posterior covariance 2.7e-9, prior covariance 1.0e-14 (DESIGN.md
section 19).
Comparisons between samples of the same model are bit for bit: a sample's bits depend
only on its own normals.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _pathwise as PW

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL


def _model(c, ctx=None, dtype=None, Xs=None):
    from mfgp_coverage_amd import _lib
    ctx = _lib.context() if ctx is None else ctx
    m = _lib.Model(ctx, _lib.SF if c["kind"] == "sf" else _lib.MF, c["hyp"], 1e-8,
                   dtype=_lib.F64 if dtype is None else dtype)
    m.set_grid(c["Xs"] if Xs is None else Xs)
    X, y, NL = c["X"], c["y"], c["NL"]
    if X.shape[0]:
        if c["kind"] == "sf":
            m.set_data(np.empty((0, 2)), np.empty(0), X, y)
        else:
            m.set_data(X[:NL], y[:NL], X[NL:], y[NL:])
    return m


_MODELS = {}


def _case(kind, shape, N):
    """One model per case with the oracle's mean and covariance: computed once, shared,
    never modified."""
    key = (kind, shape, N)
    if key not in _MODELS:
        c = PW.case(kind, shape, N)
        mu_r, cov_r = PW.oracle_mean_cov(c)
        _MODELS[key] = (c, _model(c), mu_r, cov_r)
    return _MODELS[key]


# ---- 1. / 2. mean and covariance against the oracle ---------------------------------

@pytest.mark.parametrize("kind,shape,N", PW.CASES)
def test_mean_and_covariance_vs_oracle(kind, shape, N):
    c, m, mu_r, cov_r = _case(kind, shape, N)
    hyp, M = c["hyp"], c["Xs"].shape[0]
    d = m.sample_dims()
    assert (d["M"], d["N"], d["fields"]) == (M, N, 1 if kind == "sf" else 2)
    assert d["nz"] == d["rx0"] * d["ry0"] + d["rx1"] * d["ry1"] + N
    nz = d["nz"]
    s0 = m.stats()
    f0, C = PW.basis_cov(m.sample, nz, chunk=64)
    assert f0.shape == (M,) and C.shape == (M, M)
    e_mu = O.parity_errors(f0, np.diag(cov_r), mu_r, np.diag(cov_r), O.prior_variance(hyp))[0]
    e_cov = PW.floored_rel(C, cov_r, hyp)
    print(f"pathwise {kind} {shape} N = {N}: nz = {nz}, mu error {e_mu:.3e}, covariance error {e_cov:.3e}")
    assert e_mu <= TOL
    assert e_cov <= TOL
    # the launches are counted: one solve and one GEMM per call of <= 64 samples (none without data)
    calls = 1 + (nz + 63) // 64
    s1 = m.stats()
    assert s1["sample_solve"] - s0["sample_solve"] == (calls if N else 0)
    assert s1["sample_gemm"] - s0["sample_gemm"] == (calls if N else 0)


@pytest.mark.parametrize("kind,shape,N", [(k, s, N) for k, s, N in PW.CASES if N in (0, 65, 257, 64)])
def test_prior_covariance_vs_cov_block(kind, shape, N):
    c, m, _, _ = _case(kind, shape, N)
    hyp = c["hyp"]
    d = m.sample_dims(prior=True)
    assert d["N"] == 0 and d["nz"] == d["rx0"] * d["ry0"] + d["rx1"] * d["ry1"]
    p0, P = PW.basis_cov(lambda Z: m.sample(Z, prior=True), d["nz"], chunk=64)
    assert np.all(p0 == 0.0)                       # zero mean, exactly
    e = PW.floored_rel(P, m.cov_block(prior=True), hyp)
    print(f"pathwise prior {kind} {shape}: nz = {d['nz']}, covariance error vs cov_block(prior) {e:.3e}")
    assert e <= TOL
    # the noise block of the normals is not read: wider rows give the same bits
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((3, d["nz"] + 5))
    Z[:, d["nz"]:] = np.nan
    assert np.array_equal(m.sample(np.ascontiguousarray(Z[:, :d["nz"]]), prior=True),
                          m.sample(Z[:, :d["nz"]], prior=True))


# ---- 3. bit determinism ------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape,N", [("mf", (17, 19), 257), ("sf", (13, 11), 129), ("mf", (13, 11), 0)])
def test_bits_depend_on_the_samples_own_normals(kind, shape, N):
    c, m, _, _ = _case(kind, shape, N)
    nz = m.sample_dims()["nz"]
    rng = np.random.default_rng(7)
    Z = rng.standard_normal((130, nz))
    F = m.sample(Z)
    assert F.shape == (130, c["Xs"].shape[0]) and np.all(np.isfinite(F))
    assert np.array_equal(m.sample(Z), F)                       # two calls agree
    for s in (0, 63, 64, 65, 129):                              # alone
        assert np.array_equal(m.sample(Z[s:s + 1])[0], F[s]), s
    for S in (63, 64, 65):                                      # in a permuted batch
        perm = rng.permutation(130)[:S]
        assert np.array_equal(m.sample(Z[perm]), F[perm]), S
    # a wider leading dimension on either side changes nothing
    Zw = np.full((130, nz + 3), 9.0)
    Zw[:, :nz] = Z
    out = np.full((130, F.shape[1] + 2), -7.25)
    r = m.sample(Zw[:, :nz], out=out)
    assert np.array_equal(r, F) and np.all(out[:, F.shape[1]:] == -7.25)


def test_device_pointers_equal_host():
    import torch
    c, m, _, _ = _case("mf", (17, 19), 197)
    M, nz = c["Xs"].shape[0], m.sample_dims()["nz"]
    Z = np.random.default_rng(9).standard_normal((70, nz))
    want = m.sample(Z)
    zt = torch.from_numpy(Z).cuda()
    ot = torch.full((70, M + 1), -1.5, dtype=torch.float64, device="cuda")
    assert m.sample(zt.data_ptr(), out=ot.data_ptr(), S=70, ldz=nz, ldo=M + 1) is None
    torch.cuda.synchronize()
    h = ot.cpu().numpy()
    assert np.array_equal(h[:, :M], want) and np.all(h[:, M] == -1.5)


# ---- 4. the model is untouched ------------------------------------------------------------

def _untouched(m, Z):
    """predict bits, serial and every path counter before and after sample(Z)."""
    mu0, var0 = m.predict()
    s0, st0 = m.serial(), m.stats()
    F = m.sample(Z)
    P = m.sample(Z[:, :m.sample_dims(prior=True)["nz"]], prior=True)
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(P))
    st1 = m.stats()
    calls = (Z.shape[0] + 63) // 64
    assert st1.pop("sample_solve") - st0.pop("sample_solve") == calls
    assert st1.pop("sample_gemm") - st0.pop("sample_gemm") == calls
    assert st1 == st0
    assert m.serial() == s0
    mu1, var1 = m.predict()
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0)
    assert m.stats()["full_predict"] == st0["full_predict"] and m.stats()["vstream"] == st0["vstream"]
    return F


def test_model_untouched_after_set_data():
    c = PW.case("mf", (13, 11), 129, seed=77)
    m = _model(c)
    nz = m.sample_dims()["nz"]
    F = _untouched(m, np.random.default_rng(1).standard_normal((70, nz)))
    assert F.shape == (70, 143)
    # a clone has no sample record of its own and gives the same bits
    k = m.clone()
    Z = np.random.default_rng(2).standard_normal((2, nz))
    assert np.array_equal(k.sample(Z), m.sample(Z))


def test_model_untouched_between_lattice_steps():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_lattice("force")
    gx, gy, Xs = PW.lattice(24, 24)
    rng = np.random.default_rng(31)
    cells = rng.choice(Xs.shape[0], 174, replace=False)
    X = Xs[cells]
    y = PW.field(X, rng)
    c = dict(kind="mf", Xs=Xs, X=X[:150], y=y[:150], NL=60, hyp=PW.HYP_MF)
    m = _model(c, ctx=ctx)
    m.predict()
    m.append(X[150:158], y[150:158])
    m.predict()
    assert m.stats()["lattice"] == 1, m.stats()
    nz = m.sample_dims()["nz"]
    _untouched(m, np.random.default_rng(4).standard_normal((5, nz)))
    # the sampler serves the appended model: the zero-normal sample is its mean
    c2 = dict(c, X=X[:158], y=y[:158])
    mu_r, cov_r = PW.oracle_mean_cov(c2)
    f0 = m.sample(np.zeros((1, nz)))[0]
    assert O.parity_errors(f0, np.diag(cov_r), mu_r, np.diag(cov_r), O.prior_variance(PW.HYP_MF))[0] <= TOL
    # and the next bordered append still takes the lattice step
    m.append(X[158:166], y[158:166])
    m.predict()
    assert m.stats()["lattice"] == 2, m.stats()
    assert m.sample_dims()["nz"] == nz + 8


def test_settles_a_pending_append():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_deferred_appends(True)
    c = PW.case("sf", (17, 19), 128, seed=41)
    full = dict(c)
    c = dict(c, X=c["X"][:120], y=c["y"][:120])
    m = _model(c, ctx=ctx)
    m.predict()
    m.append(full["X"][120:], full["y"][120:])
    nz = m.sample_dims()["nz"]
    f0 = m.sample(np.zeros((1, nz)))[0]
    mu_r, cov_r = PW.oracle_mean_cov(full)
    assert m.stats()["v_rows"] == 128 and m.stats()["factor_rows"] == 128
    assert O.parity_errors(f0, np.diag(cov_r), mu_r, np.diag(cov_r), O.prior_variance(c["hyp"]))[0] <= TOL
    mu, var = m.predict()
    assert max(O.parity_errors(mu, var, mu_r, np.diag(cov_r), O.prior_variance(c["hyp"]))) <= TOL


# ---- 5. errors launch nothing ------------------------------------------------------------

def test_errors_launch_nothing():
    from mfgp_coverage_amd import _lib
    c = PW.case("mf", (13, 11), 65, seed=61)
    M = c["Xs"].shape[0]
    rng = np.random.default_rng(5)

    def unchanged(m, fails):
        mu0, var0 = m.predict()
        st0, s0 = m.stats(), m.serial()
        fails(m)
        assert m.stats() == st0 and m.serial() == s0
        mu1, var1 = m.predict()
        assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0)

    # a jittered grid is no lattice
    mj = _model(c, Xs=c["Xs"] + 1e-3 * rng.standard_normal(c["Xs"].shape))
    assert mj.stats()["lattice_nx"] == 0

    def no_lattice(m):
        with pytest.raises(_lib.NoLatticeError, match="not a lattice"):
            m.sample(np.zeros((1, 500)))
        with pytest.raises(_lib.NoLatticeError):
            m.sample_dims()
    unchanged(mj, no_lattice)

    # one training row off its cell
    off = dict(c, X=c["X"].copy())
    off["X"][40] += (0.0, 1e-4)
    mo = _model(off)

    def off_cell(m):
        with pytest.raises(_lib.NoLatticeError, match="training row 40"):
            m.sample(np.zeros((1, m.sample_dims()["nz"])))
        assert m.sample(np.zeros((1, m.sample_dims(prior=True)["nz"])), prior=True).shape == (1, M)   # the prior needs no rows
    unchanged(mo, off_cell)

    # an fp32 model
    mf = _model(c, dtype=_lib.F32)

    def f32(m):
        with pytest.raises(ValueError, match="MFGP_F32"):
            m.sample(np.zeros((1, 500)))
        with pytest.raises(ValueError, match="MFGP_F32"):
            m.sample_dims()
    unchanged(mf, f32)

    # arguments
    m = _model(c)
    nz = m.sample_dims()["nz"]
    good = m.sample(np.ones((2, nz)))

    def args(m):
        with pytest.raises(ValueError, match="ldo"):
            m.sample(np.zeros((2, nz)), out=np.zeros((2, M - 1)))
        with pytest.raises(ValueError, match="ldz"):
            m.sample(np.zeros((2, nz - 1)))
        Z = np.zeros((66, nz))
        Z[65, nz - 1] = np.nan
        with pytest.raises(ValueError, match="finite"):
            m.sample(Z)
        Z[65, nz - 1] = np.inf
        with pytest.raises(ValueError, match="finite"):
            m.sample(Z)
        with pytest.raises(ValueError, match="negative"):
            _lib.check(_lib.lib().mfgp_sample_posterior(m.handle, None, -1, nz, None, M, 0))
        with pytest.raises(ValueError, match="null"):
            _lib.check(_lib.lib().mfgp_sample_posterior(m.handle, None, 1, nz, None, M, 0))
        # an empty draw writes nothing
        out = np.full((1, M), -7.25)
        assert m.sample(np.zeros((0, nz)), out=out).shape == (0, M) and np.all(out == -7.25)
    unchanged(m, args)
    assert np.array_equal(m.sample(np.ones((2, nz))), good)
    g = _lib.Model(_lib.context(), _lib.SF, PW.HYP_SF, 1e-8)
    with pytest.raises(ValueError, match="no grid"):
        g.sample(np.zeros((1, 4)))


# ---- 6. the drop-in classes ------------------------------------------------------------------

def test_dropin_on_the_headline_grid():
    from mfgp_coverage_amd.gaussian_process import MFGP
    gx, gy, Xs = PW.lattice(128, 128)
    rng = np.random.default_rng(12)
    X = Xs[rng.choice(Xs.shape[0], 200, replace=False)]
    y = PW.field(X, rng).reshape(-1, 1)
    gp = MFGP(X[:60], y[:60], X[60:], y[60:], 1, 1)
    gp.hyp = PW.HYP_MF.copy()
    gp.updt_info(gp.X_L, gp.y_L, gp.X_H, gp.y_H)
    with pytest.raises(MemoryError):            # the dense route: 2 GiB of covariance
        gp.draw_posterior_samples(Xs, 2)
    F = gp.sample_posterior(Xs, 4, rng=np.random.default_rng(0))
    assert F.shape == (16384, 4) and np.all(np.isfinite(F))
    m = gp._dev()
    nz = m.sample_dims()["nz"]
    assert np.array_equal(F, m.sample(np.random.default_rng(0).standard_normal((4, nz))).T)
    mu, cov = gp.predict(Xs)                    # the zero-normal sample is predict's mean
    f0 = gp.sample_posterior(Xs, normals=np.zeros((1, nz)))[:, 0]
    assert O.parity_errors(f0, np.diag(cov), mu[:, 0], np.diag(cov), O.prior_variance(PW.HYP_MF))[0] <= TOL
    P = gp.sample_prior(Xs, 3, rng=np.random.default_rng(1))
    assert P.shape == (16384, 3) and np.all(np.isfinite(P))
    # method="pathwise" draws from numpy's global generator, as the dense route does
    np.random.seed(5)
    a = gp.draw_posterior_samples(Xs, 2, method="pathwise")
    p = gp.draw_prior_samples(Xs, 2, method="pathwise")
    np.random.seed(5)
    assert np.array_equal(gp.draw_posterior_samples(Xs, 2, method="pathwise"), a)
    assert np.array_equal(gp.draw_prior_samples(Xs, 2, method="pathwise"), p)
    np.random.seed(5)
    assert np.array_equal(a, m.sample(np.random.standard_normal((2, nz))).T)
    with pytest.raises(ValueError, match="method"):
        gp.draw_posterior_samples(Xs, 1, method="sparse")


def test_dropin_dense_default_and_no_lattice():
    from mfgp_coverage_amd.gaussian_process import SFGP
    gx, gy, Xs = PW.lattice(9, 7)
    rng = np.random.default_rng(13)
    X = Xs[rng.choice(Xs.shape[0], 30, replace=False)]
    y = PW.field(X, rng).reshape(-1, 1)
    gp = SFGP(X, y, 1)
    gp.hyp = PW.HYP_SF.copy()
    gp.updt_info(gp.X, gp.y)
    # the default is the dense route, bit for bit what it was: numpy's draw of the dense covariance
    np.random.seed(3)
    d = gp.draw_posterior_samples(Xs, 2)
    np.random.seed(3)
    assert np.array_equal(gp.draw_posterior_samples(Xs, 2, method="dense"), d)
    mu, cov = gp.predict(Xs)
    np.random.seed(3)
    with np.errstate(all="ignore"):
        want = np.random.multivariate_normal(mu.flatten(), np.asarray(cov), 2).T
    assert np.array_equal(d, want)
    assert gp.sample_posterior(Xs, 3, rng=np.random.default_rng(0)).shape == (63, 3)
    # off the lattice: a ValueError that names the dense route
    Xj = Xs + 1e-3 * rng.standard_normal(Xs.shape)
    with pytest.raises(ValueError, match="draw_posterior_samples"):
        gp.sample_posterior(Xj, 1)
    assert gp.draw_posterior_samples(Xj, 1).shape == (63, 1)
