"""Who holds the library's device and pinned memory: every buffer of a context, a model
or a record is owned by one object that frees it (csrc/mfgp_own.h), and the library counts
what it holds (mfgp_debug_live -> _lib.live_allocations()). The counter is the library's
own, so other users of the GPU do not enter it.

test_everything_returns: a round that reaches every buffer -- the lattice step's state, a
capacity growth that moves F, the tables, V and the column store, a clone, the look-ahead
and sample records, both NLML scratches, the planners' workspace, a result buffer handed out
as a view, a new grid -- leaves nothing behind: after the second round the four counts are
exactly those after the first (the warm-up: the context's rings persist by design).

test_failed_growth_leaves_the_model: a set_data whose factor alone is twice the card is
refused by the allocator with an error code before anything is launched (no kernel runs on a
bad pointer). The call raises, the library holds what it held before, the model predicts the
bits it predicted before, HIP's last-error word is clear for the next user of the runtime
in the process (PyTorch), and the model still appends and agrees with the CPU oracle. The
same on a clone of the model. (fp64 models: PARITY_TOL is the fp64 bound.)
"""
import gc

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

HYP_SF = np.array([0.0001, -2.797478161, -1.500619305, -4.6])
HYP_MF = np.array([0.16, -2.03, -0.63, 0.0001, -3.1, -1.52, -0.65, -5.0, -2.0])
GX = GY = 12      # the lattice grid
N0, K, APPENDS = 40, 8, 3   # 40 rows, then 8 more three times: 64 rows cross the first capacity of 63
NL = 16           # MF: the lofi rows among the first 40


def _grid(nx, ny):
    ax, ay = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
    return np.array([(a, b) for a in ax for b in ay])


def _field(X):
    return 0.5 + 0.4 * np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1])


def _data(kind):
    """Distinct cells of the 12 x 12 grid in a fixed random order, with a smooth field."""
    xs = _grid(GX, GY)
    X = xs[np.random.default_rng(5).permutation(GX * GY)[:N0 + K * APPENDS]]
    y = _field(X) + 0.01 * np.random.default_rng(6).standard_normal(X.shape[0])
    nl = NL if kind == "mf" else 0
    return xs, X, y, nl


def _new(ctx, kind, dtype):
    from mfgp_coverage_amd import _lib
    xs, X, y, nl = _data(kind)
    m = _lib.Model(ctx, _lib.MF if kind == "mf" else _lib.SF, HYP_MF if kind == "mf" else HYP_SF, 1e-8, dtype=dtype)
    m.set_grid(xs)
    m.set_data(X[:nl], y[:nl], X[nl:N0], y[nl:N0])
    return m


def _oracle(kind, X, y, nl, xs):
    if kind == "mf":
        return O.mf_diag(X[:nl], y[:nl], X[nl:], y[nl:], HYP_MF, xs)
    return O.sf_diag(X, y, HYP_SF, xs)


def _round(ctx, kind, dtype):
    from mfgp_coverage_amd import _lib
    f64 = dtype == _lib.F64
    hyp = HYP_MF if kind == "mf" else HYP_SF
    xs, X, y, nl = _data(kind)
    m = _new(ctx, kind, dtype)
    m.predict()
    for a in range(APPENDS):   # the third crosses the capacity: F, the tables, V and the column store move
        lo = N0 + K * a
        m.append(X[lo:lo + K], y[lo:lo + K])
        m.predict()
    st = m.stats()
    print(kind, "f64" if f64 else "f32", "stats:", st)
    assert m.n == N0 + K * APPENDS > 63
    assert st["lattice"] >= 2 and st["lattice_vcol"] >= 1, st   # the lattice state and the store were in use
    c = m.clone()
    c.predict()
    m.query(xs[:5] + 0.013, XH_new=xs[[7, 100]] + 0.021)
    if f64:   # (sample and plan_ivr serve fp64 models)
        m.sample(np.random.default_rng(7).standard_normal((3, m.sample_dims()["nz"])))
    m.nlml(hyp, grad=True)
    m.nlml_batch(np.stack([hyp, hyp - 0.05, hyp + 0.05]), grad=True)
    if f64:
        m.plan_ivr(5)
    _, var = m.predict()
    m.sample_points(0.5 * float(var.max()), 6)
    mu_v, var_v = m.predict_view()
    del mu_v, var_v
    m.set_grid(_grid(9, 16))
    m.predict()
    del m, c
    gc.collect()
    ctx.trim()
    return _lib.live_allocations()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["mf", "sf"])
def test_everything_returns(kind, dtype):
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_lattice("force")
    dt = _lib.F64 if dtype == "f64" else _lib.F32
    first = _round(ctx, kind, dt)    # the warm-up: the context's rings and status words stay
    second = _round(ctx, kind, dt)
    print("live after round 1:", first, "after round 2:", second)
    assert second == first


def _refused_growth(m, kind, rows_before):
    """The provoking call and what must hold after it, on model m holding rows_before."""
    import torch
    from mfgp_coverage_amd import _lib
    xs, X, y, nl = _data(kind)
    mu0, var0 = (a.copy() for a in m.predict())
    total = torch.cuda.mem_get_info()[1]
    # ld = round_up(N + 1, 64) >= N + 1: 8 ld^2 >= 2 total. The allocator refuses the factor
    # with an error code; X, y, z and the append scratch before it are ~22 N doubles < 100 MB.
    N = int(np.ceil(np.sqrt(2.0 * total / 8.0)))
    assert 8 * (N + 1) ** 2 >= 2 * total and 22 * 8 * N < 100e6
    XH = np.zeros((N, 2))
    yH = np.zeros(N)
    live = _lib.live_allocations()
    serial = m.serial()
    try:
        m.set_data(np.empty((0, 2)), np.empty(0), XH, yH)
    except RuntimeError as e:
        msg = str(e)
    else:
        pytest.fail("DID NOT RAISE RuntimeError")
    print("refused:", msg)
    after = _lib.live_allocations()
    print("live before:", live, "after:", after)
    assert after == live
    assert m.n == rows_before and m.serial() == serial
    mu1, var1 = m.predict()
    np.testing.assert_array_equal(mu1, mu0)
    np.testing.assert_array_equal(var1, var0)
    torch.cuda.synchronize()   # the last-error word was cleared: the next user of the runtime sees none
    t = torch.arange(8, device="cuda", dtype=torch.float64) * 2.0
    assert float(t.sum().item()) == 56.0
    m.append(X[N0:N0 + K], y[N0:N0 + K])
    mu, var = m.predict()
    mu_r, var_r = _oracle(kind, X[:N0 + K], y[:N0 + K], nl, xs)
    e = O.parity_errors(mu, var, mu_r, var_r, O.prior_variance(HYP_MF if kind == "mf" else HYP_SF))
    print("parity after the refused growth (mu, var):", e)
    assert max(e) < O.PARITY_TOL, e


@pytest.mark.parametrize("kind", ["mf", "sf"])
def test_failed_growth_leaves_the_model(kind):
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_lattice("force")
    m = _new(ctx, kind, _lib.F64)
    m.predict()
    c = m.clone()
    _refused_growth(m, kind, N0)
    _refused_growth(c, kind, N0)
