"""One scripted life of a model that reaches every tag of the record of what its derived
buffers hold (csrc/mfgp_state.h): the factor, V, the compact rows, F, the tables, the column
store, both resident posterior buffers and the generation. 16 x 9 grid (M = 144, a lattice
with nx != ny), the lattice step forced on a private context, 56 rows to start with (MF:
16 of them lofi), MF and SF, fp64 and fp32 (plan_ivr serves fp64 models: its step is left
out of the fp32 lives). The steps, each followed by a predict() that reads the posterior
(but 4, 7 and 8):

   1 predict                       8 plan_ivr of 3 points (fp64)
   2 append 3 (lattice step)       9 set_hyp to a changed value
   3 append 8 (67 rows cross the   10 append 2
     first capacity of 63)         11 clone, append 1 to the clone
   4 batch step with k = 0         12 set_grid to 9 x 16
   5 truncate by 5                 13 predict
   6 append 5 other rows           14 append 1
   7 sample_points, 4 points

Steps 7 and 8 are read through the batch step of no rows instead (k_post_copy): a predict()
there returns the kept result of step 6 without touching the model, while the batch step
copies out the posterior buffers that the planner's loop overwrote and plan_leave copied
back. That is the one numeric check of the planner restore here (the restored V is seen by
its row count only); step 9 refactors from scratch.

After every step: stats() (all keys but early_pd, which counts eager appends that saw their
verdict within a 2 ms poll: timing by design) and the row counts of debug_read_v() /
debug_read_f() equal the literal tuples of EXPECT, recorded by running this script on the
library of the parent commit (the state as loose fields of mfgp_model), so the test passes on
both; mu / var agree with the CPU oracle at every cell (parity_errors < TOL: PARITY_TOL but
for SF fp32, see TOL); and with a fresh model given the same rows, bit for bit at the steps
where the parent is (BIT_EQUAL, from the same run: steps 1 and 9, which follow a factor and a
predict from scratch), within the same bound at the others. Measured maxima on an MI355X,
oracle | fresh, the same on both libraries: MF fp64 3.2e-15 | 1.7e-15, SF fp64 2.0e-14 |
9.8e-15, MF fp32 3.4e-7 | 3.4e-7, SF fp32 1.571e-6 | 1.571e-6. About 0.4 s a
case."""
import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

HYP = {"sf": np.array([0.0001, -2.797478161, -1.500619305, -4.6]),
       "mf": np.array([0.16, -2.03, -0.63, 0.0001, -3.1, -1.52, -0.65, -5.0, -2.0])}
GX, GY = 16, 9
N0, NL = 56, 16
STEPS = ("predict", "append 3", "append 8", "batch k=0", "truncate 5", "append 5 other", "sample_points 4",
         "plan_ivr 3", "set_hyp", "append 2", "clone + append 1", "set_grid 9x16", "predict again", "append 1")


def _grid(nx, ny):
    ax, ay = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
    return np.array([(a, b) for a in ax for b in ay])


def _rows():
    """Distinct cells of the 16 x 9 grid in a fixed random order, with a smooth field."""
    xs = _grid(GX, GY)
    X = xs[np.random.default_rng(11).permutation(GX * GY)[:90]]
    y = 0.5 + 0.4 * np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + 0.01 * np.random.default_rng(12).standard_normal(90)
    return X, y


def life(kind, dtype):
    """Runs the script; yields (step, observed tuple, oracle errors, errors against the fresh
    model, bit-equal to the fresh model) after every step."""
    import torch
    from mfgp_coverage_amd import _lib
    f64 = dtype == "f64"
    dt = _lib.F64 if f64 else _lib.F32
    nl = NL if kind == "mf" else 0
    knd = _lib.MF if kind == "mf" else _lib.SF
    ctx = _lib.Context(0)
    ctx.set_lattice("force")
    X, y = _rows()
    hyp = HYP[kind].copy()
    xs = _grid(GX, GY)
    errs = O.parity_errors
    keys = [k for k in _lib.Model.STATS_KEYS if k != "early_pd"]

    def oracle(Xc, yc):
        if kind == "mf":
            return O.mf_diag(Xc[:nl], yc[:nl], Xc[nl:], yc[nl:], hyp, xs)
        return O.sf_diag(Xc, yc, hyp, xs)

    def observe(step, mdl, Xc, yc, mu, var):
        st = mdl.stats()
        v, _vc, vcr = mdl.debug_read_v()
        seen = tuple(st[k] for k in keys) + (v.shape[0] if v.size else 0, vcr, mdl.debug_read_f().shape[0])
        assert mdl.n == Xc.shape[0]
        kss = O.prior_variance(hyp)
        e_or = errs(mu, var, *oracle(Xc, yc), kss)
        fresh = _lib.Model(ctx, knd, hyp, 1e-8, dtype=dt)
        fresh.set_grid(xs)
        fresh.set_data(Xc[:nl], yc[:nl], Xc[nl:], yc[nl:])
        mu_f, var_f = fresh.predict()
        same = bool(np.array_equal(mu, mu_f) and np.array_equal(var, var_f))
        return step, seen, e_or, errs(mu, var, mu_f, var_f, kss), same

    def grow(mdl, Xc, yc, more_X, more_y):
        mdl.append(more_X, more_y)
        return np.concatenate([Xc, more_X]), np.concatenate([yc, more_y])

    m = _lib.Model(ctx, knd, hyp, 1e-8, dtype=dt)
    m.set_grid(xs)
    Xc, yc = X[:N0], y[:N0]
    m.set_data(Xc[:nl], yc[:nl], Xc[nl:], yc[nl:])
    yield observe(1, m, Xc, yc, *m.predict())
    Xc, yc = grow(m, Xc, yc, X[56:59], y[56:59])
    yield observe(2, m, Xc, yc, *m.predict())
    Xc, yc = grow(m, Xc, yc, X[59:67], y[59:67])
    yield observe(3, m, Xc, yc, *m.predict())
    out = torch.zeros(2, xs.shape[0], dtype=torch.float64, device="cuda")

    def batch_k0():
        """The batch step that appends nothing: the resident posterior, copied out (k_post_copy)."""
        out.zero_()
        _lib.Batch([m], [0]).append_predict(0, 0, out[0].data_ptr(), out[1].data_ptr())
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()

    yield observe(4, m, Xc, yc, *batch_k0())
    m.truncate(Xc.shape[0] - nl - 5)
    Xc, yc = Xc[:-5], yc[:-5]
    yield observe(5, m, Xc, yc, *m.predict())
    Xc, yc = grow(m, Xc, yc, X[67:72], y[67:72])
    yield observe(6, m, Xc, yc, *m.predict())
    # (a predict() here would return the kept result of step 6: the batch step of no rows
    # reads the posterior buffers the planner's loop overwrote and plan_leave copied back)
    assert m.sample_points(0.0, 4).shape == (4, 2)
    yield observe(7, m, Xc, yc, *batch_k0())
    if f64:
        assert m.plan_ivr(3)[0].shape == (3,)
        yield observe(8, m, Xc, yc, *batch_k0())
    hyp = hyp + 0.05 * np.where(np.arange(hyp.shape[0]) == 1, 1.0, 0.0)
    m.set_hyp(hyp, 1e-8)
    yield observe(9, m, Xc, yc, *m.predict())
    Xc, yc = grow(m, Xc, yc, X[72:74], y[72:74])
    yield observe(10, m, Xc, yc, *m.predict())
    c = m.clone()
    Xk, yk = grow(c, Xc, yc, X[74:75], y[74:75])
    yield observe(11, c, Xk, yk, *c.predict())
    del c
    xs = _grid(9, 16)
    m.set_grid(xs)
    yield observe(12, m, Xc, yc, *m.predict())
    yield observe(13, m, Xc, yc, *m.predict())
    Xc, yc = grow(m, Xc, yc, X[75:76], y[75:76])
    yield observe(14, m, Xc, yc, *m.predict())


# (kind, dtype) -> step -> the observed tuple: stats() without early_pd in STATS_KEYS order,
# then (rows of V, valid rows of the column store, rows of F). Recorded on the parent commit.
EXPECT = {
    ("mf", "f64"): {
        1: (56, 56, 1, 0, 1, 0, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 56, 0, 0),
        2: (59, 59, 1, 1, 1, 1, 16, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 56, 59, 59, 59),
        3: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 0, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        4: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        5: (62, 62, 1, 2, 1, 3, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 62, 62, 62),
        6: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 1, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        7: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 2, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        8: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 3, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        9: (67, 67, 2, 3, 2, 4, 16, 9, 3, 0, 2, 0, 3, 0, 0, 0, 0, 3, 56, 67, 0, 0),
        10: (69, 69, 2, 4, 2, 5, 16, 9, 4, 0, 2, 0, 3, 0, 0, 0, 0, 4, 123, 69, 69, 69),
        11: (70, 70, 0, 1, 0, 1, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70, 0, 0),
        12: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 3, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        13: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 3, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        14: (70, 70, 2, 5, 3, 6, 9, 16, 5, 118, 2, 0, 3, 0, 0, 0, 0, 4, 192, 70, 70, 70),
    },
    ("mf", "f32"): {
        1: (56, 56, 1, 0, 1, 0, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 56, 0, 0),
        2: (59, 59, 1, 1, 1, 1, 16, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 56, 59, 59, 59),
        3: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 0, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        4: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        5: (62, 62, 1, 2, 1, 3, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 62, 62, 62),
        6: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 1, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        7: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 2, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        9: (67, 67, 2, 3, 2, 4, 16, 9, 3, 0, 2, 0, 2, 0, 0, 0, 0, 3, 56, 67, 0, 0),
        10: (69, 69, 2, 4, 2, 5, 16, 9, 4, 0, 2, 0, 2, 0, 0, 0, 0, 4, 123, 69, 69, 69),
        11: (70, 70, 0, 1, 0, 1, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70, 0, 0),
        12: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 2, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        13: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 2, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        14: (70, 70, 2, 5, 3, 6, 9, 16, 5, 118, 2, 0, 2, 0, 0, 0, 0, 4, 192, 70, 70, 70),
    },
    ("sf", "f64"): {
        1: (56, 56, 1, 0, 1, 0, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 56, 0, 0),
        2: (59, 59, 1, 1, 1, 1, 16, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 56, 59, 59, 59),
        3: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 0, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        4: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        5: (62, 62, 1, 2, 1, 3, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 62, 62, 62),
        6: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 1, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        7: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 2, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        8: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 3, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        9: (67, 67, 2, 3, 2, 4, 16, 9, 3, 0, 2, 0, 3, 0, 0, 0, 0, 3, 56, 67, 0, 0),
        10: (69, 69, 2, 4, 2, 5, 16, 9, 4, 0, 2, 0, 3, 0, 0, 0, 0, 4, 123, 69, 69, 69),
        11: (70, 70, 0, 1, 0, 1, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70, 0, 0),
        12: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 3, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        13: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 3, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        14: (70, 70, 2, 5, 3, 6, 9, 16, 5, 67, 2, 0, 3, 0, 0, 0, 0, 4, 192, 70, 70, 70),
    },
    ("sf", "f32"): {
        1: (56, 56, 1, 0, 1, 0, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 56, 0, 0),
        2: (59, 59, 1, 1, 1, 1, 16, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 56, 59, 59, 59),
        3: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 0, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        4: (67, 67, 1, 2, 1, 2, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 67, 67, 67),
        5: (62, 62, 1, 2, 1, 3, 16, 9, 2, 0, 1, 0, 1, 0, 0, 0, 0, 2, 56, 62, 62, 62),
        6: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 1, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        7: (67, 67, 1, 3, 1, 4, 16, 9, 3, 0, 2, 0, 2, 0, 0, 0, 0, 3, 56, 67, 67, 67),
        9: (67, 67, 2, 3, 2, 4, 16, 9, 3, 0, 2, 0, 2, 0, 0, 0, 0, 3, 56, 67, 0, 0),
        10: (69, 69, 2, 4, 2, 5, 16, 9, 4, 0, 2, 0, 2, 0, 0, 0, 0, 4, 123, 69, 69, 69),
        11: (70, 70, 0, 1, 0, 1, 16, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 70, 0, 0),
        12: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 2, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        13: (69, 69, 2, 4, 3, 5, 9, 16, 4, 0, 2, 0, 2, 0, 0, 0, 0, 4, 123, 69, 0, 0),
        14: (70, 70, 2, 5, 3, 6, 9, 16, 5, 67, 2, 0, 2, 0, 0, 0, 0, 4, 192, 70, 70, 70),
    },
}
# (kind, dtype) -> the steps whose posterior is the fresh model's bit for bit on the parent commit
BIT_EQUAL = {(kind, dtype): (1, 9) for kind in ("mf", "sf") for dtype in ("f64", "f32")}


# The bound on parity_errors, against the oracle and against the fresh model alike: PARITY_TOL
# wherever the parent commit meets it (fp64: 3.2e-15 MF, 2.0e-14 SF; MF fp32: 3.4e-7). SF
# fp32 does not, on the parent either (an fp32 V next to data, at var: 1.571e-6 at steps 6
# and 7): its bound is recorded, twice the parent's maximum.
TOL = {(kind, dtype): O.PARITY_TOL for kind in ("mf", "sf") for dtype in ("f64", "f32")}
TOL["sf", "f32"] = 2 * 1.571e-6


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["mf", "sf"])
def test_scripted_life(kind, dtype):
    tol = TOL[kind, dtype]
    expect, bit_equal = EXPECT[kind, dtype], BIT_EQUAL[kind, dtype]
    steps = []
    for step, seen, e_oracle, e_fresh, same in life(kind, dtype):
        print(f"{kind} {dtype} step {step:2d} ({STEPS[step - 1]}): {seen}",
              f"oracle {e_oracle} fresh {e_fresh} bit-equal {same}")
        steps.append(step)
        assert seen == expect[step], (step, seen, expect[step])
        assert max(e_oracle) < tol, (step, e_oracle)
        if step in bit_equal:
            assert same, (step, e_fresh)
        else:
            assert max(e_fresh) < tol, (step, e_fresh)
    assert steps == [s for s in range(1, 15) if dtype == "f64" or s != 8]
