"""The planners' error paths (mfgp_sample_points / mfgp_batch_sample_points): a loop
that fails inside -- a 1-row append whose Schur complement is not positive, or the
point cap -- must raise as the reference does (a LinAlgError from updt / updt_hifi
inside simulator.py:344-370) and leave the caller's model as it was: the reference
runs the loop on copy.deepcopy(model) (sim:339), here the loop runs on the model
itself and restores it.

The failing cases come from tests/_planner_cases.py (a gently negative jitter, so
that the pivot vmax - d * kss must cross zero before threshold 0 is reached);
tests/test_planner_failure_cases.py proves on the CPU oracle alone that they fail
where intended, by margins that rounding cannot cross. Only a non-positive pivot and
the point cap are forced here: both return an ordinary error code from launches
that complete.

"As it was" is checked the way test_batch_sample_points_leave_no_trace_headline
checks it after a success: the next predict returns the same bits, the path
counters and the row count are unchanged, nothing is left for a later
Context.synchronize to raise, a following append + predict gives the same bits as on
a twin that never met the planner (and agrees with the oracle), and the planner is
usable again.
"""
import re

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _planner_cases as P

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL
CAP = 4 * P.G * P.G + 1   # compute_sample_points' bound on a 24 x 24 grid


def _new(ctx, case, dtype=None):
    from mfgp_coverage_amd import _lib
    m = _lib.Model(ctx, _lib.SF if case.kind == "sf" else _lib.MF, case.hyp, case.jitter,
                   dtype=_lib.F64 if dtype is None else dtype)
    m.set_grid(case.xs)
    m.set_data(case.XL, case.yL, case.XH, case.yH)
    m.predict()
    m.predict()   # (a repeat predict streams the resident V, as in test_sample_points_vs_reference)
    return m


def _raises_not_pd(call):
    """call() must raise LinAlgError -> its message. (Not pytest.raises(...) as info: the
    kept traceback ties the caller's frame, its models and their context into a
    reference cycle, and the cycle collector may then destroy the context first.)"""
    try:
        call()
    except np.linalg.LinAlgError as e:
        return str(e)
    pytest.fail("DID NOT RAISE LinAlgError")


def _assert_named_row(case, n, msg):
    """The error names the first failing row (LAPACK's INFO, as np.linalg.cholesky of
    the whole matrix finds it), not a later one. Cases A and C fail at the oracle's
    step under every tie-break (test_failing_step_does_not_move_under_tie_breaks): the
    exact row n + i_fail + 1. Case B's step moves with the tie-break, inside the second
    chunk and before its last iteration (test_case_b_stays_inside_the_second_chunk_
    under_tie_breaks): n + 33 <= row < n + 64. A status word lost to the next launch's
    reset names the chunk's last row instead (n + 32 for A and C, n + 64 for B)."""
    row = int(re.search(r"leading minor of order (\d+)\)", msg).group(1))
    if case.name == "B":
        assert n + 33 <= row < n + 64, (row, n)
    else:
        assert row == n + case.i_fail + 1, (row, n, case.i_fail)


def _snapshot(m):
    mu, var = m.predict()
    return {"mu": mu.copy(), "var": var.copy(), "stats": m.stats(), "n": m.n}


def _assert_as_before(m, snap):
    mu, var = m.predict()
    np.testing.assert_array_equal(mu, snap["mu"])
    np.testing.assert_array_equal(var, snap["var"])
    assert m.stats() == snap["stats"]
    assert m.n == snap["n"]


def _assert_parity(case, XH, yH, mu, var, f32):
    mu_r, var_r = case.oracle(XH, yH)
    if f32:
        e = O.parity_errors_f32(mu, var, mu_r, var_r, case.kss)
        print("f32 parity (mu, var):", e, "smallest |var_ref| / kss:", float(np.abs(var_r).min() / case.kss))
        assert max(e) < O.F32_TOL, e
    else:
        e = O.parity_errors(mu, var, mu_r, var_r, case.kss)
        assert max(e) < TOL, e


def _assert_usable(case, m, twin, f32):
    """After the restore: 4 appended rows + predict give the twin's bits, a planner
    call above the max variance chooses nothing, and the step agrees with the oracle."""
    X, y = P.append_rows(case, 4)
    m.append(X, y)
    twin.append(X, y)
    mu, var = m.predict()
    mu_t, var_t = twin.predict()
    np.testing.assert_array_equal(mu, mu_t)
    np.testing.assert_array_equal(var, var_t)
    assert m.sample_points(2.0 * float(var.max()) + 1.0, 10).shape == (0, 2)
    _assert_parity(case, np.vstack([case.XH, X]), np.append(case.yH, y), mu, var, f32)


@pytest.fixture(scope="module")
def split_ctx():
    """Incremental, but appends and predicts as separate launch groups."""
    from mfgp_coverage_amd import _lib
    c = _lib.Context(0)
    c.set_fused(False)
    return c


@pytest.fixture(scope="module")
def fused_ctx():
    from mfgp_coverage_amd import _lib
    return _lib.Context(0)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_failing_loop_raises_and_restores(fused_ctx, split_ctx, name, dtype, fused):
    """(a) One model whose loop meets a non-positive pivot -- mid first chunk (A, C) or
    in the second chunk (B): LinAlgError, and the model is as before the call.

    The error names the first failing row (_assert_named_row: exactly for A and C, as
    a range for B, whose step depends on how near ties are broken). Before the select
    kernels read the status word the loop reported the chunk's LAST iteration instead
    (row 37 for A, 69 for B, 67 for C): every append resets the word, so the failing
    step's verdict was lost and the error surfaced only because the later iterations
    of the chunk, stepping on from the substituted pivot, failed too."""
    from mfgp_coverage_amd import _lib
    ctx = fused_ctx if fused else split_ctx
    case = P.build(name)
    dt = _lib.F32 if dtype == "f32" else _lib.F64
    m, twin = _new(ctx, case, dt), _new(ctx, case, dt)
    snap = _snapshot(m)
    twin.predict()
    ctx.planner_stats(reset=True)
    msg = _raises_not_pd(lambda: m.sample_points(0.0, P.MAX_ITERS))
    print("raised:", msg, "| oracle: step", case.i_fail, "= row", snap["n"] + case.i_fail + 1)
    _assert_named_row(case, snap["n"], msg)
    ctx.synchronize()   # nothing of the failed loop is left to raise
    _assert_as_before(m, snap)
    assert ctx.planner_stats()["runs"] == 1
    _assert_usable(case, m, twin, dtype == "f32")


def test_point_cap_raises_and_restores():
    """(b) 6 x 6 grid, threshold 0: compute_sample_points runs to its cap of 4 * 36 + 1 =
    145 points (every cell revisited, capacity grown across chunk boundaries) and
    refuses the truncated answer; the model is as before. The first 31 points are the
    31 cells that hold no row, each once (the CPU oracle's sequence, by a margin:
    test_cap_case_visits_every_free_cell_first; with 5 of the 36 cells holding a row
    the 32nd point is already a revisit), and every point is an argmax of the
    oracle's variance given the ones before it."""
    from mfgp_coverage_amd import gaussian_process as gp
    from mfgp_coverage_amd import _lib
    from mfgp_coverage_amd.planners import compute_sample_points
    case = P.build("CAP")

    def make():
        g = gp.SFGP(case.XH.copy(), case.yH.reshape(-1, 1).copy(), 1)
        g.hyp = case.hyp.copy()
        g.updt_info(g.X, g.y)
        g.predict(case.xs)
        g.predict(case.xs)
        return g

    g, gt = make(), make()
    assert g.jitter == 1e-8
    m, twin = g._dev(), gt._dev()
    ctx = _lib.context()
    snap = _snapshot(m)
    twin.predict()
    ctx.planner_stats(reset=True)
    with pytest.raises(RuntimeError, match="no convergence"):
        compute_sample_points(g, case.xs, 0.0, False)
    ctx.synchronize()
    _assert_as_before(m, snap)
    assert ctx.planner_stats()["runs"] == 1
    pts = m.sample_points(0.0, 145)
    assert pts.shape == (145, 2)
    _assert_as_before(m, snap)
    free = {tuple(r) for r in case.xs} - {tuple(r) for r in case.XH}
    assert {tuple(p) for p in pts[:31]} == free and len(free) == 31
    for i in range(145):
        _, var = case.oracle(np.vstack([case.XH, pts[:i]]), np.zeros(case.XH.shape[0] + i))
        j = np.flatnonzero((case.xs == pts[i]).all(1))
        assert j.size == 1
        vmax = var.max()
        assert var[j[0]] >= vmax - TOL * max(vmax, 1e-6 * case.kss), (i, var[j[0]], vmax)
    _assert_usable(case, m, twin, False)


def _first_difference(a, b):
    n = min(a.shape[0], b.shape[0])
    for i in range(n):
        if not np.array_equal(a[i], b[i]):
            return i
    return n


def _assert_same_points(case, XH0, pb, ps, thr):
    """The batched loop's points against the single-model loop's: equal, up to the
    first step that rounding decides (the two step forms round differently) -- there
    the oracle's two largest variances are within the parity tolerance."""
    i = _first_difference(pb, ps)
    if i < min(pb.shape[0], ps.shape[0]):
        XH = np.vstack([XH0, ps[:i]])
        _, var = case.oracle(XH, np.zeros(XH.shape[0]))
        top = np.sort(var)[-2:]
        assert top[1] - top[0] < TOL * max(top[1], 1e-6 * case.kss), (i, top)
    else:
        assert pb.shape[0] == ps.shape[0], (pb.shape, ps.shape)
        XH = np.vstack([XH0, pb])
        _, var = case.oracle(XH, np.zeros(XH.shape[0]))
        assert var.max() <= thr * (1 + TOL)


def _batch_step(models, rows):
    """One batched append + predict of one row per model -> (mu, var) of the batch."""
    import torch
    from mfgp_coverage_amd import _lib
    X = np.concatenate([r[0] for r in rows])
    y = np.concatenate([r[1] for r in rows])
    Xd = torch.tensor(X, dtype=torch.float64, device="cuda")
    yd = torch.tensor(y, dtype=torch.float64, device="cuda")
    M = sum(P.G * P.G for _ in models)
    mu = torch.empty(M, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mu)
    _lib.batch_append_predict(models, Xd.data_ptr(), yd.data_ptr(), [1] * len(models), mu.data_ptr(), var.data_ptr())
    return mu.cpu().numpy(), var.cpu().numpy()


def _batch_failure(names, factors, healthy, lattice):
    """names: the batch's cases; factors: each model's threshold as a fraction of its
    initial max variance (0: threshold 0, the failing member); healthy: the members
    that are also run alone."""
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    if lattice:
        ctx.set_lattice("force")
    cases = [P.build(n) for n in names]
    ms = [_new(ctx, c) for c in cases]
    twins = [_new(ctx, c) for c in cases]
    B = len(ms)
    rows = [P.append_rows(c, 2) for c in cases]
    extra = [np.empty((0, 2)) for _ in cases]   # rows appended by the steps below ...
    extra_y = [np.empty(0) for _ in cases]      # ... and their observations
    if lattice:
        # a forced lattice step first: the resident posterior, F and the tables exist.
        # The lattice step needs noise + jitter > 0 and the whole batch takes one step
        # form, so the negative-jitter member keeps any batch it is in on the V stream:
        # the forced variant covers the healthy members (their step here, and their
        # loop below).
        hm = [ms[b] for b in healthy]
        ht = [twins[b] for b in healthy]
        hr = [(rows[b][0][:1], rows[b][1][:1]) for b in healthy]
        ra, rb = _batch_step(hm, hr), _batch_step(ht, hr)
        np.testing.assert_array_equal(ra[0], rb[0])
        np.testing.assert_array_equal(ra[1], rb[1])
        for b in healthy:
            extra[b], extra_y[b] = rows[b][0][:1], rows[b][1][:1]
        assert all(m.stats()["lattice"] == 1 for m in hm), [m.stats() for m in hm]
    snaps = [_snapshot(m) for m in ms]
    for t in twins:
        t.predict()
    thr = [f * float(s["var"].max()) for f, s in zip(factors, snaps)]
    ctx.planner_stats(reset=True)
    msg = _raises_not_pd(lambda: _lib.batch_sample_points(ms, thr, P.MAX_ITERS))
    print("raised:", msg, "| planner paths:", ctx.planner_stats())
    bad = [b for b, c in enumerate(cases) if c.d > 0]
    assert len(bad) == 1   # the first failing row of the failing member, as in the single loop
    _assert_named_row(cases[bad[0]], snaps[bad[0]]["n"], msg)
    ctx.synchronize()   # the loop's deferred status entries are drained: nothing raises
    for m, s in zip(ms, snaps):
        _assert_as_before(m, s)   # the failing member too: it is still the valid model it was
    ps = ctx.planner_stats(reset=True)
    assert ps["runs"] == B, ps
    # one batch step of one row each: the same bits as on the twins
    step = [(r[0][1:2], r[1][1:2]) for r in rows]
    ra, rb = _batch_step(ms, step), _batch_step(twins, step)
    np.testing.assert_array_equal(ra[0], rb[0])
    np.testing.assert_array_equal(ra[1], rb[1])
    ctx.synchronize()
    M = P.G * P.G
    for b in range(B):
        # ... agrees with the oracle under the member's jitter (the failing member too),
        # and each member's planner is usable again
        extra[b], extra_y[b] = np.vstack([extra[b], step[b][0]]), np.append(extra_y[b], step[b][1])
        _assert_parity(cases[b], np.vstack([cases[b].XH, extra[b]]), np.append(cases[b].yH, extra_y[b]),
                       ra[0][b * M:(b + 1) * M], ra[1][b * M:(b + 1) * M], False)
        vtop = float(ra[1][b * M:(b + 1) * M].max())
        assert ms[b].sample_points(2.0 * vtop + 1.0, 10).shape == (0, 2)
    ctx.synchronize()
    assert ctx.planner_stats(reset=True)["runs"] == B   # (those calls)
    # the success path (its drain changed too): the healthy members alone, same thresholds.
    # With the australia8 hyperparameters (hifi noise 0.25) the thresholds the case sets,
    # 0.3 x and 0.5 x the initial max variance, take about 270 and 90 iterations on a
    # 24 x 24 grid whatever the row counts (40 + 12 ... 10 + 60 rows: 266 - 272 on the
    # oracle): more than the 200 iterations the failing calls are bounded by, so these
    # runs are bounded by compute_sample_points' own cap. Each still takes milliseconds.
    hm = [ms[b] for b in healthy]
    pb = _lib.batch_sample_points(hm, [thr[b] for b in healthy], CAP)
    ps = ctx.planner_stats(reset=True)
    assert ps["runs"] == len(healthy), ps
    if lattice:
        assert ps["lattice"] > 0, ps
    ctx.synchronize()
    for i, b in enumerate(healthy):
        single = ms[b].sample_points(thr[b], CAP)   # compute_sample_points' call ...
        assert 0 < single.shape[0] < CAP            # ... and its convergence check
        _assert_same_points(cases[b], np.vstack([cases[b].XH, extra[b]]), pb[i], single, thr[b])
    return ps


@pytest.mark.parametrize("lattice", [False, True])
def test_batch_one_member_fails(lattice):
    """(c) Three models on one context: case A (fails at step 19) between two healthy
    MF models of different sizes (thresholds 0.3 x and 0.5 x their initial max
    variance). The batch raises, nothing is left for Context.synchronize, all three
    models are as before, a batch step gives the twins' bits and the oracle's values,
    every member's planner is usable again, and the healthy pair alone still equals the
    single-model loop (about 270 and 90 iterations at these thresholds: see the note in
    _batch_failure). lattice: a context with the lattice
    step forced; the negative-jitter model is not eligible for it (noise + jitter < 0)
    and keeps its whole batch on the V stream, so the forced variant exercises the
    lattice step on the healthy members only."""
    _batch_failure(["H0", "A", "H1"], [0.3, 0.0, 0.5], [0, 2], lattice)


@pytest.mark.parametrize("lattice", [False, True])
def test_batch_failure_in_second_chunk(lattice):
    """(d) Case B (fails in the second chunk: at its 21st iteration on the oracle, a
    few steps earlier or later under other tie-breaks) with a healthy model of the same hyperparameters on other rows that is still running
    then (it needs more than 52 points): the same assertions as (c)."""
    _batch_failure(["B", "B2"], [0.0, 0.3], [1], lattice)
