"""Covariance products from the resident V (k_cov_dot, k_cov_apply; mfgp_cov_apply) and the
greedy integrated-variance planner on top of them (k_ivr_pick; mfgp_plan_ivr; DESIGN.md
section 21).

The reference is tests/_plan_ivr.py on the oracle's dense covariance. Products:
    max |got - ref| / max(|ref|, 1e-6 k** sum|x|) <= O.PARITY_TOL.
The planner: for every pick t, with ref_t the oracle's from-scratch scores given the
device's picks before it,
    |gains[t] - ref_t[cell_t]| / max(|ref_t[cell_t]|, floor) <= PARITY_TOL
    ref_t[cell_t] >= max_allowed ref_t - PARITY_TOL max(max ref_t, floor)
(_ivr.err's floor). Picks are never compared with a reference's picks: symmetric grids give
exact ties. Comparisons between calls on one model are bit for bit.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _ivr as I
from tests import _plan_ivr as P

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = ["9x7", "13x11", "40x33", "16x40_yo", "13x11_xrev"]   # M = 63, 143, 1320 (3 segments), 640, 143
NPICK = 40      # crosses the 32-iteration chunk


def _build(ctx, kind, Xs, X, y, NL, dtype=None):
    from mfgp_coverage_amd import _lib
    if X.shape[0] == 0:      # a model that never saw data: a grid, no factor
        m = _lib.Model(ctx, _lib.SF if kind == "sf" else _lib.MF, I.hyp_of(kind), 1e-8)
        m.set_grid(Xs)
        return m
    return I._model(ctx, kind, X, y, NL, Xs, dtype=dtype)


_CASES = {}


def _case(kind, gname, N):
    """One model per (kind, grid, N), its data and the oracle's dense covariance: computed
    once, shared, never modified (the planner leaves its model as it was)."""
    key = (kind, gname, N)
    if key not in _CASES:
        from mfgp_coverage_amd import _lib
        Xs = P.extra_grid(gname)
        X, y, NL = I.data(kind, Xs, N, seed=7 + N + len(gname) + len(kind))
        m = _build(_lib.context(), kind, Xs, X, y, NL)
        C = I.dense_cov(kind, X, y, NL, Xs, I.hyp_of(kind))
        C.flags.writeable = False
        _CASES[key] = (m, C, Xs, X, y, NL)
    return _CASES[key]


def _vectors(M, seed):
    rng = np.random.default_rng(seed)
    ws = I.weight_sets(M, seed)
    unit = np.zeros(M)
    unit[(5 * M) // 7] = 1.0
    x3 = np.stack((rng.standard_normal(M), unit, ws["mask"]))
    x8 = np.vstack((x3, rng.standard_normal((5, M)) * (rng.random((5, M)) < 0.5)))
    return {"random": x3[0], "unit": unit, "mask": ws["mask"], "x3": x3, "x8": x8}


# ---- 1. cov_apply against dense_cov @ x ----------------------------------------------------------

@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("gname", LATTICES + ["scatter150"])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 197])
def test_cov_apply_against_the_dense_product(kind, gname, N):
    m, C, Xs, X, y, NL = _case(kind, gname, N)
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    lat = m.stats()["lattice_nx"]
    assert (lat == 0) == (gname == "scatter150")       # the scattered grid takes the general K** form
    xs = _vectors(M, seed=11 + N)
    worst, got = {}, {}
    for name, x in xs.items():
        got[name] = m.cov_apply(x)
        assert got[name].shape == x.shape
        worst[name] = P.apply_err(got[name], (C @ x.T).T if x.ndim == 2 else C @ x, hyp, x)
    print(f"cov_apply {kind} {gname} N = {N}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL, worst
    # a column of a multi-column call is the single call, bit for bit; two calls agree
    for k, name in enumerate(("random", "unit", "mask")):
        assert np.array_equal(got["x3"][k], got[name]) and np.array_equal(got["x8"][k], got[name]), name
    assert np.array_equal(m.cov_apply(xs["x8"]), got["x8"])
    # the prior's product, and a unit vector against the covariance block's column
    pr = m.cov_apply(xs["x3"], prior=True)
    assert P.apply_err(pr, (I.prior_cov(kind, Xs, hyp) @ xs["x3"].T).T, hyp, xs["x3"]) <= TOL
    if N == 0:
        assert np.array_equal(pr, got["x3"])
    c = (5 * M) // 7
    assert P.apply_err(got["unit"], m.cov_block(None, [c])[:, 0], hyp, xs["unit"]) <= TOL


def test_cov_apply_device_vectors_and_output_equal_host():
    import torch
    m, C, Xs, X, y, NL = _case("mf", "40x33", 197)
    M = Xs.shape[0]
    x = _vectors(M, seed=21)["x3"]
    want = m.cov_apply(x)
    xd = torch.zeros((3, M + 8), dtype=torch.float64, device="cuda")
    xd[:, :M] = torch.from_numpy(x).cuda()
    od = torch.full((3, M + 2), -1.5, dtype=torch.float64, device="cuda")
    assert m.cov_apply(xd[:, :M], out=od[:, :M]) is None
    h = od.cpu().numpy()
    assert np.array_equal(h[:, :M], want) and np.all(h[:, M:] == -1.5)
    out = np.full((3, M + 2), -7.25)
    r = m.cov_apply(x, out=out[:, :M])
    assert np.array_equal(r, want) and np.all(out[:, M:] == -7.25)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import _ivr as I
from tests import _plan_ivr as P
from mfgp_coverage_amd import _lib
Xs = P.extra_grid("13x11")
X, y, NL = I.data("mf", Xs, 65, seed=31)
m = I._model(_lib.context(), "mf", X, y, NL, Xs)
x = np.load(sys.argv[2])
cells, pts, gains = m.plan_ivr(6, weights=x[2])
np.savez(sys.argv[3], u=m.cov_apply(x), cells=cells, gains=gains)
"""


def test_the_general_form_agrees_with_the_separable_one(tmp_path):
    """MFGP_PLAN_SEP=0 (read when the context is created) in a fresh child process: the
    general K** x on a lattice grid agrees with the default within PARITY_TOL."""
    from mfgp_coverage_amd import _lib
    Xs = P.extra_grid("13x11")
    M = Xs.shape[0]
    hyp = I.hyp_of("mf")
    X, y, NL = I.data("mf", Xs, 65, seed=31)
    m = I._model(_lib.context(), "mf", X, y, NL, Xs)
    x = _vectors(M, seed=32)["x3"]
    np.save(tmp_path / "x.npy", x)
    u = m.cov_apply(x)
    cells, _, gains = m.plan_ivr(6, weights=x[2])
    env = dict(os.environ, MFGP_PLAN_SEP="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "x.npy"), str(tmp_path / "o.npz")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    o = np.load(tmp_path / "o.npz")
    e = P.apply_err(o["u"], u, hyp, x)
    print(f"general against separable K** x: {e:.3e}")
    assert e <= TOL
    eg, em, _ = P.check_run("mf", X, y, NL, Xs, hyp, x[2], o["cells"], o["gains"])
    assert eg <= TOL and em <= TOL
    assert np.max(np.abs(o["gains"] - gains) / np.maximum(np.abs(gains), P.pick_floor(hyp, x[2], M))) <= TOL


def test_cov_apply_after_every_update_path():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    Xs = I.grid("24x24")
    M = Xs.shape[0]
    Xall, yall = I._distinct(Xs, 260, seed=61)
    NL, n = 60, 150
    X, y = Xall[:n].copy(), yall[:n].copy()
    hyp = I.HYP_MF
    m = I._model(ctx, "mf", X, y, NL, Xs)
    x = _vectors(M, seed=62)["x3"]
    nxt = [n]

    def take(k):
        a = nxt[0]
        nxt[0] += k
        return Xall[a:a + k], yall[a:a + k]

    def check(tag):
        ref = (I.dense_cov("mf", X, y, NL, Xs, hyp) @ x.T).T
        e = P.apply_err(m.cov_apply(x), ref, hyp, x)
        print(f"cov_apply after {tag}: N = {X.shape[0]}, error {e:.3e}")
        assert e <= TOL, tag

    check("a full factor")
    ctx.set_lattice(False)                       # a one-row append on the V stream
    Xa, ya = take(1)
    m.predict()
    vs = m.stats()["vstream"]
    m.append(Xa, ya)
    m.predict()
    X, y = np.vstack((X, Xa)), np.concatenate((y, ya))
    assert m.stats()["vstream"] == vs + 1 and m.stats()["lattice"] == 0
    check("the V stream")
    ctx.set_lattice("force")                     # a lattice step
    Xa, ya = take(8)
    m.append(Xa, ya)
    m.predict()
    X, y = np.vstack((X, Xa)), np.concatenate((y, ya))
    assert m.stats()["lattice"] == 1, m.stats()
    check("the lattice step")
    ctx.set_lattice(True)
    keep = X.shape[0] - NL - 30                  # truncate: V's rows past N are stale
    m.truncate(keep)
    X, y = X[:NL + keep], y[:NL + keep]
    check("truncate")
    ctx.set_deferred_appends(True)               # a deferred append that the call itself settles
    Xa, ya = take(3)
    m.predict()
    m.append(Xa, ya)
    X, y = np.vstack((X, Xa)), np.concatenate((y, ya))
    assert m.stats()["v_rows"] == X.shape[0] - 3
    check("a deferred append")
    assert m.stats()["v_rows"] == X.shape[0] and m.stats()["factor_rows"] == X.shape[0]
    ctx.set_deferred_appends(False)


# ---- 2. the planner against the oracle --------------------------------------------------------------

def _cand40(M, seed):
    return np.random.default_rng(seed).choice(M, 40, replace=False)


def _run_and_check(kind, gname, N, wname, cand, n_points=NPICK, **kw):
    m, C, Xs, X, y, NL = _case(kind, gname, N)
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    w = P.weights(wname, M)
    cells, pts, gains = m.plan_ivr(n_points, weights=w, cand=cand, **kw)
    assert cells.shape == (n_points,) and pts.shape == (n_points, 2) and gains.shape == (n_points,)
    assert np.array_equal(pts, Xs[cells])
    if cand is not None:
        assert set(cells.tolist()) <= set(np.asarray(cand).tolist())     # no cell outside the list
    eg, em, gaps = P.check_run(kind, X, y, NL, Xs, hyp, w, cells, gains, cand)
    print(f"plan_ivr {kind} {gname} N = {N} {wname} {'all' if cand is None else 'list'}: "
          f"gain error {eg:.3e}, shortfall {em:.3e}")
    assert eg <= TOL and em <= TOL, (eg, em)
    return m, cells, gains, gaps


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("gname", LATTICES)
@pytest.mark.parametrize("N", P.NS)
@pytest.mark.parametrize("wname", ["ones", "mask"])
@pytest.mark.parametrize("listed", [False, True], ids=["all", "list40"])
def test_planner_against_the_oracle(kind, gname, N, wname, listed):
    m, C, Xs, X, y, NL = _case(kind, gname, N)
    M = Xs.shape[0]
    cand = _cand40(M, seed=N + M) if listed else None
    _run_and_check(kind, gname, N, wname, cand)


@pytest.mark.parametrize("kind", P.KINDS)
def test_appended_rows_cross_row_64(kind):
    _run_and_check(kind, "13x11", 60, "ones", None)


def test_first_gain_is_the_variance_reduction_maximum_and_min_gain_stops_the_run():
    m, cells, gains, _ = _run_and_check("mf", "40x33", 197, "mask", None, n_points=12)
    M = 1320
    hyp = I.hyp_of("mf")
    w = P.weights("mask", M)
    _, best, _ = m.var_reduction(weights=w, with_best=True)
    assert abs(gains[0] - best) / max(abs(best), P.pick_floor(hyp, w, M)) <= TOL
    # a threshold between two of the run's recorded gains stops the run exactly there
    tested = 0
    for t in range(1, 12):
        lo = gains[:t].min()
        if not gains[t] < lo:
            continue
        c2, p2, g2 = m.plan_ivr(12, weights=w, min_gain=0.5 * (gains[t] + lo))
        assert c2.shape == (t,) and np.array_equal(c2, cells[:t]) and np.array_equal(g2, gains[:t]), t
        tested += 1
    assert tested >= 3, gains
    c0, p0, g0 = m.plan_ivr(12, weights=w, min_gain=2.0 * gains[0])
    assert c0.shape == (0,) and p0.shape == (0, 2) and g0.shape == (0,)


# ---- 3. refresh ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("gname", ["13x11", "40x33"])
def test_refresh(kind, gname):
    """refresh = 1 is the from-scratch route on the device; the recurrence (refresh = 0) and
    refresh = 7 return its gains within PARITY_TOL, and its cells up to the first pick where
    the oracle's top two scores are closer than the tolerance."""
    m, C, Xs, X, y, NL = _case(kind, gname, 65)
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    w = P.weights("mask", M)
    n = 20
    c1, _, g1 = m.plan_ivr(n, weights=w, refresh=1)
    eg, em, gaps = P.check_run(kind, X, y, NL, Xs, hyp, w, c1, g1)
    assert eg <= TOL and em <= TOL
    tie = np.nonzero(gaps <= 2 * TOL)[0]
    upto = int(tie[0]) if tie.size else n
    fl = P.pick_floor(hyp, w, M)
    for R in (0, 7):
        c, _, g = m.plan_ivr(n, weights=w, refresh=R)
        assert np.array_equal(c[:upto], c1[:upto]), (R, upto)
        e = float(np.max(np.abs(g[:upto] - g1[:upto]) / np.maximum(np.abs(g1[:upto]), fl))) if upto else 0.0
        print(f"refresh {R} against 1, {kind} {gname}: {e:.3e} over {upto} picks")
        assert e <= TOL
        eg, em, _ = P.check_run(kind, X, y, NL, Xs, hyp, w, c, g)
        assert eg <= TOL and em <= TOL


# ---- 4. the model comes back unchanged ------------------------------------------------------------------

def _unchanged(ctx, Xs, X, y, NL, Xn, yn, n_points, w):
    from mfgp_coverage_amd import _lib
    a = I._model(ctx, "mf", X, y, NL, Xs)
    b = I._model(ctx, "mf", X, y, NL, Xs)
    for m in (a, b):
        m.predict()
    mu0, var0 = a.predict()
    st0 = a.stats()
    ps0 = ctx.planner_stats()
    r1 = a.plan_ivr(n_points, weights=w)
    assert r1[0].shape == (n_points,)
    ps1 = ctx.planner_stats()
    assert ps1["runs"] == ps0["runs"] + 1 and ps1["inc_factor"] == ps0["inc_factor"] + n_points
    assert ps1["vstream"] >= ps0["vstream"] + n_points
    assert a.stats() == st0 and a.n == X.shape[0]
    mu1, var1 = a.predict()
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    r2 = a.plan_ivr(n_points, weights=w)                       # a second call: the same bits
    assert all(np.array_equal(u, v) for u, v in zip(r1, r2))
    # a call that fails its validation leaves the model as it was
    with pytest.raises(ValueError, match="outside the grid"):
        a.plan_ivr(3, cand=[0, Xs.shape[0]])
    assert a.stats() == st0
    # the next batched step: the bits of a twin that never ran the planner
    import torch
    M = Xs.shape[0]
    outs = []
    for m in (a, b):
        xd, yd = torch.from_numpy(Xn).cuda(), torch.from_numpy(yn).cuda()
        mu, var = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(2))
        _lib.batch_append_predict([m], xd.data_ptr(), yd.data_ptr(), [Xn.shape[0]], mu.data_ptr(), var.data_ptr())
        outs.append((mu.cpu().numpy(), var.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    return a, r1


def test_the_model_comes_back_unchanged():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    Xs = I.grid("40x33")
    Xall, yall = I._distinct(Xs, 204, seed=71)
    w = P.weights("mask", Xs.shape[0])
    _, (cells, _, gains) = _unchanged(ctx, Xs, Xall[:200], yall[:200], 60, Xall[200:], yall[200:], NPICK, w)
    eg, em, _ = P.check_run("mf", Xall[:200], yall[:200], 60, Xs, I.HYP_MF, w, cells[:6], gains[:6])
    assert eg <= TOL and em <= TOL


def test_the_headline_model_comes_back_unchanged():
    """128 x 128, N = 2048 MF, 8 picks: the model is as before, two calls agree, and the first
    gain is var_reduction's maximum."""
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    g = np.linspace(0.0, 1.0, 128)
    Xs = np.array([(a, b) for a in g for b in g])
    Xall, yall = I._distinct(Xs, 2052, seed=81)
    m, r = _unchanged(ctx, Xs, Xall[:2048], yall[:2048], 1024, Xall[2048:], yall[2048:], 8, None)
    m.truncate(1024)                                      # back to the planner's rows
    _, best, pos = m.var_reduction(with_best=True)
    assert abs(r[2][0] - best) <= TOL * abs(best)
    assert np.all(np.isfinite(r[2])) and np.all(np.diff(r[2]) < 0)


# ---- 5. the scattered grid --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("N", P.NS)
def test_planner_on_a_scattered_grid(kind, N):
    m, cells, gains, _ = _run_and_check(kind, "scatter150", N, "mask", None)
    assert m.stats()["lattice_nx"] == 0


# ---- 6. errors ---------------------------------------------------------------------------------------------

def test_errors_leave_the_model_usable():
    from mfgp_coverage_amd import _lib
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    X, y = I._distinct(Xs, 70, seed=91)
    ctx = _lib.Context(0)
    m = I._model(ctx, "sf", X, y, 0, Xs)
    x = _vectors(M, seed=92)["x3"]
    good = m.cov_apply(x)
    plan = m.plan_ivr(5, weights=x[2])
    st, se = m.stats(), m.serial()
    L = _lib.lib()
    buf = np.ones((9, M))
    out = np.zeros((9, M))
    cells, pts, gains, cnt = np.zeros(4, dtype=np.int64), np.zeros((4, 2)), np.zeros(4), ctypes.c_int64(0)

    def vp(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def apply_raw(nx, ldx, ldo):
        return L.mfgp_cov_apply(m.handle, vp(buf), nx, ldx, vp(out), ldo, 0)

    def plan_raw(w=None, ldw=M, cand=None, nc=M, n=4, refresh=0):
        ca = None if cand is None else np.asarray(cand, dtype=np.int64)
        return L.mfgp_plan_ivr(m.handle, vp(w), ldw, vp(ca), nc, n, 0.0, refresh, vp(cells), vp(pts), vp(gains),
                               ctypes.byref(cnt))
    for nx in (0, 9):
        with pytest.raises(ValueError, match="nx"):
            _lib.check(apply_raw(nx, M, M))
    with pytest.raises(ValueError, match="nx"):
        m.cov_apply(buf)
    with pytest.raises(ValueError, match="ldx"):
        _lib.check(apply_raw(2, M - 1, M))
    with pytest.raises(ValueError, match="ldo"):
        _lib.check(apply_raw(2, M, M - 1))
    with pytest.raises(ValueError):
        m.cov_apply(np.ones(M - 1))
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[1, M - 1] = bad
        with pytest.raises(ValueError, match="finite"):
            m.cov_apply(xb)
        with pytest.raises(ValueError, match="finite"):
            m.plan_ivr(3, weights=xb[1])
    with pytest.raises(ValueError, match="ldw"):
        _lib.check(plan_raw(w=buf[0], ldw=M - 1))
    for cand in ([-1], [M], [0, M, 1]):
        with pytest.raises(ValueError, match="outside the grid"):
            m.plan_ivr(3, cand=cand)
    with pytest.raises(ValueError, match="n_points"):
        m.plan_ivr(-1)
    with pytest.raises(ValueError, match="refresh"):
        m.plan_ivr(3, refresh=-1)
    with pytest.raises(ValueError, match="all"):
        _lib.check(plan_raw(cand=None, nc=3))
    ctx.set_incremental(False)
    with pytest.raises(ValueError, match="incremental"):
        m.plan_ivr(3)
    ctx.set_incremental(True)
    e = m.plan_ivr(0)
    assert e[0].shape == (0,) and e[1].shape == (0, 2) and e[2].shape == (0,)
    assert m.plan_ivr(3, cand=[])[0].shape == (0,)
    assert m.stats() == st and m.serial() == se
    assert np.array_equal(m.cov_apply(x), good)
    assert all(np.array_equal(u, v) for u, v in zip(m.plan_ivr(5, weights=x[2]), plan))
    g = _lib.Model(ctx, _lib.SF, I.HYP_SF, 1e-8)
    with pytest.raises(ValueError):
        g.cov_apply(np.ones(3))
    with pytest.raises(ValueError, match="no grid"):
        g.plan_ivr(3)


def test_f32_models_raise():
    from mfgp_coverage_amd import _lib
    from mfgp_coverage_amd.gaussian_process import SFGP
    from mfgp_coverage_amd.planners import compute_sample_points_ivr
    Xs = I.grid("13x11")
    X, y = I._distinct(Xs, 40, seed=93)
    m = I._model(_lib.context(), "sf", X, y, 0, Xs, dtype=_lib.F32)
    m.predict()
    with pytest.raises(ValueError, match="MFGP_F32"):
        m.cov_apply(np.ones(Xs.shape[0]))
    with pytest.raises(ValueError, match="MFGP_F32"):
        m.plan_ivr(3)
    gp = SFGP(X, y.reshape(-1, 1), 1)
    gp.precision = "f32"
    gp.hyp = I.HYP_SF
    gp.updt_info(gp.X, gp.y)
    with pytest.raises(TypeError):
        compute_sample_points_ivr(gp, Xs, 3)
    with pytest.raises(TypeError):
        gp.predict(Xs)[1].apply(np.ones(Xs.shape[0]))


# ---- 7. the drop-in classes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", P.KINDS)
def test_dropin_apply_and_planner(kind):
    from mfgp_coverage_amd.gaussian_process import MFGP, SFGP
    from mfgp_coverage_amd.planners import compute_sample_points_ivr
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    X, y = I._distinct(Xs, 90, seed=95)
    y2 = y.reshape(-1, 1)
    NL = 0 if kind == "sf" else 30
    if kind == "sf":
        gp = SFGP(X, y2, 1)
        gp.hyp = hyp.copy()
        gp.updt_info(gp.X, gp.y)
    else:
        gp = MFGP(X[:NL], y2[:NL], X[NL:], y2[NL:], 1, 1)
        gp.hyp = hyp.copy()
        gp.updt_info(gp.X_L, gp.y_L, gp.X_H, gp.y_H)
    C = I.dense_cov(kind, X, y, NL, Xs, hyp)
    mu, cov = gp.predict(Xs)
    x = _vectors(M, seed=96)["x3"]
    u1 = cov.apply(x[0])
    assert u1.shape == (M,) and np.array_equal(u1, gp._dev().cov_apply(x[0]))
    u3 = cov.apply(x.T)
    assert u3.shape == (M, 3) and np.array_equal(u3[:, 0], u1)
    assert P.apply_err(u3.T, (C @ x.T).T, hyp, x) <= TOL
    dense = np.asarray(cov)                               # __array__ and @ stay as they were
    assert dense.shape == (M, M) and np.array_equal(cov @ x[0], dense @ x[0])
    w = I.weight_sets(M, seed=97)["mask"]
    pts, gains = compute_sample_points_ivr(gp, Xs, 10, weights=w, candidates=list(range(20, 120)))
    assert pts.shape == (10, 2) and gains.shape == (10,)
    cells = np.array([int(np.nonzero((Xs == p).all(1))[0][0]) for p in pts])
    eg, em, _ = P.check_run(kind, X, y, NL, Xs, hyp, w, cells, gains, np.arange(20, 120))
    assert eg <= TOL and em <= TOL
    mu2, cov2 = gp.predict(Xs)                           # the model is unchanged, the holder stale
    assert np.array_equal(mu, mu2) and np.array_equal(np.diag(cov), np.diag(cov2))
    with pytest.raises(RuntimeError):
        cov.apply(x[0])
    assert cov2.apply(x[0]).shape == (M,)
