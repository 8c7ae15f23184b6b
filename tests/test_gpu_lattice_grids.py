"""The lattice-separable step (k_inc_lat / k_lat_gemm2) on
grids that are not square (cases: tests/_lattice_grids.py, validated on the CPU
by tests/test_lattice_grid_cases.py).

Every other lattice test uses a square, uniform, increasing, x-outer grid, on
which a swapped nx / ny or sx / sy, a table indexed by the wrong axis, a tile
count from the wrong dimension or a Z-row bound taken from nx changes nothing.
Here: rectangles both ways round and in both cell orders (the per-rank grids of
the sharded mode among them), tabw = 192, a degenerate axis, reversed and warped
axes, rows off the grid along one coordinate, the kernel forms' bit-equalities,
one launch over different grids, the sharded slice against the whole grid, the
planner's loop, and an axis too long for the step (declined: the V stream). Every step is compared with the CPU oracle at every cell
(PARITY_TOL) and, where a V-stream model runs beside it, with the V stream of
the same library (1e-8); stats() asserts for every case which path ran.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _lattice_grids as G

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL


def _hyp(name):
    from mfgp_coverage_amd.synthetic import HYP
    return HYP[name].copy()


def _model(ctx, hyp, X, y, NL, Xs, dtype=None):
    from mfgp_coverage_amd import _lib
    kind = _lib.SF if hyp.shape[0] == 4 else _lib.MF
    m = _lib.Model(ctx, kind, hyp, 1e-8, dtype=_lib.F64 if dtype is None else dtype)
    m.set_grid(Xs)
    if kind == _lib.SF:
        m.set_data(np.empty((0, 2)), np.empty(0), X, y)
    else:
        m.set_data(X[:NL], y[:NL], X[NL:], y[NL:])
    return m


def _ref(hyp, X, y, NL, Xs):
    if hyp.shape[0] == 4:
        return O.sf_diag(X, y, hyp, Xs)
    return O.mf_diag(X[:NL], y[:NL], X[NL:], y[NL:], hyp, Xs)


def _err(hyp, mu, var, mu_r, var_r):
    return max(O.parity_errors(mu, var, mu_r, var_r, O.prior_variance(hyp)))


@pytest.fixture(scope="module")
def lctx():
    """A private context that takes the lattice step for these small batches too."""
    from mfgp_coverage_amd import _lib
    c = _lib.Context(0)
    c.set_lattice("force")
    return c


@pytest.fixture(scope="module")
def vctx():
    """A context without the lattice step: the V stream of the same library."""
    from mfgp_coverage_amd import _lib
    c = _lib.Context(0)
    c.set_lattice(False)
    return c


def _sequence(case, mf, lctx, vctx, declined=False):
    """n0 base rows, one full predict, appends of 8, 3 and 12 rows on the lattice
    context and on the V-stream one: each step against the oracle and the V stream,
    then the path counters, the detected axes, the virtual rows and the factor."""
    hyp = _hyp("australia8_mf" if mf else "australia3_sf")
    Xs, X, y, NL = case.data(mf)
    n = case.n0
    m = _model(lctx, hyp, X[:n], y[:n], NL, Xs)
    v = _model(vctx, hyp, X[:n], y[:n], NL, Xs)
    m.predict()
    v.predict()
    n0 = n
    for k in G.KS:
        m.append(X[n:n + k], y[n:n + k])
        v.append(X[n:n + k], y[n:n + k])
        n0, n = n, n + k
        mu, var = m.predict()
        mu_v, var_v = v.predict()
        mu_r, var_r = _ref(hyp, X[:n], y[:n], NL, Xs)
        e_o, e_v = _err(hyp, mu, var, mu_r, var_r), _err(hyp, mu, var, mu_v, var_v)
        print(f"{case.name} mf={int(mf)} n={n} k={k}: oracle {e_o:.2e} vstream {e_v:.2e}")
        assert e_o < TOL, (n, k)
        assert e_v < 1e-8, (n, k)   # lattice == V stream to rounding
    st, sv = m.stats(), v.stats()
    print(case.name, st)
    assert (st["lattice_nx"], st["lattice_ny"]) == (case.nx, case.ny), st
    assert sv["lattice"] == 0 and sv["vstream"] == 3, sv
    if declined:
        # the host keeps the V stream for this grid, forced or not: the V-stream context's bits
        assert st["lattice"] == 0 and st["vstream"] == 3 and st["inc_factor"] == 3, st
        assert np.array_equal(mu, mu_v) and np.array_equal(var, var_v)
        return st
    assert st["lattice"] == 3 and st["inc_factor"] == 3 and st["full_predict"] == 1, st
    # the rows the last step carried as off-lattice ("virtual") K rows: exactly those
    # the cell lookup misses
    assert st["lattice_virtual"] == G.expected_virtual(Xs, X, NL, n0, mf), st
    # the factor the lattice step leaves behind equals the V stream's (both bordered)
    np.testing.assert_allclose(m.factor(), v.factor(), rtol=1e-9, atol=1e-12)
    return st


@pytest.mark.parametrize("mf", [False, True], ids=["sf", "mf"])
@pytest.mark.parametrize("case", [c for c in G.SHAPES if c.name not in G.SPECIAL], ids=lambda c: c.name)
def test_shapes(case, mf, lctx, vctx):
    """Rectangles, both ways round and in both cell orders: tabw 64, 128 and 256
    (zq = 8, 4, 2), both dimensions ragged against the tiles, M = 63 < one tile with
    rows revisiting cells. All take the lattice step; on uniform axes no row is virtual."""
    st = _sequence(case, mf, lctx, vctx)
    assert st["lattice_virtual"] == 0


@pytest.mark.parametrize("mf", [False, True], ids=["sf", "mf"])
@pytest.mark.parametrize("case", [c for c in G.SHAPES if c.name in G.SPECIAL], ids=lambda c: c.name)
def test_shapes_tabw192_and_degenerate_axis(case, mf, lctx, vctx):
    """tabw = 192 (24 x 130: three y-tiles, 130 x 24: one; zq = 2 and a second thread
    group of 64 threads whose rows the nrow bound drops) and a degenerate axis
    (40 x 1: one Z unit per part, one y-row; 1 x 40: one x-index per tile). Both take
    the lattice step (observed: lattice == 3, no virtual rows)."""
    st = _sequence(case, mf, lctx, vctx)
    assert st["lattice_virtual"] == 0


@pytest.mark.parametrize("mf", [False, True], ids=["sf", "mf"])
@pytest.mark.parametrize("case", G.AXES + G.SHIFTED, ids=lambda c: c.name)
def test_axes(case, mf, lctx, vctx):
    """(40, 33) with the x axis increasing / reversed, y in [-0.5, 0.7] increasing /
    reversed, x uniform or warped (linspace(0, 1, 40) ** 1.5, ** 2.2), and rows moved
    off the grid by 0.29 of a spacing along x only or y only (the cell lookup's half
    hits, both cell orders).

    Observed paths (pinned here from stats()): every variant takes the lattice step,
    lattice == 3. Uniform axes, either direction: lattice_virtual == 0. Warped x: the
    lookup's uniform estimate +-1 finds only the rows near the axis' ends and where
    the warp crosses the uniform spacing, all others run as virtual rows -- the count
    equals the NumPy restatement of the lookup (tests/_lattice_grids.on_lattice), at
    the last step's n0 = 211 old rows: 172 to 184 of them at exponent 1.5, 187 to 194
    at 2.2 (SF; MF counts the hifi rows again for the second kernel part: 283 to 296
    and 306 to 316). Shifted rows: the 15 moved rows among the old rows are virtual
    (MF: + 9 hifi = 24), none of the others."""
    st = _sequence(case, mf, lctx, vctx)
    if case.warp is None and case.shift is None:
        assert st["lattice_virtual"] == 0
    else:
        assert st["lattice_virtual"] > 0


@pytest.mark.parametrize("mf", [False, True], ids=["sf", "mf"])
@pytest.mark.parametrize("case", G.DECLINED, ids=lambda c: c.name)
def test_long_axis_is_declined(case, mf, lctx, vctx):
    """An axis of 257 cells (tabw = 320, more than a Z unit's 256 threads): lat_eligible
    declines it on a forced context too. The grid is still detected as a lattice; the
    three steps run the V stream (vstream == 3, lattice == 0) and match the oracle."""
    _sequence(case, mf, lctx, vctx, declined=True)


# ---- 3. kernel forms on rectangular grids (tabw = 192 both ways round) ----

FORM_GRIDS = [(24, 130), (130, 24)]


def _form_specs(nx, ny, B, seed0):
    """B MF GPs of different sizes on one nx x ny grid, a few lofi rows and a hifi row
    off the lattice (along x, along y, along both)."""
    Xs = G.make_grid(G.axis(nx), G.axis(ny, -0.5, 0.7))
    specs = []
    for i in range(B):
        nl, nh = 90 + 13 * i, 110 - 7 * i
        X, y, _ = G.make_data(Xs, nl + nh + sum(G.KS), seed0 + i)
        G.shift_rows(Xs, X, np.r_[5:9], 0, 0.31)
        G.shift_rows(Xs, X, np.r_[7:12], 1, 0.27)
        G.shift_rows(Xs, X, np.r_[nl + 2:nl + 3], 0, 0.31)
        specs.append((Xs, X, y, nl, nl + nh))
    return specs


def _run_batch(ctx, specs, hyp, dtype="f64", ks=G.KS, oracle=True):
    """One batch_append_predict per k over the models of `specs` [(Xs, X, y, NL, n0)]
    (grids may differ: the outputs are concatenated by each GP's M), device mu / var /
    vmax / vargmax. Every step: the fused max / argmax equal the host's over the
    returned variance, exactly; with `oracle`, every GP against the oracle at every
    cell. Returns the steps' outputs and the models."""
    import torch
    from mfgp_coverage_amd import _lib
    dt = _lib.F32 if dtype == "f32" else _lib.F64
    B = len(specs)
    models = [_model(ctx, hyp, X[:n0], y[:n0], nl, Xs, dtype=dt) for Xs, X, y, nl, n0 in specs]
    Ms = [s[0].shape[0] for s in specs]
    off = np.concatenate([[0], np.cumsum(Ms)])
    mu = torch.empty(int(off[-1]), dtype=torch.float64, device="cuda")
    var = torch.empty_like(mu)
    vmax = torch.empty(B, dtype=torch.float64, device="cuda")
    vam = torch.empty(B, dtype=torch.int64, device="cuda")
    _lib.batch_predict(models, mu.data_ptr(), var.data_ptr())
    ns = [s[4] for s in specs]
    out = []
    kss = O.prior_variance(hyp)
    for step, k in enumerate(ks):
        Xn = np.concatenate([s[1][n:n + k] for s, n in zip(specs, ns)])
        yn = np.concatenate([s[2][n:n + k] for s, n in zip(specs, ns)])
        Xt = torch.from_numpy(np.ascontiguousarray(Xn)).cuda()
        yt = torch.from_numpy(np.ascontiguousarray(yn)).cuda()
        _lib.batch_append_predict(models, Xt.data_ptr(), yt.data_ptr(), [k] * B, mu.data_ptr(), var.data_ptr(),
                                  vmax_ptr=vmax.data_ptr(), vargmax_ptr=vam.data_ptr())
        ns = [n + k for n in ns]
        mh, vh, xh, ah = mu.cpu().numpy(), var.cpu().numpy(), vmax.cpu().numpy(), vam.cpu().numpy()
        out.append((mh, vh, xh, ah))
        for i, ((Xs, X, y, nl, _), n) in enumerate(zip(specs, ns)):
            mi, vi = mh[off[i]:off[i + 1]], vh[off[i]:off[i + 1]]
            # the epilogue reports the cell ix sx + iy sy: the transposed index on a
            # rectangle is another cell (or none)
            assert xh[i] == vi.max() and ah[i] == int(np.argmax(vi)), (step, i, xh[i], vi.max(), ah[i])
            if oracle:
                mu_r, var_r = _ref(hyp, X[:n], y[:n], nl, Xs)
                if dtype == "f64":
                    e = O.parity_errors(mi, vi, mu_r, var_r, kss)
                    assert max(e) < TOL, (step, i, e)
                else:
                    e = O.parity_errors_f32(mi, vi, mu_r, var_r, kss)
                    assert max(e) < O.F32_TOL, (step, i, e)
    ctx.synchronize()
    return out, models


def _same_bits(ra, rb, what):
    for step, (sa, sb) in enumerate(zip(ra, rb)):
        for xa, xb in zip(sa, sb):
            assert np.array_equal(xa, xb), (what, step)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", FORM_GRIDS)
def test_forms_default_vs_oracle(nx, ny, dtype, B, lctx):
    """The default form (no diagnostic switch) at every step against the oracle,
    fp64 and fp32 models, with the fused max / argmax."""
    hyp = _hyp("australia8_mf" if dtype == "f64" else "australia9_mf")
    _, models = _run_batch(lctx, _form_specs(nx, ny, B, 300), hyp, dtype)
    for m in models:
        st = m.stats()
        assert st["lattice"] == 3 and st["lattice_virtual"] > 0, st
        assert (st["lattice_nx"], st["lattice_ny"]) == (nx, ny), st


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", FORM_GRIDS)
def test_forms_gemm2_equals_in_launch_split4(monkeypatch, nx, ny, dtype):
    """k_lat_gemm2 (MFGP_LAT_GEMM2=1) against the one-launch form with split-K 4
    through memory (MFGP_LAT_GEMM2=0, MFGP_LAT_KSPLIT=4): the same bits, as on 64 x 64
    (tests/test_gpu_lattice.py), where the two forms' tiles (64 / ka against 128 / ka
    x-indices) cover a rectangle differently."""
    from mfgp_coverage_amd import _lib
    hyp = _hyp("australia8_mf" if dtype == "f64" else "australia9_mf")
    for B in (1, 3):
        monkeypatch.setenv("MFGP_LAT_GEMM2", "0")
        monkeypatch.setenv("MFGP_LAT_KSPLIT", "4")
        a = _lib.Context(0)
        monkeypatch.setenv("MFGP_LAT_GEMM2", "1")
        monkeypatch.delenv("MFGP_LAT_KSPLIT")
        b = _lib.Context(0)
        monkeypatch.delenv("MFGP_LAT_GEMM2")
        a.set_lattice("force")
        b.set_lattice("force")
        specs = _form_specs(nx, ny, B, 310)
        ra, ma = _run_batch(a, specs, hyp, dtype, oracle=False)
        rb, mb = _run_batch(b, specs, hyp, dtype, oracle=True)
        assert all(m.stats()["lattice"] == 3 and m.stats()["lattice_g2"] == 0 for m in ma), [m.stats() for m in ma]
        assert all(m.stats()["lattice"] == 3 and m.stats()["lattice_g2"] == 3 for m in mb), [m.stats() for m in mb]
        _same_bits(ra, rb, B)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", FORM_GRIDS)
def test_forms_zcsr_equals_zunits(monkeypatch, nx, ny, dtype):
    """Z units reading the scan units' member lists (MFGP_LAT_ZCSR=1: bucketed by py,
    offsets [ny + 1]) against Z units that bucket the rows themselves (=0), under
    both GEMM forms: the same bits. At tabw = 192 the member-list unit runs without
    its stash and its second thread group reads the next unit's rows' lists."""
    from mfgp_coverage_amd import _lib
    hyp = _hyp("australia8_mf" if dtype == "f64" else "australia9_mf")
    for B, g2 in ((1, "0"), (3, "0"), (3, "1")):
        monkeypatch.setenv("MFGP_LAT_GEMM2", g2)
        monkeypatch.setenv("MFGP_LAT_ZCSR", "0")
        a = _lib.Context(0)
        monkeypatch.setenv("MFGP_LAT_ZCSR", "1")
        b = _lib.Context(0)
        monkeypatch.delenv("MFGP_LAT_ZCSR")
        monkeypatch.delenv("MFGP_LAT_GEMM2")
        a.set_lattice("force")
        b.set_lattice("force")
        specs = _form_specs(nx, ny, B, 320)
        ra, ma = _run_batch(a, specs, hyp, dtype, oracle=False)
        rb, mb = _run_batch(b, specs, hyp, dtype, oracle=(g2 == "1"))
        for m in ma + mb:
            st = m.stats()
            assert st["lattice"] == 3 and st["lattice_virtual"] > 0 and st["lattice_g2"] == 3 * int(g2), st
        _same_bits(ra, rb, (B, g2))


@pytest.mark.parametrize("ksplit", [1, 2, 8])
@pytest.mark.parametrize("wu", [1, 7])
@pytest.mark.parametrize("nx,ny", FORM_GRIDS)
def test_forms_split_and_w_units_vs_oracle(monkeypatch, nx, ny, ksplit, wu):
    """Split-K factors and w-unit counts forced through MFGP_LAT_KSPLIT / MFGP_LAT_WU
    (the one-launch form), three GPs, every step against the oracle."""
    from mfgp_coverage_amd import _lib
    monkeypatch.setenv("MFGP_LAT_GEMM2", "0")
    monkeypatch.setenv("MFGP_LAT_KSPLIT", str(ksplit))
    monkeypatch.setenv("MFGP_LAT_WU", str(wu))
    ctx = _lib.Context(0)
    ctx.set_lattice("force")
    _, models = _run_batch(ctx, _form_specs(nx, ny, 3, 330), _hyp("australia8_mf"))
    for m in models:
        st = m.stats()
        assert st["lattice"] == 3 and st["lattice_g2"] == 0, st


# ---- 4. one launch, different grids ----

def test_one_launch_different_grids(lctx):
    """A ragged batch of three MF GPs on (16, 128) x-outer, (128, 16) y-outer and
    (51, 51), different N, three steps of one batch_append_predict each: every GP
    against the oracle, its fused max / argmax, and the lattice step for all three
    (per-GP nx, ny, strides, tabw, tile and Z-unit counts in one launch)."""
    hyp = _hyp("australia8_mf")
    grids = [G.make_grid(G.axis(16), G.axis(128)), G.make_grid(G.axis(128), G.axis(16), "y_outer"),
             G.make_grid(G.axis(51), G.axis(51))]
    specs = []
    for i, (Xs, (nl, nh)) in enumerate(zip(grids, [(90, 200), (150, 37), (60, 128)])):
        X, y, _ = G.make_data(Xs, nl + nh + sum(G.KS), 400 + i)
        specs.append((Xs, X, y, nl, nl + nh))
    _, models = _run_batch(lctx, specs, hyp)
    for m, shape in zip(models, [(16, 128), (128, 16), (51, 51)]):
        st = m.stats()
        assert st["lattice"] == 3 and (st["lattice_nx"], st["lattice_ny"]) == shape, st


# ---- 5. the sharded slice equals the whole ----

@pytest.mark.parametrize("Gn,world,ranks", [(51, 2, (0, 1)), (128, 8, (0, 7))])
def test_sharded_slice_equals_whole(Gn, world, ranks, lctx):
    """sharded.predict_sharded gives each rank a block of whole outer rows as its grid:
    26 x 51 and 25 x 51 of the reference grid over 2 ranks, 16 x 128 of the headline's
    over 8. A model holding the block (training rows outside it are off its lattice:
    virtual rows, x no axis value of the block) against the same cells of a model
    holding the whole grid, two lattice steps each: below 1e-9 (two operation
    orders, as test_trinv_recursive_vs_columns_and_oracle), and the oracle."""
    from mfgp_coverage_amd import sharded
    hyp = _hyp("australia8_mf")
    Xs = G.make_grid(G.axis(Gn), G.axis(Gn))
    M = Xs.shape[0]
    row = sharded.lattice_row(Xs)
    assert row == Gn
    NL, n0, ks = 100, 250, (8, 12)
    X, y, _ = G.make_data(Xs, n0 + sum(ks), 500 + Gn)
    kss = O.prior_variance(hyp)

    def steps(grid):
        m = _model(lctx, hyp, X[:n0], y[:n0], NL, grid)
        m.predict()
        n, outs = n0, []
        for k in ks:
            m.append(X[n:n + k], y[n:n + k])
            n += k
            outs.append(m.predict())
        return m, outs

    whole, wo = steps(Xs)
    assert whole.stats()["lattice"] == 2
    refs, n = [], n0
    for k in ks:
        n += k
        refs.append(_ref(hyp, X[:n], y[:n], NL, Xs))
    for rank in ranks:
        lo, hi = sharded.shard_cells(M, world, rank, row)
        m, so = steps(Xs[lo:hi])
        st = m.stats()
        assert st["lattice"] == 2 and st["lattice_ny"] == Gn and st["lattice_nx"] == (hi - lo) // Gn, st
        assert st["lattice_nx"] in (Gn // world, Gn // world + 1) and st["lattice_virtual"] > 0, st
        for (mu, var), (mu_w, var_w), (mu_r, var_r) in zip(so, wo, refs):
            e_w = O.parity_errors(mu, var, mu_w[lo:hi], var_w[lo:hi], kss)
            e_o = O.parity_errors(mu, var, mu_r[lo:hi], var_r[lo:hi], kss)
            print(f"G={Gn} rank {rank}/{world}: whole {max(e_w):.2e} oracle {max(e_o):.2e}")
            assert max(e_w) < 1e-9, (rank, e_w)
            assert max(e_o) < TOL, (rank, e_o)


# ---- 6. the planner loop on a rectangular lattice ----

def test_sample_points_on_rectangular_lattice(lctx):
    """mfgp_sample_points on a (24, 70) grid, MF, on a context with the lattice forced,
    from a model whose last step was a lattice step: every chosen point is an argmax
    of the oracle's variance given the points before it and the loop stops at the
    threshold (as tests/test_gpu_planners.py checks); the chosen cell's coordinates
    come from the grid by the fused argmax's cell index. The loop's own iterations are
    one-row V-stream steps (planner_stats: lattice == 0), and it leaves the model as it
    was: the same predict() bits, the same counters, and the next append is a lattice
    step again."""
    hyp = _hyp("australia8_mf")
    Xs = G.make_grid(G.axis(24), G.axis(70, -0.5, 0.7))
    NL, n0 = 60, 150
    X, y, _ = G.make_data(Xs, n0 + 16, 600)
    m = _model(lctx, hyp, X[:n0], y[:n0], NL, Xs)
    m.predict()
    m.append(X[n0:n0 + 8], y[n0:n0 + 8])
    n = n0 + 8
    m.predict()
    mu0, var0 = m.predict()
    st0 = m.stats()
    assert st0["lattice"] == 1 and (st0["lattice_nx"], st0["lattice_ny"]) == (24, 70), st0
    thr = 0.25 * float(var0.max())
    lctx.planner_stats(reset=True)
    pts = m.sample_points(thr, 2000)
    ps = lctx.planner_stats(reset=True)
    print("sample_points:", pts.shape[0], "points", ps)
    assert 8 < pts.shape[0] < 2000
    assert ps["runs"] == 1 and ps["lattice"] == 0 and ps["inc_factor"] >= pts.shape[0], ps
    # as tests/test_gpu_planners._check_against_oracle, over ~550 points: the oracle's
    # variance carried forward point by point (G.GreedyVariance) and checked against
    # O.mf_diag from scratch every 128 points and at the end
    kss = O.prior_variance(hyp)
    gv = G.GreedyVariance(hyp, X[:NL], X[NL:n], Xs, room=pts.shape[0])
    for i in range(pts.shape[0] + 1):
        var = gv.var
        if i % 128 == 0 or i == pts.shape[0]:
            ref = gv.from_scratch()
            assert np.max(np.abs(var - ref) / np.maximum(np.abs(ref), 1e-6 * kss)) < 1e-9, i
        vmax = var.max()
        if i < pts.shape[0]:
            j = np.flatnonzero((Xs == pts[i]).all(1))
            assert j.size == 1, (i, pts[i])
            assert var[j[0]] >= vmax - TOL * max(vmax, 1e-6 * kss), (i, var[j[0]], vmax)
            assert vmax > thr * (1 - TOL), i        # the loop had to continue
            gv.append(pts[i])
        else:
            assert vmax <= thr * (1 + TOL)          # ... and stopped at the threshold
    mu1, var1 = m.predict()
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0)
    st1 = m.stats()
    predicts = ("vstream", "full_predict", "post_copy")    # (the predict just above)
    assert {k: v for k, v in st1.items() if k not in predicts} == \
        {k: v for k, v in st0.items() if k not in predicts}, (st0, st1)
    m.append(X[n:n + 8], y[n:n + 8])
    mu, var = m.predict()
    mu_r, var_r = _ref(hyp, X[:n + 8], y[:n + 8], NL, Xs)
    assert _err(hyp, mu, var, mu_r, var_r) < TOL
    assert m.stats()["lattice"] == 2, m.stats()
