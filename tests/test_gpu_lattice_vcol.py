"""The lattice step's column store of V (Vc[cell][row], the w
units' and producers' source of L21; mfgp_ctx_set_lattice_vcol).

The store holds the same numbers as V, so a step that reads it must give the bits of a
step that reads the producers' compact rows: every case here runs the same sequence on
a context with the store (the default) and on one without it (set_lattice_vcol(False))
and compares mean, variance, the fused max / argmax of every step and, at the end, V
and F = L^-1 (their new rows came from the steps) with array_equal. The path counters
say which source the w units read (lattice_vcol) and how many rows the catch-up
k_vcol_build transposed (vcol_rows_built). Shapes: grids of less than one 64-cell tile,
ragged against the tiles both ways, tabw 192 and a y-outer cell order; n0 at the 64-row
block and 16-row step edges; appends of 1, 3, 8 and 12 rows (KA 8 and 16); fp64 and
fp32 models; one GP and three GPs of different n0 in one launch; two new points in one
cell; a new point off the lattice (the step falls back to the compact rows); the store
behind V (a V-stream step in between, truncate + re-append, a capacity growth); the
store's content against V; and a budget of zero (no store: the parent path)."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _lattice_grids as G

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL
KS = (1, 3, 8, 12)


def _hyp(name):
    from mfgp_coverage_amd.synthetic import HYP
    return HYP[name].copy()


@pytest.fixture(scope="module")
def ctxs():
    """(store on: the default rule, store off), both past the size gate."""
    from mfgp_coverage_amd import _lib
    on, off = _lib.Context(0), _lib.Context(0)
    on.set_lattice("force")
    off.set_lattice("force")
    off.set_lattice_vcol(False)
    return on, off


GRIDS = {
    "9x7": (9, 7, "x_outer"),          # M = 63: less than one tile
    "40x33": (40, 33, "x_outer"),
    "24x130": (24, 130, "x_outer"),    # tabw 192
    "128x16_yo": (128, 16, "y_outer"),
}


def _grid(name):
    nx, ny, order = GRIDS[name]
    return G.make_grid(G.axis(nx), G.axis(ny), order)


_DATA = {}


def _data(gname, n, seed):
    """n rows at grid cells (revisiting cells where the grid has fewer), computed once."""
    key = (gname, n, seed)
    if key not in _DATA:
        Xs = _grid(gname)
        X, y, _ = G.make_data(Xs, n, seed, "cells" if n <= Xs.shape[0] else "revisit")
        _DATA[key] = (Xs, X, y)
    return _DATA[key]


def _model(ctx, hyp, X, y, NL, Xs, dtype):
    from mfgp_coverage_amd import _lib
    kind = _lib.SF if hyp.shape[0] == 4 else _lib.MF
    m = _lib.Model(ctx, kind, hyp, 1e-8, dtype=_lib.F32 if dtype == "f32" else _lib.F64)
    m.set_grid(Xs)
    if kind == _lib.SF:
        m.set_data(np.empty((0, 2)), np.empty(0), X, y)
    else:
        m.set_data(X[:NL], y[:NL], X[NL:], y[NL:])
    return m


class Batch:
    """B models on one context stepped through the batch entry points, device outputs and
    the fused max / argmax; every step's outputs are kept."""

    def __init__(self, ctx, hyp, sets, dtype="f64"):
        import torch
        self.ctx, self.hyp = ctx, hyp
        self.models = [_model(ctx, hyp, X[:n0], y[:n0], NL, Xs, dtype) for (Xs, X, y, NL, n0) in sets]
        self.M = sets[0][0].shape[0]
        B = len(sets)
        self.mu = torch.empty(B * self.M, dtype=torch.float64, device="cuda")
        self.var = torch.empty_like(self.mu)
        self.vmax = torch.empty(B, dtype=torch.float64, device="cuda")
        self.vam = torch.empty(B, dtype=torch.int64, device="cuda")
        self.out = []

    def predict(self):
        from mfgp_coverage_amd import _lib
        _lib.batch_predict(self.models, self.mu.data_ptr(), self.var.data_ptr())

    def step(self, rows):
        """rows: per model (X [k, 2], y [k]) host arrays, the same k."""
        from mfgp_coverage_amd import _lib
        k = rows[0][0].shape[0]
        Xn = np.ascontiguousarray(np.concatenate([r[0] for r in rows]))
        yn = np.ascontiguousarray(np.concatenate([r[1] for r in rows]))
        _lib.batch_append_predict(self.models, Xn.ctypes.data, yn.ctypes.data, [k] * len(rows), self.mu.data_ptr(),
                                  self.var.data_ptr(), vmax_ptr=self.vmax.data_ptr(), vargmax_ptr=self.vam.data_ptr())
        self.out.append((self.mu.cpu().numpy().copy(), self.var.cpu().numpy().copy(),
                         self.vmax.cpu().numpy().copy(), self.vam.cpu().numpy().copy()))

    def state(self):
        """Per model (V [n, M], F [n, n]) as the steps left them."""
        return [(m.debug_read_v()[0], m.debug_read_f()) for m in self.models]


def _same(a, b):
    """Two batches took the same steps to the same bits."""
    assert len(a.out) == len(b.out)
    for s, (oa, ob) in enumerate(zip(a.out, b.out)):
        for name, xa, xb in zip(("mu", "var", "vmax", "vargmax"), oa, ob):
            assert np.array_equal(xa, xb), (s, name)
    for i, ((va, fa), (vb, fb)) in enumerate(zip(a.state(), b.state())):
        assert va.shape == vb.shape and np.array_equal(va, vb), ("V", i)
        assert fa.shape == fb.shape and fa.shape[0] == va.shape[0] and np.array_equal(fa, fb), ("F", i)


def _content(m):
    """Vc[c][i] == V(i, c) for every row the model holds and every cell."""
    v, vc, rows = m.debug_read_v()
    assert vc is not None and rows == v.shape[0] == m.n, (rows, v.shape, m.n)
    assert np.array_equal(vc.T, v)


def _sets(gname, n0s, ks, seed):
    out = []
    for i, n0 in enumerate(n0s):
        Xs, X, y = _data(gname, n0 + sum(ks), seed + i)
        out.append((Xs, X, y, int(0.4 * n0), n0))
    return out


def _run_pair(ctxs, hyp, sets, ks, dtype):
    pair = []
    for ctx in ctxs:
        b = Batch(ctx, hyp, sets, dtype)
        b.predict()
        n = [s[4] for s in sets]
        for k in ks:
            b.step([(s[1][ni:ni + k], s[2][ni:ni + k]) for s, ni in zip(sets, n)])
            n = [ni + k for ni in n]
        pair.append(b)
    on, off = pair
    for m in on.models:
        st = m.stats()
        assert st["lattice"] == len(ks) and st["lattice_vcol"] == len(ks), st
        assert st["vcol_rows_built"] == st["v_rows"] - sum(ks), st   # the entry's catch-up: n0 rows
    for m in off.models:
        st = m.stats()
        assert st["lattice"] == len(ks) and st["lattice_vcol"] == 0 and st["vcol_rows_built"] == 0, st
    _same(on, off)
    return on, off


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n0", [63, 64, 65, 127, 200])
@pytest.mark.parametrize("gname", list(GRIDS))
def test_store_on_equals_store_off_one_gp(ctxs, gname, n0, dtype):
    """One GP: n0 base rows, appends of 1, 3, 8 and 12 rows (so steps at n0, n0 + 1,
    n0 + 4, n0 + 12: even and odd rows for the 16-byte stores, KA 8 and 16)."""
    hyp = _hyp("australia8_mf")
    on, _ = _run_pair(ctxs, hyp, _sets(gname, [n0], KS, 100 + n0), KS, dtype)
    _content(on.models[0])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("gname", list(GRIDS))
def test_store_on_equals_store_off_three_gps(ctxs, gname, dtype):
    """Three GPs of different n0 (63, 127, 200) in one launch."""
    hyp = _hyp("australia8_mf")
    on, _ = _run_pair(ctxs, hyp, _sets(gname, [63, 127, 200], KS, 300), KS, dtype)
    for m in on.models:
        _content(m)


def test_single_fidelity_against_the_oracle(ctxs):
    """An SF model on 40 x 33: store on == store off, and both the oracle's posterior."""
    hyp = _hyp("australia3_sf")
    sets = _sets("40x33", [200], KS, 500)
    sets = [(Xs, X, y, 0, n0) for (Xs, X, y, _, n0) in sets]
    on, _ = _run_pair(ctxs, hyp, sets, KS, "f64")
    Xs, X, y, _, n0 = sets[0]
    n = n0 + sum(KS)
    mu_r, var_r = O.sf_diag(X[:n], y[:n], hyp, Xs)
    mu, var = on.out[-1][0], on.out[-1][1]
    assert max(O.parity_errors(mu, var, mu_r, var_r, O.prior_variance(hyp))) < TOL


def test_two_agents_in_one_cell(ctxs):
    """A step whose rows 0 and 2 are the same cell (two agents; different observations)."""
    hyp = _hyp("australia8_mf")
    Xs, X, y = _data("40x33", 200 + 11, 600)
    X, y = X.copy(), y.copy()
    X[202] = X[200]
    sets = [(Xs, X, y, 80, 200)]
    _run_pair(ctxs, hyp, sets, (3, 8), "f64")


def test_off_lattice_point_falls_back(ctxs):
    """One new point off the lattice in the second of three steps: its w units take the
    compact rows (lattice_vcol counts the other two), the bits are the store-off run's and
    the posterior the oracle's."""
    hyp = _hyp("australia8_mf")
    Xs, X, y = _data("40x33", 200 + 24, 700)
    X = X.copy()
    G.shift_rows(Xs, X, [200 + 8 + 5], 0)
    sets = [(Xs, X, y, 80, 200)]
    pair = []
    for ctx in ctxs:
        b = Batch(ctx, hyp, sets)
        b.predict()
        counts = []
        for s in range(3):
            lo = 200 + 8 * s
            b.step([(X[lo:lo + 8], y[lo:lo + 8])])
            counts.append(b.models[0].stats()["lattice_vcol"])
        pair.append((b, counts))
    (on, c_on), (off, c_off) = pair
    assert c_on == [1, 1, 2] and c_off == [0, 0, 0], (c_on, c_off)
    assert on.models[0].stats()["lattice"] == 3
    _same(on, off)
    _content(on.models[0])   # the fallback step wrote its rows through all the same
    mu_r, var_r = O.mf_diag(X[:80], y[:80], X[80:224], y[80:224], hyp, Xs)
    assert max(O.parity_errors(on.out[-1][0], on.out[-1][1], mu_r, var_r, O.prior_variance(hyp))) < TOL


def test_store_behind_v_after_a_vstream_step(ctxs):
    """Lattice step, a V-stream step (the lattice switched off for it), lattice step: the
    catch-up transposes exactly the V-stream step's rows, and the bits are the store-off
    sequence's."""
    hyp = _hyp("australia8_mf")
    sets = _sets("40x33", [127], (8, 5, 8), 800)
    Xs, X, y, NL, n0 = sets[0]
    pair = []
    for ctx in ctxs:
        b = Batch(ctx, hyp, sets)
        b.predict()
        b.step([(X[127:135], y[127:135])])
        built0 = b.models[0].stats()["vcol_rows_built"]
        ctx.set_lattice(False)
        b.step([(X[135:140], y[135:140])])
        ctx.set_lattice("force")
        st = b.models[0].stats()
        assert st["lattice"] == 1 and st["vcol_rows_built"] == built0, st
        b.step([(X[140:148], y[140:148])])
        pair.append((b, built0))
    (on, built0), (off, _) = pair
    st = on.models[0].stats()
    assert built0 == 127 and st["vcol_rows_built"] == 127 + 5 and st["lattice_vcol"] == 2 and st["lattice"] == 2, st
    assert off.models[0].stats()["vcol_rows_built"] == 0
    _same(on, off)
    _content(on.models[0])


def test_truncate_and_reappend_twice(ctxs):
    """The benchmark's pattern: truncate back to the base rows, append other rows, twice;
    the store follows V's rewritten rows (no catch-up: the base rows stay)."""
    hyp = _hyp("australia8_mf")
    sets = _sets("128x16_yo", [200], (8, 8, 8), 900)
    Xs, X, y, NL, n0 = sets[0]
    pair = []
    for ctx in ctxs:
        b = Batch(ctx, hyp, sets)
        b.predict()
        b.step([(X[200:208], y[200:208])])
        for s in (1, 2):
            b.models[0].truncate(n0 - NL)
            lo = 200 + 8 * s
            b.step([(X[lo:lo + 8], y[lo:lo + 8])])
        pair.append(b)
    on, off = pair
    st = on.models[0].stats()
    assert st["lattice"] == 3 and st["lattice_vcol"] == 3 and st["vcol_rows_built"] == 200, st
    _same(on, off)
    _content(on.models[0])


def test_capacity_growth_reallocates_the_store(ctxs):
    """112 base rows hold 127: the second append of 8 grows the capacity, V moves to a new
    row stride and the store with it (its valid rows are moved: no second catch-up)."""
    hyp = _hyp("australia8_mf")
    ks = (8, 8, 8)
    sets = _sets("40x33", [112], ks, 1000)
    on, _ = _run_pair_growth(ctxs, hyp, sets, ks)
    st = on.models[0].stats()
    assert st["vcol_rows_built"] == 112 and st["lattice_vcol"] == 3, st
    _content(on.models[0])


def _run_pair_growth(ctxs, hyp, sets, ks):
    pair = []
    for ctx in ctxs:
        b = Batch(ctx, hyp, sets)
        b.predict()
        n = sets[0][4]
        for k in ks:
            b.step([(sets[0][1][n:n + k], sets[0][2][n:n + k])])
            n += k
        assert b.models[0].stats()["lattice"] == len(ks)
        pair.append(b)
    _same(*pair)
    return pair


def test_store_content(ctxs):
    """Vc[c][i] == V(i, c) bit for bit after the entry's catch-up and first step, after
    three steps, and after a catch-up behind a V-stream step (fp64 and fp32)."""
    on, _ = ctxs
    hyp = _hyp("australia8_mf")
    for dtype in ("f64", "f32"):
        sets = _sets("24x130", [65], (3, 8, 12, 5, 8), 1100)
        Xs, X, y, NL, n0 = sets[0]
        b = Batch(on, hyp, sets, dtype)
        b.predict()
        n = n0
        for i, k in enumerate((3, 8, 12)):
            b.step([(X[n:n + k], y[n:n + k])])
            n += k
            if i in (0, 2):
                _content(b.models[0])
        on.set_lattice(False)
        b.step([(X[n:n + 5], y[n:n + 5])])
        n += 5
        on.set_lattice("force")
        assert b.models[0].debug_read_v()[2] == n - 5   # the store is behind V
        b.step([(X[n:n + 8], y[n:n + 8])])
        _content(b.models[0])


def test_budget_zero_is_the_parent_path(ctxs):
    """With no budget no model gets a store: counters and outputs are the store-off run's."""
    from mfgp_coverage_amd import _lib
    _, off = ctxs
    z = _lib.Context(0)
    z.set_lattice("force")
    z.set_vcol_budget(0)
    hyp = _hyp("australia8_mf")
    sets = _sets("40x33", [127, 200], (8, 3), 1200)
    pair = []
    for ctx in (z, off):
        b = Batch(ctx, hyp, sets)
        b.predict()
        n = [s[4] for s in sets]
        for k in (8, 3):
            b.step([(s[1][ni:ni + k], s[2][ni:ni + k]) for s, ni in zip(sets, n)])
            n = [ni + k for ni in n]
        pair.append(b)
    for m in pair[0].models:
        st = m.stats()
        assert st["lattice"] == 2 and st["lattice_vcol"] == 0 and st["vcol_rows_built"] == 0, st
        assert m.debug_read_v()[1] is None
    assert [m.stats() for m in pair[0].models] == [m.stats() for m in pair[1].models]
    _same(*pair)
