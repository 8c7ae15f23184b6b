"""The lattice step's second launch (k_lat_gemm2) at the
shapes where its phases can go wrong: a K loop of one stage in all (splits with no
stage bring zeros), the four splits' sums meeting in the cells, the tile counted in
ahead of its stores (batches) and behind them (one GP, whose launch passes its
status word to the host), 1 / L22[a][a] in place of L22^-1 by substitution.

Bits: against the one-launch form with split-K 4 through memory (MFGP_LAT_GEMM2=0,
MFGP_LAT_KSPLIT=4), whose GEMM and epilogue are other code: the same stages per
split and the same order of the splits' sums, so mean, variance and the fused
max / argmax are equal bit for bit at every step (the resident posterior each
step starts from included). Values: the CPU oracle at every cell (PARITY_TOL;
F32_TOL for fp32 models). stats() pins the form that ran.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _lattice_grids as G
from tests.test_gpu_lattice_grids import _err, _form_specs, _hyp, _model, _ref, _run_batch, _same_bits

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL


def _forms(monkeypatch):
    """(the one-launch split-K-4 context, the k_lat_gemm2 context), lattice forced
    (these batches are far below the chip's size)."""
    from mfgp_coverage_amd import _lib
    monkeypatch.setenv("MFGP_LAT_GEMM2", "0")
    monkeypatch.setenv("MFGP_LAT_KSPLIT", "4")
    a = _lib.Context(0)
    monkeypatch.setenv("MFGP_LAT_GEMM2", "1")
    monkeypatch.delenv("MFGP_LAT_KSPLIT")
    b = _lib.Context(0)
    monkeypatch.delenv("MFGP_LAT_GEMM2")
    a.set_lattice("force")
    b.set_lattice("force")
    return a, b


def _both(monkeypatch, specs, hyp, ks, dtype="f64"):
    """The steps `ks` on both forms: the same bits, k_lat_gemm2 against the oracle and
    its own max / argmax (_run_batch), and the counters of the form that ran."""
    a, b = _forms(monkeypatch)
    ra, ma = _run_batch(a, specs, hyp, dtype, ks=ks, oracle=False)
    rb, mb = _run_batch(b, specs, hyp, dtype, ks=ks, oracle=True)
    n = len(ks)
    assert all(m.stats()["lattice"] == n and m.stats()["lattice_g2"] == 0 for m in ma), [m.stats() for m in ma]
    assert all(m.stats()["lattice"] == n and m.stats()["lattice_g2"] == n for m in mb), [m.stats() for m in mb]
    _same_bits(ra, rb, ks)
    return rb, mb


def _case(name):
    return next(c for c in G.ALL_CASES if c.name == name)


def test_one_ragged_tile_one_stage(monkeypatch):
    """9 x 7, SF, 3 new rows: one tile with 63 live cells of its 512 cell threads, and
    one K stage in all (zq8 = 8, one kernel part): splits 1-3 have none and bring
    zeros to the meeting. (One GP: the tile counts in behind its stores.)"""
    case = _case("9x7")
    Xs, X, y, NL = case.data(False, ks=(3,))
    _, models = _both(monkeypatch, [(Xs, X, y, NL, case.n0)], _hyp("australia3_sf"), (3,))
    st = models[0].stats()
    assert (st["lattice_nx"], st["lattice_ny"]) == (9, 7) and st["lattice_virtual"] == 0, st


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", [(24, 130), (130, 24)])
def test_tabw192_k_1_8_12(monkeypatch, nx, ny, dtype):
    """tabw = 192 both ways round (a last iy tile of 2 columns), two MF GPs of different
    sizes with rows off the lattice, steps of 1, 8 and 12 rows: 12 takes KA = 16 (4
    lattice columns per tile, 256 cell threads); fp64 and fp32 models."""
    hyp = _hyp("australia8_mf" if dtype == "f64" else "australia9_mf")
    _, models = _both(monkeypatch, _form_specs(nx, ny, 2, 700), hyp, (1, 8, 12), dtype)
    for m in models:
        st = m.stats()
        assert (st["lattice_nx"], st["lattice_ny"]) == (nx, ny) and st["lattice_virtual"] > 0, st


def test_warped_axis_virtual_pass(monkeypatch):
    """A warped x axis (40 x 33, exponent 2.2): most training rows miss the cell lookup
    and run as virtual K rows, so the second pass over the ring runs before the
    splits store their sums into the rings' place."""
    case = _case("xi_yi_w2.2")
    Xs, X, y, NL = case.data(True)
    _, models = _both(monkeypatch, [(Xs, X, y, NL, case.n0)], _hyp("australia8_mf"), G.KS)
    assert models[0].stats()["lattice_virtual"] > 100, models[0].stats()


def test_three_grids_one_launch(monkeypatch):
    """16 x 128 x-outer, 128 x 16 y-outer and 51 x 51 in one launch: the grid is the
    largest GP's, the other GPs' surplus workgroups leave at once and nothing waits
    for them (each GP's tiles count in against its own lat_tiles)."""
    grids = [G.make_grid(G.axis(16), G.axis(128)), G.make_grid(G.axis(128), G.axis(16), "y_outer"),
             G.make_grid(G.axis(51), G.axis(51))]
    specs = []
    for i, (Xs, (nl, nh)) in enumerate(zip(grids, [(90, 200), (150, 37), (60, 128)])):
        X, y, _ = G.make_data(Xs, nl + nh + sum(G.KS), 710 + i)
        specs.append((Xs, X, y, nl, nl + nh))
    _, models = _both(monkeypatch, specs, _hyp("australia8_mf"), G.KS)
    for m, shape in zip(models, [(16, 128), (128, 16), (51, 51)]):
        st = m.stats()
        assert (st["lattice_nx"], st["lattice_ny"]) == shape, st


def test_chain_with_revisited_cells(monkeypatch):
    """Three steps of 9 rows, 3 of each 9 at cells that already hold a hifi row (fresh
    noise). Each step starts from the resident posterior the step before left, so
    equal bits at step 3 say that posterior is the reference form's too; the fused
    max / argmax equal var.max() / var.argmax() of the returned variance exactly,
    first index on ties (_run_batch asserts it at every step)."""
    Xs = G.make_grid(G.axis(40), G.axis(33, -0.5, 0.7))
    nl, nh, ks = 80, 120, (9, 9, 9)
    X, y, _ = G.make_data(Xs, nl + nh + sum(ks), 720)
    rng = np.random.default_rng(721)
    n = nl + nh
    for k in ks:
        old = rng.choice(np.arange(nl, n), 3, replace=False)
        X[n + 6:n + 9] = X[old]
        n += k
    rb, _ = _both(monkeypatch, [(Xs, X, y, nl, nl + nh)], _hyp("australia8_mf"), ks)
    assert all(np.all(np.isfinite(v)) for _, v, _, _ in rb)


def test_eager_one_gp_equals_batch(monkeypatch):
    """One GP at 64 x 64 through append + predict (the eager call; a launch of one GP
    passes the status word to the host, and there the tile counts in behind its
    stores) against batch_append_predict on the same form and on the reference form:
    the same bits; and the oracle."""
    hyp = _hyp("australia8_mf")
    Xs = G.make_grid(G.axis(64), G.axis(64))
    nl, nh, ks = 120, 160, G.KS
    X, y, _ = G.make_data(Xs, nl + nh + sum(ks), 730)
    rb, _ = _both(monkeypatch, [(Xs, X, y, nl, nl + nh)], hyp, ks)
    _, b = _forms(monkeypatch)
    m = _model(b, hyp, X[:nl + nh], y[:nl + nh], nl, Xs)
    m.predict()
    n = nl + nh
    for step, k in enumerate(ks):
        m.append(X[n:n + k], y[n:n + k])
        n += k
        mu, var = m.predict()
        assert np.array_equal(mu, rb[step][0]) and np.array_equal(var, rb[step][1]), step
        mu_r, var_r = _ref(hyp, X[:n], y[:n], nl, Xs)
        assert _err(hyp, mu, var, mu_r, var_r) < TOL, step
    st = m.stats()
    assert st["lattice"] == len(ks) and st["lattice_g2"] == len(ks), st
