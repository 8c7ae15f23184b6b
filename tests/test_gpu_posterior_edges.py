"""Every route to the posterior mean and variance on the grid -- the full factor plus
k_predict, the bordered append plus the V stream (fused, unfused, deferred), the one-launch
batch, the lattice step with its GEMM in the launch and as the second launch (k_lat_gemm2),
the k = 0 re-predict, the off-grid fallback solve, k_post_copy, and the consumers of V
(mfgp_query, the diagonal of mfgp_cov_block) --
at the edges of their tiles, against extended-precision values
(tests/golden/posterior_edges_reference.npz, made by oracle.gp_oracle.posterior_extended in
80-bit long double; tests/_posterior_edges.py lists the cases, the metric and the bound).

Metric per case and stage: e_mu = max_c |mu_c - ref_c| / max_c |ref_c| and
e_var = max_c |var_c - ref_c| / k**. Bound, for each of the two:
    16 * max(e_oracle, eps64 * cond(K) * max(N, 64))          (16 * eps64 at N = 0)
with e_oracle the fp64 NumPy oracle's own error against the extended values: a margin over
the reference's error, never over the code under test. Each test prints its figures
(POST_EDGE lines, pytest -s); test_zz_summary prints the largest per hyperparameter set and
route (POST_EDGE_SUMMARY lines).

Measured on an MI355X: the largest error over the cases and stages of a hyperparameter set on a
route, as device / fp64 oracle / bound of the stage that gave it (n: outputs compared; DESIGN.md
section 5):
    set                 route                          n  mu                            var
    australia3_sf       full recompute                23  2.7e-15 / 4.3e-15 / 1.4e-10   9.2e-16 / 9.9e-16 / 1.2e-10
    australia3_sf       bordered append + V stream    69  2.5e-15 / 4.3e-15 / 1.4e-10   9.2e-16 / 9.9e-16 / 1.2e-10
    australia3_sf       k = 0 re-predict              45  2.6e-15 / 4.3e-15 / 1.4e-10   8.7e-16 / 8.8e-16 / 1.4e-10
    australia3_sf       capacity growth                3  2.1e-15 / 8.3e-15 / 3.1e-10   5.5e-16 / 1.5e-15 / 3.1e-10
    australia3_sf       batch_predict                 64  2.3e-15 / 3.1e-15 / 1.2e-10   9.2e-16 / 9.9e-16 / 1.2e-10
    australia3_sf       one-launch batch              40  2.5e-15 / 4.3e-15 / 1.4e-10   8.2e-16 / 1.0e-15 / 1.4e-10
    australia3_sf       lattice step                  80  2.5e-15 / 8.3e-15 / 3.1e-10   9.3e-16 / 8.8e-16 / 1.4e-10
    australia3_sf       lattice step, 2nd launch      40  2.8e-15 / 8.3e-15 / 3.1e-10   9.2e-16 / 8.8e-16 / 1.4e-10
    australia3_sf       mfgp_query                     8  2.6e-15 / 4.3e-15 / 1.4e-10   7.5e-16 / 8.9e-16 / 1.4e-10
    australia3_sf       cov_block diagonal             8  -                             1.7e-15 / 1.6e-15 / 3.1e-10
    australia8_mf       full recompute                17  3.0e-14 / 1.6e-14 / 1.3e-09   7.0e-16 / 6.7e-16 / 5.5e-10
    australia8_mf       bordered append + V stream    51  3.0e-14 / 1.6e-14 / 1.3e-09   8.2e-16 / 8.0e-16 / 1.4e-09
    australia8_mf       k = 0 re-predict              33  2.9e-14 / 1.9e-14 / 1.4e-09   7.0e-16 / 6.5e-16 / 5.6e-10
    australia8_mf       batch_predict                 48  3.0e-14 / 1.6e-14 / 1.3e-09   7.0e-16 / 5.9e-16 / 1.3e-09
    australia8_mf       one-launch batch              30  3.0e-14 / 1.9e-14 / 1.4e-09   8.2e-16 / 8.0e-16 / 1.4e-09
    australia8_mf       lattice step                  60  3.0e-14 / 1.9e-14 / 1.4e-09   7.0e-16 / 5.3e-16 / 1.4e-09
    australia8_mf       lattice step, 2nd launch      30  3.0e-14 / 1.9e-14 / 1.4e-09   7.0e-16 / 6.7e-16 / 5.5e-10
    australia8_mf       mfgp_query                     6  2.9e-14 / 1.9e-14 / 1.4e-09   7.0e-16 / 6.5e-16 / 5.6e-10
    australia8_mf       cov_block diagonal             6  -                             1.3e-15 / 9.2e-16 / 3.9e-09
    australia9_mf       full recompute                17  3.1e-15 / 3.2e-15 / 7.8e-11   4.6e-16 / 3.5e-16 / 1.7e-10
    australia9_mf       bordered append + V stream    51  3.3e-15 / 3.2e-15 / 7.9e-11   5.7e-16 / 4.0e-16 / 5.1e-10
    australia9_mf       k = 0 re-predict              33  3.1e-15 / 3.2e-15 / 7.9e-11   4.6e-16 / 3.8e-16 / 5.1e-10
    australia9_mf       batch_predict                 48  3.1e-15 / 3.2e-15 / 7.8e-11   4.6e-16 / 3.7e-16 / 1.5e-10
    australia9_mf       one-launch batch              30  3.3e-15 / 3.2e-15 / 7.9e-11   5.7e-16 / 4.0e-16 / 5.1e-10
    australia9_mf       lattice step                  60  3.1e-15 / 3.2e-15 / 7.8e-11   4.6e-16 / 4.4e-16 / 1.6e-10
    australia9_mf       lattice step, 2nd launch      30  3.1e-15 / 3.2e-15 / 7.8e-11   4.6e-16 / 4.4e-16 / 1.6e-10
    australia9_mf       mfgp_query                     6  3.1e-15 / 3.2e-15 / 7.9e-11   4.6e-16 / 4.0e-16 / 5.1e-10
    australia9_mf       cov_block diagonal             6  -                             6.8e-16 / 3.7e-16 / 1.6e-10
    anti_two_corners_sf full recompute                 6  1.3e-08 / 1.9e-09 / 7.3e-05   3.8e-13 / 1.2e-13 / 1.4e-05
    anti_two_corners_sf bordered append + V stream    18  1.3e-08 / 1.9e-09 / 7.3e-05   4.0e-13 / 9.1e-14 / 1.6e-05
    anti_two_corners_sf k = 0 re-predict              12  1.3e-08 / 1.9e-09 / 7.3e-05   4.0e-13 / 9.1e-14 / 1.6e-05
    anti_two_corners_sf batch_predict                 16  9.6e-09 / 1.2e-09 / 6.3e-05   3.8e-13 / 1.2e-13 / 1.4e-05
    anti_two_corners_sf one-launch batch              10  1.3e-08 / 1.9e-09 / 7.3e-05   4.0e-13 / 9.1e-14 / 1.6e-05
    anti_two_corners_sf mfgp_query                     2  1.3e-08 / 1.9e-09 / 7.3e-05   3.7e-14 / 7.1e-16 / 1.7e-05
    anti_two_corners_sf cov_block diagonal             2  -                             3.7e-14 / 7.1e-16 / 1.7e-05
    anti_two_corners_sf lattice step (V stream)       30  1.3e-08 / 1.9e-09 / 7.3e-05   4.0e-13 / 9.1e-14 / 1.6e-05

No output exceeded its bound; the closest came to 1/511 of it (var of the one-row SF model, 4.4e-16
against 2.3e-13), and the factor of the full recompute to 1/1015 of it against _chol_ld's L. The
anti_two_corners_sf rows of the lattice step ran the V stream: the step's condition gate refuses
them. The lattice step sat inside the oracle's bound everywhere, in-launch and with k_lat_gemm2 as
its second launch (MFGP_LAT_GEMM2=1, lattice_g2 == lattice), so no e_lattice_* was needed. The
cov_block route gives the variance alone.
A k = 0 re-predict into device memory (one sweep over all rows of V) differs from the append's
launch in the last bits (it is held to the fixture and to its own bits on a second run);
predict() again returns the append's bits.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _fixtures as F
from tests import _posterior_edges as E

pytestmark = pytest.mark.gpu

E2, E1 = np.empty((0, 2)), np.empty(0)
ILL = "anti_two_corners_sf"
OFFGRID = [c[0] for c in E.CASES if c[7]][0]
RECORD = []        # (hyp key, route, name, stage, e_mu, b_mu, e_var, b_var, e_oracle_mu, e_oracle_var)


@pytest.fixture(scope="module")
def fx():
    return F.load("posterior_edges_reference.npz")


@pytest.fixture(scope="module")
def ctxs():
    """Private contexts, one per route (nothing to restore): the full recompute; the drop-in
    V stream with the fused launch, without it and with deferred appends; the batch's V
    stream; the lattice step past its size gate with the column store of V and without (both
    with the GEMM tiles in the launch: these batches are far below the chip's size), and with
    its GEMM and cells as the second launch (k_lat_gemm2, MFGP_LAT_GEMM2=1 as the context is
    created: the form the headline workload runs)."""
    from mfgp_coverage_amd import _lib
    c = {k: _lib.Context(0) for k in ("full", "dropin", "fused_off", "deferred", "stream", "lattice", "lattice_novcol")}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MFGP_LAT_GEMM2", "1")
        c["lattice_g2"] = _lib.Context(0)
    c["lattice_g2"].set_lattice("force")
    c["full"].set_incremental(False)
    for k in ("dropin", "fused_off", "deferred", "stream"):
        c[k].set_lattice(False)
    c["fused_off"].set_fused(False)
    c["deferred"].set_deferred_appends(True)
    c["lattice"].set_lattice("force")
    c["lattice_novcol"].set_lattice("force")
    c["lattice_novcol"].set_lattice_vcol(False)
    return c


def _model(ctx, fx, name, s=None):
    """A model of the case's first s rows on its grid (None: no data yet)."""
    from mfgp_coverage_amd import _lib
    _, _, _, _, hyp, jitter, Xs = E.case_inputs(fx, name)
    m = _lib.Model(ctx, _lib.SF if hyp.shape[0] == 4 else _lib.MF, hyp, jitter)
    m.set_grid(Xs)
    if s is not None:
        m.set_data(*E.stage_rows(fx, name, s))
    return m


def _rows(fx, name, a, b):
    """Rows [a, b) of a case (hifi rows: a >= NL)."""
    nl = fx[f"{name}_XL"].shape[0]
    return fx[f"{name}_XH"][a - nl:b - nl], fx[f"{name}_yH"][a - nl:b - nl]


def _meets(fx, name, s, route, mu, var):
    """mu None: a route that gives the variance alone (its mu figure is 0 and counts nowhere)."""
    mu_ref, var_ref, kss = E.stage_ref(fx, name, s)
    e_mu, e_var = E.errors(mu_ref if mu is None else mu, var, mu_ref, var_ref, kss)
    b_mu, b_var = E.bounds(fx, name, s)
    print(f"POST_EDGE {name} s {s} route {route} mu {e_mu:.3e} bound {b_mu:.3e} var {e_var:.3e} bound {b_var:.3e}")
    RECORD.append((E.BY_NAME[name][2], route, name, s, e_mu, b_mu, e_var, b_var,
                   float(fx[f"{name}_s{s}_e_oracle_mu"]), float(fx[f"{name}_s{s}_e_oracle_var"])))
    assert e_mu <= b_mu and e_var <= b_var, (name, s, route, e_mu, b_mu, e_var, b_var)


def _delta(after, before, keys):
    return {k: after[k] - before[k] for k in keys}


# ---------------------------------------------------------------------------
# 1. full recompute: mfgp_set_data, the blocked Cholesky, k_predict
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.NAMES)
def test_full_recompute(fx, ctxs, name):
    """set_data of each stage's rows on a context that refactors and recomputes V on every
    update; the factor itself against _chol_ld's L within the same bound, relative to max |L|."""
    m = _model(ctxs["full"], fx, name)
    _, _, _, _, hyp, jitter, Xs = E.case_inputs(fx, name)
    for s in E.case_stages(name):
        before = m.stats()
        m.set_data(*E.stage_rows(fx, name, s))
        mu, var = m.predict()
        _meets(fx, name, s, "full", mu, var)
        d = _delta(m.stats(), before, ("full_factor", "full_predict", "inc_factor", "vstream", "lattice"))
        if s:
            assert d == {"full_factor": 1, "full_predict": 1, "inc_factor": 0, "vstream": 0, "lattice": 0}, (s, d)
            L = m.factor()
            L_ref = O._chol_ld(O._posterior_parts_ld(*E.stage_rows(fx, name, s), hyp, Xs, jitter)[0])
            e_L = float(np.max(np.abs(L - L_ref)) / np.max(np.abs(L_ref)))
            b_L = min(E.bounds(fx, name, s))
            print(f"POST_EDGE {name} s {s} route full_L L {e_L:.3e} bound {b_L:.3e}")
            assert L.shape == (s, s) and e_L <= b_L, (s, e_L, b_L)


# ---------------------------------------------------------------------------
# 2. the drop-in bordered append of one model: fused, unfused, deferred
# ---------------------------------------------------------------------------

def _repredicts(fx, name, s, route, m, mu, var):
    """Nothing appended: predict() again gives the same bits -- it copies the result the model
    kept and runs no kernel, so that assertion holds the host path only. The kernel's k = 0 pass
    is the predict into device memory: one sweep over all rows of the resident V (k_vstream,
    counted by stats()). That pass sums the
    rows in one sweep where the append's launch added the new rows to the old rows' sums, so
    it is held to the fixture, not to the append's bits; run twice it gives its own bits twice."""
    import torch
    from mfgp_coverage_amd import _lib
    mu2, var2 = m.predict()
    assert mu2.tobytes() == mu.tobytes() and var2.tobytes() == var.tobytes(), (name, s)
    before = m.stats()
    M = mu.shape[0]
    got = []
    for _ in range(2):
        out = torch.full((2 * M,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.batch_predict([m], out.data_ptr(), out.data_ptr() + 8 * M)      # (odd M: var 8-byte aligned)
        got.append(out.cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes(), (name, s)
    _meets(fx, name, s, route + "_k0", got[0][:M], got[0][M:])
    return _delta(m.stats(), before, ("vstream", "full_predict", "full_factor", "inc_factor"))


@pytest.mark.parametrize("route", ["dropin", "fused_off", "deferred"])
@pytest.mark.parametrize("name", E.NAMES)
def test_dropin_append(fx, ctxs, name, route):
    """set_data of the first stage, predict, then append + predict across the edge (8 rows,
    then 1); the off-grid case's appended rows take the fallback forward solve for L21."""
    st = E.case_stages(name)
    m = _model(ctxs[route], fx, name, st[0])
    mu, var = m.predict()
    _meets(fx, name, st[0], route, mu, var)
    for a, b in zip(st, st[1:]):
        m.append(*_rows(fx, name, a, b))
        if route == "deferred" and a > 0:
            assert m.stats()["factor_rows"] == a, m.stats()          # staged: the predict runs it
        mu, var = m.predict()
        _meets(fx, name, b, route, mu, var)
        d = _repredicts(fx, name, b, route, m, mu, var)
        assert d == {"vstream": 2, "full_predict": 0, "full_factor": 0, "inc_factor": 0}, (b, d)
    s = m.stats()
    assert s["inc_factor"] == len(st) - 1 and s["vstream"] >= 3 * (len(st) - 1) and s["lattice"] == 0, s
    assert (s["full_factor"] == 1 or st[0] == 0) and s["factor_rows"] == st[-1] and s["v_rows"] == st[-1], s
    if route != "dropin":
        return
    # the same truth through the consumers of the resident V, at the final stage
    _, _, _, _, _, _, Xs = E.case_inputs(fx, name)
    q = m.query(Xs, mu=True, var0=True, var=False)
    _meets(fx, name, st[-1], "query", q.mu, q.var0)
    C = m.cov_block()
    assert C.shape == (Xs.shape[0], Xs.shape[0])
    _meets(fx, name, st[-1], "cov_diag", None, np.diag(C).copy())
    s2 = m.stats()
    assert s2["look_query"] > s["look_query"], (s, s2)


def test_capacity_growth(fx, ctxs):
    """From one row by appends of 16: the row capacity starts at 63 and grows by 1.5x to
    127 (at row 64) and 191 (at row 128), so A, Linv, z and V are copied to a new leading
    dimension twice before the first stage and a third time at the second (192 rows)."""
    name = "sf_australia3_sf_n193_15x13"
    st = E.case_stages(name)
    assert st == [184, 192, 193]
    m = _model(ctxs["dropin"], fx, name, 1)
    m.predict()
    at, appends = 1, 0
    for s in st:
        while at < s:
            k = min(16, s - at)
            m.append(*_rows(fx, name, at, at + k))
            mu, var = m.predict()
            at += k
            appends += 1
        _meets(fx, name, s, "growth", mu, var)
    s = m.stats()
    assert appends == 14 and s["inc_factor"] == appends and s["vstream"] >= appends and s["full_factor"] == 1, s


# ---------------------------------------------------------------------------
# 3. the batch entry points: one k_inc_stream launch, the lattice step, k_post_copy
# ---------------------------------------------------------------------------

# ragged batches of 2 and of 4: other grids, other N and NL, SF beside MF, both australia MF
# sets, odd M in front so that the next member's outputs are only 8-byte aligned
BATCHES = {
    "b2_n63_n129": ["sf_australia3_sf_n63_8x8", "mf_australia8_mf_n129_nl63_13x11"],
    "b4_n64_n65": ["sf_australia3_sf_n64_13x5", "sf_australia3_sf_n65_13x11", "mf_australia9_mf_n64_nl0_8x8",
                   "mf_australia8_mf_n65_nl64_13x5"],
    "b4_n128_n129": ["sf_australia3_sf_n128_43x3", "sf_australia3_sf_n129_13x11", "mf_australia9_mf_n129_nl64_43x3",
                     "mf_australia8_mf_n129_nl65_16x9"],
    "b4_n193_offgrid": ["sf_australia3_sf_n193_15x13", "mf_australia8_mf_n193_nl128_15x13",
                        "mf_australia9_mf_n193_nl128_15x13", OFFGRID],
    "b4_mf": ["mf_australia9_mf_n65_nl64_13x5", "mf_australia8_mf_n64_nl0_8x8", "mf_australia9_mf_n129_nl63_13x11",
              "mf_australia8_mf_n129_nl64_43x3"],
    "b2_n1": ["sf_australia3_sf_n1_9x7", "mf_australia9_mf_n129_nl65_16x9"],
    "b2_ill": ["sf_anti_two_corners_sf_n65_13x5", "sf_anti_two_corners_sf_n129_13x11"],
}


def test_batches_hold_every_case():
    assert sorted(n for b in BATCHES.values() for n in b) == sorted(E.NAMES)


def _stages3(name):
    """[N - 9, N - 1, N], none below NL: a case with fewer stages appends nothing in a step."""
    _, _, _, n, nl, _, _, _ = E.BY_NAME[name]
    return [max(nl, n - E.TAIL), max(nl, n - 1), n]


class _Batch:
    """The cases of one batch as models on one context, stepped through the batch entry
    points with device outputs and the fused max / argmax."""

    def __init__(self, ctx, fx, names):
        import torch
        self.fx, self.names = fx, names
        self.at = [_stages3(n)[0] for n in names]
        self.models = [_model(ctx, fx, n, s) for n, s in zip(names, self.at)]
        Ms = [fx[f"{n}_Xs"].shape[0] for n in names]
        self.off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
        self.mu = torch.empty(int(self.off[-1]), dtype=torch.float64, device="cuda")
        self.var = torch.empty_like(self.mu)
        self.vmax = torch.empty(len(names), dtype=torch.float64, device="cuda")
        self.vam = torch.empty(len(names), dtype=torch.int64, device="cuda")

    def _outs(self):
        mu, var = self.mu.cpu().numpy(), self.var.cpu().numpy()
        return [(mu[a:b].copy(), var[a:b].copy()) for a, b in zip(self.off, self.off[1:])]

    def predict(self):
        from mfgp_coverage_amd import _lib
        self.mu.fill_(float("nan"))
        self.var.fill_(float("nan"))
        _lib.batch_predict(self.models, self.mu.data_ptr(), self.var.data_ptr())
        return self._outs()

    def step(self, to):
        """Append the rows up to `to[i]` to member i (none where it is there already) and
        predict: per member (mu, var); the fused max / argmax are checked here."""
        from mfgp_coverage_amd import _lib
        rows = [_rows(self.fx, n, a, b) for n, a, b in zip(self.names, self.at, to)]
        ks = [b - a for a, b in zip(self.at, to)]
        Xn = np.ascontiguousarray(np.concatenate([r[0] for r in rows] + [np.zeros((1, 2))]))
        yn = np.ascontiguousarray(np.concatenate([r[1] for r in rows] + [np.zeros(1)]))
        self.mu.fill_(float("nan"))
        self.var.fill_(float("nan"))
        self.vmax.fill_(float("nan"))
        self.vam.fill_(-1)
        _lib.batch_append_predict(self.models, Xn.ctypes.data, yn.ctypes.data, ks, self.mu.data_ptr(),
                                  self.var.data_ptr(), vmax_ptr=self.vmax.data_ptr(), vargmax_ptr=self.vam.data_ptr())
        self.at = list(to)
        outs = self._outs()
        vmax, vam = self.vmax.cpu().numpy(), self.vam.cpu().numpy()
        for i, (_, var) in enumerate(outs):
            assert vmax[i] == var.max() and vam[i] == int(np.argmax(var)), (self.names[i], vmax[i], vam[i])
        return outs

    def stats(self):
        return [m.stats() for m in self.models]


COUNTERS = ("inc_factor", "vstream", "lattice", "post_copy", "full_factor", "full_predict")


def _run_batch(ctx, fx, names, plan, route, lattice):
    """batch_predict at the first stage, one step to N - 1, then to N -- all members at once
    (plan "all") or in two further steps, the even members first and the odd ones after
    (plan "halves": the others append nothing and are served from their resident posterior).
    Every output meets the fixture; the path counters say which launch served each member."""
    b = _Batch(ctx, fx, names)
    st3 = [_stages3(n) for n in names]
    outs = [b.predict()]
    for i, n in enumerate(names):
        _meets(fx, n, b.at[i], route + "_predict", *outs[0][i])
    targets = [[s[1] for s in st3]]
    if plan == "all":
        targets.append([s[2] for s in st3])
    else:
        targets.append([s[2] if i % 2 == 0 else s[1] for i, s in enumerate(st3)])
        targets.append([s[2] for s in st3])
    ill = any(E.BY_NAME[n][2] == ILL for n in names)
    want = [dict.fromkeys(COUNTERS, 0) for _ in names]
    for to in targets:
        before, at = b.stats(), list(b.at)
        outs.append(b.step(to))
        after = b.stats()
        ks = [t - a for a, t in zip(at, to)]
        # the lattice step takes a launch whose appending members all hold rows and pass its
        # condition gate k** / (noise + jitter) <= 1e4
        lat = lattice and not ill and all(a >= 1 for a, k in zip(at, ks) if k > 0)
        for i, n in enumerate(names):
            _meets(fx, n, to[i], route, *outs[-1][i])
            d = _delta(after[i], before[i], COUNTERS)
            if ks[i] > 0:
                assert d == {"inc_factor": 1, "vstream": 1, "lattice": int(lat), "post_copy": 0, "full_factor": 0,
                             "full_predict": 0}, (n, to[i], d)
            else:
                # nothing appended: the bits of the member's last predict, copied by k_post_copy
                prev_mu, prev_var = outs[-2][i]
                assert outs[-1][i][0].tobytes() == prev_mu.tobytes() and outs[-1][i][1].tobytes() == prev_var.tobytes(), n
                assert d == {"inc_factor": 0, "vstream": 0, "lattice": 0, "post_copy": 1, "full_factor": 0,
                             "full_predict": 0}, (n, to[i], d)
            for k in COUNTERS:
                want[i][k] += d[k]
    return b, outs, want


@pytest.mark.parametrize("plan", ["all", "halves"])
@pytest.mark.parametrize("bname", list(BATCHES))
def test_batch_stream(fx, ctxs, bname, plan):
    """The one-launch batch with the lattice step off: bordered append + one-pass predict of
    every appending member in one k_inc_stream launch, k_post_copy for the others."""
    b, _, want = _run_batch(ctxs["stream"], fx, BATCHES[bname], plan, "batch_stream", lattice=False)
    for s, w in zip(b.stats(), want):
        assert s["lattice"] == 0 and s["inc_factor"] == w["inc_factor"] >= 1 and s["vstream"] >= w["vstream"] >= 1, s
    if plan == "halves":
        assert all(w["post_copy"] >= 1 for w in want), want


@pytest.mark.parametrize("plan", ["all", "halves"])
@pytest.mark.parametrize("bname", list(BATCHES))
def test_batch_lattice(fx, ctxs, bname, plan):
    """The same batches with the lattice step forced: with the column store of V and without
    it (the same bits), and with k_lat_gemm2 as its second launch. The step takes every appending launch of the australia cases whose
    members all hold at least one row; the anti_two_corners_sf cases fail its condition gate
    and meet their bound through the V stream; the off-grid case's tail rows are virtual rows."""
    names = BATCHES[bname]
    b, outs, want = _run_batch(ctxs["lattice"], fx, names, plan, "batch_lattice", lattice=True)
    b2, outs2, want2 = _run_batch(ctxs["lattice_novcol"], fx, names, plan, "batch_lattice_novcol", lattice=True)
    assert want == want2
    for step, (oa, ob) in enumerate(zip(outs, outs2)):
        for n, (mu_a, var_a), (mu_b, var_b) in zip(names, oa, ob):
            assert mu_a.tobytes() == mu_b.tobytes() and var_a.tobytes() == var_b.tobytes(), (step, n)
    # ... and with the GEMM and cells as the second launch: another summation order (four K
    # splits inside a workgroup), so held to the fixture, not to the in-launch form's bits
    b3, _, want3 = _run_batch(ctxs["lattice_g2"], fx, names, plan, "batch_lattice_g2", lattice=True)
    assert want3 == want
    for n, s, s2, s3, w in zip(names, b.stats(), b2.stats(), b3.stats(), want):
        key, n0 = E.BY_NAME[n][2], _stages3(n)[0]
        assert s["lattice"] == s2["lattice"] == s3["lattice"] == w["lattice"], (n, s, s2, s3)
        assert s["lattice_g2"] == 0 and s2["lattice_g2"] == 0 and s3["lattice_g2"] == s3["lattice"], (n, s, s2, s3)
        # the store-on run read the store (else both runs took the compact rows and their equal
        # bits would say nothing); a step whose new rows are off the cells does not count
        assert s2["lattice_vcol"] == 0 and s2["vcol_rows_built"] == 0, (n, s2)
        if n == OFFGRID:
            assert s["lattice"] == 2 and s["lattice_vcol"] == 0, (n, s)
        else:
            assert s["lattice_vcol"] == s["lattice"] and (s["vcol_rows_built"] > 0) == (s["lattice"] > 0), (n, s)
        if key == ILL:
            assert s["lattice"] == 0 and s["vstream"] >= w["vstream"] >= 2, (n, s)
        elif n0 >= 1 and bname != "b2_n1":
            assert s["lattice"] == w["inc_factor"] >= 1, (n, s)          # every append of this case
        elif n0 >= 1:
            assert s["lattice"] >= 1, (n, s)      # (its 8-row step; the 1-row step runs beside the empty model's)
        if n == OFFGRID:
            assert s["lattice_virtual"] > 0 and s2["lattice_virtual"] == s["lattice_virtual"], (s, s2)


# ---------------------------------------------------------------------------
# 4. exact ties: the fused argmax is the first maximal cell
# ---------------------------------------------------------------------------

def _prior_variance_libm(hyp):
    """oracle.gp_oracle.prior_variance, the same operations in the same order, with the C
    library's exp (math.exp) in place of np.exp. The library's host code calls the C library's;
    NumPy's own vectorised exp is an ulp off it at australia3_sf's log s^2 (0.09362397763413459
    against 0.0936239776341346, which is also what the extended-precision value rounds to), so
    a bit-for-bit check has to evaluate the formula with the exp the formula's user has."""
    import math
    if hyp.shape[0] == 4:
        return np.float64(math.exp(hyp[1]))
    rho = math.exp(hyp[6])
    return np.float64(rho ** 2 * math.exp(hyp[1]) + math.exp(hyp[4]))


def _empty_models(ctx):
    """An N = 0 model on each of the seven grids, SF and MF alternating."""
    from mfgp_coverage_amd import _lib, synthetic
    ms, hyps = [], []
    for i, (nx, ny) in enumerate(E.GRIDS):
        hyp = synthetic.HYP["australia3_sf" if i % 2 == 0 else "australia8_mf"]
        m = _lib.Model(ctx, _lib.SF if hyp.shape[0] == 4 else _lib.MF, hyp, O.JITTER)
        m.set_grid(E.make_grid(nx, ny))
        m.set_data(E2, E1, E2, E1)
        ms.append(m)
        hyps.append(hyp)
    return ms, hyps


@pytest.mark.parametrize("route", ["stream", "lattice"])
def test_empty_models_are_the_prior_bit_for_bit(ctxs, route):
    """Constant variance: every cell is maximal. Through a batch step of fresh models,
    batch_predict and k_post_copy (odd M: the scalar branch for every member behind the
    first), var is the prior variance bit for bit (_prior_variance_libm; within an ulp of
    prior_variance(hyp), whose np.exp is not the C library's), vmax equals it and vargmax is
    cell 0."""
    import torch
    from mfgp_coverage_amd import _lib
    ms, hyps = _empty_models(ctxs[route])
    Ms = [nx * ny for nx, ny in E.GRIDS]
    off = np.concatenate([[0], np.cumsum(Ms)])
    mu = torch.empty(int(off[-1]), dtype=torch.float64, device="cuda")
    var = torch.empty_like(mu)
    vmax = torch.empty(len(ms), dtype=torch.float64, device="cuda")
    vam = torch.empty(len(ms), dtype=torch.int64, device="cuda")
    dummy_X, dummy_y = np.zeros((1, 2)), np.zeros(1)

    def check(tag, with_max):
        v, u = var.cpu().numpy(), mu.cpu().numpy()
        for i, hyp in enumerate(hyps):
            kss = _prior_variance_libm(hyp)
            assert abs(kss - O.prior_variance(hyp)) <= np.spacing(kss)
            seg = v[off[i]:off[i + 1]]
            assert seg.tobytes() == np.full(Ms[i], kss).tobytes(), (tag, i, seg[0], kss)
            assert np.all(u[off[i]:off[i + 1]] == u[off[i]]) and abs(u[off[i]] - O.prior_mean(hyp)) <= 4 * np.spacing(u[off[i]])
            if with_max:
                assert vmax.cpu().numpy()[i].tobytes() == kss.tobytes() and int(vam.cpu().numpy()[i]) == 0, (tag, i)

    def step():
        for t in (mu, var, vmax):
            t.fill_(float("nan"))
        vam.fill_(-1)
        _lib.batch_append_predict(ms, dummy_X.ctypes.data, dummy_y.ctypes.data, [0] * len(ms), mu.data_ptr(),
                                  var.data_ptr(), vmax_ptr=vmax.data_ptr(), vargmax_ptr=vam.data_ptr())

    step()                                             # fresh models: the batch step computes them
    check("batch step", True)
    assert all(m.stats()["post_copy"] == 0 for m in ms)
    mu.fill_(float("nan"))
    var.fill_(float("nan"))
    _lib.batch_predict(ms, mu.data_ptr(), var.data_ptr())
    check("batch_predict", False)
    pc0 = [m.stats()["post_copy"] for m in ms]
    step()                                             # nothing changed: k_post_copy
    check("post_copy", True)
    pc1 = [m.stats()["post_copy"] for m in ms]
    print(f"POST_EDGE empty models route {route} post_copy {pc0} -> {pc1}")
    assert all(b == a + 1 for a, b in zip(pc0, pc1)), (pc0, pc1)


@pytest.mark.parametrize("route", ["stream", "lattice"])
def test_symmetric_variance_argmax_is_the_first_maximal_cell(ctxs, route):
    """One observation at the centre cell of the 9 x 7 grid: the four corners are equally far
    from it (0.5 - 0 and 1 - 0.5 are exact), so their variances tie. The fused argmax of a
    full predict in a batch step, of a bordered append from the empty model and of
    k_post_copy is the first of the maximal cells."""
    import torch
    from mfgp_coverage_amd import _lib, synthetic
    hyp = synthetic.HYP["australia3_sf"]
    Xs = E.make_grid(9, 7)
    centre = Xs[4 * 7 + 3:4 * 7 + 4].copy()
    assert np.array_equal(centre, [[0.5, 0.5]])
    y1 = np.array([0.7])
    mu = torch.empty(63, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mu)
    vmax = torch.empty(1, dtype=torch.float64, device="cuda")
    vam = torch.empty(1, dtype=torch.int64, device="cuda")
    checked = []

    def step(m, X, y, tag):
        var.fill_(float("nan"))
        vam.fill_(-1)
        Xn = np.ascontiguousarray(np.vstack([X, np.zeros((1, 2))]))
        yn = np.ascontiguousarray(np.concatenate([y, np.zeros(1)]))
        _lib.batch_append_predict([m], Xn.ctypes.data, yn.ctypes.data, [X.shape[0]], mu.data_ptr(), var.data_ptr(),
                                  vmax_ptr=vmax.data_ptr(), vargmax_ptr=vam.data_ptr())
        v = var.cpu().numpy()
        top = np.flatnonzero(v == v.max())
        print(f"POST_EDGE symmetric route {route} {tag} maximal cells {top.tolist()} vargmax {int(vam.cpu().numpy()[0])}")
        assert vmax.cpu().numpy()[0] == v.max()
        if top.shape[0] >= 2:
            assert int(vam.cpu().numpy()[0]) == int(top[0]) == 0, (tag, top)
            checked.append(tag)
        return v.copy()

    a = _lib.Model(ctxs[route], _lib.SF, hyp, O.JITTER)            # the row set at once: factor + k_predict
    a.set_grid(Xs)
    a.set_data(E2, E1, centre, y1)
    va = step(a, E2, E1, "full")
    b = _lib.Model(ctxs[route], _lib.SF, hyp, O.JITTER)            # appended to the empty model
    b.set_grid(Xs)
    b.set_data(E2, E1, E2, E1)
    step(b, E2, E1, "empty")
    vb = step(b, centre, y1, "append")
    pc = b.stats()["post_copy"]
    vc = step(b, E2, E1, "post_copy")
    assert b.stats()["post_copy"] == pc + 1 and vc.tobytes() == vb.tobytes()
    mu_r, var_r, kss = O.posterior_extended(E2, E1, centre, y1, hyp, Xs) if np.finfo(np.longdouble).eps < 1e-18 \
        else (None, O.sf_diag(centre, y1, hyp, Xs)[1], O.prior_variance(hyp))
    for v in (va, vb):
        assert np.max(np.abs(v - var_r.astype(np.float64))) / float(kss) <= E.bound_of(0.0, 1.0, 1)
    if len(checked) < 4:
        pytest.skip(f"the returned variance had a single maximal cell on some route (ties checked on {checked}): "
                    "the first-of-the-maximal-cells assertion did not run there")


# ---------------------------------------------------------------------------
# 5. the figures of this run
# ---------------------------------------------------------------------------

def test_zz_summary():
    """Prints, per hyperparameter set and route, the largest error over the cases and stages
    that ran (device / fp64 oracle / bound of that stage), for mu and for var, and the
    closest approach of any error to its bound."""
    groups = {}
    closest = 0.0
    for key, route, name, s, e_mu, b_mu, e_var, b_var, o_mu, o_var in RECORD:
        g = groups.setdefault((key, route), [None, None, 0])
        if g[0] is None or e_mu > g[0][0]:
            g[0] = (e_mu, o_mu, b_mu, name, s)
        if g[1] is None or e_var > g[1][0]:
            g[1] = (e_var, o_var, b_var, name, s)
        g[2] += 1
        closest = max(closest, e_mu / b_mu, e_var / b_var)
    for (key, route), (gm, gv, cnt) in sorted(groups.items()):
        print(f"POST_EDGE_SUMMARY {key:20s} {route:22s} n {cnt:3d}  mu {gm[0]:.1e} / {gm[1]:.1e} / {gm[2]:.1e} "
              f"({gm[3]} s{gm[4]})  var {gv[0]:.1e} / {gv[1]:.1e} / {gv[2]:.1e} ({gv[3]} s{gv[4]})")
    print(f"POST_EDGE_SUMMARY closest approach to a bound: {closest:.3g} of it")
    assert closest <= 1.0
