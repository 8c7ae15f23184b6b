"""Integrated variance reduction per candidate cell from the resident V (k_ivr_partial,
k_ivr_finish, k_ivr_best; mfgp_var_reduction).

The reference is tests/_ivr.py: the closed form on the oracle's dense covariance, in the
floored-relative metric
    max_c |ivr - ref| / max(|ref|, 1e-6 k** sum_i |w_i|) <= O.PARITY_TOL.
Comparisons between calls on the same model are bit for bit: a score's bits depend only on
the model, its cell and its weight vector. Measured maxima against the reference (MI355X):
see DESIGN.md section 20.
"""
import copy
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _ivr as I

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL


def _build(ctx, kind, Xs, X, y, NL, hyp=None):
    from mfgp_coverage_amd import _lib
    if X.shape[0] == 0:      # a model that never saw data: a grid, no factor
        m = _lib.Model(ctx, _lib.SF if kind == "sf" else _lib.MF, I.hyp_of(kind) if hyp is None else hyp, 1e-8)
        m.set_grid(Xs)
        return m
    return I._model(ctx, kind, X, y, NL, Xs, hyp=hyp)


_CASES = {}


def _case(kind, gname, N=197):
    """One model per (kind, grid, N), its all-cells scores under no weights and the oracle's
    dense covariance: computed once, shared, never modified."""
    key = (kind, gname, N)
    if key not in _CASES:
        from mfgp_coverage_amd import _lib
        Xs = I.grid(gname)
        X, y, NL = I.data(kind, Xs, N, seed=7 + N + len(gname) + len(kind))
        m = _build(_lib.context(), kind, Xs, X, y, NL)
        full = m.var_reduction()
        full.flags.writeable = False
        C = I.dense_cov(kind, X, y, NL, Xs, I.hyp_of(kind))
        _CASES[key] = (m, full, C, Xs)
    return _CASES[key]


# ---- 1. against the reference ------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sf", "mf"])
@pytest.mark.parametrize("gname", ["9x7", "13x11", "40x33"])       # M = 63, 143, 1320 (3 row segments)
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 197])
def test_against_the_reference(kind, gname, N):
    from mfgp_coverage_amd._lib import IVR_SEG_CELLS
    m, full, C, Xs = _case(kind, gname, N)
    M = Xs.shape[0]
    if gname == "40x33":
        assert M > 2 * IVR_SEG_CELLS       # at least two row segments are exercised
    hyp = I.hyp_of(kind)
    assert full.shape == (M,)
    worst = {"none": I.err(full, I.ivr_closed(C, hyp), hyp, None, M)}
    for name, w in I.weight_sets(M, seed=11 + N).items():
        got = m.var_reduction(weights=w)
        assert got.shape == ((w.shape[0], M) if w.ndim == 2 else (M,))
        worst[name] = I.err(got, I.ivr_closed(C, hyp, w), hyp, w, M)
    print(f"ivr {kind} {gname} N = {N}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL, worst


# ---- 2. candidate lists ----------------------------------------------------------------------

LISTS = [[5], list(range(37, 100)), list(range(101, 166)), [700, 3, 3, 1319, 64, 63]]


@pytest.mark.parametrize("cand", LISTS, ids=["one", "run63", "run65", "unsorted"])
def test_candidate_lists_equal_the_all_cells_entries(cand):
    m, full, _, Xs = _case("mf", "40x33")
    w = I.weight_sets(Xs.shape[0], seed=21)["w3"]
    fullw = m.var_reduction(weights=w)
    got = m.var_reduction(cand)
    assert got.shape == (len(cand),)
    assert np.array_equal(got, full[cand])
    gw = m.var_reduction(cand, w)
    assert np.array_equal(gw, fullw[:, cand])
    perm = np.random.default_rng(22).permutation(len(cand))
    assert np.array_equal(m.var_reduction(np.asarray(cand)[perm], w), gw[:, perm])
    for j in sorted(set(range(len(cand))) & {0, 1, 2, len(cand) // 2, len(cand) - 1}):
        assert np.array_equal(m.var_reduction([cand[j]], w)[:, 0], gw[:, j])


# ---- 3. weights ----------------------------------------------------------------------------------

def test_weight_rows_are_independent():
    m, full, _, Xs = _case("mf", "40x33")
    M = Xs.shape[0]
    ws = I.weight_sets(M, seed=31)
    cand = list(range(600, 760))
    for name in ("w3", "w8"):
        multi = m.var_reduction(cand, ws[name])
        assert np.array_equal(m.var_reduction(cand, ws[name]), multi)          # two calls agree
        for k, wk in enumerate(ws[name]):
            assert np.array_equal(m.var_reduction(cand, wk), multi[k]), (name, k)
    assert np.array_equal(m.var_reduction(weights=np.ones(M)), full)            # explicit ones == None
    assert np.array_equal(m.var_reduction(), full)
    # an out wider than the list: the padding keeps its sentinel
    out = np.full((3, len(cand) + 2), -7.25)
    r = m.var_reduction(cand, ws["w3"], out=out)
    assert np.array_equal(r, m.var_reduction(cand, ws["w3"])) and np.all(out[:, len(cand):] == -7.25)


def test_device_weights_and_output_equal_host():
    import torch
    m, full, _, Xs = _case("mf", "40x33")
    M = Xs.shape[0]
    w = I.weight_sets(M, seed=33)["w3"]
    cand = [1319, 0, 65, 64, 700] + list(range(300, 420))
    want = m.var_reduction(cand, w)
    wd = torch.zeros((3, M + 8), dtype=torch.float64, device="cuda")
    wd[:, :M] = torch.from_numpy(w).cuda()
    od = torch.full((3, len(cand) + 2), -1.5, dtype=torch.float64, device="cuda")
    res, best, pos = m.var_reduction(cand, wd, out=od, with_best=True)
    assert res is None
    h = od.cpu().numpy()
    assert np.array_equal(h[:, :len(cand)], want) and np.all(h[:, len(cand):] == -1.5)
    assert np.array_equal(best, want.max(1)) and np.array_equal(pos, want.argmax(1))


# ---- 4. best / best_pos --------------------------------------------------------------------------

def test_best_and_best_pos():
    m, full, _, Xs = _case("sf", "40x33")
    M = Xs.shape[0]
    w = I.weight_sets(M, seed=41)["w8"]
    s, best, pos = m.var_reduction(weights=w, with_best=True)          # 6 finish workgroups
    assert best.shape == (8,) and pos.shape == (8,)
    assert np.array_equal(best, s.max(1)) and np.array_equal(pos, s.argmax(1))
    s1, b1, p1 = m.var_reduction(with_best=True)
    assert isinstance(p1, int) and b1 == full.max() and p1 == int(full.argmax())
    # the repeated candidate is a tie: the first position wins
    top = int(full.argmax())
    cand = [700, top, top, 1319, 64, top]
    s2, b2, p2 = m.var_reduction(cand, with_best=True)
    assert s2[1] == s2[2] == s2[5] == b2 and p2 == 1
    s3, b3, p3 = m.var_reduction([700, 3, 3, 1319, 64, 63], with_best=True)
    assert s3[1] == s3[2] and b3 == s3.max() and p3 == int(s3.argmax())


# ---- 5. end to end on the device, without the oracle -------------------------------------------------

@pytest.mark.parametrize("kind", ["sf", "mf"])
def test_equals_lookahead_and_a_real_append(kind):
    from mfgp_coverage_amd.gaussian_process import MFGP, SFGP
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    X, y, NL = I.data(kind, Xs, 90, seed=51)
    y2 = y.reshape(-1, 1)
    if kind == "sf":
        gp = SFGP(X, y2, 1)
        gp.hyp = hyp.copy()
        gp.updt_info(gp.X, gp.y)
    else:
        gp = MFGP(X[:NL], y2[:NL], X[NL:], y2[NL:], 1, 1)
        gp.hyp = hyp.copy()
        gp.updt_info(gp.X_L, gp.y_L, gp.X_H, gp.y_H)
    cand = [0, 5, 64, 71, 100, 127, 128, 142]
    w = I.weight_sets(M, seed=52)["w3"]
    got = gp.variance_reduction(Xs, cand, w)
    assert got.shape == (3, 8)

    def look(xc):
        if kind == "mf":
            return gp.pred_var_diag(Xs, [], xc)
        return gp._query(Xs, None, xc, mu=False, var=True).var
    v0 = look(np.empty((0, 2)))
    la = np.stack([w @ (v0 - look(Xs[c:c + 1])) for c in cand], axis=1)
    e_look = I.err(got, la, hyp, w, M)
    ap = np.empty_like(la)
    var0 = np.diag(gp.predict(Xs)[1]).copy()
    for j, c in enumerate(cand):
        g2 = copy.deepcopy(gp)
        (g2.updt if kind == "sf" else g2.updt_hifi)(Xs[c:c + 1], np.zeros((1, 1)))
        ap[:, j] = w @ (var0 - np.diag(g2.predict(Xs)[1]))
    e_app = I.err(got, ap, hyp, w, M)
    print(f"ivr {kind} 13x11 vs look-ahead {e_look:.3e}, vs deepcopy + append + predict {e_app:.3e}")
    assert e_look <= TOL and e_app <= TOL


# ---- 6. after every update path --------------------------------------------------------------------

def test_after_every_update_path():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    Xs = I.grid("24x24")
    M = Xs.shape[0]
    Xall, yall = I._distinct(Xs, 260, seed=61)
    NL, n = 60, 150
    X, y = Xall[:n].copy(), yall[:n].copy()
    hyp = I.HYP_MF
    m = I._model(ctx, "mf", X, y, NL, Xs)
    w = I.weight_sets(M, seed=62)["w3"]
    nxt = [n]

    def take(k):
        a = nxt[0]
        nxt[0] += k
        return Xall[a:a + k], yall[a:a + k]

    def check(tag, Xs_=None, hyp_=None, w_=w):
        g = Xs if Xs_ is None else Xs_
        h = hyp if hyp_ is None else hyp_
        ref = I.ivr_closed(I.dense_cov("mf", X, y, NL, g, h), h, w_)
        e = I.err(m.var_reduction(weights=w_), ref, h, w_, g.shape[0])
        print(f"ivr after {tag}: N = {X.shape[0]}, error {e:.3e}")
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
    fp = m.stats()["full_predict"]
    check("truncate")
    assert m.stats()["full_predict"] == fp       # served from the rows V holds
    ctx.set_deferred_appends(True)               # a deferred append that the call itself settles
    Xa, ya = take(3)
    m.predict()
    m.append(Xa, ya)
    X, y = np.vstack((X, Xa)), np.concatenate((y, ya))
    assert m.stats()["v_rows"] == X.shape[0] - 3
    check("a deferred append")
    assert m.stats()["v_rows"] == X.shape[0] and m.stats()["factor_rows"] == X.shape[0]
    ctx.set_deferred_appends(False)
    hyp = I.HYP_MF.copy()                        # new hyperparameters
    hyp[2] += 0.2
    hyp[5] -= 0.1
    hyp[8] += 0.3
    m.set_hyp(hyp, 1e-8)
    check("a hyperparameter change")
    Xs2 = I.grid("9x7")                          # another grid
    m.set_grid(Xs2)
    check("a new grid", Xs_=Xs2, w_=I.weight_sets(63, seed=63)["w3"])


# ---- 7. the model is untouched ----------------------------------------------------------------------

def test_the_model_is_untouched():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    Xs = I.grid("24x24")
    M = Xs.shape[0]
    Xall, yall = I._distinct(Xs, 140, seed=71)
    a = I._model(ctx, "mf", Xall[:130], yall[:130], 60, Xs)
    b = I._model(ctx, "mf", Xall[:130], yall[:130], 60, Xs)
    for m in (a, b):
        m.predict()
    mu0, var0 = a.predict()
    st0, se0 = a.stats(), a.serial()
    w = I.weight_sets(M, seed=72)["w8"]
    s = a.var_reduction(list(range(100, 400)), w, with_best=True)[0]
    assert np.all(np.isfinite(s))
    assert a.stats() == st0 and a.serial() == se0
    mu1, var1 = a.predict()
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    st1 = a.stats()
    sb = b.stats()
    b.predict()
    sb1 = b.stats()
    assert {k: st1[k] - st0[k] for k in st0} == {k: sb1[k] - sb[k] for k in sb}
    # the next append takes the path it would have taken
    for m in (a, b):
        m.append(Xall[130:], yall[130:])
    ra, rb = a.predict(), b.predict()
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    assert {k: a.stats()[k] - st1[k] for k in st1} == {k: b.stats()[k] - sb1[k] for k in sb1}


# ---- 8. errors ---------------------------------------------------------------------------------------

def test_errors_leave_the_model_usable():
    from mfgp_coverage_amd import _lib
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    X, y = I._distinct(Xs, 70, seed=81)
    m = I._model(_lib.context(), "sf", X, y, 0, Xs)
    w = I.weight_sets(M, seed=82)["w3"]
    good = m.var_reduction([1, 2, 100], w)
    st, se = m.stats(), m.serial()
    L = _lib.lib()
    out = np.zeros((9, M))
    wbuf = np.ones((9, M))

    def raw(cand, nc, wp, nw, ldw, ldo):
        ca = None if cand is None else np.asarray(cand, dtype=np.int64)
        return L.mfgp_var_reduction(m.handle, None if ca is None else ctypes.c_void_p(ca.ctypes.data), nc,
                                    None if wp is None else ctypes.c_void_p(wp.ctypes.data), nw, ldw,
                                    ctypes.c_void_p(out.ctypes.data), ldo, None, None)
    for cand in ([-1], [M], [0, M, 1]):
        with pytest.raises(ValueError, match="outside the grid"):
            m.var_reduction(cand)
    with pytest.raises(ValueError, match="nw"):
        m.var_reduction([0], wbuf)                                   # nw = 9
    with pytest.raises(ValueError, match="nw"):
        _lib.check(raw([0], 1, wbuf, 0, M, M))                       # nw = 0
    with pytest.raises(ValueError, match="nw"):
        _lib.check(raw([0], 1, None, 2, M, M))                       # NULL weights mean nw = 1
    with pytest.raises(ValueError, match="ldw"):
        _lib.check(raw([0], 1, wbuf, 2, M - 1, M))
    with pytest.raises(ValueError, match="ldo"):
        _lib.check(raw([0, 1, 2], 3, wbuf, 2, M, 2))
    with pytest.raises(ValueError, match="ldo"):
        m.var_reduction([0, 1, 2], w, out=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="all"):
        _lib.check(raw(None, 3, None, 1, M, M))                      # NULL list: nc must be M
    for bad in (np.nan, np.inf):
        wb = w.copy()
        wb[1, M - 1] = bad
        with pytest.raises(ValueError, match="finite"):
            m.var_reduction([0], wb)
    assert m.var_reduction([]).shape == (0,)                         # nc = 0: OK, nothing written
    assert m.stats() == st and m.serial() == se
    assert np.array_equal(m.var_reduction([1, 2, 100], w), good)
    mu, var = m.predict()
    mu_r, var_r = O.sf_diag(X, y, I.HYP_SF, Xs)
    assert max(O.parity_errors(mu, var, mu_r, var_r, O.prior_variance(I.HYP_SF))) < TOL
    g = _lib.Model(_lib.context(), _lib.SF, I.HYP_SF, 1e-8)
    with pytest.raises(ValueError, match="no grid"):
        g.var_reduction([])


def test_f32_model_raises():
    from mfgp_coverage_amd import _lib
    from mfgp_coverage_amd.gaussian_process import SFGP
    Xs = I.grid("13x11")
    X, y = I._distinct(Xs, 40, seed=83)
    m = I._model(_lib.context(), "sf", X, y, 0, Xs, dtype=_lib.F32)
    m.predict()
    with pytest.raises(ValueError, match="MFGP_F32"):
        m.var_reduction([0])
    gp = SFGP(X, y.reshape(-1, 1), 1)
    gp.precision = "f32"
    gp.hyp = I.HYP_SF
    gp.updt_info(gp.X, gp.y)
    with pytest.raises(TypeError):
        gp.variance_reduction(Xs)


# ---- 9. the drop-in classes ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sf", "mf"])
def test_dropin_variance_reduction(kind):
    from mfgp_coverage_amd.gaussian_process import MFGP, SFGP
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    hyp = I.hyp_of(kind)
    X, y = I._distinct(Xs, 90, seed=91)
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
    w = I.weight_sets(M, seed=92)
    s = gp.variance_reduction(Xs)
    assert s.shape == (M,)
    assert np.array_equal(s, gp._dev().var_reduction())
    assert I.err(s, I.ivr_closed(I.dense_cov(kind, X, y, NL, Xs, hyp), hyp), hyp, None, M) <= TOL
    cand = [3, 140, 3, 77]
    assert np.array_equal(gp.variance_reduction(Xs, cand), s[cand])
    s3 = gp.variance_reduction(Xs, cand, w["w3"])
    assert s3.shape == (3, 4) and np.array_equal(s3, gp._dev().var_reduction(cand, w["w3"]))
    s1 = gp.variance_reduction(Xs, weights=w["mask"])
    assert s1.shape == (M,) and np.array_equal(s1[cand], s3[1])
    # another X_star moves the device to the new grid, as predict does
    Xs2 = I.grid("9x7")
    s2 = gp.variance_reduction(Xs2)
    assert s2.shape == (63,)
    assert I.err(s2, I.ivr_closed(I.dense_cov(kind, X, y, NL, Xs2, hyp), hyp), hyp, None, 63) <= TOL
