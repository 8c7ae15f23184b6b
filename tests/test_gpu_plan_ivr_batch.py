"""The batched greedy integrated-variance planner with per-group quotas (mfgp_batch_plan_ivr,
k_ivr_pick_batch and the batched covariance-product kernels).

The reference is tests/_plan_ivr_batch.py on the oracle's dense covariance. Every member of
every batch passes _plan_ivr.check_run's two conditions at O.PARITY_TOL: for every pick t, with
ref_t the oracle's from-scratch scores given the device's picks before it,
    |gains[t] - ref_t[cell_t]| / max(|ref_t[cell_t]|, floor) <= PARITY_TOL
    ref_t[cell_t] >= max_allowed ref_t - PARITY_TOL max(max ref_t, floor).
Picks of two device runs are compared only on the fixtures whose oracle scores have no near
ties (tests/test_plan_ivr_batch_host.py asserts that); elsewhere up to the first pick the
oracle shows decided by rounding. A batch of one member is the single planner bit for bit:
mfgp_plan_ivr is the same loop entered with one member.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import _ivr as I
from tests import _plan_ivr as P
from tests import _plan_ivr_batch as Q

pytestmark = pytest.mark.gpu

TOL = O.PARITY_TOL
NPICK = Q.NPICK


def _build(ctx, member):
    from mfgp_coverage_amd import _lib
    kind, gname, N = member
    Xs, X, y, NL = Q.case_data(kind, gname, N)
    if N == 0:               # a model that never saw data: a grid, no factor
        m = _lib.Model(ctx, _lib.SF if kind == "sf" else _lib.MF, I.hyp_of(kind), 1e-8)
        m.set_grid(Xs)
        return m
    return I._model(ctx, kind, X, y, NL, Xs)


_MODELS = {}


def _model(member):
    """One model per member on the thread's context: built once, shared, never modified (the
    planner leaves its models as they were)."""
    if member not in _MODELS:
        from mfgp_coverage_amd import _lib
        _MODELS[member] = _build(_lib.context(), member)
    return _MODELS[member]


def _weights(members, wname):
    return None if wname == "ones" else [P.weights(wname, Q.case_data(*m)[0].shape[0]) for m in members]


def _cands(members, listed):
    if not listed:
        return None
    out = []
    for k, g, N in members:
        M = Q.case_data(k, g, N)[0].shape[0]
        out.append(np.random.default_rng(N + M).choice(M, 40, replace=False))
    return out


def _check_member(member, w, cand, run, n_points, group=None, quota=None, tag=""):
    """A member's run against the oracle: shapes, points, list membership and the two
    conditions -> the oracle's gaps per pick."""
    kind, gname, N = member
    Xs, X, y, NL = Q.case_data(kind, gname, N)
    hyp = I.hyp_of(kind)
    cells, pos, pts, gains = run
    assert cells.shape == pos.shape == gains.shape == (n_points,) and pts.shape == (n_points, 2), (member, cells.shape)
    assert np.array_equal(pts, Xs[cells])
    if cand is not None:
        assert set(cells.tolist()) <= set(np.asarray(cand).tolist())
    if group is None:
        eg, em, gaps = P.check_run(kind, X, y, NL, Xs, hyp, w, cells, gains, cand)
        lst = np.arange(Xs.shape[0]) if cand is None else np.asarray(cand)
        assert np.array_equal(cells, lst[pos])
    else:
        eg, em, gaps = Q.check_quota_run(kind, X, y, NL, Xs, hyp, w, cells, pos, gains, cand, group, quota)
    print(f"batch_plan_ivr {tag} {member}: gain error {eg:.3e}, shortfall {em:.3e}")
    assert eg <= TOL and em <= TOL, (member, eg, em)
    return gaps


def _gain_err(member, w, got, ref):
    kind, gname, N = member
    M = Q.case_data(kind, gname, N)[0].shape[0]
    fl = P.pick_floor(I.hyp_of(kind), w, M)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), fl))) if len(ref) else 0.0


def _same_up_to_ties(member, w, a, b, gaps, what):
    """The policy where no precondition was asserted: equal cells up to the first pick the
    oracle shows decided by rounding, gains within the tolerance up to there."""
    tie = np.nonzero(gaps <= 2 * TOL)[0]
    upto = int(tie[0]) if tie.size else len(gaps)
    assert np.array_equal(a[0][:upto], b[0][:upto]), (what, member, upto)
    assert _gain_err(member, w, a[3][:upto], b[3][:upto]) <= TOL, (what, member)


# ---- 1. the oracle, per member ---------------------------------------------------------------------

@pytest.mark.parametrize("nb", [1, 3, 8])
@pytest.mark.parametrize("wname", ["ones", "mask"])
@pytest.mark.parametrize("listed", [False, True], ids=["all", "list40"])
def test_every_member_against_the_oracle(nb, wname, listed):
    from mfgp_coverage_amd import _lib
    members = {1: Q.MEMBERS8[2:3], 3: Q.MEMBERS3, 8: Q.MEMBERS8}[nb]
    ws, cands = _weights(members, wname), _cands(members, listed)
    runs = _lib.batch_plan_ivr([_model(m) for m in members], NPICK, weights=ws, cand=cands)
    assert len(runs) == nb
    for b, member in enumerate(members):
        _check_member(member, None if ws is None else ws[b], None if cands is None else cands[b], runs[b], NPICK,
                      tag=f"B = {nb} {wname}")


# ---- 2. against the single call ----------------------------------------------------------------------

def _one_row_steps(ctx, members, batched):
    """A one-row append + predict of fresh models, batched or one by one -> [(mu, var)]."""
    import torch
    from mfgp_coverage_amd import _lib
    ms = [_build(ctx, m) for m in members]
    for m in ms:
        m.predict()
    rows = [Q.case_data(*m)[0][17:18] for m in members]
    Ms = [Q.case_data(*m)[0].shape[0] for m in members]
    groups = [list(range(len(ms)))] if batched else [[b] for b in range(len(ms))]
    out = [None] * len(ms)
    for grp in groups:
        xd = torch.from_numpy(np.vstack([rows[b] for b in grp])).cuda()
        yd = torch.full((len(grp),), 0.25, dtype=torch.float64, device="cuda")
        tot = sum(Ms[b] for b in grp)
        mu, var = (torch.empty(tot, dtype=torch.float64, device="cuda") for _ in range(2))
        _lib.batch_append_predict([ms[b] for b in grp], xd.data_ptr(), yd.data_ptr(), [1] * len(grp), mu.data_ptr(),
                                  var.data_ptr())
        mu, var, o = mu.cpu().numpy(), var.cpu().numpy(), 0
        for b in grp:
            out[b] = (mu[o:o + Ms[b]], var[o:o + Ms[b]])
            o += Ms[b]
    return out


@pytest.mark.parametrize("lattice", [0, "force"], ids=["vstream", "lattice"])
@pytest.mark.parametrize("members,wname", Q.EXACT, ids=["mask", "ones"])
def test_members_equal_the_single_planner(members, wname, lattice):
    """On the fixtures without near ties every member's cells are those of plan_ivr on the
    member alone and its gains agree within PARITY_TOL, with the step form pinned on both
    sides. Where a batched one-row append + predict gives the single step's bits in that
    form, cells and gains are equal bit for bit. Both entries run the same loop: this guards
    the single entry's argument mapping, and that a member's sums do not depend on the
    batch around it."""
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_lattice(lattice)
    try:
        ms = [_build(ctx, m) for m in members]
        ws = _weights(members, wname)
        runs = _lib.batch_plan_ivr(ms, NPICK, weights=ws)
        ps = ctx.planner_stats()
        assert (ps["lattice"] > 0) == (lattice == "force"), ps
        single = [m.plan_ivr(NPICK, weights=None if ws is None else ws[b]) for b, m in enumerate(ms)]
        sb, ss = _one_row_steps(ctx, members, True), _one_row_steps(ctx, members, False)
        step_bits = all(np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]) for u, v in zip(sb, ss))
        print(f"step form {lattice}: the batched one-row step {'has' if step_bits else 'has not'} the single step's bits")
        for b, member in enumerate(members):
            w = None if ws is None else ws[b]
            cells, pos, pts, gains = runs[b]
            assert np.array_equal(cells, single[b][0]), (member, cells, single[b][0])
            e = _gain_err(member, w, gains, single[b][2])
            print(f"batch against single {member} {wname}: {e:.3e}")
            assert e <= TOL
            if step_bits:
                assert np.array_equal(gains, single[b][2]) and np.array_equal(pts, single[b][1]), member
    finally:
        ctx.set_lattice(True)


def test_a_batch_of_one_is_the_single_planner_bit_for_bit():
    """mfgp_plan_ivr is the batch of one of the same loop, so this guards its argument mapping
    (count = 1, cand_off = {0, nc}, no groups, no positions) against the batched entry's:
    equal bits with all cells and with a list. Also group=None against the unconstrained run,
    and a quota that never binds."""
    from mfgp_coverage_amd import _lib
    for member in (Q.MEMBERS8[0], Q.MEMBERS8[6], Q.MEMBERS8[4]):
        m = _model(member)
        M = Q.case_data(*member)[0].shape[0]
        w = P.weights("mask", M)
        cand = np.random.default_rng(5).choice(M, 40, replace=False)
        for kw in ({}, {"cand": cand}):
            want = m.plan_ivr(NPICK, weights=w, **kw)
            (cells, pos, pts, gains), = _lib.batch_plan_ivr([m], NPICK, weights=w, **kw)
            assert np.array_equal(cells, want[0]) and np.array_equal(pts, want[1]) and np.array_equal(gains, want[2])
            nc = M if not kw else 40
            (c2, p2, t2, g2), = _lib.batch_plan_ivr([m], NPICK, weights=w, groups=np.zeros(nc, dtype=np.int64),
                                                    quota=[NPICK], **kw)
            assert np.array_equal(c2, cells) and np.array_equal(p2, pos) and np.array_equal(g2, gains)


def test_the_single_entry_with_a_repeated_cell_and_with_one_cell():
    """Through mfgp_plan_ivr, a list that names a cell twice and a list of one cell: what the
    batched entry returns for the same list (the numerators are scattered over the list
    alone, a repeated cell receiving the same bits twice), and the model's predict bits are
    those from before."""
    from mfgp_coverage_amd import _lib
    member = Q.MEMBERS8[0]                                     # 13 x 11, MF, N = 65
    m = _build(_lib.context(), member)
    w = P.weights("mask", 143)
    mu0, var0 = m.predict()
    for cand, n in (([71, 20, 71, 5], 6), ([71], 3)):
        cells, pts, gains = m.plan_ivr(n, weights=w, cand=cand)
        (bc, bp, bt, bg), = _lib.batch_plan_ivr([m], n, weights=w, cand=cand)
        assert cells.shape == (n,) and set(cells.tolist()) <= set(cand)
        assert np.array_equal(cells, bc) and np.array_equal(pts, bt) and np.array_equal(gains, bg)
        assert np.array_equal(cells, np.asarray(cand)[bp])
        _check_member(member, w, cand, (cells, bp, pts, gains), n, tag=f"single entry, list {cand}")
    mu1, var1 = m.predict()
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)


# ---- 3. groups ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("member", [("mf", "13x11", 65), ("sf", "13x11", 0)], ids=["mf65", "sf0"])
def test_groups_and_quotas(member):
    from mfgp_coverage_amd import _lib
    kind, gname, N = member
    Xs = Q.case_data(*member)[0]
    M = Xs.shape[0]
    quad = Q.quadrants(Xs)
    other = ("sf", "9x7", 197)                                 # a second member, unconstrained in effect
    m, mo = _model(member), _model(other)
    Mo = Q.case_data(*other)[0].shape[0]
    free = np.zeros(Mo, dtype=np.int64)
    for wname in ("ones", "mask"):
        w = P.weights(wname, M)
        ws = None if w is None else [w, np.ones(Mo)]
        # quota 1: exactly four picks, one per quadrant
        r, ro = _lib.batch_plan_ivr([m, mo], 10, weights=ws, groups=[quad, free], quota=[5, 1, 1, 1])
        assert ro[0].shape == (5,)
        r1, = _lib.batch_plan_ivr([m], 10, weights=w, groups=quad)
        assert r1[0].shape == (4,) and sorted(quad[r1[1]].tolist()) == [0, 1, 2, 3]
        _check_member(member, w, None, r1, 4, quad, None, tag="quota 1")
        # quotas [2, 1, 0, 3] and 10 points: six picks, none in group 2
        r2, = _lib.batch_plan_ivr([m], 10, weights=w, groups=quad, quota=[2, 1, 0, 3])
        assert r2[0].shape == (6,)
        assert np.bincount(quad[r2[1]], minlength=4).tolist() == [2, 1, 0, 3]
        _check_member(member, w, None, r2, 6, quad, [2, 1, 0, 3], tag="quota 2103")
        # beside another member (all its cells in group 0): the counters are per member
        assert r[0].shape == (8,) and np.bincount(quad[r[1]], minlength=4).tolist() == [5, 1, 1, 1]
        _check_member(member, w, None, r, 8, quad, [5, 1, 1, 1], tag="quota 5,1,1,1 in a batch of 2")
    # a cell listed twice under two groups is taken once for each, the first position first
    r3, = _lib.batch_plan_ivr([m], 10, cand=[71, 71], groups=[0, 1])
    assert r3[0].tolist() == [71, 71] and r3[1].tolist() == [0, 1] and r3[3][1] < r3[3][0]
    _check_member(member, None, [71, 71], r3, 2, [0, 1], None, tag="listed twice")
    twice = np.concatenate((np.arange(M), [71]))
    g2 = np.concatenate((quad, [(quad[71] + 1) % 4]))
    r4, = _lib.batch_plan_ivr([m], 10, cand=twice, groups=g2)
    assert r4[0].shape == (4,) and np.array_equal(r4[0], twice[r4[1]])
    _check_member(member, None, twice, r4, 4, g2, None, tag="listed twice among all")


# ---- 4. ragged stops -----------------------------------------------------------------------------------

def test_members_stop_at_their_own_crossings():
    from mfgp_coverage_amd import _lib
    ms = [_model(m) for m in Q.RAGGED]
    runs = _lib.batch_plan_ivr(ms, Q.RAGGED_PICKS, min_gain=Q.RAGGED_GAIN)
    assert tuple(r[0].shape[0] for r in runs) == Q.RAGGED_COUNTS, [r[3] for r in runs]
    assert runs[2][2].shape == (0, 2) and runs[2][1].shape == (0,)
    for member, r, n in zip(Q.RAGGED, runs, Q.RAGGED_COUNTS):
        if n:
            _check_member(member, None, None, r, n, tag="ragged")
            assert np.all(r[3] >= Q.RAGGED_GAIN)
    # the member that goes on longest is unaffected by those that stopped: a batch without them
    alone, = _lib.batch_plan_ivr(ms[:1], Q.RAGGED_PICKS, min_gain=Q.RAGGED_GAIN)
    assert np.array_equal(alone[0], runs[0][0])
    assert _gain_err(Q.RAGGED[0], None, runs[0][3], alone[3]) <= TOL
    # and in another order of the batch
    rev = _lib.batch_plan_ivr(ms[::-1], Q.RAGGED_PICKS, min_gain=Q.RAGGED_GAIN)
    assert tuple(r[0].shape[0] for r in rev) == Q.RAGGED_COUNTS[::-1]
    assert np.array_equal(rev[2][0], runs[0][0]) and np.array_equal(rev[1][0], runs[1][0])
    # a gain no member reaches: zero picks for all, and the models are usable
    none = _lib.batch_plan_ivr(ms, 5, min_gain=1e9)
    assert all(r[0].shape == (0,) for r in none)


# ---- 5. rows crossing 64 --------------------------------------------------------------------------------

def test_appended_rows_cross_row_64():
    from mfgp_coverage_amd import _lib
    members = (("mf", "13x11", 60), ("sf", "13x11", 60), ("sf", "9x7", 197))
    ms = [_model(m) for m in members]
    runs = _lib.batch_plan_ivr(ms, 8)
    for b, member in enumerate(members):
        _check_member(member, None, None, runs[b], 8, tag="rows 60..68")
    for b in (0, 1):                                           # (the fixtures of the CPU precondition)
        c, _, g = ms[b].plan_ivr(8)
        assert np.array_equal(runs[b][0], c) and _gain_err(members[b], None, runs[b][3], g) <= TOL


# ---- 6. refresh ------------------------------------------------------------------------------------------

def test_refresh():
    """refresh = 1 is the from-scratch route on the device; the recurrence (refresh = 0) and
    refresh = 7 return its cells (the fixtures have no near ties) and its gains within
    PARITY_TOL, the tolerance of tests/test_gpu_plan_ivr.py::test_refresh."""
    from mfgp_coverage_amd import _lib
    members = Q.MEMBERS3
    ms = [_model(m) for m in members]
    ws = _weights(members, "mask")
    n = 20
    # member 1 on a list of every second cell (the refresh scatters too), the others on all cells
    cl = [np.arange(0, Q.case_data(*m)[0].shape[0], 2 if b == 1 else 1) for b, m in enumerate(members)]
    r1 = _lib.batch_plan_ivr(ms, n, weights=ws, cand=cl, refresh=1)
    gaps = [_check_member(m, ws[b], cl[b], r1[b], n, tag="refresh 1") for b, m in enumerate(members)]
    for R in (0, 7):
        r = _lib.batch_plan_ivr(ms, n, weights=ws, cand=cl, refresh=R)
        for b, member in enumerate(members):
            _check_member(member, ws[b], cl[b], r[b], n, tag=f"refresh {R}")
            _same_up_to_ties(member, ws[b], r[b], r1[b], gaps[b], f"refresh {R}")
            if b != 1:                                         # all cells, mask weights: a fixture without near ties
                assert np.array_equal(r[b][0], r1[b][0]), (R, member)


# ---- 7. leaves no trace -----------------------------------------------------------------------------------

def test_the_batch_leaves_no_trace():
    import torch
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    members = Q.MEMBERS3
    a = [_build(ctx, m) for m in members]
    b = [_build(ctx, m) for m in members]                      # twins that never run the planner
    for m in a + b:
        m.predict()
    before = [m.predict() for m in a]
    st0, se0 = [m.stats() for m in a], [m.serial() for m in a]
    ws = _weights(members, "mask")
    r1 = _lib.batch_plan_ivr(a, NPICK, weights=ws)             # (the models' capacity grows once, here)
    assert [m.stats() for m in a] == st0
    live0 = _lib.live_allocations()
    ps0 = ctx.planner_stats()
    r2 = _lib.batch_plan_ivr(a, NPICK, weights=ws)             # a second call: the same bits
    assert _lib.live_allocations() == live0
    ps1 = ctx.planner_stats()
    assert ps1["runs"] == ps0["runs"] + 3 and ps1["inc_factor"] == ps0["inc_factor"] + 3 * NPICK
    assert [m.stats() for m in a] == st0
    assert all(m.serial() != s for m, s in zip(a, se0))        # moved, as after the single planner
    assert [m.n for m in a] == [mm[2] for mm in members]
    for m, (mu0, var0) in zip(a, before):
        mu1, var1 = m.predict()
        assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    for u, v in zip(r1, r2):
        assert all(np.array_equal(x, y) for x, y in zip(u, v))
    short = _lib.batch_plan_ivr(a, 3, weights=ws)              # a shorter run: the longer one's first picks
    assert all(np.array_equal(x, y[:3]) for x, y in zip(short[0], r1[0]))
    # the next batched step: the bits of the twins
    Ms = [Q.case_data(*m)[0].shape[0] for m in members]
    rows = np.vstack([Q.case_data(*m)[0][23:24] for m in members])
    outs = []
    for ms in (a, b):
        xd = torch.from_numpy(rows).cuda()
        yd = torch.full((3,), 0.5, dtype=torch.float64, device="cuda")
        mu, var = (torch.empty(sum(Ms), dtype=torch.float64, device="cuda") for _ in range(2))
        _lib.batch_append_predict(ms, xd.data_ptr(), yd.data_ptr(), [1, 1, 1], mu.data_ptr(), var.data_ptr())
        outs.append((mu.cpu().numpy(), var.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- 8. errors ----------------------------------------------------------------------------------------------

def test_errors_launch_nothing_and_leave_the_models_usable():
    from mfgp_coverage_amd import _lib
    ctx = _lib.Context(0)
    members = (("mf", "13x11", 65), ("sf", "9x7", 197))
    ms = [_build(ctx, m) for m in members]
    M0, M1 = 143, 63
    quad = Q.quadrants(Q.case_data(*members[0])[0])
    w = [P.weights("mask", M0), P.weights("mask", M1)]
    groups = [quad, np.zeros(M1, dtype=np.int64)]
    good = _lib.batch_plan_ivr(ms, 6, weights=w, groups=groups, quota=[2, 1, 1, 1])
    st, se, ps = [m.stats() for m in ms], [m.serial() for m in ms], ctx.planner_stats()
    L = _lib.lib()
    P4 = 4
    cells, pos = np.zeros((2, P4), dtype=np.int64), np.zeros((2, P4), dtype=np.int64)
    pts, gains, cnt = np.zeros((2, P4, 2)), np.zeros((2, P4)), np.zeros(2, dtype=np.int64)
    wbuf = np.ones((2, M0))

    def vp(a):
        return None if a is None else ctypes.c_void_p(np.ascontiguousarray(a).ctypes.data)

    def raw(models=ms, count=2, wa=None, ldw=M0, cand=None, off=None, group=None, quota=None, ngroups=0, n=P4,
            refresh=0, out=(cells, pos, pts, gains, cnt)):
        keep = [None if v is None else np.ascontiguousarray(v) for v in (wa, cand, off, group, quota)]
        return L.mfgp_batch_plan_ivr(_lib._handles(models), count, vp(keep[0]), ldw, vp(keep[1]), vp(keep[2]),
                                     vp(keep[3]), vp(keep[4]), ngroups, n, 0.0, refresh, *[vp(o) for o in out])

    def i64(v):
        return np.asarray(v, dtype=np.int64)

    g32 = np.zeros(M0 + M1, dtype=np.int32)
    cases = [
        ("count", dict(count=0)),
        ("null output", dict(out=(None, pos, pts, gains, cnt))),
        ("null output", dict(out=(cells, pos, None, gains, cnt))),
        ("null output", dict(out=(cells, pos, pts, None, cnt))),
        ("counts", dict(out=(cells, pos, pts, gains, None))),
        ("n_points", dict(n=-1)),
        ("refresh", dict(refresh=-1)),
        ("ldw", dict(wa=wbuf, ldw=M0 - 1)),
        ("outside the grid", dict(cand=i64([0, 1, M1]), off=i64([0, 1, 3]))),
        ("outside the grid", dict(cand=i64([-1, 1]), off=i64([0, 1, 2]))),
        ("cand_off", dict(cand=i64([0, 1, 2]), off=i64([1, 2, 3]))),
        ("cand_off", dict(cand=i64([0, 1, 2]), off=i64([0, 2, 1]))),
        ("cand_off", dict(cand=i64([0, 1, 2]))),
        ("group", dict(group=np.where(np.arange(M0 + M1) == 150, 4, g32).astype(np.int32), ngroups=4)),
        ("group", dict(group=np.where(np.arange(M0 + M1) == 3, -1, g32).astype(np.int32), ngroups=4)),
        ("ngroups", dict(group=g32, ngroups=0)),
        ("ngroups", dict(group=g32, ngroups=65)),
        ("quota", dict(group=g32, ngroups=2, quota=i64([1, -1]))),
        ("quota", dict(quota=i64([1, 1]), ngroups=2)),
        ("twice", dict(models=[ms[0], ms[0]])),
    ]
    for text, kw in cases:
        with pytest.raises(ValueError, match=text):
            _lib.check(raw(**kw))
    for bad in (np.nan, np.inf):
        wb = [w[0].copy(), w[1].copy()]
        wb[1][M1 - 1] = bad
        with pytest.raises(ValueError, match="finite"):
            _lib.batch_plan_ivr(ms, 3, weights=wb)
    with pytest.raises(ValueError, match="ldw"):
        _lib.batch_plan_ivr(ms, 3, weights=[np.ones(M0 - 1), np.ones(M1)])
    with pytest.raises(ValueError, match="groups"):
        _lib.batch_plan_ivr(ms, 3, groups=[quad[:-1], groups[1]])
    Xs1, X1, y1, _ = Q.case_data(*members[1])
    f32 = I._model(ctx, "sf", X1, y1, 0, Xs1, dtype=_lib.F32)
    with pytest.raises(ValueError, match="MFGP_F32"):
        _lib.batch_plan_ivr([ms[0], f32], 3)
    bare = _lib.Model(ctx, _lib.SF, I.HYP_SF, 1e-8)
    with pytest.raises(ValueError, match="no grid"):
        _lib.batch_plan_ivr([ms[0], bare], 3)
    foreign = _build(_lib.Context(0), members[1])
    with pytest.raises(ValueError, match="context"):
        _lib.batch_plan_ivr([ms[0], foreign], 3)
    ctx.set_incremental(False)
    with pytest.raises(ValueError, match="incremental"):
        _lib.batch_plan_ivr(ms, 3)
    ctx.set_incremental(True)
    # nothing ran: the models, their serials and the planners' counters are as they were
    assert [m.stats() for m in ms] == st and [m.serial() for m in ms] == se and ctx.planner_stats() == ps
    zero = _lib.batch_plan_ivr(ms, 0)
    assert all(r[0].shape == (0,) and r[2].shape == (0, 2) for r in zero)
    empty = _lib.batch_plan_ivr(ms, 3, cand=[[], [5]])          # an empty list: no picks for that member
    assert empty[0][0].shape == (0,) and empty[1][0].tolist() == [5, 5, 5]
    assert [m.stats() for m in ms] == st
    again = _lib.batch_plan_ivr(ms, 6, weights=w, groups=groups, quota=[2, 1, 1, 1])
    for u, v in zip(good, again):
        assert all(np.array_equal(x, y) for x, y in zip(u, v))
    assert ps["runs"] + 4 == ctx.planner_stats()["runs"]        # (the `empty` call's two runs and these two)


# ---- 9. the drop-in classes ------------------------------------------------------------------------------------

def test_dropin_batch_planner():
    from mfgp_coverage_amd.gaussian_process import MFGP, SFGP
    from mfgp_coverage_amd.planners import compute_sample_points_ivr, compute_sample_points_ivr_batch
    Xs = I.grid("13x11")
    M = Xs.shape[0]
    quad = Q.quadrants(Xs)
    gps, data = [], []
    for kind, seed in (("sf", 95), ("mf", 96), ("sf", 97)):
        hyp = I.hyp_of(kind)
        X, y = I._distinct(Xs, 90, seed=seed)
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
        gps.append(gp)
        data.append((kind, X, y, NL, hyp))
    w = I.weight_sets(M, seed=98)["mask"]
    cand = np.arange(20, 120)
    before = [gp.predict(Xs) for gp in gps]
    out = compute_sample_points_ivr_batch(gps, Xs, 10, weights=w, candidates=cand, groups=quad[cand], quota=[3, 3, 3, 3])
    assert len(out) == 3
    for (pts, gains, picked), (kind, X, y, NL, hyp), gp in zip(out, data, gps):
        assert pts.shape == (10, 2) and gains.shape == (10,) and picked.shape == (10,)
        cells = np.array([int(np.nonzero((Xs == p).all(1))[0][0]) for p in pts])
        assert np.array_equal(picked, quad[cells]) and np.bincount(picked, minlength=4).max() <= 3
        pos = np.array([int(np.nonzero(cand == c)[0][0]) for c in cells])
        eg, em, _ = Q.check_quota_run(kind, X, y, NL, Xs, hyp, w, cells, pos, gains, cand, quad[cand], [3, 3, 3, 3])
        assert eg <= TOL and em <= TOL
    for gp, (mu0, cov0) in zip(gps, before):                   # the models are unchanged
        mu1, cov1 = gp.predict(Xs)
        assert np.array_equal(mu0, mu1) and np.array_equal(np.diag(cov0), np.diag(cov1))
    free = compute_sample_points_ivr_batch(gps[:1], Xs, 5, weights=w)
    one = compute_sample_points_ivr(gps[0], Xs, 5, weights=w)
    assert free[0][2] is None and np.array_equal(free[0][0], one[0]) and np.array_equal(free[0][1], one[1])
    assert compute_sample_points_ivr_batch([], Xs, 5) == []
    with pytest.raises(TypeError):
        compute_sample_points_ivr_batch([gps[0], object()], Xs, 3)
    kind, X, y, NL, hyp = data[0]
    f32 = SFGP(X, y.reshape(-1, 1), 1)
    f32.precision = "f32"
    f32.hyp = hyp.copy()
    f32.updt_info(f32.X, f32.y)
    with pytest.raises(TypeError):
        compute_sample_points_ivr_batch([gps[0], f32], Xs, 3)
