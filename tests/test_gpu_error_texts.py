"""The error texts of the consumers of the resident V -- cov_block, var_reduction, cov_apply,
plan_ivr, sample, sample_dims -- whole, as include/mfgp_hip.h's callers see them in
mfgp_last_error(): _lib.check dispatches on message text and callers match substrings, so
prefix, wording, the numbers printed and the order in which the checks fail are part of
the ABI. One SF model on the 13 x 11 lattice (M = 143) with N = 70, its MFGP_F32 twin and a
model without a grid; every expected string is written out."""
import ctypes

import numpy as np
import pytest

from tests import _ivr as I

pytestmark = pytest.mark.gpu

M = 143
F32_TEXT = "%s: MFGP_F32 models (fp32 V) are not supported; use an MFGP_F64 model"
NO_GRID_TEXT = "%s: the model has no grid (mfgp_set_grid)"
CONSUMERS = ("mfgp_cov_block", "mfgp_var_reduction", "mfgp_cov_apply", "mfgp_plan_ivr", "mfgp_sample_posterior",
             "mfgp_sample_dims")


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def i64(v):
    return None if v is None else np.asarray(v, dtype=np.int64)


class Models:
    def __init__(self):
        from mfgp_coverage_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        Xs = I.grid("13x11")
        assert Xs.shape[0] == M
        X, y = I._distinct(Xs, 70, seed=91)
        # the thread's context, which outlives every model: text() leaves tracebacks that hold
        # this object in reference cycles, and the collector that frees those finalises in no
        # order -- a context of this object's own could be destroyed before its models
        self.ctx = _lib.context()
        self.m = I._model(self.ctx, "sf", X, y, 0, Xs)
        self.f32 = I._model(self.ctx, "sf", X, y, 0, Xs, dtype=_lib.F32)
        self.bare = _lib.Model(self.ctx, _lib.SF, I.HYP_SF, 1e-8)
        self.buf = np.ones((9, M))
        self.out = np.zeros((9, M))
        self.cells, self.pts, self.gains = np.zeros(4, dtype=np.int64), np.zeros((4, 2)), np.zeros(4)

    def text(self, rc):
        """The whole message of a failed call."""
        with pytest.raises(ValueError) as e:
            self.lib.check(rc)
        return str(e.value)

    # the raw entry points, on model `m`
    def cov_block(self, m, rows, na, cols, nb, ldo=M):
        return self.L.mfgp_cov_block(m.handle, vp(i64(rows)), na, vp(i64(cols)), nb, vp(self.out), ldo, 0)

    def var_reduction(self, m, cand, nc, w=None, nw=1, ldw=M, ldo=M):
        return self.L.mfgp_var_reduction(m.handle, vp(i64(cand)), nc, vp(w), nw, ldw, vp(self.out), ldo, None, None)

    def cov_apply(self, m, x=None, nx=1, ldx=M, ldo=M):
        return self.L.mfgp_cov_apply(m.handle, vp(self.buf if x is None else x), nx, ldx, vp(self.out), ldo, 0)

    def plan_ivr(self, m, cand=None, nc=M, w=None, ldw=M):
        n = ctypes.c_int64(0)
        return self.L.mfgp_plan_ivr(m.handle, vp(w), ldw, vp(i64(cand)), nc, 4, 0.0, 0, vp(self.cells), vp(self.pts),
                                    vp(self.gains), ctypes.byref(n))

    def sample(self, m, z=None, S=1, ldz=M + 100, ldo=M):
        return self.L.mfgp_sample_posterior(m.handle, vp(self.buf if z is None else z), S, ldz, vp(self.out), ldo, 0)

    def sample_dims(self, m):
        d = (ctypes.c_int64 * 8)()
        return self.L.mfgp_sample_dims(m.handle, d, 8, 0)

    def every(self, m):
        """One otherwise valid raw call of each consumer on m, in CONSUMERS' order (to be made
        one at a time: the message is the last call's)."""
        return (lambda: self.cov_block(m, [0], 1, [0], 1), lambda: self.var_reduction(m, [0], 1),
                lambda: self.cov_apply(m), lambda: self.plan_ivr(m), lambda: self.sample(m),
                lambda: self.sample_dims(m))


@pytest.fixture(scope="module")
def ms():
    return Models()


def test_f32_refusal(ms):
    for who, call in zip(CONSUMERS, ms.every(ms.f32)):
        assert ms.text(call()) == F32_TEXT % who
    # ... and through the Python layer
    for who, call in (("mfgp_cov_block", lambda: ms.f32.cov_block([0], [0])),
                      ("mfgp_var_reduction", lambda: ms.f32.var_reduction([0])),
                      ("mfgp_cov_apply", lambda: ms.f32.cov_apply(np.ones(M))),
                      ("mfgp_plan_ivr", lambda: ms.f32.plan_ivr(3)),
                      ("mfgp_sample_posterior", lambda: ms.f32.sample(np.zeros((1, 4)))),
                      ("mfgp_sample_dims", lambda: ms.f32.sample_dims())):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == F32_TEXT % who


def test_no_grid_refusal(ms):
    g = ms.bare
    calls = (lambda: ms.cov_block(g, [], 0, [], 0), lambda: ms.var_reduction(g, [], 0),
             lambda: ms.cov_apply(g, ldx=1, ldo=1), lambda: ms.plan_ivr(g, None, 0), lambda: ms.sample(g),
             lambda: ms.sample_dims(g))
    for who, call in zip(CONSUMERS, calls):
        assert ms.text(call()) == NO_GRID_TEXT % who
    for who, call in (("mfgp_cov_block", lambda: g.cov_block([], [])),
                      ("mfgp_var_reduction", lambda: g.var_reduction([])),
                      ("mfgp_plan_ivr", lambda: g.plan_ivr(3)),
                      ("mfgp_sample_posterior", lambda: g.sample(np.zeros((1, 4)))),
                      ("mfgp_sample_dims", lambda: g.sample_dims())):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == NO_GRID_TEXT % who


@pytest.mark.parametrize("bad", [-1, M])
@pytest.mark.parametrize("pos", [0, 2])
def test_index_out_of_range(ms, bad, pos):
    lst = [5, 6, 7]
    lst[pos] = bad
    tail = "[%d] = %d is outside the grid's cells [0, 143)" % (pos, bad)
    m = ms.m
    assert ms.text(ms.cov_block(m, lst, 3, [0], 1)) == "mfgp_cov_block: rows" + tail
    assert ms.text(ms.cov_block(m, [0], 1, lst, 3)) == "mfgp_cov_block: cols" + tail
    assert ms.text(ms.cov_block(m, None, M, lst, 3)) == "mfgp_cov_block: cols" + tail
    assert ms.text(ms.var_reduction(m, lst, 3)) == "mfgp_var_reduction: cand" + tail
    assert ms.text(ms.plan_ivr(m, lst, 3)) == "mfgp_plan_ivr: cand" + tail
    for who, call in (("mfgp_cov_block: rows", lambda: m.cov_block(lst, [0])),
                      ("mfgp_var_reduction: cand", lambda: m.var_reduction(lst)),
                      ("mfgp_plan_ivr: cand", lambda: m.plan_ivr(2, cand=lst))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == who + tail


def test_both_lists_bad_reports_rows_first(ms):
    assert ms.text(ms.cov_block(ms.m, [0, 1, 200], 3, [-4], 1)) == \
        "mfgp_cov_block: rows[2] = 200 is outside the grid's cells [0, 143)"


def test_null_list_with_a_wrong_count(ms):
    m = ms.m
    assert ms.text(ms.cov_block(m, None, 3, None, M)) == \
        "mfgp_cov_block: a NULL index list means all 143 cells (got na = 3, nb = 143)"
    assert ms.text(ms.cov_block(m, [1], 1, None, 7)) == \
        "mfgp_cov_block: a NULL index list means all 143 cells (got na = 1, nb = 7)"
    assert ms.text(ms.var_reduction(m, None, 3)) == \
        "mfgp_var_reduction: a NULL candidate list means all 143 cells (got nc = 3)"
    assert ms.text(ms.plan_ivr(m, None, 144)) == \
        "mfgp_plan_ivr: a NULL candidate list means all 143 cells (got nc = 144)"


def test_leading_dimension_one_short(ms):
    m = ms.m
    assert ms.text(ms.var_reduction(m, [0], 1, ms.buf, 2, ldw=M - 1)) == \
        "mfgp_var_reduction: ldw = 142 is less than M = 143"
    assert ms.text(ms.var_reduction(m, [0, 1, 2], 3, ms.buf, 2, ldo=2)) == \
        "mfgp_var_reduction: ldo = 2 is less than nc = 3"
    assert ms.text(ms.cov_apply(m, nx=2, ldx=M - 1)) == "mfgp_cov_apply: ldx = 142 is less than M = 143"
    assert ms.text(ms.cov_apply(m, nx=2, ldo=M - 1)) == "mfgp_cov_apply: ldo = 142 is less than M = 143"
    assert ms.text(ms.cov_block(m, [0, 1], 2, [0, 1, 2], 3, ldo=2)) == "mfgp_cov_block: ldo = 2 is less than nb = 3"
    assert ms.text(ms.plan_ivr(m, w=ms.buf, ldw=M - 1)) == "mfgp_plan_ivr: ldw = 142 is less than M = 143"
    assert ms.text(ms.sample(m, ldo=M - 1)) == "mfgp_sample_posterior: ldo = 142 is less than M = 143"
    nz = m.sample_dims()["nz"]
    assert ms.text(ms.sample(m, ldz=nz - 1)) == \
        "mfgp_sample_posterior: ldz = %d is less than nz = %d" % (nz - 1, nz)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_inputs(ms, bad):
    m = ms.m
    w = np.ones((3, M))
    w[1, M - 1] = bad                                     # vector / column 1, its last entry
    assert ms.text(ms.var_reduction(m, [0], 1, w, 3)) == "mfgp_var_reduction: the weights must be finite (vector 1)"
    assert ms.text(ms.cov_apply(m, w, 3)) == "mfgp_cov_apply: the vectors must be finite (column 1)"
    assert ms.text(ms.plan_ivr(m, w=w[1])) == "mfgp_plan_ivr: the weights must be finite"
    w[0, 0] = bad                                         # the first offender is reported
    assert ms.text(ms.var_reduction(m, [0], 1, w, 3)) == "mfgp_var_reduction: the weights must be finite (vector 0)"
    assert ms.text(ms.cov_apply(m, w, 3)) == "mfgp_cov_apply: the vectors must be finite (column 0)"
    with pytest.raises(ValueError) as e:
        m.var_reduction([0], w[1:])
    assert str(e.value) == "mfgp_var_reduction: the weights must be finite (vector 0)"
    nz = m.sample_dims()["nz"]
    z = np.zeros((3, nz))
    z[2, nz - 1] = bad
    assert ms.text(ms.sample(m, z, 3, ldz=nz)) == "mfgp_sample_posterior: the normals must be finite"
    # past the columns that count, a non-finite entry is not read
    pad = np.ones((2, M + 1))
    pad[:, M] = bad
    assert ms.var_reduction(m, [0], 1, pad, 2, ldw=M + 1) == 0
    assert ms.cov_apply(m, pad, 2, ldx=M + 1) == 0


def test_two_faults_at_once_report_the_model_first(ms):
    f = ms.f32
    assert ms.text(ms.cov_block(f, [-1], 1, [0], 1)) == F32_TEXT % "mfgp_cov_block"
    assert ms.text(ms.var_reduction(f, [M], 1)) == F32_TEXT % "mfgp_var_reduction"
    assert ms.text(ms.plan_ivr(f, [0, 1, -1], 3)) == F32_TEXT % "mfgp_plan_ivr"
    assert ms.text(ms.cov_apply(f, nx=2, ldx=M - 1)) == F32_TEXT % "mfgp_cov_apply"
    # and within one model: the order of the argument checks
    m = ms.m
    assert ms.text(ms.var_reduction(m, [M], 1, ms.buf, 2, ldw=M - 1)) == \
        "mfgp_var_reduction: ldw = 142 is less than M = 143"                      # ldw before the entries
    assert ms.text(ms.var_reduction(m, None, 3, ms.buf, 2, ldw=M - 1)) == \
        "mfgp_var_reduction: a NULL candidate list means all 143 cells (got nc = 3)"   # the count before ldw
    assert ms.text(ms.plan_ivr(m, [M], 1, w=ms.buf, ldw=M - 1)) == "mfgp_plan_ivr: ldw = 142 is less than M = 143"
    bad = np.ones(M)
    bad[3] = np.nan
    assert ms.text(ms.plan_ivr(m, [M], 1, w=bad)) == "mfgp_plan_ivr: cand[0] = 143 is outside the grid's cells [0, 143)"
    assert ms.text(ms.cov_block(m, [M], 1, [0, 1, 2], 3, ldo=2)) == "mfgp_cov_block: ldo = 2 is less than nb = 3"


def test_the_model_is_as_before(ms):
    """After all of the above (this module's last test): the failed calls changed nothing."""
    m = ms.m
    fresh = Models().m
    for a, b in zip(m.predict(), fresh.predict()):
        assert np.array_equal(a, b)
    assert np.array_equal(m.cov_apply(np.ones(M)), fresh.cov_apply(np.ones(M)))
    for a, b in zip(m.plan_ivr(3), fresh.plan_ivr(3)):
        assert np.array_equal(a, b)
    ms.ctx.synchronize()
