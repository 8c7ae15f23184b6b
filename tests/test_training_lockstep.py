"""training.lockstep_minimize on the host: the NumPy oracle's NLML and gradient
(oracle.gp_oracle.nlml) as the batched objective, on a 70-row MF workload. Every start
is its solo L-BFGS-B run bit for bit, the objective runs on the calling thread only,
once per round, and a start that is answered with LinAlgError ends alone.
"""
import threading

import numpy as np
import pytest
from scipy.optimize import minimize

from mfgp_coverage_amd import synthetic, training
from oracle import gp_oracle as O

OPTIONS = {"maxiter": 12}


@pytest.fixture(scope="module")
def problem():
    wl = synthetic.Workload(16, 30, 40, 1, 1, seed=70)
    h0 = synthetic.HYP["australia9_mf"]
    rng = np.random.default_rng(70)
    starts = np.vstack([h0] + [h0 + 0.3 * rng.standard_normal(9) for _ in range(4)])

    def fun(x):
        return O.nlml(wl.XH, wl.yH, x, XL=wl.XL, yL=wl.yL, grad=True)

    solo, seen = [], []
    for x0 in starts:
        xs = []

        def traced(x, xs=xs):
            xs.append(np.array(x))
            return fun(x)

        solo.append(minimize(traced, x0, jac=True, method="L-BFGS-B", options=OPTIONS))
        seen.append(xs)
    return fun, starts, solo, seen


class _Batch:
    """batch_fun over `fun` that records its calls; points in `poison` (by their bytes)
    are answered with LinAlgError."""

    def __init__(self, fun, poison=()):
        self.fun = fun
        self.poison = {np.asarray(p, dtype=np.float64).tobytes() for p in poison}
        self.sizes = []
        self.threads = set()

    def __call__(self, xs):
        self.sizes.append(len(xs))
        self.threads.add(threading.get_ident())
        return [np.linalg.LinAlgError("Matrix is not positive definite") if x.tobytes() in self.poison else self.fun(x)
                for x in xs]


def _no_workers_left():
    return not [t for t in threading.enumerate() if t.name.startswith("lockstep-")]


def _same_run(r, s):
    return (r.x.tobytes() == s.x.tobytes() and np.float64(r.fun).tobytes() == np.float64(s.fun).tobytes()
            and r.nfev == s.nfev and r.nit == s.nit)


def test_every_start_is_its_solo_run(problem):
    fun, starts, solo, _ = problem
    bf = _Batch(fun)
    res = training.lockstep_minimize(bf, starts, options=OPTIONS)
    assert len(res) == len(starts)
    for r, s in zip(res, solo):
        assert _same_run(r, s), (r, s)
    nfev = sorted(s.nfev for s in solo)
    assert len(set(nfev)) > 1, nfev                      # (the starts do not all end together)
    assert len(bf.sizes) == nfev[-1]                     # one call per round, as many rounds as the longest run
    # round r serves the starts with at least r evaluations: the batch shrinks as starts finish
    assert bf.sizes == [sum(n >= r for n in nfev) for r in range(1, nfev[-1] + 1)]
    assert bf.sizes[0] == len(starts) and bf.sizes[-1] < len(starts)
    assert bf.threads == {threading.get_ident()}         # the objective ran on the calling thread only
    assert _no_workers_left()


def test_a_failed_start_ends_alone(problem):
    fun, starts, solo, seen = problem
    k = 2
    assert len(seen[k]) >= 3
    bf = _Batch(fun, poison=[seen[k][2]])                # start k's third evaluation is not positive definite
    res = training.lockstep_minimize(bf, starts, options=OPTIONS)
    assert isinstance(res[k], np.linalg.LinAlgError)
    for i, (r, s) in enumerate(zip(res, solo)):
        if i != k:
            assert _same_run(r, s), i
    others = [s.nfev for i, s in enumerate(solo) if i != k]
    assert len(bf.sizes) == max(max(others), 3)
    assert bf.sizes[2] == len(starts) and bf.sizes[3] == sum(n >= 4 for n in others)
    assert bf.threads == {threading.get_ident()}
    assert _no_workers_left()


def test_all_starts_fail(problem):
    fun, starts, _, _ = problem
    bf = _Batch(fun, poison=list(starts))                # every first evaluation fails
    res = training.lockstep_minimize(bf, starts, options=OPTIONS)
    assert len(res) == len(starts) and all(isinstance(r, np.linalg.LinAlgError) for r in res)
    assert bf.sizes == [len(starts)]
    assert _no_workers_left()


def test_an_objective_that_raises_ends_every_start(problem):
    fun, starts, _, _ = problem

    def broken(xs):
        raise RuntimeError("device lost")

    with pytest.raises(RuntimeError, match="device lost"):
        training.lockstep_minimize(broken, starts, options=OPTIONS)
    assert _no_workers_left()


def test_no_starts():
    assert training.lockstep_minimize(lambda xs: [], np.empty((0, 9))) == []
