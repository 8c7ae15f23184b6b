"""Multi-start training in lockstep on a batched objective.

``lockstep_minimize`` runs one ``scipy.optimize.minimize(..., jac=True,
method="L-BFGS-B")`` per start, each in a thread of its own, and serves their
objective evaluations together: every minimiser parks its request, the calling
thread collects one request from every minimiser that is still running, evaluates
them in one call of ``batch_fun`` (``Model.nlml_batch``: one set of launches for all
of them) and hands the answers back. A minimiser sees exactly the values a solo run
from its start would see, so its iterates, ``x``, ``fun`` and ``nfev`` are those of the
solo run bit for bit, and the number of ``batch_fun`` calls is the largest ``nfev``.

Only the calling thread calls ``batch_fun``: the device context is per host thread
(``_lib.context()``), a worker thread never touches the device.
"""
from __future__ import annotations

import queue
import threading

import numpy as np


class _Start:
    """One minimiser: its thread, the slot its answers arrive in and its result."""

    def __init__(self, index, x0, requests, options):
        self.index = index
        self.x0 = np.array(x0, dtype=np.float64).reshape(-1)
        self.requests = requests            # shared: ("eval", index, x) / ("done", index, None)
        self.answers = queue.Queue(1)       # (value, grad) or an exception instance
        self.options = options
        self.result = None
        self.thread = threading.Thread(target=self._run, name=f"lockstep-{index}", daemon=True)

    def _fun(self, x):
        self.requests.put(("eval", self.index, np.array(x, dtype=np.float64)))
        ans = self.answers.get()
        if isinstance(ans, BaseException):
            raise ans
        return ans

    def _run(self):
        from scipy.optimize import minimize
        try:
            self.result = minimize(self._fun, self.x0, jac=True, method="L-BFGS-B", **self.options)
        except BaseException as e:   # the start ends as failed; the others go on
            self.result = e
        finally:
            self.requests.put(("done", self.index, None))


def lockstep_minimize(batch_fun, starts, **lbfgsb_options):
    """Minimise from every row of ``starts`` [S, n] with L-BFGS-B, in lockstep.

    batch_fun(list_of_x) -> one ``(value, grad)`` or one exception instance (a
    ``numpy.linalg.LinAlgError`` for a point that is not positive definite) per entry,
    in order. It is called by the calling thread only, once per round, with the
    pending request of every start that is still running (in start order), so the
    batch shrinks as starts finish. ``lbfgsb_options`` go to ``minimize`` (``bounds``,
    ``tol``, ``options``...).

    Returns the per-start results in start order: the ``OptimizeResult``, or the
    exception that ended the start (the one ``batch_fun`` answered it with). If
    ``batch_fun`` itself raises, every start is ended and the exception propagates.
    No worker thread is left alive on return.
    """
    starts = [np.array(x0, dtype=np.float64).reshape(-1) for x0 in starts]
    requests = queue.Queue()
    runs = [_Start(i, x0, requests, lbfgsb_options) for i, x0 in enumerate(starts)]
    for r in runs:
        r.thread.start()
    live = len(runs)
    failure = None
    while live:
        pending = {}
        for _ in range(live):            # every live start posts exactly one message per round
            what, i, x = requests.get()
            if what == "eval":
                pending[i] = x
        live = len(pending)
        if not pending:
            break
        order = sorted(pending)
        try:
            if failure is not None:
                raise failure
            answers = list(batch_fun([pending[i] for i in order]))
            if len(answers) != len(order):
                raise ValueError(f"batch_fun returned {len(answers)} answers for {len(order)} points")
        except BaseException as e:       # end every start, then report it
            failure = e
            answers = [e] * len(order)
        for i, a in zip(order, answers):
            runs[i].answers.put(a)
    for r in runs:
        r.thread.join()
    if failure is not None:
        raise failure
    return [r.result for r in runs]
