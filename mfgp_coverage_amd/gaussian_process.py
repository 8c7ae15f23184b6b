"""Drop-in SFGP / MFGP with the reference's Python surface, computed on MI355X.

Mirrors ``gaussian_process.py`` of MSU-dcypherlab/mfgp-coverage (imported by the
simulator at simulator.py:25): same class names, constructor signatures,
writable ``.hyp`` / ``.jitter``, the ``X, y`` / ``X_L, y_L, X_H, y_H`` attributes,
``updt_info`` / ``updt`` / ``updt_hifi`` / ``predict``, ``copy.deepcopy`` and
``isinstance`` (simulator.py:339, 361-366). The training set, the Cholesky
factor and the grid live on the GPU (libmfgp_hip.so); numpy arrays are kept on
the host only as the readable mirror the callers use.

Differences from the reference, all on the output side of the contract:

* ``predict`` returns ``(mu [M,1] ndarray, DiagCov)``. ``DiagCov`` carries the
  diagonal of the posterior covariance -- the only part any caller reads
  (``np.diag`` at simulator.py:301, 341, 685, 855; ``np.amax`` at 672, 842,
  1014; plotter.py:160). ``np.diag``/``np.amax``/``np.argmax`` of it give what
  they give on the dense matrix (for a PSD covariance the maximum entry lies on
  the diagonal). The off-diagonal entries are computed on demand from the V the
  device keeps (k_cov_block): ``cov[i, j]``, slices and ``cov.block(rows, cols)``
  take one block without forming M x M; ``np.asarray(cov)``, ``np.linalg.*`` and
  arithmetic materialise the dense matrix once (up to ``DiagCov.DENSE_MAX_BYTES``).
  A covariance whose model has since been updated raises RuntimeError off the
  diagonal. ``precision = "f32"`` models keep the diagonal only.
* The factorisation is the GPU's; results agree with the reference to the
  tolerance in oracle/gp_oracle.py (mu rel 1e-6, var rel 1e-6 floored at
  1e-6 * k**).
* ``likelihood``/``train`` (gp:81-119, 344-399) run on the GPU with an analytic
  gradient in place of autograd (``likelihood_and_grad``).
  ``likelihood_batch`` / ``likelihood_and_grad_batch`` evaluate many hyperparameter
  vectors in one set of launches, and ``train(n_restarts=..)`` / ``train(starts=..)``
  runs L-BFGS-B from several starts in lockstep on them (no callback prints then);
  ``train()`` alone is the reference's.
* ``draw_prior_samples`` / ``draw_posterior_samples`` (gp:180-217) draw from the
  device's covariance; the posterior draws are of ``predict``'s posterior (the
  reference's omit the prior mean and do not centre y).
* ``predict_at`` (new), ``MFGP.pred_var`` / ``pred_var_diag`` / ``get_neg_var`` /
  ``get_max_var`` (gp:440-481, 544-578) and ``SFGP.ExpectedImprovement``
  (gp:150-178) evaluate the posterior at arbitrary points, with prospective points
  that are not in the model, from the resident factor (k_look_border /
  k_look_query): the grid, the resident V and the posterior stay as they are.
  ``ExpectedImprovement`` uses ``predict``'s posterior (the reference's mean there
  has no prior mean and uncentred y), and ``get_max_var``'s differential evolution
  updates per generation, one launch each.
"""
from __future__ import annotations

import copy

import numpy as np

from . import _lib


class DiagCov:
    """The posterior covariance of gp:146 / gp:435-436: its diagonal held, the rest on demand.

    var: the diagonal, as the predict computed it. fused: (max, first argmax) of
    ``var`` as the launch that computed it reduced them (the eager append's epilogue,
    mfgp_view_max), or None: then ``np.amax`` / ``np.argmax`` return it instead of
    rescanning the M-vector on the host. The maximum of a vector is exact, so the
    value is the host scan's bit for bit (tests/test_boundary.py).

    source / serial: the device model (``_lib.Model``: ``cov_block``, ``serial``) whose
    resident V holds this posterior, and its posterior serial at predict time. With
    them the off-diagonal entries are computed when asked for (k_cov_block):
    ``block(rows, cols)``, ``cov[i, j]`` and any pair of ints / slices take one block
    call without forming the matrix; every other use (``np.asarray``, ufuncs, linalg,
    arithmetic) materialises the dense matrix once and keeps it, up to
    ``DENSE_MAX_BYTES``. Once the model has moved on (its serial changed: an update,
    new hyperparameters, another grid) such an access raises RuntimeError -- the V
    it would read belongs to another posterior. The diagonal (``np.diag``,
    ``np.amax``, ``np.argmax``, ``np.trace``, ``cov[i, i]``) stays ``var`` throughout.
    Without a source (as before): only the diagonal, anything else raises TypeError."""

    __slots__ = ("var", "fused", "source", "serial", "_cache")

    DENSE_MAX_BYTES = 1 << 30

    def __init__(self, var, fused=None, source=None, serial=None):
        self.var = np.asarray(var, dtype=np.float64).reshape(-1)
        self.fused = fused
        self.source = source
        self.serial = (source.serial() if serial is None else serial) if source is not None else None
        self._cache = None

    @property
    def shape(self):
        return (self.var.shape[0], self.var.shape[0])

    ndim = 2
    dtype = np.dtype(np.float64)

    def diagonal(self):
        return self.var.copy()

    def __len__(self):
        return self.var.shape[0]

    def _live(self):
        """The source model, checked to hold this posterior still."""
        if self.source is None:
            raise TypeError("DiagCov holds only the diagonal of the posterior covariance (the off-diagonal "
                            "entries are never computed); use np.diag(cov) / np.amax(cov)")
        if self.source.serial() != self.serial:
            raise RuntimeError("the model has been updated since this predict (its data, hyperparameters or grid "
                               "changed): the off-diagonal covariance of the earlier posterior is gone; "
                               "np.diag(cov) still holds its diagonal")
        return self.source

    def _cells(self, sel):
        """An index list for one axis: None (all cells) or an int64 array in [0, M)."""
        M = self.var.shape[0]
        if sel is None:
            return None
        if isinstance(sel, slice):
            return np.arange(*sel.indices(M), dtype=np.int64)
        a = np.asarray(sel)
        if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
            if a.size:
                raise IndexError("cell indices must be integers")
            a = a.astype(np.int64)
        a = a.astype(np.int64).reshape(-1)
        if a.size and (a.min() < -M or a.max() >= M):
            raise IndexError(f"cell index out of range for {M} cells")
        return np.where(a < 0, a + M, a)

    def block(self, rows, cols=None):
        """cov[rows, cols] as an [a, b] ndarray: rows / cols are sequences of cell indices
        (negative ones count from the end), slices, or None = all cells. One k_cov_block
        launch; the M x M matrix is never formed."""
        src = self._live()
        return src.cov_block(self._cells(rows), self._cells(cols))

    def apply(self, x):
        """cov @ x without the matrix: x is [M] or [M, k] (k <= 8 columns), the result has the
        same shape. Two streamed passes over the model's resident V per column
        (_lib.Model.cov_apply), so it also serves grids whose dense covariance np.asarray
        refuses -- e.g. w @ cov.apply(w), the variance of the field's mass over a region.
        Stale once the model has moved on (RuntimeError), as the off-diagonal accessors;
        not available on precision="f32" models (TypeError)."""
        src = self._live()
        if getattr(src, "dtype", _lib.F64) != _lib.F64:
            raise TypeError("DiagCov.apply needs the fp64 resident V: not available on precision='f32' models")
        xa = np.asarray(x, dtype=np.float64)
        M = self.var.shape[0]
        if xa.ndim not in (1, 2) or xa.shape[0] != M:
            raise ValueError(f"x must be [M] or [M, k] with M = {M}")
        if xa.ndim == 1:
            return src.cov_apply(xa)
        if xa.shape[1] == 0:
            return np.empty((M, 0), dtype=np.float64)
        return np.ascontiguousarray(src.cov_apply(np.ascontiguousarray(xa.T)).T)

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 2 and all(isinstance(i, (int, np.integer)) for i in idx):
            i, j = (int(v) % self.var.shape[0] for v in idx)
            if i == j and (self.source is None or all(-len(self) <= int(v) < len(self) for v in idx)):
                return self.var[i]
        if (self.source is not None and isinstance(idx, tuple) and len(idx) == 2
                and all(isinstance(i, (int, np.integer, slice)) for i in idx)):
            M = self.var.shape[0]
            sel = []
            for i in idx:
                if isinstance(i, slice):
                    sel.append(i)
                else:
                    if not -M <= int(i) < M:
                        raise IndexError(f"index {int(i)} is out of bounds for axis of size {M}")
                    sel.append([int(i)])
            b = self.block(*sel)
            # (an int drops its axis, as on an ndarray)
            return b[tuple(slice(None) if isinstance(i, slice) else 0 for i in idx)]
        return self._dense()[idx]

    def _dense(self):
        if self.var.shape[0] == 1 and self.source is None:
            return self.var.reshape(1, 1).copy()
        src = self._live()
        if self._cache is None:
            M = self.var.shape[0]
            if 8 * M * M > self.DENSE_MAX_BYTES:
                raise MemoryError(f"the dense {M} x {M} covariance takes {8 * M * M} bytes, more than "
                                  f"DiagCov.DENSE_MAX_BYTES = {self.DENSE_MAX_BYTES}; take the entries you need "
                                  "with cov.block(rows, cols)")
            d = src.cov_block(None, None)
            d.flags.writeable = False   # (shared by every later use of this covariance)
            self._cache = d
        return self._cache

    def __array__(self, dtype=None, copy=None):
        d = self._dense()
        if dtype is not None and np.dtype(dtype) != d.dtype:
            return d.astype(dtype)
        return d.copy() if copy else d

    def __array_function__(self, func, types, args, kwargs):
        if func in (np.diag, np.diagonal):
            k = kwargs.get("k", kwargs.get("offset", args[1] if len(args) > 1 else 0))
            if k == 0:
                # what np.diag / np.diagonal of a 2-D array give: a read-only view of
                # the diagonal (no copy; the view keeps the result buffer alive)
                d = self.var.view()
                d.flags.writeable = False
                return d
        if (func in (np.amax, np.max) and len(args) == 1 and not kwargs):
            return self.fused[0] if self.fused is not None else self.var.max()
        if func in (np.amax, np.max) and kwargs.get("axis", args[1] if len(args) > 1 else None) is None:
            return self.var.max()
        if func is np.argmax and kwargs.get("axis", args[1] if len(args) > 1 else None) is None:
            # flat index of the maximum of the dense matrix (first diagonal maximum)
            i = self.fused[1] if (self.fused is not None and len(args) == 1 and not kwargs) else int(np.argmax(self.var))
            return i * self.var.shape[0] + i
        if func is np.trace:
            return self.var.sum()
        args = tuple(self._dense() if a is self else a for a in args)
        return func(*args, **kwargs)

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        inputs = tuple(self._dense() if x is self else x for x in inputs)
        return getattr(ufunc, method)(*inputs, **kwargs)

    def __repr__(self):
        return f"DiagCov(M={self.var.shape[0]}, diag={self.var!r})"


def _dense_op(name):
    def op(self, *other):
        return getattr(self._dense(), name)(*other)
    op.__name__ = name
    return op


for _name in ("__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__",
              "__rtruediv__", "__neg__", "__abs__", "__lt__", "__le__", "__gt__", "__ge__"):
    setattr(DiagCov, _name, _dense_op(_name))


def _as2(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 2))


def _as1(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


class _DeviceGP:
    """Shared device plumbing of SFGP / MFGP."""

    _kind = None
    # precision of the device-resident V = L^-1 psi^T: "f64" (the reference's) or
    # "f32" (BASELINE configs[4]: V stored and streamed in fp32, the factor, solves
    # and reductions in fp64); set on the instance before its first update
    precision = "f64"

    def _dev(self):
        m = self.__dict__.get("_model")
        if m is None:
            dt = _lib.F32 if self.precision == "f32" else _lib.F64
            m = _lib.Model(_lib.context(), self._kind, self._hyp_vec(), self.jitter, dtype=dt)
            self.__dict__["_model"] = m
            self.__dict__["_synced"] = None
            self.__dict__["_grid"] = None
            self.__dict__["_hyp_pushed"] = None
        return m

    def _hyp_vec(self):
        return np.ascontiguousarray(np.asarray(self.hyp, dtype=np.float64).reshape(-1))

    def _push_hyp(self):
        h = self._hyp_vec()
        key = (h.tobytes(), float(self.jitter))
        if self.__dict__.get("_hyp_pushed") == key and self.__dict__.get("_model") is not None:
            return   # the device model already holds these hyperparameters
        self._dev().set_hyp(h, self.jitter)
        self.__dict__["_hyp_pushed"] = key

    def _grid_to_device(self, X_star):
        # every predict compares all M cells of X_star with the grid the device
        # holds (a private copy): an in-place edit of the caller's array, anywhere,
        # moves the device to the new grid (the reference evaluates the kernel on
        # whatever X_star holds at the call, gp:139 / gp:426-429); ~10-20 us at M = 16384
        g = self.__dict__.get("_grid")
        xs = _as2(X_star)
        if g is None or g.shape != xs.shape or not np.array_equal(g, xs):
            self._dev().set_grid(xs)
            self.__dict__["_grid"] = xs.copy()

    def _predict_dev(self, X_star):
        self._sync_data()
        self._push_hyp()
        self._grid_to_device(X_star)
        # (the arrays are the model's pinned result buffer, handed over: no copy;
        # with the max / argmax of var its launch reduced, when it did)
        m = self._dev()
        mu, var, fused = m.predict_view(with_max=True)
        if m.dtype != _lib.F64:   # (an fp32 V serves no covariance blocks: the diagonal only)
            return mu.reshape(-1, 1), DiagCov(var, fused)
        return mu.reshape(-1, 1), DiagCov(var, fused, source=m, serial=m.serial())

    def _pathwise(self, X_star, N_samples, rng, normals, prior):
        """Pathwise samples on the lattice grid X_star -> [M, N_samples] (_lib.Model.sample)."""
        if not prior:
            self._sync_data()
        self._push_hyp()
        self._grid_to_device(X_star)
        m = self._dev()
        try:
            if normals is None:
                nz = m.sample_dims(prior=prior)["nz"]
                if rng is None:
                    rng = np.random.default_rng()
                draw = rng if callable(rng) else rng.standard_normal
                normals = draw((int(N_samples), nz))
            return m.sample(normals, prior=prior).T
        except _lib.NoLatticeError as e:
            raise ValueError(f"{e}; pathwise samples need a lattice grid with every training row on one of its "
                             "cells: draw_posterior_samples / draw_prior_samples take the dense route") from None

    def sample_posterior(self, X_star, N_samples=1, rng=None, normals=None):
        """N_samples joint draws of predict(X_star)'s posterior on the whole grid ->
        [M, N_samples], by pathwise (Matheron) conditioning from the resident V at a cost
        linear in M (mfgp_sample_posterior): no M x M covariance is formed, so it
        serves grids draw_posterior_samples cannot. X_star must be a lattice (meshgrid
        order) and every training row one of its cells, else ValueError. rng: a
        np.random.Generator (default np.random.default_rng()); normals [N_samples, nz]
        (nz: _lib.Model.sample_dims) replaces the draw, and a sample's bits depend on its
        own row of normals only."""
        return self._pathwise(X_star, N_samples, rng, normals, False)

    def sample_prior(self, X_star, N_samples=1, rng=None, normals=None):
        """N_samples joint draws of the zero-mean (hifi) prior on the lattice grid X_star ->
        [M, N_samples], from the separable axis factors (no data involved)."""
        return self._pathwise(X_star, N_samples, rng, normals, True)

    @staticmethod
    def _method(method):
        if method not in ("dense", "pathwise"):
            raise ValueError("method must be 'dense' or 'pathwise'")
        return method == "pathwise"

    def draw_prior_samples(self, X_star, N_samples=1, method="dense"):
        """gaussian_process.py:180-191: N_samples joint draws of the zero-mean prior at
        X_star -> [n, N_samples]. K is the prior covariance k**(X_star, X_star) computed
        on the device (SF: s k; MF: the hifi prior rho^2 s_L k_L + s_H k_H); the draw is
        numpy's (np.random.multivariate_normal, the global generator) as there.
        method="pathwise": sample_prior with normals from np.random.standard_normal (the
        same global generator), linear in the grid's size."""
        if self._method(method):
            return self._pathwise(X_star, N_samples, np.random.standard_normal, None, True)
        self._push_hyp()
        self._grid_to_device(X_star)
        K = self._dev().cov_block(None, None, prior=True)
        return np.random.multivariate_normal(np.zeros(K.shape[0]), K, N_samples).T

    def draw_posterior_samples(self, X_star, N_samples=1, method="dense"):
        """gaussian_process.py:193-217: N_samples joint draws of the posterior at X_star ->
        [n, N_samples]. These are draws of predict(X_star)'s posterior (mean with the
        prior mean and centred observations, gp:132-143 / 414-432); the reference's
        method leaves both out (gp:210-211), see DESIGN.md section 9.
        method="pathwise": sample_posterior with normals from np.random.standard_normal
        (the same global generator), without the dense covariance."""
        if self._method(method):
            return self._pathwise(X_star, N_samples, np.random.standard_normal, None, False)
        mu, cov = self.predict(X_star)
        return np.random.multivariate_normal(mu.flatten(), np.asarray(cov), N_samples).T

    def variance_reduction(self, X_star, candidates=None, weights=None):
        """Integrated variance reduction per candidate: how much the weighted posterior
        variance of predict(X_star), summed over all of X_star's points, falls if the
        (hifi) field is measured at X_star[c], sum_i w_i cov(i, c)^2 / (cov(c, c) + noise +
        jitter) -- the A-optimal criterion, from the resident V without the dense
        covariance (_lib.Model.var_reduction). candidates: row indices
        of X_star (any order, repeats allowed), None = every row. weights: None (ones),
        [M] or [nw, M] with nw <= 8. Returns [nc], or [nw, nc] for 2-D weights. Not
        available on precision="f32" models (TypeError, as their covariance blocks)."""
        if self._dev().dtype != _lib.F64:
            raise TypeError("variance_reduction needs the fp64 resident V: not available on precision='f32' models")
        self._sync_data()
        self._push_hyp()
        self._grid_to_device(X_star)
        return self._dev().var_reduction(candidates, weights)

    def _query(self, X, X_L_new=None, X_H_new=None, **want):
        """_lib.Model.query on the current data and hyperparameters (no grid involved)."""
        self._sync_data()
        self._push_hyp()
        return self._dev().query(_as2(X), None if X_L_new is None else _as2(X_L_new),
                                 None if X_H_new is None else _as2(X_H_new), **want)

    def predict_at(self, X):
        """(mu [n,1], var [n]): predict's posterior mean and variance at the arbitrary
        points X [n,D], from the resident factor. Unlike predict(X) it leaves the grid,
        the resident V and the resident posterior as they are."""
        q = self._query(X, mu=True, var=True)
        return q.mu.reshape(-1, 1), q.var

    @property
    def L(self):
        """Lower Cholesky factor of K + jitter*I (gp:254 / gp:529), downloaded on demand."""
        self._sync_data()
        self._push_hyp()
        return self._dev().factor()

    def likelihood(self, hyp):
        """gaussian_process.py:81-106 / 344-385: negative log-marginal likelihood of the
        training data under `hyp`, on the GPU. (The reference also stores the factor
        of K(hyp) in self.L as a side effect; here .L always reflects .hyp.)"""
        self._sync_data()
        return self._dev().nlml(self._hyp_arg(hyp))

    def likelihood_and_grad(self, hyp):
        """(NLML, dNLML/dhyp) -- what autograd's value_and_grad(self.likelihood) gives the
        reference's train (gp:117, 397); the gradient is analytic here."""
        self._sync_data()
        return self._dev().nlml(self._hyp_arg(hyp), grad=True)

    def _hyp_arg(self, hyp):
        h = np.ascontiguousarray(np.asarray(hyp, dtype=np.float64).reshape(-1))
        if h.shape[0] != self._hyp_vec().shape[0]:
            raise TypeError("Hyperparameters must be of length 4 (single-fidelity) or 9 (multi-fidelity)")
        return h

    def callback(self, params):
        """gaussian_process.py:219-227 / 483-491."""
        print("Log likelihood {}".format(self.likelihood(params)))

    def _hyps_arg(self, hyps):
        h = np.ascontiguousarray(np.asarray(hyps, dtype=np.float64))
        if h.ndim != 2 or h.shape[1] != self._hyp_vec().shape[0]:
            raise TypeError("Hyperparameters must be of length 4 (single-fidelity) or 9 (multi-fidelity)")
        return h

    def likelihood_batch(self, hyps):
        """likelihood for every row of hyps [S, nhyp] in one set of launches
        (mfgp_nlml_batch): values [S], row s with the bits of likelihood(hyps[s]). A row
        that is not positive definite raises LinAlgError, as likelihood does."""
        self._sync_data()
        return self._dev().nlml_batch(self._hyps_arg(hyps))

    def likelihood_and_grad_batch(self, hyps):
        """(values [S], gradients [S, nhyp]): likelihood_and_grad for every row of hyps."""
        self._sync_data()
        return self._dev().nlml_batch(self._hyps_arg(hyps), grad=True)

    def train(self, n_restarts=0, starts=None, scale=1.0, seed=None):
        """gaussian_process.py:108-119 / 388-399: L-BFGS-B on the NLML with its gradient.

        With n_restarts > 0 or explicit starts [S, nhyp] (not in the reference) it trains
        from several starts in lockstep on the batched likelihood
        (training.lockstep_minimize on mfgp_nlml_batch): self.hyp followed by n_restarts
        draws of self.hyp + scale * N(0, 1) from np.random.default_rng(seed), or the given
        starts as they are. Each start's run is the solo L-BFGS-B run from it. self.hyp
        becomes the x of the lowest final NLML among the starts that did not fail (a tie:
        the earliest); self.train_runs holds one record per start (x0, x, fun, nit, nfev,
        success, message). A start that reaches a point that is not positive definite
        ends as failed; if every start fails, LinAlgError is raised and self.hyp stays.
        There is no per-iteration callback in this mode (it would cost one more device
        evaluation per iteration)."""
        if not n_restarts and starts is None:
            from scipy.optimize import minimize
            result = minimize(self.likelihood_and_grad, self.hyp, jac=True, method="L-BFGS-B",
                              callback=self.callback)
            self.hyp = result.x
            return
        from .training import lockstep_minimize
        if starts is None:
            h0 = self._hyp_vec()
            rng = np.random.default_rng(seed)
            starts = np.vstack([h0] + [h0 + scale * rng.standard_normal(h0.shape[0]) for _ in range(int(n_restarts))])
        starts = self._hyps_arg(starts).copy()
        self._sync_data()
        model = self._dev()

        def batch_fun(xs):
            v, g, st = model.nlml_batch(np.vstack(xs), grad=True, status=True)
            return [(float(v[i]), g[i].copy()) if st[i] == 0 else
                    np.linalg.LinAlgError(f"Matrix is not positive definite (leading minor of order {int(st[i])})")
                    for i in range(len(xs))]

        results = lockstep_minimize(batch_fun, starts)
        runs, best = [], None
        for x0, r in zip(starts, results):
            if isinstance(r, BaseException):
                if not isinstance(r, np.linalg.LinAlgError):
                    raise r
                runs.append({"x0": x0, "x": None, "fun": float("nan"), "nit": 0, "nfev": 0, "success": False,
                             "message": str(r)})
                continue
            runs.append({"x0": x0, "x": r.x, "fun": float(r.fun), "nit": int(r.nit), "nfev": int(r.nfev),
                         "success": bool(r.success), "message": r.message})
            if best is None or runs[-1]["fun"] < best["fun"]:
                best = runs[-1]
        self.train_runs = runs
        if best is None:
            raise np.linalg.LinAlgError("train: every start reached a point that is not positive definite")
        self.hyp = best["x"].copy()

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_model":
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        m = self.__dict__.get("_model")
        if m is not None:
            new.__dict__["_model"] = m.clone()
            # the clone holds exactly the device state of `self`; re-key its sync marker
            syn = self.__dict__.get("_synced")
            if syn is not None:
                new.__dict__["_synced"] = tuple(copy.deepcopy(a, memo) if a is not None else None for a in syn)
        return new


class SFGP(_DeviceGP):
    """Single-fidelity GP (gaussian_process.py:23-268) on the GPU."""

    _kind = _lib.SF

    def __init__(self, X, y, len):
        self.D = X.shape[1]                   # gp:36
        self.X = X
        self.y = y
        self.hyp = self.init_params(len)      # gp:40
        self.jitter = 1e-8                    # gp:42
        # gp:44 computes the NLML here only to set self.L; the factor is built
        # lazily on the device at the first updt*/predict instead.

    def init_params(self, len):
        """gaussian_process.py:46-64."""
        hyp = np.log(np.ones(self.D + 1))
        self.idx_theta = np.arange(hyp.shape[0])
        logsigma_n = np.array([-4.0])
        hyp = np.concatenate([hyp, logsigma_n])
        hyp[0] = -4.0
        hyp[2] = np.log(len)
        return hyp

    def _sync_data(self):
        syn = self.__dict__.get("_synced")
        if syn is not None and syn[0] is self.X and syn[1] is self.y:
            return
        X, y = _as2(self.X), _as1(self.y)
        self._push_hyp()
        self._dev().set_data(np.empty((0, 2)), np.empty(0), X, y)
        self.__dict__["_synced"] = (self.X, self.y)

    def updt_info(self, X_new, y_new):
        """gaussian_process.py:229-255: replace the data and refactor (raises LinAlgError if not PD)."""
        self.X = X_new
        self.y = y_new
        self.__dict__["_synced"] = None
        self._sync_data()

    def updt(self, X_addition, y_addition):
        """gaussian_process.py:257-268: append (k >= 0 rows) and refactor."""
        prev = (self.X, self.y)
        self.X = np.vstack((self.X, X_addition))
        self.y = np.vstack((self.y, y_addition))
        syn = self.__dict__.get("_synced")
        if syn is not None and syn[0] is prev[0] and syn[1] is prev[1]:
            self._push_hyp()
            self.__dict__["_synced"] = None
            self._dev().append(_as2(X_addition), _as1(y_addition))
            self.__dict__["_synced"] = (self.X, self.y)
        else:
            self.__dict__["_synced"] = None
            self._sync_data()

    def predict(self, X_star):
        """gaussian_process.py:121-148 -> (mu [M,1], DiagCov of the posterior covariance)."""
        return self._predict_dev(X_star)

    def ExpectedImprovement(self, X_star):
        """gaussian_process.py:150-178 -> [n,1]: gp:171-176 applied to predict's posterior
        at X_star (predict_at; the reference's own mean there has no prior mean and
        uncentred y)."""
        from scipy.stats import norm
        mu, var = self.predict_at(X_star)
        v = np.abs(var).reshape(-1, 1)       # gp:171: |variance|, not its root
        gain = np.min(self.y) - mu           # gp:174: the best observed value minus the mean
        z = gain / v                         # gp:175
        return gain * norm.cdf(z) + v * norm.pdf(z)   # gp:176


class MFGP(_DeviceGP):
    """Two-level AR(1) multi-fidelity GP (gaussian_process.py:271-578) on the GPU."""

    _kind = _lib.MF

    def __init__(self, X_L, y_L, X_H, y_H, len_L, len_H):
        self.D = X_H.shape[1]                 # gp:287
        self.X_L = X_L
        self.y_L = y_L
        self.X_H = X_H
        self.y_H = y_H
        self.idx_theta_L = np.empty([0, 0])
        self.idx_theta_H = np.empty([0, 0])
        self.hyp = self.init_params(len_L, len_H)
        self.jitter = 1e-8                    # gp:298

    def init_params(self, len_L, len_H):
        """gaussian_process.py:300-327."""
        hyp = np.ones(self.D + 1)
        hyp[0] = 0
        self.idx_theta_L = np.arange(hyp.shape[0])
        hyp = np.concatenate((hyp, hyp))
        self.idx_theta_H = np.arange(self.idx_theta_L[-1] + 1, hyp.shape[0])
        rho = np.array([-1.0])
        sigma_n = np.array([0, 0])
        hyp = np.concatenate((hyp, rho, sigma_n))
        hyp[0] = 0
        hyp[3] = 0
        hyp[2] = np.log(len_L)
        hyp[5] = np.log(len_H)
        return hyp

    def _sync_data(self):
        syn = self.__dict__.get("_synced")
        if syn is not None and all(a is b for a, b in zip(syn, (self.X_L, self.y_L, self.X_H, self.y_H))):
            return
        self._push_hyp()
        self._dev().set_data(_as2(self.X_L), _as1(self.y_L), _as2(self.X_H), _as1(self.y_H))
        self.__dict__["_synced"] = (self.X_L, self.y_L, self.X_H, self.y_H)

    def updt_info(self, X_L_new, y_L_new, X_H_new, y_H_new):
        """gaussian_process.py:493-529."""
        self.X_L, self.y_L, self.X_H, self.y_H = X_L_new, y_L_new, X_H_new, y_H_new
        self.__dict__["_synced"] = None
        self._sync_data()

    def updt_hifi(self, X_H_addition, y_H_addition):
        """gaussian_process.py:531-542: append hifi rows (k >= 0) and refactor."""
        prev = (self.X_L, self.y_L, self.X_H, self.y_H)
        syn = self.__dict__.get("_synced")
        xa, ya = np.atleast_2d(X_H_addition), np.atleast_2d(y_H_addition)
        if (syn is not None and all(a is b for a, b in zip(syn, prev)) and xa.ndim == 2 and ya.ndim == 2
                and xa.shape[1:] == np.shape(self.X_H)[1:] and ya.shape[1:] == np.shape(self.y_H)[1:]):
            # the rows go to the device first: the append returns at the step's
            # positive-definiteness verdict, and the host copies below overlap the
            # posterior the launch is still computing (the reference stacks before it
            # factors; a non-PD append still leaves the stacked rows, as there)
            self._push_hyp()
            self.__dict__["_synced"] = None
            try:
                self._dev().append(_as2(X_H_addition), _as1(y_H_addition))
            finally:
                self.X_H = np.vstack((self.X_H, X_H_addition))
                self.y_H = np.vstack((self.y_H, y_H_addition))
            self.__dict__["_synced"] = (self.X_L, self.y_L, self.X_H, self.y_H)
        else:
            self.X_H = np.vstack((self.X_H, X_H_addition))
            self.y_H = np.vstack((self.y_H, y_H_addition))
            self.__dict__["_synced"] = None
            self._sync_data()

    def predict(self, X_star):
        """gaussian_process.py:401-438 -> (mu [M,1], DiagCov of the posterior covariance)."""
        return self._predict_dev(X_star)

    def pred_var(self, x, X_L_new, X_H_new):
        """gaussian_process.py:440-481: the dense [n,n] posterior covariance at x with the
        prospective points X_L_new / X_H_new (at most _lib.LOOK_MAX together) added to the
        model, which stays as it is. MemoryError above DiagCov.DENSE_MAX_BYTES;
        pred_var_diag gives the diagonal without the matrix."""
        n = _as2(x).shape[0]
        if 8 * n * n > DiagCov.DENSE_MAX_BYTES:
            raise MemoryError(f"the dense {n} x {n} covariance takes {8 * n * n} bytes, more than "
                              f"DiagCov.DENSE_MAX_BYTES = {DiagCov.DENSE_MAX_BYTES}; use pred_var_diag")
        return self._query(x, X_L_new, X_H_new, mu=False, var=False, cov=True).cov

    def pred_var_diag(self, x, X_L_new, X_H_new):
        """np.diag(pred_var(x, X_L_new, X_H_new)) -> [n], without forming the matrix."""
        return self._query(x, X_L_new, X_H_new, mu=False, var=True).var

    def _neg_var_many(self, X, thrd, c, X_L_new, X_H_new):
        """get_neg_var at every row of X [n,2] -> [n], one query launch."""
        q = self._query(X, X_L_new, X_H_new, mu=True, var0=True, var=True)
        return np.where(q.mu + c * q.var0 <= thrd, 0.0, -q.var)

    def get_neg_var(self, x, thrd, c, X_L_new, X_H_new):
        """gaussian_process.py:544-563: x is one point [D]; 0 where mean + c * var_old <= thrd
        (the variance, not its root, as there), else minus the look-ahead variance at
        x as a 1 x 1 array."""
        x = np.asarray(x, dtype=np.float64)[None, :]
        q = self._query(x, X_L_new, X_H_new, mu=True, var0=True, var=True)
        if q.mu[0] + c * q.var0[0] <= thrd:
            return 0
        return -q.var.reshape(1, 1)

    def get_max_var(self, Bounds, Thrd, c, X_L_new, X_H_new):
        """gaussian_process.py:565-578 -> (x [1,D], value). scipy's differential evolution
        as there (init='random'), but vectorised: a generation is one query launch
        (updating='deferred'; the reference's updates point by point)."""
        from scipy.optimize import differential_evolution
        lo, hi = Bounds[0], Bounds[1]                 # gp:576 reads Bounds as [[x_lo, y_lo], [x_hi, y_hi]]
        box = [(lo[0], hi[0]), (lo[1], hi[1])]

        def neg_var(x, thrd, c_, xl, xh):
            # a generation [D, S], or the polish step's single point [D]
            x = np.asarray(x, dtype=np.float64)
            if x.ndim == 1:
                return self._neg_var_many(x[None, :], thrd, c_, xl, xh)[0]
            return self._neg_var_many(x.T, thrd, c_, xl, xh)
        res = differential_evolution(neg_var, box, args=(Thrd, c, X_L_new, X_H_new), init="random",
                                     vectorized=True, updating="deferred")
        return res.x.reshape(1, -1), -res.fun
