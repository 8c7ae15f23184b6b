"""GPU versions of the planner helpers that sit on the GP hot path.

``compute_sample_points`` mirrors simulator.py:326-374 (the Choi doubling
planner's sample-set selection, called once per period at sim:1031): on a copy
of the model, append the grid cell of maximal posterior variance with its
posterior mean as the observation until the maximal variance is at or below
the threshold, and return the chosen cells in order. Here the whole loop runs
on the device (libmfgp_hip's mfgp_sample_points): every iteration is a 1-row
bordered Cholesky append plus one pass over the resident V with a fused argmax,
and the host synchronises once per 32 iterations. Same signature, same return
value, same model-unchanged contract: the reference works on ``copy.deepcopy``;
here the rows go past the model's own and are dropped at the end (the leading
rows' factor, V and F do not depend on them), and what the loop overwrites
besides -- the resident posterior, the kept result, the path counters -- is saved
and restored, so no copy of the model's device state is made.

``compute_sample_points_batch`` runs the same loop for many models at once (the
Choi planner of a rank's Monte-Carlo seeds: one seed's sample set each): every
iteration is one decision launch for all of them and one batched 1-row append +
predict (libmfgp_hip's mfgp_batch_sample_points, the lattice step where the batch
takes it); each model stops at its own threshold.

``compute_sample_points_ivr`` is the greedy planner on the integrated-variance
criterion instead of the maximal variance (libmfgp_hip's mfgp_plan_ivr, DESIGN.md
section 21): the same in-place loop, each pick scored by a rank-one update from one
product of the posterior covariance with a grid vector.
``compute_sample_points_ivr_batch`` runs it for many models at once, one launch of each
kind per pick for the whole batch, with per-group quotas on the picks ("one cell per
agent"; libmfgp_hip's mfgp_batch_plan_ivr).

On any error (a step that is not positive definite raises LinAlgError, as updt /
updt_hifi does inside the reference's loop) the models are as before the call, and
the points are unspecified.
"""
from __future__ import annotations

import numpy as np

from .gaussian_process import MFGP, SFGP


def _to_device(models, x_star, f64_for=None):
    """What every planner here does first: the models' types checked (f64_for: the caller's
    name, where it needs fp64 models), then each model's data, hyperparameters and the grid
    ``x_star`` brought to the device -> the grid as a contiguous [M, 2] float64 array."""
    from . import _lib
    for m in models:
        if not isinstance(m, (SFGP, MFGP)):
            raise TypeError("Invalid model type: must be SFGP or MFGP")
    for m in models:
        if f64_for and m._dev().dtype != _lib.F64:
            raise TypeError(f"{f64_for} needs the fp64 resident V: not available on precision='f32' models")
    xs = np.ascontiguousarray(np.asarray(x_star, dtype=np.float64).reshape(-1, 2))
    for m in models:
        m._sync_data()
        m._push_hyp()
        m._grid_to_device(xs)
    return xs


def compute_sample_points(model, x_star, threshold, console):
    """simulator.py:326-374 -> [n, 2] ndarray of the cells to sample, in order."""
    xs = _to_device([model], x_star)
    # the reference loops until the threshold is met; bound the output buffer
    # generously and refuse to return a truncated answer
    cap = 4 * xs.shape[0] + 1
    pts = model._dev().sample_points(float(threshold), cap)
    if pts.shape[0] >= cap:
        raise RuntimeError("compute_sample_points: no convergence within %d points" % cap)
    if console:
        print("Sample points to reduce max var below " + str(threshold) + ": " + str(pts.shape[0]))
    return pts


def compute_sample_points_batch(models, x_star, thresholds, console=False):
    """compute_sample_points (simulator.py:326-374) for every model of ``models``
    (one context, one dtype, the same grid ``x_star``), stepped together ->
    list of [n_b, 2] arrays, each model's cells in order. ``thresholds``: one value
    or one per model."""
    from . import _lib
    if not models:
        return []
    xs = _to_device(models, x_star)
    cap = 4 * xs.shape[0] + 1
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (len(models),))
    pts = _lib.batch_sample_points([m._dev() for m in models], thr, cap)
    for b, p in enumerate(pts):
        if p.shape[0] >= cap:
            raise RuntimeError("compute_sample_points: no convergence within %d points" % cap)
        if console:
            print("Sample points to reduce max var below " + str(thr[b]) + ": " + str(p.shape[0]))
    return pts


def compute_sample_points_ivr(model, x_star, n_points, weights=None, candidates=None, min_gain=0.0, refresh=0):
    """The greedy integrated-variance planner: up to ``n_points`` cells of ``x_star``, each
    the allowed cell whose measurement lowers the weighted posterior variance of the
    whole grid most given the picks before it (the A-optimal score of
    ``variance_reduction``) -> ``(points [n, 2], gains [n])``,
    ``gains[t]`` the score of pick t when it was chosen. ``weights``: None (ones) or [M];
    ``candidates``: the allowed rows of ``x_star`` (None = all); the run stops before the
    first pick whose score is below ``min_gain``; ``refresh = R > 0`` recomputes the scores'
    numerators from scratch after every R picks. The model is unchanged, as after
    ``compute_sample_points``; data, hyperparameters and grid reach the device the same way.
    Not available on precision="f32" models (TypeError)."""
    _to_device([model], x_star, f64_for="compute_sample_points_ivr")
    _, pts, gains = model._dev().plan_ivr(n_points, weights, candidates, min_gain, refresh)
    return pts, gains


def compute_sample_points_ivr_batch(models, x_star, n_points, weights=None, candidates=None, groups=None, quota=None,
                                    min_gain=0.0, refresh=0):
    """``compute_sample_points_ivr`` for every model of ``models`` (one context, the same
    grid ``x_star``), stepped together, with per-group quotas on the picks (libmfgp_hip's
    mfgp_batch_plan_ivr) -> a list of ``(points [n_b, 2], gains [n_b],
    groups_of_picks)`` per model. ``weights``: None (ones), one [M] vector for all, or one per
    model; ``candidates``: the allowed rows of ``x_star``, None (all), one list for all, or one
    per model; ``groups``: None (no constraint, ``groups_of_picks`` is None) or the group of
    every candidate position (of every row of ``x_star`` where ``candidates`` is None), one
    list for all or one per model -- a model then makes at most ``quota[g]`` picks (None: one)
    in group g, "one cell per agent", and ``groups_of_picks[t]`` is the group pick t was taken
    for. Each model stops at its own ``min_gain`` crossing, after ``n_points`` picks or when
    no allowed position is left, and is unchanged. Not available on precision="f32" models
    (TypeError)."""
    from . import _lib
    if not models:
        return []
    _to_device(models, x_star, f64_for="compute_sample_points_ivr_batch")
    n = len(models)
    runs = _lib.batch_plan_ivr([m._dev() for m in models], n_points, weights, candidates, groups, quota, min_gain,
                               refresh)
    gl = _lib._per_member(groups, n)
    out = []
    for b, (_, pos, pts, gains) in enumerate(runs):
        picked = None if gl is None else np.asarray(gl[b], dtype=np.int64).reshape(-1)[pos]
        out.append((pts, gains, picked))
    return out
