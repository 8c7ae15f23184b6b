"""The shared reference of the integrated-variance-reduction tests (tests/test_ivr_host.py,
tests/test_gpu_ivr.py), in numpy on the oracle's dense covariance.

Measuring the hifi field at grid cell c lowers the posterior variance of cell i by
cov(i, c)^2 / (cov(c, c) + sigma_H + jitter); sigma_H + jitter is the diagonal term a hifi
append adds to K (gp:253-254 / gp:525-529; SF: the model's single noise). With C the
reference's dense covariance on the grid (O.sf_faithful / O.mf_faithful, return_cov=True):

    closed form   ivr_w(c) = sum_i w_i C[i, c]^2 / (C[c, c] + exp(hyp[-1]) + jitter)
    append form   ivr_w(c) = sum_i w_i (diag C - diag C')[i],  C' with x_c stacked under the hifi rows

The metric is the project's floored-relative one carried to this quantity:
    max_c |ivr - ref| / max(|ref|, 1e-6 k** sum_i |w_i|) <= O.PARITY_TOL.

Hyperparameters, grids and revisited cells are those of tests/test_gpu_cov_block.py.
"""
import numpy as np

from oracle import gp_oracle as O
from tests.test_gpu_cov_block import GRIDS, HYP_MF, HYP_SF, _distinct, _grid, _model, _revisit  # noqa: F401

JITTER = O.JITTER
NL_MF = 60


def hyp_of(kind):
    return HYP_SF if kind == "sf" else HYP_MF


def grid(name):
    return _grid(*GRIDS[name])


def data(kind, Xs, N, seed):
    """N revisited cells (drawn with replacement) and the lofi count: MF takes the first
    min(60, N // 2) rows as lofi."""
    NL = 0 if kind == "sf" else min(NL_MF, N // 2)
    X, y = _revisit(Xs, max(N, 1), seed)
    return X[:N], y[:N], NL


def prior_cov(kind, Xs, hyp):
    if kind == "sf":
        return O.se_kernel(Xs, Xs, hyp[1], hyp[2])
    rho = np.exp(hyp[6])
    return rho ** 2 * O.se_kernel(Xs, Xs, hyp[1], hyp[2]) + O.se_kernel(Xs, Xs, hyp[4], hyp[5])


def dense_cov(kind, X, y, NL, Xs, hyp, jitter=JITTER):
    """The reference's dense posterior covariance on Xs (the prior's without rows)."""
    if X.shape[0] == 0:
        return prior_cov(kind, Xs, hyp)
    if kind == "sf":
        return O.sf_faithful(X, y, hyp, Xs, jitter=jitter, return_cov=True)[1]
    return O.mf_faithful(X[:NL], y[:NL], X[NL:], y[NL:], hyp, Xs, jitter=jitter, return_cov=True)[1]


def weights2(w, M):
    w = np.ones((1, M)) if w is None else np.asarray(w, dtype=np.float64)
    return w.reshape(-1, w.shape[-1])[:, :M]


def ivr_closed(C, hyp, w=None, cand=None, jitter=JITTER):
    """[nw, nc] from the dense covariance C: the closed form."""
    M = C.shape[0]
    cand = np.arange(M) if cand is None else np.asarray(cand, dtype=np.int64)
    d = np.diag(C)[cand] + np.exp(hyp[-1]) + jitter
    Cc = C[:, cand]
    return np.stack([(wk[:, None] * Cc ** 2).sum(0) / d for wk in weights2(w, M)])


def ivr_append(kind, X, y, NL, Xs, hyp, cand, w=None, jitter=JITTER):
    """[nw, nc]: the weighted fall of the diagonal when x_c joins the hifi rows."""
    M = Xs.shape[0]
    W = weights2(w, M)
    v0 = np.diag(dense_cov(kind, X, y, NL, Xs, hyp, jitter))
    out = np.empty((W.shape[0], len(cand)))
    for j, c in enumerate(cand):
        X1, y1 = np.vstack((X, Xs[c:c + 1])), np.concatenate((y, [0.0]))
        v1 = np.diag(dense_cov(kind, X1, y1, NL, Xs, hyp, jitter))
        out[:, j] = W @ (v0 - v1)
    return out


def floor(hyp, w, M):
    """[nw, 1]: the metric's floor per weight vector."""
    return 1e-6 * O.prior_variance(hyp) * np.abs(weights2(w, M)).sum(1, keepdims=True)


def err(got, ref, hyp, w, M):
    got, ref = np.atleast_2d(np.asarray(got)), np.atleast_2d(np.asarray(ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), floor(hyp, w, M))))


def weight_sets(M, seed):
    """The weight vectors of the tests: random positive, a mask that zeroes whole 64-cell
    tiles and parts of others, and stacks of 3 and 8 vectors (mask and ones among them)."""
    rng = np.random.default_rng(seed)
    pos = rng.random(M) + 0.05
    mask = (rng.random(M) < 0.7).astype(np.float64) * (rng.random(M) + 0.1)
    for t in range(0, (M + 63) // 64, 3):          # every third tile: all zeros
        mask[64 * t:64 * (t + 1)] = 0.0
    if M > 64:
        mask[64:64 + 40] = 0.0                       # and a part of tile 1
    if not mask.any():
        mask[M // 2] = 1.0
    w3 = np.stack((pos, mask, np.ones(M)))
    w8 = np.vstack((w3, rng.random((5, M)) * (rng.random((5, M)) < 0.5)))
    return {"pos": pos, "mask": mask, "w3": w3, "w8": w8}
