"""The shared reference of the covariance-product and greedy-planner tests
(tests/test_plan_ivr_host.py, tests/test_gpu_plan_ivr.py), in numpy on the oracle's dense
covariance; built on tests/_ivr.py (its models, grids, weights and metric).

With weights w, C_t the posterior covariance on the grid after t picks and
S_t(c) = sum_i w_i C_t(i, c)^2, picking cell c* as a hifi row gives C_{t+1} = C_t - g g^T,
g = C_t[:, c*] / sqrt(C_t[c*, c*] + sigma_H + jitter), and with x = w o g, tau = w . g^2,
u = C_{t+1} x:

    S_{t+1}(c) = S_t(c) - 2 g(c) u(c) - g(c)^2 tau,   score(c) = S(c) / (diag C(c) + sigma_H + jitter)

recurrence() runs that; scratch_scores() is the independent reference: I.ivr_closed on the
oracle's covariance with the picks stacked under the hifi rows. The metric is _ivr.err's,
the tolerance O.PARITY_TOL. Symmetric grids with N = 0 give exact ties, so picks are never
compared with a reference's picks: each pick is compared with the reference's maximum.
"""
import numpy as np

from oracle import gp_oracle as O
from tests import _ivr as I
from tests._lattice_grids import axis, make_grid

TOL = O.PARITY_TOL
KINDS = ("sf", "mf")
NS = (0, 65, 197)


def extra_grid(name):
    """The grids beyond _ivr.GRIDS: a 16 x 40 y-outer rectangle, a 13 x 11 grid with x
    descending, and 150 scattered points that are no lattice."""
    if name == "16x40_yo":
        return make_grid(axis(16), axis(40, -0.5, 0.7), "y_outer")
    if name == "13x11_xrev":
        return make_grid(axis(13, reverse=True), axis(11))
    if name == "scatter150":
        return np.random.default_rng(150).random((150, 2))
    return I.grid(name)


def weights(name, M, seed=3):
    return None if name == "ones" else I.weight_sets(M, seed)[name]


def wvec(w, M):
    return np.ones(M) if w is None else np.asarray(w, dtype=np.float64)[:M]


def noise_of(hyp):
    return np.exp(hyp[-1]) + I.JITTER


def stacked(X, y, Xs, picks):
    """The training rows with the picked cells stacked under the hifi rows (the values do
    not enter a covariance)."""
    picks = np.asarray(picks, dtype=np.int64)
    return np.vstack((X.reshape(-1, 2), Xs[picks])), np.concatenate((y, np.zeros(picks.shape[0])))


def scratch_cov(kind, X, y, NL, Xs, hyp, picks):
    X1, y1 = stacked(X, y, Xs, picks)
    return I.dense_cov(kind, X1, y1, NL, Xs, hyp)


def scratch_scores(kind, X, y, NL, Xs, hyp, w, picks):
    """[M]: the from-scratch closed form given the picks."""
    return I.ivr_closed(scratch_cov(kind, X, y, NL, Xs, hyp, picks), hyp, w)[0]


def recurrence(C0, hyp, w, n_points, allowed=None):
    """The greedy run by the rank-one recurrence on the dense covariance C0 ->
    (cells [n], gains [n], scores: the list of the [M] score vectors each pick saw)."""
    M = C0.shape[0]
    wv = wvec(w, M)
    allowed = np.arange(M) if allowed is None else np.asarray(allowed, dtype=np.int64)
    nz = noise_of(hyp)
    C = C0.copy()
    S = (wv[:, None] * C ** 2).sum(0)
    cells, gains, scores = [], [], []
    for _ in range(n_points):
        var = np.diag(C)
        sc = S / (var + nz)
        c = int(allowed[np.argmax(sc[allowed])])
        cells.append(c)
        gains.append(sc[c])
        scores.append(sc)
        g = C[:, c] / np.sqrt(var[c] + nz)
        C = C - np.outer(g, g)
        x = wv * g
        tau = wv @ (g * g)
        u = C @ x
        S = S - 2.0 * g * u - g * g * tau
    return np.asarray(cells, dtype=np.int64), np.asarray(gains), scores


def score_err(got, ref, hyp, w, M):
    """_ivr.err's floored-relative metric for one weight vector."""
    return I.err(np.asarray(got).reshape(1, -1), np.asarray(ref).reshape(1, -1), hyp, w, M)


def pick_floor(hyp, w, M):
    return float(I.floor(hyp, w, M)[0, 0])


def check_run(kind, X, y, NL, Xs, hyp, w, cells, gains, allowed=None):
    """The two conditions on every pick of a run, against the from-scratch scores given the
    picks before it -> (worst gain error, worst shortfall from the maximum, both in units of
    max(|ref|, floor)); the caller asserts both <= TOL. Also returns the smallest gap
    between the reference's top two allowed scores per pick (a tie detector)."""
    M = Xs.shape[0]
    allowed = np.arange(M) if allowed is None else np.asarray(allowed, dtype=np.int64)
    fl = pick_floor(hyp, w, M)
    e_gain = e_max = 0.0
    gaps = []
    for t, c in enumerate(cells):
        ref = scratch_scores(kind, X, y, NL, Xs, hyp, w, cells[:t])
        e_gain = max(e_gain, abs(gains[t] - ref[c]) / max(abs(ref[c]), fl))
        best = ref[allowed].max()
        e_max = max(e_max, (best - ref[c]) / max(best, fl))
        top = np.sort(ref[np.unique(allowed)])[-2:]
        gaps.append(((top[-1] - top[0]) / max(top[-1], fl)) if top.shape[0] > 1 else np.inf)
    return e_gain, e_max, np.asarray(gaps)


def v_of(kind, X, NL, Xs, hyp):
    """V = L^-1 psi^T [N, M] from the oracle's factor."""
    if kind == "sf":
        N = X.shape[0]
        K = O.se_kernel(X, X, hyp[1], hyp[2]) + np.eye(N) * np.exp(hyp[-1]) + np.eye(N) * I.JITTER
        psi = O.se_kernel(Xs, X, hyp[1], hyp[2])
    else:
        K = O.mf_K(X[:NL], X[NL:], hyp, I.JITTER)
        psi = O.mf_psi(Xs, X[:NL], X[NL:], hyp)
    return np.linalg.solve(np.linalg.cholesky(K), psi.T)


def cov_apply_from_v(kind, X, NL, Xs, hyp, x):
    """K** x - V^T (V x): the two-pass form, x [M] or [M, k]."""
    Kx = I.prior_cov(kind, Xs, hyp) @ x
    if X.shape[0] == 0:
        return Kx
    V = v_of(kind, X, NL, Xs, hyp)
    return Kx - V.T @ (V @ x)


def kss_separable(kind, gx, gy, order, hyp, x):
    """K** x of the lattice make_grid(gx, gy, order) by the axis products:
    sum_part s_part Kx X Ky^T on the nx x ny reshaping of x."""
    nx, ny = len(gx), len(gy)
    X = x.reshape(nx, ny) if order == "x_outer" else x.reshape(ny, nx).T

    def gram(a, log_l):
        s = np.asarray(a, dtype=np.float64) / np.exp(log_l)
        return np.exp(-0.5 * (s[:, None] - s[None, :]) ** 2)
    if kind == "sf":
        parts = [(np.exp(hyp[1]), hyp[2])]
    else:
        parts = [(np.exp(hyp[6]) ** 2 * np.exp(hyp[1]), hyp[2]), (np.exp(hyp[4]), hyp[5])]
    out = sum(s * (gram(gx, ll) @ X @ gram(gy, ll).T) for s, ll in parts)
    return out.reshape(-1) if order == "x_outer" else out.T.reshape(-1)


def apply_err(got, ref, hyp, x):
    """max |got - ref| / max(|ref|, 1e-6 k** sum|x|), per column of x ([M] or [k, M] rows)."""
    got, ref, x = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (got, ref, x))
    assert got.shape == ref.shape == x.shape, (got.shape, ref.shape, x.shape)
    fl = 1e-6 * O.prior_variance(hyp) * np.abs(x).sum(1, keepdims=True)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), np.maximum(fl, 1e-300))))
