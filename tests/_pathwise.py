"""Shared pieces of the pathwise-sampling tests (test_pathwise_host.py,
test_gpu_pathwise.py): a numpy restatement of the sampler, the fixed cases and the
basis trick that turns the sampler's linear map into a covariance without statistics.

Pathwise (Matheron) conditioning: with K the training covariance (noise and jitter
included), psi the cross covariance and m the prior means,
    f_post(grid) = m_H + f_prior(grid) + psi K^-1 (y - m - f_prior(X) - eps).
On a lattice the SE prior separates: sqrt(s) Ax Z Ay^T with Ax Ax^T = Kx, Ay Ay^T = Ky
(pchol: diagonally pivoted Cholesky of the unit-diagonal axis Gram, stopped at a largest
remaining diagonal entry <= 2^-50). SF: one field; MF: u_L and delta, hifi = rho u_L +
delta, a lofi row sees u_L. A sample is affine in its nz normals, f = f(0) + J z, and its
covariance is J J^T = sum_i a_i a_i^T with a_i = f(e_i) - f(0): exactly
k** - psi K^-1 psi^T.
"""
import numpy as np

from oracle import gp_oracle as O
from tests._lookahead import HYP_MF, HYP_SF, field, floored_rel   # noqa: F401

STOP = 2.0 ** -50

# grid -> training-row counts (the issue's table)
SHAPES = [((13, 11), (0, 1, 63, 64, 65, 129)),     # M = 143: a ragged last tile
          ((17, 19), (197, 257)),
          ((8, 8), (65,)),                         # M = 64 exactly
          ((5, 13), (64,))]                        # M = 65
CASES = [(kind, g, N) for kind in ("sf", "mf") for g, Ns in SHAPES for N in Ns]


def hyp_of(kind):
    return HYP_SF if kind == "sf" else HYP_MF


def axis_gram(a, l):
    t = np.asarray(a, dtype=np.float64) / l
    return np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2)


def pchol(K, stop=STOP):
    """Diagonally pivoted Cholesky of a PSD matrix -> A [n, r] with A A^T = K up to a PSD
    remainder whose largest diagonal entry is <= stop (rows are not permuted)."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    d = np.diag(K).copy()
    used = np.zeros(n, dtype=bool)
    cols = []
    for _ in range(n):
        dm = np.where(used, -np.inf, d)
        p = int(np.argmax(dm))
        if not dm[p] > stop:
            break
        c = K[:, p].copy()
        for cj in cols:
            c -= cj * cj[p]
        piv = np.sqrt(d[p])
        c /= piv
        c[used] = 0.0
        c[p] = piv
        d -= c * c
        d[p] = 0.0
        used[p] = True
        cols.append(c)
    return np.array(cols).T.reshape(n, len(cols))


def lattice(nx, ny, ylo=0.0, yhi=1.0):
    gx, gy = np.linspace(0.0, 1.0, nx), np.linspace(ylo, yhi, ny)
    return gx, gy, np.array([(a, b) for a in gx for b in gy])


def case(kind, shape, N, seed=None):
    """Grid axes, the grid, and N training rows on random cells with two repeated cells
    (N >= 3); MF: N_L = N // 3 and (N_L >= 1, N_H >= 1) one cell holding both a lofi and a
    hifi row. -> dict(gx, gy, Xs, ix, iy, X, y, NL, hyp)."""
    nx, ny = shape
    gx, gy, Xs = lattice(nx, ny)
    rng = np.random.default_rng(1000 * nx + 10 * N + (kind == "mf") if seed is None else seed)
    cells = rng.integers(0, nx * ny, N)
    NL = 0 if kind == "sf" else N // 3
    if N >= 3:
        cells[N - 1] = cells[N - 2]                  # a repeated cell
        cells[(N - 1) // 2] = cells[N - 2]           # and again
    if NL >= 1 and N - NL >= 1:
        cells[NL] = cells[0]                         # one cell with a lofi and a hifi row
    X = Xs[cells].copy()
    y = field(X, rng) if N else np.empty(0)
    return dict(kind=kind, gx=gx, gy=gy, Xs=Xs, ix=cells // ny, iy=cells % ny, X=X, y=y, NL=NL, hyp=hyp_of(kind))


def fields_of(c):
    """Per field (s, l) -> [(sqrt(s) scaling is applied by the caller) Ax, Ay]."""
    h = c["hyp"]
    ls = [np.exp(h[2])] if c["kind"] == "sf" else [np.exp(h[2]), np.exp(h[5])]
    return [(pchol(axis_gram(c["gx"], l)), pchol(axis_gram(c["gy"], l))) for l in ls]


def dims(c, prior=False):
    fs = fields_of(c)
    nzf = sum(ax.shape[1] * ay.shape[1] for ax, ay in fs)
    return nzf + (0 if prior else c["X"].shape[0]), fs


def oracle_mean_cov(c):
    """(mu, dense posterior covariance) of the oracle's restatement of the reference."""
    X, y, NL, hyp, Xs = c["X"], c["y"], c["NL"], c["hyp"], c["Xs"]
    if X.shape[0] == 0:
        return np.full(Xs.shape[0], O.prior_mean(hyp)), prior_cov(c)
    if c["kind"] == "sf":
        return O.sf_faithful(X, y, hyp, Xs, return_cov=True)
    return O.mf_faithful(X[:NL], y[:NL], X[NL:], y[NL:], hyp, Xs, return_cov=True)


def prior_cov(c):
    hyp, Xs = c["hyp"], c["Xs"]
    if c["kind"] == "sf":
        return O.se_kernel(Xs, Xs, hyp[1], hyp[2])
    rho = np.exp(hyp[6])
    return rho ** 2 * O.se_kernel(Xs, Xs, hyp[1], hyp[2]) + O.se_kernel(Xs, Xs, hyp[4], hyp[5])


def pathwise(c, Z, prior=False):
    """The sampler in numpy: Z [S, nz] -> samples [S, M] (grid order: x outer)."""
    h, kind = c["hyp"], c["kind"]
    Z = np.asarray(Z, dtype=np.float64)
    S = Z.shape[0]
    nz, fs = dims(c, prior)
    assert Z.shape[1] == nz
    X, NL = c["X"], c["NL"]
    N = 0 if prior else X.shape[0]
    if kind == "sf":
        sc, rho = [np.sqrt(np.exp(h[1]))], 1.0
        mL = mH = np.exp(h[0])
        nL = nH = np.exp(h[3])
    else:
        sc, rho = [np.sqrt(np.exp(h[1])), np.sqrt(np.exp(h[4]))], np.exp(h[6])
        mL = np.exp(h[0])
        mH = rho * mL + np.exp(h[3])
        nL, nH = np.exp(h[7]), np.exp(h[8])
    off, U = 0, []
    for (ax, ay), s in zip(fs, sc):
        k = ax.shape[1] * ay.shape[1]
        Zf = Z[:, off:off + k].reshape(S, ax.shape[1], ay.shape[1])
        U.append(s * np.einsum("ia,sab,jb->sij", ax, Zf, ay))
        off += k
    hifi = rho * U[0] + (U[1] if kind == "mf" else 0.0)
    out = hifi.reshape(S, -1) + (0.0 if prior else mH)
    if N == 0:
        return out
    ix, iy = c["ix"], c["iy"]
    lo = np.arange(N) < NL
    fX = np.where(lo[None, :], U[0][:, ix, iy], hifi[:, ix, iy])
    m = np.where(lo, mL, mH)
    sd = np.sqrt(np.where(lo, nL, nH) + O.JITTER)
    r = (c["y"] - m)[None, :] - fX - sd[None, :] * Z[:, off:off + N]
    if kind == "sf":
        K = O.se_kernel(X, X, h[1], h[2]) + np.eye(N) * (nH + O.JITTER)
        psi = O.se_kernel(c["Xs"], X, h[1], h[2])
    else:
        K = O.mf_K(X[:NL], X[NL:], h)
        psi = O.mf_psi(c["Xs"], X[:NL], X[NL:], h)
    L = np.linalg.cholesky(K)
    import scipy.linalg as sla
    V = sla.solve_triangular(L, psi.T, lower=True)
    W = sla.solve_triangular(L, r.T, lower=True)
    return out + (V.T @ W).T


def basis_cov(sample, nz, chunk=64):
    """sum_i a_i a_i^T, a_i = sample(e_i) - sample(0), with the unit vectors fed in calls
    of at most `chunk` rows -> (f(0) [M], covariance [M, M])."""
    f0 = sample(np.zeros((1, nz)))[0]
    C = np.zeros((f0.shape[0], f0.shape[0]))
    for i0 in range(0, nz, chunk):
        n = min(chunk, nz - i0)
        E = np.zeros((n, nz))
        E[np.arange(n), i0 + np.arange(n)] = 1.0
        A = sample(E) - f0[None, :]
        C += A.T @ A
    return f0, C
