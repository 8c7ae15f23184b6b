"""CPU oracle for the GP posterior update -- TEST INFRASTRUCTURE ONLY.

This module is the checker, never the product. Only ``tests/``,
``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of ``bench.py`` may
import it. The product path (``mfgp_coverage_amd``) never imports it and fails
loudly when its HIP library is missing.

It restates, in NumPy, the single hot path of MSU-dcypherlab/mfgp-coverage
(``/root/reference``):

* ``se_kernel``        <- ``SFGP.kernel`` gaussian_process.py:66-79
                          (``MFGP.kernel`` gaussian_process.py:329-342 is identical)
* ``sf_faithful``      <- ``SFGP.updt_info`` gp:229-255 + ``SFGP.predict`` gp:121-148,
                          same op sequence (dense K(X*,X*), four ``np.linalg.solve``,
                          dense ``psi @ beta``), returns ``diag`` of the covariance.
* ``mf_faithful``      <- ``MFGP.updt_info`` gp:493-529 + ``MFGP.predict`` gp:401-438.
* ``sf_diag``/``mf_diag`` -- the same math with a Cholesky, two triangular solves
                          and a row-sum of squares (no M x M matrices). This is the
                          semantic spec of the HIP kernels and the stronger CPU
                          baseline.
* ``nlml``             <- ``likelihood`` gp:81-106 / 344-385 with an analytic gradient;
  ``nlml_extended``       the same formula wholly in 80-bit long double, the yardstick
                          of both ``nlml`` and mfgp_nlml at tile edges
                          (tests/golden/make_nlml_edges_golden.py).
* ``posterior_extended``  ``sf_diag`` / ``mf_diag`` wholly in 80-bit long double, the
                          yardstick of both and of every device route to the posterior
                          at tile edges (tests/golden/make_posterior_edges_golden.py).

Pinning: ``tests/test_oracle.py`` checks this module
against golden vectors produced by importing the reference itself in the build
container (``tests/golden/make_golden.py``), against the reference's own logged
runs (``Data/*_agent.csv`` VarMax / Var0 replays), and against closed forms.

Hyperparameter layouts (log-scaled, simulator.py:53-56, 83-84):
  SF: [mu, s^2, L, noise]
  MF: [mu_lo, s^2_lo, L_lo, mu_hi, s^2_hi, L_hi, rho, noise_lo, noise_hi]
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

JITTER = 1e-8  # gaussian_process.py:42 (SF) and :298 (MF)


def se_kernel(x, xp, log_s2, log_l):
    """Squared-exponential kernel, gaussian_process.py:66-79.

    Scales before subtracting (``x/l - xp/l``, gp:77-78); ``s`` and ``l`` are the
    exponentiated log hyperparameters (gp:75-76).
    """
    output_scale = np.exp(log_s2)
    lengthscale = np.exp(log_l)
    diffs = np.expand_dims(x / lengthscale, 1) - np.expand_dims(xp / lengthscale, 0)
    return output_scale * np.exp(-0.5 * np.sum(diffs ** 2, axis=2))


# ---------------------------------------------------------------------------
# Reference-faithful restatements (same op sequence, dense covariance)
# ---------------------------------------------------------------------------

def sf_faithful(X, y, hyp, Xs, jitter=JITTER, return_cov=False):
    """SFGP.updt_info (gp:229-255) then SFGP.predict (gp:121-148)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    y = np.asarray(y, dtype=np.float64).reshape(-1, 1)
    hyp = np.asarray(hyp, dtype=np.float64)
    N = y.shape[0]
    sigma_n = np.exp(hyp[-1])                                        # gp:248-249
    K = se_kernel(X, X, hyp[1], hyp[2]) + np.eye(N) * sigma_n        # gp:253
    L = np.linalg.cholesky(K + np.eye(N) * jitter)                  # gp:254
    mean = np.exp(hyp[0])                                            # gp:132
    yc = y - mean                                                    # gp:133
    psi = se_kernel(Xs, X, hyp[1], hyp[2])                           # gp:139
    alpha = np.linalg.solve(np.transpose(L), np.linalg.solve(L, yc))  # gp:141
    mu = np.matmul(psi, alpha) + mean                                # gp:142-143
    beta = np.linalg.solve(np.transpose(L), np.linalg.solve(L, psi.T))  # gp:145
    cov = se_kernel(Xs, Xs, hyp[1], hyp[2]) - np.matmul(psi, beta)   # gp:146
    if return_cov:
        return mu[:, 0], cov
    return mu[:, 0], np.diag(cov).copy()


def _mf_parts(hyp):
    hyp = np.asarray(hyp, dtype=np.float64)
    theta_L, theta_H = hyp[0:3], hyp[3:6]                            # gp:310-313
    rho = np.exp(hyp[-3])                                            # gp:414
    mean_L = np.exp(theta_L[0])                                      # gp:415
    mean_H = rho * mean_L + np.exp(theta_H[0])                       # gp:416
    return theta_L, theta_H, rho, mean_L, mean_H


def mf_K(XL, XH, hyp, jitter=JITTER):
    """Block covariance of MFGP.updt_info, gp:510-529 (jitter included)."""
    theta_L, theta_H, rho, _, _ = _mf_parts(hyp)
    sigma_n_L = np.exp(hyp[-2])
    sigma_n_H = np.exp(hyp[-1])
    NL, NH = XL.shape[0], XH.shape[0]
    K_LL = se_kernel(XL, XL, theta_L[1], theta_L[2]) + np.eye(NL) * sigma_n_L   # gp:523
    K_LH = rho * se_kernel(XL, XH, theta_L[1], theta_L[2])                     # gp:524
    K_HH = rho ** 2 * se_kernel(XH, XH, theta_L[1], theta_L[2]) + \
        se_kernel(XH, XH, theta_H[1], theta_H[2]) + np.eye(NH) * sigma_n_H     # gp:525-526
    K = np.vstack((np.hstack((K_LL, K_LH)), np.hstack((K_LH.T, K_HH))))       # gp:527-528
    return K + np.eye(NL + NH) * jitter


def mf_psi(Xs, XL, XH, hyp):
    """Cross covariance of MFGP.predict, gp:426-429."""
    theta_L, theta_H, rho, _, _ = _mf_parts(hyp)
    psi1 = rho * se_kernel(Xs, XL, theta_L[1], theta_L[2])
    psi2 = rho ** 2 * se_kernel(Xs, XH, theta_L[1], theta_L[2]) + \
        se_kernel(Xs, XH, theta_H[1], theta_H[2])
    return np.hstack((psi1, psi2))


def mf_faithful(XL, yL, XH, yH, hyp, Xs, jitter=JITTER, return_cov=False):
    """MFGP.updt_info (gp:493-529) then MFGP.predict (gp:401-438)."""
    XL = np.asarray(XL, dtype=np.float64).reshape(-1, 2)
    XH = np.asarray(XH, dtype=np.float64).reshape(-1, 2)
    yL = np.asarray(yL, dtype=np.float64).reshape(-1, 1)
    yH = np.asarray(yH, dtype=np.float64).reshape(-1, 1)
    theta_L, theta_H, rho, mean_L, mean_H = _mf_parts(hyp)
    L = np.linalg.cholesky(mf_K(XL, XH, hyp, jitter))                # gp:529
    y = np.vstack((yL - mean_L, yH - mean_H))                        # gp:419-424
    psi = mf_psi(Xs, XL, XH, hyp)                                    # gp:426-429
    alpha = np.linalg.solve(np.transpose(L), np.linalg.solve(L, y))  # gp:431
    mu = mean_H + np.matmul(psi, alpha)                              # gp:432
    beta = np.linalg.solve(np.transpose(L), np.linalg.solve(L, psi.T))  # gp:434
    cov = rho ** 2 * se_kernel(Xs, Xs, theta_L[1], theta_L[2]) + \
        se_kernel(Xs, Xs, theta_H[1], theta_H[2]) - np.matmul(psi, beta)  # gp:435-436
    if return_cov:
        return mu[:, 0], cov
    return mu[:, 0], np.diag(cov).copy()


# ---------------------------------------------------------------------------
# Diag-only restatements (semantic spec of the kernels; scalable CPU baseline)
# ---------------------------------------------------------------------------

def _diag_solve(K, psi, r, kss, mean):
    N = K.shape[0]
    if N == 0:
        M = psi.shape[0]
        return np.full(M, mean, dtype=np.float64), np.full(M, kss, dtype=np.float64)
    L = np.linalg.cholesky(K)
    V = sla.solve_triangular(L, psi.T, lower=True, check_finite=False)   # V = L^-1 psi^T
    z = sla.solve_triangular(L, r, lower=True, check_finite=False)       # z = L^-1 (y - m)
    mu = mean + V.T @ z                       # psi alpha = psi L^-T L^-1 r = V^T z
    var = kss - np.einsum("ij,ij->j", V, V)   # diag(k** - psi K^-1 psi^T)
    return mu, var


def sf_diag(X, y, hyp, Xs, jitter=JITTER):
    """Posterior mean and diagonal variance of SFGP (gp:229-255, 121-148)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    hyp = np.asarray(hyp, dtype=np.float64)
    N = X.shape[0]
    K = se_kernel(X, X, hyp[1], hyp[2]) + np.eye(N) * np.exp(hyp[-1])
    K = K + np.eye(N) * jitter
    psi = se_kernel(Xs, X, hyp[1], hyp[2])
    mean = np.exp(hyp[0])
    kss = np.exp(hyp[1])            # kernel(X*,X*) diagonal = s * exp(0)
    return _diag_solve(K, psi, y - mean, kss, mean)


def mf_diag(XL, yL, XH, yH, hyp, Xs, jitter=JITTER):
    """Posterior mean and diagonal variance of MFGP (gp:493-529, 401-438)."""
    XL = np.asarray(XL, dtype=np.float64).reshape(-1, 2)
    XH = np.asarray(XH, dtype=np.float64).reshape(-1, 2)
    yL = np.asarray(yL, dtype=np.float64).reshape(-1)
    yH = np.asarray(yH, dtype=np.float64).reshape(-1)
    theta_L, theta_H, rho, mean_L, mean_H = _mf_parts(hyp)
    K = mf_K(XL, XH, hyp, jitter)
    psi = mf_psi(Xs, XL, XH, hyp)
    r = np.concatenate((yL - mean_L, yH - mean_H))
    kss = rho ** 2 * np.exp(theta_L[1]) + np.exp(theta_H[1])
    return _diag_solve(K, psi, r, kss, mean_H)


def prior_variance(hyp):
    """Known-answer Var0: variance of the empty GP."""
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.shape[0] == 4:
        return np.exp(hyp[1])
    rho = np.exp(hyp[6])
    return rho ** 2 * np.exp(hyp[1]) + np.exp(hyp[4])


def prior_mean(hyp):
    hyp = np.asarray(hyp, dtype=np.float64)
    if hyp.shape[0] == 4:
        return np.exp(hyp[0])
    return _mf_parts(hyp)[4]


# ---------------------------------------------------------------------------
# Tolerance policy (BASELINE.json north_star "1e-6 rel fp64")
# ---------------------------------------------------------------------------

def parity_errors(mu, var, mu_ref, var_ref, kss):
    """Return (mu_rel, var_floored_rel).

    mu:  max |d| / |ref|.
    var: max |d| / max(|ref|, 1e-6 * k**) -- posterior variance next to data is
         ~1e-9 against a prior of ~0.06, i.e. pure catastrophic cancellation in
         k** - sum(V^2); the reference's own rounding is larger than 1e-6 * 1e-9
         there, so the relative bound is floored at 1e-6 * k**.
    """
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    var = np.asarray(var, dtype=np.float64).reshape(-1)
    mu_ref = np.asarray(mu_ref, dtype=np.float64).reshape(-1)
    var_ref = np.asarray(var_ref, dtype=np.float64).reshape(-1)
    mu_err = np.max(np.abs(mu - mu_ref) / np.maximum(np.abs(mu_ref), 1e-300)) if mu.size else 0.0
    den = np.maximum(np.abs(var_ref), 1e-6 * kss)
    var_err = np.max(np.abs(var - var_ref) / den) if var.size else 0.0
    return float(mu_err), float(var_err)


PARITY_TOL = 1e-6


def parity_errors_f32(mu, var, mu_ref, var_ref, kss):
    """Tolerance metric of the MFGP_F32 mode (BASELINE configs[4]: the resident V
    stored and streamed in fp32, everything else fp64) against this fp64 oracle.
    Returns (mu_err, var_err):

    mu:  max |d| / max(|ref|, 1e-2 * max|ref|, 1e-300) -- fp32 storage of V puts
         an absolute error of ~1e-8 on mu (2^-24 per V entry times |V^T z|); the
         posterior mean of a [0, 1] field crosses zero, so the relative bound is
         floored at 1 % of the field's largest |mu|: where |ref| is below that
         floor the gate F32_TOL is an ABSOLUTE bound of F32_TOL * 1e-2 * max|mu_ref|
         (1e-6 * max|mu_ref|), elsewhere relative; an all-zero mu_ref is compared
         against the 1e-300 floor (finite, never nan);
    var: max |d| / max(|ref|, 1e-6 * k**), the fp64 metric.
    Measured on australia9 (128x128, N = 2048, numpy emulation of the kernels'
    arithmetic): fp32 V alone 7e-7 / 3e-7; with the f32 accumulation of
    psi_new - L21 V_old 1.2e-6 / 2.2e-6. Gate: F32_TOL.
    """
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    var = np.asarray(var, dtype=np.float64).reshape(-1)
    mu_ref = np.asarray(mu_ref, dtype=np.float64).reshape(-1)
    var_ref = np.asarray(var_ref, dtype=np.float64).reshape(-1)
    if not mu.size:
        return 0.0, 0.0
    mden = np.maximum(np.maximum(np.abs(mu_ref), 1e-2 * np.max(np.abs(mu_ref))), 1e-300)
    vden = np.maximum(np.abs(var_ref), 1e-6 * kss)
    return float(np.max(np.abs(mu - mu_ref) / mden)), float(np.max(np.abs(var - var_ref) / vden))


F32_TOL = 1e-4


# ---------------------------------------------------------------------------
# Voronoi-cell reductions (simulator.py:105-136, 194-323) -- checker for
# mfgp_cells.hip / geometry.py. Membership is in_polygon (sim:105-124), i.e.
# matplotlib's Path.contains_points crossing rule, restated here on arrays.
# ---------------------------------------------------------------------------

def in_polygon(pts, verts):
    """Crossing-number test of matplotlib's point_in_path for a closed polygon:
    an edge whose end points straddle the point's y (yflag = vy >= ty) toggles
    when ((vy1 - ty) * (vx0 - vx1) >= (vx1 - tx) * (vy0 - vy1)) == yflag1."""
    tx, ty = pts[:, 0], pts[:, 1]
    inside = np.zeros(pts.shape[0], dtype=bool)
    n = verts.shape[0]
    x0, y0 = verts[0]
    f0 = y0 >= ty
    for e in range(1, n + 1):
        x1, y1 = verts[e % n]
        f1 = y1 >= ty
        hit = ((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1
        inside ^= (f0 != f1) & hit
        f0, x0, y0 = f1, x1, y1
    return inside


def poly_area(v):
    """Shoelace area (sim:127-136)."""
    x, y = v[:, 0], v[:, 1]
    return 0.5 * np.abs(np.dot(x, np.roll(y, 1)) - np.dot(y, np.roll(x, 1)))


def cell_reductions(polys, seeds, xs, w=None, f=None, var=None):
    """Per cell: (members, centroid, loss term, max var, argmax index) with the
    reference's formulas (sim:210-221, 255-270, 305-311)."""
    res = []
    for v, s in zip(polys, seeds):
        m = in_polygon(xs, v)
        area = poly_area(v)
        pts = xs[m]
        cen = loss = vmax = amax = None
        if w is not None:
            ww = w[m]
            cen = (np.mean(ww[:, None] * pts, axis=0) * area) / (np.mean(ww) * area)
        if f is not None:
            loss = np.mean(np.sum((pts - s) ** 2, axis=1) * f[m]) * area
        if var is not None and m.any():
            idx = np.flatnonzero(m)
            vmax = var[idx].max()
            amax = int(idx[np.argmax(var[idx])])
        res.append((m, cen, loss, vmax, amax))
    return res


# ---------------------------------------------------------------------------
# Negative log-marginal likelihood and its gradient (gp:81-106 SF, gp:344-385
# MF; the reference differentiates it with autograd for L-BFGS-B, gp:108-119 /
# 388-399) -- checker for mfgp_nlml. Analytic gradient:
#   NLML = 1/2 r^T K^-1 r + sum log L_ii + N/2 log(2 pi),  r = y - m(hyp)
#   dNLML/dh = 1/2 tr((K^-1 - a a^T) dK/dh) + a^T dr/dh,   a = K^-1 r
# ---------------------------------------------------------------------------

def _sq_dist_scaled(x, xp, log_l):
    lx = np.exp(log_l)
    d = x[:, None, :] / lx - xp[None, :, :] / lx
    return np.sum(d ** 2, axis=2)


def nlml(X, y, hyp, XL=None, yL=None, jitter=JITTER, grad=False):
    """SF: X, y = the data, hyp [4]. MF: XL, yL = lofi, X, y = hifi, hyp [9].
    Returns NLML (and its gradient w.r.t. the log-scaled hyp when grad)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if hyp.shape[0] == 4:
        m, s, lx = np.exp(hyp[0]), np.exp(hyp[1]), hyp[2]
        sn = np.exp(hyp[3])
        r2 = _sq_dist_scaled(X, X, lx)
        E = s * np.exp(-0.5 * r2)
        N = X.shape[0]
        K = E + np.eye(N) * sn + np.eye(N) * jitter
        res = y - m
        dK = [None, E, E * r2, np.eye(N) * sn]
        dr = [-m * np.ones(N), None, None, None]
    else:
        XL = np.asarray(XL, dtype=np.float64).reshape(-1, 2)
        yL = np.asarray(yL, dtype=np.float64).reshape(-1)
        mL, sL, sH = np.exp(hyp[0]), np.exp(hyp[1]), np.exp(hyp[4])
        rho, snL, snH = np.exp(hyp[6]), np.exp(hyp[7]), np.exp(hyp[8])
        mH = rho * mL + np.exp(hyp[3])
        NL, NH = XL.shape[0], X.shape[0]
        Xa = np.vstack([XL, X])
        N = NL + NH
        rL2 = _sq_dist_scaled(Xa, Xa, hyp[2])
        rH2 = _sq_dist_scaled(Xa, Xa, hyp[5])
        EL = sL * np.exp(-0.5 * rL2)
        EH = sH * np.exp(-0.5 * rH2)
        lo = np.zeros(N, dtype=bool)
        lo[:NL] = True
        hi = ~lo
        cL = np.where(lo[:, None] & lo[None, :], 1.0, np.where(hi[:, None] & hi[None, :], rho ** 2, rho))
        cH = (hi[:, None] & hi[None, :]).astype(np.float64)
        dn = np.where(lo, snL, snH)
        K = cL * EL + cH * EH + np.diag(dn) + np.eye(N) * jitter
        res = np.concatenate([yL - mL, y - mH])
        drho = np.where(lo[:, None] & lo[None, :], 0.0, np.where(hi[:, None] & hi[None, :], 2 * rho ** 2, rho))
        dK = [None, cL * EL, cL * EL * rL2, None, cH * EH, cH * EH * rH2, drho * EL,
              np.diag(np.where(lo, snL, 0.0)), np.diag(np.where(hi, snH, 0.0))]
        dr = [np.concatenate([-mL * np.ones(NL), -rho * mL * np.ones(NH)]), None, None,
              np.concatenate([np.zeros(NL), -np.exp(hyp[3]) * np.ones(NH)]), None, None,
              np.concatenate([np.zeros(NL), -rho * mL * np.ones(NH)]), None, None]
    L = np.linalg.cholesky(K)
    a = np.linalg.solve(L.T, np.linalg.solve(L, res))
    val = 0.5 * res @ a + np.sum(np.log(np.diag(L))) + 0.5 * np.log(2.0 * np.pi) * res.shape[0]
    if not grad:
        return float(val)
    Kinv = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(L.shape[0])))
    W = Kinv - np.outer(a, a)
    g = np.zeros(hyp.shape[0])
    for p in range(hyp.shape[0]):
        if dK[p] is not None:
            g[p] += 0.5 * np.sum(W * dK[p])
        if dr[p] is not None:
            g[p] += a @ dr[p]
    return float(val), g


# ---------------------------------------------------------------------------
# The same NLML and gradient wholly in extended precision -- the yardstick of
# nlml() above and of mfgp_nlml at block edges (tests/golden/
# make_nlml_edges_golden.py). np.linalg does not take longdouble: the Cholesky
# and the substitutions are plain row loops with vectorised inner products.
# ---------------------------------------------------------------------------

LD = np.longdouble


def _require_extended():
    eps = np.finfo(LD).eps
    if not eps < 1e-18:
        raise RuntimeError(f"np.longdouble has eps = {float(eps):.3g} here (not the 80-bit x87 format, eps 1.08e-19): "
                           "nlml_extended would be no extended-precision reference on this platform")


def _chol_ld(K):
    """Lower Cholesky factor of a longdouble matrix, column by column."""
    N = K.shape[0]
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        d = K[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < N:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _fwd_ld(L, B):
    """L^-1 B by forward substitution (B [N] or [N, k])."""
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _back_ld(L, B):
    """L^-T B by back substitution."""
    Y = np.zeros_like(B)
    for i in range(L.shape[0] - 1, -1, -1):
        Y[i] = (B[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


# exp and log from +, -, *, / alone. libm's expl / logl run the x87 f2xm1 / fyl2x
# instructions, whose last bits differ from one CPU vendor to the next; cond(K)
# amplifies that difference (measured between two hosts: 18 float64 ulp on the value
# at cond 2.6e3, 3e-13 relative at cond 1.7e8). The basic operations are correctly
# rounded everywhere, so these give the same bits on every x86-64 host.
_LN2_HI = LD(6.93147180369123816490e-01)     # the leading 32 bits of ln 2: k * _LN2_HI is exact
_LN2_LO = LD(1.90821492927058770002e-10)     # ln 2 - _LN2_HI
_LN2 = _LN2_HI + _LN2_LO
_PI = LD(3.141592653589793) + LD(1.2246467991473532e-16)      # pi = hi + lo (float64 each)


def _exp_ld(x):
    """exp(x) = 2^k exp(r), |r| <= ln(2) / 2, exp(r) by its Taylor series (Horner; the
    22nd term is below 1e-31; r in two steps, the first exact). Relative error a few
    eps (1.08e-19)."""
    x = np.asarray(x, dtype=LD)
    k = np.rint(x / _LN2)
    r = (x - k * _LN2_HI) - k * _LN2_LO
    s = np.ones_like(r)
    for n in range(22, 0, -1):
        s = LD(1) + r * s / LD(n)
    return np.ldexp(s, k.astype(np.int64))


def _log_ld(x):
    """log(x), x > 0, by Newton's iteration y += x exp(-y) - 1 from e ln 2 + (m - 1)
    (x = m 2^e; the first error is below 0.2 and squares in every step)."""
    x = np.asarray(x, dtype=LD)
    m, e = np.frexp(x)
    y = e.astype(LD) * _LN2 + (m - LD(1))
    for _ in range(7):
        y = y + (x * _exp_ld(-y) - LD(1))
    return y


def _sq_dist_scaled_ld(x, log_l, xp=None):
    """Squared distances of the rows of x to those of xp (default: x), scaled as se_kernel does."""
    lx = _exp_ld(log_l)
    d = x[:, None, :] / lx - (x if xp is None else xp)[None, :, :] / lx
    return np.sum(d * d, axis=2)


def _mf_parts_ld(NL, N, rho, snL, snH):
    """The MF block structure over NL lofi rows and N - NL hifi rows, shared by nlml_extended and
    posterior_extended: the masks (lo, hi, ll, hh), the coefficients cL (1 | rho | rho^2) and
    cH (0 | 1) of the lofi and hifi kernels in K, and the noise diagonal."""
    lo = np.zeros(N, dtype=bool)
    lo[:NL] = True
    hi = ~lo
    ll, hh = lo[:, None] & lo[None, :], hi[:, None] & hi[None, :]
    cL = np.where(ll, LD(1), np.where(hh, rho * rho, rho)).astype(LD)
    cH = np.where(hh, LD(1), LD(0)).astype(LD)
    return lo, hi, ll, hh, cL, cH, np.diag(np.where(lo, snL, snH))


def _posterior_parts_ld(XL, yL, XH, yH, hyp, Xs, jitter=JITTER):
    """(K [N, N], psi [M, N], r [N], mean, k**) of the posterior in longdouble: the SF / MF
    assembly of posterior_extended (K with the noise and the jitter on its diagonal)."""
    _require_extended()
    hyp = np.asarray(hyp, dtype=np.float64).astype(LD)
    XL = np.asarray(XL, dtype=np.float64).reshape(-1, 2).astype(LD)
    XH = np.asarray(XH, dtype=np.float64).reshape(-1, 2).astype(LD)
    yL = np.asarray(yL, dtype=np.float64).reshape(-1).astype(LD)
    yH = np.asarray(yH, dtype=np.float64).reshape(-1).astype(LD)
    Xs = np.asarray(Xs, dtype=np.float64).reshape(-1, 2).astype(LD)
    jit, half = LD(jitter), LD(0.5)
    if hyp.shape[0] == 4:
        mean, s, sn = _exp_ld(hyp[0]), _exp_ld(hyp[1]), _exp_ld(hyp[3])
        N = XH.shape[0]
        eye = np.eye(N, dtype=LD)
        K = s * _exp_ld(-half * _sq_dist_scaled_ld(XH, hyp[2])) + eye * sn + eye * jit
        psi = s * _exp_ld(-half * _sq_dist_scaled_ld(Xs, hyp[2], XH))
        res, kss = yH - mean, s
    else:
        mL, sL, sH = _exp_ld(hyp[0]), _exp_ld(hyp[1]), _exp_ld(hyp[4])
        rho, snL, snH = _exp_ld(hyp[6]), _exp_ld(hyp[7]), _exp_ld(hyp[8])
        mean = rho * mL + _exp_ld(hyp[3])
        NL, NH = XL.shape[0], XH.shape[0]
        N = NL + NH
        Xa = np.vstack([XL, XH])
        lo, hi, _, _, cL, cH, noise = _mf_parts_ld(NL, N, rho, snL, snH)
        K = cL * (sL * _exp_ld(-half * _sq_dist_scaled_ld(Xa, hyp[2]))) + \
            cH * (sH * _exp_ld(-half * _sq_dist_scaled_ld(Xa, hyp[5]))) + noise + np.eye(N, dtype=LD) * jit
        # a grid cell is a hifi point: its columns of K's last block row
        pL = np.where(lo, rho, rho * rho).astype(LD)[None, :]
        pH = np.where(hi, LD(1), LD(0)).astype(LD)[None, :]
        psi = pL * (sL * _exp_ld(-half * _sq_dist_scaled_ld(Xs, hyp[2], Xa))) + \
            pH * (sH * _exp_ld(-half * _sq_dist_scaled_ld(Xs, hyp[5], Xa)))
        res, kss = np.concatenate([yL - mL, yH - mean]), rho * rho * sL + sH
    return K, psi, res, mean, kss


def posterior_extended(XL, yL, XH, yH, hyp, Xs, jitter=JITTER):
    """sf_diag / mf_diag (hyp [4]: XL / yL empty; hyp [9]: MF) evaluated wholly in
    np.longdouble: kernel assembly with _exp_ld, _chol_ld, V = L^-1 psi^T and z = L^-1 r by
    _fwd_ld, mu = mean + V^T z, var = k** - colsum(V o V). The float64 inputs are taken as
    exact; N = 0 gives the prior. Returns (mu [M], var [M], k**) as longdouble -- the
    yardstick of the fp64 oracle and of every device route to the posterior at tile edges
    (tests/golden/make_posterior_edges_golden.py). No libm function is called. Raises
    RuntimeError where longdouble is no wider than 64 bits of mantissa, LinAlgError on a
    K that is not positive definite."""
    K, psi, res, mean, kss = _posterior_parts_ld(XL, yL, XH, yH, hyp, Xs, jitter)
    N = K.shape[0]
    M = psi.shape[0]
    if N == 0:
        return np.full(M, mean, dtype=LD), np.full(M, kss, dtype=LD), kss
    assert K.dtype == LD and psi.dtype == LD and res.dtype == LD
    L = _chol_ld(K)
    V = _fwd_ld(L, np.ascontiguousarray(psi.T))
    z = _fwd_ld(L, res)
    mu = mean + V.T @ z
    var = kss - np.sum(V * V, axis=0)
    assert mu.dtype == LD and var.dtype == LD
    return mu, var, kss


def nlml_extended(X, y, hyp, XL=None, yL=None, jitter=JITTER):
    """nlml(..., grad=True) evaluated wholly in np.longdouble (80-bit on x86-64): kernel
    assembly, exp and log (from the basic operations: _exp_ld, _log_ld), Cholesky, both
    triangular solves, K^-1, the trace and the mean terms. The float64 inputs are taken as exact. Returns (value, grad) as longdouble.
    Raises RuntimeError where longdouble is no wider than 64 bits of mantissa."""
    _require_extended()
    hyp = np.asarray(hyp, dtype=np.float64).astype(LD)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2).astype(LD)
    y = np.asarray(y, dtype=np.float64).reshape(-1).astype(LD)
    jit = LD(jitter)
    one, half, two = LD(1), LD(0.5), LD(2)
    if hyp.shape[0] == 4:
        m, s, sn = _exp_ld(hyp[0]), _exp_ld(hyp[1]), _exp_ld(hyp[3])
        N = X.shape[0]
        r2 = _sq_dist_scaled_ld(X, hyp[2])
        E = s * _exp_ld(-half * r2)
        eye = np.eye(N, dtype=LD)
        K = E + eye * sn + eye * jit
        res = y - m
        dK = [None, E, E * r2, eye * sn]
        dr = [-m * np.ones(N, dtype=LD), None, None, None]
    else:
        XL = np.asarray(XL, dtype=np.float64).reshape(-1, 2).astype(LD)
        yL = np.asarray(yL, dtype=np.float64).reshape(-1).astype(LD)
        mL, sL, sH = _exp_ld(hyp[0]), _exp_ld(hyp[1]), _exp_ld(hyp[4])
        rho, snL, snH = _exp_ld(hyp[6]), _exp_ld(hyp[7]), _exp_ld(hyp[8])
        eH = _exp_ld(hyp[3])
        mH = rho * mL + eH
        NL, NH = XL.shape[0], X.shape[0]
        N = NL + NH
        Xa = np.vstack([XL, X])
        rL2 = _sq_dist_scaled_ld(Xa, hyp[2])
        rH2 = _sq_dist_scaled_ld(Xa, hyp[5])
        EL = sL * _exp_ld(-half * rL2)
        EH = sH * _exp_ld(-half * rH2)
        lo, hi, ll, hh, cL, cH, noise = _mf_parts_ld(NL, N, rho, snL, snH)
        zero = LD(0)
        K = cL * EL + cH * EH + noise + np.eye(N, dtype=LD) * jit
        res = np.concatenate([yL - mL, y - mH])
        drho = np.where(ll, zero, np.where(hh, two * rho * rho, rho)).astype(LD)
        oL, oH = np.ones(NL, dtype=LD), np.ones(NH, dtype=LD)
        dK = [None, cL * EL, cL * EL * rL2, None, cH * EH, cH * EH * rH2, drho * EL,
              np.diag(np.where(lo, snL, zero)), np.diag(np.where(hi, snH, zero))]
        dr = [np.concatenate([-mL * oL, -rho * mL * oH]), None, None,
              np.concatenate([zero * oL, -eH * oH]), None, None,
              np.concatenate([zero * oL, -rho * mL * oH]), None, None]
    g = np.zeros(hyp.shape[0], dtype=LD)
    if N == 0:
        return LD(0), g
    assert K.dtype == LD and res.dtype == LD
    L = _chol_ld(K)
    a = _back_ld(L, _fwd_ld(L, res))
    val = half * (res @ a) + np.sum(_log_ld(np.diag(L))) + half * _log_ld(two * _PI) * LD(N)
    Kinv = _back_ld(L, _fwd_ld(L, np.eye(N, dtype=LD)))
    W = Kinv - np.outer(a, a)
    for p in range(hyp.shape[0]):
        if dK[p] is not None:
            g[p] += half * np.sum(W * dK[p])
        if dr[p] is not None:
            g[p] += a @ dr[p]
    assert val.dtype == LD and g.dtype == LD
    return val, g
