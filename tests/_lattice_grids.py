"""Cases of tests/test_gpu_lattice_grids.py: lattice grids that are not square,
and the training sets on them (no GPU here: tests/test_lattice_grid_cases.py
checks the cases themselves on the CPU).

The lattice step (k_inc_lat / k_lat_gemm2) keeps the two grid axes apart almost
everywhere -- nx / ny, the cell strides sx / sy, tabw = round_up(max(nx, ny), 64),
zq = 2 NT / tabw rows per Z unit, tiles of (128 | 64) / ka x-indices by 64
y-indices, member lists bucketed by py, cells at ix sx + iy sy -- and a square,
uniform, increasing, x-outer grid cannot tell one axis from the other. These
grids can: rectangles both ways round, both cell orders, reversed and warped
axes, a degenerate axis, and tabw = 192 (max(nx, ny) in 129..192).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


def axis(n, lo=0.0, hi=1.0, reverse=False, warp=None):
    """n strictly monotone axis values from lo to hi: uniform, or warped
    (lo + (hi - lo) linspace(0, 1, n) ** warp: uneven spacing); reversed: descending."""
    t = np.linspace(0.0, 1.0, n)
    if warp is not None:
        t = t ** warp
    a = lo + (hi - lo) * t
    return a[::-1].copy() if reverse else a


def make_grid(gx, gy, order="x_outer"):
    """The [nx ny, 2] cells of the axes gx, gy. x_outer: x constant along runs of ny
    cells (the reference's order, cell = ix ny + iy); y_outer: y constant along
    runs of nx cells (cell = iy nx + ix)."""
    gx, gy = np.asarray(gx, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    if order == "x_outer":
        return np.array([(a, b) for a in gx for b in gy], dtype=np.float64).reshape(-1, 2)
    if order == "y_outer":
        return np.array([(a, b) for b in gy for a in gx], dtype=np.float64).reshape(-1, 2)
    raise ValueError(order)


def _monotone(v):
    if v.shape[0] < 2:
        return bool(v[0] == v[0])
    d = np.diff(v)
    return bool(np.all(d > 0) if v[1] > v[0] else np.all(d < 0))


def expected_lattice(Xs):
    """The contract of the library's lattice detection, restated: (nx, ny, sx, sy) --
    axis lengths and cell strides, cell(ix, iy) = ix sx + iy sy -- when the grid is
    two strictly monotone axes (either direction, any spacing) in meshgrid order with
    one coordinate constant along runs of consecutive cells; the x-constant reading
    is tried first (so a single column of cells is nx = 1, a single row ny = 1);
    (0, 0, 0, 0) when the grid is no lattice."""
    Xs = np.asarray(Xs, dtype=np.float64).reshape(-1, 2)
    M = Xs.shape[0]
    if M < 1:
        return (0, 0, 0, 0)
    for s in (0, 1):
        f = 1 - s
        ne = np.flatnonzero(Xs[:, s] != Xs[0, s])
        run = int(ne[0]) if ne.size else M
        if M % run:
            continue
        blk = Xs.reshape(M // run, run, 2)
        if not (np.all(blk[:, :, s] == blk[:, :1, s]) and np.all(blk[:, :, f] == blk[:1, :, f])):
            continue
        if not (_monotone(blk[:, 0, s]) and _monotone(blk[0, :, f])):
            continue
        ns = M // run
        return (ns, run, run, 1) if s == 0 else (run, ns, 1, run)
    return (0, 0, 0, 0)


def axes_of(Xs):
    """(gx, gy) of a lattice grid, read back through expected_lattice's strides."""
    nx, ny, sx, sy = expected_lattice(Xs)
    Xs = np.asarray(Xs, dtype=np.float64).reshape(-1, 2)
    return Xs[np.arange(nx) * sx, 0].copy(), Xs[np.arange(ny) * sy, 1].copy()


def on_lattice(Xs, X):
    """Per row of X: does the device's cell lookup find it on the lattice? The lookup
    (lattice_xy) rounds a uniform estimate (p - a[0]) (n - 1) / (a[n-1] - a[0]) of each
    axis index and compares the axis values at the estimate and its two neighbours for
    exact equality; a row is on the lattice when both axes hit. On a warped axis most
    axis values lie further from their uniform estimate than one index: those rows are
    off the lattice for the step ("virtual" rows, which it handles at full accuracy)."""
    gx, gy = axes_of(Xs)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)

    def hit(a, p):
        n = a.shape[0]
        inv = (n - 1) / (a[-1] - a[0]) if n > 1 else 0.0
        e = np.rint(np.minimum(np.maximum((p - a[0]) * inv, 0.0), float(n - 1))).astype(np.int64)
        ok = np.zeros(p.shape[0], dtype=bool)
        for t in (-1, 0, 1):
            c = e + t
            inb = (c >= 0) & (c < n)
            ok |= inb & (a[np.clip(c, 0, n - 1)] == p)
        return ok

    return hit(gx, X[:, 0]) & hit(gy, X[:, 1])


def expected_virtual(Xs, X, NL, n0, mf):
    """stats()["lattice_virtual"] after a lattice step whose old rows are X[:n0]: the
    off-lattice rows of each kernel part (part 0: every row; MF part 1: the hifi rows
    [NL, n0)), summed."""
    off = ~on_lattice(Xs, X[:n0])
    return int(off.sum()) + (int(off[NL:].sum()) if mf else 0)


def make_data(Xs, n, seed, kind="cells"):
    """n training rows at grid cells and their values: a smooth field (three Gaussian
    bumps, normalised) plus 0.1 noise. Every row -- the base rows and the rows appended
    later alike -- comes from ONE permutation of the cells, so no append duplicates a
    base row; kind="revisit" (grids with fewer than n cells): the permutation repeated,
    so rows past the M-th revisit cells, with fresh noise."""
    Xs = np.asarray(Xs, dtype=np.float64).reshape(-1, 2)
    M = Xs.shape[0]
    rng = np.random.default_rng(seed)
    perm = rng.permutation(M)
    if kind == "cells":
        if n > M:
            raise ValueError(f"{n} distinct cells of {M}")
        idx = perm[:n]
    elif kind == "revisit":
        idx = np.resize(perm, n)
    else:
        raise ValueError(kind)
    X = Xs[idx].copy()
    lo, span = Xs.min(0), np.maximum(Xs.max(0) - Xs.min(0), 1.0)
    c = lo + span * rng.random((3, 2))
    y = sum(np.exp(-np.sum((X - ci) ** 2, 1) / 0.05) for ci in c)
    y = y / max(y.max(), 1e-12) + 0.1 * rng.standard_normal(n)
    return X, y, idx


def shift_rows(Xs, X, rows, coord, frac=0.29):
    """Move rows `rows` of X (in place) off the grid along one coordinate (0: x, 1: y)
    by frac of that axis' first spacing: the other coordinate stays an axis value."""
    g = axes_of(Xs)[coord]
    X[rows, coord] += frac * abs(g[1] - g[0])
    return X


class GreedyVariance:
    """The oracle's MF posterior variance over a sequence of hifi rows appended one at
    a time (the planner's loop, hundreds of points): O.mf_diag's own quantities --
    L = chol(K), V = L^-1 psi^T, var = k** - sum V^2 -- carried forward by the bordered
    Cholesky step in NumPy fp64 instead of being rebuilt per point (O(N M) instead of
    O(N^2 M) each). from_scratch() is O.mf_diag itself for the same rows: the tests
    compare the two at checkpoints, so the reference stays O.mf_diag."""

    def __init__(self, hyp, XL, XH, Xs, room=1024):
        import scipy.linalg as sla
        from oracle import gp_oracle as O
        self.O, self.sla = O, sla
        self.hyp, self.Xs = np.asarray(hyp, dtype=np.float64), Xs
        self.XL, self.XH = np.asarray(XL).reshape(-1, 2), np.asarray(XH).reshape(-1, 2)
        n = self.n = self.XL.shape[0] + self.XH.shape[0]
        self.Lb = np.zeros((n + room, n + room))
        self.Vb = np.zeros((n + room, Xs.shape[0]))
        self.Lb[:n, :n] = np.linalg.cholesky(O.mf_K(self.XL, self.XH, self.hyp))
        self.Vb[:n] = sla.solve_triangular(self.Lb[:n, :n], O.mf_psi(Xs, self.XL, self.XH, self.hyp).T, lower=True,
                                           check_finite=False)
        self.kss = O.prior_variance(self.hyp)
        self.var = self.kss - np.einsum("ij,ij->j", self.Vb[:n], self.Vb[:n])

    def append(self, x):
        O, hyp, n = self.O, self.hyp, self.n
        x = np.asarray(x, dtype=np.float64).reshape(1, 2)
        none = np.empty((0, 2))
        k12 = O.mf_psi(x, self.XL, self.XH, hyp)[0]               # K_HL | K_HH rows of the new hifi row
        k22 = O.mf_psi(x, none, x, hyp)[0, 0] + np.exp(hyp[-1]) + O.JITTER
        l21 = self.sla.solve_triangular(self.Lb[:n, :n], k12, lower=True, check_finite=False)
        l22 = np.sqrt(k22 - l21 @ l21)
        self.Lb[n, :n], self.Lb[n, n] = l21, l22
        v = (O.mf_psi(self.Xs, none, x, hyp)[:, 0] - l21 @ self.Vb[:n]) / l22
        self.Vb[n] = v
        self.var = self.var - v * v
        self.XH = np.vstack([self.XH, x])
        self.n = n + 1

    def from_scratch(self):
        O = self.O
        return O.mf_diag(self.XL, np.zeros(self.XL.shape[0]), self.XH, np.zeros(self.XH.shape[0]), self.hyp, self.Xs)[1]


KS = (8, 3, 12)   # appends: KA = 8, a partial group, KA = 16


@dataclass(frozen=True)
class Case:
    name: str
    nx: int
    ny: int
    order: str = "x_outer"
    n0: int = 200
    xrev: bool = False
    yrev: bool = False
    warp: float | None = None
    ylo: float = 0.0
    yhi: float = 1.0
    kind: str = "cells"
    shift: int | None = None      # coordinate along which rows leave the grid
    seed: int = field(default=0, compare=False)

    def grid(self):
        gx = axis(self.nx, 0.0, 1.0, self.xrev, self.warp)
        gy = axis(self.ny, self.ylo, self.yhi, self.yrev)
        return make_grid(gx, gy, self.order)

    def data(self, mf, ks=KS):
        """(Xs, X, y, NL): n0 + sum(ks) rows, the first NL of them lofi (MF)."""
        Xs = self.grid()
        n = self.n0 + sum(ks)
        X, y, _ = make_data(Xs, n, 1000 + self.seed + (500 if mf else 0), self.kind)
        if self.shift is not None:
            # off the grid along one coordinate only: lofi rows, hifi rows, new rows
            rows = np.r_[3:9, self.n0 - 5:self.n0, self.n0 + 2:self.n0 + 6, n - 4:n]
            shift_rows(Xs, X, rows, self.shift)
        return Xs, X, y, (int(0.4 * self.n0) if mf else 0)


def _shape(nx, ny, order="x_outer", **kw):
    tag = f"{nx}x{ny}" + ("_yo" if order == "y_outer" else "")
    return Case(tag, nx, ny, order, **kw)


# 1. shapes (single model, SF and MF). tabw: 64 up to 64, 128, 192 (24 x 130: three
# y-tiles; 130 x 24: one), 256 with zq = 2; M = 63 is less than one tile
SHAPES = [
    _shape(16, 128, seed=1), _shape(128, 16, seed=2),       # the headline's 8-rank slice, its transpose
    _shape(26, 51, seed=3), _shape(25, 51, seed=4),         # the reference grid's 2-rank slices
    _shape(40, 33, seed=5), _shape(33, 40, seed=6),         # ragged against 16 and 64 both ways
    _shape(24, 130, seed=7), _shape(130, 24, seed=8),       # tabw 192
    _shape(256, 8, seed=9), _shape(8, 256, seed=10),        # tabw 256, zq = 2, one short axis
    _shape(9, 7, n0=60, kind="revisit", seed=11),           # M = 63 < n0: rows revisit cells
    _shape(40, 1, n0=30, kind="revisit", seed=12),          # a degenerate axis
    _shape(1, 40, n0=30, kind="revisit", seed=13),
    _shape(40, 33, "y_outer", seed=14), _shape(16, 128, "y_outer", seed=15), _shape(24, 130, "y_outer", seed=16),
]
# (the cases whose hand-offs were settled by reading before their first run: their own group)
SPECIAL = {"24x130", "130x24", "24x130_yo", "40x1", "1x40"}

# 2. axes on (40, 33): x increasing / reversed, y in [-0.5, 0.7] increasing / reversed,
# x uniform / warped (exponents 1.5 and 2.2)
AXES = [
    Case(f"x{'r' if xr else 'i'}_y{'r' if yr else 'i'}_{'w%g' % wp if wp else 'u'}", 40, 33, n0=200,
         xrev=xr, yrev=yr, warp=wp, ylo=-0.5, yhi=0.7, seed=20 + i)
    for i, (xr, yr, wp) in enumerate((xr, yr, wp) for xr in (False, True) for yr in (False, True)
                                     for wp in (None, 1.5, 2.2))
]
# ... and rows off the grid along x only, then along y only (the lookup's half hits)
SHIFTED = [
    Case("shift_x", 40, 33, ylo=-0.5, yhi=0.7, shift=0, seed=40),
    Case("shift_y", 40, 33, ylo=-0.5, yhi=0.7, shift=1, seed=41),
    Case("shift_x_yo", 40, 33, "y_outer", ylo=-0.5, yhi=0.7, shift=0, seed=42),
    Case("shift_y_yo", 40, 33, "y_outer", ylo=-0.5, yhi=0.7, shift=1, seed=43),
]

# an axis longer than the Z unit's thread count (tabw = 320 > 256): the host declines
# the lattice step, the V stream serves the grid
DECLINED = [_shape(257, 8, seed=50), _shape(8, 257, seed=51)]

ALL_CASES = SHAPES + AXES + SHIFTED + DECLINED
