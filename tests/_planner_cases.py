"""Failing compute_sample_points cases (test infrastructure; plain NumPy, no GPU).

The planners' loop (simulator.py:344-370) appends the cell of maximal posterior
variance until that maximum is at or below the threshold. A step of it is a 1-row
bordered append whose pivot (Schur complement) is

    k(x, x) + noise + jitter - psi K^-1 psi^T  =  vmax + noise + jitter,

vmax being the current largest posterior variance. With

    jitter = -(noise + d * kss)          (noise_H for MF, kss the prior variance)

the matrix carries an effective nugget of -d * kss: the model's own well-separated
rows stay positive definite, every pivot is vmax - d * kss, and with threshold 0 the
pivot has to cross zero before the loop could stop. The failure is therefore
certain. WHERE it happens is not independent of how near ties between cells of
(almost) equal variance are broken: a near tie does not change vmax at the step
where it occurs, but the other cell is then taken a step later and the path may
differ from there on. ``oracle_loop(..., tie=...)`` replays the loop with other
tie-breaks; the CPU test shows that cases A and C fail at the same step under all
of them, and that case B (near ties from its first step on: top-two gap 5e-10 kss)
moves by a few steps but stays inside the second chunk, before its last iteration.
The GPU tests therefore assert the exact failing row for A and C and that range for B.

Under the negative nugget the posterior variance changes sign near the rows. The
fp32 mode's variance metric (oracle.parity_errors_f32) is relative to |var_ref|, and
the fp32 V carries an absolute variance error of about 2 * 2^-24 * kss, so that metric
means what it means for a positive definite model only while no cell's variance lies
near zero: F32_TOL = 1e-4 needs |var_ref| >= 1.2e-3 kss, and the cases keep every cell
at least 1e-2 kss from zero after the step the GPU tests check against the oracle.
The smooth australia3 / australia8 length scales (6 and 17 grid cells) cannot: some
cell of their variance surface always lies within ~1e-3 kss of zero (rounding the
oracle's own V to fp32 then already misses F32_TOL, 7e-4). Cases A and C therefore
shorten the length scale to 2.8 and 4 cells (log -2.15 and -1.8) and take a larger d.

``build(name)`` returns a Case: grid, rows, hyp, jitter, and -- from the CPU oracle
run in the reference's loop -- the pivot sequence and ``i_fail``, the (0-based) step
whose append np.linalg.cholesky rejects. tests/test_planner_failure_cases.py
asserts the margins on the oracle alone before any GPU test relies on them.
"""
from dataclasses import dataclass, field

import numpy as np

from oracle import gp_oracle as O

HYP_SF = np.array([0.001, -2.368468757, -1.353149618, -4.596652374])        # australia3_sf_hyp.csv
HYP_MF = np.array([-1.700903132, -1.947362545, -0.309197345, -14.9598621, -3.655273338,
                   -1.317607182, -0.721748367, -5.926942955, -1.371689752])  # australia8_mf_hyp.csv
G = 24
MAX_ITERS = 200


def grid(g=G):
    a = np.linspace(0.0, 1.0, g)
    return np.array([(p, q) for p in a for q in a])


def cells(ij, g=G):
    """Grid points of the (i, j) index pairs."""
    a = np.linspace(0.0, 1.0, g)
    return np.array([(a[i], a[j]) for i, j in ij])


def initial_cells(g=G):
    """Five asymmetric hifi cells: no two of the grid's symmetries map the set onto itself."""
    return [(1, 2), (3, g - 5), (g - 2, 4), (g - 6, g - 3), (g // 2 + 1, g // 2 - 2)]


def field_values(X):
    """A smooth [0, 1] field (the chosen points do not depend on it; predict's mean does)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    return 0.5 + 0.4 * np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1])


def random_cells(n, seed, g=G, exclude=()):
    """n distinct random cells (index pairs) outside `exclude`."""
    rng = np.random.default_rng(seed)
    taken = set(exclude)
    out = []
    for f in rng.permutation(g * g):
        ij = (int(f) // g, int(f) % g)
        if ij in taken:
            continue
        out.append(ij)
        if len(out) == n:
            break
    return out


@dataclass
class Case:
    name: str
    kind: str            # "sf" | "mf"
    hyp: np.ndarray
    jitter: float
    d: float             # the effective nugget is -d * kss (0: a healthy model)
    xs: np.ndarray       # [G*G, 2]
    XL: np.ndarray
    yL: np.ndarray
    XH: np.ndarray
    yH: np.ndarray
    kss: float = 0.0
    # from the oracle's loop at threshold 0 (failing cases only)
    pivots: np.ndarray = field(default_factory=lambda: np.empty(0))   # pivot of step i, i <= i_fail
    i_fail: int = -1

    def oracle(self, XH=None, yH=None):
        """Posterior (mu, var) on the grid under this case's jitter."""
        XH = self.XH if XH is None else XH
        yH = self.yH if yH is None else yH
        if self.kind == "sf":
            return O.sf_diag(XH, yH, self.hyp, self.xs, jitter=self.jitter)
        return O.mf_diag(self.XL, self.yL, XH, yH, self.hyp, self.xs, jitter=self.jitter)


def oracle_loop(case, threshold, max_iters=MAX_ITERS, tie=None):
    """The reference's loop (sim:339-370) on the oracle: -> (points, vmax per step,
    i_fail). Step i takes the first argmax of the posterior variance given the i points
    before it, with the posterior mean there as its observation; i_fail is the step
    whose append np.linalg.cholesky rejects (-1: the loop reached the threshold, or
    max_iters). tie = (tol, how): among the cells within tol * kss of the maximum take
    the last one (how = "last") or a random one (how = a numpy Generator) -- the
    choices a device whose variances differ by rounding may make."""
    XH, yH = case.XH.copy(), case.yH.copy()
    mu, var = case.oracle(XH, yH)   # (raises if the initial rows are not positive definite)
    pts, vmaxs = [], []
    for i in range(max_iters):
        vmax = float(var.max())
        if not vmax > threshold:
            return np.array(pts).reshape(-1, 2), np.array(vmaxs), -1
        j = int(np.argmax(var))
        if tie is not None:
            near = np.flatnonzero(var >= vmax - tie[0] * case.kss)
            j = int(near[-1]) if isinstance(tie[1], str) else int(tie[1].choice(near))
        pts.append(case.xs[j])
        vmaxs.append(vmax)
        XH = np.vstack([XH, case.xs[j]])
        yH = np.append(yH, mu[j])
        try:
            mu, var = case.oracle(XH, yH)
        except np.linalg.LinAlgError:
            return np.array(pts).reshape(-1, 2), np.array(vmaxs), i
    return np.array(pts).reshape(-1, 2), np.array(vmaxs), -1


def _make(name, kind, hyp, d, hifi_cells, lofi_cells=(), jitter=None, g=G):
    hyp = np.asarray(hyp, dtype=np.float64)
    kss = float(O.prior_variance(hyp))
    if jitter is None:
        jitter = -(float(np.exp(hyp[-1])) + d * kss)
    XH = cells(hifi_cells, g)
    XL = cells(lofi_cells, g) if len(lofi_cells) else np.empty((0, 2))
    c = Case(name, kind, hyp, float(jitter), d, grid(g), XL, field_values(XL) - 0.05, XH, field_values(XH), kss)
    if d > 0:
        _, vmaxs, c.i_fail = oracle_loop(c, 0.0)
        c.pivots = vmaxs - d * kss
    return c


_cache = {}


def build(name):
    """Cases "A", "B", "C" (failing, see the module docstring), "B2" (case B's model
    with five other rows and the normal jitter: healthy), "H0" / "H1" (healthy MF models
    on the same grid), "CAP" (a healthy SF model on a 6 x 6 grid: the point-cap case).
    Built once per process; treat the arrays as read-only."""
    if name in _cache:
        return _cache[name]
    init = initial_cells()
    if name == "A":
        h = HYP_SF.copy()
        h[2] = -2.15
        c = _make("A", "sf", h, 0.6, init)
    elif name == "B":
        h = HYP_SF.copy()
        h[2] = -2.3
        c = _make("B", "sf", h, 0.2, init)
    elif name == "B2":
        h = HYP_SF.copy()
        h[2] = -2.3
        c = _make("B2", "sf", h, 0.0, random_cells(5, seed=11), jitter=1e-8)
    elif name == "C":
        h = HYP_MF.copy()
        h[7] = 0.0   # noise_lo = 1: the negative jitter lands on the lofi block too
        h[2] = h[5] = -1.8
        c = _make("C", "mf", h, 0.3, init, random_cells(30, seed=7, exclude=init))
    elif name == "CAP":
        c = _make("CAP", "sf", HYP_SF, 0.0, initial_cells(6), jitter=1e-8, g=6)
    elif name in ("H0", "H1"):
        s = int(name[1])
        hc = random_cells(12 + 9 * s, seed=20 + s)
        c = _make(name, "mf", HYP_MF, 0.0, hc, random_cells(40 - 12 * s, seed=30 + s, exclude=hc), jitter=1e-8)
    else:
        raise KeyError(name)
    _cache[name] = c
    return c


def append_rows(case, n):
    """n on-grid rows (X [n, 2], y [n]) for an append that stays positive definite under
    the case's jitter: the oracle loop's first n cells, each the cell of largest
    posterior variance given the ones before it, hence far from every existing row;
    their pivots are the loop's first n (the CPU test asserts their margin)."""
    healthy = case.d == 0
    pts, vmaxs, _ = oracle_loop(case, 0.0, n)
    assert pts.shape[0] == n
    if not healthy:
        assert case.i_fail > n
    return pts.copy(), field_values(pts) + 0.02
