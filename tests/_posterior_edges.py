"""The posterior tile-edge cases shared by tests/golden/make_posterior_edges_golden.py and
the tests that read tests/golden/posterior_edges_reference.npz (test infrastructure).

The routes to the posterior work in 64-row factor blocks, 128-row producer chunks (and the
padded row stride of V) along N, and in 64-cell tiles, 128-cell workgroups and 32-cell wave
groups along M. The cases are the smallest shapes that put N, the lofi / hifi split NL and
M on, just before and just after those edges. Training points are distinct grid cells (an
append then takes L21 from the resident V); the off-grid case ends in 9 random points of
the box (the fallback forward solve, virtual rows of the lattice step). Every case is
carried across its edge in stages: N - 9 rows, an 8-row append, a 1-row append.
"""
import numpy as np

EPS64 = 2.22e-16
HEADROOM = 16.0
TAIL = 9                                 # rows of the off-grid tail, and N minus the first stage

SF_N_GRID = ((1, 9, 7), (63, 8, 8), (64, 13, 5), (65, 13, 11), (128, 43, 3), (129, 13, 11), (193, 15, 13))
MF_N_NL_GRID = ((64, 0, 8, 8), (65, 64, 13, 5), (129, 63, 13, 11), (129, 64, 43, 3), (129, 65, 16, 9),
                (193, 128, 15, 13))
ILL_N_GRID = ((65, 13, 5), (129, 13, 11))          # anti_two_corners_sf: cond 1e7 and up
OFFGRID = (129, 13, 11)                            # australia3_sf, the last TAIL rows off the grid
GRIDS = ((9, 7), (8, 8), (13, 5), (13, 11), (43, 3), (16, 9), (15, 13))    # M = 63 64 65 143 129 144 195


def _cases():
    out = []
    for n, nx, ny in SF_N_GRID:
        out.append((f"sf_australia3_sf_n{n}_{nx}x{ny}", "sf", "australia3_sf", n, 0, nx, ny, False))
    for key in ("australia8_mf", "australia9_mf"):
        for n, nl, nx, ny in MF_N_NL_GRID:
            out.append((f"mf_{key}_n{n}_nl{nl}_{nx}x{ny}", "mf", key, n, nl, nx, ny, False))
    for n, nx, ny in ILL_N_GRID:
        out.append((f"sf_anti_two_corners_sf_n{n}_{nx}x{ny}", "sf", "anti_two_corners_sf", n, 0, nx, ny, False))
    n, nx, ny = OFFGRID
    out.append((f"sf_australia3_sf_n{n}_{nx}x{ny}_offgrid", "sf", "australia3_sf", n, 0, nx, ny, True))
    return out


# (name, kind, key of synthetic.HYP, N, NL, nx, ny, off-grid tail)
CASES = _cases()
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
INPUT_KEYS = ("XL", "yL", "XH", "yH", "hyp", "jitter", "Xs")
STAGE_KEYS = ("mu", "var", "kss", "cond", "e_oracle_mu", "e_oracle_var")


def stages(n, nl):
    """The row counts a case is checked at: N - 9 (not below NL), N - 1, N."""
    return sorted({max(nl, n - TAIL), max(nl, n - 1), n})


def case_stages(name):
    _, _, _, n, nl, _, _, _ = BY_NAME[name]
    return stages(n, nl)


STAGE_IDS = [(name, s) for name in NAMES for s in case_stages(name)]


def make_grid(nx, ny):
    """The [nx ny, 2] cells of linspace(0, 1, nx) x linspace(0, 1, ny), x constant along runs
    of ny cells (the reference's order)."""
    gx, gy = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
    return np.array([(a, b) for a in gx for b in gy], dtype=np.float64).reshape(-1, 2)


def make_inputs(n, nl, nx, ny, offgrid):
    """(Xs, X [n, 2], y [n]): n distinct cells of the grid in a random order (the first nl
    of them are the lofi rows) and y as in tests/test_gpu_factor._data, seeded by n; offgrid:
    the last TAIL rows are uniform points of the unit box instead."""
    rng = np.random.default_rng(n)
    Xs = make_grid(nx, ny)
    X = Xs[rng.choice(Xs.shape[0], n, replace=False)].copy()
    if offgrid:
        X[n - TAIL:] = rng.random((TAIL, 2))
    y = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    return Xs, X, y


def case_inputs(fx, name):
    """(XL, yL, XH, yH, hyp, jitter, Xs) of a fixture case: all N rows."""
    XL, yL, XH, yH, hyp, jitter, Xs = (fx[f"{name}_{k}"] for k in INPUT_KEYS)
    return XL, yL, XH, yH, hyp, float(jitter), Xs


def stage_rows(fx, name, s):
    """(XL, yL, XH, yH) of the first s rows of a case (s >= NL: every lofi row is there)."""
    XL, yL, XH, yH = (fx[f"{name}_{k}"] for k in ("XL", "yL", "XH", "yH"))
    nh = s - XL.shape[0]
    assert nh >= 0
    return XL, yL, XH[:nh], yH[:nh]


def stage_ref(fx, name, s):
    """(mu, var, k**) of a stage: the extended values rounded once to float64."""
    return fx[f"{name}_s{s}_mu"], fx[f"{name}_s{s}_var"], float(fx[f"{name}_s{s}_kss"])


def oracle(XL, yL, XH, yH, hyp, Xs, jitter):
    """The fp64 oracle's posterior of these rows (sf_diag / mf_diag)."""
    from oracle import gp_oracle as O
    if hyp.shape[0] == 4:
        return O.sf_diag(XH, yH, hyp, Xs, jitter)
    return O.mf_diag(XL, yL, XH, yH, hyp, Xs, jitter)


def errors(mu, var, mu_ref, var_ref, kss):
    """(e_mu, e_var), norm-wise: max_c |mu_c - mu_ref_c| / max_c |mu_ref_c| and
    max_c |var_c - var_ref_c| / k**."""
    mu, var = np.asarray(mu).reshape(-1), np.asarray(var).reshape(-1)
    e_mu = np.max(np.abs(mu - mu_ref)) / np.max(np.abs(mu_ref))
    e_var = np.max(np.abs(var - var_ref)) / kss
    return float(e_mu), float(e_var)


def bound_of(e_oracle, cond, n):
    """16 * max(e_oracle, eps64 * cond(K) * max(N, 64)); 16 * eps64 at N = 0 (the prior: one
    rounding of a product and a sum of exponentials)."""
    if n == 0:
        return HEADROOM * EPS64
    return HEADROOM * max(float(e_oracle), EPS64 * float(cond) * max(n, 64))


def bounds(fx, name, s):
    """(mu bound, var bound) of a stage: a margin over the fp64 oracle's own error against the
    extended-precision values, with the n * eps * cond(K) scale of a solve as the floor (the
    floor on N covers the tile-deep sums at tiny N). Never derived from the code under test."""
    cond = fx[f"{name}_s{s}_cond"]
    return (bound_of(fx[f"{name}_s{s}_e_oracle_mu"], cond, s), bound_of(fx[f"{name}_s{s}_e_oracle_var"], cond, s))
