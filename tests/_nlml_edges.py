"""The NLML block-edge cases shared by tests/golden/make_nlml_edges_golden.py and the
tests that read tests/golden/nlml_edges_reference.npz (test infrastructure).

mfgp_nlml.hip works in 64 x 64 tiles. The cases put N, and the lofi / hifi split NL,
on, just before and just after a tile edge, at the smallest sizes that reach one tile,
two and three tile rows (the off-diagonal tiles of k_kinv and k_nlml_grad, k_trinv's
chain over K with a ragged last block) and a single fidelity (NL = 0 or NH = 0).
"""
import numpy as np

EPS64 = 2.22e-16
HEADROOM = 16.0

SF_N = (1, 2, 63, 64, 65, 127, 128, 129, 193)
MF_N_NL = ((1, 0), (1, 1), (2, 1), (64, 0), (64, 64), (65, 64), (129, 63), (129, 64), (129, 65),
           (130, 1), (130, 129), (193, 128))
ILL_N = (65, 129)                       # anti_two_corners_sf: the trained, ill-conditioned point
PERTURBED = ("mf", 129, 64, "australia9_mf")   # hyp + 0.05 N(0, 1) (seed 129), jitter 1e-6


def _cases():
    out = []
    for n in SF_N:
        out.append((f"sf_australia3_sf_n{n}", "sf", n, 0, "australia3_sf", False))
    for key in ("australia9_mf", "australia8_mf"):
        for n, nl in MF_N_NL:
            out.append((f"mf_{key}_n{n}_nl{nl}", "mf", n, nl, key, False))
    for n in ILL_N:
        out.append((f"sf_anti_two_corners_sf_n{n}", "sf", n, 0, "anti_two_corners_sf", False))
    kind, n, nl, key = PERTURBED
    out.append((f"{kind}_{key}_n{n}_nl{nl}_perturbed", kind, n, nl, key, True))
    return out


# (name, kind, N, NL, key of synthetic.HYP, perturbed)
CASES = _cases()
NAMES = [c[0] for c in CASES]


def case_inputs(fx, name):
    """(XL, yL, XH, yH, hyp, jitter) of a fixture case."""
    return tuple(fx[f"{name}_{k}"] for k in ("XL", "yL", "XH", "yH", "hyp")) + (float(fx[f"{name}_jitter"]),)


def oracle_kwargs(XL, yL, hyp):
    return {} if hyp.shape[0] == 4 else {"XL": XL, "yL": yL}


def errors(v, g, v_ref, g_ref):
    """(value error, gradient error) in the metrics of tests/test_gpu_nlml.py:
    |v - v_ref| / max(|v_ref|, 1) and max_p |g_p - g_ref_p| / max(|g_ref_p|, 1)."""
    ev = abs(v - v_ref) / max(abs(v_ref), 1.0)
    eg = np.max(np.abs(g - g_ref) / np.maximum(np.abs(g_ref), 1.0))
    return float(ev), float(eg)


def bounds(fx, name):
    """(value bound, gradient bound) = 16 * max(e_oracle, eps64 * cond * max(N, 64)):
    a margin over the fp64 oracle's own error against the extended-precision values, with
    the n * eps * cond(K) scale of a solve as the floor (the floor on N covers the
    tile-deep sums at tiny N). Never derived from the code under test."""
    n = fx[f"{name}_XL"].shape[0] + fx[f"{name}_XH"].shape[0]
    floor = EPS64 * float(fx[f"{name}_cond"]) * max(n, 64)
    return (HEADROOM * max(float(fx[f"{name}_e_oracle_val"]), floor),
            HEADROOM * max(float(fx[f"{name}_e_oracle_grad"]), floor))
