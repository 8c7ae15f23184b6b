"""Time k_cov_block (mfgp_cov_block into device memory) on its two yardstick cases:

  ref51     the reference's own 51 x 51 grid, all cells (2601 x 2601), MF, N = 300
  head4096  a 4096 x 4096 block (cells 0..4095 twice) of the headline's 128 x 128
            grid, MF, N = 2048

Per case: `--reps` calls after a warm-up, host wall time per call (the call
synchronises), and 2 a b N flop over it. The kernel time itself comes from a
kernel trace of this script in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o cov -- python3 tools/bench_cov.py

(then `k_cov_block`'s mean duration per case: the cases' launches are the first and
the last `reps + 1` dispatches of the kernel). --oracle also times
O.mf_faithful(return_cov=True) for the 51 x 51 case on this host's CPU.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid(G):
    g = np.linspace(0.0, 1.0, G)
    return np.array([(a, b) for a in g for b in g])


def make(G, N, NL, seed):
    from mfgp_coverage_amd import _lib
    from mfgp_coverage_amd.synthetic import HYP
    hyp = HYP["australia8_mf"].copy()
    rng = np.random.default_rng(seed)
    Xs = grid(G)
    X = Xs[rng.choice(Xs.shape[0], N, replace=False)].copy()
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(N)
    m = _lib.Model(_lib.context(), _lib.MF, hyp, 1e-8)
    m.set_grid(Xs)
    m.set_data(X[:NL], y[:NL], X[NL:], y[NL:])
    m.predict()
    return m, hyp, Xs, X, y


def time_case(m, rows, cols, a, b, N, reps):
    import torch
    out = torch.empty((a, b), dtype=torch.float64, device="cuda")
    m.cov_block(rows, cols, out=out.data_ptr())          # warm-up (workspace, code object)
    t0 = time.perf_counter()
    for _ in range(reps):
        m.cov_block(rows, cols, out=out.data_ptr())
    dt = (time.perf_counter() - t0) / reps
    return {"a": a, "b": b, "N": N, "reps": reps, "wall_us_per_call": 1e6 * dt,
            "flop": 2.0 * a * b * N, "wall_tflops": 2.0 * a * b * N / dt / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    res = {}
    m, hyp, Xs, X, y = make(51, 300, 100, seed=1)
    res["ref51"] = time_case(m, None, None, Xs.shape[0], Xs.shape[0], 300, args.reps)
    if args.oracle:
        from oracle import gp_oracle as O
        t0 = time.perf_counter()
        _, C = O.mf_faithful(X[:100], y[:100], X[100:], y[100:], hyp, Xs, return_cov=True)
        res["ref51"]["oracle_cpu_s"] = time.perf_counter() - t0
        D = m.cov_block()
        res["ref51"]["err_vs_oracle"] = float(np.max(np.abs(D - C) / np.maximum(np.abs(C), 1e-6 * O.prior_variance(hyp))))
    del m
    m, hyp, Xs, X, y = make(128, 2048, 1024, seed=2)
    idx = list(range(4096))
    res["head4096"] = time_case(m, idx, idx, 4096, 4096, 2048, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
