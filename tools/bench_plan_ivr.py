"""Time the greedy integrated-variance planner through its single entry (mfgp_plan_ivr: the
batch of one of the loop behind mfgp_batch_plan_ivr, so per pick k_ivr_pick_batch, the one-row
batch step and the _batch forms of k_plan_x, k_cov_dot, k_cov_psum, k_kss_t / k_kss_out and
k_cov_apply; KERNELS' substrings match either form) on the headline case: the 128 x 128 grid
(M = 16384), N = 2048 MF, 64 picks, all cells allowed.

--route new (default): Model.plan_ivr(64), host wall time per call (the call synchronises),
the median of --reps calls after a warm-up; also one cov_apply of a single vector.

--route parent: the same selection using only what the engine offered before this call
existed -- var_reduction over all cells with its fused argmax, a one-row hifi append of the
chosen cell with its posterior mean, predict, and truncate at the end -- so the same file
runs on a checkout without the planner. Its picks are compared with plan_ivr's where both
exist.

The kernel times come from a kernel trace of this script in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o plan -- python3 tools/bench_plan_ivr.py --trace

(--trace: `reps` + 1 plan_ivr calls and nothing else; --trace-summary CSV prints, per kernel
of the loop, the dispatch count and the median duration, and for the two passes over V the
bytes they stream over that time). Prints one JSON line and, with --out, writes it to that file.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_ivr_pick", "k_plan_x", "k_cov_dot", "k_cov_psum", "k_kss_t", "k_kss_out", "k_cov_apply",
           "k_ivr_partial", "k_inc_stream", "k_inc_lat", "k_lat_gemm2")
G, N, NL, PICKS = 128, 2048, 1024, 64


def make(seed=2):
    from mfgp_coverage_amd import _lib
    from mfgp_coverage_amd.synthetic import HYP
    hyp = HYP["australia8_mf"].copy()
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, G)
    Xs = np.array([(a, b) for a in g for b in g])
    X = Xs[rng.choice(Xs.shape[0], N, replace=False)].copy()
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(N)
    m = _lib.Model(_lib.context(), _lib.MF, hyp, 1e-8)
    m.set_grid(Xs)
    m.set_data(X[:NL], y[:NL], X[NL:], y[NL:])
    m.predict()
    return m, Xs


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t)), 1e6 * float(np.min(t)), 1e6 * float(np.max(t))


def parent_route(m, Xs, picks):
    """score all cells, take the argmax, append it with its posterior mean, predict; truncate
    at the end -> (cells, gains)."""
    nh0 = N - NL
    cells, gains = [], []
    mu, _ = m.predict()
    for _ in range(picks):
        _, best, pos = m.var_reduction(with_best=True)
        cells.append(pos)
        gains.append(float(best))
        m.append(Xs[pos:pos + 1], mu[pos:pos + 1])
        mu, _ = m.predict()
    m.truncate(nh0)
    m.predict()
    return np.asarray(cells), np.asarray(gains)


def trace_summary(path, reps):
    rows = {k: [] for k in KERNELS}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name", "")
            for k in KERNELS:
                if k in name:
                    rows[k].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                    break
    out = {}
    for k, v in rows.items():
        if v:
            out[k] = {"dispatches": len(v), "median_us": float(np.median(v)) / 1e3}
    # bytes per pass: the M x (N + t) doubles of V, at the run's mean row count
    rows_mean = N + (PICKS - 1) / 2.0
    vbytes = 8.0 * G * G * rows_mean
    for k in ("k_cov_dot", "k_cov_apply"):
        if k in out:
            out[k]["v_bytes"] = vbytes
            out[k]["tb_per_s"] = vbytes / (out[k]["median_us"] * 1e-6) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route", choices=("new", "parent"), default="new")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-summary", metavar="CSV", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_summary:
        res = trace_summary(args.trace_summary, args.reps)
    else:
        m, Xs = make()
        res = {"M": G * G, "N": N, "picks": PICKS, "reps": args.reps, "route": args.route}
        if args.trace:
            for _ in range(args.reps + 1):
                m.plan_ivr(PICKS)
        elif args.route == "parent":
            got = []
            med, lo, hi = timed(lambda: got.__setitem__(slice(None), [parent_route(m, Xs, PICKS)]), args.reps)
            res.update(wall_us=med, wall_us_min=lo, wall_us_max=hi, per_pick_us=med / PICKS)
            if hasattr(m, "plan_ivr"):
                cells, _, gains = m.plan_ivr(PICKS)
                pc, pg = got[0]
                res["same_cells"] = int(np.sum(cells == pc))
                res["max_rel_gain_diff"] = float(np.max(np.abs(gains - pg) / np.abs(pg)))
        else:
            med, lo, hi = timed(lambda: m.plan_ivr(PICKS), args.reps)
            res.update(wall_us=med, wall_us_min=lo, wall_us_max=hi, per_pick_us=med / PICKS)
            r1, _, _ = timed(lambda: m.plan_ivr(1), args.reps)
            res["one_pick_call_us"] = r1                    # the call's fixed part: the GEMM of S_0
            res["per_pick_after_first_us"] = (med - r1) / (PICKS - 1)
            x = np.random.default_rng(3).standard_normal(G * G)
            import torch
            xd = torch.from_numpy(x).cuda()
            od = torch.empty_like(xd)
            res["cov_apply_us"] = timed(lambda: m.cov_apply(xd, out=od), args.reps)[0]
            res["planner_stats"] = m.ctx.planner_stats()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
