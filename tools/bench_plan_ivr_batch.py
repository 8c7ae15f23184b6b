"""Time the batched greedy integrated-variance planner (mfgp_batch_plan_ivr: k_ivr_pick_batch,
the batched one-row step, k_plan_x_batch, k_cov_dot_batch, k_cov_psum_batch, k_kss_t_batch /
k_kss_out_batch, k_cov_apply_batch) on the headline batch: B = 8 models on the 128 x 128 grid
(M = 16384), N = 2048 MF each (tools/bench_plan_ivr.py's model under eight seeds), 64 picks,
all cells allowed, weights ones.

--route batch (default): _lib.batch_plan_ivr(models, 64), host wall time per call (the call
synchronises), every timed call listed, after a warm-up call.
--route loop: the loop of B Model.plan_ivr(64) calls, one model after another -- the baseline,
which uses nothing this tool's commit added, so the same file runs on a checkout of its parent.

Both routes then time the candidate-list shape: 1024 candidates (every 16th cell), 8 picks,
and the call's fixed part (a call of one pick: the numerators' GEMM over the list).

The kernel times come from a kernel trace of this script in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o plan -- python3 tools/bench_plan_ivr_batch.py --trace

(--trace: `reps` + 1 batched calls and nothing else; --trace-summary CSV prints, per kernel of
the loop, the dispatch count and the median duration, and for the two passes over V the bytes
all members stream over that time). Prints one JSON line and, with --out, writes it to that file.
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

KERNELS = ("k_ivr_pick_batch", "k_plan_x_batch", "k_cov_dot_batch", "k_cov_psum_batch", "k_kss_t_batch",
           "k_kss_out_batch", "k_cov_apply_batch", "k_ivr_partial", "k_plan_scatter", "k_inc_stream", "k_inc_lat",
           "k_lat_gemm2", "k_vstream")
G, N, NL, PICKS, B = 128, 2048, 1024, 64, 8
LIST_STRIDE, LIST_PICKS = 16, 8


def make(seed):
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
    return m


def timed(f, reps):
    """Every timed call's wall time in microseconds, after one warm-up call."""
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(1e6 * (time.perf_counter() - t0))
    return t


def stats(t):
    return {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)),
            "runs_us": [float(v) for v in t]}


def trace_summary(path):
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
    # bytes per pass: the M x (N + t) doubles of every member's V, at the run's mean row count
    vbytes = 8.0 * G * G * (N + (PICKS - 1) / 2.0) * B
    for k in ("k_cov_dot_batch", "k_cov_apply_batch"):
        if k in out:
            out[k]["v_bytes"] = vbytes
            out[k]["tb_per_s"] = vbytes / (out[k]["median_us"] * 1e-6) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--route", choices=("batch", "loop"), default="batch")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-summary", metavar="CSV", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_summary:
        res = trace_summary(args.trace_summary)
    else:
        from mfgp_coverage_amd import _lib
        ms = [make(2 + b) for b in range(B)]
        cand = np.arange(0, G * G, LIST_STRIDE)
        res = {"B": B, "M": G * G, "N": N, "picks": PICKS, "reps": args.reps, "route": args.route,
               "list": {"candidates": int(cand.shape[0]), "picks": LIST_PICKS}}
        if args.route == "batch":
            def run(n, c=None):
                return _lib.batch_plan_ivr(ms, n, cand=c)
        else:
            def run(n, c=None):
                return [m.plan_ivr(n, cand=c) for m in ms]
        if args.trace:
            for _ in range(args.reps + 1):
                run(PICKS)
        else:
            head = timed(lambda: run(PICKS), args.reps)
            res["headline"] = stats(head)
            res["headline"]["per_round_us"] = float(np.median(head)) / PICKS
            one = timed(lambda: run(1), args.reps)
            res["headline"]["one_pick_call"] = stats(one)                 # the fixed part: B GEMMs of S_0
            res["headline"]["per_round_after_first_us"] = (float(np.median(head)) - float(np.median(one))) / (PICKS - 1)
            res["list"]["call"] = stats(timed(lambda: run(LIST_PICKS, cand), args.reps))
            res["list"]["one_pick_call"] = stats(timed(lambda: run(1, cand), args.reps))
            res["planner_stats"] = ms[0].ctx.planner_stats()
            r = run(4)
            res["first_cells"] = [[int(v) for v in x[0]] for x in r]      # (both routes: the same picks)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
