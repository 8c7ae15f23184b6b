"""Time the integrated-variance-reduction call (mfgp_var_reduction: k_ivr_partial,
k_ivr_finish, k_ivr_best) on three cases, all MF:

  head4096  the headline's 128 x 128 grid (M = 16384), N = 2048, C = 4096 contiguous
            candidates (cells 0..4095), nw = 1 and nw = 8
  headall   the same model, all cells: C = M = 16384, nw = 1
  ref51     the reference's own 51 x 51 grid (M = 2601), N = 300, all cells, nw = 1

Per case: host wall time per call (the call synchronises; device weights and device
output), the median of --reps calls after a warm-up, and 2 M C N flop over it.

--route cov times what the engine offered before this call existed, on head4096 only:
mfgp_cov_block of the M x C block into device memory (512 MB) followed by a torch reduction
(square in place, then W @ block, divided by the denominators) -- it uses nothing of the
fused call, so the same file runs on a checkout without it. Its scores are compared with
the fused ones where both exist.

The kernel times come from a kernel trace of this script in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o ivr -- python3 tools/bench_ivr.py --trace

(--trace: per case, in the order above, `reps` + 1 calls and nothing else of these kernels;
--trace-summary CSV groups a kernel-trace CSV that way and prints the medians, the first
dispatch of each group dropped). Prints one JSON line and, with --out, writes it to that file.
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

KERNELS = ("k_ivr_partial", "k_ivr_finish", "k_ivr_best")
GROUPS = ("head4096_nw1", "head4096_nw8", "headall_nw1", "ref51_nw1")


def make(G, N, NL, seed):
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
    _, var = m.predict()
    return m, hyp, Xs.shape[0], var, rng


def med_us(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t)), 1e6 * float(np.min(t)), 1e6 * float(np.max(t))


def weights(rng, M, nw):
    import torch
    w = rng.random((nw, M)) + 0.05
    return w, torch.from_numpy(w).cuda()


def fused_case(m, M, N, cand, nw, rng, reps, trace):
    import torch
    C = M if cand is None else len(cand)
    _, wd = weights(rng, M, nw)
    out = torch.empty((nw, C), dtype=torch.float64, device="cuda")
    res = {"M": M, "C": C, "N": N, "nw": nw, "reps": reps, "flop": 2.0 * M * C * N}
    if trace:
        for _ in range(reps + 1):
            m.var_reduction(cand, wd, out=out)
        return res
    med, lo, hi = med_us(lambda: m.var_reduction(cand, wd, out=out, with_best=True), reps)
    res.update(wall_us=med, wall_us_min=lo, wall_us_max=hi, wall_tflops=res["flop"] / med / 1e6)
    return res


def cov_route(m, hyp, M, N, var, cand, nw, rng, reps):
    """cov_block into device memory + a torch reduction, and its scores."""
    import torch
    C = len(cand)
    _, wd = weights(rng, M, nw)
    buf = torch.empty((M, C), dtype=torch.float64, device="cuda")
    d = torch.from_numpy(var[cand] + np.exp(hyp[-1]) + 1e-8).cuda()
    out = []

    def run():
        m.cov_block(None, cand, out=buf.data_ptr())
        s = torch.matmul(wd, buf.square_()) / d
        torch.cuda.synchronize()
        out[:] = [s]
    med, lo, hi = med_us(run, reps)

    def block_only():
        m.cov_block(None, cand, out=buf.data_ptr())
    bmed, _, _ = med_us(block_only, reps)
    res = {"M": M, "C": C, "N": N, "nw": nw, "reps": reps, "wall_us": med, "wall_us_min": lo, "wall_us_max": hi,
           "cov_block_us": bmed, "block_bytes": 8 * M * C}
    if hasattr(m, "var_reduction"):
        f = torch.empty((nw, C), dtype=torch.float64, device="cuda")
        m.var_reduction(cand, wd, out=f)
        s = out[0]
        res["max_rel_diff_vs_fused"] = float(((f - s).abs() / s.abs()).max())
    return res


def trace_summary(path, reps):
    """Median dispatch durations (us) per kernel and group from a kernel-trace CSV of a
    --trace run: per kernel the dispatches in start order are the groups' `reps` + 1 each."""
    rows = {k: [] for k in KERNELS}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name", "")
            for k in KERNELS:
                if k + "(" in name:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    out = {}
    n = reps + 1
    for k, v in rows.items():
        v.sort()
        if not v:       # (k_ivr_best runs only when the maxima are asked for: not in --trace)
            continue
        assert len(v) == len(GROUPS) * n, (k, len(v))
        for i, tag in enumerate(GROUPS):
            out.setdefault(tag, {})[k + "_us"] = float(np.median([d for _, d in v[i * n + 1:(i + 1) * n]])) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route", choices=("fused", "cov"), default="fused")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-summary", metavar="CSV", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_summary:
        res = trace_summary(args.trace_summary, args.reps)
    elif args.route == "cov":
        m, hyp, M, var, rng = make(128, 2048, 1024, seed=2)
        cand = list(range(4096))
        res = {"head4096_nw1": cov_route(m, hyp, M, 2048, var, cand, 1, rng, args.reps),
               "head4096_nw8": cov_route(m, hyp, M, 2048, var, cand, 8, rng, args.reps)}
    else:
        res = {}
        m, hyp, M, var, rng = make(128, 2048, 1024, seed=2)
        cand = list(range(4096))
        res["head4096_nw1"] = fused_case(m, M, 2048, cand, 1, rng, args.reps, args.trace)
        res["head4096_nw8"] = fused_case(m, M, 2048, cand, 8, rng, args.reps, args.trace)
        res["headall_nw1"] = fused_case(m, M, 2048, None, 1, rng, args.reps, args.trace)
        del m
        m, hyp, M, var, rng = make(51, 300, 100, seed=1)
        res["ref51_nw1"] = fused_case(m, M, 300, None, 1, rng, args.reps, args.trace)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
