"""Time the pathwise sampler (mfgp_sample_posterior: k_sample_t, k_sample_field,
k_sample_resid, k_sample_solve, k_sample_gemm) on two cases:

  ref    the reference's size: 51 x 51 grid, N_L = 100, N_H = 200
  head   the headline's size: 128 x 128 grid, N_L = 1024, N_H = 1024

Per case, host wall time per call (every call synchronises), medians over --reps, with
host normals and host output:
  s1_us / s64_us        S = 1 / S = 64 posterior samples
  s64_dev_us            S = 64 with device normals and device output
  prior64_us            S = 64 prior samples (no solve, no GEMM)
  dense2_us (ref only)  the parent's only way: draw_posterior_samples(X, 2) through the
                        dense covariance and numpy's multivariate_normal, alternating with
                        sample_posterior(X, 2) (pathwise2_us) in one loop
The kernel times come from a kernel trace of this script in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o sample -- python3 tools/bench_sample.py --trace

(--trace: per case, ref first, `reps` + 1 calls of S = 1, then `reps` + 1 of S = 64 and
nothing else of the sampler: the durations per case and S follow from the dispatch
order; --trace-summary CSV groups a kernel-trace CSV that way and prints the medians).
Prints one JSON line and, with --out, writes it to that file.
"""
import argparse
import csv
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_sample_t", "k_sample_field", "k_sample_resid", "k_sample_solve", "k_sample_gemm")


def make(G, NL, NH, seed):
    from mfgp_coverage_amd.gaussian_process import MFGP
    from mfgp_coverage_amd.synthetic import HYP
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, G)
    Xs = np.array([(a, b) for a in g for b in g])
    X = Xs[rng.choice(Xs.shape[0], NL + NH, replace=False)].copy()
    y = (np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(NL + NH))[:, None]
    mf = MFGP(X[:NL], y[:NL], X[NL:], y[NL:], 1, 1)
    mf.hyp = HYP["australia8_mf"].copy()
    mf.updt_info(mf.X_L, mf.y_L, mf.X_H, mf.y_H)
    mf.predict(Xs)
    return mf, Xs, rng


def med_us(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def case(G, NL, NH, reps, trace, dense, seed):
    mf, Xs, rng = make(G, NL, NH, seed)
    m = mf._dev()
    d = m.sample_dims()
    nz, M, N = d["nz"], d["M"], d["N"]
    res = {"grid": G, "NL": NL, "NH": NH, "reps": reps, "dims": d}
    Z1, Z64 = rng.standard_normal((1, nz)), rng.standard_normal((64, nz))
    o1, o64 = np.empty((1, M)), np.empty((64, M))
    if trace:
        for _ in range(reps + 1):
            m.sample(Z1, out=o1)
        for _ in range(reps + 1):
            m.sample(Z64, out=o64)
        return res
    res["s1_us"] = med_us(lambda: m.sample(Z1, out=o1), reps)
    res["s64_us"] = med_us(lambda: m.sample(Z64, out=o64), reps)
    import torch
    zt = torch.from_numpy(Z64).cuda()
    ot = torch.empty((64, M), dtype=torch.float64, device="cuda")
    res["s64_dev_us"] = med_us(lambda: m.sample(zt.data_ptr(), out=ot.data_ptr(), S=64, ldz=nz, ldo=M), reps)
    assert np.array_equal(ot.cpu().numpy(), o64)
    nzp = m.sample_dims(prior=True)["nz"]
    Zp = np.ascontiguousarray(Z64[:, :nzp])
    res["prior64_us"] = med_us(lambda: m.sample(Zp, prior=True, out=o64), reps)
    # one pass over V per 64 samples, and the GEMM's flops
    res["v_bytes"] = 8 * N * 64 * ((M + 63) // 64)
    res["gemm_flop_s64"] = 2.0 * 64 * N * M
    if dense:
        g2 = np.random.default_rng(0)
        td, tp = [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mf.draw_posterior_samples(Xs, 2)
            mf.sample_posterior(Xs, 2, rng=g2)
            for _ in range(reps):
                t0 = time.perf_counter()
                mf.sample_posterior(Xs, 2, rng=g2)
                t1 = time.perf_counter()
                mf.draw_posterior_samples(Xs, 2)
                t2 = time.perf_counter()
                tp.append(t1 - t0)
                td.append(t2 - t1)
        res["pathwise2_us"] = 1e6 * float(np.median(tp))
        res["dense2_us"] = 1e6 * float(np.median(td))
    return res


def trace_summary(path, reps):
    """Median dispatch durations (us) per kernel, case and S from a rocprofv3 kernel-trace
    CSV of a --trace run: per kernel the dispatches in start order are ref S = 1, ref
    S = 64, head S = 1, head S = 64, `reps` + 1 each (the first of each group dropped)."""
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
        assert len(v) == 4 * n, (k, len(v))
        for i, tag in enumerate(("ref_s1", "ref_s64", "head_s1", "head_s64")):
            out.setdefault(tag, {})[k + "_us"] = float(np.median([d for _, d in v[i * n + 1:(i + 1) * n]])) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-summary", metavar="CSV", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_summary:
        res = trace_summary(args.trace_summary, args.reps)
    else:
        res = {"ref": case(51, 100, 200, args.reps, args.trace, True, seed=1),
               "head": case(128, 1024, 1024, args.reps, args.trace, False, seed=2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
