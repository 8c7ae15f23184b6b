"""Time the look-ahead path (mfgp_query: k_look_border, k_look_query) on two cases:

  ref    the reference's size: N_L = 100, N_H = 200, P = 8 prospective hifi points
  head   the headline's size: N_L = 1024, N_H = 1024, P = 8

Per case, host wall time per call (every call synchronises), medians over --reps:
  border_us          a query of one point with a new prospective set (border + query)
                     minus the same query on the kept border
  query30_us         Q = 30 (one generation of get_max_var) on the kept border
  query4096_us       Q = 4096 on the kept border
  get_max_var_s      MFGP.get_max_var end to end (seeded), with its launches
  parent_gen30_us    the only way without mfgp_query: copy.deepcopy(model) + updt_hifi(the
                     P points) + predict(the 30 points), per generation; alternating with
                     query30 in the same loop
  oracle_point_us    a numpy restatement of the reference's per-point get_neg_var
                     (predict + pred_var: two Cholesky factors of N and N + P rows) from
                     oracle/gp_oracle.py on this host's CPU
The kernel times come from a kernel trace of this script in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o look -- python3 tools/bench_look.py --trace

(--trace: only the border / Q = 30 / Q = 4096 calls, `reps` each per case, ref first:
the mean durations of k_look_border and k_look_query per case and Q follow from the
dispatch order). Prints one JSON line and, with --out, writes it to that file.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(NL, NH, seed):
    from mfgp_coverage_amd.gaussian_process import MFGP
    from mfgp_coverage_amd.synthetic import HYP
    rng = np.random.default_rng(seed)
    X = rng.random((NL + NH, 2))
    y = (np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(NL + NH))[:, None]
    mf = MFGP(X[:NL], y[:NL], X[NL:], y[NL:], 1, 1)
    mf.hyp = HYP["australia8_mf"].copy()
    mf.updt_info(mf.X_L, mf.y_L, mf.X_H, mf.y_H)
    return mf, rng


def med_us(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def case(NL, NH, P, reps, trace, seed):
    from oracle import gp_oracle as O
    mf, rng = make(NL, NH, seed)
    m = mf._dev()
    E2 = np.empty((0, 2))
    sets = [rng.random((P, 2)) for _ in range(2 * reps + 4)]
    x1, x30, x4096 = rng.random((1, 2)), rng.random((30, 2)), rng.random((4096, 2))
    it = iter(sets)
    res = {"NL": NL, "NH": NH, "P": P, "reps": reps}
    new_set = med_us(lambda: m.query(x1, E2, next(it)), reps)
    kept = med_us(lambda: m.query(x1, E2, sets[-1]), reps)
    res["border_us"] = new_set - kept
    res["query1_us"] = kept
    if trace:
        m.query(x30, E2, sets[-1])
        for _ in range(reps):
            m.query(x30, E2, sets[-1])
        for _ in range(reps):
            m.query(x4096, E2, sets[-1])
        return res
    # one generation two ways, alternating
    def parent_gen():
        cp = copy.deepcopy(mf)
        cp.updt_hifi(sets[-1], np.zeros((P, 1)))
        return cp.predict(x30)
    tq, tp = [], []
    parent_gen()
    m.query(x30, E2, sets[-1])
    for _ in range(reps):
        t0 = time.perf_counter()
        m.query(x30, E2, sets[-1], mu=True, var0=True, var=True)
        t1 = time.perf_counter()
        parent_gen()
        t2 = time.perf_counter()
        tq.append(t1 - t0)
        tp.append(t2 - t1)
    res["query30_us"] = 1e6 * float(np.median(tq))
    res["parent_gen30_us"] = 1e6 * float(np.median(tp))
    res["query4096_us"] = med_us(lambda: m.query(x4096, E2, sets[-1], mu=True, var0=True, var=True), reps)
    # the look-ahead variance both ways agree (the parent's way is a real append)
    cp = copy.deepcopy(mf)
    cp.updt_hifi(sets[-1], np.zeros((P, 1)))
    v_parent = np.array(np.diag(cp.predict(x30)[1]))
    v_look = m.query(x30, E2, sets[-1]).var
    res["look_vs_parent"] = float(np.max(np.abs(v_look - v_parent) /
                                         np.maximum(np.abs(v_parent), 1e-6 * O.prior_variance(mf.hyp))))
    # get_max_var end to end
    st0 = m.stats()
    np.random.seed(0)
    t0 = time.perf_counter()
    xm, vm = mf.get_max_var(np.array([[0.2, 0.2], [0.8, 0.8]]), -1e9, 1.0, E2, sets[-1])
    res["get_max_var_s"] = time.perf_counter() - t0
    st1 = m.stats()
    res["get_max_var_launches"] = {k: st1[k] - st0[k] for k in ("look_border", "look_query")}
    # the reference's per-point get_neg_var restated on the host CPU
    XL, yL, XH, yH = mf.X_L, mf.y_L[:, 0], mf.X_H, mf.y_H[:, 0]
    XHs = np.vstack((XH, sets[-1]))
    def oracle_point():
        O.mf_faithful(XL, yL, XH, yH, mf.hyp, x1, return_cov=True)
        O.mf_faithful(XL, np.zeros(NL), XHs, np.zeros(NH + P), mf.hyp, x1, return_cov=True)
    res["oracle_point_us"] = med_us(oracle_point, max(3, reps // 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"ref": case(100, 200, 8, args.reps, args.trace, seed=1),
           "head": case(1024, 1024, 8, args.reps, args.trace, seed=2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
