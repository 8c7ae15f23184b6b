"""Time likelihood + analytic gradient at N = 2048 (MF, australia9 hyperparameters) on
the device: one mfgp_nlml call, S sequential mfgp_nlml calls against one mfgp_nlml_batch
of the same S vectors (in the same process, after a warm-up of both), and the oracle's
NumPy version on the host.

    python tools/bench_nlml.py [N [S]]        (defaults 2048 and 8)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

R = 5   # repeats; the median is reported


def _median_ms(f):
    ts = []
    for _ in range(R):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    from mfgp_coverage_amd import _lib, synthetic
    from oracle import gp_oracle as O
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    hyp = synthetic.HYP["australia9_mf"]
    wl = synthetic.Workload(128, N // 2, N - N // 2, 1, 1, seed=0)
    m = _lib.Model(_lib.context(), _lib.MF, hyp, 1e-8)
    m.set_data(wl.XL, wl.yL, wl.XH, wl.yH)
    rng = np.random.default_rng(0)
    H = np.vstack([hyp] + [hyp + 0.05 * rng.standard_normal(9) for _ in range(S - 1)])
    # warm-up of both paths (the batch's scratch is allocated here), and the promise itself
    seq = [m.nlml(h, grad=True) for h in H]
    vb, gb = m.nlml_batch(H, grad=True)
    same = all(np.float64(v).tobytes() == vb[s].tobytes() and g.tobytes() == gb[s].tobytes()
               for s, (v, g) in enumerate(seq))
    one = _median_ms(lambda: m.nlml(hyp, grad=True))
    sequential = _median_ms(lambda: [m.nlml(h, grad=True) for h in H])
    batch = _median_ms(lambda: m.nlml_batch(H, grad=True))
    t0 = time.perf_counter()
    O.nlml(wl.XH, wl.yH, hyp, XL=wl.XL, yL=wl.yL, grad=True)
    cpu = time.perf_counter() - t0
    print(json.dumps({"N": N, "gpu_ms": one, "cpu_oracle_ms": cpu * 1e3, "nlml": seq[0][0], "S": S,
                      "sequential_ms": sequential, "batch_ms": batch, "ratio": sequential / batch,
                      "batch_bits_equal_sequential": bool(same)}))


if __name__ == "__main__":
    main()
