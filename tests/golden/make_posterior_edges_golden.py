"""Generate tests/golden/posterior_edges_reference.npz -- BUILD CONTAINER ONLY.

The posterior mean and variance on the grid at the tile edges of the routes that produce
them (tests/_posterior_edges.py lists the cases and why), evaluated in 80-bit extended
precision by ``oracle.gp_oracle.posterior_extended`` on ``_posterior_edges.make_inputs``
(distinct grid cells in a random order, seeded by N) at the hyperparameters
``synthetic.HYP[key]``. Needs no reference checkout, only an x86-64 host (80-bit long
double). Stored per case c:

* the inputs ``c_XL, c_yL, c_XH, c_yH, c_hyp, c_jitter, c_Xs`` (SF: XL / yL empty), all N rows;
* per stage s (the first s rows, ``_posterior_edges.stages``):
  ``c_s<s>_mu``, ``c_s<s>_var``, ``c_s<s>_kss``: the extended values rounded once to float64;
  ``c_s<s>_cond``: the 2-norm condition number of the float64 K (1 at s = 0);
  ``c_s<s>_e_oracle_mu``, ``c_s<s>_e_oracle_var``: the error of the fp64
  ``oracle.gp_oracle.sf_diag`` / ``mf_diag`` against the extended values,
  ``max_c |mu_c - ref_c| / max_c |ref_c|`` and ``max_c |var_c - ref_c| / k**``.

Plain data, no pickles. The archive is written with fixed member times, so a second run
on the same machine gives the same bytes; ``--check`` recomputes and compares with the
committed file instead of writing. ``posterior_extended`` uses no libm function, so
``mu``, ``var`` and ``kss`` come out bit for bit on any x86-64 host; the inputs' ``y`` (libm
sin / cos), ``cond`` and ``e_oracle_*`` go through the host's libm / fp64 BLAS / LAPACK and
may differ in their last digits on another CPU (``--check`` then names them).

Run: ``python tests/golden/make_posterior_edges_golden.py [--check]`` (the GPU box only
reads the committed .npz).
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mfgp_coverage_amd import synthetic  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from tests import _posterior_edges as E  # noqa: E402

PATH = os.path.join(HERE, "posterior_edges_reference.npz")


def _K64(XL, XH, hyp, jitter):
    if hyp.shape[0] == 9:
        return O.mf_K(XL, XH, hyp, jitter)
    n = XH.shape[0]
    return O.se_kernel(XH, XH, hyp[1], hyp[2]) + np.eye(n) * np.exp(hyp[-1]) + np.eye(n) * jitter


def compute():
    out = {}
    for name, kind, key, n, nl, nx, ny, offgrid in E.CASES:
        hyp, jitter = synthetic.HYP[key].copy(), O.JITTER
        Xs, X, y = E.make_inputs(n, nl, nx, ny, offgrid)
        assert X.shape == (n, 2) and (kind == "mf" or nl == 0) and hyp.shape[0] == (4 if kind == "sf" else 9)
        assert np.unique(X, axis=0).shape[0] == n
        for k, a in dict(XL=X[:nl], yL=y[:nl], XH=X[nl:], yH=y[nl:], hyp=hyp, jitter=jitter, Xs=Xs).items():
            out[f"{name}_{k}"] = np.asarray(a).astype(np.float64)
        for s in E.stages(n, nl):
            XL, yL, XH, yH = X[:nl], y[:nl], X[nl:s], y[nl:s]
            mu, var, kss = O.posterior_extended(XL, yL, XH, yH, hyp, Xs, jitter)
            mu_o, var_o = E.oracle(XL, yL, XH, yH, hyp, Xs, jitter)
            e_mu = np.max(np.abs(mu_o - mu)) / np.max(np.abs(mu))
            e_var = np.max(np.abs(var_o - var)) / kss
            cond = np.linalg.cond(_K64(XL, XH, hyp, jitter), 2) if s else 1.0
            for k, a in dict(mu=mu, var=var, kss=kss, cond=cond, e_oracle_mu=e_mu, e_oracle_var=e_var).items():
                out[f"{name}_s{s}_{k}"] = np.asarray(a).astype(np.float64)
            floor = E.EPS64 * float(cond) * max(s, 64)
            print(f"{name:44s} s {s:3d} M {Xs.shape[0]:3d} cond {float(cond):9.3g}  oracle err mu {float(e_mu):8.2e} "
                  f"var {float(e_var):8.2e}  floor {floor:8.2e}")
    return out


def write(out, path):
    """np.savez_compressed with fixed member times (the same bytes on every run)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a, order="C"), allow_pickle=False)   # (0-d stays 0-d)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    out = compute()
    if "--check" in sys.argv[1:]:
        with np.load(PATH) as z:
            assert sorted(z.files) == sorted(out), "the committed fixture holds other arrays"
            bad = [k for k in out if out[k].shape != z[k].shape or out[k].tobytes() != z[k].tobytes()]
        assert not bad, f"differs from the committed fixture: {bad}"
        print("identical to", PATH)
        return
    write(out, PATH)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
