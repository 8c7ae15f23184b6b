"""Generate tests/golden/nlml_edges_reference.npz -- BUILD CONTAINER ONLY.

The NLML and its gradient at the block edges of mfgp_nlml.hip (tests/_nlml_edges.py
lists the cases and why), evaluated in 80-bit extended precision by
``oracle.gp_oracle.nlml_extended`` on ``synthetic.Workload(32, NL, N - NL, 1, 1, seed=N)``
at the hyperparameters ``synthetic.HYP[key]`` (one case at ``hyp + 0.05 N(0, 1)``, seed
129, with jitter 1e-6). Needs no reference checkout, only an x86-64 host (80-bit long
double). Stored per case c:

* the inputs ``c_XL, c_yL, c_XH, c_yH, c_hyp, c_jitter`` (SF: XL / yL empty);
* ``c_nlml``, ``c_grad``: the extended values rounded once to float64;
* ``c_cond``: the 2-norm condition number of the float64 K;
* ``c_e_oracle_val``, ``c_e_oracle_grad``: the error of the fp64 ``oracle.gp_oracle.nlml``
  against the extended values, ``|v - v_ref| / max(|v_ref|, 1)`` and
  ``max_p |g_p - g_ref_p| / max(|g_ref_p|, 1)``.

Plain data, no pickles. The archive is written with fixed member times, so a second run
on the same machine gives the same bytes; ``--check`` recomputes and compares with the
committed file instead of writing. ``nlml_extended`` uses no libm function, so the
inputs, ``nlml`` and ``grad`` come out bit for bit on any x86-64 host; ``cond`` and
``e_oracle_*`` go through the host's fp64 BLAS / LAPACK and may differ in their last
digits on another CPU (``--check`` then names them).

Run: ``python tests/golden/make_nlml_edges_golden.py [--check]`` (the GPU box only reads
the committed .npz).
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
from tests import _nlml_edges as E  # noqa: E402

PATH = os.path.join(HERE, "nlml_edges_reference.npz")


def _K64(XL, XH, hyp, jitter):
    if hyp.shape[0] == 9:
        return O.mf_K(XL, XH, hyp, jitter)
    n = XH.shape[0]
    return O.se_kernel(XH, XH, hyp[1], hyp[2]) + np.eye(n) * np.exp(hyp[-1]) + np.eye(n) * jitter


def compute():
    out = {}
    for name, kind, n, nl, key, perturbed in E.CASES:
        wl = synthetic.Workload(32, nl, n - nl, 1, 1, seed=n)
        hyp, jitter = synthetic.HYP[key].copy(), O.JITTER
        if perturbed:
            hyp = hyp + 0.05 * np.random.default_rng(n).standard_normal(hyp.shape[0])
            jitter = 1e-6
        XL, yL, XH, yH = wl.XL.reshape(-1, 2), wl.yL, wl.XH.reshape(-1, 2), wl.yH
        assert XL.shape[0] == nl and XH.shape[0] == n - nl and (kind == "mf" or nl == 0)
        kw = E.oracle_kwargs(XL, yL, hyp)
        v, g = O.nlml_extended(XH, yH, hyp, jitter=jitter, **kw)
        vo, go = O.nlml(XH, yH, hyp, jitter=jitter, grad=True, **kw)
        one = np.longdouble(1)
        ev = abs(vo - v) / max(abs(v), one)
        eg = np.max(np.abs(go - g) / np.maximum(np.abs(g), one))
        for k, a in dict(XL=XL, yL=yL, XH=XH, yH=yH, hyp=hyp, jitter=jitter, nlml=v, grad=g,
                         cond=np.linalg.cond(_K64(XL, XH, hyp, jitter), 2), e_oracle_val=ev,
                         e_oracle_grad=eg).items():
            out[f"{name}_{k}"] = np.asarray(a).astype(np.float64)
        print(f"{name:42s} cond {float(out[name + '_cond']):9.3g}  oracle err val {float(ev):8.2e} grad {float(eg):8.2e}")
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
