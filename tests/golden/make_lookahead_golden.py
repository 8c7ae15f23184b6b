"""Generate tests/golden/lookahead_reference.npz -- BUILD CONTAINER ONLY.

Outputs of the reference's OWN ``MFGP.pred_var`` (gp:440-481) and ``MFGP.get_neg_var``
(gp:544-563), imported from the read-only checkout with the pass-through ``autograd``
shim as make_golden.py does (no reference text is copied): three small MF cases with
N_L = 60, N_H = 137 and (P_L, P_H, Q) = (3, 5, 70), (0, 1, 1), (7, 0, 33). Stored per
case c: the inputs (``c_XL, c_yL, c_XH, c_yH, c_XLn, c_XHn, c_x``), the dense
``c_pred_var`` [Q,Q], and ``get_neg_var`` at the 40 points ``c_xn`` for two (thrd, c)
pairs ``c_tc`` [2,2] -> ``c_neg`` [2,40] (the second pair masks part of the points:
those values are 0). Plain data, no pickles.

Run: ``python tests/golden/make_lookahead_golden.py`` (needs the reference checkout; the
GPU box only reads the committed .npz).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_golden import _import_reference  # noqa: E402
from tests import _lookahead as LA  # noqa: E402

CASES = {"a": (3, 5, 70), "b": (0, 1, 1), "c": (7, 0, 33)}


def main():
    gp = _import_reference()
    out = {"hyp": LA.HYP_MF}
    for i, (name, (PL, PH, Q)) in enumerate(CASES.items()):
        rng = np.random.default_rng(100 + i)
        X = rng.random((197, 2))
        y = LA.field(X, rng)
        XL, yL, XH, yH = X[:60], y[:60, None], X[60:], y[60:, None]
        XLn, XHn = rng.random((PL, 2)), rng.random((PH, 2))
        x, xn = rng.random((Q, 2)), rng.random((40, 2))
        m = gp.MFGP(XL, yL, XH, yH, 1, 1)
        m.hyp = LA.HYP_MF.copy()
        m.updt_info(XL, yL, XH, yH)
        pv = m.pred_var(x, XLn, XHn)
        # thresholds from the current model's own mean + c var at xn: below all of them
        # (nothing masked), and their median (about half masked)
        mean, cov = m.predict(xn)
        tcs = []
        for c in (2.0, 0.5):
            s = mean[:, 0] + c * np.diag(cov)
            tcs.append((float(s.min() - 1.0) if c == 2.0 else float(np.median(s)), c))
        neg = np.array([[float(np.asarray(m.get_neg_var(p, t, c, XLn, XHn)).reshape(-1)[0]) for p in xn]
                        for (t, c) in tcs])
        assert np.all(neg[0] < 0) and 0 < np.count_nonzero(neg[1] == 0) < 40
        for k, v in dict(XL=XL, yL=yL[:, 0], XH=XH, yH=yH[:, 0], XLn=XLn, XHn=XHn, x=x, pred_var=pv, xn=xn,
                         tc=np.array(tcs), neg=neg).items():
            out[f"{name}_{k}"] = np.asarray(v, dtype=np.float64)
    path = os.path.join(HERE, "lookahead_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
