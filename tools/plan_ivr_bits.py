"""The bits of Model.plan_ivr on a fixed set of cases, to compare two builds of the library
(the single planner as the batch of one against the by-value loop
before it). It calls nothing but Model.plan_ivr, so the same file runs on either checkout.

  python tools/plan_ivr_bits.py run OUT.npz        cells, points and gains of every case
  python tools/plan_ivr_bits.py compare A.npz B.npz   np.array_equal on every array; exit 1 if any differs

Cases: members 0, 4 and 6 of tests/_plan_ivr_batch.py's MEMBERS8, 40 picks, all cells and a
list of 40, weights of ones and the mask, refresh 0 and 7; and 13x11 MF with N = 60, 8 picks
(the appended rows cross row 64). Each with the V stream pinned and with the lattice forced.
The .npz holds the bits of one compiler build on one device: it is no fixture.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _ivr as I  # noqa: E402
from tests import _plan_ivr as P  # noqa: E402
from tests import _plan_ivr_batch as Q  # noqa: E402


def _build(ctx, member):
    from mfgp_coverage_amd import _lib
    kind, gname, N = member
    Xs, X, y, NL = Q.case_data(kind, gname, N)
    if N == 0:
        m = _lib.Model(ctx, _lib.SF if kind == "sf" else _lib.MF, I.hyp_of(kind), 1e-8)
        m.set_grid(Xs)
        return m
    return I._model(ctx, kind, X, y, NL, Xs)


def run(path):
    from mfgp_coverage_amd import _lib
    out = {}
    for lattice in (0, "force"):
        ctx = _lib.Context(0)
        ctx.set_lattice(lattice)
        for member in (Q.MEMBERS8[0], Q.MEMBERS8[4], Q.MEMBERS8[6], ("mf", "13x11", 60)):
            m = _build(ctx, member)
            M = Q.case_data(*member)[0].shape[0]
            cand = np.random.default_rng(5).choice(M, 40, replace=False)
            rows60 = member[2] == 60
            for listed in ((False,) if rows60 else (False, True)):
                for wname in (("ones",) if rows60 else ("ones", "mask")):
                    for refresh in ((0,) if rows60 else (0, 7)):
                        r = m.plan_ivr(8 if rows60 else Q.NPICK, weights=P.weights(wname, M),
                                       cand=cand if listed else None, refresh=refresh)
                        key = f"{lattice}/{'-'.join(map(str, member))}/{'list40' if listed else 'all'}/{wname}/r{refresh}"
                        for name, a in zip(("cells", "points", "gains"), r):
                            out[f"{key}/{name}"] = a
                        print(key, r[0].shape[0], "picks", flush=True)
    np.savez(path, **out)
    print(f"{len(out) // 3} cases -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    bad += [k for k in sorted(set(A.files) & set(B.files)) if not np.array_equal(A[k], B[k])]
    for k in bad:
        print("differs:", k)
    print(f"{len(A.files)} arrays, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
