"""Host side of the covariance blocks (no GPU): the built library exports and binds
mfgp_cov_block / mfgp_model_serial, k_cov_block's code object keeps its shape
(call-free, no scratch, LDS within 64 KB), and DiagCov serves every indexing form
from a source -- here a duck-typed fake with a numpy matrix behind cov_block /
serial -- as numpy serves them from the matrix itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge


def test_library_exports_and_binds(built):
    from mfgp_coverage_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("mfgp_cov_block", "mfgp_model_serial"):
        assert name in syms
        assert name in _lib.SIGNATURES
    assert "mfgp_cov.hip" in built.SOURCES
    h = _lib.lib()
    assert h.mfgp_cov_block.argtypes == _lib.SIGNATURES["mfgp_cov_block"][1]
    assert len(_lib.SIGNATURES["mfgp_cov_block"][1]) == 8
    with open(os.path.join(ROOT, "include", "mfgp_hip.h")) as fh:
        text = fh.read()
    assert "int mfgp_cov_block(" in text and "int mfgp_model_serial(" in text and "#define MFGP_COV_PRIOR 1" in text
    assert _lib.COV_PRIOR == 1


def test_cov_kernel_code_object(built, tmp_path):
    """k_cov_block as compiled for gfx950: everything inlined, nothing in scratch, the
    two operand panels in at most 64 KB of LDS, and registers for two workgroups per CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    obj = tmp_path / "cov.o"
    subprocess.run([built.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c",
                    os.path.join(built.CSRC, "mfgp_cov.hip"), "-o", str(obj)], check=True, capture_output=True)
    rep = check_codeobj.kernel_report(str(obj))
    ks = {n: r for n, r in rep.items() if "k_cov_block" in n}
    assert len(ks) == 1 and len(rep) == 1, sorted(rep)
    for n, r in ks.items():
        assert not any(s in n for s in ("k_inc_stream", "k_inc_lat", "k_vstream"))
        assert r["calls"] == 0 and r["scratch"] == 0 and r["vgpr_spill"] == 0, (n, r)
        assert r["lds"] <= 64 * 1024, (n, r)
        assert r["vgpr"] + r["agpr"] <= 256, (n, r)


class FakeSource:
    """What DiagCov needs of a model: cov_block(rows, cols) and serial()."""

    def __init__(self, C):
        self.C = C
        self.calls = []
        self.s = 17

    def serial(self):
        return self.s

    def cov_block(self, rows=None, cols=None):
        self.calls.append((None if rows is None else np.asarray(rows).tolist(),
                           None if cols is None else np.asarray(cols).tolist()))
        M = self.C.shape[0]
        r = np.arange(M) if rows is None else np.asarray(rows, dtype=np.int64)
        c = np.arange(M) if cols is None else np.asarray(cols, dtype=np.int64)
        assert r.size == 0 or (r.min() >= 0 and r.max() < M)
        assert c.size == 0 or (c.min() >= 0 and c.max() < M)
        return self.C[np.ix_(r, c)].copy()


def _cov(M=23, seed=3):
    from mfgp_coverage_amd.gaussian_process import DiagCov
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, M))
    C = A @ A.T
    src = FakeSource(C)
    # (the diagonal a predict hands over is its own vector: here another one, to tell them apart)
    var = np.diag(C) + 1e-3
    return DiagCov(var, None, source=src), src, C, var


TWO = [((3, 7), [3], [7]),
       ((-1, 0), [22], [0]),
       ((slice(10, 20), slice(None, None, 5)), list(range(10, 20)), list(range(0, 23, 5))),
       ((slice(None, None, -3), 4), list(range(22, -1, -3)), [4]),
       ((-2, slice(-5, None)), [21], list(range(18, 23))),
       ((slice(5, 5), slice(None)), [], list(range(23))),
       ((np.int64(2), slice(1, 9, 2)), [2], [1, 3, 5, 7])]


@pytest.mark.parametrize("idx,rows,cols", TWO)
def test_two_index_forms_take_one_block(idx, rows, cols, monkeypatch):
    from mfgp_coverage_amd.gaussian_process import DiagCov
    cov, src, C, _ = _cov()
    monkeypatch.setattr(DiagCov, "_dense", lambda self: pytest.fail("formed the dense matrix"))
    got = cov[idx]
    want = C[idx]
    assert np.shape(got) == np.shape(want) and np.array_equal(got, want)
    assert src.calls == [(rows, cols)]


def test_other_forms_go_through_one_dense_matrix():
    cov, src, C, var = _cov()
    assert np.array_equal(cov[5], C[5])
    assert np.array_equal(cov[[1, 2], [3, 4]], C[[1, 2], [3, 4]])
    assert np.array_equal(cov[C > 0], C[C > 0])
    assert np.array_equal(cov[..., 2], C[..., 2])
    assert np.array_equal(np.asarray(cov), C)
    assert np.array_equal(np.array(cov, dtype=np.float32), C.astype(np.float32))
    assert np.array_equal(cov + 1.0, C + 1.0) and np.array_equal(2.0 * cov, 2.0 * C) and np.array_equal(-cov, -C)
    assert np.array_equal(np.sqrt(np.abs(cov)), np.sqrt(np.abs(C)))
    assert np.array_equal(np.linalg.eigvalsh(cov), np.linalg.eigvalsh(C))
    assert np.array_equal(np.sum(cov, axis=0), C.sum(axis=0))
    assert src.calls == [(None, None)]                 # materialised once, then kept
    with pytest.raises(ValueError):
        np.asarray(cov)[0, 0] = 1.0                   # (the kept matrix is shared: read-only)
    # block(): lists with negative entries, slices, None
    assert np.array_equal(cov.block([5, 5, -1], slice(2, 9)), C[np.ix_([5, 5, 22], range(2, 9))])
    assert src.calls[-1] == ([5, 5, 22], list(range(2, 9)))
    assert np.array_equal(cov.block(None), C)
    with pytest.raises(IndexError):
        cov.block([23])
    with pytest.raises(IndexError):
        cov[23, 0]
    with pytest.raises(IndexError):
        cov.block([0.5])
    # the diagonal's fast paths: the predict's own vector, no source call
    n = len(src.calls)
    assert np.array_equal(np.diag(cov), var) and np.amax(cov) == var.max() and np.trace(cov) == var.sum()
    assert np.argmax(cov) == int(np.argmax(var)) * 24 and cov[4, 4] == var[4] and cov[-1, -1] == var[-1]
    assert len(src.calls) == n


def test_stale_serial_raises():
    cov, src, C, var = _cov()
    np.asarray(cov)                     # (even with the dense matrix already kept)
    src.s += 1
    for use in (lambda: cov[3, 7], lambda: cov[1:3, 2:4], lambda: cov[5], lambda: np.asarray(cov),
                lambda: cov.block([1], [2]), lambda: cov * 2.0, lambda: np.linalg.eigvalsh(cov)):
        with pytest.raises(RuntimeError, match="updated"):
            use()
    assert np.array_equal(np.diag(cov), var) and np.amax(cov) == var.max() and cov[3, 3] == var[3]
    src.s -= 1
    assert cov[3, 7] == C[3, 7]


def test_dense_cap(monkeypatch):
    from mfgp_coverage_amd.gaussian_process import DiagCov
    assert DiagCov.DENSE_MAX_BYTES == 2 ** 30
    cov, src, C, _ = _cov()
    monkeypatch.setattr(DiagCov, "DENSE_MAX_BYTES", 1024)      # 23 x 23 doubles = 4232 bytes
    with pytest.raises(MemoryError, match=r"\.block"):
        np.asarray(cov)
    with pytest.raises(MemoryError):
        cov + 1.0
    assert src.calls == []
    assert np.array_equal(cov.block([1, 2], [3]), C[1:3, 3:4]) and cov[1, 3] == C[1, 3]
    monkeypatch.setattr(DiagCov, "DENSE_MAX_BYTES", 8 * 23 * 23)
    assert np.array_equal(np.asarray(cov), C)


def test_sourceless_diagcov_is_as_before():
    from mfgp_coverage_amd.gaussian_process import DiagCov
    cov = DiagCov(np.arange(4.0))
    assert cov.source is None and cov.serial is None
    for use in (lambda: cov[0, 1], lambda: cov[0:2, 0:2], lambda: np.asarray(cov), lambda: cov + 1.0,
                lambda: cov.block([0], [1])):
        with pytest.raises(TypeError, match="only the diagonal"):
            use()
    assert cov[2, 2] == 2.0 and np.array_equal(np.diag(cov), np.arange(4.0)) and np.amax(cov) == 3.0
    one = DiagCov(np.array([2.5]))
    assert np.array_equal(np.asarray(one), [[2.5]])
