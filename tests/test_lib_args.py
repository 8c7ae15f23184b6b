"""The argument helpers of mfgp_coverage_amd/_lib.py (_dev_matrix, _host_out, _cells, _addr,
_handles): what cov_block, var_reduction, cov_apply, plan_ivr, query, sample and the batch
functions make of their arguments before the call into the library. None of them loads
the library, so these run without a GPU; a stand-in with data_ptr(), shape, stride() and
dtype plays the device tensor."""
import ctypes

import numpy as np
import pytest

from mfgp_coverage_amd import _lib


class _Dtype:
    def __init__(self, name):
        self.name = name

    def __str__(self):
        return "torch." + self.name


class FakeTensor:
    def __init__(self, shape, stride=None, dtype="float64", addr=0x7000):
        self.shape = tuple(shape)
        if stride is None:
            stride, n = [], 1
            for d in reversed(self.shape):
                stride.insert(0, n)
                n *= d
        self._stride = tuple(stride)
        self.dtype = _Dtype(dtype)
        self._addr = addr

    def stride(self):
        return self._stride

    def data_ptr(self):
        return self._addr


def test_dev_matrix_accepts_one_and_two_dimensions():
    p, rows, cols, ld, two = _lib._dev_matrix(FakeTensor((143,), addr=0x1234), "weights", "[n] or [nw, n]")
    assert (p.value, rows, cols, ld, two) == (0x1234, 1, 143, 143, False)
    p, rows, cols, ld, two = _lib._dev_matrix(FakeTensor((3, 143), addr=0x5678), "weights", "[n] or [nw, n]")
    assert (p.value, rows, cols, ld, two) == (0x5678, 3, 143, 143, True)


def test_dev_matrix_leading_dimension():
    # from stride()[0] only with more than one row; else the column count, whatever the stride says
    assert _lib._dev_matrix(FakeTensor((3, 143), stride=(200, 1)), "x", "[M] or [k, M]")[3] == 200
    assert _lib._dev_matrix(FakeTensor((1, 143), stride=(999, 1)), "x", "[M] or [k, M]")[3] == 143
    assert _lib._dev_matrix(FakeTensor((143,), stride=(1,)), "x", "[M] or [k, M]")[3] == 143
    # a single column may carry any column stride
    assert _lib._dev_matrix(FakeTensor((4, 1), stride=(7, 5)), "x", "[M] or [k, M]")[1:4] == (4, 1, 7)


@pytest.mark.parametrize("t", [FakeTensor((3, 143), dtype="float32"), FakeTensor((2, 3, 143)),
                               FakeTensor((3, 143), stride=(286, 2)), FakeTensor((143,), stride=(2,))],
                         ids=["float32", "3d", "column_stride", "column_stride_1d"])
def test_dev_matrix_rejects(t):
    with pytest.raises(ValueError) as e:
        _lib._dev_matrix(t, "weights", "[n] or [nw, n]")
    assert str(e.value) == "weights must be a float64 tensor [n] or [nw, n] with unit column stride"
    with pytest.raises(ValueError, match=r"^out must be a float64 tensor \[M\] or \[k, M\] with unit column stride$"):
        _lib._dev_matrix(t, "out", "[M] or [k, M]")


def _read_only(a):
    a.flags.writeable = False
    return a


@pytest.mark.parametrize("out, two", [
    (np.zeros((3, 10), dtype=np.float32), True),                  # dtype
    (_read_only(np.zeros((3, 10))), True),                        # read-only
    (np.zeros(10), True), (np.zeros((3, 10)), False), (np.zeros((1, 3, 10)), True),   # ndim
    (np.zeros((2, 10)), True),                                    # too few rows
    (np.zeros((3, 10))[:, ::2], True),                            # column stride
    (np.zeros((3, 4)), True), (np.zeros(4), False),               # too few columns
    ([[0.0] * 10] * 3, True),                                     # no ndarray
], ids=["dtype", "read_only", "1d_for_2d", "2d_for_1d", "3d", "rows", "column_stride", "cols", "cols_1d", "list"])
def test_host_out_rejects(out, two):
    with pytest.raises(ValueError) as e:
        _lib._host_out(out, two, 3, 5, "out must be as asked")
    assert str(e.value) == "out must be as asked"


def test_host_out_rejects_a_row_stride_off_the_doubles():
    raw = np.zeros(3 * 84 + 8, dtype=np.uint8)
    out = np.ndarray((3, 10), dtype=np.float64, buffer=raw.data, strides=(84, 8))   # rows 84 bytes apart
    with pytest.raises(ValueError, match="^bad out$"):
        _lib._host_out(out, True, 3, 10, "bad out")
    ok = np.ndarray((3, 10), dtype=np.float64, buffer=np.zeros(3 * 88, dtype=np.uint8).data, strides=(88, 8))
    assert _lib._host_out(ok, True, 3, 10, "bad out")[1] == 11


def test_host_out_leading_dimension():
    big = np.zeros((5, 12))
    buf, ld = _lib._host_out(big, True, 3, 10, "x")
    assert buf is big and ld == 12
    buf, ld = _lib._host_out(big[:, :10], True, 3, 10, "x")        # several rows: the row stride
    assert ld == 12 and buf.shape == (5, 10)
    buf, ld = _lib._host_out(big[2:3, :10], True, 1, 10, "x")      # one row: the column count
    assert ld == 10


def test_host_out_one_dimension_is_one_row_over_the_same_memory():
    out = np.zeros(10)
    buf, ld = _lib._host_out(out, False, 1, 10, "x")
    assert buf.shape == (1, 10) and ld == 10 and np.shares_memory(buf, out)
    buf[0, 3] = 7.0
    assert out[3] == 7.0


def test_cells():
    assert _lib._cells(None, 143) == (None, None, 143)
    a, p, n = _lib._cells([], 143)
    assert n == 0 and a.dtype == np.int64 and isinstance(p, ctypes.c_void_p) and p.value     # an empty list: non-null
    a, p, n = _lib._cells([[1, 2], [3, 4]], 143)                   # flattened
    assert n == 4 and a.tolist() == [1, 2, 3, 4] and p.value == a.ctypes.data
    src = np.array([5, 0, 142], dtype=np.int32)
    a, p, n = _lib._cells(src, 143)                                # converted
    assert a.dtype == np.int64 and a.flags.c_contiguous and a.tolist() == [5, 0, 142] and n == 3
    a, p, n = _lib._cells(np.arange(10, dtype=np.int64)[::3], 143)   # strided: packed
    assert a.flags.c_contiguous and a.tolist() == [0, 3, 6, 9]


def test_addr():
    assert _lib._addr(None) is None
    e = np.empty(0)
    assert _lib._addr(e).value == e.ctypes.data and _lib._addr(e).value   # unlike ptr(): non-null when empty
    assert _lib.ptr(e) is None
    a = np.zeros(4)
    assert _lib._addr(a).value == a.ctypes.data


def test_handles_keep_the_order():
    class M:
        def __init__(self, v):
            self.handle = ctypes.c_void_p(v)
    arr = _lib._handles([M(30), M(10), M(20)])
    assert len(arr) == 3 and list(arr) == [30, 10, 20]
    assert len(_lib._handles([])) == 0


def test_stats_keys_are_a_class_constant():
    assert len(_lib.Model.STATS_KEYS) == 20 and len(set(_lib.Model.STATS_KEYS)) == 20
    assert _lib.Model.STATS_KEYS[:2] == ("factor_rows", "v_rows") and _lib.Model.STATS_KEYS[-1] == "vcol_rows_built"
