"""ctypes binding of libmfgp_hip.so (C ABI declared in include/mfgp_hip.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU
is visible, every entry point raises instead of computing on the host.
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFGP_LIB") or os.path.join(HERE, "libmfgp_hip.so")

OK, ERR_NOT_PD, ERR_ARG, ERR_DEVICE, ERR_NO_V, ERR_NO_LATTICE = 0, 1, 2, 3, 4, 5
COV_PRIOR = 1
SAMPLE_PRIOR = 1
LOOK_MAX = 64   # prospective points per query (MFGP_LOOK_MAX)
IVR_MAXW = 8    # weight vectors per var_reduction call (MFGP_IVR_MAXW)
IVR_SEG_CELLS = 512   # grid cells per row segment of k_ivr_partial (8 tiles of 64): one partial sum each
QueryResult = collections.namedtuple("QueryResult", ("mu", "var0", "var", "cov"))
SF, MF = 0, 1
F64, F32 = 0, 1
ASYNC = 1

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int64_p = ctypes.POINTER(ctypes.c_int64)

# name -> (restype, argtypes); every symbol declared in include/mfgp_hip.h
SIGNATURES = {
    "mfgp_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "mfgp_ctx_destroy": (None, [ctypes.c_void_p]),
    "mfgp_ctx_trim": (ctypes.c_int, [ctypes.c_void_p]),
    "mfgp_ctx_set_nlml_chunk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_ctx_get_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "mfgp_ctx_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "mfgp_ctx_set_incremental": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_set_fused": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_set_deferred_appends": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_set_lattice": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_set_lattice_vcol": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_set_vcol_budget": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_debug_read_v": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         _c_int64_p, _c_int64_p]),
    "mfgp_debug_read_f": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_int64_p]),
    "mfgp_debug_live": (ctypes.c_int, [_c_int64_p]),
    "mfgp_ctx_set_timing_stride": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_ctx_set_concurrent": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_batch_append_predict_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "mfgp_model_stats": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, ctypes.c_int]),
    "mfgp_nlml": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, _c_double_p, ctypes.c_void_p]),
    "mfgp_nlml_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_cell_reduce": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_batch_cell_reduce": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_sample_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p,
                                          _c_int64_p]),
    "mfgp_batch_sample_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_ctx_enable_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mfgp_ctx_get_timing": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_int64_p, _c_double_p, _c_int64_p]),
    "mfgp_ctx_reset_timing": (ctypes.c_int, [ctypes.c_void_p]),
    "mfgp_ctx_planner_stats": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, ctypes.c_int, ctypes.c_int]),
    "mfgp_model_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)]),
    "mfgp_model_destroy": (None, [ctypes.c_void_p]),
    "mfgp_clone": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "mfgp_model_set_hyp": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double]),
    "mfgp_set_grid": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_set_data": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_append": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_predict_view": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                         ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "mfgp_predict_view_running": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_int)]),
    "mfgp_cov_block": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "mfgp_var_reduction": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_cov_apply": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "mfgp_plan_ivr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_int64_p]),
    "mfgp_batch_plan_ivr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "mfgp_query": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_sample_axis_factor": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                               ctypes.POINTER(ctypes.c_int)]),
    "mfgp_sample_dims": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, ctypes.c_int, ctypes.c_int]),
    "mfgp_sample_posterior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "mfgp_model_serial": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "mfgp_release_view": (ctypes.c_int, [ctypes.c_void_p]),
    "mfgp_view_max": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_int64_p, ctypes.POINTER(ctypes.c_int)]),
    "mfgp_model_n": (ctypes.c_int64, [ctypes.c_void_p]),
    "mfgp_model_nl": (ctypes.c_int64, [ctypes.c_void_p]),
    "mfgp_model_m": (ctypes.c_int64, [ctypes.c_void_p]),
    "mfgp_get_factor": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mfgp_batch_append_predict": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_void_p, _c_int64_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int]),
    "mfgp_batch_append_factor": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, _c_int64_p, ctypes.c_int]),
    "mfgp_batch_predict": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int]),
    "mfgp_truncate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "mfgp_batch_truncate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "mfgp_last_error": (ctypes.c_char_p, []),
    "mfgp_version": (ctypes.c_char_p, []),
}

_lib = None
_lib_lock = threading.Lock()


def lib():
    """Load libmfgp_hip.so (once). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
            # One HIP runtime per process: PyTorch-ROCm bundles its own
            # libamdhip64.so.7 (same SONAME as /opt/rocm's). Loading torch first
            # makes the dynamic linker bind this library to that same runtime, so
            # torch tensors, streams and RCCL share one HIP runtime with the kernels.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            h = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                f = getattr(h, name)
                f.restype = res
                f.argtypes = args
            _lib = h
    return _lib


class NoLatticeError(ValueError):
    """MFGP_ERR_NO_LATTICE: the grid is not a lattice, or a training row is not one of its cells."""


def check(rc):
    if rc == OK:
        return
    msg = lib().mfgp_last_error().decode(errors="replace")
    if rc == ERR_NO_LATTICE:
        raise NoLatticeError(msg)
    if rc == ERR_NOT_PD:
        raise np.linalg.LinAlgError(msg)
    if rc == ERR_ARG:
        if "Hyperparameters must be" in msg:
            raise TypeError(msg)
        raise ValueError(msg)
    raise RuntimeError(f"libmfgp_hip: {msg}")


def ptr(a):
    """Host pointer of a C-contiguous float64 ndarray (None for empty)."""
    if a is None or a.size == 0:
        return None
    return ctypes.c_void_p(a.ctypes.data)


# Argument helpers of the entry points below (no call into the library: tests/test_lib_args.py).

def _addr(a):
    """Pointer of an ndarray, non-null also for an empty one (an empty list or output is
    still one); None for None."""
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _handles(models):
    """The models' handles as a C array, in order."""
    return (ctypes.c_void_p * len(models))(*[m.handle.value for m in models])


def _cells(v, M):
    """A list of grid cells -> (int64 array, its pointer, its length); None = all M cells:
    (None, None, M)."""
    if v is None:
        return None, None, M
    a = np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int64)
    return a, _addr(a), a.shape[0]


def _dev_matrix(t, what, shape_text):
    """A device tensor (data_ptr(), shape, stride(), dtype) [n] or [rows, n] of float64 with unit
    column stride -> (address, rows, columns, leading dimension, 2-D?)."""
    shape, stride = tuple(t.shape), tuple(t.stride())
    if str(getattr(t, "dtype", "")).rsplit(".", 1)[-1] != "float64" or len(shape) not in (1, 2) or \
            (shape[-1] > 1 and stride[-1] != 1):
        raise ValueError(f"{what} must be a float64 tensor {shape_text} with unit column stride")
    two = len(shape) == 2
    ld = int(stride[0]) if two and shape[0] > 1 else int(shape[-1])
    return ctypes.c_void_p(int(t.data_ptr())), (int(shape[0]) if two else 1), int(shape[-1]), ld, two


def _host_out(out, two, rows, min_cols, what):
    """A caller's host output, float64 and writable with unit column stride: [>= rows, >= min_cols]
    if two, else [>= min_cols] (taken as one row) -> (the [r, c] array over its memory, its leading
    dimension). what: the text of the ValueError."""
    if not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.ndim != (2 if two else 1) or \
            out.strides[-1] != 8 or not out.flags.writeable or out.shape[-1] < min_cols or \
            (two and (out.shape[0] < rows or out.strides[0] % 8)):
        raise ValueError(what)
    buf = out if two else out.reshape(1, -1)
    return buf, (int(buf.strides[0] // 8) if buf.shape[0] > 1 else int(buf.shape[1]))


class Context:
    """One HIP stream + workspace (mfgp_ctx)."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        check(lib().mfgp_ctx_create(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = device

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib is not None:
            _lib.mfgp_ctx_destroy(h)
            self.handle = None

    def synchronize(self):
        check(lib().mfgp_ctx_synchronize(self.handle))

    def trim(self):
        """Free the context's scratch (the MFGP_F32 full predict's fp64 V scratch and
        the workspace); models keep their state."""
        check(lib().mfgp_ctx_trim(self.handle))

    def set_nlml_chunk(self, n):
        """Members per set of launches of Model.nlml_batch (0: automatic, as many as its
        scratch budget holds). The results do not depend on it."""
        check(lib().mfgp_ctx_set_nlml_chunk(self.handle, int(n)))

    def set_stream(self, stream_ptr):
        check(lib().mfgp_ctx_set_stream(self.handle, ctypes.c_void_p(stream_ptr)))

    def set_incremental(self, on=True):
        """Bordered-Cholesky appends + one-pass predicts over the resident V (default),
        or full refactor + full V recompute on every update (the reference's work)."""
        check(lib().mfgp_ctx_set_incremental(self.handle, 1 if on else 0))

    def set_fused(self, on=True):
        """Bordered append + one-pass predict of a batch in one launch (default on)."""
        check(lib().mfgp_ctx_set_fused(self.handle, 1 if on else 0))

    def set_deferred_appends(self, on=True):
        """Stage appends and run them with the next predict, in one launch (default off:
        an append factors at once, so a non-PD step raises in updt / updt_hifi as in
        the reference; deferred, it raises in the predict that runs it)."""
        check(lib().mfgp_ctx_set_deferred_appends(self.handle, 1 if on else 0))

    def set_lattice(self, on=True):
        """Lattice-separable appends (k_inc_lat, default on where they apply: lattice
        grid, kss / (noise + jitter) <= 1e4, the old rows' posterior resident, enough
        GEMM tiles in the batch to fill the GPU), or always the one-pass V stream.
        on="force": also for batches too small to fill the GPU (tests)."""
        check(lib().mfgp_ctx_set_lattice(self.handle, 2 if on == "force" else (1 if on else 0)))

    def set_lattice_vcol(self, mode="auto"):
        """The lattice step's column store of V (mfgp_ctx_set_lattice_vcol): "auto" (default:
        a batch whose models all have a store reads L21 from it), False (never, none is
        allocated) or True (as auto). The results are the same bits either way."""
        check(lib().mfgp_ctx_set_lattice_vcol(self.handle, -1 if mode == "auto" else (1 if mode else 0)))

    def set_vcol_budget(self, nbytes=-1):
        """Bytes one model's column store may take (-1: the built-in bound; 0: none)."""
        check(lib().mfgp_ctx_set_vcol_budget(self.handle, int(nbytes)))

    def set_concurrent(self, on=True):
        """This context's launches may run beside other contexts' on the same GPU
        (mfgp_ctx_set_concurrent): no launch relies on all its workgroups being
        resident at once (the lattice GEMM always as its own launch)."""
        check(lib().mfgp_ctx_set_concurrent(self.handle, 1 if on else 0))

    def enable_timing(self, on=True, predict_only=False):
        """HIP-event timing of the predict launches (and, unless predict_only, the factor stages)."""
        check(lib().mfgp_ctx_enable_timing(self.handle, (2 if predict_only else 1) if on else 0))

    def set_timing_stride(self, stride):
        """Time only every stride-th eligible launch (events sample the kernel durations)."""
        check(lib().mfgp_ctx_set_timing_stride(self.handle, int(stride)))

    def reset_timing(self):
        check(lib().mfgp_ctx_reset_timing(self.handle))

    def timing(self):
        pm, fm = ctypes.c_double(), ctypes.c_double()
        pn, fn = ctypes.c_int64(), ctypes.c_int64()
        check(lib().mfgp_ctx_get_timing(self.handle, ctypes.byref(pm), ctypes.byref(pn),
                                        ctypes.byref(fm), ctypes.byref(fn)))
        return {"predict_ms": pm.value, "predict_launches": pn.value,
                "factor_ms": fm.value, "factor_calls": fn.value}

    PLANNER_KEYS = ("runs", "inc_factor", "vstream", "lattice", "lattice_arg", "lattice_g2", "full_factor",
                    "full_predict", "batch_setup_us", "batch_loop_us", "batch_finish_us")

    def planner_stats(self, reset=False):
        """Path counters of the planners' loops (mfgp_sample_points /
        mfgp_batch_sample_points) since the last reset: how many model runs, and which step
        form their iterations took (vstream counts every one-pass predict, lattice steps
        included)."""
        out = (ctypes.c_int64 * len(self.PLANNER_KEYS))()
        check(lib().mfgp_ctx_planner_stats(self.handle, out, len(self.PLANNER_KEYS), 1 if reset else 0))
        return dict(zip(self.PLANNER_KEYS, (int(v) for v in out)))


_tls = threading.local()
_default_device = int(os.environ.get("MFGP_DEVICE", "0"))


def live_allocations():
    """Tests only: (device buffers, their bytes, pinned buffers, their bytes) the library holds."""
    out = (ctypes.c_int64 * 4)()
    check(lib().mfgp_debug_live(out))
    return tuple(int(v) for v in out)


def set_device(device):
    """Device used by models created afterwards in this process (one process per GPU)."""
    global _default_device
    _default_device = int(device)


def set_deferred_appends(on=True, device=None):
    """Deferred appends on the calling thread's context (see Context.set_deferred_appends):
    updt / updt_hifi stage their rows and the next predict runs the bordered append and
    the one-pass predict as one launch."""
    context(device).set_deferred_appends(on)


def context(device=None):
    """The calling thread's context for `device` (one stream per host thread)."""
    dev = _default_device if device is None else int(device)
    ctxs = getattr(_tls, "ctxs", None)
    if ctxs is None:
        ctxs = _tls.ctxs = {}
    if dev not in ctxs:
        ctxs[dev] = Context(dev)
    return ctxs[dev]


class _ViewLease:
    """One buffer handed over by mfgp_predict_view; returned to the pool when the
    last array over it is gone."""

    __slots__ = ("view",)

    def __init__(self, view):
        self.view = view

    def __del__(self):
        if _lib is not None and self.view:
            _lib.mfgp_release_view(ctypes.c_void_p(self.view))
            self.view = None


class _HostView:
    """[n] float64 at a host address, for np.asarray (which keeps this object, and
    so the lease, as the array's base)."""

    __slots__ = ("__array_interface__", "lease")

    def __init__(self, addr, n, lease):
        self.__array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(addr), False), "version": 3}
        self.lease = lease


class Model:
    """Owning handle of one device-resident GP (mfgp_model)."""

    def __init__(self, ctx, kind, hyp, jitter, handle=None, dtype=F64):
        """dtype: F64 (default; everything in fp64, the reference's precision) or F32
        (the resident V = L^-1 psi^T -- the only O(M N) state -- stored and streamed in
        fp32; factor, solves and reductions stay fp64; BASELINE configs[4])."""
        self.ctx = ctx
        self.kind = kind
        self.dtype = dtype
        if handle is None:
            hyp = np.ascontiguousarray(hyp, dtype=np.float64)
            h = ctypes.c_void_p()
            check(lib().mfgp_model_create(ctx.handle, kind, int(dtype), ptr(hyp), int(hyp.shape[0]),
                                          float(jitter), ctypes.byref(h)))
            handle = h
        self.handle = handle

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib is not None:
            _lib.mfgp_model_destroy(h)
            self.handle = None

    def clone(self):
        h = ctypes.c_void_p()
        check(lib().mfgp_clone(self.handle, ctypes.byref(h)))
        return Model(self.ctx, self.kind, None, None, handle=h, dtype=self.dtype)

    def set_hyp(self, hyp, jitter):
        hyp = np.ascontiguousarray(hyp, dtype=np.float64).reshape(-1)
        check(lib().mfgp_model_set_hyp(self.handle, ptr(hyp), int(hyp.shape[0]), float(jitter)))

    def set_grid(self, xs):
        xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(-1, 2)
        check(lib().mfgp_set_grid(self.handle, ptr(xs), xs.shape[0]))

    def set_data(self, XL, yL, XH, yH):
        XL, yL, XH, yH = (np.ascontiguousarray(a, dtype=np.float64) for a in (XL, yL, XH, yH))
        check(lib().mfgp_set_data(self.handle, ptr(XL), ptr(yL), XL.size // 2, ptr(XH), ptr(yH), XH.size // 2))

    def append(self, X, y):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        check(lib().mfgp_append(self.handle, ptr(X), ptr(y), X.size // 2))

    def predict(self):
        M = lib().mfgp_model_m(self.handle)
        mu = np.empty(M, dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        check(lib().mfgp_predict(self.handle, ptr(mu) if M else None, ptr(var) if M else None))
        return mu, var

    def predict_view(self, with_max=False):
        """predict() without the host copy: (mu, var) are writable arrays over the
        model's pinned result buffer, handed over to them (mfgp_predict_view); the
        buffer goes back to the library's pool when both arrays are gone. with_max:
        (mu, var, fused) where fused is (max var, its first cell) as the launch that
        wrote the buffer reduced them (mfgp_view_max), or None."""
        mu_p, var_p, view, running = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(0)
        L = lib()
        check(L.mfgp_predict_view_running(self.handle, ctypes.byref(mu_p), ctypes.byref(var_p), ctypes.byref(view),
                                          ctypes.byref(running)))
        M = L.mfgp_model_m(self.handle)
        if not view.value:
            e = np.empty(M, dtype=np.float64), np.empty(M, dtype=np.float64)
            return (*e, None) if with_max else e
        lease = _ViewLease(view.value)
        mu, var = np.asarray(_HostView(mu_p.value, M, lease)), np.asarray(_HostView(var_p.value, M, lease))
        if running.value:
            # the eager append's launch was still computing into the buffer: the arrays
            # were wrapped meanwhile and are given out once it has ended
            check(L.mfgp_ctx_synchronize(self.ctx.handle))
        if not with_max:
            return mu, var
        vm, am, ok = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int(0)
        check(L.mfgp_view_max(ctypes.c_void_p(view.value), ctypes.byref(vm), ctypes.byref(am), ctypes.byref(ok)))
        return mu, var, ((np.float64(vm.value), int(am.value)) if ok.value else None)

    def cov_block(self, rows=None, cols=None, out=None, prior=False, ldo=None):
        """cov[rows, cols] of the dense posterior covariance (gp:146 / gp:435-436) from the
        resident V (mfgp_cov_block): an [a, b] ndarray. rows / cols: sequences of grid
        cell indices in [0, M) (any order, repeats allowed), None = all cells. out: a host
        float64 matrix to fill in place (its row stride is the leading dimension), or the
        integer device address of a row-major [a, ldo] float64 buffer (ldo defaults to b;
        returns None). prior: the prior covariance k** alone.
        Settles a pending append / new hyperparameters / a new grid as predict() would."""
        L = lib()
        M = L.mfgp_model_m(self.handle)
        _r, rp, na = _cells(rows, M)
        _c, cp, nb = _cells(cols, M)
        flags = COV_PRIOR if prior else 0
        if isinstance(out, np.ndarray):
            # a caller's host matrix: row-major float64 rows, leading dimension = its row stride
            _host_out(out, True, na, 0, "out must be a writable row-major float64 matrix of at least [a] rows")
            res, o_p, ld = out[:na, :nb], _addr(out), out.strides[0] // 8
        elif out is not None:
            res, o_p, ld = None, ctypes.c_void_p(int(out)), nb
        else:
            res = np.empty((na, nb), dtype=np.float64)
            o_p, ld, ldo = _addr(res), nb, None
        check(L.mfgp_cov_block(self.handle, rp, na, cp, nb, o_p, int(ld if ldo is None else ldo), flags))
        return res

    def var_reduction(self, cand=None, weights=None, out=None, with_best=False):
        """Integrated variance reduction per candidate cell (mfgp_var_reduction): how much the
        weighted posterior variance of the whole grid falls if the hifi field is measured at
        cell cand[j], sum_i w_i cov(i, c)^2 / (cov(c, c) + noise_H + jitter), from the
        resident V without the M x C block. cand: grid cell indices in [0, M) (any order,
        repeats allowed), None = all cells. weights: None (ones), [M], or [nw, >= M] with
        nw <= IVR_MAXW -- a float64 ndarray or a device tensor (anything with data_ptr(),
        shape and stride()); a 2-D weights gives [nw, nc], else [nc]. out: a host float64
        array or a device tensor of that shape to fill in place (a device out returns None
        for the scores). with_best: (scores, best, best_pos) with the maximum of every row
        and its first position in the candidate list (scalars for 1-D weights).
        Settles the model as cov_block() does and leaves it unchanged; a score's bits depend
        only on the model, its cell and its weight vector."""
        L = lib()
        M = L.mfgp_model_m(self.handle)
        _ca, cp, nc = _cells(cand, M)
        if weights is None:
            wp, nw, ldw, two = None, 1, M, False
        elif hasattr(weights, "data_ptr"):
            wp, nw, wn, ldw, two = _dev_matrix(weights, "weights", "[n] or [nw, n]")
            if wn < M:
                raise ValueError(f"weights must have at least M = {M} columns")
        else:
            wa = np.asarray(weights, dtype=np.float64)
            if wa.ndim not in (1, 2) or wa.shape[-1] < M:
                raise ValueError(f"weights must be [M] or [nw, >= M] with M = {M}")
            two = wa.ndim == 2
            wa = np.ascontiguousarray(wa.reshape(-1, wa.shape[-1]))
            wp, nw, ldw = _addr(wa), wa.shape[0], wa.shape[1]
        bv = np.empty(max(nw, 1), dtype=np.float64) if with_best else None
        bp = np.empty(max(nw, 1), dtype=np.int64) if with_best else None
        if out is not None and hasattr(out, "data_ptr"):
            o_p, orows, ocols, ldo, otwo = _dev_matrix(out, "out", "[n] or [nw, n]")
            if otwo != two or orows < nw:
                raise ValueError("out must have the shape of the result")
            res = None
        else:
            buf, ldo = (np.empty((nw, nc), dtype=np.float64), nc) if out is None else \
                _host_out(out, two, nw, 0, "out must be a writable float64 array of the result's shape")
            o_p = _addr(buf)
            res = buf[:nw, :nc] if two else buf[0, :nc]
        check(L.mfgp_var_reduction(self.handle, cp, nc, wp, nw, ldw, o_p, ldo, _addr(bv), _addr(bp)))
        if not with_best:
            return res
        if two:
            return res, bv[:nw], bp[:nw]
        return res, np.float64(bv[0]), int(bp[0])

    def cov_apply(self, x, out=None, prior=False):
        """The posterior covariance applied to grid vectors (mfgp_cov_apply): cov @ x from the
        resident V in two streamed passes per vector, without the M x M matrix. x: a float64
        ndarray [M] or [k, M] with k <= IVR_MAXW (row k one vector), or a device tensor of
        that shape (data_ptr(), shape, stride(); unit column stride). Returns the same shape;
        out: a host float64 array or a device tensor of that shape to fill in place (a
        device out returns None). prior: K** @ x alone. Settles the model as cov_block() does
        and leaves it unchanged; a row's bits depend only on the model and that row of x."""
        L = lib()
        M = L.mfgp_model_m(self.handle)
        if hasattr(x, "data_ptr"):
            xp, nx, xn, ldx, two = _dev_matrix(x, "x", "[M] or [k, M]")
        else:
            xa = np.asarray(x, dtype=np.float64)
            if xa.ndim not in (1, 2):
                raise ValueError(f"x must be [M] or [k, M] with M = {M}")
            two = xa.ndim == 2
            xa = np.ascontiguousarray(xa.reshape(-1, xa.shape[-1]))
            xp, nx, xn, ldx = _addr(xa), xa.shape[0], xa.shape[1], xa.shape[1]
        if xn != M:
            raise ValueError(f"x must have M = {M} columns (got {xn})")
        flags = COV_PRIOR if prior else 0
        if out is not None and hasattr(out, "data_ptr"):
            o_p, orows, ocols, ldo, otwo = _dev_matrix(out, "out", "[M] or [k, M]")
            if otwo != two or orows < nx or ocols < M:
                raise ValueError("out must have the shape of x")
            check(L.mfgp_cov_apply(self.handle, xp, nx, ldx, o_p, ldo, flags))
            return None
        buf, ldo = (np.empty((nx, M), dtype=np.float64), M) if out is None else \
            _host_out(out, two, nx, M, "out must be a writable float64 array of x's shape")
        check(L.mfgp_cov_apply(self.handle, xp, nx, ldx, _addr(buf), ldo, flags))
        return buf[:nx, :M] if two else buf[0, :M]

    def plan_ivr(self, n_points, weights=None, cand=None, min_gain=0.0, refresh=0):
        """The greedy integrated-variance planner (mfgp_plan_ivr): up to n_points grid cells,
        each the allowed cell with the largest var_reduction() score given the picks before
        it -> (cells [n] int64, points [n, 2], gains [n]); gains[t] is pick t's score when it
        was chosen. weights: None (ones) or [>= M], a float64 ndarray or a device tensor.
        cand: the allowed cells (None = all). The run stops before the first pick whose
        score is < min_gain. refresh = R > 0: the numerators are recomputed from scratch after
        every R picks. The model is unchanged; its loop is counted in Context.planner_stats()."""
        L = lib()
        M = L.mfgp_model_m(self.handle)
        n_points = int(n_points)
        _ca, cp, nc = _cells(cand, M)
        if weights is None:
            wp, ldw = None, M
        elif hasattr(weights, "data_ptr"):
            shape, stride = tuple(weights.shape), tuple(weights.stride())
            if str(getattr(weights, "dtype", "")).rsplit(".", 1)[-1] != "float64" or len(shape) != 1 or \
                    (shape[0] > 1 and stride[0] != 1):
                raise ValueError("weights must be a contiguous float64 tensor [>= M]")
            wp, ldw = ctypes.c_void_p(int(weights.data_ptr())), int(shape[0])
        else:
            wa = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
            if wa.ndim != 1:
                raise ValueError(f"weights must be [>= M] with M = {M}: one weight vector")
            wp, ldw = _addr(wa), wa.shape[0]
        P = max(n_points, 1)
        cells = np.empty(P, dtype=np.int64)
        pts = np.empty((P, 2), dtype=np.float64)
        gains = np.empty(P, dtype=np.float64)
        n = ctypes.c_int64(0)
        check(L.mfgp_plan_ivr(self.handle, wp, ldw, cp, nc, n_points, float(min_gain), int(refresh),
                              _addr(cells), _addr(pts), _addr(gains), ctypes.byref(n)))
        k = int(n.value)
        return cells[:k].copy(), pts[:k].copy(), gains[:k].copy()

    def query(self, Xq, XL_new=None, XH_new=None, mu=True, var0=False, var=True, cov=False, ldc=None):
        """The posterior at arbitrary points Xq [n, 2], optionally with prospective lofi /
        hifi points XL_new / XH_new (at most LOOK_MAX together; an SF model takes its in
        XH_new) that are not in the model (mfgp_query): QueryResult(mu, var0, var, cov)
        with None for what was not asked for -- mu and var0 [n] of the current model,
        var [n] with the prospective points added, cov the dense [n, n] look-ahead
        covariance (ldc: its leading dimension, default n). The model's rows, grid,
        resident V and posterior stay as they are."""
        def pts(a):
            if a is None:
                return np.empty((0, 2), dtype=np.float64)
            return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 2))
        Xq, XL, XH = pts(Xq), pts(XL_new), pts(XH_new)
        n = Xq.shape[0]
        ldc = n if ldc is None else int(ldc)
        o_mu = np.empty(n, dtype=np.float64) if mu else None
        o_v0 = np.empty(n, dtype=np.float64) if var0 else None
        o_v = np.empty(n, dtype=np.float64) if var else None
        o_c = np.empty((n, max(ldc, 1)), dtype=np.float64) if cov else None
        check(lib().mfgp_query(self.handle, _addr(Xq), n, _addr(XL), XL.shape[0], _addr(XH), XH.shape[0],
                               _addr(o_mu), _addr(o_v0), _addr(o_v), _addr(o_c), ldc))
        return QueryResult(o_mu, o_v0, o_v, None if o_c is None else o_c[:, :n])

    SAMPLE_DIMS = ("nz", "M", "N", "fields", "rx0", "ry0", "rx1", "ry1")
    STATS_KEYS = ("factor_rows", "v_rows", "full_factor", "inc_factor", "full_predict", "vstream",
                  "lattice_nx", "lattice_ny", "lattice", "lattice_virtual", "lattice_arg", "lattice_g2",
                  "post_copy", "early_pd", "look_border", "look_query", "sample_solve", "sample_gemm",
                  "lattice_vcol", "vcol_rows_built")

    def sample_dims(self, prior=False):
        """{nz, M, N, fields, rx0, ry0, rx1, ry1} of sample() (mfgp_sample_dims): nz normals
        per sample = field 0's rx0 x ry0 block, field 1's rx1 x ry1 (MF), then one per
        training row (none with prior). Settles the model as sample() does."""
        out = (ctypes.c_int64 * 8)()
        check(lib().mfgp_sample_dims(self.handle, out, 8, SAMPLE_PRIOR if prior else 0))
        return dict(zip(self.SAMPLE_DIMS, (int(v) for v in out)))

    def sample(self, normals, prior=False, out=None, ldz=None, ldo=None, S=None):
        """Pathwise joint samples on the whole lattice grid (mfgp_sample_posterior): [S, M],
        row s the sample of normals[s] ([S, >= nz] float64 standard normals, sample_dims()).
        prior: zero-mean draws of the hifi prior (no data involved). out: a host float64
        matrix [>= S, >= M] to fill in place (its row stride is the leading dimension).
        With normals / out as integer device addresses give S and ldz / ldo (returns None
        for a device out). A sample's bits depend on its own normals only."""
        L = lib()
        M = L.mfgp_model_m(self.handle)
        flags = SAMPLE_PRIOR if prior else 0
        if isinstance(normals, (int, np.integer)):
            if S is None or ldz is None:
                raise ValueError("device normals need S and ldz")
            zp, S, ldz = ctypes.c_void_p(int(normals)), int(S), int(ldz)
        else:
            z = np.asarray(normals, dtype=np.float64)
            if z.ndim != 2:
                raise ValueError("normals must be [S, >= nz]")
            if z.strides[1] != 8 or z.strides[0] % 8 or z.strides[0] < 8 * z.shape[1]:
                z = np.ascontiguousarray(z)
            S = z.shape[0] if S is None else int(S)
            if S > z.shape[0]:
                raise ValueError("S exceeds the rows of normals")
            ldz = (z.strides[0] // 8 if z.shape[0] > 1 else z.shape[1]) if ldz is None else int(ldz)
            zp = _addr(z)
        if isinstance(out, np.ndarray):
            _, ld = _host_out(out, True, S, 0, "out must be a writable row-major float64 matrix of at least [S] rows")
            res, o_p = out[:S, :M], _addr(out)
        elif out is not None:
            res, o_p, ld = None, ctypes.c_void_p(int(out)), M
        else:
            buf = np.empty((S, max(M, 1)), dtype=np.float64)
            res, o_p, ld, ldo = buf[:, :M], _addr(buf), max(M, 1), None
        check(L.mfgp_sample_posterior(self.handle, zp, S, ldz, o_p, int(ld if ldo is None else ldo), flags))
        return res

    def serial(self):
        """The model's posterior serial (mfgp_model_serial): changes whenever its rows,
        hyperparameters, jitter or grid change, and never repeats."""
        v = ctypes.c_uint64(0)
        check(lib().mfgp_model_serial(self.handle, ctypes.byref(v)))
        return int(v.value)

    def factor(self):
        n = lib().mfgp_model_n(self.handle)
        L = np.zeros((n, n), dtype=np.float64)
        if n:
            check(lib().mfgp_get_factor(self.handle, ptr(L)))
        return L

    @property
    def n(self):
        return lib().mfgp_model_n(self.handle)

    def stats(self):
        """{factor_rows, v_rows, full_factor, inc_factor, full_predict, vstream} (path
        counters; vstream counts every one-pass predict, lattice steps included), the
        grid's lattice axes {lattice_nx, lattice_ny} (0: not a lattice) and {lattice}:
        the steps that took the lattice-separable path (k_inc_lat); {lattice_virtual}: the
        off-lattice training rows (extra K rows) the last lattice step ran, as its
        device counters hold them (MF: summed over both kernel parts); {lattice_arg}:
        the lattice steps launched with their descriptors by value (k_inc_lat_arg);
        {lattice_g2}: the lattice steps whose GEMM and cells ran as a second launch
        (k_lat_gemm2); {post_copy}: batch predicts served from the resident posterior
        because the model appended nothing (k_post_copy); {early_pd}: eager appends that
        returned at the launch's published L22 verdict (mfgp_append, one GP);
        {look_border, look_query}: the k_look_border / k_look_query launches of query();
        {sample_solve, sample_gemm}: the k_sample_solve / k_sample_gemm launches of sample();
        {lattice_vcol}: the lattice steps whose w units read the column store of V;
        {vcol_rows_built}: the rows its catch-up (k_vcol_build) transposed into it."""
        out = (ctypes.c_int64 * len(self.STATS_KEYS))()
        check(lib().mfgp_model_stats(self.handle, out, len(self.STATS_KEYS)))
        return dict(zip(self.STATS_KEYS, (int(v) for v in out)))

    def debug_read_v(self):
        """Tests only: (V [n, M], Vc [M, n] or None, the store's valid rows): the resident V's
        rows and the column store's, as float64."""
        n, M = int(self.n), int(lib().mfgp_model_m(self.handle))
        v = np.zeros((max(n, 1), max(M, 1)), dtype=np.float64)
        vc = np.zeros((max(M, 1), max(n, 1)), dtype=np.float64)
        rows, vcr = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().mfgp_debug_read_v(self.handle, ptr(v), None, n, ctypes.byref(rows), ctypes.byref(vcr)))
        r = rows.value
        vc = np.zeros((max(M, 1), max(r, 1)), dtype=np.float64)
        check(lib().mfgp_debug_read_v(self.handle, None, ptr(vc), n, ctypes.byref(rows), ctypes.byref(vcr)))
        return v[:r, :M], (vc[:M, :r] if vcr.value > 0 else None), int(vcr.value)

    def debug_read_f(self):
        """Tests only: the explicit inverse F = L^-1 the lattice steps keep, [n, n] float64
        (n = 0: the model holds no current one)."""
        n = int(self.n)
        f = np.zeros((max(n, 1), max(n, 1)), dtype=np.float64)
        rows = ctypes.c_int64(0)
        check(lib().mfgp_debug_read_f(self.handle, ptr(f), n, ctypes.byref(rows)))
        r = rows.value
        if r == n:
            return f[:n, :n]
        g = np.zeros((max(r, 1), max(r, 1)), dtype=np.float64)
        if r:
            check(lib().mfgp_debug_read_f(self.handle, ptr(g), r, ctypes.byref(rows)))
        return g[:r, :r]

    def sample_points(self, threshold, max_points):
        """compute_sample_points (simulator.py:326-374) on a device copy of this model:
        the [n, 2] grid cells chosen until max var <= threshold (at most max_points)."""
        pts = np.empty((max(int(max_points), 1), 2), dtype=np.float64)
        n = ctypes.c_int64(0)
        check(lib().mfgp_sample_points(self.handle, float(threshold), int(max_points), ptr(pts), ctypes.byref(n)))
        return pts[:n.value].copy()

    def nlml(self, hyp, grad=False):
        """likelihood (gp:81-106 / 344-385) of this model's data under `hyp`; with grad, (value, gradient)."""
        h = np.ascontiguousarray(hyp, dtype=np.float64).reshape(-1)
        v = ctypes.c_double(0.0)
        g = np.empty(h.shape[0], dtype=np.float64) if grad else None
        check(lib().mfgp_nlml(self.handle, ptr(h), int(h.shape[0]), ctypes.byref(v),
                              ctypes.c_void_p(g.ctypes.data) if grad else None))
        return (v.value, g) if grad else v.value

    def nlml_batch(self, hyps, grad=False, status=False):
        """nlml for the S rows of hyps [S, nhyp] in one set of launches per chunk
        (mfgp_nlml_batch): values [S], then grads [S, nhyp] if grad, then status [S] (int)
        if status. Row s has the bits of nlml(hyps[s], grad). With status, a row that is
        not positive definite gets status > 0 (the order of the failing leading minor) and
        NaN outputs; without it, such a row raises LinAlgError."""
        h = np.ascontiguousarray(hyps, dtype=np.float64)
        if h.ndim != 2:
            raise ValueError("hyps must be [S, nhyp]")
        S, nhyp = h.shape
        v = np.empty(S, dtype=np.float64)
        g = np.empty((S, nhyp), dtype=np.float64) if grad else None
        st = np.zeros(S, dtype=np.intc) if status else None
        # (ptr() gives None for an empty array: pass the addresses themselves)
        check(lib().mfgp_nlml_batch(self.handle, ctypes.c_void_p(h.ctypes.data), int(S), int(nhyp),
                                    ctypes.c_void_p(v.ctypes.data),
                                    ctypes.c_void_p(g.ctypes.data) if grad else None,
                                    ctypes.c_void_p(st.ctypes.data) if status else None))
        out = (v,) + ((g,) if grad else ()) + ((st.astype(np.int64),) if status else ())
        return out if len(out) > 1 else v

    def truncate(self, n_keep_hifi):
        check(lib().mfgp_truncate(self.handle, int(n_keep_hifi)))


def sample_axis_factor(axis, lengthscale):
    """mfgp_sample_axis_factor (host only): (A [n, rank], rank), the pivoted-Cholesky
    factor of the unit-diagonal SE Gram of the axis values at that length scale."""
    a = np.ascontiguousarray(np.asarray(axis, dtype=np.float64).reshape(-1))
    n = a.shape[0]
    A = np.zeros((n, n), dtype=np.float64)
    r = ctypes.c_int(0)
    check(lib().mfgp_sample_axis_factor(ctypes.c_void_p(a.ctypes.data), n, float(lengthscale),
                                        ctypes.c_void_p(A.ctypes.data), ctypes.byref(r)))
    return A[:, :r.value].copy(), int(r.value)


def batch_append_predict(models, X, y, k, mu_ptr, var_ptr, asynchronous=False, vmax_ptr=None, vargmax_ptr=None):
    """Batched update+predict over device-resident models.

    X, y: integer device (or host) addresses of the concatenated new rows;
    k: per-model row counts; mu_ptr/var_ptr: device addresses of [sum M] outputs;
    vmax_ptr / vargmax_ptr: optional device addresses of [n] float64 / int64 outputs
    (fused np.amax / np.argmax of each model's variance; without them the _ex entry point
    is mfgp_batch_append_predict itself).
    """
    Batch(models, k).append_predict(X, y, mu_ptr, var_ptr, asynchronous, vmax_ptr, vargmax_ptr)


class Batch:
    """A fixed list of models with its handle / row-count arrays built once: the
    per-step calls of a seed ensemble without rebuilding ctypes arrays."""

    def __init__(self, models, k):
        self.models = list(models)
        self.n = len(self.models)
        self.arr = _handles(self.models)
        self.ks = (ctypes.c_int64 * self.n)(*[int(v) for v in k])

    def truncate(self, n_keep_hifi):
        check(lib().mfgp_batch_truncate(self.arr, self.n, int(n_keep_hifi)))

    def append_predict(self, X, y, mu_ptr, var_ptr, asynchronous=False, vmax_ptr=None, vargmax_ptr=None):
        check(lib().mfgp_batch_append_predict_ex(self.arr, self.n, ctypes.c_void_p(X), ctypes.c_void_p(y), self.ks,
                                                 ctypes.c_void_p(mu_ptr), ctypes.c_void_p(var_ptr),
                                                 ctypes.c_void_p(vmax_ptr), ctypes.c_void_p(vargmax_ptr),
                                                 ASYNC if asynchronous else 0))


def batch_append_factor(models, X, y, k, asynchronous=False):
    """Append + refactor a batch (device or host row pointers); no predict."""
    b = Batch(models, k)
    check(lib().mfgp_batch_append_factor(b.arr, b.n, ctypes.c_void_p(X), ctypes.c_void_p(y), b.ks,
                                         ASYNC if asynchronous else 0))


def batch_sample_points(models, thresholds, max_points):
    """mfgp_batch_sample_points: compute_sample_points (simulator.py:326-374) for every
    model of the batch, stepped together -> one [n_b, 2] array of chosen cells per model."""
    n = len(models)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (n,)))
    P = max(int(max_points), 1)
    pts = np.empty((n, P, 2), dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int64)
    check(lib().mfgp_batch_sample_points(_handles(models), n, ptr(thr), int(max_points), ptr(pts), ptr(cnt)))
    return [pts[b, :cnt[b]].copy() for b in range(n)]


def _per_member(v, n):
    """None, one value for all members, or one per member -> a list of n entries (None: None).
    One per member: a list / tuple of n array-likes, or a 2-D array of n rows."""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        if v.ndim == 2:
            if v.shape[0] != n:
                raise ValueError(f"one row per member expected: {n} rows (got {v.shape[0]})")
            return [v[b] for b in range(n)]
        return [v] * n
    v = list(v)
    if len(v) == n and all(np.ndim(e) >= 1 for e in v):
        return v
    if any(np.ndim(e) >= 1 for e in v):
        raise ValueError(f"one entry per member expected: {n} (got {len(v)})")
    return [v] * n


def batch_plan_ivr(models, n_points, weights=None, cand=None, groups=None, quota=None, min_gain=0.0, refresh=0):
    """mfgp_batch_plan_ivr: the greedy integrated-variance planner (Model.plan_ivr) for every
    model of the batch, stepped together -> a list of (cells [n_b] int64, pos [n_b] int64,
    points [n_b, 2], gains [n_b]) per member; pos[t] is pick t's position in the member's
    candidate list. weights: None (ones), one [>= largest M] vector for all, one per member
    (a list or [count, >= largest M]), or a contiguous float64 device tensor [count, ld].
    cand: None (all cells), one list for all, or one per member. groups: None (no constraint)
    or, parallel to cand (to 0 .. M - 1 where cand is None), the group in [0, ngroups) of every
    candidate position, one list for all or one per member; a member makes at most quota[g]
    picks (quota None: 1) in group g. The models are unchanged; their loop is counted in
    Context.planner_stats()."""
    L = lib()
    models = list(models)
    n = len(models)
    n_points = int(n_points)
    Ms = [int(L.mfgp_model_m(m.handle)) for m in models]
    maxM = max(Ms) if Ms else 0
    keep = []   # the arrays the call reads
    if weights is None:
        wp, ldw = None, maxM
    elif hasattr(weights, "data_ptr"):
        shape, stride = tuple(weights.shape), tuple(weights.stride())
        if str(getattr(weights, "dtype", "")).rsplit(".", 1)[-1] != "float64" or len(shape) != 2 or shape[0] != n or \
                (shape[1] > 1 and stride[1] != 1):
            raise ValueError("weights must be a float64 tensor [count, >= M] with contiguous rows")
        wp, ldw = ctypes.c_void_p(int(weights.data_ptr())), int(stride[0])
    else:
        rows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in _per_member(weights, n)]
        ldw = max([maxM] + [r.shape[0] for r in rows])
        wa = np.zeros((n, ldw), dtype=np.float64)
        for b, r in enumerate(rows):
            if r.shape[0] < Ms[b]:
                raise ValueError(f"weights of member {b} must be [>= M] with M = {Ms[b]} (ldw = {r.shape[0]})")
            wa[b, :r.shape[0]] = r
        keep.append(wa)
        wp = _addr(wa)
    lists = _per_member(cand, n)
    cp = op = None
    if lists is not None:
        lists = [np.ascontiguousarray(np.asarray(v, dtype=np.int64).reshape(-1)) for v in lists]
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([v.shape[0] for v in lists])
        ca = np.ascontiguousarray(np.concatenate(lists)) if n else np.zeros(0, dtype=np.int64)
        keep += [ca, off]
        cp, op = _addr(ca), _addr(off)
    sizes = Ms if lists is None else [v.shape[0] for v in lists]
    gp_, qp, ngroups = None, None, 0
    gl = _per_member(groups, n)
    if gl is not None:
        gl = [np.asarray(v, dtype=np.int64).reshape(-1) for v in gl]
        for b, v in enumerate(gl):
            if v.shape[0] != sizes[b]:
                raise ValueError(f"groups of member {b}: {sizes[b]} entries expected, one per candidate position "
                                 f"(got {v.shape[0]})")
        ga64 = np.concatenate(gl) if n else np.zeros(0, dtype=np.int64)
        ga = np.ascontiguousarray(np.clip(ga64, -1, 2 ** 31 - 1).astype(np.int32))
        keep.append(ga)
        gp_ = _addr(ga)
        if quota is not None:
            qa = np.ascontiguousarray(np.asarray(quota, dtype=np.int64).reshape(-1))
            keep.append(qa)
            qp, ngroups = _addr(qa), qa.shape[0]
        else:
            ngroups = int(ga64.max()) + 1 if ga64.size else 1
    elif quota is not None:
        raise ValueError("quota needs groups")
    P = max(n_points, 1)
    cells = np.empty((n, P), dtype=np.int64)
    pos = np.empty((n, P), dtype=np.int64)
    pts = np.empty((n, P, 2), dtype=np.float64)
    gains = np.empty((n, P), dtype=np.float64)
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    check(L.mfgp_batch_plan_ivr(_handles(models), n, wp, ldw, cp, op, gp_, qp, ngroups, n_points, float(min_gain),
                                int(refresh), _addr(cells), _addr(pos), _addr(pts), _addr(gains), _addr(cnt)))
    return [(cells[b, :cnt[b]].copy(), pos[b, :cnt[b]].copy(), pts[b, :cnt[b]].copy(), gains[b, :cnt[b]].copy())
            for b in range(n)]


def batch_predict(models, mu_ptr, var_ptr, asynchronous=False):
    """Posterior mean / variance of a batch from its current factors."""
    check(lib().mfgp_batch_predict(_handles(models), len(models), ctypes.c_void_p(mu_ptr), ctypes.c_void_p(var_ptr),
                                   ASYNC if asynchronous else 0))


def cell_reduce(grid, verts, vstart, seeds, w=None, f=None, var=None, ctx=None):
    """mfgp_cell_reduce on host arrays -> (out [n, 6], argmax [n]); see include/mfgp_hip.h."""
    ctx = ctx or context()
    g = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1, 2)
    v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 2)
    vs = np.ascontiguousarray(vstart, dtype=np.int32).reshape(-1)
    sd = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 2)
    n = vs.shape[0] - 1
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (w, f, var)]
    out = np.empty((max(n, 1), 6), dtype=np.float64)
    am = np.empty(max(n, 1), dtype=np.int64)
    check(lib().mfgp_cell_reduce(ctx.handle, ptr(g), g.shape[0], n, ctypes.c_void_p(vs.ctypes.data), ptr(v), ptr(sd),
                                 *[ptr(a) for a in arrs], ctypes.c_void_p(out.ctypes.data),
                                 ctypes.c_void_p(am.ctypes.data)))
    return out[:n], am[:n]


def batch_cell_reduce(grid, verts, vstart, seeds, field, nfield, w=None, f=None, var=None, ctx=None, M=None):
    """mfgp_batch_cell_reduce -> (out [n, 6], argmax [n]). verts / seeds / vstart /
    field are host arrays; grid a host array [M, 2] or (with M) the integer device
    address of one; w and var host arrays [nfield, M] or integer device addresses
    of [nfield * M] float64 (a batch's predict outputs); f a host array [M] or a
    device address."""
    ctx = ctx or context()
    keep = []

    def arg(a):
        if a is None:
            return None
        if isinstance(a, int):
            return ctypes.c_void_p(a)
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        keep.append(a)
        return ptr(a)
    if isinstance(grid, int):
        if M is None:
            raise ValueError("a device grid needs M")
        g_arg, Mg = ctypes.c_void_p(grid), int(M)
    else:
        g = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1, 2)
        g_arg, Mg = ptr(g), g.shape[0]
        keep.append(g)
    v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 2)
    vs = np.ascontiguousarray(vstart, dtype=np.int32).reshape(-1)
    fd = np.ascontiguousarray(field, dtype=np.int32).reshape(-1)
    sd = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 2)
    n = vs.shape[0] - 1
    if fd.shape[0] != n:
        raise ValueError("field needs one entry per cell")
    out = np.empty((max(n, 1), 6), dtype=np.float64)
    am = np.empty(max(n, 1), dtype=np.int64)
    check(lib().mfgp_batch_cell_reduce(ctx.handle, g_arg, Mg, n, ctypes.c_void_p(vs.ctypes.data), ptr(v),
                                       ptr(sd), ctypes.c_void_p(fd.ctypes.data), int(nfield), arg(w), arg(f), arg(var),
                                       ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(am.ctypes.data)))
    return out[:n], am[:n]
