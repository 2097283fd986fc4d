"""ctypes binding of libscsopt (include/scsopt.h).

The library is built in-tree (``make -C selfconcordantsmoothoptimization.jl_amd/csrc``)
and is the only compute path: nothing here falls back to a CPU
implementation.  If the shared object is missing, importing this module
raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCSOPT_LIB", os.path.join(_HERE, "libscsopt.so"))

SCS_OK, SCS_ERR_ARG, SCS_ERR_HIP, SCS_ERR_SOLVE, SCS_ERR_STATE, SCS_ERR_REF, SCS_ERR_COMM, SCS_ERR_CALLBACK = range(8)
SCS_MULTI_HOST_EXCHANGE = 1   # scs_create_multi_ex flag
SCS_CB_F, SCS_CB_GRAD, SCS_CB_HESS, SCS_CB_GGN, SCS_CB_FTEST, SCS_CB_GRAD_X = range(6)
SCS_CB_NO_METHOD = 2   # a callback's answer to SCS_CB_GRAD_X when grad_fx takes no single argument

SCS_SW_VALUE, SCS_SW_D1, SCS_SW_D2, SCS_SW_GGN = 1, 2, 4, 8   # scs_samplewise_fn's `what` bits

LOSS = {"logistic_margin": 1, "logistic_ce": 2, "least_squares": 3, "quadratic": 4, "rosenbrock": 5, "callback": 6,
        "samplewise": 7, "softmax_ce": 8, "multi_least_squares": 9}
GGN = {None: 0, "sigmoid_ce": 1, "linear_ls": 2, "samplewise": 3, "linear_softmax_ce": 4, "linear_multi_ls": 5}
REG = {"l1": 1, "l2": 2, "indbox": 3, "gl": 4}
SMOOTH = {"phuber_l1l2": 1, "phuber_indbox": 2, "phuber_gl": 3, "exp_indbox": 4, "logexp_indbox": 5, "osba_l1l2": 6,
          "osba_gl": 7}
METHOD = {"nscore": 1, "ggnscore": 2, "lqnscore": 3}
SOLVER = {"default": 0, "reference": 1}

# One HIP runtime per process.  The product needs no torch: without it, libscsopt binds
# /opt/rocm's HIP runtime and RCCL (preloaded RTLD_GLOBAL below).  torch's wheel bundles its own
# copies, whose NEEDED names ("libamdhip64.so") differ from their SONAMEs ("libamdhip64.so.7"):
# a torch imported AFTER /opt/rocm's runtime is bound would load a second runtime.  So when torch
# is already imported (the tests, torch.distributed users), libscsopt's NEEDED entries resolve to
# torch's loaded copies (same SONAMEs) instead, and scsopt.shard refuses to import torch late.
if "torch" in sys.modules:
    RUNTIME = "torch"
else:
    _ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
    for _so in ("libamdhip64.so.7", "librccl.so.1"):
        _p = os.path.join(_ROCM, "lib", _so)
        if os.path.exists(_p):
            C.CDLL(_p, mode=C.RTLD_GLOBAL)
    RUNTIME = "rocm"


def require_torch_runtime(what):
    """torch may join the process only when libscsopt is bound to torch's runtime.  With RUNTIME ==
    "rocm" /opt/rocm's HIP runtime is already bound, and a torch imported since (or imported by the
    caller of `what`) brings its own second copy -- refused either way."""
    if RUNTIME == "rocm":
        late = "torch" in sys.modules
        raise ImportError(f"{what} needs torch, but scsopt was imported first and bound /opt/rocm's HIP runtime"
                          + (" (torch was imported after scsopt: the process now holds two HIP runtimes)"
                             if late else "") + "; import torch before scsopt in a process that uses torch")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"libscsopt.so not found at {LIB_PATH}: build it with "
        "`make -C selfconcordantsmoothoptimization.jl_amd/csrc` (there is no CPU fallback)")

lib = C.CDLL(LIB_PATH)

c_dp = C.POINTER(C.c_double)
c_i64p = C.POINTER(C.c_int64)
c_i32p = C.POINTER(C.c_int32)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
LOSS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, c_dp, C.c_int64, c_dp)
# (user, what, n, z, y, val, d1, d2, s, stream): plain addresses, host or device (scs_set_loss_samplewise)
SAMPLEWISE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p)


class Synth(C.Structure):
    _fields_ = [("N_global", C.c_int64), ("row0", C.c_int64), ("N", C.c_int64), ("m", C.c_int64),
                ("seed", C.c_uint64), ("kind", C.c_int), ("density", C.c_double)]


class Timing(C.Structure):
    _fields_ = [("gram_ms", C.c_double), ("gram_calls", C.c_int64),
                ("gemv_ms", C.c_double), ("gemv_calls", C.c_int64),
                ("solve_ms", C.c_double), ("solve_calls", C.c_int64),
                ("step_ms", C.c_double), ("step_calls", C.c_int64),
                ("reduce_ms", C.c_double), ("reduce_calls", C.c_int64)]


class History(C.Structure):
    _fields_ = [("obj", C.POINTER(C.c_double)), ("fval", C.POINTER(C.c_double)),
                ("pri_res_norm", C.POINTER(C.c_double)), ("rel", C.POINTER(C.c_double)),
                ("objrel", C.POINTER(C.c_double)), ("times", C.POINTER(C.c_double)),
                ("fvaltest", C.POINTER(C.c_double))]


_SIGS = {
    "scs_version": (C.c_char_p, []),
    "scs_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "scs_destroy": (C.c_int, [C.c_void_p]),
    "scs_create_multi": (C.c_int, [c_i32p, C.c_int, C.POINTER(C.c_void_p)]),
    "scs_create_multi_ex": (C.c_int, [c_i32p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "scs_group_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "scs_last_error": (C.c_char_p, [C.c_void_p]),
    "scs_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "scs_set_comm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]),
    "scs_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "scs_set_comm_rccl": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "scs_set_comm_force": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_reduce_buffer_size": (C.c_int, [C.c_void_p, c_i64p]),
    "scs_set_reduce_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "scs_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_int), C.c_char_p, C.c_int64]),
    "scs_set_outputs": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_sparse_outputs": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_multi_sample": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_multi_batches": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_multi_sparse_batches": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_get_outputs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), c_i64p]),
    "scs_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, c_dp, C.c_int64, c_dp, C.c_int64, C.c_int64]),
    "scs_gen_data": (C.c_int, [C.c_void_p, C.POINTER(Synth)]),
    "scs_set_dense_f32": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_data_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_dp, C.c_int64,
                                   C.c_int64]),
    "scs_data_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), c_i64p, c_i64p]),
    "scs_set_data_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "scs_get_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, c_dp, C.c_int64, c_dp]),
    "scs_get_dims": (C.c_int, [C.c_void_p, c_i64p, c_i64p, c_i64p, c_i64p]),
    "scs_set_test_data": (C.c_int, [C.c_void_p, C.c_int64, c_dp, C.c_int64, c_dp, C.c_int64, C.c_int64]),
    "scs_set_test_data_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_dp, C.c_int64, C.c_int64]),
    "scs_set_test_data_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "scs_set_test_sparse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, c_i64p, c_i32p, c_dp, C.c_int, c_dp,
                                      C.c_int64, C.c_int64]),
    "scs_gen_test_data": (C.c_int, [C.c_void_p, C.POINTER(Synth)]),
    "scs_set_test_callback": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_eval_ftest": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "scs_has_test": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "scs_set_sparse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, c_i64p, c_i32p, c_dp, c_i64p, c_i32p,
                                 c_dp, C.c_int, c_dp, C.c_int64, C.c_int64]),
    "scs_gen_sparse": (C.c_int, [C.c_void_p, C.POINTER(Synth), C.c_int]),
    "scs_get_nnz": (C.c_int, [C.c_void_p, c_i64p]),
    "scs_get_sparse": (C.c_int, [C.c_void_p, c_i64p, c_i32p, c_dp]),
    "scs_get_sparse_csc": (C.c_int, [C.c_void_p, c_i64p, c_i32p, c_dp]),
    "scs_set_sparse_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_int64]),
    "scs_set_test_sparse_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_int64]),
    "scs_set_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "scs_set_loss_callback": (C.c_int, [C.c_void_p, LOSS_FN, C.c_void_p, C.c_int64]),
    "scs_set_loss_samplewise": (C.c_int, [C.c_void_p, SAMPLEWISE_FN, C.c_void_p, C.c_int, C.c_int]),
    "scs_set_reg": (C.c_int, [C.c_void_p, C.c_int, c_dp, C.c_int, c_dp, c_dp, C.c_int64, c_i64p, C.c_int64]),
    "scs_set_smoother": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, c_dp, c_dp,
                                   C.c_int64]),
    "scs_set_L": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "scs_method_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "scs_eval_f": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "scs_eval_grad": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "scs_eval_reg": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "scs_set_gram_cache": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_solver": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_compute_f32": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_group_map": (C.c_int, [C.c_void_p, c_i64p, C.c_int64]),
    "scs_set_batches": (C.c_int, [C.c_void_p, c_i64p, c_i64p, C.c_int64]),
    "scs_select_batch": (C.c_int, [C.c_void_p, C.c_int64]),
    "scs_get_batch_data": (C.c_int, [C.c_void_p, C.c_int64, c_dp, C.c_int64, c_dp]),
    "scs_set_sparse_batches": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_set_sparse_sample": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_batch_info": (C.c_int, [C.c_void_p, c_i64p, c_i64p, c_i64p]),
    "scs_step": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, c_dp, c_dp, c_dp]),
    "scs_step_grad": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, c_dp, c_dp, c_dp, c_dp]),
    "scs_iterate": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, C.c_double, C.c_double, C.c_int, c_dp,
                              C.POINTER(History), c_i64p, c_i64p]),
    "scs_iterate_ex": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, C.c_double, C.c_double, C.c_int, c_dp,
                                 C.POINTER(History), C.c_size_t, c_i64p, c_i64p]),
    "scs_smoother_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, c_dp]),
    "scs_prox_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_double, C.c_double, c_dp]),
    "scs_gram_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64]),
    "scs_sample_gram_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64]),
    "scs_sample_system_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, c_dp]),
    "scs_gemv_t_eval": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "scs_gemv_n_eval": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "scs_solve_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, c_dp, C.c_int, c_dp, C.POINTER(C.c_int)]),
    "scs_lu_eval": (C.c_int, [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_i32p, C.POINTER(C.c_int)]),
    "scs_chol_eval": (C.c_int, [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_dp, C.POINTER(C.c_int)]),
    "scs_qr_eval": (C.c_int, [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_dp]),
    "scs_get_columns": (C.c_int, [C.c_void_p, c_i64p, C.c_int64, c_dp]),
    "scs_gram_atv_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, c_i64p, C.c_int64, c_dp, c_dp, C.POINTER(C.c_int)]),
    "scs_multi_products_eval": (C.c_int, [C.c_void_p, C.c_int, c_dp, c_dp, c_dp, c_dp]),
    "scs_multi_system_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, c_dp, c_dp]),
    "scs_multi_sample_system_eval": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_int64, c_dp]),
    "scs_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "scs_timing_get": (C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    "scs_timing_reset": (C.c_int, [C.c_void_p]),
    "scs_fallback_counts": (C.c_int, [C.c_void_p, c_i64p, C.c_int]),
    "scs_kernel_names": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64]),
    "scs_sync": (C.c_int, [C.c_void_p]),
}

for _name, (_res, _args) in _SIGS.items():
    _f = getattr(lib, _name)  # AttributeError here = the .so does not export the header's symbol
    _f.restype = _res
    _f.argtypes = _args

EXPORTED = tuple(_SIGS)


class ScsError(RuntimeError):
    """A non-reference failure (HIP, argument, state, communication)."""

    def __init__(self, code, msg):
        super().__init__(f"[scsopt rc={code}] {msg}")
        self.code = code


class ScsReferenceError(ScsError):
    """An error the reference itself raises via Base.error (same message text)."""


def version():
    return lib.scs_version().decode()


def dptr(a):
    """Pointer to a C-contiguous float64 numpy array (or None)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "expected a contiguous float64 array"
    return a.ctypes.data_as(c_dp)


def is_device_array(a):
    """An object that exposes __cuda_array_interface__ (a torch-ROCm tensor, a CuPy array, ...)."""
    if a is None or isinstance(a, np.ndarray):
        return False
    try:   # a torch CPU tensor has the attribute and raises from it: a host array, as before
        return isinstance(a.__cuda_array_interface__, dict)
    except Exception:
        return False


def parse_device_matrix(iface):
    """A 2-D __cuda_array_interface__ dict -> what scs_set_data_device takes:
    {"ptr", "N", "m", "elem_bytes", "stride_n", "stride_m", "stream"}; strides in elements, one of them
    1.  "<f8" and "<f4" are accepted (anything else: TypeError); two non-unit strides raise ValueError
    -- the binding never copies silently.  strides = None means C-contiguous.  `stream` is the
    interface's value: None (the producer is done), 1 (the legacy default stream), 2 (the per-thread
    default stream) -- scs_set_data_device takes both as src_stream and resolves them itself -- or a
    stream handle."""
    typestr = iface["typestr"]
    if typestr not in ("<f8", "<f4"):
        raise TypeError(f"device array of type {typestr!r}: float64 ('<f8') or float32 ('<f4') is needed")
    es = 8 if typestr == "<f8" else 4
    shape = tuple(int(v) for v in iface["shape"])
    if len(shape) != 2:
        raise ValueError(f"a device matrix has two dimensions, this array has shape {shape}")
    N, m = shape
    strides = iface.get("strides")
    if strides is None:
        sn, sm = m, 1
    else:
        if any(int(b) % es for b in strides):
            raise ValueError(f"device array strides {tuple(strides)} are not multiples of the element size {es}")
        sn, sm = (int(b) // es for b in strides)
    # the stride of an extent-1 axis addresses nothing: take the contiguous value
    if N == 1 and sm != 1:
        sn = 1
    elif N == 1:
        sn = max(sn, m)
    if m == 1 and sn != 1:
        sm = 1
    elif m == 1:
        sm = max(sm, N)
    if sn != 1 and sm != 1:
        raise ValueError(f"device array with strides ({sn}, {sm}) elements: one axis must be contiguous -- pass "
                         "a contiguous array (x.contiguous() / cupy.ascontiguousarray); it is not copied here")
    if sn < 0 or sm < 0 or (sm == 1 and N > 1 and sn < m) or (sn == 1 and sm != 1 and m > 1 and sm < N):
        raise ValueError(f"device array with strides ({sn}, {sm}) elements overlaps itself for shape {shape}")
    ptr, _readonly = iface["data"]
    stream = iface.get("stream")
    if stream is not None and int(stream) == 0:
        raise ValueError("__cuda_array_interface__ forbids stream = 0 (1 and 2 name the default streams)")
    return {"ptr": int(ptr) if ptr else 0, "N": N, "m": m, "elem_bytes": es, "stride_n": sn, "stride_m": sm,
            "stream": None if stream is None else int(stream)}


def parse_device_targets(iface, n, k):
    """A device Y of a multi-output problem: n x k float64, column-major with leading dimension n (a
    Fortran-ordered array, or the transpose of a C-contiguous k x n one) -> its pointer."""
    if iface["typestr"] != "<f8":
        raise TypeError(f"a device Y must be float64, got {iface['typestr']!r}")
    shape = tuple(int(v) for v in iface["shape"])
    if shape != (n, k):
        raise ValueError(f"Y has shape {shape}, expected ({n}, {k})")
    strides = iface.get("strides")
    st = (8 * k, 8) if strides is None else tuple(int(b) for b in strides)
    if not ((n == 1 or st[0] == 8) and (k == 1 or st[1] == 8 * n)):
        raise ValueError(f"a device Y must be column-major with leading dimension N (strides (8, {8 * n}) bytes), got "
                         f"{st}: pass Y.t().contiguous().t() / cupy.asfortranarray(Y); it is not copied here")
    return int(iface["data"][0] or 0)


def parse_device_vector(iface, n):
    """A device y: n contiguous float64 -> its pointer."""
    if iface["typestr"] != "<f8":
        raise TypeError(f"a device y must be float64, got {iface['typestr']!r}")
    shape = tuple(int(v) for v in iface["shape"])
    if shape != (n,):
        raise ValueError(f"y has shape {shape}, expected ({n},)")
    strides = iface.get("strides")
    if strides is not None and n > 1 and int(strides[0]) != 8:
        raise ValueError("a device y must be contiguous")
    return int(iface["data"][0] or 0)


class DeviceVector:
    """n contiguous float64 at a device address, as __cuda_array_interface__ (version 2; stream None:
    the consumer orders its own work) -- what torch.as_tensor reads to alias the library's buffers
    for a device-mode sample-wise loss.  It owns nothing: the buffer belongs to the context.  (The
    read-only flag stays False, the only value torch accepts; z and y are inputs by contract.)"""

    def __init__(self, ptr, n):
        self.ptr, self.n = int(ptr), int(n)

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.n,), "typestr": "<f8", "data": (self.ptr, False), "version": 2, "strides": None}


def _is_torch_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "layout")


def is_device_csr(A):
    """A CSR matrix whose three arrays live on the GPU: a 2-D torch tensor with layout ==
    torch.sparse_csr on a GPU, or any object with indptr / indices / data / shape whose arrays expose
    __cuda_array_interface__ (CuPy's csr_matrix).  A torch sparse tensor this door cannot take raises
    ValueError with what to call instead: a COO (or CSC / blocked) layout, a batched CSR, a CPU tensor."""
    if A is None or isinstance(A, np.ndarray):
        return False
    if _is_torch_tensor(A):
        torch = sys.modules["torch"]
        if A.layout == torch.strided:
            return False
        if A.layout != torch.sparse_csr:
            raise ValueError(f"a torch sparse tensor with layout {A.layout}: the device door takes CSR -- call "
                             "A.to_sparse_csr() first")
        if A.dim() != 2:
            raise ValueError(f"a batched CSR tensor of shape {tuple(A.shape)}: pass one 2-D matrix (A[i]) per "
                             "problem")
        if not A.is_cuda:
            raise ValueError("a CPU sparse torch tensor: move it to the GPU (A.to('cuda')) for the device door, "
                             "or pass a scipy.sparse matrix for the host door")
        return True
    try:
        parts = (A.indptr, A.indices, A.data)
        A.shape
    except AttributeError:
        return False
    return all(is_device_array(p) for p in parts)


def device_csr_arrays(A):
    """(shape, indptr, indices, data) of a matrix that passed is_device_csr; nothing is copied."""
    if _is_torch_tensor(A):
        return tuple(A.shape), A.crow_indices(), A.col_indices(), A.values()
    return tuple(A.shape), A.indptr, A.indices, A.data


def _parse_csr_array(iface, name, types, n):
    typestr = iface["typestr"]
    if typestr not in types:
        raise TypeError(f"device CSR {name} of type {typestr!r}: one of {sorted(types)} is needed")
    es = types[typestr]
    shape = tuple(int(v) for v in iface["shape"])
    if shape != (n,):
        raise ValueError(f"device CSR {name} has shape {shape}, expected ({n},)")
    strides = iface.get("strides")
    if strides is not None and n > 1 and int(strides[0]) != es:
        raise ValueError(f"device CSR {name} must be contiguous (stride {int(strides[0])} bytes for {es}-byte "
                         "elements); it is not copied here")
    ptr = iface["data"][0]
    stream = iface.get("stream")
    if stream is not None and int(stream) == 0:
        raise ValueError("__cuda_array_interface__ forbids stream = 0 (1 and 2 name the default streams)")
    return (int(ptr) if ptr else 0), es, (None if stream is None else int(stream))


def parse_device_csr(shape, iface_ptr, iface_idx, iface_val):
    """The matrix shape and the __cuda_array_interface__ dicts of indptr / indices / data -> what
    scs_set_sparse_device takes: {"rowptr", "ptr_bytes", "colidx", "idx_bytes", "val", "val_bytes", "N",
    "m", "nnz", "stream"}.  "<i4" / "<i8" index arrays and "<f4" / "<f8" values (anything else:
    TypeError), each contiguous, of lengths N + 1, nnz and nnz (ValueError otherwise); nothing is copied.
    With nnz = 0 the data pointers may be null.  `stream` is the first stream entry the three
    interfaces name (None, 1, 2 or a handle, as parse_device_matrix returns it)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2:
        raise ValueError(f"a device CSR matrix has two dimensions, this one has shape {shape}")
    N, m = shape
    nnz = int(tuple(iface_val["shape"])[0]) if len(tuple(iface_val["shape"])) == 1 else -1
    ints, floats = {"<i4": 4, "<i8": 8}, {"<f4": 4, "<f8": 8}
    rp, pb, s0 = _parse_csr_array(iface_ptr, "indptr", ints, N + 1)
    if nnz < 0:
        raise ValueError(f"device CSR data has shape {tuple(iface_val['shape'])}, expected one dimension")
    ci, ib, s1 = _parse_csr_array(iface_idx, "indices", ints, nnz)
    va, vb, s2 = _parse_csr_array(iface_val, "data", floats, nnz)
    stream = next((s for s in (s0, s1, s2) if s is not None), None)
    return {"rowptr": rp, "ptr_bytes": pb, "colidx": ci, "idx_bytes": ib, "val": va, "val_bytes": vb, "N": N, "m": m,
            "nnz": nnz, "stream": stream}


class Context:
    """Owns one scs_ctx: one device and stream (scs_create), or -- devices=[d0, d1, ...] -- one
    process driving several GPUs (scs_create_multi: the library splits the rows across them).
    device_exchange="host": the group's exchange through host memory instead of RCCL
    (SCS_MULTI_HOST_EXCHANGE; devices may repeat a GPU)."""

    def __init__(self, device=0, stream=None, devices=None, device_exchange="rccl"):
        h = C.c_void_p()
        if device_exchange not in ("rccl", "host"):
            raise ValueError("device_exchange is 'rccl' or 'host'")
        if devices is not None:
            devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            flags = SCS_MULTI_HOST_EXCHANGE if device_exchange == "host" else 0
            rc = lib.scs_create_multi_ex(devs, len(devices), flags, C.byref(h))
            if rc != SCS_OK:
                raise ScsError(rc, f"scs_create_multi_ex(devices={list(devices)}, {device_exchange}) failed")
            device = int(devices[0])
        else:
            rc = lib.scs_create(int(device), stream, C.byref(h))
            if rc != SCS_OK:
                raise ScsError(rc, f"scs_create(device={device}) failed")
        self.h = h
        self._pid = os.getpid()
        self.device = device
        self.devices = list(devices) if devices is not None else [device]
        self._keep = []  # ctypes callbacks / buffers that must outlive the context
        self._cb_exc = None  # the exception a Python loss callback raised (re-raised by check)

    def check(self, rc):
        if rc != SCS_OK:
            if rc == SCS_ERR_CALLBACK and self._cb_exc is not None:
                exc, self._cb_exc = self._cb_exc, None
                raise exc
            msg = lib.scs_last_error(self.h).decode(errors="replace")
            if rc == SCS_ERR_REF:
                raise ScsReferenceError(rc, msg)
            raise ScsError(rc, msg)

    def close(self):
        if getattr(self, "h", None):
            # a forked child (multiprocessing's fork start method, a Manager's server) inherits the object
            # but neither the HIP runtime's state nor a group's worker threads: the handle is the parent's
            if getattr(self, "_pid", None) == os.getpid():
                lib.scs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        s = C.c_void_p()
        self.check(lib.scs_get_stream(self.h, C.byref(s)))
        return s.value

    FALLBACKS = ("lu_coop_refused", "lu_coop_redo", "solve_blocks", "qr_blocks", "chain_redo", "pipe_redo",
                 "qr_coop_refused", "qr_coop_redo")

    def fallback_counts(self):
        """The fallbacks taken instead of failing since the context was created (scs_fallback_counts;
        SCS_FB_* in include/scsopt.h), as {name: count}."""
        n = len(self.FALLBACKS)
        out = (C.c_int64 * n)()
        self.check(lib.scs_fallback_counts(self.h, out, n))
        return dict(zip(self.FALLBACKS, (int(v) for v in out)))

    def kernel_names(self):
        """(main Gram kernel, sparse product kernel) of the latest launches, rocprofv3's names."""
        g, p = C.create_string_buffer(128), C.create_string_buffer(128)
        self.check(lib.scs_kernel_names(self.h, g, 128, p, 128))
        return g.value.decode(), p.value.decode()

    def comm_info(self):
        """What the exchange runs on, read back from the library (scs_comm_info): kind, the
        communicator's own rank count and rank (ncclCommCount / ncclCommUserRank for RCCL), the
        RCCL version and the path of the RCCL library the process resolved."""
        k, n, r, v = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        path = C.create_string_buffer(4096)
        self.check(lib.scs_comm_info(self.h, C.byref(k), C.byref(n), C.byref(r), C.byref(v), path, 4096))
        kinds = {0: "none", 1: "rccl", 2: "callback", 3: "group_rccl", 4: "group_host"}
        return {"kind": kinds.get(k.value, str(k.value)), "nranks": n.value, "rank": r.value,
                "rccl_version": v.value, "rccl_lib": path.value.decode(errors="replace")}

    def timing(self):
        t = Timing()
        self.check(lib.scs_timing_get(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timing._fields_}
