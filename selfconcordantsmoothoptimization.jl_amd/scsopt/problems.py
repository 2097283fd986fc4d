"""Problem containers (src/problems.jl) backed by a device context.

``Problem(A, y, x0, f, λ; ...)`` uploads A (column-major, the Julia Matrix
layout) and y to HBM once; ``Problem(x0, f, λ; ...)`` is the data-free
ProblemGeneric (problems.jl:44-59).  ``Problem.synthetic(...)`` generates A
and y on the device (counter-based RNG, any row shard in place), which is how
the BASELINE configurations are built without ever materialising A on the
host.  Row sharding: pass ``comm=shard.Comm(...)`` and the local rows.
"""
from __future__ import annotations

import ctypes as C
import sys
import logging
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np

from . import _lib
from ._lib import LOSS, GGN, REG, SMOOTH, dptr
from .losses import Loss, OutFn, ggn_kind
from .smoothers import Smoother, bounds_array

log = logging.getLogger("scsopt")


def _accepts_one_arg(fn):
    """Whether fn(x) binds: the Python reading of Julia's `applicable(grad_fx, x)` (a callable
    whose signature cannot be inspected is taken at its word and called)."""
    import inspect
    try:
        inspect.signature(fn).bind(None)
    except TypeError:
        return False
    except ValueError:
        return True
    return True


def _samplewise_put_host(dst, src, name):
    """A host-mode sample-wise callable's result into the library's output area: n numbers, or a
    scalar (broadcast); anything else raises (the device mode applies the same rule through copy_)."""
    src = np.asarray(src, dtype=np.float64)
    if src.ndim != 0 and src.shape != dst.shape:
        raise ValueError(f"samplewise: {name} returned shape {src.shape}, expected {dst.shape}")
    dst[...] = src


@dataclass
class GetP:
    """get_P(n, G, ind) (prox-reg-utils.jl:9-62): group structure for "gl".
    ind is 3 x grpNUM (1-based start, end; Int weight), its ranges partitioning
    1..n; G (1-based) maps the entries of P.matrix*x to variables -- a
    permutation of 1..n, read by get_reg only (the prox and the GL smoothers
    index x directly, as in the reference)."""
    n: int
    G: np.ndarray
    ind: np.ndarray

    def __post_init__(self):
        self.ind = np.asarray(self.ind, dtype=np.int64)
        self.G = np.asarray(self.G, dtype=np.int64)
        if self.ind.ndim != 2 or self.ind.shape[0] != 3:
            raise ValueError("ind must be a 3 x grpNUM integer matrix")
        self.grpNUM = int(self.ind.shape[1])
        self.grpSIZES = self.ind[1] - self.ind[0] + 1
        self.ntotal = int(self.grpSIZES.sum())
        if self.ntotal != self.n or self.G.shape != (self.n,) or \
                not np.array_equal(np.sort(self.G), np.arange(1, self.n + 1)):
            # get_Cmat / the GL smoothers raise DimensionMismatch for ntotal != n in the reference
            raise ValueError("gl groups must partition 1..n and G must be a permutation of 1..n")


def get_P(n, G, ind):
    return GetP(int(n), np.asarray(G), np.asarray(ind))


def _lam_tuple(lam):
    if isinstance(lam, (list, tuple, np.ndarray)):
        v = [float(t) for t in lam]
    else:
        v = [float(lam)]
    if len(v) not in (1, 2):
        raise ValueError("λ must be a scalar or a pair")
    return v


def _is_sparse(A):
    return hasattr(A, "tocsr") and hasattr(A, "tocsc") and hasattr(A, "nnz")


class Problem:
    """problems.jl:21-40 (data) / :5-19 (generic)."""

    def __init__(self, *args, Atest=None, ytest=None, L=None, sol=None, C_set=None, P=None,
                 out_fn: Optional[OutFn] = None, name=None, device=0, comm=None, N_global=None, row0=0,
                 sparse_f32=False, devices=None, device_exchange="rccl", Ntest_global=None, test_row0=0,
                 dense_f32=False, sparse_batches=False, sparse_sample=False, sparse_outputs=False, multi_sample=False,
                 multi_batches=False, multi_sparse_batches=False, _ctx=None):
        if len(args) == 5:
            A, y, x0, f, lam = args
        elif len(args) == 3:
            A, y = None, None
            x0, f, lam = args
        else:
            raise TypeError("Problem(A, y, x0, f, λ; ...) or Problem(x0, f, λ; ...)")
        if not isinstance(f, Loss):
            raise TypeError("f must be a scsopt.losses kind (device losses replace Julia closures)")
        self.x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
        self.m = int(self.x0.shape[0])
        self.f = f
        self.λ = lam
        self.L = L
        self.x = np.zeros(self.m) if sol is None else np.ascontiguousarray(np.asarray(sol, dtype=np.float64))
        self.C_set = C_set
        self.P = P
        self.out_fn = out_fn
        self.name = name
        self.comm = comm
        self.generic = A is None and _ctx is None
        # multi-output losses (losses.softmax_ce / multi_least_squares): K = nout outputs on one N x d A,
        # x = vec(X) with X d x K, Y N x K (scs_set_outputs)
        # sparse_outputs: a multi-output loss on a sparse A (scipy matrix or device CSR) -- the products run
        # with nout right-hand sides in one pass over the nonzeros (scs_set_sparse_outputs)
        self.sparse_outputs = bool(sparse_outputs)
        # multi_sample: with nout set and N·nout + 1 <= d·nout, ProxGGNSCORE runs the reference's sample-space
        # branch on the device (a dense A) instead of being refused (scs_set_multi_sample)
        if not isinstance(multi_sample, (bool, np.bool_)):
            raise TypeError(f"multi_sample must be a bool, got {type(multi_sample).__name__}")
        self.multi_sample = bool(multi_sample)
        if self.multi_sample and devices is not None:
            raise ValueError("multi_sample=True takes a single-device context: devices=[...] is not supported with "
                             "nout")
        # multi_batches: with nout set, minibatches (batch_size / slice_samples / set_batches) of a dense A are
        # gathered on the device instead of being refused (scs_set_multi_batches)
        if not isinstance(multi_batches, (bool, np.bool_)):
            raise TypeError(f"multi_batches must be a bool, got {type(multi_batches).__name__}")
        self.multi_batches = bool(multi_batches)
        if self.multi_batches and devices is not None:
            raise ValueError("multi_batches=True takes a single-device context: devices=[...] is not supported with "
                             "nout")
        # multi_sparse_batches: with nout and multi_batches set, minibatches of a sparse A (sparse_outputs) are
        # accepted as well: densified views, or sparse K-column views under ProxLQNSCORE with sparse_batches
        # (scs_set_multi_sparse_batches)
        if not isinstance(multi_sparse_batches, (bool, np.bool_)):
            raise TypeError(f"multi_sparse_batches must be a bool, got {type(multi_sparse_batches).__name__}")
        self.multi_sparse_batches = bool(multi_sparse_batches)
        if self.multi_sparse_batches and devices is not None:
            raise ValueError("multi_sparse_batches=True takes a single-device context: devices=[...] is not supported "
                             "with nout")
        self._sparse_batches = bool(sparse_batches)
        self._sparse_A = _lib.is_device_csr(A) or _is_sparse(A)
        self.nout = self._check_outputs(f, out_fn, A, comm, devices, _ctx)
        self.d = self.m // self.nout   # A's columns
        if f.kind == "callback":   # the data stays with the caller's closures; the device holds none
            if _ctx is not None or comm is not None:
                raise ValueError("a callback loss runs on one rank with host-side data")
            # y keeps its shape: an N x ny target is a multi-output problem (iterate.jl:105-107)
            self._cb_data = None if A is None else (A, np.asarray(y, dtype=np.float64))
            A, y, self.generic = None, None, True
        # a device CSR is asked for before _is_sparse: a CuPy csr_matrix has tocsr / tocsc / nnz as well
        dev_csr = _lib.is_device_csr(A)
        if devices is not None and (comm is not None or (_is_sparse(A) and not dev_csr)):
            raise ValueError("devices=[...] (one process, several GPUs) takes a dense A and no comm")
        if devices is not None and (_lib.is_device_array(A) or _lib.is_device_array(Atest) or dev_csr
                                    or _lib.is_device_csr(Atest)):
            raise ValueError("devices=[...] splits host rows across its GPUs: a device array lives on one of them "
                             "(pass a host array, or one process per GPU with a row slice each)")
        self.ctx = _ctx if _ctx is not None else _lib.Context(device, devices=devices, device_exchange=device_exchange)
        # dense_f32: a dense A (and dense held-out rows) stored as fp32 on the device, fp64 arithmetic --
        # bit for bit what the same values widened to fp64 give (scs_set_dense_f32)
        self.dense_f32 = bool(dense_f32)
        if sparse_batches:   # a mode of the context: set before any batch view exists
            self.ctx.check(_lib.lib.scs_set_sparse_batches(self.ctx.h, 1))
        if sparse_sample:
            self.ctx.check(_lib.lib.scs_set_sparse_sample(self.ctx.h, 1))
        if self.sparse_outputs:   # a mode of the context: inert without nout
            self.ctx.check(_lib.lib.scs_set_sparse_outputs(self.ctx.h, 1))
        if self.multi_sample:     # likewise inert without nout
            self.ctx.check(_lib.lib.scs_set_multi_sample(self.ctx.h, 1))
        if self.multi_batches:    # likewise
            self.ctx.check(_lib.lib.scs_set_multi_batches(self.ctx.h, 1))
        if self.multi_sparse_batches:   # likewise, and inert on a dense A
            self.ctx.check(_lib.lib.scs_set_multi_sparse_batches(self.ctx.h, 1))
        if self.nout > 1:   # before the data door: its m is then A's column count d, y is N x nout
            self.ctx.check(_lib.lib.scs_set_outputs(self.ctx.h, self.nout))
        if comm is not None and comm.active and _ctx is None:
            comm.attach(self.ctx)
        if _ctx is None:
            if self.generic:
                self.N = 0
                self.ctx.check(_lib.lib.scs_set_data(self.ctx.h, 0, self.m, None, 0, None, 0, 0))
            elif dev_csr:
                self.N = self._set_sparse_device(A, y, False, N_global, row0, bool(sparse_f32))
            elif _is_sparse(A):
                self._set_sparse(A, y, N_global, row0, f32=bool(sparse_f32))
            elif _lib.is_device_array(A):
                self.N = self._set_device(A, y, False, N_global, row0)
            elif self.nout > 1:
                self.N = self._set_host_multi(A, y, False)
            else:
                # a float32 matrix goes to the device as it is only with dense_f32; the default widens it
                as32 = self.dense_f32 and isinstance(A, np.ndarray) and A.dtype == np.float32
                A = np.asarray(A, dtype=np.float32 if as32 else np.float64)
                if A.ndim != 2 or A.shape[1] != self.m:
                    raise ValueError(f"A must be N x m with m = length(x0) = {self.m}")
                Af = np.asfortranarray(A)  # Julia layout: column-major, lda = N
                yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
                self.N = int(A.shape[0])
                Ng = self.N if N_global is None else int(N_global)
                if as32:
                    self.ctx.check(_lib.lib.scs_set_data_f32(self.ctx.h, self.N, self.m, Af.ctypes.data_as(C.c_void_p),
                                                             self.N, dptr(yv), Ng, int(row0)))
                else:
                    if self.dense_f32:   # fp64 (or any other) input: rounded to fp32 on the device
                        self.ctx.check(_lib.lib.scs_set_dense_f32(self.ctx.h, 1))
                    self.ctx.check(_lib.lib.scs_set_data(self.ctx.h, self.N, self.m,
                                                         Af.ctypes.data_as(_lib.c_dp), self.N, dptr(yv), Ng,
                                                         int(row0)))
        else:
            N = C.c_int64()
            self.ctx.check(_lib.lib.scs_get_dims(self.ctx.h, C.byref(N), None, None, None))
            self.N = int(N.value)
        Ng, r0 = C.c_int64(), C.c_int64()
        self.ctx.check(_lib.lib.scs_get_dims(self.ctx.h, None, None, C.byref(Ng), C.byref(r0)))
        self.N_global = int(Ng.value)   # the rows of all ranks (the minibatch loader's N)
        self.row0 = int(r0.value)       # this rank's first global row
        if comm is not None and comm.active:
            comm.bind_buffer(self.ctx)
        ggn = ggn_kind(out_fn)
        if out_fn is not None and f.kind in ("quadratic", "rosenbrock"):
            raise ValueError("out_fn needs a data loss")
        if out_fn is not None and out_fn.scale != f.scale:
            raise ValueError("f and out_fn must use the same scale (one device loss scale)")
        scale = f.scale
        if f.kind == "samplewise":
            if self.generic:
                raise ValueError("a sample-wise loss needs data: Problem(A, y, x0, samplewise(...), λ)")
            if out_fn is not None:
                raise ValueError("a sample-wise loss carries its own GGN pieces (link, link_d1, grad_fy, hess_fy): "
                                 "no out_fn")
            self._bind_samplewise(f)
            ggn = "samplewise" if f.has_ggn else None
        self.ctx.check(_lib.lib.scs_set_loss(self.ctx.h, LOSS[f.kind], GGN[ggn], scale))
        self._cb_test = None
        if f.kind == "callback":
            self._bind_callback(f)
        self.set_test(Atest, ytest, Ntest_global=Ntest_global, row0=test_row0)

    # held-out data (problems.jl:27-28,67-68; iterate.jl:169-175) --------------------------
    def set_test(self, Atest=None, ytest=None, *, Ntest_global=None, row0=0, sparse_f32=False):
        """Atest / ytest: ftest(x) = f(Atest, ytest, x) -- the problem's own f, scale literal
        included -- is pushed into Solution.fvaltest at every stats push.  Both are required; one
        alone is the reference's xor case (iterate.jl:170-171): optim_loop! logs "Will skip
        testing..." and then, since `ftest` is never assigned, its first show_stat! (:201) raises
        UndefVarError -- iterate() does the same (scs_iterate_ex / the host loop).  Sharded: this
        rank's rows of the held-out set (Ntest_global rows in all); a devices=[...] problem takes
        the whole set."""
        self.ctx.check(_lib.lib.scs_set_test_data(self.ctx.h, 0, None, 0, None, 0, 0))   # clear
        self._cb_test = None
        self.test_model = False
        self.test_xor = False
        if Atest is None and ytest is None:
            return
        if self.generic and getattr(self.f, "kind", None) != "callback":
            raise ValueError("a ProblemGeneric has no test data (problems.jl:5-19)")
        if Atest is None or ytest is None:    # iterate.jl:170-171: recorded; the loop raises (:201)
            one = np.zeros(1)
            self.ctx.check(_lib.lib.scs_set_test_data(self.ctx.h, 0, None if Atest is None else dptr(one), 0,
                                                      None if ytest is None else dptr(one), 0, 0))
            self.test_xor = True
            return
        if self.f.kind == "quadratic":   # 1/2*(x'*(Atest*x)) + ytest'*x: Julia's DimensionMismatch otherwise
            shp = Atest.shape if hasattr(Atest, "shape") else np.shape(Atest)
            nglob = int(Ntest_global) if Ntest_global is not None else int(shp[0])
            if nglob != self.m or np.size(ytest) != shp[0]:
                raise ValueError(f"DimensionMismatch: the quadratic loss needs an m x m Atest (m = {self.m}) and "
                                 f"len(ytest) = m, got Atest {tuple(shp)}")
        if self.f.kind == "callback":
            if self._cb_data is None:
                raise ValueError("Atest / ytest need a data problem: Problem(A, y, x0, f, λ; Atest, ytest)")
            self._cb_test = (Atest, np.asarray(ytest, dtype=np.float64))
            self.ctx.check(_lib.lib.scs_set_test_callback(self.ctx.h, 1))
            self.test_model = True
            return
        if self.nout > 1 and _lib.is_device_csr(Atest) and not self.sparse_outputs:
            raise ValueError("a sparse Atest is not supported with nout (multi-output losses take dense rows); "
                             "pass sparse_outputs=True / scs_set_sparse_outputs")
        if _lib.is_device_csr(Atest):
            if len(self.ctx.devices) > 1:
                raise ValueError("a devices=[...] problem takes host held-out rows, not a device CSR")
            self._set_sparse_device(Atest, ytest, True, Ntest_global, row0, bool(sparse_f32))
            self.test_model = True
            return
        if _lib.is_device_array(Atest):
            if len(self.ctx.devices) > 1:
                raise ValueError("a devices=[...] problem takes host held-out rows, not a device array")
            self._set_device(Atest, ytest, True, Ntest_global, row0)
            self.test_model = True
            return
        if self.nout > 1 and not (_is_sparse(Atest) and self.sparse_outputs):
            if _is_sparse(Atest):
                raise ValueError("a sparse Atest is not supported with nout (multi-output losses take dense rows); "
                                 "pass sparse_outputs=True / scs_set_sparse_outputs")
            self._set_host_multi(Atest, ytest, True)
            self.test_model = True
            return
        if self.nout > 1:   # Ntest x nout targets, column-major
            _yp, yv = self._targets(ytest, int(Atest.shape[0]))
            if yv is None:
                raise ValueError("a host sparse Atest takes host targets")
            yv = yv.reshape(-1, order="F")
        else:
            yv = np.ascontiguousarray(np.asarray(ytest, dtype=np.float64).reshape(-1))
        Ng = int(Ntest_global) if Ntest_global is not None else 0
        if _is_sparse(Atest):
            csr = Atest.tocsr()
            if csr.shape[1] != self.d or csr.shape[0] * self.nout != yv.shape[0]:
                raise ValueError(f"Atest must be Ntest x m (m = {self.d}) with len(ytest) = Ntest")
            rowptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
            colidx = np.ascontiguousarray(csr.indices, dtype=np.int32)
            val = np.ascontiguousarray(csr.data, dtype=np.float64)
            self.ctx.check(_lib.lib.scs_set_test_sparse(
                self.ctx.h, int(csr.shape[0]), int(val.shape[0]), rowptr.ctypes.data_as(_lib.c_i64p),
                colidx.ctypes.data_as(_lib.c_i32p), dptr(val), 1 if sparse_f32 else 0, dptr(yv), Ng, int(row0)))
        else:
            # the held-out rows follow the context's storage mode (float32 rows as they are with dense_f32)
            as32 = self.dense_f32 and isinstance(Atest, np.ndarray) and Atest.dtype == np.float32
            At = np.asarray(Atest, dtype=np.float32 if as32 else np.float64)
            if At.ndim != 2 or At.shape[1] != self.m or At.shape[0] != yv.shape[0]:
                raise ValueError(f"Atest must be Ntest x m (m = {self.m}) with len(ytest) = Ntest")
            Af = np.asfortranarray(At)
            if as32:
                self.ctx.check(_lib.lib.scs_set_test_data_f32(self.ctx.h, int(At.shape[0]),
                                                              Af.ctypes.data_as(C.c_void_p), int(At.shape[0]),
                                                              dptr(yv), Ng, int(row0)))
            else:
                self.ctx.check(_lib.lib.scs_set_test_data(self.ctx.h, int(At.shape[0]), Af.ctypes.data_as(_lib.c_dp),
                                                          int(At.shape[0]), dptr(yv), Ng, int(row0)))
        self.test_model = True

    def _check_outputs(self, f, out_fn, A, comm, devices, _ctx):
        """nout of a multi-output problem (1 otherwise) after the refusals of scs_set_outputs, each
        naming the option it refuses."""
        k = getattr(f, "nout", None)
        ko = getattr(out_fn, "nout", None)
        if k is None and ko is None:
            return 1
        if k is None:
            raise ValueError(f"out_fn {out_fn.kind}(nout={ko}) needs a multi-output loss (losses.softmax_ce / "
                             f"losses.multi_least_squares): the {f.kind} loss is not supported with nout")
        pair = {"softmax_ce": "linear_softmax_ce", "multi_least_squares": "linear_multi_ls"}[f.kind]
        if out_fn is not None and (out_fn.kind != pair or ko != k):
            raise ValueError(f"{f.kind}(nout={k}) takes out_fn = losses.{pair}({k}, scale)")
        if not 2 <= k <= 16:
            raise ValueError(f"nout = {k} is outside 2..16")
        if A is None or _ctx is not None:
            raise ValueError("a multi-output loss (nout) needs a dense A: Problem(A, Y, x0, f, λ)")
        if (_lib.is_device_csr(A) or _is_sparse(A)) and not self.sparse_outputs:
            raise ValueError("a sparse A is not supported with nout (multi-output losses take a dense A); "
                             "pass sparse_outputs=True / scs_set_sparse_outputs")
        if devices is not None:
            raise ValueError("devices=[...] is not supported with nout (multi-output losses run on one device)")
        if comm is not None and comm.active:
            raise ValueError("nranks > 1 (comm) is not supported with nout (multi-output losses run on one rank)")
        if self.m % k:
            raise ValueError(f"len(x0) = {self.m} is not A.shape[1] * nout (nout = {k}): x = vec(X), X d x nout")
        return int(k)

    def _targets(self, Y, N):
        """Y of a multi-output problem as what the data doors take: N x nout, column-major."""
        if _lib.is_device_array(Y):
            return _lib.parse_device_targets(Y.__cuda_array_interface__, N, self.nout), None
        Yf = np.asfortranarray(np.asarray(Y, dtype=np.float64))
        if Yf.shape != (N, self.nout):
            raise ValueError(f"Y must be N x nout = ({N}, {self.nout}), got {Yf.shape}")
        return Yf.ctypes.data, Yf

    def _set_host_multi(self, A, Y, test):
        """Host rows of a multi-output problem: A N x d with d * nout = len(x0), Y N x nout."""
        as32 = self.dense_f32 and isinstance(A, np.ndarray) and A.dtype == np.float32
        A = np.asarray(A, dtype=np.float32 if as32 else np.float64)
        if A.ndim != 2 or A.shape[1] * self.nout != self.m:
            raise ValueError(f"A must be N x d with d * nout = length(x0) = {self.m} (nout = {self.nout})")
        N = int(A.shape[0])
        Af = np.asfortranarray(A)
        yp, _keep = self._targets(Y, N)
        yp = C.cast(yp, _lib.c_dp)
        h = self.ctx.h
        if self.dense_f32 and not as32:
            self.ctx.check(_lib.lib.scs_set_dense_f32(h, 1))
        if test:
            if as32:
                rc = _lib.lib.scs_set_test_data_f32(h, N, Af.ctypes.data_as(C.c_void_p), N, yp, 0, 0)
            else:
                rc = _lib.lib.scs_set_test_data(h, N, Af.ctypes.data_as(_lib.c_dp), N, yp, 0, 0)
        elif as32:
            rc = _lib.lib.scs_set_data_f32(h, N, self.d, Af.ctypes.data_as(C.c_void_p), N, yp, N, 0)
        else:
            rc = _lib.lib.scs_set_data(h, N, self.d, Af.ctypes.data_as(_lib.c_dp), N, yp, N, 0)
        self.ctx.check(rc)
        return N

    def _set_device(self, A, y, test, N_global, row0):
        """A (and possibly y) already on the GPU, through __cuda_array_interface__ (a torch-ROCm tensor, a
        CuPy array): scs_set_data_device / scs_set_test_data_device re-tile it on the device, no host
        copy.  Row- or column-major, float64 or float32; the stored type follows dense_f32 as for host
        arrays (float32 kept only with dense_f32=True, float64 rounded on the device with it).
        Returns N."""
        d = _lib.parse_device_matrix(A.__cuda_array_interface__)
        if d["m"] * self.nout != self.m:
            raise ValueError(f"A must be N x m with m = length(x0) = {self.m}" if self.nout == 1 else
                             f"A must be N x d with d * nout = length(x0) = {self.m} (nout = {self.nout})")
        N = d["N"]
        yp, stream, _keep = self._device_y_and_stream((A,), y, N, d["stream"])
        if self.dense_f32:
            self.ctx.check(_lib.lib.scs_set_dense_f32(self.ctx.h, 1))
        Ng = 0 if N_global is None else int(N_global)
        if test:
            rc = _lib.lib.scs_set_test_data_device(self.ctx.h, N, d["ptr"], d["elem_bytes"], d["stride_n"],
                                                   d["stride_m"], yp, stream, Ng, int(row0))
        else:
            rc = _lib.lib.scs_set_data_device(self.ctx.h, N, self.d, d["ptr"], d["elem_bytes"], d["stride_n"],
                                              d["stride_m"], yp, stream, Ng if Ng else N, int(row0))
        self.ctx.check(rc)
        return N

    def _device_y_and_stream(self, arrays, y, N, stream):
        """y of a device door (a device array or anything NumPy reads) and the src_stream to pass:
        `stream` if the source's interface named one, else y's, else torch's current stream.  Returns
        (pointer of y, stream, the host copy of y to keep alive or None)."""
        torch_stream = None
        for a in (*arrays, y):
            if type(a).__module__.split(".")[0] == "torch":
                _lib.require_torch_runtime("a torch tensor as A / y")   # a second runtime's pointer is not ours
                torch_stream = sys.modules["torch"].cuda.current_stream(a.device)
        if self.nout > 1:   # N x nout targets, host or device
            yp, yv = self._targets(y, N)
            ystream = y.__cuda_array_interface__.get("stream") if yv is None else None
        elif _lib.is_device_array(y):
            yi = y.__cuda_array_interface__
            yp, yv = _lib.parse_device_vector(yi, N), None
            ystream = yi.get("stream")
        else:
            yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
            if yv.shape[0] != N:
                raise ValueError(f"y has {yv.shape[0]} entries, A has {N} rows")
            yp, ystream = yv.ctypes.data, None
        if stream is None and ystream is not None:
            stream = int(ystream)
        if stream is None and torch_stream is not None:
            # torch's interface names no stream: the tensor's producer is the current one (its default
            # stream is drained here: a handle of 0 would read as "the source is complete")
            if torch_stream.cuda_stream:
                stream = int(torch_stream.cuda_stream)
            else:
                torch_stream.synchronize()
        return yp, stream, yv

    def _set_sparse_device(self, A, y, test, N_global, row0, f32):
        """A CSR matrix whose arrays are already on the GPU (torch.sparse_csr_tensor, a CuPy csr_matrix):
        scs_set_sparse_device / scs_set_test_sparse_device validate it, build the CSC copy and both
        blocked copies on the device, no host copy.  int32 or int64 pointers and indices, float32 or
        float64 values; f32 (sparse_f32) alone decides the stored type.  Unsorted rows and duplicate
        entries are taken as scipy's tocsr() / tocsc() keep them.  Returns N."""
        shape, indptr, indices, data = _lib.device_csr_arrays(A)
        d = _lib.parse_device_csr(shape, *(a.__cuda_array_interface__ for a in (indptr, indices, data)))
        if d["m"] * self.nout != self.m:
            raise ValueError(f"A must be N x m with m = length(x0) = {self.m}" if self.nout == 1 else
                             f"A must be N x d with d * nout = length(x0) = {self.m} (nout = {self.nout})")
        N = d["N"]
        yp, stream, _keep = self._device_y_and_stream((indptr, indices, data), y, N, d["stream"])
        Ng = 0 if N_global is None else int(N_global)
        src = (d["rowptr"], d["ptr_bytes"], d["colidx"], d["idx_bytes"], d["val"], d["val_bytes"], 1 if f32 else 0,
               yp, stream)
        if test:
            rc = _lib.lib.scs_set_test_sparse_device(self.ctx.h, N, d["nnz"], *src, Ng, int(row0))
        else:
            rc = _lib.lib.scs_set_sparse_device(self.ctx.h, N, self.d, d["nnz"], *src, Ng if Ng else N, int(row0))
        self.ctx.check(rc)
        return N

    def gen_test(self, Ntest, *, row0=None, seed=1234, kind=1, density=0.1):
        """Held-out rows of the synthetic generator: rows [row0, row0 + Ntest) with row0 = N_global
        by default (samples the training rows never saw, same x_true).  Sharded: this rank
        generates its contiguous block of the Ntest rows."""
        from .shard import row_range
        r0 = self.N_global if row0 is None else int(row0)
        comm = self.comm
        # one process per GPU: this rank's block; one process (one or several devices): all rows
        # (a devices=[...] context splits them itself)
        a, b = row_range(Ntest, comm.world, comm.rank) if comm is not None else (0, int(Ntest))
        spec = _lib.Synth(N_global=int(Ntest), row0=r0 + a, N=b - a, m=self.m, seed=seed, kind=kind, density=density)
        self.ctx.check(_lib.lib.scs_gen_test_data(self.ctx.h, C.byref(spec)))
        self._cb_test = None
        self.test_xor = False
        self.test_model = True

    def ftest(self, x):
        """f(Atest, ytest, x) (iterate.jl:173) on the device (a callback loss: on the host)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = C.c_double()
        self.ctx.check(_lib.lib.scs_eval_ftest(self.ctx.h, dptr(x), C.byref(out)))
        return out.value

    def _bind_callback(self, f):
        """Register f / grad_fx / hess_fx with scs_set_loss_callback; a Python exception inside a
        call is kept and re-raised by Context.check."""
        data = self._cb_data
        args = (lambda x: (x,)) if data is None else (lambda x: (data[0], data[1], x))
        ctx = self.ctx
        nout = 0
        if f.has_ggn:
            if data is None:
                raise ValueError("ProxGGNSCORE callbacks take the data: Problem(A, y, x0, callback(...), λ)")
            nout = int(np.asarray(f.out_fn(data[0], self.x0)).size)

        def ggn_pieces(x, m, outp):
            """prox-GGN-SCORE.jl:44-49 on the host; a non-diagonal Q is eigen-rotated (J̃ = VᵀJ,
            r̃ = Vᵀr, q = eigenvalues), which leaves JᵀQJ, Jᵀr and the sample-space system exact."""
            A, y = data
            yhat = f.out_fn(A, x)
            J = np.asarray(f.jac_yx(A, y, yhat, x), dtype=np.float64).reshape(nout, m)
            r = np.asarray(f.grad_fy(A, y, yhat), dtype=np.float64).ravel(order="F")
            Q = np.asarray(f.hess_fy(A, y, yhat), dtype=np.float64)
            if Q.ndim == 2 and np.count_nonzero(Q - np.diag(np.diagonal(Q))) == 0:
                Q = np.diagonal(Q).copy()
            if Q.ndim == 2:
                lam, V = np.linalg.eigh(0.5 * (Q + Q.T))
                J, r, q = V.T @ J, V.T @ r, lam
            else:
                q = Q.reshape(nout)
            out = np.ctypeslib.as_array(outp, shape=(nout * (m + 2),))
            out[:nout * m] = J.ravel(order="F")
            out[nout * m:nout * (m + 1)] = r
            out[nout * (m + 1):] = q

        def call(user, what, xp, m, outp):
            try:
                x = np.ctypeslib.as_array(xp, shape=(m,)).copy()
                if what == _lib.SCS_CB_F:
                    outp[0] = float(f.f(*args(x)))
                elif what == _lib.SCS_CB_GRAD:
                    if f.grad_fx is None:
                        raise ValueError("this method needs grad_fx: the device path has no automatic "
                                         "differentiation (the reference's ForwardDiff default)")
                    g = np.asarray(f.grad_fx(*args(x)), dtype=np.float64).reshape(m)
                    np.ctypeslib.as_array(outp, shape=(m,))[:] = g
                elif what == _lib.SCS_CB_GRAD_X:
                    # ProxGGNSCORE: grad_f = x -> model.grad_fx(x), ONE argument (prox-GGN-SCORE.jl:58-59),
                    # reached from its ss_type 3 line search (:83-84): Julia's MethodError when the
                    # user's grad_fx has no one-argument method (a data problem's grad_fx(A, y, x))
                    if f.grad_fx is None:
                        raise ValueError("this method needs grad_fx: the device path has no automatic "
                                         "differentiation (the reference's ForwardDiff default)")
                    if not _accepts_one_arg(f.grad_fx):
                        return _lib.SCS_CB_NO_METHOD
                    g = np.asarray(f.grad_fx(x), dtype=np.float64).reshape(m)
                    np.ctypeslib.as_array(outp, shape=(m,))[:] = g
                elif what == _lib.SCS_CB_HESS:
                    if f.hess_fx is None:
                        raise ValueError("ProxNSCORE needs hess_fx: the device path has no automatic "
                                         "differentiation (the reference's ForwardDiff default)")
                    H = np.asarray(f.hess_fx(*args(x)), dtype=np.float64).reshape(m, m)
                    np.ctypeslib.as_array(outp, shape=(m * m,))[:] = H.ravel(order="F")   # column-major
                elif what == _lib.SCS_CB_GGN:
                    ggn_pieces(x, m, outp)
                elif what == _lib.SCS_CB_FTEST:   # iterate.jl:173: the same closure on the held-out data
                    At, yt = self._cb_test
                    outp[0] = float(f.f(At, yt, x))
                else:
                    raise ValueError(f"unknown callback request {what}")
                return 0
            except BaseException as e:   # noqa: BLE001 -- handed back to the caller by Context.check
                ctx._cb_exc = e
                return 1

        cb = _lib.LOSS_FN(call)
        self.ctx._keep.append(cb)
        self.ctx.check(_lib.lib.scs_set_loss_callback(self.ctx.h, cb, None, nout))

    def _bind_samplewise(self, f):
        """Register a losses.samplewise(...) with scs_set_loss_samplewise.  The library hands over z and
        y of the view in use (n entries) and the output areas it wants filled: NumPy views of its pinned
        host buffers, or -- f.device -- torch tensors aliasing its device buffers, with the callables
        run on the context's stream.  A Python exception inside a call is kept and re-raised by
        Context.check."""
        ctx = self.ctx
        noad = ": the device path has no automatic differentiation (the reference's ForwardDiff default)"

        def need(fn, name, who="this method"):
            if fn is None:
                raise ValueError(f"{who} needs {name}{noad}")
            return fn

        if f.device:
            _lib.require_torch_runtime("a device-mode sample-wise loss")
            import torch
            dev = torch.device("cuda", ctx.device)

            def wrap(p, n, readonly=False):
                return torch.as_tensor(_lib.DeviceVector(p, n), device=dev)

            def put(dst, src, name):
                src = torch.as_tensor(src, dtype=torch.float64, device=dev)
                if src.dim() != 0 and tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"samplewise: {name} returned shape {tuple(src.shape)}, expected "
                                     f"{tuple(dst.shape)}")
                dst.copy_(src)

            def on_stream(stream):
                s = torch.cuda.ExternalStream(int(stream), device=dev) if stream else torch.cuda.default_stream(dev)
                return torch.cuda.stream(s)
        else:
            import contextlib

            def wrap(p, n, readonly=False):
                a = np.ctypeslib.as_array(C.cast(p, _lib.c_dp), shape=(n,))
                if readonly:
                    a.flags.writeable = False
                return a

            put = _samplewise_put_host

            def on_stream(stream):
                return contextlib.nullcontext()

        def call(user, what, n, zp, yp, vp, d1p, d2p, sp, stream):
            try:
                n = int(n)
                with on_stream(stream):
                    z, y = wrap(zp, n, True), wrap(yp, n, True)
                    if what & _lib.SCS_SW_VALUE:
                        put(wrap(vp, n), f.value(z, y), "value")
                    if what & _lib.SCS_SW_D1:
                        put(wrap(d1p, n), need(f.d1, "d1")(z, y), "d1")
                    if what & _lib.SCS_SW_D2:
                        put(wrap(d2p, n), need(f.d2, "d2", "ProxNSCORE")(z, y), "d2")
                    if what & _lib.SCS_SW_GGN:
                        for nm in ("link", "link_d1", "grad_fy", "hess_fy"):
                            need(getattr(f, nm), nm, "ProxGGNSCORE")
                        yhat = f.link(z)
                        put(wrap(sp, n), f.link_d1(z), "link_d1")
                        put(wrap(d1p, n), f.grad_fy(y, yhat), "grad_fy")
                        put(wrap(d2p, n), f.hess_fy(y, yhat), "hess_fy")
                return 0
            except BaseException as e:   # noqa: BLE001 -- handed back to the caller by Context.check
                ctx._cb_exc = e
                return 1

        cb = _lib.SAMPLEWISE_FN(call)
        ctx._keep.append(cb)
        ctx.check(_lib.lib.scs_set_loss_samplewise(ctx.h, cb, None, 1 if f.device else 0, 1 if f.has_ggn else 0))

    @classmethod
    def synthetic(cls, N, m, x0, f, lam, *, kind=1, seed=1234, density=0.1, out_fn=None, device=0,
                  comm=None, devices=None, device_exchange="rccl", test_N=None, dense_f32=False, **kw):
        """A ~ N(0,1)/sqrt(m) (kind 1, 2) or N(0,1) (kind 3) generated on the device, y from a
        sparse x_true (kind 1: Bernoulli(σ(A x_true)) ∈ {0,1}; kind 2: ±1; kind 3: A x_true + 0.1ε).
        With comm, this rank generates its contiguous row shard in place; with devices=[...] one
        process drives those GPUs and the library generates each one's row block.  dense_f32: the
        rows are stored rounded to fp32 and y is formed from the stored rows."""
        from .shard import row_range
        if devices is not None and comm is not None:
            raise ValueError("devices=[...] (one process, several GPUs) and comm (one process per GPU) exclude "
                             "each other")
        rank, world = (comm.rank, comm.world) if comm is not None else (0, 1)
        r0, r1 = row_range(N, world, rank)
        ctx = _lib.Context(device, devices=devices, device_exchange=device_exchange)
        if comm is not None and comm.active:
            comm.attach(ctx)
        spec = _lib.Synth(N_global=N, row0=r0, N=r1 - r0, m=m, seed=seed, kind=kind, density=density)
        if dense_f32:
            ctx.check(_lib.lib.scs_set_dense_f32(ctx.h, 1))
        ctx.check(_lib.lib.scs_gen_data(ctx.h, C.byref(spec)))
        p = cls(x0, f, lam, out_fn=out_fn, device=device, comm=comm, dense_f32=dense_f32, _ctx=ctx, **kw)
        if test_N:   # held-out rows [N, N + test_N) of the same generator (same x_true)
            p.gen_test(int(test_N), row0=N, seed=seed, kind=kind, density=density)
        return p

    @classmethod
    def synthetic_sparse(cls, N, m, x0, f, lam, *, density=0.01, seed=1234, f32=False, device=0, **kw):
        """Sparse A (the README's sprandn(N, m, ρ) problem class, BASELINE configs[4]) generated on
        the device: k = round(ρ m) nonzeros per row, N(0,1)/sqrt(k) values, CSR + CSC copies;
        x_true ~ U(-1.5, 1.5), y = A x_true + 0.1ε.  N must be a power of two and a multiple of m."""
        ctx = _lib.Context(device)
        spec = _lib.Synth(N_global=N, row0=0, N=N, m=m, seed=seed, kind=4, density=density)
        ctx.check(_lib.lib.scs_gen_sparse(ctx.h, C.byref(spec), 1 if f32 else 0))
        return cls(x0, f, lam, device=device, _ctx=ctx, **kw)

    def _set_sparse(self, A, y, N_global, row0, f32):
        csr = A.tocsr()
        csc = A.tocsc()
        if csr.shape[1] * self.nout != self.m:
            raise ValueError(f"A must be N x m with m = length(x0) = {self.m}" if self.nout == 1 else
                             f"A must be N x d with d * nout = length(x0) = {self.m} (nout = {self.nout})")
        self.N = int(csr.shape[0])
        rowptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
        colidx = np.ascontiguousarray(csr.indices, dtype=np.int32)
        val = np.ascontiguousarray(csr.data, dtype=np.float64)
        colptr = np.ascontiguousarray(csc.indptr, dtype=np.int64)
        rowidx = np.ascontiguousarray(csc.indices, dtype=np.int32)
        valT = np.ascontiguousarray(csc.data, dtype=np.float64)
        if self.nout > 1:   # N x nout targets, column-major
            _yp, yv = self._targets(y, self.N)
            if yv is None:
                raise ValueError("a host sparse A takes host targets (a device CSR takes either)")
            yv = yv.reshape(-1, order="F")
        else:
            yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        Ng = self.N if N_global is None else int(N_global)
        i64, i32 = _lib.c_i64p, _lib.c_i32p
        self.ctx.check(_lib.lib.scs_set_sparse(
            self.ctx.h, self.N, self.d, int(val.shape[0]), rowptr.ctypes.data_as(i64), colidx.ctypes.data_as(i32),
            dptr(val), colptr.ctypes.data_as(i64), rowidx.ctypes.data_as(i32), dptr(valT), 1 if f32 else 0,
            dptr(yv), Ng, int(row0)))

    @property
    def nnz(self):
        n = C.c_int64()
        self.ctx.check(_lib.lib.scs_get_nnz(self.ctx.h, C.byref(n)))
        return int(n.value)

    def get_sparse(self):
        """The device CSR copy of A as a scipy.sparse.csr_matrix (values widened to fp64), and y."""
        import scipy.sparse as sp
        nnz = self.nnz
        rowptr = np.zeros(self.N + 1, dtype=np.int64)
        colidx = np.zeros(max(nnz, 1), dtype=np.int32)
        val = np.zeros(max(nnz, 1), dtype=np.float64)
        self.ctx.check(_lib.lib.scs_get_sparse(self.ctx.h, rowptr.ctypes.data_as(_lib.c_i64p),
                                               colidx.ctypes.data_as(_lib.c_i32p), dptr(val)))
        y = np.zeros(self.N * self.nout, dtype=np.float64)   # (multi-output: N x nout, column-major)
        self.ctx.check(_lib.lib.scs_get_data(self.ctx.h, 0, self.N, None, self.N, dptr(y)))
        if self.nout > 1:
            y = np.ascontiguousarray(y.reshape(self.nout, self.N).T)
        return sp.csr_matrix((val[:nnz], colidx[:nnz], rowptr), shape=(self.N, self.d)), y

    def get_sparse_csc(self):
        """The device CSC copy of A as a scipy.sparse.csc_matrix (values widened to fp64), entries as
        the device holds them: rows ascending within a column, duplicates kept."""
        import scipy.sparse as sp
        nnz = self.nnz
        colptr = np.zeros(self.d + 1, dtype=np.int64)
        rowidx = np.zeros(max(nnz, 1), dtype=np.int32)
        valT = np.zeros(max(nnz, 1), dtype=np.float64)
        self.ctx.check(_lib.lib.scs_get_sparse_csc(self.ctx.h, colptr.ctypes.data_as(_lib.c_i64p),
                                                   rowidx.ctypes.data_as(_lib.c_i32p), dptr(valT)))
        return sp.csc_matrix((valT[:nnz], rowidx[:nnz], colptr), shape=(self.N, self.d))

    # device evaluation helpers ------------------------------------------------
    def fx(self, x):
        """f(A, y, x) on the device (iterate.jl:168)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = C.c_double()
        self.ctx.check(_lib.lib.scs_eval_f(self.ctx.h, dptr(x), C.byref(out)))
        return out.value

    def gradx(self, x):
        """∇f(A, y, x) on the device (grad_fx)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.empty(self.m)
        self.ctx.check(_lib.lib.scs_eval_grad(self.ctx.h, dptr(x), dptr(g)))
        return g

    def get_data(self, r0=0, nr=None):
        nr = self.N - r0 if nr is None else nr
        A = np.zeros((self.d, nr), dtype=np.float64)   # column-major view: A.T is N x m
        y = np.zeros(nr * self.nout, dtype=np.float64)   # (multi-output: nr x nout, column-major)
        self.ctx.check(_lib.lib.scs_get_data(self.ctx.h, r0, nr, dptr(A), nr, dptr(y)))
        if self.nout > 1:
            return np.ascontiguousarray(A.T), np.ascontiguousarray(y.reshape(self.nout, nr).T)
        return np.ascontiguousarray(A.T), y

    def data_info(self):
        """(element bytes of the dense A: 8 or 4, bytes of that block, device bytes the context holds)
        -- scs_data_info."""
        eb, ab, cb = C.c_int(), C.c_int64(), C.c_int64()
        self.ctx.check(_lib.lib.scs_data_info(self.ctx.h, C.byref(eb), C.byref(ab), C.byref(cb)))
        return int(eb.value), int(ab.value), int(cb.value)

    def configure(self, reg_name, hmu: Smoother):
        """Push reg_name / λ / C_set / P and the smoother to the device context."""
        if reg_name not in REG:
            raise _lib.ScsReferenceError(_lib.SCS_ERR_REF, "reg_name not valid.")
        lam = np.ascontiguousarray(_lam_tuple(self.λ), dtype=np.float64)
        lb = ub = None
        nb = 0
        ind = None
        ng = 0
        if reg_name == "indbox":
            if self.C_set is None:
                raise ValueError("indbox needs C_set")
            lo, hi = self.C_set[0], self.C_set[1]
            lb, ub = bounds_array(lo, self.m), bounds_array(hi, self.m)
            if lb.size != ub.size:
                lb = np.broadcast_to(lb, (self.m,)).copy()
                ub = np.broadcast_to(ub, (self.m,)).copy()
            nb = lb.size
        if reg_name == "gl":
            if self.P is None:
                raise ValueError("gl needs P = get_P(n, G, ind)")
            ind = np.ascontiguousarray(self.P.ind.T.reshape(-1), dtype=np.int64)  # column-major 3 x G
            ng = self.P.grpNUM
        self.ctx.check(_lib.lib.scs_set_reg(self.ctx.h, REG[reg_name], dptr(lam), lam.size, dptr(lb), dptr(ub),
                                            nb, ind.ctypes.data_as(_lib.c_i64p) if ind is not None else None,
                                            ng))
        if reg_name == "gl":
            G = np.ascontiguousarray(self.P.G, dtype=np.int64)
            self.ctx.check(_lib.lib.scs_set_group_map(self.ctx.h, G.ctypes.data_as(_lib.c_i64p), int(G.size)))
        slb = sub = None
        snb = 0
        if hmu.kind in ("phuber_indbox", "exp_indbox", "logexp_indbox"):
            slb, sub = bounds_array(hmu.lb, self.m), bounds_array(hmu.ub, self.m)
            if slb.size != sub.size:
                slb = np.broadcast_to(slb, (self.m,)).copy()
                sub = np.broadcast_to(sub, (self.m,)).copy()
            snb = slb.size
        self.ctx.check(_lib.lib.scs_set_smoother(self.ctx.h, SMOOTH[hmu.kind], hmu.mu, hmu.Mh, hmu.nu, dptr(slb),
                                                 dptr(sub), snb))
        self.ctx.check(_lib.lib.scs_set_L(self.ctx.h, int(self.L is not None),
                                          float(self.L) if self.L is not None else 0.0))

    def get_reg(self, x):
        """get_reg(model, x, reg_name) for the configured reg_name (regularizers.jl:4-31)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = C.c_double()
        self.ctx.check(_lib.lib.scs_eval_reg(self.ctx.h, dptr(x), C.byref(out)))
        return out.value

    def set_gram_cache(self, on=True):
        """Opt-in reuse of AᵀQA across steps when it is x-independent (least squares under
        ProxNSCORE, or ProxGGNSCORE with the linear out_fn); the reference recomputes it every
        step (prox-GGN-SCORE.jl:129), which stays the default.  Results are bit-identical."""
        self.ctx.check(_lib.lib.scs_set_gram_cache(self.ctx.h, int(bool(on))))

    def set_compute_f32(self, on=True):
        """The compute arm of the fp32-vs-fp64 study (BASELINE configs[4]): the sparse products of
        fp32-stored values (sparse_f32 / f32=True) and the L-BFGS two-loop in fp32 arithmetic;
        f, η, the step, the prox and the solves stay fp64.  Off (fp64) by default."""
        self.ctx.check(_lib.lib.scs_set_compute_f32(self.ctx.h, int(bool(on))))

    def set_solver(self, kind="default"):
        """"default": Cholesky (LU fallback) / LU; "reference": the reference's factorizations --
        Householder QR for ProxGGNSCORE's systems (prox-GGN-SCORE.jl:126,131), LU for ProxNSCORE's
        (prox-N-SCORE.jl:70).  scs_set_solver."""
        self.ctx.check(_lib.lib.scs_set_solver(self.ctx.h, _lib.SOLVER[kind]))

    def set_batches(self, batches=None):
        """Register the collected loader batches (iterate.jl:141-146): a list of row-index arrays
        (0-based, GLOBAL rows: on several ranks every rank passes the same list and keeps the rows
        it owns), gathered on the device as the As, ys of their step! calls (iterate.jl:205-207).
        None / [] clears the list.  f / get_reg stay on the full data."""
        self._bsel, self._bsizes = -1, []
        if not batches:
            self.ctx.check(_lib.lib.scs_set_batches(self.ctx.h, None, None, 0))
            return
        rs = [np.asarray(b, dtype=np.int64).reshape(-1) for b in batches]
        self._bsizes = [int(r.size) for r in rs]
        rows = np.ascontiguousarray(np.concatenate(rs))
        off = np.zeros(len(rs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([r.size for r in rs])
        self.ctx.check(_lib.lib.scs_set_batches(self.ctx.h, rows.ctypes.data_as(_lib.c_i64p),
                                                off.ctypes.data_as(_lib.c_i64p), len(rs)))
        if self.comm is not None and self.comm.active:   # the exchange payload may have grown
            self.comm.bind_buffer(self.ctx)

    def set_sparse_batches(self, on=True):
        """Opt-in: under ProxLQNSCORE a minibatch of a sparse A stays sparse -- scs_select_batch builds
        the blocked copies scs_set_sparse would build from A[rows_b, :] instead of the n_b x m_pad dense
        view, bit for bit, and keeps them per batch within a budget (the bytes of the sparse data, or
        SCS_SPARSE_BATCH_CACHE_MB).  ProxNSCORE / ProxGGNSCORE keep the dense view.  Changing the mode
        drops the pooled views; the registered list stays.  scs_set_sparse_batches."""
        self.ctx.check(_lib.lib.scs_set_sparse_batches(self.ctx.h, int(bool(on))))
        self._sparse_batches = bool(on)

    def set_sparse_sample(self, on=True):
        """Opt-in: ProxGGNSCORE's sample-space branch (N + 1 <= m) on a sparse A forms P = A diag(1/Hr) Aᵀ
        from the nonzeros -- no dense mirror, no Aᵀ copy, no tiles; the (N+1)² system and its solve are
        unchanged.  With set_sparse_batches also on, batches with n_b + 1 <= m become sparse views under
        ProxGGNSCORE as well (a step on one equals the step of a Problem holding A[rows_b], y[rows_b]).
        Stored without effect on a sharded or multi-device context and on a dense A.  Changing the mode
        drops the pooled views.  scs_set_sparse_sample."""
        self.ctx.check(_lib.lib.scs_set_sparse_sample(self.ctx.h, int(bool(on))))

    def set_multi_sample(self, on=True):
        """Opt-in: with nout set and N·nout + 1 <= d·nout, ProxGGNSCORE runs the reference's sample-space branch
        on the device (a dense A): K Grams A diag(h_l) Aᵀ, the order-(N·nout + 1) block system, one LU.  Off: that
        shape is refused.  Stored without effect while nout is unset.  scs_set_multi_sample."""
        self.ctx.check(_lib.lib.scs_set_multi_sample(self.ctx.h, int(bool(on))))
        self.multi_sample = bool(on)

    def set_multi_batches(self, on=True):
        """Opt-in: with nout set, set_batches / iterate(batch_size=..., slice_samples=...) accept a dense A: a
        batch's rows of A and of Y are gathered on the device in one launch, and ProxGGNSCORE picks its branch per
        batch (the sample-space one needs multi_sample).  Off: refused.  Stored without effect while nout is
        unset; changing it drops the pooled views, and switching it off clears a multi-output problem's
        registered list.  scs_set_multi_batches."""
        self.ctx.check(_lib.lib.scs_set_multi_batches(self.ctx.h, int(bool(on))))
        self.multi_batches = bool(on)
        if not self.multi_batches and self.nout > 1:
            self._bsel, self._bsizes = -1, []

    def set_multi_sparse_batches(self, on=True):
        """Opt-in: with nout and multi_batches set, set_batches / iterate(batch_size=..., slice_samples=...) also
        accept a sparse A held with sparse_outputs.  A batch is a densified view (its CSR rows written into a dense
        n_b x d block, Y_b gathered; all three methods, ProxGGNSCORE picking its branch per batch) or, with
        sparse_batches also on and ProxLQNSCORE, a sparse K-column view.  Off: the dense-A refusal.  Stored without
        effect while nout is unset or on a dense A; changing it drops the pooled views, and switching it off
        clears a sparse multi-output problem's registered list.  scs_set_multi_sparse_batches."""
        self.ctx.check(_lib.lib.scs_set_multi_sparse_batches(self.ctx.h, int(bool(on))))
        self.multi_sparse_batches = bool(on)
        if not self.multi_sparse_batches and self.nout > 1 and self._sparse_A:
            self._bsel, self._bsizes = -1, []

    def _products_rows(self):
        """The rows multi_products runs on: the selected batch's on a sparse K-column view (a sparse multi-output
        problem with multi_sparse_batches and sparse_batches under ProxLQNSCORE), else the full data's."""
        sel = getattr(self, "_bsel", -1)
        if (sel >= 0 and self.nout > 1 and self._sparse_A and self.multi_sparse_batches and self._sparse_batches
                and getattr(self, "_method_code", None) == 3):   # ProxLQNSCORE.code
            return self._bsizes[sel]
        return self.N

    def get_batch_data(self, b):
        """(A_b, y_b) of registered batch b as a step sees it, gathered by select_batch's own path: the n_b x d
        rows as float64 and the n_b (x nout) targets.  The selection stays as it was.  scs_get_batch_data."""
        b = int(b)
        sizes = getattr(self, "_bsizes", [])
        if not 0 <= b < len(sizes):
            raise IndexError(f"batch {b} of {len(sizes)}")
        n = sizes[b]
        Ab = np.zeros((n, self.d), order="F")
        yb = np.zeros((n, self.nout), order="F") if self.nout > 1 else np.zeros(n)
        self.ctx.check(_lib.lib.scs_get_batch_data(self.ctx.h, b, C.cast(Ab.ctypes.data, _lib.c_dp), n,
                                                   C.cast(yb.ctypes.data, _lib.c_dp)))
        return Ab, yb

    def batch_info(self):
        """(sparse batch views held, their device bytes, views built since set_batches) -- scs_batch_info."""
        nv, vb, bd = C.c_int64(), C.c_int64(), C.c_int64()
        self.ctx.check(_lib.lib.scs_batch_info(self.ctx.h, C.byref(nv), C.byref(vb), C.byref(bd)))
        return int(nv.value), int(vb.value), int(bd.value)

    def select_batch(self, b=-1):
        """The registered batch the following step! calls see as As, ys (-1: the full data)."""
        self.ctx.check(_lib.lib.scs_select_batch(self.ctx.h, int(b)))
        self._bsel = int(b) if int(b) >= 0 else -1

    def _smoother_eval(self, hmu, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        gr = np.empty(self.m)
        Hr = np.empty(self.m)
        self.ctx.check(_lib.lib.scs_smoother_eval(self.ctx.h, dptr(x), dptr(gr), dptr(Hr)))
        return gr, Hr

    # kernel-level entry points used by the parity tests -----------------------
    def prox(self, z, Hr, lam, alpha):
        z = np.ascontiguousarray(z, dtype=np.float64)
        Hr = np.ascontiguousarray(Hr, dtype=np.float64)
        out = np.empty(self.m)
        self.ctx.check(_lib.lib.scs_prox_eval(self.ctx.h, dptr(z), dptr(Hr), float(lam), float(alpha), dptr(out)))
        return out

    def gram(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        G = np.zeros((self.m, self.m))
        self.ctx.check(_lib.lib.scs_gram_eval(self.ctx.h, dptr(w), dptr(G), self.m))
        return G.T.copy()  # column-major -> row-major (lower triangle valid)

    def sample_gram(self, h):
        """A diag(h) Aᵀ of the selected batch or the full data, by the path a ProxGGNSCORE sample-space step
        takes (scs_sample_gram_eval); the full symmetric N x N matrix."""
        h = np.ascontiguousarray(h, dtype=np.float64)
        if h.shape != (self.m,):
            raise ValueError(f"h must have length m = {self.m}")
        sel = getattr(self, "_bsel", -1)
        n = self.N if sel < 0 else self._bsizes[sel]   # the rows select_batch chose last
        P = np.zeros((n, n))
        self.ctx.check(_lib.lib.scs_sample_gram_eval(self.ctx.h, dptr(h), dptr(P), n))
        return P

    def sample_system(self, x):
        """(M, b) of the sample-space system a single-output ProxGGNSCORE step solves at x (N + 1 <= m, a GGN
        loss kind; configure() first: h = 1 ./ Hr and λ gr enter it), of the selected batch or the full data, by
        the step's own function up to the solve (scs_sample_system_eval).  M has order N + 1, column-major."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.m,):
            raise ValueError(f"x must have length m = {self.m}")
        sel = getattr(self, "_bsel", -1)
        n1 = (self.N if sel < 0 else self._bsizes[sel]) + 1   # the rows select_batch chose last
        Mm = np.zeros((n1, n1), order="F")
        b = np.empty(n1)
        self.ctx.check(_lib.lib.scs_sample_system_eval(self.ctx.h, dptr(x), C.cast(Mm.ctypes.data, _lib.c_dp), n1,
                                                       dptr(b)))
        return Mm, b

    def gemv_t(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.empty(self.m)
        self.ctx.check(_lib.lib.scs_gemv_t_eval(self.ctx.h, dptr(v), dptr(out)))
        return out

    def gemv_n(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty(self.N)
        self.ctx.check(_lib.lib.scs_gemv_n_eval(self.ctx.h, dptr(x), dptr(out)))
        return out

    def solve_eval(self, w, dvec, rhs, mode=0):
        """(Aᵀ diag(w) A + diag(dvec)) \\ rhs through the step's solve path (mode 0: Cholesky with
        the LU fallback; 1: the LU).  Returns (x, used_lu)."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        dvec = np.ascontiguousarray(dvec, dtype=np.float64)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.empty(self.m)
        used = C.c_int()
        self.ctx.check(_lib.lib.scs_solve_eval(self.ctx.h, dptr(w), dptr(dvec), dptr(rhs), int(mode), dptr(x),
                                               C.byref(used)))
        return x, bool(used.value)

    def multi_products(self, X=None, V=None):
        """A X (N x K) and Aᵀ V (d x K) through the multi-output kernels (scs_multi_products_eval); X is
        d x K, V is N x K, 1 <= K <= 16 (K need not be the problem's nout).  Returns (AX, ATV), None for
        an operand not given.  With a sparse batch view selected (multi_sparse_batches) the products run on that
        view: N is then the batch's n_b."""
        K = (X if X is not None else V).shape[1]
        N = self._products_rows()
        cap = max(N, self.N) * K   # the buffers hold the full data's rows whatever view the context selects
        ax = atv = Xf = Vf = None
        if X is not None:
            Xf = np.asfortranarray(np.asarray(X, dtype=np.float64))
            if Xf.shape != (self.d, K):
                raise ValueError(f"X must be d x K = ({self.d}, {K})")
            ax = np.zeros(cap)
        if V is not None:
            V = np.asarray(V, dtype=np.float64)
            if V.shape != (N, K):
                raise ValueError(f"V must be N x K = ({N}, {K})")
            Vf = np.zeros(cap)
            Vf[:N * K] = V.reshape(-1, order="F")
            atv = np.zeros((self.d, K), order="F")
        p = lambda a: None if a is None else C.cast(a.ctypes.data, _lib.c_dp)   # noqa: E731
        self.ctx.check(_lib.lib.scs_multi_products_eval(self.ctx.h, int(K), p(Xf), p(Vf), p(ax), p(atv)))
        if ax is not None:
            ax = ax[:N * K].reshape((N, K), order="F")
        return ax, atv

    def multi_system(self, x):
        """(JᵀQJ before λ diag Hr, vec(AᵀR), f) of a multi-output problem at x, by the step's own path
        (scs_multi_system_eval)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        G = np.zeros((self.m, self.m), order="F")
        g = np.empty(self.m)
        f = C.c_double()
        self.ctx.check(_lib.lib.scs_multi_system_eval(self.ctx.h, dptr(x), C.cast(G.ctypes.data, _lib.c_dp), self.m,
                                                      dptr(g), C.byref(f)))
        return G, g, f.value

    def multi_sample_system(self, x):
        """(M, b) of the sample-space system a multi-output ProxGGNSCORE step solves at x (multi_sample=True,
        N·nout + 1 <= d·nout; configure() first: h = 1 ./ Hr and λ gr enter it) -- M of order N·nout + 1, rows and
        columns (i, k) = i + N·k, by the step's own forward pass and assembly (scs_multi_sample_system_eval)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.m,):
            raise ValueError(f"x must have length d * nout = {self.m}")
        n1 = self.N * self.nout + 1
        Mm = np.zeros((n1, n1), order="F")
        b = np.empty(n1)
        self.ctx.check(_lib.lib.scs_multi_sample_system_eval(self.ctx.h, dptr(x), C.cast(Mm.ctypes.data, _lib.c_dp), n1,
                                                             dptr(b)))
        return Mm, b

    def get_columns(self, cols):
        """Columns of the local A (N x len(cols), float64)."""
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        out = np.empty((cols.size, self.N))
        self.ctx.check(_lib.lib.scs_get_columns(self.ctx.h, cols.ctypes.data_as(_lib.c_i64p), cols.size, dptr(out)))
        return out.T

    def gram_atv_sample(self, w, v, pairs):
        """The production Gram launch (Aᵀv fused where a step fuses it): G entries at pairs (k x 2),
        Aᵀv, and whether the pass was fused."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        ij = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        g = np.empty(ij.shape[0])
        atv = np.empty(self.m)
        fused = C.c_int()
        self.ctx.check(_lib.lib.scs_gram_atv_eval(self.ctx.h, dptr(w), dptr(v), ij.ctypes.data_as(_lib.c_i64p),
                                                  ij.shape[0], dptr(g), dptr(atv), C.byref(fused)))
        return g, atv, bool(fused.value)


def lu_solve(A, b, device=0, ctx=None):
    """Julia's `A \\ b` for a dense square matrix (getrf + getrs) on the device: the hand-written
    blocked LU with partial pivoting (lu.hip).  Returns (x, ipiv (0-based), info); with info > 0 (a
    zero pivot, dgetrf's info) x is None and ipiv holds dgetrf's pivots."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    n = A.shape[0]
    if A.shape != (n, n) or b.shape != (n,):
        raise ValueError("A must be n x n and b of length n")
    ctx = ctx or _lib.Context(device)
    x = np.zeros(n)
    ipiv = np.zeros(n, dtype=np.int32)
    info = C.c_int()
    ctx.check(_lib.lib.scs_lu_eval(ctx.h, n, dptr(A), dptr(b), dptr(x), ipiv.ctypes.data_as(_lib.c_i32p),
                                   C.byref(info)))
    return (x if info.value == 0 else None), ipiv, int(info.value)


def chol_solve(M, b, ctx=None, device=0):
    """M x = b for a symmetric positive definite M (potrf + potrs, upper) on the device: the hand-written
    blocked Cholesky (chol.hip) on the sequence a step runs, through the test door scs_chol_eval.  Only
    M's upper triangle is read.  Returns (x, U, info): U the upper factor M = UᵀU (strict lower triangle
    zeroed), info dpotrf's (the first non-positive pivot, 1-based; x is then None)."""
    M = np.asarray(M, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    n = M.shape[0]
    if M.shape != (n, n) or b.shape != (n,):
        raise ValueError("M must be n x n and b of length n")
    Mc = np.ascontiguousarray(M.T)   # the door's column-major M
    ctx = ctx or _lib.Context(device)
    x = np.zeros(n)
    Uc = np.zeros((n, n))
    info = C.c_int()
    ctx.check(_lib.lib.scs_chol_eval(ctx.h, n, dptr(Mc), dptr(b), dptr(x), dptr(Uc), C.byref(info)))
    return (x if info.value == 0 else None), np.triu(Uc.T), int(info.value)


def qr_solve(A, b, ctx=None, device=0):
    """A x = b for a dense square matrix by Householder QR (geqrf conventions) on the device (qr.hip),
    on the sequence of the sample-space system, through the test door scs_qr_eval.  Returns (x, R): R
    the upper triangular factor (strict lower triangle zeroed)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    n = A.shape[0]
    if A.shape != (n, n) or b.shape != (n,):
        raise ValueError("A must be n x n and b of length n")
    ctx = ctx or _lib.Context(device)
    x = np.zeros(n)
    Rc = np.zeros((n, n))
    ctx.check(_lib.lib.scs_qr_eval(ctx.h, n, dptr(A), dptr(b), dptr(x), dptr(Rc)))
    return x, np.triu(Rc.T)

