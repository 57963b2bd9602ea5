"""Python host mirror of the cpkrylov interface, running on MI355X through libcpk.

Reference (MATLAB)                                   This module
-------------------------------------------------   ------------------------------------------
[x,stats,flag] = reg_cpkrylov(method,b,A,B,C,G,opts) x, stats, flag = reg_cpkrylov(method, b, A, B, C, G, opts)
   (reg_cpkrylov.m:1)
[x,y,stats,flag] = cpminres(b,A,C,M,opts)            x, y, stats, flag = cpminres(b, A, C, M, opts)
   (kernels/cpminres.m:1; same for cpcg, cpcglanczos, cpsymmlq, cpgmres, cpdqgmres)
M = opLDL2(A,B,C); M.nitref = 1; y = M*z            M = opLDL2(A, B, C); M.nitref = 1; y = M * z
   (ops/opLDL2.m:60, 45-50, 161)
[c,s,d] = SymGivens(a,b)  (util/SymGivens.m:1)       c, s, d = SymGivens(a, b)

`opts` is a dict whose keys behave like MATLAB struct fields (absent = solver default).
`stats` / `flag` are dicts with the reference's field names.  Matrices are scipy.sparse (or
dense numpy) arrays; `A` may also be an `Operator`, a product on device memory (the reference's
"A may be a matrix or a linear operator"; a scipy LinearOperator works on host arrays and is
refused).  Errors raise CpkError / IndefiniteError.
"""
import ctypes as C
import os
import sys

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import CpkError, IndefiniteError, check, lib, make_opts

_P = C.POINTER


def _dptr(a):
    return a.ctypes.data_as(_P(C.c_double))


class Context:
    """One GPU, one HIP stream (and an RCCL communicator when nranks > 1).

    timing_standin=True (diagnostic, cpk_ctx_create_null): rank `rank` of an nranks-way context
    whose collectives are no-ops -- one rank's share of the work, timed on one GPU; its results
    are meaningless."""

    def __init__(self, device=None, rank=0, nranks=1, unique_id=None, simgroup=None, options=None,
                 timing_standin=False):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        h = C.c_void_p()
        if simgroup is not None:  # ranks as threads on one GPU (tests), see cpk_ctx_create_sim
            check(lib.cpk_ctx_create_sim(device, simgroup.h, rank, nranks, C.byref(h)))
        elif timing_standin:
            check(lib.cpk_ctx_create_null(device, rank, nranks, C.byref(h)))
        else:
            uid = None
            if unique_id is not None:
                buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
                uid = C.cast(buf, _P(C.c_ubyte))
            check(lib.cpk_ctx_create(device, rank, nranks, uid, C.byref(h)))
        self.h = h
        self.device, self.rank, self.nranks = device, rank, nranks
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        """Engine option of this context (cpk_ctx_set_option); applies to objects created later."""
        if isinstance(value, bool):
            value = "1" if value else "0"
        check(lib.cpk_ctx_set_option(self.h, name.encode(), str(value).encode()))

    def get_option(self, name):
        """The value this context's objects use (sweep: the per-path default unless set)."""
        buf = C.create_string_buffer(256)
        check(lib.cpk_ctx_get_option(self.h, name.encode(), buf, 256))
        return buf.value.decode()

    def options_string(self):
        """Every engine option as "name=value;..." (cpk_ctx_get_options): analyze(options=...)
        and dist_plan(options=...) then plan exactly as this context's preconditioners."""
        buf = C.create_string_buffer(4096)
        check(lib.cpk_ctx_get_options(self.h, buf, 4096))
        return buf.value.decode()

    def info(self):
        """device, rank, nranks, the communicator's kind and rank count (RCCL: ncclCommCount),
        and whether preconditioners built here take the distributed path (cpk_ctx_get_info)."""
        v = (C.c_int64 * 8)()
        check(lib.cpk_ctx_get_info(self.h, v))
        return {"device": v[0], "rank": v[1], "nranks": v[2], "comm": _lib.COMM_KINDS.get(v[3], str(v[3])),
                "comm_ranks": v[4], "distributed": bool(v[5])}

    def synchronize(self):
        check(lib.cpk_ctx_synchronize(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib.cpk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SimGroup:
    """A group of `nranks` simulated ranks sharing one GPU (one thread per rank)."""

    def __init__(self, nranks):
        h = C.c_void_p()
        check(lib.cpk_simgroup_create(int(nranks), C.byref(h)))
        self.h, self.nranks = h, nranks

    def __del__(self):
        if getattr(self, "h", None):
            lib.cpk_simgroup_destroy(self.h)
            self.h = None


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


class engine_options:
    """Context manager: engine options of a context (default: the default context) for the
    duration of a block, restored afterwards -- e.g. `with engine_options(sweep="256,768,64"):`."""

    def __init__(self, ctx=None, **kw):
        self.ctx, self.kw, self.old = ctx, kw, {}

    def __enter__(self):
        self.ctx = self.ctx or default_context()
        for k, v in self.kw.items():
            self.old[k] = self.ctx.get_option(k)
            self.ctx.set_option(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)
        return False


def get_unique_id():
    buf = (C.c_ubyte * 128)()
    check(lib.cpk_get_unique_id(buf))
    return bytes(buf)


class Matrix:
    """A sparse matrix handle (host copy + lazily uploaded HBM copy)."""

    def __init__(self, M, ctx=None, host_only=False, csc=False):
        """csc=True hands the matrix over as MATLAB stores it (mxGetJc / mxGetIr / mxGetPr:
        0-based, size_t column pointers and row indices), through cpk_mat_create_csc -- the
        entry the MEX gateway uses (matlab/cpk_mex.c)."""
        if isinstance(M, Matrix):
            raise TypeError("already a Matrix")
        if not sp.issparse(M):
            M = np.asarray(M, dtype=np.float64)
            if M.ndim != 2:
                raise CpkError(_lib.CPK_ERR_ARGS, "matrix expected")
            M = sp.csr_matrix(M)
        self.ctx = None if host_only else (ctx or default_context())
        h = C.c_void_p()
        cx = self.ctx.h if self.ctx else None
        if csc:
            M = sp.csc_matrix(M, dtype=np.float64)
            M.sum_duplicates()
            M.sort_indices()
            self.shape = M.shape
            self._ptr = np.ascontiguousarray(M.indptr, dtype=np.uintp)
            self._ind = np.ascontiguousarray(M.indices, dtype=np.uintp)
            self._val = np.ascontiguousarray(M.data, dtype=np.float64)
            check(lib.cpk_mat_create_csc(cx, M.shape[0], M.shape[1], self._ptr.ctypes.data_as(_P(C.c_size_t)),
                                         self._ind.ctypes.data_as(_P(C.c_size_t)), _dptr(self._val), C.byref(h)))
        else:
            M = sp.csr_matrix(M, dtype=np.float64)
            M.sum_duplicates()
            M.sort_indices()
            self.shape = M.shape
            self._ptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
            self._ind = np.ascontiguousarray(M.indices, dtype=np.int32)
            self._val = np.ascontiguousarray(M.data, dtype=np.float64)
            check(lib.cpk_mat_create_csr(cx, M.shape[0], M.shape[1], self._ptr.ctypes.data_as(_P(C.c_int64)),
                                         self._ind.ctypes.data_as(_P(C.c_int32)), _dptr(self._val), C.byref(h)))
        self.h = h
        self._csc = bool(csc)

    def set_values(self, v):
        """New values with the same sparsity, written into this handle (cpk_mat_set_values /
        cpk_mat_set_values_device): the device copy, the Krylov operators cached on the handle and
        the solvers a preconditioner cached (with their captured graphs) all stay and see the new
        values at their next use; a preconditioner changes at its next `refactor`.  v is one of
          * a NumPy array in the order of the canonical (sorted, duplicate-free) CSR data the
            constructor passed down -- CSC data for a matrix created with csc=True;
          * a scipy.sparse matrix, canonicalised as the constructor does; CPK_ERR_ARGS unless its
            indptr and indices equal this handle's;
          * a device tensor (anything with is_cuda, data_ptr(), dtype and is_contiguous(), e.g. a
            torch tensor on the GPU) in the same order: float64 and contiguous; its current stream
            is synchronised, then the values are gathered on the device with no host round trip.
        """
        if all(hasattr(v, a) for a in ("is_cuda", "data_ptr", "dtype", "is_contiguous")):
            if not v.is_cuda:
                v = v.detach().cpu().numpy()  # a host tensor: the NumPy path below
            else:
                if "float64" not in str(v.dtype) or not v.is_contiguous():
                    raise CpkError(_lib.CPK_ERR_ARGS, "set_values: a contiguous float64 device tensor expected")
                mod = sys.modules[type(v).__module__.split(".")[0]]  # the tensor's own library, already loaded
                mod.cuda.current_stream(v.device).synchronize()
                return self.set_values_device(v.data_ptr(), v.numel())
        if sp.issparse(v):
            M = (sp.csc_matrix if self._csc else sp.csr_matrix)(v, dtype=np.float64)
            M.sum_duplicates()
            M.sort_indices()
            if M.shape != tuple(self.shape) or not (np.array_equal(M.indptr, self._ptr) and np.array_equal(M.indices, self._ind)):
                raise CpkError(_lib.CPK_ERR_ARGS, "set_values: the sparsity differs from this matrix's")
            v = M.data
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        check(lib.cpk_mat_set_values(self.h, _dptr(v) if v.size else None, v.size))
        self._val = v.copy()

    def set_values_device(self, ptr, count):
        """The same from `count` float64 values at device address `ptr`, complete when the call is
        made; blocks until they are consumed (cpk_mat_set_values_device)."""
        check(lib.cpk_mat_set_values_device(self.h, C.c_void_p(int(ptr) if ptr else None), int(count)))
        self._val = None  # this object's host values are no longer the matrix's

    def sample_outer(self, U, V, alpha=1.0, out=None):
        """g = alpha * (u_0 v_0' + ... + u_{k-1} v_{k-1}') sampled on this matrix's sparsity, in the
        order `set_values` takes values in (cpk_mat_sample_outer[_device]): the transpose of
        `set_values`, a gradient with respect to those values.  Each entry's sum starts at 0.0 and
        adds the separately rounded products in column order, alpha last; the matrix's values are
        not read.  U (nrows x k) and V (ncols x k) are NumPy arrays (a vector is one column), and
        the result is a new array or `out`; or both are device tensors (float64, contiguous, one
        column after the other, so a (k, nrows) row-major tensor is the block) and the result goes
        to the device tensor passed as out=, complete when the call returns."""
        count = self.info()["entries"]
        if _is_device(U) or _is_device(V):
            if not (_is_device(U) and _is_device(V) and out is not None and _is_device(out)):
                raise CpkError(_lib.CPK_ERR_ARGS, "sample_outer on device operands: U, V and out= are device tensors")
            up, k, ldu = _device_operand(U, "U", self.shape[0])
            vp, kv, ldv = _device_operand(V, "V", self.shape[1])
            op, _, _ = _device_operand(out, "out", count)
            if kv != k:
                raise CpkError(_lib.CPK_ERR_DIM, "U and V must have the same number of columns")
            check(lib.cpk_mat_sample_outer_device(self.h, k, up, ldu, vp, ldv, float(alpha), op, int(out.numel())))
            check(lib.cpk_ctx_synchronize(self.ctx.h))
            return out
        U, V = (np.asarray(a, dtype=np.float64) for a in (U, V))
        U, V = (np.asfortranarray(a.reshape(a.shape[0], -1) if a.ndim else a.reshape(1, 1)) for a in (U, V))
        if U.shape[0] != self.shape[0] or V.shape[0] != self.shape[1] or U.shape[1] != V.shape[1]:
            raise CpkError(_lib.CPK_ERR_DIM, "sample_outer: U is nrows x k and V is ncols x k")
        if out is None:
            out = np.zeros(count)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous):
            raise CpkError(_lib.CPK_ERR_ARGS, "sample_outer: out is a contiguous float64 array")
        check(lib.cpk_mat_sample_outer(self.h, U.shape[1], _dptr(U), max(self.shape[0], 1), _dptr(V), max(self.shape[1], 1),
                                       float(alpha), _dptr(out) if out.size else None, out.size))
        return out

    def info(self):
        """Diagnostic (cpk_mat_get_info): sizes, the values generation (0 at creation, +1 per
        successful set_values), whether a device copy exists, and the Krylov operators
        blkdiag(self, C) cached on this handle."""
        v = (C.c_int64 * 8)()
        check(lib.cpk_mat_get_info(self.h, v))
        return {"nrows": v[0], "ncols": v[1], "nnz": v[2], "entries": v[3], "values_generation": v[4],
                "device_copy": bool(v[5]), "krylov_operators": v[6]}

    def __matmul__(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.shape[0])
        check(lib.cpk_mat_spmv(self.h, _dptr(x), _dptr(y)))
        return y

    def __del__(self):
        if getattr(self, "h", None):
            lib.cpk_mat_destroy(self.h)
            self.h = None


def _as_matrix(M, ctx):
    if isinstance(M, Matrix):
        return M
    if isinstance(M, Operator):
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED, "an Operator stands for A in a single-column solve only; "
                       "B, C, G, the preconditioner's blocks and K's blocks must be matrices")
    if isinstance(M, sp.linalg.LinearOperator):
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED,
                       "a scipy LinearOperator works on host arrays; wrap a device product in cpk.Operator")
    return Matrix(M, ctx)


class _DeviceView:
    """n float64 values at a device address, as __cuda_array_interface__ describes them (torch
    takes writable views only, so the input's view is writable too: f must not write to x)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Operator:
    """The (1,1) block A as a product on device memory (cpk_op): `fn(x_ptr, y_ptr, n, stream_ptr)`
    enqueues y[0:n) = A @ x[0:n) (float64 device addresses as ints) on the HIP stream
    `stream_ptr`, and returns None / 0, or nonzero to abort the solve.  The solvers take it where
    they take the matrix A: cpcg ... cpdqgmres(b, A, C, M, opts) and
    reg_cpkrylov(method, b, A, B, C, G, opts), one right-hand side, one GPU.

    capturable=False (default): fn is called eagerly, once per Krylov product, and may do
    anything on the stream; the solver runs one iteration per batch without graphs, so fn is
    never called for an iteration that has already stopped.  capturable=True: fn may be called
    while the stream is capturing -- it must only enqueue on `stream_ptr` (no synchronisation,
    allocation or other stream) and what it enqueues may depend only on its arguments and on
    device memory, because it is called once per captured iteration and replays do not call it.

    An exception raised in fn aborts the solve: the CpkError (CPK_ERR_CALLBACK) the solve raises
    carries it as __cause__.  A's symmetry is the caller's responsibility."""

    def __init__(self, n, fn, ctx=None, capturable=False):
        if not callable(fn):
            raise CpkError(_lib.CPK_ERR_ARGS, "Operator: fn must be callable")
        if int(n) != n or int(n) < 0:
            raise CpkError(_lib.CPK_ERR_ARGS, "Operator: n must be an integer >= 0")
        self.n, self.shape, self.capturable = int(n), (int(n), int(n)), bool(capturable)
        self._fn, self._exc = fn, None

        def trampoline(_user, x, y, nn, stream):
            try:
                rc = fn(x or 0, y or 0, nn, stream or 0)
                return int(rc) if rc else 0
            except BaseException as e:  # nothing may propagate through the C frames
                self._exc = e
                return -1

        self._cb = _lib.OpFn(trampoline)  # kept alive with the handle
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib.cpk_op_create(self.ctx.h, self.n, self._cb, None, _lib.CPK_OP_CAPTURABLE if capturable else 0,
                                C.byref(h)))
        self.h = h

    @classmethod
    def from_torch(cls, n, f, ctx=None):
        """A from a torch function f(x: Tensor) -> Tensor (an autograd Hessian-vector product, a
        dense mv, ...): x and the result's destination are zero-copy views of the engine's buffers
        (__cuda_array_interface__), and f runs under torch.cuda.ExternalStream(stream_ptr), so its
        kernels are ordered with the solver's.  Always non-capturable."""
        import torch

        views = {}

        def fn(x_ptr, y_ptr, nn, stream_ptr):
            if nn == 0:
                return 0
            key = (x_ptr, y_ptr, nn)
            if key not in views:
                views[key] = (torch.as_tensor(_DeviceView(x_ptr, nn), device="cuda"),
                              torch.as_tensor(_DeviceView(y_ptr, nn), device="cuda"))
            x, y = views[key]
            with torch.cuda.stream(torch.cuda.ExternalStream(stream_ptr)):
                y.copy_(f(x))
            return 0

        return cls(n, fn, ctx=ctx, capturable=False)

    def info(self):
        """cpk_op_get_info: n, capturable, the calls of fn so far and those that returned nonzero."""
        v = (C.c_int64 * 4)()
        check(lib.cpk_op_get_info(self.h, v))
        return {"n": v[0], "capturable": bool(v[1] & _lib.CPK_OP_CAPTURABLE), "calls": v[2], "failed": v[3]}

    def _solve(self, call):
        """Run one C solve entry; an exception fn raised becomes the cause of the solve's error."""
        self._exc = None
        rc = call()
        if rc != _lib.CPK_OK:
            exc, self._exc = self._exc, None
            try:
                check(rc)
            except CpkError as e:
                if exc is not None and rc == _lib.CPK_ERR_CALLBACK:
                    raise e from exc
                raise

    def __del__(self):
        if getattr(self, "h", None):
            lib.cpk_op_destroy(self.h)
            self.h = None


class opLDL2:
    """Operator for the inverse of [A B'; B C] via its LDL' factorization (ops/opLDL2.m).

    Public properties with the reference's setter semantics (opLDL2.m:45-50, 97-115):
      nitref          = max(0, round(val))          (default 3)
      itref_tol       stored as given (the reference's `sef.itref_tol` typo) (default 1e-8)
      force_itref     anything other than false/true becomes false (default false)
      residual_update stored as given (default false); a functional no-op, as in the reference

    `M * z` / `M @ z` with a vector (or an N x 1 array) is opLDL2.multiply; with an N x k array,
    k != 1, it is the block apply `apply_block`: M on every column, bit for bit.
    """

    def __init__(self, A, B, Cm, ctx=None, _handle=None, krylov_A=None):
        """krylov_A (optional): the Krylov operator's A, a placement hint for a distributed
        context (cpk_pc_create_hint); ignored on one GPU."""
        self.ctx = ctx or default_context()
        if _handle is not None:
            self.h = _handle
        else:
            mats = [_as_matrix(M, self.ctx) for M in (A, B, Cm)]
            h = C.c_void_p()
            pt = C.c_double()
            if krylov_A is not None:
                ka = _as_matrix(krylov_A, self.ctx)
                check(lib.cpk_pc_create_hint(self.ctx.h, mats[0].h, mats[1].h, mats[2].h, ka.h, C.byref(pt),
                                             C.byref(h)))
            else:
                check(lib.cpk_pc_create(self.ctx.h, mats[0].h, mats[1].h, mats[2].h, C.byref(pt), C.byref(h)))
            self.h = h
            self.ptime = pt.value
        info = _lib.PcInfo()
        check(lib.cpk_pc_get_info(self.h, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in _lib.PcInfo._fields_}
        self.nA, self.nC, self.n = info.n, info.m, info.N
        self.shape = (info.N, info.N)

    def refactor(self, A, B, Cm):
        """New values of (A, B, C) with the sparsity this operator was built with: the factors
        of opLDL2(A, B, C) recomputed on the device, symbolic analysis reused (cpk_pc_refactor;
        an IPM outer iteration's rebuild of opLDL2, opLDL2.m:60-92).  Returns the seconds taken.
        A, B, Cm may be `Matrix` objects: the handles this operator was built from, updated in
        place with `Matrix.set_values`, are refactored from their device copies with nothing
        converted or uploaded again."""
        mats = [_as_matrix(M, self.ctx) for M in (A, B, Cm)]
        pt = C.c_double()
        check(lib.cpk_pc_refactor(self.h, mats[0].h, mats[1].h, mats[2].h, C.byref(pt)))
        self.ptime = pt.value
        return pt.value

    # ---- properties --------------------------------------------------------------------------
    def _get(self):
        v = [C.c_double() for _ in range(4)]
        check(lib.cpk_pc_get(self.h, *[C.byref(x) for x in v]))
        return [x.value for x in v]

    def _set(self, **kw):
        check(lib.cpk_pc_set(self.h, C.byref(make_opts(kw))))

    nitref = property(lambda s: s._get()[0], lambda s, v: s._set(nitref=v))
    itref_tol = property(lambda s: s._get()[1], lambda s, v: s._set(itref_tol=v))
    force_itref = property(lambda s: bool(s._get()[2]), lambda s, v: s._set(force_itref=v))
    residual_update = property(lambda s: s._get()[3], lambda s, v: s._set(residual_update=v))

    @property
    def handle_semantics(self):
        """Opt-in (not in the reference): keep op.Aty / op.Cy between applies (cpk_pc_set_handle)."""
        return getattr(self, "_handle", False)

    @handle_semantics.setter
    def handle_semantics(self, on):
        check(lib.cpk_pc_set_handle(self.h, 1 if on else 0))
        self._handle = bool(on)

    # ---- operator surface --------------------------------------------------------------------
    def __mul__(self, z):
        z = np.asarray(z, dtype=np.float64)
        if z.ndim == 2 and z.shape[1] != 1:  # a block: M*Z column by column (apply_block)
            return self.apply_block(z)
        z = np.ascontiguousarray(z).ravel()
        if z.shape[0] != self.n:
            raise CpkError(_lib.CPK_ERR_DIM, "Dimensions do not match")
        y = np.empty(self.n)
        check(lib.cpk_pc_apply(self.h, _dptr(z), _dptr(y)))
        return y

    __matmul__ = __mul__

    def apply_block(self, Z, return_steps=False):
        """Y = M*Z for an N x k array (any memory order), defined column by column: Y[:, j] equals
        `M * Z[:, j]` bit for bit under the current nitref / itref_tol / force_itref, each column
        with its own refinement predicate (cpk_pc_apply_multi: panels of 8 columns stream the
        factor and Kp once per panel).  return_steps: also the refinement solves each column
        took (int32, 0...nitref).  The reference's matrix path (norm(r) over the whole block) is
        not reproduced."""
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[0] != self.n:
            raise CpkError(_lib.CPK_ERR_DIM, "Dimensions do not match")
        k = Z.shape[1]
        X = np.asfortranarray(Z)
        Y = np.empty((self.n, k), order="F")
        nit = np.zeros(k, np.int32)
        if k:
            check(lib.cpk_pc_apply_multi(self.h, k, _dptr(X), max(self.n, 1), _dptr(Y), max(self.n, 1),
                                         nit.ctypes.data_as(_P(C.c_int32))))
        return (Y, nit) if return_steps else Y

    def divide(self, b):
        """M \\ b = Kp*b  (opLDL2.divide, opLDL2.m:193-195)."""
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        x = np.empty(self.n)
        check(lib.cpk_pc_divide(self.h, _dptr(b), _dptr(x)))
        return x

    def transpose(self):  # opLDL2.m:120-122
        return self

    T = property(transpose)

    def ctranspose(self):  # opLDL2.m:134-136: M' is the bare factor composite, not M
        return opLDL2Factor(self)

    H = property(ctranspose)
    conj = ctranspose  # opLDL2.m:127-129: the same composite

    def solver_info(self):
        """Diagnostic (cpk_pc_solver_info): the solvers this operator caches and the hipGraph
        instantiations they made so far -- a solve that replays cached graphs adds none."""
        v = (C.c_int64 * 4)()
        check(lib.cpk_pc_solver_info(self.h, v))
        return dict(zip(("solvers", "graph_instantiations", "block_solvers", "block_graph_instantiations"), list(v)))

    def multi_info(self):
        """Diagnostic: the multi-column sweep of M' as launched (cpk_pc_multi_info)."""
        v = (C.c_int64 * 4)()
        check(lib.cpk_pc_multi_info(self.h, v))
        return dict(zip(("kp", "launches", "staged_blocks", "direct_blocks"), list(v)))

    def to_dense(self, chunk=64):
        """double(op), opLDL2.m:138-149: one op*e per column, `chunk` columns per block apply
        (device memory O(N * chunk)); bit-equal to the loop of `self * e_j`."""
        X = np.empty((self.n, self.n), order="F")
        if self.ctx.info()["distributed"] or (self.handle_semantics and self.residual_update):
            # the block entry is single-GPU and keeps no residual-update state: one apply per column
            e = np.zeros(self.n)
            for i in range(self.n):
                e[i] = 1
                X[:, i] = self * e
                e[i] = 0
            return X
        for j0 in range(0, self.n, chunk):
            j1 = min(self.n, j0 + chunk)
            E = np.zeros((self.n, j1 - j0), order="F")
            E[np.arange(j0, j1), np.arange(j1 - j0)] = 1.0
            X[:, j0:j1] = self.apply_block(E)
        return X

    def sep_info(self):
        """Diagnostic: the distributed separator solve's staging (cpk_pc_sep_info)."""
        v = (C.c_int64 * 12)()
        check(lib.cpk_pc_sep_info(self.h, v))
        return dict(zip(("dist", "nT", "nlev", "nrec", "lds", "lds_g", "kt", "tkr", "sched", "fused", "tsweep",
                         "tsweep_rounds"), list(v)))

    def sweep_info(self):
        """Diagnostic: the sweep schedule as launched (cpk_pc_sweep_info)."""
        v = (C.c_int64 * 8)()
        check(lib.cpk_pc_sweep_info(self.h, v))
        return dict(zip(("rounds", "round0_blocks", "upper_blocks", "round0_assigned", "resid_assigned",
                         "bwd_assigned", "persistent", "chain_tasks"), list(v)))

    def block_model(self):
        """Diagnostic: the upper rounds' loop-cost model (cpk_debug_block_model), one row per
        (upper block, direction): block, direction (0 forward), rows, level trips, dataflow trips,
        outside terms behind in-block ones, column sweep valid, loop chosen (0 level, 1 dataflow,
        2 / 3 column sweep without / with drains, 4 row-span), row-span eligible, its drain trips."""
        n = C.c_int64(0)
        check(lib.cpk_debug_block_model(self.h, None, 1 << 40, C.byref(n)))
        mod = np.zeros(max(n.value, 1), np.int64)
        check(lib.cpk_debug_block_model(self.h, mod.ctypes.data_as(_P(C.c_int64)), n.value, C.byref(n)))
        return mod[:n.value].reshape(-1, 10)

    def local_dofs(self):
        """Global indices of this rank's local vector entries ([x-part; y-part]) and n_loc."""
        nl, ml = C.c_int64(), C.c_int64()
        check(lib.cpk_pc_local_dofs(self.h, C.byref(nl), C.byref(ml), None))
        d = np.empty(nl.value + ml.value, np.int32)
        check(lib.cpk_pc_local_dofs(self.h, C.byref(nl), C.byref(ml), d.ctypes.data_as(_P(C.c_int32))))
        return d, nl.value

    def export_factors(self):
        """(L (CSC, strict lower), D, perm) with P'*Kp*P = L*D*L', perm[k] = original index."""
        N, nnz = self.info["N"], self.info["nnz_l"]
        Lp = np.empty(N + 1, np.int64)
        Li = np.empty(max(nnz, 1), np.int32)
        Lx = np.empty(max(nnz, 1))
        D = np.empty(N)
        perm = np.empty(N, np.int32)
        check(lib.cpk_pc_export(self.h, Lp.ctypes.data_as(_P(C.c_int64)), Li.ctypes.data_as(_P(C.c_int32)),
                                _dptr(Lx), _dptr(D), perm.ctypes.data_as(_P(C.c_int32))))
        L = sp.csc_matrix((Lx[:nnz], Li[:nnz], Lp), shape=(N, N))
        return L, D, perm

    def factor_report(self):
        """What the last successful factorization (construction or refactor) found, as a dict of
        cpk_factor_report's fields: the inertia (n_pos, n_neg) and pivot information MA57's ldl
        returns with the factors (opLDL2.m:81-82).  Positions index D and perm of
        export_factors()."""
        r = _lib.FactorReport()
        check(lib.cpk_pc_factor_report(self.h, C.byref(r)))
        return _report_dict(r)

    def pivot_shift(self):
        """E (N values, original dof order): the factors are those of Kp + diag(E) exactly; zeros
        unless the engine option pivot_min replaced pivots.  M's Kp stays the unperturbed matrix."""
        E = np.empty(self.info["N"])
        check(lib.cpk_pc_pivot_shift(self.h, _dptr(E)))
        return E

    def __del__(self):
        if getattr(self, "h", None):
            lib.cpk_pc_destroy(self.h)
            self.h = None


def _report_dict(r):
    return {k: getattr(r, k) for k, _ in _lib.FactorReport._fields_}


class opLDL2Factor:
    """M' and conj(M) of an opLDL2: the bare factor composite P*L'^-1*D^-1*L^-1*P'
    (opLDL2.m:127-136), applied once -- no refinement, no residual update, none of M's properties
    read or written.  It shares M's handle and keeps M alive.  It takes a block of
    right-hand sides: `F @ X` with an N x k array solves the k columns in panels, streaming the
    factor once per panel (cpk_pc_apply_ldl_multi); each column equals `F * X[:, j]` bit for bit."""

    def __init__(self, parent):
        self.parent = parent
        self.n = parent.n
        self.shape = parent.shape

    def __mul__(self, z):
        z = np.asarray(z, dtype=np.float64)
        h = self.parent.h
        if z.ndim == 2:
            if z.shape[0] != self.n:
                raise CpkError(_lib.CPK_ERR_DIM, "Dimensions do not match")
            X = np.asfortranarray(z)
            Y = np.empty((self.n, z.shape[1]), order="F")
            if z.shape[1]:
                check(lib.cpk_pc_apply_ldl_multi(h, z.shape[1], _dptr(X), max(self.n, 1), _dptr(Y), max(self.n, 1)))
            return Y
        z = np.ascontiguousarray(z).ravel()
        if z.shape[0] != self.n:
            raise CpkError(_lib.CPK_ERR_DIM, "Dimensions do not match")
        y = np.empty(self.n)
        check(lib.cpk_pc_apply_ldl(h, _dptr(z), _dptr(y)))
        return y

    __matmul__ = __mul__

    def transpose(self):  # the composite is symmetric and real
        return self

    T = property(transpose)
    ctranspose = transpose
    H = property(transpose)
    conj = transpose

    def to_dense(self, chunk=64):
        """double(op) = op * eye(n), `chunk` columns at a time (device memory O(N * chunk))."""
        X = np.empty((self.n, self.n), order="F")
        for j0 in range(0, self.n, chunk):
            j1 = min(self.n, j0 + chunk)
            E = np.zeros((self.n, j1 - j0), order="F")
            E[np.arange(j0, j1), np.arange(j1 - j0)] = 1.0
            X[:, j0:j1] = self @ E
        return X


def _options_spec(ctx, options):
    """The engine-option spec of cpk_analyze: a context's full set (so the analysis plans as that
    context's preconditioner would), then `options` (dict or "name=value;..." string) on top."""
    parts = []
    if ctx is not None:
        parts.append(ctx.options_string())
    if isinstance(options, dict):
        parts.append("".join(f"{k}={('1' if v else '0') if isinstance(v, bool) else v};" for k, v in options.items()))
    elif options:
        parts.append(str(options))
    return ";".join(p.strip(";") for p in parts if p).encode() if parts else None


def analyze(A, B, Cm, ctx=None, options=None):
    """Host-only half of opLDL2(A, B, C) (no GPU): ordering, LDL', sweep schedule.  Engine
    options: the CPK_* environment, then those of `ctx` (if given), then `options`."""
    mats = [M if isinstance(M, Matrix) else Matrix(M, host_only=True) for M in (A, B, Cm)]
    h = C.c_void_p()
    check(lib.cpk_analyze(mats[0].h, mats[1].h, mats[2].h, _options_spec(ctx, options), C.byref(h)))
    try:
        info = _lib.PcInfo()
        check(lib.cpk_analysis_get_info(h, C.byref(info)))
        info = {k: getattr(info, k) for k, _ in _lib.PcInfo._fields_}
        N, nnz = info["N"], info["nnz_l"]
        Lp = np.empty(N + 1, np.int64)
        Li = np.empty(max(nnz, 1), np.int32)
        Lx = np.empty(max(nnz, 1))
        D = np.empty(N)
        perm = np.empty(N, np.int32)
        check(lib.cpk_analysis_export(h, Lp.ctypes.data_as(_P(C.c_int64)), Li.ctypes.data_as(_P(C.c_int32)),
                                      _dptr(Lx), _dptr(D), perm.ctypes.data_as(_P(C.c_int32))))
        nl = C.c_int64()
        check(lib.cpk_analysis_schedule(h, C.byref(nl), None, None, None, None))
        rp = np.empty(info["nrounds"] + 1, np.int64)
        bl = np.empty(info["nblocks"] + 1, np.int64)
        lr = np.empty(nl.value + 1, np.int64)
        order = np.empty(N, np.int32)
        check(lib.cpk_analysis_schedule(h, None, rp.ctypes.data_as(_P(C.c_int64)), bl.ctypes.data_as(_P(C.c_int64)),
                                        lr.ctypes.data_as(_P(C.c_int64)), order.ctypes.data_as(_P(C.c_int32))))
        rcap, rrows = np.empty(info["nrounds"], np.int32), np.empty(info["nrounds"], np.int32)
        check(lib.cpk_analysis_round_caps(h, rcap.ctypes.data_as(_P(C.c_int32)), rrows.ctypes.data_as(_P(C.c_int32))))
        rep = _lib.FactorReport()
        check(lib.cpk_analysis_factor_report(h, C.byref(rep)))
        E = np.empty(N)
        check(lib.cpk_analysis_pivot_shift(h, _dptr(E)))
    finally:
        lib.cpk_analysis_destroy(h)
    L = sp.csc_matrix((Lx[:nnz], Li[:nnz], Lp), shape=(N, N))
    return dict(info=info, L=L, D=D, perm=perm, round_ptr=rp, blk_lvl=bl, lvl_row=lr, order=order,
                round_cap=rcap, round_rows=rrows, report=_report_dict(rep), E=E)


_PLAN_F64 = {"fsub_Lx", "fsub_D", "extra_val", "tf_val", "tb_val", "DT", "kp_val", "ac_val", "ab_val"}
_PLAN_NAMES = ("sizes", "dofs", "node_rank", "T", "fsub_Lp", "fsub_Li", "fsub_Lx", "fsub_D", "fsub_perm",
               "fsub_parent", "fsub_key", "extra_ptr", "extra_col", "extra_key", "extra_val", "tf_ptr", "tf_col",
               "tf_val", "tf_src", "tb_ptr", "tb_col", "tb_val", "DT", "tlev_ptr", "tlev_rows", "tsend", "tdof") + \
    tuple(f"{k}_{a}" for k in ("kp", "ac", "ab") for a in ("ptr", "col", "val", "send"))


def rowspan_layouts(A, B, Cm, ctx=None, options=None, cap_entries=0):
    """Host-only (no GPU): the row-span layout (cpk_analysis_rowspan) of every upper-round block of
    opLDL2(A, B, C)'s sweep schedule and both directions, as the device layout builds it.  A list
    of dicts: block, dir, eligible, r0, nr, rowptr, col, val, step and, where eligible, slots, ndr,
    nrp, trips, dset, dest, lead, mask (nr x 2, by step), base, first, run0 (by step), tab
    (ndr x nrp)."""
    mats = [M if isinstance(M, Matrix) else Matrix(M, host_only=True) for M in (A, B, Cm)]
    h = C.c_void_p()
    check(lib.cpk_analyze(mats[0].h, mats[1].h, mats[2].h, _options_spec(ctx, options), C.byref(h)))
    out = []
    try:
        info = _lib.PcInfo()
        check(lib.cpk_analysis_get_info(h, C.byref(info)))
        rp = np.empty(info.nrounds + 1, np.int64)
        check(lib.cpk_analysis_schedule(h, None, rp.ctypes.data_as(_P(C.c_int64)), None, None, None))
        i32, i64 = (lambda n: np.zeros(max(n, 1), np.int32)), (lambda n: np.zeros(max(n, 1), np.int64))
        ptr = lambda a, t: a.ctypes.data_as(_P(t))  # noqa: E731
        for b in range(int(rp[1]) if len(rp) > 2 else int(rp[-1]), int(rp[-1])):
            for d in (0, 1):
                ri = _lib.RowspanInfo()
                check(lib.cpk_analysis_rowspan(h, b, d, cap_entries, C.byref(ri), *([None] * 11)))
                nr, ne = ri.nr, ri.ne
                rowptr, col, val, dest, step, lead = i64(nr + 1), i32(ne), np.zeros(max(ne, 1)), i32(ne), i32(nr), i32(nr)
                mask, base, first, run0 = np.zeros(2 * max(nr, 1), np.uint64), i32(nr), i32(nr), i32(nr)
                tab = np.zeros(max(ri.ndr * ri.nrp, 1), np.uint8)
                check(lib.cpk_analysis_rowspan(h, b, d, cap_entries, C.byref(ri), ptr(rowptr, C.c_int64), ptr(col, C.c_int32),
                                               _dptr(val), ptr(dest, C.c_int32), ptr(step, C.c_int32),
                                               ptr(lead, C.c_int32), ptr(mask, C.c_uint64), ptr(base, C.c_int32),
                                               ptr(first, C.c_int32), ptr(run0, C.c_int32), ptr(tab, C.c_uint8)))
                r = dict(block=b, dir=d, eligible=bool(ri.eligible), r0=ri.r0, nr=nr, rowptr=rowptr[:nr + 1],
                         col=col[:ne], val=val[:ne], step=step[:nr])
                if ri.eligible:
                    r.update(slots=ri.slots, ndr=ri.ndr, nrp=ri.nrp, trips=ri.trips, dset=(int(ri.dset[0]), int(ri.dset[1])),
                             dest=dest[:ne], lead=lead[:nr], mask=mask[:2 * nr].reshape(nr, 2), base=base[:nr],
                             first=first[:nr], run0=run0[:nr], tab=tab[:ri.ndr * ri.nrp].reshape(ri.ndr, ri.nrp))
                out.append(r)
    finally:
        lib.cpk_analysis_destroy(h)
    return out


def dist_plan(G, B, Cneg, A, Cop, nranks, rank, ctx=None, options=None):
    """Host-only row-block plan of `rank` for opLDL2(G, B, Cneg) and the
    Krylov operator blocks A, Cop: a dict of numpy arrays (see cpk_plan_array in cpk.h).  Engine
    options (split_tol) as in analyze(): pass the distributed context to get exactly the plan its
    preconditioner builds."""
    mats = [Matrix(M, host_only=True) for M in (G, B, Cneg, A, Cop)]
    h = C.c_void_p()
    check(lib.cpk_analyze(mats[0].h, mats[1].h, mats[2].h, _options_spec(ctx, options), C.byref(h)))
    p = C.c_void_p()
    try:
        check(lib.cpk_analysis_plan(h, mats[3].h, mats[4].h, int(nranks), int(rank), C.byref(p)))
    finally:
        lib.cpk_analysis_destroy(h)
    out = {}
    try:
        for nm in _PLAN_NAMES:
            cnt = C.c_int64()
            check(lib.cpk_plan_array(p, nm.encode(), C.byref(cnt), None))
            arr = np.empty(cnt.value, np.float64 if nm in _PLAN_F64 else np.int64)
            check(lib.cpk_plan_array(p, nm.encode(), C.byref(cnt), arr.ctypes.data_as(C.c_void_p)))
            out[nm] = arr
    finally:
        lib.cpk_plan_destroy(p)
    keys = ("P", "rank", "n", "m", "N", "n_loc", "m_loc", "N_loc", "nsub", "nT", "kt", "kp_kmax", "ac_kmax", "ab_kmax")
    out.update({k: int(v) for k, v in zip(keys, out["sizes"])})
    return out


# ---- solvers ----------------------------------------------------------------------------------
_STATUS = {0: "maximum number of iterations attained",
           1: "residual small compared to initial residual",
           2: "backward error small"}


def _hist_cap(method, opts, n, m):
    itmax = (opts or {}).get("itmax", n + m if method in ("gmres", "dqgmres") else n)
    itmax = int(min(max(itmax, 0), 1e8))
    if method == "gmres":
        r = int((opts or {}).get("restart", 50))
        itmax = -(-itmax // max(r, 1)) * max(r, 1)
    return itmax + 4


def _stats_from(method, st, hist, lq, qr):
    stats = {"niters": int(st.niters)}
    if method == "symmlq":
        stats["cgresidHistory"] = hist[:st.hist_len].copy()
        stats["lqresidHistory"] = lq[:st.lq_len].copy()
        stats["qrresidHistory"] = qr[:st.qr_len].copy()
    else:
        stats["residHistory"] = hist[:st.hist_len].copy()
    if method == "cglanczos":
        stats["status"] = _STATUS[st.status]
    stats["loop_ms"] = st.loop_ms
    stats["bytes_moved"] = st.bytes_moved
    return stats, {"solved": bool(st.solved)}


def _new_stats(cap):
    hist, lq, qr = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    st = _lib.Stats()
    st.hist, st.hist_lq, st.hist_qr = _dptr(hist), _dptr(lq), _dptr(qr)
    st.hist_cap = cap
    return st, hist, lq, qr


BLOCK_METHODS = ("cg", "minres")  # the methods with a lockstep block solve (cpk_method_solve_multi)


def _is_block(b):
    """An n x k array with k != 1 is a block of right-hand sides; a vector or an n x 1 array keeps
    the single-column path and return shapes (the convention of opLDL2.__mul__ / apply_block)."""
    return b.ndim == 2 and b.shape[1] != 1


def _block_call(name, k, opts, n, m, call, raise_on_error):
    """One block entry: per-column stats buffers and statuses around `call(stats_array, status_array)`;
    returns (the C stats, stats list, flag list, the error to raise or None); a refusal or a failure
    of the whole call raises at once, a failing column gives an error carrying `columns` (the
    caller adds `partial`)."""
    if name not in BLOCK_METHODS:
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED,
                       f"cp{name} takes one right-hand side; the block solve covers cpcg and cpminres")
    cap = _hist_cap(name, opts, n, m)
    sts = (_lib.Stats * max(k, 1))()
    hists = [np.zeros(cap) for _ in range(k)]
    for j in range(k):
        sts[j].hist, sts[j].hist_cap = _dptr(hists[j]), cap
    status = (C.c_int * max(k, 1))()
    rc = call(sts, status)
    columns = [int(status[j]) for j in range(k)]
    if rc != _lib.CPK_OK and not any(columns):
        check(rc)  # refused, or failed as a whole: nothing was written
    stats, flags = [], []
    for j in range(k):
        st, fl = _stats_from(name, sts[j], hists[j], None, None)
        if columns[j]:
            fl["error"] = columns[j]
        stats.append(st)
        flags.append(fl)
    err = None
    if rc != _lib.CPK_OK:
        msg = lib.cpk_last_error().decode()
        err = (IndefiniteError if rc == _lib.CPK_ERR_INDEFINITE else CpkError)(rc, msg)
        err.columns = columns
        flags[columns.index(rc) if rc in columns else 0].setdefault("message", msg)
    return sts, stats, flags, (err if raise_on_error else None)


def _method_block(name, b, Am, Cmat, M, opts, raise_on_error):
    n, m = Am.shape[0], Cmat.shape[0]
    if b.shape[0] != n:
        raise CpkError(_lib.CPK_ERR_DIM, "b must have n rows")
    k = b.shape[1]
    Bf = np.asfortranarray(b)
    X, Y = np.zeros((n, k), order="F"), np.zeros((m, k), order="F")

    def call(sts, status):
        return lib.cpk_method_solve_multi(M.ctx.h, _lib.METHODS[name], k, _dptr(Bf), max(n, 1), Am.h, Cmat.h, M.h,
                                          C.byref(make_opts(opts)), _dptr(X), max(n, 1), _dptr(Y), max(m, 1), sts, status)

    _, stats, flags, err = _block_call(name, k, opts, n, m, call, raise_on_error)
    if err is not None:
        err.partial = (X, Y, stats, flags)
        raise err
    return X, Y, stats, flags


def _method(name):
    def run(b, A, Cm, M, opts=None, raise_on_error=True):
        if not isinstance(M, opLDL2):
            raise CpkError(_lib.CPK_ERR_ARGS, "M must be an opLDL2 operator")
        ctx = M.ctx
        is_op = isinstance(A, Operator)
        Am, Cmat = (A if is_op else _as_matrix(A, ctx)), _as_matrix(Cm, ctx)
        n, m = Am.shape[0], Cmat.shape[0]
        b = np.asarray(b, dtype=np.float64)
        if _is_block(b):
            if is_op:
                raise CpkError(_lib.CPK_ERR_UNSUPPORTED, "an Operator takes one right-hand side; the block solve is matrix-only")
            return _method_block(name, b, Am, Cmat, M, opts, raise_on_error)
        b = np.ascontiguousarray(b).ravel()
        if b.shape[0] != n:
            raise CpkError(_lib.CPK_ERR_DIM, "b must have n entries")
        x, y = np.zeros(n), np.zeros(m)
        st, hist, lq, qr = _new_stats(_hist_cap(name, opts, n, m))
        if is_op:
            Am._solve(lambda: lib.cpk_method_solve_op(ctx.h, _lib.METHODS[name], _dptr(b), Am.h, Cmat.h, M.h,
                                                      C.byref(make_opts(opts)), _dptr(x), _dptr(y), C.byref(st)))
        else:
            check(lib.cpk_method_solve(ctx.h, _lib.METHODS[name], _dptr(b), Am.h, Cmat.h, M.h,
                                       C.byref(make_opts(opts)), _dptr(x), _dptr(y), C.byref(st)))
        stats, flag = _stats_from(name, st, hist, lq, qr)
        return x, y, stats, flag

    run.__name__ = "cp" + name
    run._cpk_method = name
    run.__doc__ = (f"[x, y, stats, flag] = cp{name}(b, A, C, M, opts)  (kernels/cp{name}.m).\n\n"
                   "An n x k array b with k != 1 is a block of right-hand sides (cpcg and cpminres; the other "
                   "methods raise CPK_ERR_UNSUPPORTED): the k columns are solved in lockstep on the GPU "
                   "(cpk_method_solve_multi), each column exactly as if solved alone, and the call returns "
                   "X (n x k), Y (m x k) and stats, flag as lists of k dicts.  opts['print'] is ignored for a "
                   "block.  A column that hits the reference's indefinite stop raises CpkError carrying "
                   "`columns` (the per-column status codes) and `partial` (X, Y, stats, flag); with "
                   "raise_on_error=False the results are returned with flag[j]['error'] set instead.\n\n"
                   "A may be an `Operator` (one right-hand side): the product A*v is then the operator's "
                   "callback, everything else is unchanged.")
    return run


cpcg = _method("cg")
cpcglanczos = _method("cglanczos")
cpminres = _method("minres")
cpsymmlq = _method("symmlq")
cpgmres = _method("gmres")
cpdqgmres = _method("dqgmres")


_PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")


def _reg_block(name, b, mats, opts, ctx, raise_on_error):
    """reg_cpkrylov for an N x k block: M = opLDL2(G, B, -C) built once with the preconditioner
    fields of opts (reg_cpkrylov.m:128-148), then the shift, the method and the recovery per
    column (reg_cpkrylov.m:152-175, cpk_reg_solve_multi)."""
    Am, Bm, Cmat, Gm = mats
    n, m = Am.shape[0], Bm.shape[0]
    if b.shape[0] != n + m:
        raise CpkError(_lib.CPK_ERR_DIM, "b must have n+m rows")
    if name not in BLOCK_METHODS:
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED,
                       f"cp{name} takes one right-hand side; the block solve covers cpcg and cpminres")
    if Cmat._val is None:
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED, "reg_cpkrylov on a block builds -C on the host: C was last "
                       "updated from device memory; pass its values with set_values from the host, or build "
                       "M = opLDL2(G, B, -C) and call the method")
    negC = sp.csr_matrix((-Cmat._val, Cmat._ind, Cmat._ptr.astype(np.int64)), shape=Cmat.shape)
    M = opLDL2(Gm, Bm, negC, ctx=ctx)
    props = {k: opts[k] for k in _PC_PROPS if opts and k in opts}
    if props:
        M._set(**props)
    k, N = b.shape[1], n + m
    Bf = np.asfortranarray(b)
    X = np.zeros((N, k), order="F")

    def call(sts, status):
        return lib.cpk_reg_solve_multi(ctx.h, _lib.METHODS[name], k, _dptr(Bf), max(N, 1), Am.h, Bm.h, Cmat.h, M.h,
                                       C.byref(make_opts(opts)), _dptr(X), max(N, 1), sts, status)

    sts, stats, flags, err = _block_call(name, k, opts, n, m, call, raise_on_error)
    for j in range(k):
        stats[j]["ptime"], stats[j]["stime"] = M.ptime, sts[j].stime
    if stats:
        stats[0]["M"] = M
    if err is not None:
        err.partial = (X, stats, flags)
        raise err
    return X, stats, flags


def _negated(Cmat, what):
    """-C on the host from a Matrix handle's canonical CSR arrays (M = opLDL2(G, B, -C))."""
    if Cmat._val is None:
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED, f"{what} builds -C on the host: C was last "
                       "updated from device memory; pass its values with set_values from the host, or build "
                       "M = opLDL2(G, B, -C) and call the method")
    if Cmat._csc:
        return sp.csc_matrix((-Cmat._val, Cmat._ind.astype(np.int64), Cmat._ptr.astype(np.int64)), shape=Cmat.shape)
    return sp.csr_matrix((-Cmat._val, Cmat._ind, Cmat._ptr.astype(np.int64)), shape=Cmat.shape)


def _reg_op(name, b, A, mats, opts, ctx):
    """reg_cpkrylov with an Operator A: M = opLDL2(G, B, -C) with the preconditioner fields of opts
    (reg_cpkrylov.m:128-148), then the shift (one call of A's fn when b(n+1:N) is not zero), the
    method and the recovery on the device (cpk_reg_solve_op)."""
    Bm, Cmat, Gm = mats
    n, m = A.n, Bm.shape[0]
    b = np.ascontiguousarray(b).ravel()
    if b.shape[0] != n + m:
        raise CpkError(_lib.CPK_ERR_DIM, "b must have n+m entries")
    M = opLDL2(Gm, Bm, _negated(Cmat, "reg_cpkrylov with an Operator"), ctx=ctx)
    props = {k: opts[k] for k in _PC_PROPS if opts and k in opts}
    if props:
        M._set(**props)
    x = np.zeros(n + m)
    st, hist, lq, qr = _new_stats(_hist_cap(name, opts, n, m))
    A._solve(lambda: lib.cpk_reg_solve_op(ctx.h, _lib.METHODS[name], _dptr(b), A.h, Bm.h, Cmat.h, M.h,
                                          C.byref(make_opts(opts)), _dptr(x), C.byref(st)))
    stats, flag = _stats_from(name, st, hist, lq, qr)
    stats["ptime"], stats["stime"], stats["M"] = M.ptime, st.stime, M
    return x, stats, flag


def reg_cpkrylov(method, b, A, B, Cm, G, opts=None, ctx=None, raise_on_error=True):
    """[x, stats, flag] = reg_cpkrylov(method, b, A, B, C, G, opts)   (reg_cpkrylov.m:1-180).

    A may be an `Operator` (one right-hand side, one GPU): M is built from G, B, C as always.

    An N x k array b with k != 1 is a block (cpcg and cpminres): M is built once and returned in
    stats[0]["M"], every column is shifted, solved and recovered as if alone, and x is N x k with
    stats, flag lists of k dicts (see cpminres for the error convention)."""
    if any(v is None for v in (method, b, A, B, Cm, G)):
        raise CpkError(_lib.CPK_ERR_ARGS, "reg_cpkrylov: not enough inputs")
    name = getattr(method, "_cpk_method", method)
    if name not in _lib.METHODS:
        raise CpkError(_lib.CPK_ERR_ARGS, f"unknown method {method!r}")
    if isinstance(A, Operator):
        ctx = ctx or A.ctx
        b = np.asarray(b, dtype=np.float64)
        if _is_block(b):
            raise CpkError(_lib.CPK_ERR_UNSUPPORTED, "an Operator takes one right-hand side; the block solve is matrix-only")
        return _reg_op(name, b, A, [_as_matrix(M, ctx) for M in (B, Cm, G)], opts, ctx)
    ctx = ctx or default_context()
    mats = [_as_matrix(M, ctx) for M in (A, B, Cm, G)]
    n, m = mats[0].shape[0], mats[1].shape[0]
    b = np.asarray(b, dtype=np.float64)
    if _is_block(b):
        return _reg_block(name, b, mats, opts, ctx, raise_on_error)
    b = np.ascontiguousarray(b).ravel()
    if b.shape[0] != n + m:
        raise CpkError(_lib.CPK_ERR_DIM, "b must have n+m entries")
    x = np.zeros(n + m)
    st, hist, lq, qr = _new_stats(_hist_cap(name, opts, n, m))
    Mh = C.c_void_p()
    check(lib.cpk_reg_solve(ctx.h, _lib.METHODS[name], _dptr(b), mats[0].h, mats[1].h, mats[2].h, mats[3].h,
                            C.byref(make_opts(opts)), _dptr(x), C.byref(st), C.byref(Mh)))
    stats, flag = _stats_from(name, st, hist, lq, qr)
    stats["ptime"], stats["stime"] = st.ptime, st.stime
    if Mh:
        stats["M"] = opLDL2(None, None, None, ctx=ctx, _handle=Mh)
    return x, stats, flag


def _is_device(v):
    """A device tensor, duck-typed as Matrix.set_values does (no tensor library is imported)."""
    return all(hasattr(v, a) for a in ("is_cuda", "data_ptr", "dtype", "is_contiguous")) and bool(v.is_cuda)


def _device_operand(v, what, rows):
    """(address, columns, leading dimension) of a contiguous float64 device tensor holding `rows`
    values, or k columns of `rows` values each, one column after the other (a (k, rows) row-major
    tensor is the N x k column-major block); its stream is synchronised first."""
    if "float64" not in str(v.dtype) or not v.is_contiguous():
        raise CpkError(_lib.CPK_ERR_ARGS, f"{what}: a contiguous float64 device tensor expected")
    count = int(v.numel())
    if rows == 0 or count % rows:
        if count != rows:
            raise CpkError(_lib.CPK_ERR_DIM, f"{what}: a multiple of N = {rows} values expected")
    mod = sys.modules[type(v).__module__.split(".")[0]]  # the tensor's own library, already loaded
    mod.cuda.current_stream(v.device).synchronize()
    return C.c_void_p(v.data_ptr() or None), (count // rows if rows else 1), max(rows, 1)


def _norms_dict(nr, vector):
    q = np.asarray(nr, dtype=np.float64).reshape(-1, 4)
    d = {"rr_x": q[:, 0].copy(), "rr_y": q[:, 1].copy(), "bb_x": q[:, 2].copy(), "bb_y": q[:, 3].copy()}
    d["rnorm"] = np.sqrt(d["rr_x"] + d["rr_y"])
    d["bnorm"] = np.sqrt(d["bb_x"] + d["bb_y"])
    return {k: float(v[0]) for k, v in d.items()} if vector else d


def _raise_partial(rc, partial):
    """The C status rc, unless it is CPK_OK, as its CpkError (`check`) carrying `partial`"""
    try:
        check(rc)
    except CpkError as e:
        e.partial = partial
        raise


def _verified_stats(stats, st, sums0, sums):
    """What K's solves add to a column's stats: the times, and the sums and norms of the start
    residual and of the returned x's (four sums each, as the C entries return them)"""
    stats["ptime"], stats["stime"] = st.ptime, st.stime
    stats["true_resid0"], stats["true_resid"] = _norms_dict(sums0, True), _norms_dict(sums, True)


class KKT:
    """The saddle-point operator K = [A B'; B -C] of the system reg_cpkrylov solves (A, B, C as
    the solvers take them: C is the positive block; A may be nonsymmetric), resident on the GPU.

    K follows its matrices: after `Matrix.set_values` (host or device values) the next use
    regathers K's values on the device.  A, B, C may be `Matrix` handles (shared with the solvers
    and the preconditioner) or scipy / dense matrices; K keeps them alive.

    Operands are NumPy arrays (a vector, or an N x k array for a block) or device tensors (anything
    with is_cuda, data_ptr(), dtype, is_contiguous(): float64, contiguous, one column of N values
    after the other, so a (k, N) row-major tensor is the N x k block).  With device operands the
    result goes to the device tensor passed as `out=` and nothing crosses PCIe but the sums."""

    def __init__(self, A, B, Cm, ctx=None):
        if any(isinstance(M, Operator) for M in (A, B, Cm)):
            raise CpkError(_lib.CPK_ERR_UNSUPPORTED, "K holds its blocks' entries: an Operator has none "
                           "(use the solvers with the Operator, and check residuals with its own product)")
        first = next((M for M in (A, B, Cm) if isinstance(M, Matrix)), None)
        self.ctx = ctx or (first.ctx if first is not None else None) or default_context()
        self.A, self.B, self.C = (_as_matrix(M, self.ctx) for M in (A, B, Cm))
        h = C.c_void_p()
        check(lib.cpk_kkt_create(self.ctx.h, self.A.h, self.B.h, self.C.h, C.byref(h)))
        self.h = h
        self.n, self.m = self.A.shape[0], self.C.shape[0]
        self.N = self.n + self.m
        self.shape = (self.N, self.N)

    def info(self):
        """Diagnostic (cpk_kkt_get_info): sizes, the values generations of A, B, C that K holds, the
        device regather passes so far and the device address of K's value array (it never moves)."""
        v = (C.c_int64 * 8)()
        check(lib.cpk_kkt_get_info(self.h, v))
        return {"n": v[0], "m": v[1], "nnz": v[2], "values_generations": (v[3], v[4], v[5]), "refreshes": v[6],
                "values_address": v[7]}

    def set_route(self, route):
        """Routing of the block residual: "auto" (panels of 8 columns from the measured crossover,
        a loop of single-column passes below it), "panel" or "loop" (forced; the same bits)."""
        check(lib.cpk_kkt_set_route(self.h, {"auto": 0, "panel": 1, "loop": 2}[route]))

    def route_info(self):
        v = (C.c_int64 * 4)()
        check(lib.cpk_kkt_route_info(self.h, v))
        return {"panel_columns": v[0], "crossover": v[1], "route": ("auto", "panel", "loop")[v[2]], "panels": v[3]}

    def _host_block(self, a, what):
        a = np.asarray(a, dtype=np.float64)
        vector = a.ndim == 1
        if a.ndim not in (1, 2) or a.shape[0] != self.N:
            raise CpkError(_lib.CPK_ERR_DIM, f"{what} must have N = {self.N} rows")
        return np.asfortranarray(a.reshape(self.N, -1)), vector

    def __matmul__(self, z):
        return self.apply(z)

    def apply(self, z, out=None):
        """y = K @ z: a vector or an N x k array; device tensors with out=.  A host block is a
        convenience: one staged cpk_kkt_apply per column (device tensors avoid the staging)."""
        if _is_device(z):
            if out is None or not _is_device(out):
                raise CpkError(_lib.CPK_ERR_ARGS, "K @ z on device operands: pass the result tensor as out=")
            zp, k, ld = _device_operand(z, "z", self.N)
            op, ko, _ = _device_operand(out, "out", self.N)
            if ko != k:
                raise CpkError(_lib.CPK_ERR_DIM, "out must have z's shape")
            for j in range(k):
                off = 8 * j * ld
                check(lib.cpk_kkt_apply_device(self.h, C.c_void_p((zp.value or 0) + off), C.c_void_p((op.value or 0) + off)))
            check(lib.cpk_ctx_synchronize(self.ctx.h))
            return out
        Z, vector = self._host_block(z, "z")
        Y = np.zeros_like(Z, order="F")
        for j in range(Z.shape[1]):
            zj, yj = np.ascontiguousarray(Z[:, j]), np.zeros(self.N)
            check(lib.cpk_kkt_apply(self.h, _dptr(zj), _dptr(yj)))
            Y[:, j] = yj
        return Y[:, 0].copy() if vector else Y

    def residual(self, z, b, out=None, want_r=True):
        """r = b - K @ z and the sums of squares of r and b, split at row n: returns (r, norms) with
        norms = {rr_x, rr_y, bb_x, bb_y, rnorm, bnorm} (floats for a vector, arrays of k for a
        block).  rr_* and bb_* are the device's sums (exact under engine option exact_dots), rnorm
        and bnorm their roots.  Device operands: r goes to out= (which may be b itself); with
        want_r=False no r is stored and None is returned for it."""
        return self._residual(lib.cpk_kkt_residual, lib.cpk_kkt_residual_device_sums, z, b, out, want_r)

    def residual_exact(self, z, b, out=None):
        """`residual` with the exactly rounded row sum (cpk_kkt_residual_exact): r_i is the exact sum
        of b_i and the TwoProd pairs of -K_ie * z_col(e) over row i's stored entries, rounded once to
        nearest even, so its own rounding error is half an ulp of r_i instead of eps * |K| |z|.  One
        definition whatever the entry order or the grid; a non-finite term gives a NaN in its row
        only.  Operands, blocks, out= and the returned (r, norms) are `residual`'s; the sums are
        those `residual` would form on that r and b.  A block is a loop of single-column passes."""
        return self._residual(lib.cpk_kkt_residual_exact, lib.cpk_kkt_residual_exact_device_sums, z, b, out, True)

    def _residual(self, host_entry, device_entry, z, b, out, want_r):
        if _is_device(z) or _is_device(b):
            if not (_is_device(z) and _is_device(b)):
                raise CpkError(_lib.CPK_ERR_ARGS, "residual: z and b must both be host arrays or both device tensors")
            zp, k, ld = _device_operand(z, "z", self.N)
            bp, kb, _ = _device_operand(b, "b", self.N)
            if kb != k:
                raise CpkError(_lib.CPK_ERR_DIM, "b must have z's shape")
            rp = C.c_void_p(None)
            if want_r:
                if out is None or not _is_device(out):
                    raise CpkError(_lib.CPK_ERR_ARGS, "residual on device operands: pass the result tensor as out=")
                rp, kr, _ = _device_operand(out, "out", self.N)
                if kr != k:
                    raise CpkError(_lib.CPK_ERR_DIM, "out must have z's shape")
            nr = np.zeros(4 * max(k, 1))  # host memory: the entry copies the sums back and waits
            check(device_entry(self.h, k, zp, ld, bp, ld, rp, ld, _dptr(nr)))
            return (out if want_r else None), _norms_dict(nr[:4 * k], getattr(z, "ndim", 2) == 1)
        Z, vector = self._host_block(z, "z")
        Bm, _ = self._host_block(b, "b")
        if Bm.shape != Z.shape:
            raise CpkError(_lib.CPK_ERR_DIM, "b must have z's shape")
        k, ld = Z.shape[1], max(self.N, 1)
        R = np.zeros_like(Z, order="F") if want_r else None
        nr = np.zeros(4 * max(k, 1))
        check(host_entry(self.h, k, _dptr(Z), ld, _dptr(Bm), ld, _dptr(R) if want_r else None, ld, _dptr(nr)))
        r = None if not want_r else (R[:, 0].copy() if vector else R)
        return r, _norms_dict(nr[:4 * k], vector)

    def solve(self, method, b, M, opts=None, x0=None, out=None):
        """x, stats, flag = K.solve(method, b, M, opts, x0): reg_cpkrylov's driver with the existing
        preconditioner M (an opLDL2 built on K's matrices), checked against K itself.

        x0 is None: the cold solve, cpk_reg_solve_device on K's handles unchanged.  With x0 the
        call forms r = b - K @ x0 on the device, runs the same driver on r and returns x0 + dx: THE
        STOP TEST THEN RUNS ON THE CORRECTION SYSTEM (atol, rtol relative to r's initial
        preconditioned residual, not b's).  stats["true_resid0"] and stats["true_resid"] hold the
        sums and norms (as `residual` returns them) of the start residual (cold: of b) and of
        b - K @ x for the returned x.  Device operands: b a device tensor and the result in out=; a
        warm start passes x0=out, which holds x0 on entry and is updated in place.  A stop inside
        the driver raises its own error, carrying `partial` = (x0 plus whatever the driver wrote,
        the eight sums)."""
        name = self._solving_method(method, M, (b, x0, out),
                                    "K.solve is matrix-only: K's (1,1) block is the matrix it was built on")
        (bp, xp), x, _ = self._one_rhs("solve", (b,), x0, out, ("b", "x0", "out"))
        st, hist, lq, qr = _new_stats(_hist_cap(name, opts, self.n, self.m))
        res = np.zeros(8)
        entry = lib.cpk_kkt_solve_device if _is_device(x) else lib.cpk_kkt_solve
        rc = entry(self.h, _lib.METHODS[name], bp, M.h, C.byref(make_opts(opts)), xp, int(x0 is not None), C.byref(st),
                   _dptr(res))
        _raise_partial(rc, (x, res))  # x0 plus whatever the driver wrote, and the sums
        stats, flag = _stats_from(name, st, hist, lq, qr)
        _verified_stats(stats, st, res[:4], res[4:])
        return x, stats, flag

    def solve_refined(self, method, b, M, opts=None, x0=None, max_steps=3, out=None):
        """x, stats, flag = K.solve_refined(method, b, M, opts, x0, max_steps): `solve` followed by up
        to max_steps corrections of iterative refinement on the exactly rounded residual
        (cpk_kkt_solve_refined).  Driver call j = 0 .. max_steps runs `solve`'s driver from zero on
        r_j = residual_exact(x_j, b) (cold, j = 0: on b) and gives the trial x_j + dx_j: EACH
        CALL'S STOP TEST RUNS ON ITS CORRECTION SYSTEM.  A trial whose residual's sum of squares is
        not below r_j's is dropped and ends the loop with x_j; the last call's trial is taken
        unchecked, so max_steps=0 with x0=None is the cold `solve`.  stats are the last driver
        call's, with stats["refine_steps"] (the corrections in x: driver calls after the first whose
        trial was taken; -1 when the first call's own trial was dropped and x is x0 or zero),
        stats["resid_sums"] (one row [rr_x, rr_y, bb_x, bb_y] per residual formed: refine_steps + 1
        rows, the residuals the taken driver calls ran on; where a trial was dropped two more, of the
        returned x and of the dropped trial) and stats["true_resid"] as
        `solve` sets it (the plain residual of the returned x).  Operands and out= are `solve`'s; a
        stop inside the driver raises its error with `partial` = (x_j plus whatever the driver wrote,
        resid_sums)."""
        name = self._solving_method(method, M, (b, x0, out),
                                    "K.solve_refined is matrix-only: K's (1,1) block is the matrix it was built on")
        max_steps = int(max_steps)
        if max_steps < 0:
            raise CpkError(_lib.CPK_ERR_ARGS, "max_steps >= 0 required")
        (bp, xp), x, (b,) = self._one_rhs("solve_refined", (b,), x0, out, ("b", "x0", "out"))
        st, hist, lq, qr = _new_stats(_hist_cap(name, opts, self.n, self.m))
        res, steps = np.zeros(4 * (max_steps + 1)), C.c_int(0)
        entry = lib.cpk_kkt_solve_refined_device if _is_device(x) else lib.cpk_kkt_solve_refined
        rc = entry(self.h, _lib.METHODS[name], bp, M.h, C.byref(make_opts(opts)), xp, int(x0 is not None), max_steps,
                   C.byref(st), _dptr(res), C.byref(steps))
        # the residuals formed: one per taken driver call, and where a trial was dropped (the loop ended
        # early without an error) those of the returned x and of that trial
        dropped = rc == _lib.CPK_OK and steps.value < max_steps
        rows = res.reshape(max_steps + 1, 4)[:steps.value + (3 if dropped else 1)].copy()
        _raise_partial(rc, (x, rows))
        stats, flag = _stats_from(name, st, hist, lq, qr)
        stats["refine_steps"], stats["resid_sums"] = steps.value, rows
        # true_resid0 is K.solve's key: with max_steps=0 the stats are K.solve's
        _verified_stats(stats, st, rows[0], rows[0])
        stats["true_resid"] = self.residual(x, b, out=None, want_r=False)[1]  # the plain residual of the returned x
        return x, stats, flag

    def adjoint(self, method, x, gx, M, opts=None, KT=None, lam0=None, out=None):
        """The adjoint of `solve` (cpk_kkt_adjoint): with x = K \\ b and gx = dL/dx, returns
        dict(db, dA, dB, dC, stats, flag) where db = lambda = K' \\ gx = dL/db and dA, dB, dC are
        dL/d(values) of K's A, B and C on their own sparsity, each in the order its handle's
        `set_values` takes values in: -lambda_x x_x', -(lambda_y x_x' + x_y lambda_x') and
        +lambda_y x_y' sampled there (Matrix.sample_outer).  lambda is solved by
        `(KT or self).solve(method, gx, M, opts, x0=lam0)`: stats and flag are that solve's, and
        with lam0 (usually the previous outer iteration's lambda) its stop test runs on the
        correction system.  KT is the KKT of the transposed system, KKT(A.T, B, C); without it the
        caller asserts that A is symmetric, which is not checked.  One right-hand side.

        Operands as for `solve`.  Host arrays: `out` may be a dict holding NumPy arrays for any
        of "db", "dA", "dB", "dC" to be filled in place.  Device tensors (x and gx): out= is a dict
        of device tensors, "db" required (lam0, if given, is out["db"] itself, updated in place)
        and "dA", "dB", "dC" each optional -- a gradient that is absent is not formed.  A stop
        inside the driver raises its own error, carrying `partial` = (lambda as far as the driver
        wrote it, the eight sums); the gradient arrays are then untouched."""
        name = self._solving_method(method, M, (x, gx, KT, lam0),
                                    "K.adjoint is matrix-only: an Operator has no entries to take a gradient on")
        if KT is not None and not isinstance(KT, KKT):
            raise CpkError(_lib.CPK_ERR_ARGS, "KT must be a KKT operator (of A.T, B, C)")
        out = dict(out or {})
        if set(out) - {"db", "dA", "dB", "dC"}:
            raise CpkError(_lib.CPK_ERR_ARGS, "adjoint: out= holds db, dA, dB, dC")
        (xp, gxp, lp), lam, _ = self._one_rhs("adjoint", (x, gx), lam0, out.get("db"), ("x", "gx", "lam0", "out['db']"),
                                              fill_host_out=True)
        device = _is_device(lam)
        gp = self._grad_args(out, device)
        st, hist, lq, qr = _new_stats(_hist_cap(name, opts, self.n, self.m))
        res = np.zeros(8)
        entry = lib.cpk_kkt_adjoint_device if device else lib.cpk_kkt_adjoint
        rc = entry(self.h, KT.h if KT is not None else None, _lib.METHODS[name], xp, gxp, M.h, C.byref(make_opts(opts)), lp,
                   int(lam0 is not None), *gp, C.byref(st), _dptr(res))
        _raise_partial(rc, (lam, res))
        stats, flag = _stats_from(name, st, hist, lq, qr)
        _verified_stats(stats, st, res[:4], res[4:])
        return dict(db=lam, dA=out.get("dA"), dB=out.get("dB"), dC=out.get("dC"), stats=stats, flag=flag)

    # ---- the block forms: N x k blocks (a (k, N) row-major device tensor is the N x k block) ----------
    def _host_cols(self, a, what):
        """An N x k Fortran-ordered float64 copy of a host block (a vector is one column)"""
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2 or a.shape[0] != self.N:
            raise CpkError(_lib.CPK_ERR_DIM, f"{what} must have N = {self.N} rows")
        return np.array(a, dtype=np.float64, order="F")

    def _device_cols(self, vs, whats):
        """The addresses of device blocks of one shape, their column count and leading dimension"""
        ptrs, k = [], None
        for v, what in zip(vs, whats):
            if not _is_device(v):
                raise CpkError(_lib.CPK_ERR_ARGS, f"{what}: the operands are all host arrays or all device tensors")
        for v, what in zip(vs, whats):
            p, kv, ld = _device_operand(v, what, self.N)
            if k is not None and kv != k:
                raise CpkError(_lib.CPK_ERR_DIM, f"{what} must have the other operands' shape")
            k = kv
            ptrs.append(p)
        return ptrs, k, max(self.N, 1)

    _BLOCK_MATRIX_ONLY = "K's block entries are matrix-only: K's (1,1) block is the matrix it was built on"

    def _solving_method(self, method, M, operands, matrix_only):
        """The method's name after the checks the five solving methods share, in their order: a known
        method, no Operator among M and the operands (matrix_only: the caller's refusal), M an opLDL2"""
        name = getattr(method, "_cpk_method", method)
        if name not in _lib.METHODS:
            raise CpkError(_lib.CPK_ERR_ARGS, f"unknown method {method!r}")
        if any(isinstance(v, Operator) for v in (M,) + tuple(operands)):
            raise CpkError(_lib.CPK_ERR_UNSUPPORTED, matrix_only)
        if not isinstance(M, opLDL2):
            raise CpkError(_lib.CPK_ERR_ARGS, "M must be an opLDL2 operator")
        return name

    def _one_rhs(self, who, inputs, x0, out, names, fill_host_out=False):
        """One right-hand side for the single-column C entries.  inputs: the vectors the entry reads
        (the right-hand side last); x0: the start, or None; names: the inputs', x0's and out's.
        Device form (an input is a device tensor): the inputs and out are device tensors of one column
        of N values, and x0 is out itself.  Host form: the inputs ravelled, N entries each; the result
        is a new array -- or out, filled in place, where fill_host_out -- with x0 copied into it.
        Returns ([the inputs' pointers..., the result's], the result, the inputs as marshalled)."""
        *in_names, x0_name, out_name = names
        if any(_is_device(v) for v in inputs):
            if not (all(_is_device(v) for v in inputs) and _is_device(out)):
                raise CpkError(_lib.CPK_ERR_ARGS,
                               f"{who} on device operands: {', '.join(in_names)} and {out_name} are device tensors")
            if x0 is not None and x0 is not out:
                raise CpkError(_lib.CPK_ERR_ARGS, f"{who} on device operands: {x0_name} is {out_name} itself (updated in place)")
            ptrs = []
            for v, what in zip(tuple(inputs) + (out,), in_names + [out_name]):
                p, k, _ = _device_operand(v, what, self.N)
                if k != 1:
                    raise CpkError(_lib.CPK_ERR_DIM, f"{who} takes one right-hand side of N entries")
                ptrs.append(p)
            return ptrs, out, tuple(inputs)
        vals = tuple(np.ascontiguousarray(np.asarray(v, dtype=np.float64)).ravel() for v in inputs)
        for v, what in zip(vals, in_names):
            if v.shape[0] != self.N:
                raise CpkError(_lib.CPK_ERR_DIM, f"{what} must have n+m entries")
        x = out if fill_host_out and out is not None else np.zeros(self.N)
        if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
            raise CpkError(_lib.CPK_ERR_ARGS, f"{who}: {out_name} is a contiguous float64 array")
        if x.size != self.N:
            raise CpkError(_lib.CPK_ERR_DIM, f"{out_name} must have n+m entries")
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64).ravel()
            if x0.shape[0] != self.N:
                raise CpkError(_lib.CPK_ERR_DIM, f"{x0_name} must have n+m entries")
            x[:] = x0
        return [_dptr(v) for v in vals] + [_dptr(x)], x, vals

    def _block_stats(self, sts, stats, res, k):
        for j in range(k):
            _verified_stats(stats[j], sts[j], res[8 * j:8 * j + 4], res[8 * j + 4:8 * j + 8])

    def solve_block(self, method, B, M, opts=None, X0=None, out=None):
        """X, stats, flags = K.solve_block(method, B, M, opts, X0): `solve` for the k columns of an
        N x k block in lockstep (cpk_kkt_solve_multi; cpcg and cpminres, the other methods raise
        CPK_ERR_UNSUPPORTED).  Column j is K.solve(method, B[:, j], M, opts, x0=X0[:, j]): with X0
        (one start for the whole block) every column's stop test runs on its correction system.
        stats and flags are lists of k dicts, each stats with `true_resid0` and `true_resid`.
        Device operands as `residual` takes blocks: B a (k, N) device tensor, the result in out=,
        and a warm start passes X0=out.  A column whose driver stops raises its error carrying
        `columns` (the per-column status codes) and `partial` = (X, stats, flags)."""
        name = self._solving_method(method, M, (B, X0, out), self._BLOCK_MATRIX_ONLY)
        if _is_device(B):
            if out is None or not _is_device(out):
                raise CpkError(_lib.CPK_ERR_ARGS, "solve_block on device operands: pass the result tensor as out=")
            if X0 is not None and X0 is not out:
                raise CpkError(_lib.CPK_ERR_ARGS, "solve_block on device operands: X0 is out itself (updated in place)")
            (bp, xp), k, ld = self._device_cols((B, out), ("B", "out"))
            X, entry, args = out, lib.cpk_kkt_solve_multi_device, (bp, xp)
        else:
            if _is_device(X0) or _is_device(out):
                raise CpkError(_lib.CPK_ERR_ARGS, "solve_block: B, X0 and out are all host arrays or all device tensors")
            Bf = self._host_cols(B, "B")
            k, ld = Bf.shape[1], max(self.N, 1)
            X = np.zeros((self.N, k), order="F") if out is None else out
            if not (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.shape == (self.N, k) and
                    (X.flags.f_contiguous or k == 0)):
                raise CpkError(_lib.CPK_ERR_ARGS, "solve_block: out is a Fortran-ordered float64 N x k array")
            if X0 is not None:
                X0f = self._host_cols(X0, "X0")
                if X0f.shape != Bf.shape:
                    raise CpkError(_lib.CPK_ERR_DIM, "X0 must have B's shape")
                X[...] = X0f
            entry, args = lib.cpk_kkt_solve_multi, (_dptr(Bf), _dptr(X))
        res = np.zeros(8 * max(k, 1))

        def call(sts, status):
            return entry(self.h, _lib.METHODS[name], k, args[0], ld, M.h, C.byref(make_opts(opts)), args[1], ld,
                         int(X0 is not None), sts, status, _dptr(res))

        sts, stats, flags, err = _block_call(name, k, opts, self.n, self.m, call, True)
        self._block_stats(sts, stats, res, k)
        if err is not None:
            err.partial = (X, stats, flags)
            raise err
        return X, stats, flags

    def _grad_args(self, out, device):
        """The six gradient arguments of the C entries from out= (host: all three, created where
        absent; device: those present)"""
        counts = [h.info()["entries"] for h in (self.A, self.B, self.C)]
        gp = []
        for key, cnt in zip(("dA", "dB", "dC"), counts):
            g = out.get(key)
            if device:
                if g is None:
                    gp += [C.c_void_p(None), 0]
                    continue
                if not _is_device(g):
                    raise CpkError(_lib.CPK_ERR_ARGS, f"out[{key!r}] is a device tensor, as the operands are")
                gp += [_device_operand(g, key, cnt)[0], int(g.numel())]
            else:
                if g is None:
                    g = out[key] = np.zeros(cnt)
                if not (isinstance(g, np.ndarray) and g.dtype == np.float64 and g.flags.c_contiguous):
                    raise CpkError(_lib.CPK_ERR_ARGS, f"out[{key!r}] is a contiguous float64 array")
                gp += [_dptr(g) if g.size else None, g.size]
        return gp

    def set_sample_route(self, route):
        """Routing of `sample_block`'s kernel: "auto" (by the measured rule: the panel kernel where the
        last panel of 8 columns is full), "panel" (the panel
        kernel on interleaved copies of X and Lam, k >= 2) or "outer" (the run-time-k kernel of
        `Matrix.sample_outer` on the blocks themselves); the same bits on either."""
        check(lib.cpk_kkt_set_sample_route(self.h, {"auto": 0, "panel": 1, "outer": 2}[route]))

    def sample_route_info(self):
        v = (C.c_int64 * 4)()
        check(lib.cpk_kkt_sample_route_info(self.h, v))
        return {"panel_columns": v[0], "max_pad": v[1], "route": ("auto", "panel", "outer")[v[2]], "panel_calls": v[3]}

    def sample_block(self, X, Lam, out=None):
        """dict(dA, dB, dC) = K.sample_block(X, Lam): the three gradient passes alone
        (cpk_kkt_sample_multi), the sums over the k columns of -lam_x x_x', -(lam_y x_x' + x_y lam_x')
        and +lam_y x_y' sampled on the sparsity of K's A, B and C, each in the order its handle's
        `set_values` takes.  Per entry the products are added in column order from 0.0, each rounded
        on its own.  Host blocks: out= may hold NumPy arrays to fill.  Device tensors: out= is a
        dict of device tensors; a gradient that is absent is not formed."""
        out = dict(out or {})
        if set(out) - {"dA", "dB", "dC"}:
            raise CpkError(_lib.CPK_ERR_ARGS, "sample_block: out= holds dA, dB, dC")
        if _is_device(X) or _is_device(Lam):
            (xp, lp), k, ld = self._device_cols((X, Lam), ("X", "Lam"))
            check(lib.cpk_kkt_sample_multi_device(self.h, k, xp, ld, lp, ld, *self._grad_args(out, True)))
        else:
            Xf, Lf = self._host_cols(X, "X"), self._host_cols(Lam, "Lam")
            if Xf.shape != Lf.shape:
                raise CpkError(_lib.CPK_ERR_DIM, "Lam must have X's shape")
            gp = self._grad_args(out, False)
            check(lib.cpk_kkt_sample_multi(self.h, Xf.shape[1], _dptr(Xf), max(self.N, 1), _dptr(Lf), max(self.N, 1), *gp))
        return dict(dA=out.get("dA"), dB=out.get("dB"), dC=out.get("dC"))

    def adjoint_block(self, method, X, GX, M, opts=None, Lam0=None, out=None):
        """The adjoint of `solve_block` (cpk_kkt_adjoint_multi): with X = K \\ B and GX = dL/dX
        returns dict(db, dA, dB, dC, stats, flags), db = Lam = K \\ GX by
        `solve_block(method, GX, M, opts, X0=Lam0)` (stats and flags are that call's lists) and dA,
        dB, dC = `sample_block(X, Lam)`: the gradients of the batch, summed over its columns.  There
        is no KT: the caller asserts that A is symmetric.  Host and device operands as `adjoint`
        takes them: on device, out["db"] is required and Lam0 is out["db"] itself.  A column whose
        driver stops raises its error (`columns`, `partial` = (Lam, stats, flags)); the gradient
        arrays are then untouched."""
        name = self._solving_method(method, M, (X, GX, Lam0), self._BLOCK_MATRIX_ONLY)
        out = dict(out or {})
        if set(out) - {"db", "dA", "dB", "dC"}:
            raise CpkError(_lib.CPK_ERR_ARGS, "adjoint_block: out= holds db, dA, dB, dC")
        device = _is_device(X) or _is_device(GX)
        if device:
            if not _is_device(out.get("db")):
                raise CpkError(_lib.CPK_ERR_ARGS, "adjoint_block on device operands: X, GX and out['db'] are device tensors")
            if Lam0 is not None and Lam0 is not out["db"]:
                raise CpkError(_lib.CPK_ERR_ARGS, "adjoint_block on device operands: Lam0 is out['db'] itself (updated in place)")
            (xp, gxp, lp), k, ld = self._device_cols((X, GX, out["db"]), ("X", "GX", "out['db']"))
            entry = lib.cpk_kkt_adjoint_multi_device
        else:
            if _is_device(Lam0) or any(_is_device(v) for v in out.values()):
                raise CpkError(_lib.CPK_ERR_ARGS, "adjoint_block: the operands are all host arrays or all device tensors")
            Xf, Gf = self._host_cols(X, "X"), self._host_cols(GX, "GX")
            if Xf.shape != Gf.shape:
                raise CpkError(_lib.CPK_ERR_DIM, "GX must have X's shape")
            k, ld = Xf.shape[1], max(self.N, 1)
            lam = out.setdefault("db", np.zeros((self.N, k), order="F"))
            if not (isinstance(lam, np.ndarray) and lam.dtype == np.float64 and lam.shape == (self.N, k) and
                    (lam.flags.f_contiguous or k == 0)):
                raise CpkError(_lib.CPK_ERR_ARGS, "adjoint_block: out['db'] is a Fortran-ordered float64 N x k array")
            if Lam0 is not None:
                L0 = self._host_cols(Lam0, "Lam0")
                if L0.shape != Xf.shape:
                    raise CpkError(_lib.CPK_ERR_DIM, "Lam0 must have X's shape")
                lam[...] = L0
            xp, gxp, lp = _dptr(Xf), _dptr(Gf), _dptr(lam)
            entry = lib.cpk_kkt_adjoint_multi
        gp = self._grad_args(out, device)
        res = np.zeros(8 * max(k, 1))

        def call(sts, status):
            return entry(self.h, _lib.METHODS[name], k, xp, ld, gxp, ld, M.h, C.byref(make_opts(opts)), lp, ld,
                         int(Lam0 is not None), *gp, sts, status, _dptr(res))

        sts, stats, flags, err = _block_call(name, k, opts, self.n, self.m, call, True)
        self._block_stats(sts, stats, res, k)
        if err is not None:
            err.partial = (out["db"], stats, flags)
            raise err
        return dict(db=out["db"], dA=out.get("dA"), dB=out.get("dB"), dC=out.get("dC"), stats=stats, flags=flags)

    def __del__(self):
        if getattr(self, "h", None):
            lib.cpk_kkt_destroy(self.h)
            self.h = None


def SymGivens(a, b):
    """[c, s, d] = SymGivens(a, b)  (util/SymGivens.m)."""
    c, s, d = C.c_double(), C.c_double(), C.c_double()
    check(lib.cpk_symgivens(float(a), float(b), C.byref(c), C.byref(s), C.byref(d)))
    return c.value, s.value, d.value
