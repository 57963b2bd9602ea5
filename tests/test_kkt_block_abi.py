"""The block forms of K.solve and its adjoint (cpk_kkt_solve_multi, cpk_kkt_sample_multi,
cpk_kkt_adjoint_multi) without a device: the entries are declared and exported with the header's
signatures, the ABI version is unchanged, a NULL handle is refused with the outputs untouched, and
the Python front end checks shapes, dtypes and host/device mixing before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpk_kkt_solve_multi", "cpk_kkt_solve_multi_device", "cpk_kkt_sample_multi", "cpk_kkt_sample_multi_device",
       "cpk_kkt_adjoint_multi", "cpk_kkt_adjoint_multi_device", "cpk_kkt_set_sample_route", "cpk_kkt_sample_route_info")
PD = C.POINTER(C.c_double)
HEADER = open(os.path.join(ROOT, "include", "cpk.h")).read()


def _ctype(param):
    """the ctypes type _SIGS must hold for one parameter of a declaration in cpk.h"""
    param = " ".join(param.split())
    name = re.search(r"(\w+)(\[\d*\])?$", param).group(1)
    if re.match(r"(const )?cpk_(pc|kkt)\b", param):
        return C.c_void_p
    if "cpk_opts" in param:
        return C.POINTER(_lib.Opts)
    if "cpk_stats" in param:
        return C.POINTER(_lib.Stats)
    if "double" in param:
        assert "*" in param, param
        return C.c_void_p if name.startswith("d_") else PD  # device pointers travel as void *
    if "int64_t" in param:
        return C.POINTER(C.c_int64) if param.endswith("]") else C.c_int64
    if re.match(r"int \*\w+$", param):
        return C.POINTER(C.c_int)
    if re.match(r"int \w+$", param):
        return C.c_int
    raise AssertionError(f"unmapped parameter {param!r}")


def test_declared_exported_and_bound_with_the_headers_signatures():
    for n in NEW:
        m = re.search(r"^int\s+" + n + r"\s*\(([^)]*)\)\s*;", HEADER, re.M)
        assert m, f"{n} is not declared in cpk.h"
        want = [_ctype(p) for p in m.group(1).split(",")]
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTED, n
        args, res = _lib._SIGS[n]
        assert res is C.c_int and args == want, (n, args, want)


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3
    assert "#define CPK_ABI_VERSION 3" in HEADER


def test_header_states_the_contract():
    text = " ".join(HEADER.split())
    for phrase in ("column j is cpk_kkt_solve on B(:, j)", "CORRECTION SYSTEM", "in column order c = 0 ... k-1",
                   "ly_c[i] * xx_c[j], then xy_c[i] * lx_c[j]", "There is no KT", "before any gradient pass is enqueued"):
        assert phrase in text, phrase


def test_python_front_end_exists():
    for name in ("solve_block", "sample_block", "adjoint_block", "set_sample_route", "sample_route_info"):
        assert hasattr(cpk.KKT, name), name
    assert hasattr(cpk.autograd, "kkt_solve_batch")


def test_null_handles_are_refused_with_the_outputs_untouched():
    lib = _lib.lib
    sent = np.full(16, -7.5)
    out = sent.copy()
    pd = out.ctypes.data_as(PD)
    status = (C.c_int * 2)(-9, -9)
    A = _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_solve_multi(None, 2, 1, pd, 8, None, None, pd, 8, 0, None, status, pd) == A
    assert b"NULL" in lib.cpk_last_error()
    assert lib.cpk_kkt_solve_multi_device(None, 2, 1, None, 8, None, None, None, 8, 1, None, status, pd) == A
    assert lib.cpk_kkt_sample_multi(None, 1, pd, 8, pd, 8, pd, 1, pd, 1, pd, 1) == A
    assert lib.cpk_kkt_sample_multi_device(None, 1, None, 8, None, 8, None, 0, None, 0, None, 0) == A
    assert lib.cpk_kkt_adjoint_multi(None, 2, 1, pd, 8, pd, 8, None, None, pd, 8, 0, pd, 1, pd, 1, pd, 1, None, status,
                                     pd) == A
    assert lib.cpk_kkt_adjoint_multi_device(None, 2, 1, None, 8, None, 8, None, None, None, 8, 0, None, 0, None, 0, None,
                                            0, None, status, pd) == A
    info = (C.c_int64 * 4)(*([-7] * 4))
    assert lib.cpk_kkt_set_sample_route(None, 1) == A
    assert lib.cpk_kkt_sample_route_info(None, info) == A and list(info) == [-7] * 4
    assert np.array_equal(out, sent) and list(status) == [-9, -9]


class _FakeKKT(cpk.KKT):
    """The Python checks alone: a K of N = 5 that has no handle, so a check that let a call through
    would fail on the NULL handle (CPK_ERR_ARGS from the library, with "NULL" in its message)"""

    def __init__(self):  # noqa: D107
        self.h, self.n, self.m, self.N = None, 3, 2, 5


class _FakeM(cpk.opLDL2):
    def __init__(self):  # noqa: D107
        self.h = None

    def __del__(self):
        pass


class _FakeTensor:
    """What the front end takes for a device tensor; data_ptr() is never reached by a refused call"""
    is_cuda, dtype = True, "torch.float64"

    def __init__(self, count, dtype="torch.float64", contiguous=True):
        self.count, self.dtype, self.contiguous = count, dtype, contiguous

    def is_contiguous(self):
        return self.contiguous

    def numel(self):
        return self.count

    def data_ptr(self):
        raise AssertionError("a refused call must not reach the device operand's address")


def _raises(code, fn, *a, **kw):
    with pytest.raises(cpk.CpkError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert "NULL" not in str(e.value)


def test_python_argument_checks_raise_before_a_device_is_touched():
    K, M = _FakeKKT(), _FakeM()
    B = np.zeros((5, 3))
    D, A, U = _lib.CPK_ERR_DIM, _lib.CPK_ERR_ARGS, _lib.CPK_ERR_UNSUPPORTED
    # solve_block
    _raises(A, K.solve_block, "nosuch", B, M)
    _raises(A, K.solve_block, "minres", B, object())
    _raises(D, K.solve_block, "minres", np.zeros((4, 3)), M)
    _raises(D, K.solve_block, "minres", B, M, X0=np.zeros((5, 2)))
    _raises(A, K.solve_block, "minres", B, M, out=np.zeros((5, 3), dtype=np.float32, order="F"))
    _raises(A, K.solve_block, "minres", B, M, out=np.zeros((5, 3)))  # row-major
    _raises(A, K.solve_block, "minres", B, M, out=_FakeTensor(15))  # host B, device out
    _raises(A, K.solve_block, "minres", _FakeTensor(15), M)  # device B without out=
    _raises(A, K.solve_block, "minres", _FakeTensor(15), M, out=np.zeros((5, 3), order="F"))
    _raises(A, K.solve_block, "minres", _FakeTensor(15), M, X0=_FakeTensor(15), out=_FakeTensor(15))  # X0 is not out
    _raises(A, K.solve_block, "minres", _FakeTensor(15, dtype="torch.float32"), M, out=_FakeTensor(15))
    _raises(A, K.solve_block, "minres", _FakeTensor(15, contiguous=False), M, out=_FakeTensor(15))
    _raises(D, K.solve_block, "minres", _FakeTensor(14), M, out=_FakeTensor(14))
    _raises(U, K.solve_block, "gmres", B, M)
    # sample_block
    _raises(D, K.sample_block, np.zeros((5, 3)), np.zeros((5, 2)))
    _raises(D, K.sample_block, np.zeros((4, 3)), np.zeros((4, 3)))
    _raises(A, K.sample_block, np.zeros((5, 3)), np.zeros((5, 3)), out={"db": np.zeros(5)})
    _raises(A, K.sample_block, _FakeTensor(15), np.zeros((5, 3)))
    _raises(A, K.sample_block, np.zeros((5, 3)), _FakeTensor(15))
    _raises(A, K.sample_block, _FakeTensor(15, dtype="torch.float32"), _FakeTensor(15))
    # adjoint_block
    _raises(A, K.adjoint_block, "nosuch", B, B, M)
    _raises(D, K.adjoint_block, "minres", B, np.zeros((5, 2)), M)
    _raises(D, K.adjoint_block, "minres", B, B, M, Lam0=np.zeros((5, 4)))
    _raises(A, K.adjoint_block, "minres", B, B, M, out={"dx": np.zeros(5)})
    _raises(A, K.adjoint_block, "minres", B, B, M, out={"db": np.zeros((5, 3))})  # row-major
    _raises(A, K.adjoint_block, "minres", B, B, M, out={"db": _FakeTensor(15)})
    _raises(A, K.adjoint_block, "minres", _FakeTensor(15), _FakeTensor(15), M)  # no out["db"]
    _raises(A, K.adjoint_block, "minres", _FakeTensor(15), B, M, out={"db": _FakeTensor(15)})
    _raises(A, K.adjoint_block, "minres", _FakeTensor(15), _FakeTensor(15), M, Lam0=_FakeTensor(15),
            out={"db": _FakeTensor(15)})


def test_kkt_solve_batch_checks_its_arguments_before_a_device_is_touched():
    K = _FakeKKT()
    _raises(_lib.CPK_ERR_ARGS, cpk.autograd.kkt_solve_batch, K, _FakeM(), "minres", None, None, None, None, None)
