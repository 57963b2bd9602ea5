"""The operator-valued A at the ABI and in Python, without a GPU: the new symbols are declared in
include/cpk.h and exported, the new status has its number, and cpk.Operator checks its arguments
before it touches a device."""
import os
import re

import pytest

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpk_op_create", "cpk_op_destroy", "cpk_op_get_info", "cpk_op_apply_device", "cpk_method_solve_op",
       "cpk_method_solve_op_device", "cpk_reg_solve_op", "cpk_reg_solve_op_device", "cpk_mat_spmv_device")


def header():
    return open(os.path.join(ROOT, "include", "cpk.h")).read()


def test_new_symbols_are_declared_and_exported():
    src = header()
    for name in NEW:
        assert re.search(r"^int\s+" + name + r"\s*\(", src, re.M), name
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
    assert re.search(r"typedef int \(\*cpk_op_fn\)\(void \*user, const double \*d_x, double \*d_y, int64_t n, "
                     r"void \*stream\);", src)
    assert re.search(r"#define CPK_OP_CAPTURABLE 1\b", src) and _lib.CPK_OP_CAPTURABLE == 1


def test_callback_status_number_and_abi_version():
    assert _lib.CPK_ERR_CALLBACK == 9
    assert re.search(r"CPK_ERR_CALLBACK = 9\b", header())
    assert _lib.lib.cpk_abi_version() == 3  # the additions are additive


def test_operator_checks_its_arguments_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(api, "default_context", no_device)
    for bad in (None, 3, "spmv"):
        with pytest.raises(cpk.CpkError) as e:
            cpk.Operator(4, bad)
        assert e.value.code == _lib.CPK_ERR_ARGS
    for n in (-1, 2.5):
        with pytest.raises(cpk.CpkError) as e:
            cpk.Operator(n, lambda x, y, n, s: 0)
        assert e.value.code == _lib.CPK_ERR_ARGS


def test_null_handles_are_refused_without_a_device():
    import ctypes as C
    v = (C.c_int64 * 4)()
    assert _lib.lib.cpk_op_get_info(None, v) == _lib.CPK_ERR_ARGS
    assert _lib.lib.cpk_op_apply_device(None, None, None) == _lib.CPK_ERR_ARGS
    assert _lib.lib.cpk_mat_spmv_device(None, None, None) == _lib.CPK_ERR_ARGS
    h = C.c_void_p()
    assert _lib.lib.cpk_op_create(None, 1, _lib.OpFn(), None, 0, C.byref(h)) == _lib.CPK_ERR_ARGS
    assert _lib.lib.cpk_op_destroy(None) == _lib.CPK_OK


def test_matrix_only_entries_refuse_an_operator_in_python(monkeypatch):
    """KKT, the preconditioner's blocks and B, C, G take matrices: refused before any C entry."""
    op = object.__new__(cpk.Operator)  # no handle: the refusals may not reach the library
    op.h = None
    for call in (lambda: api._as_matrix(op, None), lambda: cpk.KKT(op, None, None)):
        with pytest.raises(cpk.CpkError) as e:
            call()
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
