"""The C ABI and the Python surface of the lockstep block solve (cpcg and cpminres on a block of
right-hand sides, kernels/cpcg.m:1 and kernels/cpminres.m:1 column by column) without a device:
the entries exist, the ABI version is unchanged (they are additive), NULL arguments and bad
dimensions are refused before anything is touched, the Python solvers take a block and refuse it
for the methods that have none, and the MEX gateway's `method_solve_multi` counts its arguments
before a device is touched."""
import ctypes as C
import inspect

import numpy as np
import pytest

from cpkrylov_amd import _lib
from test_mex_shim import Func, Mex, _expect_error

NEW = ("cpk_method_solve_multi", "cpk_method_solve_multi_device", "cpk_reg_solve_multi", "cpk_reg_solve_multi_device",
       "cpk_debug_spmm")
PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_new_symbols_exported():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.EXPORTED, n


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3


def _host_mats():
    """A (3 x 3) and C (2 x 2) without a device: the dimension checks read nothing else"""
    import cpkrylov_amd as cpk
    return cpk.Matrix(np.eye(3), host_only=True), cpk.Matrix(np.eye(2), host_only=True)


def test_null_arguments_are_refused():
    L = _lib.lib
    A, Cm = _host_mats()
    b, x, y = np.ones(6), np.full(6, 2.0), np.full(4, 3.0)
    status = (C.c_int * 2)(7, 7)
    pb, px, py = (v.ctypes.data_as(PD) for v in (b, x, y))
    h = C.c_void_p(b.ctypes.data)  # stands for a context / preconditioner / device pointer; never dereferenced
    for args in ((None, 2, 2, pb, 3, A.h, Cm.h, h, None, px, 3, py, 2, None, status),  # no context
                 (h, 2, 2, pb, 3, A.h, Cm.h, None, None, px, 3, py, 2, None, status),  # no preconditioner
                 (h, 2, 2, pb, 3, None, Cm.h, h, None, px, 3, py, 2, None, status),    # no A
                 (h, 2, 2, None, 3, A.h, Cm.h, h, None, px, 3, py, 2, None, status),   # no B
                 (h, 2, 2, pb, 3, A.h, Cm.h, h, None, None, 3, py, 2, None, status),   # no X
                 (h, 2, 2, pb, 3, A.h, Cm.h, h, None, px, 3, None, 2, None, status)):  # no Y with m > 0
        assert L.cpk_method_solve_multi(*args) == _lib.CPK_ERR_ARGS
        assert b"NULL" in L.cpk_last_error()
    assert L.cpk_method_solve_multi_device(h, 2, 2, None, 3, A.h, Cm.h, h, None, h, 5, None, status) == _lib.CPK_ERR_ARGS
    assert L.cpk_method_solve_multi_device(h, 2, 2, h, 3, A.h, Cm.h, h, None, None, 5, None, status) == _lib.CPK_ERR_ARGS
    assert L.cpk_method_solve_multi_device(h, 2, 2, h, 3, A.h, Cm.h, None, None, h, 5, None, status) == _lib.CPK_ERR_ARGS
    assert L.cpk_reg_solve_multi(h, 2, 2, None, 5, A.h, A.h, Cm.h, h, None, px, 5, None, status) == _lib.CPK_ERR_ARGS
    assert L.cpk_reg_solve_multi(h, 2, 2, pb, 5, A.h, A.h, Cm.h, None, None, px, 5, None, status) == _lib.CPK_ERR_ARGS
    assert L.cpk_reg_solve_multi_device(h, 2, 2, h, 5, A.h, None, Cm.h, h, None, h, 5, None, status) == _lib.CPK_ERR_ARGS
    assert L.cpk_debug_spmm(h, A.h, Cm.h, None, 1, pb, 5, px, 5, py) == _lib.CPK_ERR_ARGS
    assert np.all(b == 1.0) and np.all(x == 2.0) and np.all(y == 3.0) and list(status) == [7, 7]  # nothing written


def test_bad_dimensions_are_refused():
    """k < 0 or a leading dimension below the column length: CPK_ERR_DIM from the arguments and the
    host matrices alone (n = 3, m = 2), before the preconditioner is looked at"""
    L = _lib.lib
    A, Cm = _host_mats()
    b, x, y = np.ones(6), np.full(6, 2.0), np.full(4, 3.0)
    status = (C.c_int * 2)(7, 7)
    pb, px, py = (v.ctypes.data_as(PD) for v in (b, x, y))
    h = C.c_void_p(b.ctypes.data)
    ok = dict(k=2, ldb=3, ldx=3, ldy=2)
    for bad in (dict(k=-1), dict(ldb=2), dict(ldx=2), dict(ldy=1)):
        a = dict(ok, **bad)
        rc = L.cpk_method_solve_multi(h, 2, a["k"], pb, a["ldb"], A.h, Cm.h, h, None, px, a["ldx"], py, a["ldy"], None,
                                      status)
        assert rc == _lib.CPK_ERR_DIM, bad
    assert L.cpk_method_solve_multi_device(h, 2, -1, h, 3, A.h, Cm.h, h, None, h, 5, None, status) == _lib.CPK_ERR_DIM
    assert L.cpk_method_solve_multi_device(h, 2, 2, h, 2, A.h, Cm.h, h, None, h, 5, None, status) == _lib.CPK_ERR_DIM
    assert L.cpk_method_solve_multi_device(h, 2, 2, h, 3, A.h, Cm.h, h, None, h, 4, None, status) == _lib.CPK_ERR_DIM
    assert L.cpk_reg_solve_multi(h, 2, 2, pb, 4, A.h, A.h, Cm.h, h, None, px, 5, None, status) == _lib.CPK_ERR_DIM
    assert L.cpk_reg_solve_multi(h, 2, -3, pb, 5, A.h, A.h, Cm.h, h, None, px, 5, None, status) == _lib.CPK_ERR_DIM
    assert L.cpk_reg_solve_multi_device(h, 2, 2, h, 5, A.h, A.h, Cm.h, h, None, h, 4, None, status) == _lib.CPK_ERR_DIM
    assert np.all(x == 2.0) and np.all(y == 3.0) and list(status) == [7, 7]


def test_python_solvers_take_a_block():
    import cpkrylov_amd as cpk
    from cpkrylov_amd import api
    for fn in (cpk.cpcg, cpk.cpminres, cpk.cpgmres):
        p = inspect.signature(fn).parameters
        assert list(p) == ["b", "A", "Cm", "M", "opts", "raise_on_error"] and p["raise_on_error"].default is True
    assert inspect.signature(cpk.reg_cpkrylov).parameters["raise_on_error"].default is True
    assert api.BLOCK_METHODS == ("cg", "minres")
    # a vector or an n x 1 array keeps the single-column path
    assert not api._is_block(np.ones(4)) and not api._is_block(np.ones((4, 1)))
    assert api._is_block(np.ones((4, 2))) and api._is_block(np.ones((4, 0)))


@pytest.mark.parametrize("name", ("cglanczos", "symmlq", "gmres", "dqgmres"))
def test_other_methods_refuse_a_block(name):
    """decided from the method alone, before a device is touched"""
    from cpkrylov_amd import api
    with pytest.raises(_lib.CpkError) as e:
        api._block_call(name, 2, {}, 3, 2, None, True)
    assert e.value.code == _lib.CPK_ERR_UNSUPPORTED


def test_mex_method_solve_multi_argument_count():
    """the command exists (not the gateway's `unknown command` exit, which has the same identifier)
    and its own count check answers, with the count it expects and the count it got"""
    mex = Mex()
    for args, given in (((), 1), ((Func("@cpminres"), np.ones((3, 2))), 3),
                        ((Func("@cpminres"), np.ones((3, 2)), 1.0, 1.0), 5)):
        e = _expect_error(mex, "cpk:args", "method_solve_multi", *args, nlhs=4)
        assert e.msg == f"cpk_mex method_solve_multi: 6 arguments expected, {given} given", e.msg
    # enough arguments: the method's name is looked at first, before any matrix is converted
    e = _expect_error(mex, "cpk:args", "method_solve_multi", Func("@cpnothing"), np.ones((3, 2)), 1.0, 1.0, 1.0, nlhs=4)
    assert e.msg == "unknown method @cpnothing", e.msg
    # a sparse B is refused by the command itself, still before a device is touched
    import scipy.sparse as sp
    e = _expect_error(mex, "cpk:args", "method_solve_multi", Func("@cpminres"), sp.identity(3, format="csc"), 1.0, 1.0,
                      1.0, nlhs=4)
    assert e.msg == "B must be a dense real matrix", e.msg
    assert mex.live()["mats"] == 0 and mex.live()["calloc"] == 0
