"""The C ABI of the refined block apply Y = M*X (opLDL2.multiply column by column,
ops/opLDL2.m:138-149, 161-188) without a device: the two entries exist, refuse NULL arguments
before anything is touched, the ABI version is unchanged (the entries are additive), the MEX
gateway's `pc_apply_multi` counts its arguments before a device is touched, and the Python
operator has its block method."""
import ctypes as C
import inspect

import numpy as np

from cpkrylov_amd import _lib
from test_mex_shim import Mex, _expect_error

NEW = ("cpk_pc_apply_multi", "cpk_pc_apply_multi_device")


def test_new_symbols_exported():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.EXPORTED, n


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3


def test_null_arguments_are_refused():
    L = _lib.lib
    x = np.ones(4)
    y = np.ones(4)
    nit = np.full(2, 7, np.int32)
    px, py = x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double))
    pn = nit.ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(x.ctypes.data)  # stands for a device pointer; never dereferenced
    # NULL handle
    assert L.cpk_pc_apply_multi(None, 2, px, 2, py, 2, pn) == _lib.CPK_ERR_ARGS
    assert b"NULL" in L.cpk_last_error()
    assert L.cpk_pc_apply_multi_device(None, 2, fake, 2, fake, 2, fake) == _lib.CPK_ERR_ARGS
    # NULL arrays: the check comes before the handle is looked at, so a stand-in handle is safe
    h = C.c_void_p(x.ctypes.data)
    assert L.cpk_pc_apply_multi(h, 2, None, 2, py, 2, pn) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_multi(h, 2, px, 2, None, 2, pn) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_multi(h, 2, None, 2, None, 2, None) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_multi_device(h, 2, None, 2, fake, 2, fake) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_multi_device(h, 2, fake, 2, None, 2, None) == _lib.CPK_ERR_ARGS
    assert np.all(x == 1.0) and np.all(y == 1.0) and list(nit) == [7, 7]  # nothing written


def test_operator_has_the_block_method():
    import cpkrylov_amd as cpk
    sig = inspect.signature(cpk.opLDL2.apply_block)
    assert list(sig.parameters) == ["self", "Z", "return_steps"]
    assert sig.parameters["return_steps"].default is False
    assert inspect.signature(cpk.opLDL2.to_dense).parameters["chunk"].default == 64
    assert cpk.opLDL2.__matmul__ is cpk.opLDL2.__mul__


def test_engine_option_is_known():
    """the option that forces the panel kernels parses like every boolean engine option"""
    import cpkrylov_amd as cpk
    a = cpk.analyze(np.eye(2), np.ones((1, 2)), -np.eye(1), options=dict(apply_multi_panel=1))
    assert a["info"]["N"] == 3


def test_mex_pc_apply_multi_argument_count():
    mex = Mex()
    _expect_error(mex, "cpk:args", "pc_apply_multi")  # no handle, no matrix
    _expect_error(mex, "cpk:args", "pc_apply_multi", 1.0)  # no matrix
    _expect_error(mex, "cpk:args", "pc_apply_multi", 1.0, np.ones(3))  # not a handle
    assert mex.live()["mats"] == 0 and mex.live()["calloc"] == 0
