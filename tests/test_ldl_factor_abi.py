"""The C ABI of the bare factor operator (opLDL2's M' / conj(M), ops/opLDL2.m:127-136) without a
device: the five entries exist, refuse NULL arguments before anything is touched, the ABI version
is unchanged (the entries are additive), and the MEX gateway's `pc_apply_ldl` counts its
arguments before a device is touched."""
import ctypes as C

import numpy as np

from cpkrylov_amd import _lib
from test_mex_shim import Mex, _expect_error

NEW = ("cpk_pc_apply_ldl", "cpk_pc_apply_ldl_device", "cpk_pc_apply_ldl_multi", "cpk_pc_apply_ldl_multi_device",
       "cpk_pc_multi_info")


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
    px, py = x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double))
    info = (C.c_int64 * 4)(7, 7, 7, 7)
    fake = C.c_void_p(x.ctypes.data)  # stands for a device pointer; never dereferenced
    # NULL handle
    assert L.cpk_pc_apply_ldl(None, px, py) == _lib.CPK_ERR_ARGS
    assert b"NULL" in L.cpk_last_error()
    assert L.cpk_pc_apply_ldl_device(None, fake, fake) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_multi(None, 2, px, 2, py, 2) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_multi_device(None, 2, fake, 2, fake, 2) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_multi_info(None, info) == _lib.CPK_ERR_ARGS
    # NULL arrays: the check comes before the handle is looked at, so a stand-in handle is safe
    h = C.c_void_p(x.ctypes.data)
    assert L.cpk_pc_apply_ldl(h, None, py) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl(h, px, None) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_device(h, None, fake) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_device(h, fake, None) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_multi(h, 2, None, 2, py, 2) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_multi(h, 2, px, 2, None, 2) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_multi_device(h, 2, None, 2, fake, 2) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_apply_ldl_multi_device(h, 2, fake, 2, None, 2) == _lib.CPK_ERR_ARGS
    assert L.cpk_pc_multi_info(h, None) == _lib.CPK_ERR_ARGS
    assert list(info) == [7, 7, 7, 7] and np.all(y == 1.0)  # nothing written


def test_package_exports_the_operator_class():
    import cpkrylov_amd as cpk
    assert cpk.opLDL2Factor.__name__ == "opLDL2Factor" and "opLDL2Factor" in cpk.__all__
    assert cpk.opLDL2.H.fget is cpk.opLDL2.ctranspose and cpk.opLDL2.conj is cpk.opLDL2.ctranspose
    assert cpk.opLDL2.ctranspose is not cpk.opLDL2.transpose  # M' is no longer an alias of M


def test_mex_pc_apply_ldl_argument_count():
    mex = Mex()
    _expect_error(mex, "cpk:args", "pc_apply_ldl")  # no handle, no matrix
    _expect_error(mex, "cpk:args", "pc_apply_ldl", 1.0)  # no matrix
    _expect_error(mex, "cpk:args", "pc_apply_ldl", 1.0, np.ones(3))  # not a handle
    assert mex.live()["mats"] == 0 and mex.live()["calloc"] == 0
