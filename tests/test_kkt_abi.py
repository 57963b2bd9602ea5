"""The saddle-point operator's C entries (cpk_kkt_*) without a device: they exist with the
header's signatures, the header says what a caller must know, the ABI version is unchanged, and
every refusal that needs no device answers with its code and leaves the outputs untouched."""
import ctypes as C
import os
import re

import numpy as np

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpk_kkt_create", "cpk_kkt_destroy", "cpk_kkt_get_info", "cpk_kkt_apply", "cpk_kkt_apply_device",
       "cpk_kkt_residual", "cpk_kkt_residual_device", "cpk_kkt_residual_device_sums", "cpk_kkt_solve", "cpk_kkt_solve_device", "cpk_kkt_set_route",
       "cpk_kkt_route_info")
PD = C.POINTER(C.c_double)
HEADER = open(os.path.join(ROOT, "include", "cpk.h")).read()


def _ctype(param):
    """the ctypes type _SIGS must hold for one parameter of a declaration in cpk.h"""
    param = " ".join(param.split())
    name = re.search(r"(\w+)(\[\d*\])?$", param).group(1)
    pointer = "*" in param or param.endswith("]")
    if re.match(r"cpk_kkt \*", param):
        return C.POINTER(C.c_void_p)
    if re.match(r"(const )?cpk_(mat|pc|ctx|kkt)\b", param):
        return C.c_void_p
    if "cpk_opts" in param:
        return C.POINTER(_lib.Opts)
    if "cpk_stats" in param:
        return C.POINTER(_lib.Stats)
    if "double" in param and pointer:
        return C.c_void_p if name.startswith("d_") else PD  # device pointers travel as void *
    if "int64_t" in param:
        return C.POINTER(C.c_int64) if pointer else C.c_int64
    if re.match(r"int \w+$", param):
        return C.c_int
    raise AssertionError(f"unmapped parameter {param!r}")


def test_signatures_match_the_header():
    for n in NEW:
        m = re.search(r"^int\s+" + n + r"\s*\(([^)]*)\)\s*;", HEADER, re.M)
        assert m, f"{n} is not declared in cpk.h"
        want = [_ctype(p) for p in m.group(1).split(",")]
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTED, n
        args, res = _lib._SIGS[n]
        assert res is C.c_int and args == want, (n, args, want)
    assert re.search(r"typedef struct cpk_kkt_s \*cpk_kkt;", HEADER)


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3
    assert "#define CPK_ABI_VERSION 3" in HEADER


def test_header_states_the_contract():
    text = " ".join(HEADER.split())
    for phrase in ("HANDLES MUST OUTLIVE K", "reg_cpkrylov.m:152-175", "CORRECTION SYSTEM", "CPK_ERR_UNSUPPORTED",
                   "R == Bm with ldr == ldb"):
        assert phrase in text, phrase


def test_python_front_end_exists():
    assert hasattr(cpk, "KKT") and "KKT" in cpk.__all__
    for name in ("apply", "residual", "solve", "info", "set_route", "route_info", "__matmul__"):
        assert hasattr(cpk.KKT, name), name


def test_refusals_without_a_device():
    lib = _lib.lib
    h = C.c_void_p()
    sentinel = np.full(8, -7.5)
    out, info = sentinel.copy(), (C.c_int64 * 8)(*([-7] * 8))
    pd = out.ctypes.data_as(PD)
    # NULL handles and operands: CPK_ERR_ARGS, nothing written
    assert lib.cpk_kkt_create(None, None, None, None, C.byref(h)) == _lib.CPK_ERR_ARGS and not h
    assert lib.cpk_kkt_get_info(None, info) == _lib.CPK_ERR_ARGS and list(info) == [-7] * 8
    assert lib.cpk_kkt_apply(None, pd, pd) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_apply_device(None, None, None) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual(None, 1, pd, 8, pd, 8, pd, 8, pd) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual_device(None, 1, None, 8, None, 8, None, 8, None) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual_device_sums(None, 1, None, 8, None, 8, None, 8, pd) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_solve(None, 2, pd, None, None, pd, 0, None, pd) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_solve_device(None, 2, None, None, None, None, 1, None, pd) == _lib.CPK_ERR_ARGS
    assert b"NULL" in lib.cpk_last_error()
    assert np.array_equal(out, sentinel)
    assert lib.cpk_kkt_destroy(None) == _lib.CPK_OK
    assert lib.cpk_kkt_set_route(None, 1) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_route_info(None, info) == _lib.CPK_ERR_ARGS and list(info) == [-7] * 8
    # a NULL context with live matrix handles: still the NULL check, before anything is built
    A = cpk.Matrix(np.eye(2), host_only=True)
    assert lib.cpk_kkt_create(None, A.h, A.h, A.h, C.byref(h)) == _lib.CPK_ERR_ARGS and not h
