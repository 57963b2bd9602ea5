"""The exactly rounded residual's and the refined solve's entries without a device: they exist with
the header's signatures, the Python methods have the documented signatures, the header states what a
caller must know, the ABI version is unchanged, and the refusals that need no device answer with
their code and leave the outputs untouched."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpk_kkt_residual_exact", "cpk_kkt_residual_exact_device", "cpk_kkt_residual_exact_device_sums",
       "cpk_kkt_solve_refined", "cpk_kkt_solve_refined_device")
PD = C.POINTER(C.c_double)
HEADER = open(os.path.join(ROOT, "include", "cpk.h")).read()


def _ctype(param):
    """the ctypes type _SIGS must hold for one parameter of a declaration in cpk.h"""
    param = " ".join(param.split())
    name = re.search(r"(\w+)$", param).group(1)
    pointer = "*" in param
    if re.match(r"(const )?cpk_(pc|kkt)\b", param):
        return C.c_void_p
    if "cpk_opts" in param:
        return C.POINTER(_lib.Opts)
    if "cpk_stats" in param:
        return C.POINTER(_lib.Stats)
    if "double" in param and pointer:
        return C.c_void_p if name.startswith("d_") else PD  # device pointers travel as void *
    if "int64_t" in param and not pointer:
        return C.c_int64
    if re.match(r"int \*\w+$", param):
        return C.POINTER(C.c_int)
    if re.match(r"int \w+$", param):
        return C.c_int
    raise AssertionError(f"unmapped parameter {param!r}")


def _params(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", HEADER, re.M)
    assert m, f"{name} is not declared in cpk.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_signatures_match_the_header():
    for n in NEW:
        want = [_ctype(p) for p in _params(n)]
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTED, n
        args, res = _lib._SIGS[n]
        assert res is C.c_int and args == want, (n, args, want)


def test_argument_lists_are_those_of_the_plain_entries():
    """cpk_kkt_residual_exact* take cpk_kkt_residual*'s arguments; cpk_kkt_solve_refined* take
    cpk_kkt_solve*'s with max_steps after warm and steps_out at the end"""
    for suffix in ("", "_device", "_device_sums"):
        assert _params("cpk_kkt_residual_exact" + suffix) == _params("cpk_kkt_residual" + suffix)
    for suffix in ("", "_device"):
        plain, refined = _params("cpk_kkt_solve" + suffix), _params("cpk_kkt_solve_refined" + suffix)
        w = plain.index("int warm")
        assert refined == plain[:w + 1] + ["int max_steps"] + plain[w + 1:] + ["int *steps_out"]


def test_python_signatures():
    sig = inspect.signature(cpk.KKT.residual_exact)
    assert list(sig.parameters) == ["self", "z", "b", "out"] and sig.parameters["out"].default is None
    sig = inspect.signature(cpk.KKT.solve_refined)
    assert list(sig.parameters) == ["self", "method", "b", "M", "opts", "x0", "max_steps", "out"]
    assert [sig.parameters[k].default for k in ("opts", "x0", "max_steps", "out")] == [None, None, 3, None]
    assert list(inspect.signature(cpk.KKT.residual).parameters) == ["self", "z", "b", "out", "want_r"]


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3
    assert "#define CPK_ABI_VERSION 3" in HEADER


def test_header_states_the_contract():
    text = " ".join(HEADER.split())
    for phrase in ("r_i = RN( b_i - sum_e K_ie * z_col(e) )", "rounded once to nearest even", "a NaN, in that row only",
                   "EACH DRIVER CALL'S STOP TEST RUNS ON ITS CORRECTION SYSTEM", "4 (max_steps + 1) doubles",
                   "a loop of single-column passes", "under- or overflows"):
        assert phrase in text, phrase


def test_refusals_without_a_device():
    lib = _lib.lib
    sentinel = np.full(8, -7.5)
    out, steps = sentinel.copy(), C.c_int(-7)
    pd = out.ctypes.data_as(PD)
    assert lib.cpk_kkt_residual_exact(None, 1, pd, 8, pd, 8, pd, 8, pd) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual_exact_device(None, 1, None, 8, None, 8, None, 8, None) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual_exact_device_sums(None, 1, None, 8, None, 8, None, 8, pd) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_solve_refined(None, 2, pd, None, None, pd, 0, 3, None, pd, C.byref(steps)) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_solve_refined_device(None, 2, None, None, None, None, 1, 3, None, pd,
                                            C.byref(steps)) == _lib.CPK_ERR_ARGS
    assert b"NULL" in lib.cpk_last_error()
    assert np.array_equal(out, sentinel) and steps.value == -7
