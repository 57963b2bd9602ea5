"""The C ABI of the factor report and the pivot_min engine option without a device: the four
entries exist, refuse NULL arguments, the ABI version is unchanged (the entries are additive) and
the option is validated like split_tol."""
import ctypes as C

import numpy as np
import pytest

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib
from cpkrylov_amd.synthetic import saddle_system
from test_mex_shim import Mex, _expect_error

NEW = ("cpk_pc_factor_report", "cpk_pc_pivot_shift", "cpk_analysis_factor_report", "cpk_analysis_pivot_shift")


def test_new_symbols_exported():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.EXPORTED, n


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3


def test_report_struct_layout():
    """cpk_factor_report: six int64 then four doubles, no padding."""
    assert C.sizeof(_lib.FactorReport) == 80
    assert [f[0] for f in _lib.FactorReport._fields_] == [
        "n_pos", "n_neg", "n_wrong", "first_wrong", "n_perturbed", "argmin_abs", "min_abs", "max_abs", "max_shift",
        "pivot_min"]


def test_null_arguments_are_refused():
    L = _lib.lib
    x = np.ones(4)
    px = x.ctypes.data_as(C.POINTER(C.c_double))
    rep = _lib.FactorReport()
    rep.n_pos = 7
    for f in (L.cpk_pc_factor_report, L.cpk_analysis_factor_report):
        assert f(None, C.byref(rep)) == _lib.CPK_ERR_ARGS
        assert b"NULL" in L.cpk_last_error()
    for f in (L.cpk_pc_pivot_shift, L.cpk_analysis_pivot_shift):
        assert f(None, px) == _lib.CPK_ERR_ARGS
    # NULL outputs: the check comes before the handle is looked at, so a stand-in handle is safe
    h = C.c_void_p(x.ctypes.data)
    for f in NEW:
        assert getattr(L, f)(h, None) == _lib.CPK_ERR_ARGS, f
    assert rep.n_pos == 7 and np.all(x == 1.0)  # nothing written


@pytest.mark.parametrize("bad", ["-1", "nan", "inf", "abc", "-inf", "1e-9x", ""])
def test_pivot_min_refused(bad, monkeypatch):
    S = saddle_system(N=400)
    with pytest.raises(cpk.CpkError) as e:
        cpk.analyze(S["G"], S["B"], -S["C"], options=f"pivot_min={bad};")
    assert e.value.code == _lib.CPK_ERR_ARGS
    if bad:  # an empty variable is a set one: refused too
        monkeypatch.setenv("CPK_PIVOT_MIN", bad)
        with pytest.raises(cpk.CpkError) as e:
            cpk.analyze(S["G"], S["B"], -S["C"])
        assert e.value.code == _lib.CPK_ERR_ARGS


def test_pivot_min_accepted_from_options_and_environment(monkeypatch):
    S = saddle_system(N=400)
    assert cpk.analyze(S["G"], S["B"], -S["C"])["report"]["pivot_min"] == 0.0
    for spec in ({"pivot_min": 1e-9}, "pivot_min=1e-9;", {"pivot_min": "1e-9"}):
        assert cpk.analyze(S["G"], S["B"], -S["C"], options=spec)["report"]["pivot_min"] == 1e-9
    monkeypatch.setenv("CPK_PIVOT_MIN", "2.5e-7")
    assert cpk.analyze(S["G"], S["B"], -S["C"])["report"]["pivot_min"] == 2.5e-7
    assert cpk.analyze(S["G"], S["B"], -S["C"], options={"pivot_min": 0})["report"]["pivot_min"] == 0.0


def test_mex_pc_factor_report_argument_count():
    mex = Mex()
    _expect_error(mex, "cpk:args", "pc_factor_report", nlhs=2)  # no handle
    _expect_error(mex, "cpk:args", "pc_factor_report", np.ones(3), nlhs=2)  # not a handle
    assert mex.live()["mats"] == 0 and mex.live()["calloc"] == 0
