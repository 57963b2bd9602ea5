"""The engine option basis_f32 at the C boundary.

Without a device (a context needs one, the host-only analysis does not): cpk_analyze parses the same
option specs and the same CPK_* environment as a context (opts.cpp), so it shows that the option is
known, validated as a boolean and read from CPK_BASIS_F32; the header names and defines it; the ABI
version is unchanged (an option is no new entry).  With a device (marked gpu): the round trip through
cpk_ctx_set_option / cpk_ctx_get_option / cpk_ctx_get_options and the environment at context creation.

Before the option existed every spec below was refused as an unknown engine option."""
import os

import pytest

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib
from structures import saddle_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = " ".join(open(os.path.join(ROOT, "include", "cpk.h")).read().split())


def _analyze(options=None):
    S = saddle_system(N=400)
    return cpk.analyze(S["G"], S["B"], -S["C"], options=options)["info"]["N"]


@pytest.mark.parametrize("spec", ("basis_f32=1;", "basis_f32=0;", dict(basis_f32=1), dict(basis_f32=0),
                                  dict(basis_f32=True), "exact_dots=1;basis_f32=1;"))
def test_option_is_known(spec, monkeypatch):
    monkeypatch.delenv("CPK_BASIS_F32", raising=False)
    assert _analyze(spec) == _analyze()  # (the analysis itself does not depend on it)


@pytest.mark.parametrize("bad", ("half", "2x", "f32"))
def test_bad_values_are_refused(bad, monkeypatch):
    monkeypatch.delenv("CPK_BASIS_F32", raising=False)
    with pytest.raises(cpk.CpkError) as e:
        _analyze(f"basis_f32={bad};")
    assert e.value.code == _lib.CPK_ERR_ARGS and "basis_f32" in str(e.value)
    monkeypatch.setenv("CPK_BASIS_F32", bad)
    with pytest.raises(cpk.CpkError) as e:
        _analyze()
    assert e.value.code == _lib.CPK_ERR_ARGS and "basis_f32" in str(e.value)


def test_environment_is_accepted(monkeypatch):
    for v in ("1", "0"):
        monkeypatch.setenv("CPK_BASIS_F32", v)
        assert _analyze() > 0


def test_header_names_and_defines_the_option():
    for phrase in ("basis_f32", "CPK_BASIS_F32", "rounded ONCE", "converts the float exactly to double",
                   "on the unrounded vector", "CPK_ERR_UNSUPPORTED before anything is written"):
        assert phrase in HEADER, phrase


def test_abi_version_unchanged():
    assert _lib.lib.cpk_abi_version() == 3
    assert "#define CPK_ABI_VERSION 3" in HEADER


def _listed(ctx):
    return dict(item.split("=", 1) for item in ctx.options_string().split(";") if item)


@pytest.mark.gpu
def test_context_round_trip(monkeypatch):
    monkeypatch.delenv("CPK_BASIS_F32", raising=False)
    ctx = cpk.Context()
    try:
        assert ctx.get_option("basis_f32") == "0" and _listed(ctx)["basis_f32"] == "0"  # off by default
        for value, want in ((1, "1"), ("0", "0"), (True, "1"), (0, "0")):
            ctx.set_option("basis_f32", value)
            assert ctx.get_option("basis_f32") == want and _listed(ctx)["basis_f32"] == want
        with pytest.raises(cpk.CpkError) as e:
            ctx.set_option("basis_f32", "half")
        assert e.value.code == _lib.CPK_ERR_ARGS and ctx.get_option("basis_f32") == "0"
        with cpk.engine_options(ctx, basis_f32=1):
            assert ctx.get_option("basis_f32") == "1"
            again = cpk.Context(options=dict(_listed(ctx)))  # the listing is itself a valid set of options
            assert again.get_option("basis_f32") == "1"
            again.close()
        assert ctx.get_option("basis_f32") == "0"
    finally:
        ctx.close()


@pytest.mark.gpu
def test_environment_is_read_at_context_creation(monkeypatch):
    monkeypatch.setenv("CPK_BASIS_F32", "1")
    ctx = cpk.Context()
    monkeypatch.setenv("CPK_BASIS_F32", "0")  # a later change of the variable does not reach a living context
    try:
        assert ctx.get_option("basis_f32") == "1"
        other = cpk.Context()
        assert other.get_option("basis_f32") == "0"
        other.close()
    finally:
        ctx.close()
