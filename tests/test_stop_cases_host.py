"""The stop-logic case table (stop_cases.py) against the oracle in exact mode -- without a device.

Every case runs through the oracle's reg_cpkrylov on its own RCM factorization and must report
the table's niters, solved and history length with a finite x, and none may raise: this is what
keeps tests/test_gpu_stop_matrix.py, which holds the engine to the oracle case by case, from
passing on an error path (on these fixtures no method reaches its indefinite-preconditioner
error within the iterations the table asks for).  The one expected error, cpgmres with
itmax < 1, is an argument error that names the reference line."""
import functools

import numpy as np
import pytest

import fixtures as F
import stop_cases as S
from oracle import oracle as O


@functools.lru_cache(maxsize=None)
def _run(i):
    c = S.CASES[i]
    P = S.problem(c)
    with O.exact():
        return O.reg_cpkrylov(c.method, P["rhs"], P["Q"], P["B"], P["C"], P["G"], S.options(c), order="rcm")


def test_table_covers_the_issue():
    """every family for every method, and the two option grids on both systems"""
    by = {}
    for c in S.CASES:
        by.setdefault((c.group, c.method), []).append(c)
    for method in S.METHODS:
        itmaxes = sorted(c.extra["itmax"] for c in by[("itmax", method)])
        assert itmaxes == ([1, 2, 7, 15, 16, 17] if method == "gmres" else [0, 1, 2, 7, 15, 16, 17])
        assert len(by[("zero_tol", method)]) == 1 and len(by[("iter0", method)]) == 2
        assert len(by[("early", method)]) == 1 and len(by[("tol", method)]) == 1
        assert [c.rhs for c in by[("zero_rhs", method)]] == ["zero"]
        assert all(c.system == S.BIG for g in S.BAND_GROUPS + ("early", "tol") for c in by[(g, method)])
    grid = {(c.system, c.extra["restart"], c.extra["itmax"]) for c in by[("restart", "gmres")]}
    assert grid == {(s, r, i) for s in (S.BIG, S.SMALL) for r in (1, 5, 16, 17) for i in (1, 15, 16, 17, 60)}
    grid = {(c.system, c.extra["mem"], c.extra["itmax"]) for c in by[("mem", "dqgmres")]}
    assert grid == {(s, q, i) for s in (S.BIG, S.SMALL) for q in (1, 2, 3, 16, 17, 1000) for i in (1, 15, 16, 17, 60)}
    assert len(by[("cycle_end", "gmres")]) == 1 and len(by[("overrun", "gmres")]) == 1
    assert F.load(S.BIG)["n"] + F.load(S.BIG)["m"] == 5500 and F.load(S.SMALL)["n"] + F.load(S.SMALL)["m"] == 725
    # the table's measured values, spelled out where the issue lists them
    big = {(c.extra["restart"], c.extra["itmax"]): c.expect for c in by[("restart", "gmres")] if c.system == S.BIG}
    small = {(c.extra["restart"], c.extra["itmax"]): c.expect for c in by[("restart", "gmres")] if c.system == S.SMALL}
    assert [big[(16, i)]["niters"] for i in (1, 15, 16, 17, 60)] == [16, 16, 16, 32, 63] and big[(16, 60)]["solved"]
    assert [big[(17, i)]["niters"] for i in (1, 15, 16, 17, 60)] == [17, 17, 17, 17, 63] and big[(17, 60)]["solved"]
    assert all(big[(1, i)]["niters"] == i and small[(1, i)]["niters"] == i for i in (1, 15, 16, 17, 60))
    assert (small[(16, 60)]["niters"], small[(17, 60)]["niters"]) == (64, 68)
    assert not small[(16, 60)]["solved"] and not small[(17, 60)]["solved"]
    assert [c.expect["niters"] for c in by[("itmax", "gmres")]] == [5, 5, 10, 15, 20, 20]
    assert by[("zero_tol", "gmres")][0].expect["niters"] == 25


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=S.IDS)
def test_oracle_reports_the_table(i):
    c = S.CASES[i]
    x, stats = _run(i)  # an OracleError here fails the case: no case may raise
    assert stats["niters"] == c.expect["niters"]
    assert stats["solved"] == c.expect["solved"]
    hists = [k for k in stats if k.endswith("History")]
    assert len(hists) == (3 if c.method == "symmlq" else 1)
    for k in hists:
        assert len(stats[k]) == c.expect["hist_len"], k
        assert np.all(np.isfinite(stats[k])), k
    assert np.all(np.isfinite(x))
    if c.method == "cglanczos":
        assert stats["status"] == S.expected_status(c)
    if c.expect.get("x") == "shift":
        P, opts = S.problem(c), S.options(c)
        with O.exact():
            xy0 = S.shift(P, S.oracle_precond(O, P, opts))
        assert np.any(xy0 != 0)  # the fixture's second block is not zero: the shift is live
        assert np.array_equal(x, xy0)
    if c.expect.get("x") == "zero":
        assert not np.any(x != 0)  # zeros of either sign, no NaN
        assert all(np.array_equal(stats[k], [0.0]) for k in hists)


def test_cycle_end_precondition():
    """the cycle-end case stops because residHistory[10] is the first entry under rtol * residHistory[0],
    at the last iteration of the second cycle of 5"""
    (i,) = [j for j, c in enumerate(S.CASES) if c.group == "cycle_end"]
    c = S.CASES[i]
    h = _run(i)[1]["residHistory"]
    assert c.extra["restart"] == 5 and c.extra["atol"] == 0.0 and c.extra["rtol"] == S.CYCLE_END_RTOL
    assert h[10] / h[0] < S.CYCLE_END_RTOL < h[9] / h[0]
    assert abs(h[9] / h[0] - 0.02059) < 5e-6 and abs(h[10] / h[0] - 0.01496) < 5e-6
    assert np.all(h[:10] > S.CYCLE_END_RTOL * h[0])


@pytest.mark.parametrize("c", S.ERROR_CASES, ids=[S.case_id(c) for c in S.ERROR_CASES])
def test_oracle_refuses_the_error_cases(c):
    P = S.problem(c)
    with pytest.raises(O.OracleError) as e:
        with O.exact():
            O.reg_cpkrylov(c.method, P["rhs"], P["Q"], P["B"], P["C"], P["G"], S.options(c), order="rcm")
    assert e.value.code == 3  # ORC_ERR_ARGS
    assert c.expect["error"] in e.value.msg


def test_oracle_gmres_refuses_itmax_below_one_on_every_entry():
    """cpgmres.m:148: outermax = ceil(itmax/restart) < 1 for itmax <= 0, whatever the restart"""
    P = F.load(S.SMALL)
    M = S.oracle_precond(O, P, F.EXPROG_OPTS)
    for itmax in (0, -3):
        for r in (1, 5):
            with pytest.raises(O.OracleError) as e:
                O.method("gmres", P["rhs"][:P["n"]], P["Q"], P["C"], M, dict(F.EXPROG_OPTS, itmax=itmax, restart=r))
            assert e.value.code == 3 and "cpgmres.m:267" in e.value.msg
    # itmax in (0, 1) still runs one cycle, as the reference does
    x, y, stats = O.method("gmres", P["rhs"][:P["n"]], P["Q"], P["C"], M, dict(F.EXPROG_OPTS, itmax=0.5, restart=2))
    assert stats["niters"] == 2 and len(stats["residHistory"]) == 3


def test_oracle_history_capacity():
    """the default capacity covers cpgmres's overrun of itmax (cpgmres.m:148,203); a caller's own
    hist_cap is taken as given, and one that is too small is still refused"""
    P = F.load(S.SMALL)
    for itmax, r, cap in ((1, 5, 8), (7, 5, 13), (17, 5, 23), (15, 5, 18), (0, 5, 3), (60, 17, 71)):
        assert O._hist_cap("gmres", dict(itmax=itmax, restart=r), 725) == cap
    assert O._hist_cap("gmres", None, 725) == 753 and O._hist_cap("gmres", dict(restart=100), 725) == 803
    for m in ("cg", "cglanczos", "minres", "symmlq", "dqgmres"):
        assert O._hist_cap(m, dict(itmax=7, restart=5), 725) == 10 and O._hist_cap(m, None, 725) == 728
    opts = dict(F.EXPROG_OPTS, itmax=7, restart=5)
    x, s = O.reg_cpkrylov("gmres", P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts)
    assert s["niters"] == 10 and len(s["residHistory"]) == 11
    x2, s2 = O.reg_cpkrylov("gmres", P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts, hist_cap=11)
    assert np.array_equal(x, x2) and np.array_equal(s["residHistory"], s2["residHistory"])
    with pytest.raises(O.OracleError) as e:
        O.reg_cpkrylov("gmres", P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts, hist_cap=10)
    assert "history buffer too small" in e.value.msg
