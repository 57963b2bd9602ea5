"""Every solver's stop logic against the oracle, across batch boundaries.

The cases of stop_cases.py (the stop by itmax around the end of a batch of 16, at iteration 0,
after one or two iterations, by tolerance, at the end of a GMRES cycle, restart = 1, mem = 1,
mem > itmax, a zero right-hand side), each solved with cpk.reg_cpkrylov under exact_dots on four
engine settings -- adaptive batches, batch = 1, batch = 16 and eager replay -- and compared with
the oracle's exact mode on the product's own factors with ==: niters, solved, status, every
history, x.  A batch is a captured graph of b iterations, so a kernel that does not test the
device's `running` flag, or a post-loop step that reads a scalar the no-op iterations have moved,
changes a bit on the settings whose batch runs past the stop and not on batch = 1; equal to the
oracle on all four, the settings are equal to each other.  The cases stopped by itmax or at
iteration 0 run once more in the default mode against the oracle within the parity tests' bar
(sensitivity.band).  (A fifth setting, batch = 3, which the batch loop rounds up to 4, passed on
every case as well; it was left out to keep the module near the time of test_gpu_exact.py.)

tests/test_stop_cases_host.py proves, without a device, that the oracle reports the table's
values on every case and raises on none."""
import functools

import numpy as np
import pytest

import stop_cases as S
from oracle import oracle as O
from sensitivity import band

pytestmark = pytest.mark.gpu

FLOOR, SAFETY = 1e-8, 10.0  # the parity tests' bar (test_gpu_parity.py): max(FLOOR, SAFETY * band)
SETTINGS = (("adaptive", {}), ("batch1", {"batch": 1}), ("batch16", {"batch": 16}), ("no_graph", {"no_graph": 1}))


class _Rig:
    """one context per engine setting, all with exact inner products, and a default one, each with
    its matrix handles of a system (created once: the solves are short, and converting and
    uploading Q, B, C, G anew for each would be most of the module's time)"""

    def __init__(self):
        import cpkrylov_amd as cpk
        self.ctx = {name: cpk.Context(options=dict(exact_dots=1, **o)) for name, o in SETTINGS}
        self.ctx["default"] = cpk.Context()
        self.handles = {}

    def mats(self, name, P):
        import cpkrylov_amd as cpk
        key = (name, P["name"])
        if key not in self.handles:
            self.handles[key] = [cpk.Matrix(P[k], self.ctx[name]) for k in ("Q", "B", "C", "G")]
        return self.handles[key]


@pytest.fixture(scope="module")
def contexts():
    """the contexts are released with the last object that holds them"""
    return _Rig()


@functools.lru_cache(maxsize=None)
def _problem(system, rhs):
    """the fixture of a case, loaded once and shared: nothing below writes to it"""
    return S.problem(S.Case(system, None, None, None, rhs, None))


def _solve(rig, name, c, P, opts):
    import cpkrylov_amd as cpk
    Q, B, Cm, G = rig.mats(name, P)
    return cpk.reg_cpkrylov(getattr(cpk, "cp" + c.method), P["rhs"], Q, B, Cm, G, opts, ctx=rig.ctx[name])


def _assert_table(c, x, stats, solved, who):
    """what the table (and so the host test's oracle) says of the case"""
    got = (stats["niters"], solved, len(S.history(stats)))
    assert got == (c.expect["niters"], c.expect["solved"], c.expect["hist_len"]), who
    if c.method == "cglanczos":
        assert stats["status"] == S.expected_status(c), who
    if c.expect.get("x") == "zero":
        assert not np.any(x != 0), who  # zeros of either sign, no NaN
        assert np.array_equal(S.history(stats), [0.0]), who


def _assert_same(who, x, stats, flag, xo, so):
    assert stats["niters"] == so["niters"], who
    assert flag["solved"] == so["solved"], who
    if "status" in so:
        assert stats["status"] == so["status"], who
    for k in [k for k in so if k.endswith("History")]:
        assert len(stats[k]) == len(so[k]), (who, k)
        bad = np.flatnonzero(stats[k] != so[k])
        assert bad.size == 0, (who, k, bad[:5], stats[k][bad[:3]], so[k][bad[:3]])
    bad = np.flatnonzero(x != xo)
    assert bad.size == 0, (who, bad.size, bad[:5], np.max(np.abs(x - xo)))


def _assert_in_band(c, P, opts, rig, perm):
    """the default mode: counts equal to the oracle's, values within the parity tests' bar"""
    x, stats, flag = _solve(rig, "default", c, P, opts)
    xo, so = O.reg_cpkrylov(c.method, P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts, perm=perm)
    _assert_table(c, x, stats, flag["solved"], "default mode")
    _assert_table(c, xo, so, so["solved"], "default mode, oracle")
    if "status" in so:
        assert stats["status"] == so["status"]
    if c.rhs == "zero":
        return  # exactly zero on both sides (_assert_table): nothing to take a band of
    bd = band(c.system, c.method, c.extra, perm)
    h0 = S.history(so)[0]
    for k in [k for k in so if k.endswith("History")]:
        assert len(stats[k]) == len(so[k]), k
        dev = np.max(np.abs(stats[k] - so[k])) / h0
        assert dev <= max(FLOOR, SAFETY * bd[k]), (k, dev, bd[k])
    dx = np.linalg.norm(x - xo) / np.linalg.norm(xo)
    assert dx <= max(FLOOR, SAFETY * bd["x"]), (dx, bd["x"])


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=S.IDS)
def test_stop_matches_oracle_on_every_batch_setting(contexts, i):
    c = S.CASES[i]
    P, opts = _problem(c.system, c.rhs), S.options(c)
    runs = [(name, _solve(contexts, name, c, P, opts)) for name, _ in SETTINGS]
    factors = runs[0][1][1]["M"].export_factors()
    Mo = S.oracle_precond(O, P, opts, factors)
    with O.exact():
        xo, so = O.reg_solve(c.method, P["rhs"], P["Q"], P["B"], P["C"], Mo, opts)
        xy0 = S.shift(P, Mo) if c.expect.get("x") == "shift" else None
    for name, (x, stats, flag) in runs:
        print(f"STOP {S.IDS[i]} {name}: niters {stats['niters']} solved {flag['solved']} "
              f"len {len(S.history(stats))} | table {c.expect['niters']} {c.expect['solved']} {c.expect['hist_len']}")
    _assert_table(c, xo, so, so["solved"], "oracle")
    if xy0 is not None:
        assert np.any(xy0 != 0) and np.array_equal(xo, xy0)
    failed = {}  # every setting is compared, so a failure names the settings that differ
    for name, (x, stats, flag) in runs:
        try:
            _assert_same(name, x, stats, flag, xo, so)
            _assert_table(c, x, stats, flag["solved"], name)
        except AssertionError as e:
            failed[name] = str(e).splitlines()[0][:200]
    assert not failed, (sorted(failed), failed)
    if c.group in S.BAND_GROUPS:
        _assert_in_band(c, P, opts, contexts, factors[2])


@pytest.mark.parametrize("c", S.ERROR_CASES, ids=[S.case_id(c) for c in S.ERROR_CASES])
def test_stop_error_cases_are_refused(contexts, c):
    """cpgmres with itmax < 1 (cpgmres.m:267 reads an undefined k): an argument error on every
    setting, as from the oracle, not a "solved" that never looked at the residual"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P, opts = _problem(c.system, c.rhs), S.options(c)
    with pytest.raises(O.OracleError) as eo:
        O.reg_cpkrylov(c.method, P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts)
    assert eo.value.code == 3 and c.expect["error"] in eo.value.msg  # ORC_ERR_ARGS
    for name in [s for s, _ in SETTINGS] + ["default"]:
        with pytest.raises(cpk.CpkError) as e:
            _solve(contexts, name, c, P, opts)
        assert e.value.code == _lib.CPK_ERR_ARGS, name
        assert c.expect["error"] in str(e.value), name
    # the method entry refuses it too, and a fractional itmax still runs its one cycle
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=contexts.ctx["batch16"])
    with pytest.raises(cpk.CpkError) as e:
        cpk.cpgmres(P["rhs"][:P["n"]], P["Q"], P["C"], M, dict(opts, itmax=-2))
    assert e.value.code == _lib.CPK_ERR_ARGS and c.expect["error"] in str(e.value)
    x, y, stats, flag = cpk.cpgmres(P["rhs"][:P["n"]], P["Q"], P["C"], M, dict(opts, itmax=0.5, restart=2))
    assert stats["niters"] == 2 and len(stats["residHistory"]) == 3
