"""The stop-logic case table: where each method stops, and what it reports at that moment.

Every solver decides on the device when to stop; a batch of iterations is one captured graph, so
after the stop the rest of the batch has to be a no-op in every kernel, and each method has code
that runs once around the stop (cpminres's folded update, cpsymmlq's pre-step and CG-point
transfer, cpsymmlq.m:317-347, cpgmres's back-solve per cycle and its overrun of itmax,
cpgmres.m:148,203, cpdqgmres's mem = min(mem, itmax), cpdqgmres.m:125).  The cases put the stop
where that code is exposed: by itmax one before, at and one after the end of a batch of 16, at
iteration 0, after one or two iterations, by tolerance inside the first batch, at the end of a
GMRES cycle, with restart = 1 and mem = 1, with mem > itmax, and with a zero right-hand side.

A case is Case(system, method, extra, expect, rhs, group): the fixture (fixtures.load), the
method, the options on top of fixtures.EXPROG_OPTS, and what the oracle reports in exact mode with
its RCM ordering: niters, solved, hist_len (residHistory; cpsymmlq: cgresidHistory), and x ("shift":
the iterate reg_cpkrylov returns before any iteration, reg_cpkrylov.m:156; "zero": exactly zero),
or error (an argument error citing the reference line).  rhs is "fixture" or "zero"; group names
the family.  tests/test_stop_cases_host.py holds the oracle to this table without a device,
tests/test_gpu_stop_matrix.py the engine to the oracle.

A plain module (not a conftest); test infrastructure only."""
from collections import namedtuple

import numpy as np

import fixtures as F

Case = namedtuple("Case", "system method extra expect rhs group")

METHODS = ("cg", "cglanczos", "minres", "symmlq", "gmres", "dqgmres")
BATCH = 16  # the base batch size (solve_loop.hpp, SolveDriver::batch)
BIG, SMALL = "cvxqp1_m", "cvxqp2_s"  # N = 5500 and N = 725
GMRES_RESTART, DQGMRES_MEM = 5, 3  # unless a row says otherwise
STATUS_ITMAX = "maximum number of iterations attained"  # cpcglanczos.m's status strings
STATUS_RESID = "residual small compared to initial residual"
# the groups whose cases are run once more in the default (non-exact) mode
BAND_GROUPS = ("itmax", "zero_tol", "iter0", "zero_rhs")


def _base(method):
    return {"gmres": {"restart": GMRES_RESTART}, "dqgmres": {"mem": DQGMRES_MEM}}.get(method, {})


def _exp(niters, solved, **kw):
    return dict(niters=niters, solved=solved, hist_len=niters + 1, **kw)


def _overrun(itmax, restart):
    """cpgmres runs whole cycles: ceil(itmax/restart) of them when none converges (cpgmres.m:148,203)"""
    return -(-itmax // restart) * restart


def _build():
    out = []

    def add(system, method, extra, expect, rhs="fixture", group=""):
        out.append(Case(system, method, dict(_base(method), **extra), expect, rhs, group))

    for method in METHODS:
        # 1. stopped by itmax one before, at and one after the end of a batch
        for itmax in (0, 1, 2, 7, BATCH - 1, BATCH, BATCH + 1):
            if method == "gmres":
                if itmax == 0:
                    continue  # an argument error: ERROR_CASES
                add(BIG, method, {"itmax": itmax}, _exp(_overrun(itmax, GMRES_RESTART), False), group="itmax")
            else:
                add(BIG, method, {"itmax": itmax}, _exp(itmax, False), group="itmax")
        # 2. a zero tolerance: runs to itmax
        n23 = _overrun(23, GMRES_RESTART) if method == "gmres" else 23
        add(BIG, method, {"atol": 0.0, "rtol": 0.0, "itmax": 23}, _exp(n23, False), group="zero_tol")
        # 3. stop at iteration 0: x is the shift of reg_cpkrylov.m:156
        add(BIG, method, {"atol": 1e300, "rtol": 0.0}, _exp(0, True, x="shift"), group="iter0")
        add(BIG, method, {"atol": 0.0, "rtol": 1.0}, _exp(0, True, x="shift"), group="iter0")
        # 4. stop after one or two iterations
        early = {"minres": 1, "gmres": 1, "dqgmres": 1, "cg": 2, "cglanczos": 2, "symmlq": 2}[method]
        add(BIG, method, {"atol": 0.0, "rtol": 0.5}, _exp(early, True), group="early")
        # 5. a stop by tolerance inside the first batch (cpgmres: three iterations into its third
        # cycle, a back-solve with k < restart); the two GMRES values are the oracle's, as recorded
        tol = {"minres": 12, "cg": 13, "cglanczos": 13, "symmlq": 13, "gmres": 13, "dqgmres": 12}[method]
        add(BIG, method, {"atol": 1e-6, "rtol": 1e-2}, _exp(tol, True), group="tol")
        # 6. a zero right-hand side: nothing may be divided by the zero norm
        add(BIG, method, {}, _exp(0, True, x="zero"), rhs="zero", group="zero_rhs")

    # cpgmres: restart x itmax, the overrun and the niters formula (cpgmres.m:267)
    for system in (BIG, SMALL):
        for r in (1, 5, BATCH, BATCH + 1):
            for itmax in (1, BATCH - 1, BATCH, BATCH + 1, 60):
                e = _exp(_overrun(itmax, r), False)
                if system == BIG and itmax == 60 and r >= BATCH:
                    e = _exp(63, True)  # converges in its last cycle
                add(system, "gmres", {"restart": r, "itmax": itmax}, e, group="restart")
    # the default restart with itmax = 1: one whole cycle, 50 iterations past itmax and more than
    # three batches of 16 (the batch loop's guard has to count the cycle, not itmax)
    add(SMALL, "gmres", {"restart": 50, "itmax": 1}, _exp(50, False), group="overrun")
    # convergence exactly at the end of a cycle: no third cycle, both inner conditions at once
    add(BIG, "gmres", {"restart": 5, "atol": 0.0, "rtol": CYCLE_END_RTOL}, _exp(10, True), group="cycle_end")

    # cpdqgmres: mem x itmax; mem = 1000 > itmax takes min(mem, itmax), 16 and 17 wrap at a batch end
    for system in (BIG, SMALL):
        for mem in (1, 2, 3, BATCH, BATCH + 1, 1000):
            for itmax in (1, BATCH - 1, BATCH, BATCH + 1, 60):
                e = _exp(itmax, False)
                if system == BIG and itmax == 60 and mem >= 2:
                    e = _exp(54, True)
                add(system, "dqgmres", {"mem": mem, "itmax": itmax}, e, group="mem")
    return out


CYCLE_END_RTOL = 0.015  # between residHistory[10]/[0] = 0.01496 and residHistory[9]/[0] = 0.02059
CASES = _build()
# cpgmres with itmax < 1: the outer loop never runs and cpgmres.m:267 reads an undefined k
ERROR_CASES = [Case(BIG, "gmres", {"restart": GMRES_RESTART, "itmax": 0}, dict(error="cpgmres.m:267"), "fixture", "error")]


def case_id(c):
    opts = "-".join(f"{k}{v:g}" for k, v in sorted(c.extra.items())) or "default"
    return f"{c.group}-{c.system}-{c.method}-{opts}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def problem(c):
    """the fixture of a case, with its right-hand side"""
    P = F.load(c.system)
    if c.rhs == "zero":
        P["rhs"] = np.zeros_like(P["rhs"])
    return P


def options(c):
    return dict(F.EXPROG_OPTS, **c.extra)


def expected_status(c):
    """cpcglanczos's status (btol is not set, so never the backward-error stop)"""
    return STATUS_RESID if c.expect["solved"] else STATUS_ITMAX


def history(stats):
    return stats["residHistory"] if "residHistory" in stats else stats["cgresidHistory"]


PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")


def oracle_precond(O, P, opts, factors=None):
    """the oracle's M = opLDL2(G, B, -C) with the preconditioner fields of opts
    (reg_cpkrylov.m:131-148), on its own RCM factorization or on given factors"""
    Mo = O.LDL2(P["G"], P["B"], -P["C"], factors=factors)
    Mo.set(**{k: float(opts[k]) for k in PC_PROPS if k in opts})
    return Mo


def shift(P, Mo):
    """x as reg_cpkrylov returns it when the method makes no iteration: dx = dy = 0 around the shift
    xy0 = M * [0; b2] (reg_cpkrylov.m:154-156, 166-168), zero when b2 is"""
    n = P["n"]
    z = np.zeros(P["n"] + P["m"])
    z[n:] = P["rhs"][n:]
    return Mo @ z if np.any(z) else z
