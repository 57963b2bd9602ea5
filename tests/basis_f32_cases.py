"""The systems, windows and options that the compressed-basis tests share (test_arnoldi_f32_ref_host.py
on the CPU, test_gpu_basis_f32_solve.py on the device), so that what the CPU test pins is what the
GPU test uses.

  systems   the tiny members (structures.py) with a seeded random right-hand side (a member's own
            rhs(1:n) without reg_cpkrylov's shift can give a rounding-sized negative squared
            residual, where the reference stops with its error: test_gpu_solve_multi.py), and
            cvxqp2_s with its rhs(1:n);
  windows   cpdqgmres with mem = 5 (the ring wraps within the run) and mem = 40, cpgmres with
            restart = 20 (several cycles) and restart = 100;
  options   the example's (fixtures.EXPROG_OPTS) with itmax = 200: cvxqp2_s without reg_cpkrylov's
            shift runs long enough for the cycles and the wraps (a count the CPU test asserts), and
            cpdqgmres(5) does not converge on it at all -- with the float basis its squared norm
            H(k+1,k)^2 turns negative at iteration 269, the reference's error, which
            test_gpu_basis_f32_solve.py checks on its own (ERROR_CASE).

The right-hand sides of the tiny members are the first seeds at which every solve here ends without
that error.  With the float basis most do not: on these members the preconditioned residual
collapses in one step, H(k+1,k)^2 is then rounding noise of the basis, 2^-24 instead of 2^-53, and
its sign is arbitrary (DESIGN.md "Compressed basis": 97-100 of 100 right-hand sides stop with the
error, against 6-20 with the double basis).  tiny1x1 and tiny2x1 are used with the double basis only.

A plain module (not a conftest); test infrastructure only."""
import functools

import numpy as np

import arnoldi_f32_ref as RF
import fixtures as F
import structures as ST
from oracle import oracle as O

TINY = ("tiny1x1", "tiny2x1", "tiny3x2", "tiny65x63")
SYSTEMS = TINY + ("cvxqp2_s",)
GPU_SYSTEMS = ("tiny3x2", "tiny65x63", "cvxqp2_s")
WINDOWS = (("dqgmres", 5), ("dqgmres", 40), ("gmres", 20), ("gmres", 100))
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
TOL = F.EXPROG_OPTS["atol"]
ITMAX = 200
RHS_SEED = {"tiny1x1": 7, "tiny2x1": 1, "tiny3x2": 99, "tiny65x63": 18}
ERROR_CASE = ("cvxqp2_s", "dqgmres", 5, 300, 269)  # (system, method, window, itmax, the iteration of err = 4)
# default mode: (system, method, window) whose iteration count does not move under 1e-15
# perturbations of the rhs (test_arnoldi_f32_ref_host.py keeps checking it on the CPU)
DEFAULT_CASES = (("cvxqp2_s", "dqgmres", 40), ("cvxqp2_s", "gmres", 20), ("tiny65x63", "dqgmres", 5),
                 ("tiny65x63", "gmres", 100))
FLOOR = 1e-8  # tests/test_gpu_parity.py
SAFETY = 10.0


@functools.lru_cache(maxsize=None)
def _system(name):
    if name in TINY:
        S = ST.get(name)
        b = np.random.default_rng(RHS_SEED[name]).standard_normal(S["n"])
    else:
        S = F.load(name)
        b = S["rhs"][:S["n"]].copy()
    S = dict(S)
    S["N"] = S["n"] + S["m"]
    return S, b


def system(name):
    S, b = _system(name)
    return S, b.copy()


def opts(method, window, **extra):
    o = dict(F.EXPROG_OPTS, atol=TOL, rtol=TOL, itmax=ITMAX)
    o["mem" if method == "dqgmres" else "restart"] = window
    o.update(extra)
    return o


def oracle_M(S, factors=None):
    """the oracle's opLDL2 with the example's properties: its own factorization, or the product's
    exported factors (then M*z is the product's bit for bit, test_gpu_solve_multi.py)"""
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=factors)
    Mo.set(**{k: float(F.EXPROG_OPTS[k]) for k in PC_PROPS})
    return Mo


def ref_system(S, Mo, rational=False, itmax=ITMAX):
    return RF.System(S["Q"], S["C"], Mo, TOL, TOL, itmax, rational=rational)


_BANDS = {}


def band(name, method, window, factors=None, trials=4, eps=1e-15):
    """tests/sensitivity.py for the compressed solve: the reference's own spread (history relative to
    history[0], [x; y] relative to its norm) under relative perturbations of 1e-15 of the rhs, whether
    niters moved, and the unperturbed result"""
    key = (name, method, window, factors is not None)
    if key in _BANDS:
        return _BANDS[key]
    S, b = system(name)
    Sy = ref_system(S, oracle_M(S, factors))
    x1, y1, s1 = RF.solve(method, Sy, b, window, rd=RF.f32)
    out = {"hist": 0.0, "x": 0.0, "stable": True, "ref": (x1, y1, s1), "niters": [s1["niters"]]}
    rng = np.random.default_rng(12345)
    z1 = np.concatenate([x1, y1])
    for _ in range(trials):
        x2, y2, s2 = RF.solve(method, Sy, b * (1 + eps * rng.standard_normal(b.shape[0])), window, rd=RF.f32)
        h1, h2 = s1["residHistory"], s2["residHistory"]
        out["stable"] = out["stable"] and s1["niters"] == s2["niters"]
        out["niters"].append(s2["niters"])
        L = min(len(h1), len(h2))
        out["hist"] = max(out["hist"], float(np.max(np.abs(h1[:L] - h2[:L])) / h1[0]))
        out["x"] = max(out["x"], float(np.linalg.norm(z1 - np.concatenate([x2, y2])) / np.linalg.norm(z1)))
    _BANDS[key] = out
    return out
