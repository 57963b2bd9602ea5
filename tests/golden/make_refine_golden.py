"""The reference solution and the oracle's refinement figures for
tests/test_gpu_solve_refined.py::test_refinement_gain.

x* solves K x = b for cvxqp1_m's K = [A B'; B -C] and right-hand side AS THE DOUBLES THEY ARE, in
mpmath arithmetic at 60 digits: iterative refinement whose residuals b - K x are formed in mpmath on
K's stored entries and whose corrections come from a double-precision LU of K, until the mpmath
residual is below 1e-45 of b.  It is stored as the double-double (xstar_hi, xstar_lo).

The figures are measured with the CPU oracle alone (the product's factors from its host analysis,
exact inner products, cpminres; the example options, and the same with atol = 0): the forward
error of the cold solve, of three corrections on the exactly rounded residual
(resid_exact_ref.residual, with cpk_kkt_solve_refined's rule for dropping a trial) and of three
warm restarts on the plain entry-order residual (kkt_ref.residual).  They are printed and recorded
beside x*; tests/test_gpu_solve_refined.py quotes them.

  python tests/golden/make_refine_golden.py      # under a minute

Output: tests/golden/cvxqp1_m_refine.npz (data only).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpmath as mp  # noqa: E402
import scipy.linalg as sla  # noqa: E402

import cpkrylov_amd as cpk  # noqa: E402  (host-only analysis: no GPU is touched)
import fixtures as F  # noqa: E402
import kkt_ref as R  # noqa: E402
import resid_exact_ref as E  # noqa: E402
from oracle import oracle as O  # noqa: E402

NAME, METHOD, STEPS = "cvxqp1_m", "minres", 3
PC = ("nitref", "itref_tol", "force_itref", "residual_update")


def mp_solution(K, b):
    ptr, ind, val = K
    N = len(ptr) - 1
    mp.mp.dps = 60
    lu = sla.lu_factor(R.as_scipy(K).toarray())
    vm, bm = [mp.mpf(float(v)) for v in val], [mp.mpf(float(v)) for v in b]
    x = [mp.mpf(0)] * N
    bmax = max(abs(v) for v in bm)
    for it in range(40):
        r = [bm[i] - mp.fsum(vm[e] * x[ind[e]] for e in range(ptr[i], ptr[i + 1])) for i in range(N)]
        rel = max(abs(v) for v in r) / bmax
        print(f"  mpmath refinement {it}: max |b - K x| / max |b| = {mp.nstr(rel, 5)}", flush=True)
        if rel < mp.mpf(10) ** -45:
            break
        dx = sla.lu_solve(lu, np.array([float(v) for v in r]))
        x = [x[i] + mp.mpf(float(dx[i])) for i in range(N)]
    else:
        raise SystemExit("the mpmath refinement did not converge")
    hi = np.array([float(v) for v in x])
    lo = np.array([float(x[i] - mp.mpf(float(hi[i]))) for i in range(N)])
    return hi, lo


def err(x, hi, lo):
    return float(np.linalg.norm((x - hi) - lo) / np.linalg.norm(hi))


def main():
    P, K = R.system(NAME), R.operator(NAME)
    b = P["rhs"]
    hi, lo = mp_solution(K, b)
    # the product's own factors from its host analysis (no GPU): with them and exact inner products
    # the oracle runs the device's arithmetic operation for operation
    an = cpk.analyze(P["G"], P["B"], -P["C"])
    Mo = O.LDL2(P["G"], P["B"], -P["C"], factors=(an["L"], an["D"], np.ascontiguousarray(an["perm"], np.int32)))
    n = P["n"]
    out = dict(xstar_hi=hi, xstar_lo=lo, cond_est=np.linalg.cond(R.as_scipy(K).toarray()))

    def rr_of(r):
        return O.xdot(r[:n], r[:n]) + O.xdot(r[n:], r[n:])

    # "example": the example options; "atol0": the same with atol = 0, so that a driver call on a small
    # residual still iterates (with atol = 1e-6 the corrections' stop tests pass at once)
    for tag, opts in (("example", dict(F.EXPROG_OPTS)), ("atol0", dict(F.EXPROG_OPTS, atol=0.0))):
        Mo.set(**{k: float(opts[k]) for k in PC if k in opts})
        with O.exact():
            x_cold, _ = O.reg_solve(METHOD, b, P["A"], P["B"], P["C"], Mo, opts)
            # cpk_kkt_solve_refined's loop: a trial whose exactly rounded residual does not decrease is dropped
            x, trial, rr_prev, errs = np.zeros_like(b), x_cold, rr_of(b), []
            for j in range(1, STEPS + 1):
                r = E.residual(K, trial, b)
                rr = rr_of(r)
                print(f"  {tag} refined: sum r^2 of trial {j} = {rr:.6e} (before {rr_prev:.6e})")
                if not rr < rr_prev:
                    print("  that trial is dropped")
                    trial = None
                    break
                x, rr_prev = trial, rr
                errs.append(err(x, hi, lo))
                dx, _ = O.reg_solve(METHOD, r, P["A"], P["B"], P["C"], Mo, opts)
                trial = x + dx
            if trial is not None:
                x = trial
                errs.append(err(x, hi, lo))
            e_ref = err(x, hi, lo)
            # three warm restarts on the plain entry-order residual, each taken as it comes
            x, perrs = x_cold, []
            for j in range(STEPS):
                dx, _ = O.reg_solve(METHOD, R.residual(K, x, b), P["A"], P["B"], P["C"], Mo, opts)
                x = x + dx
                perrs.append(err(x, hi, lo))
        e_cold = err(x_cold, hi, lo)
        print(f"{tag}: forward errors: cold {e_cold:.6e}; refined {e_ref:.6e} (iterates {errs}); "
              f"plain warm restarts {perrs}")
        out.update({f"{tag}_err_cold": e_cold, f"{tag}_err_refined": e_ref, f"{tag}_err_refined_iterates": np.array(errs),
                    f"{tag}_err_plain": np.array(perrs)})
    np.savez(os.path.join(HERE, f"{NAME}_refine.npz"), **out)


if __name__ == "__main__":
    main()
