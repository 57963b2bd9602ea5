"""CPU check behind tests/test_gpu_operator.py::test_from_torch_dense_product (no GPU).

A dense product sums each row of A in another order than the sparse product the oracle runs, and
nothing else differs.  A row sum of k terms taken in any order is the exact sum of the terms
perturbed by relative amounts of at most (k - 1) u, u = 2^-53 (the standard backward-error bound
of recursive summation), so the oracle -- its own recurrences, its own preconditioner -- is run on
A with every entry perturbed by a relative u x (its row's length) x U(-1, 1), a model at the
bound's size.  For the four symmetric methods it prints, over --seeds seeds, the largest deviation
of every history (relative to history[0]) and of x (relative to ||x||) from the unperturbed
oracle, beside the sensitivity band of tests/sensitivity.py and the parity rule's bound
max(1e-8, 10 x band), and whether the integers (niters, solved) moved.  The systems and right-hand
sides are the test's: cvxqp1_m through reg_cpkrylov, tiny65x63 at the method level on the column
of tests/test_gpu_solve_multi.py's TINY_COLUMNS (its band is not computed: the rule's floor).

  python tools/operator_dense_check.py [--seeds 4]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cpkrylov_amd as cpk  # noqa: E402
import fixtures as F  # noqa: E402
import structures as ST  # noqa: E402
from oracle import oracle as O  # noqa: E402
from sensitivity import band  # noqa: E402

U = 2.0 ** -53
OPTS = dict(F.EXPROG_OPTS)


def perturbed(A, rng):
    A = A.tocsr().copy()
    rowlen = np.repeat(np.diff(A.indptr), np.diff(A.indptr))
    A.data = A.data * (1.0 + U * rowlen * rng.uniform(-1.0, 1.0, A.nnz))
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=4)
    a = ap.parse_args()
    for name in ("cvxqp1_m", "tiny65x63"):
        P = F.load(name) if name == "cvxqp1_m" else ST.get(name)
        an = cpk.analyze(P["G"], P["B"], -P["C"])
        perm = an["perm"]
        Mo = O.LDL2(P["G"], P["B"], -P["C"], factors=(an["L"], an["D"], perm))
        Mo.set(**{k: float(OPTS[k]) for k in ("nitref", "itref_tol", "force_itref", "residual_update")})
        col = np.random.default_rng(1000 + 13).standard_normal(P["n"])  # TINY_COLUMNS["tiny65x63"]

        def method_level(method, Q):
            x, y, st = O.method(method, col.copy(), Q, P["C"], Mo, OPTS)
            return np.concatenate([x, y]), st

        for method in ("cg", "cglanczos", "minres", "symmlq"):
            if name == "cvxqp1_m":
                run = lambda Q: O.reg_cpkrylov(method, P["rhs"], Q, P["B"], P["C"], P["G"], OPTS, perm=perm)  # noqa: E731
            else:
                run = lambda Q: method_level(method, Q)  # noqa: E731
            x0, s0 = run(P["Q"])
            keys = [k for k in s0 if k.endswith("History")]
            h0 = s0[keys[0] if method != "symmlq" else "cgresidHistory"][0]
            dev = {k: 0.0 for k in keys}
            dev["x"] = 0.0
            same = True
            for seed in range(a.seeds):
                x1, s1 = run(perturbed(P["Q"], np.random.default_rng(100 + seed)))
                same = same and s1["niters"] == s0["niters"] and s1["solved"] == s0["solved"]
                for k in keys:
                    L = min(len(s0[k]), len(s1[k]))
                    dev[k] = max(dev[k], float(np.max(np.abs(s0[k][:L] - s1[k][:L])) / h0))
                dev["x"] = max(dev["x"], float(np.linalg.norm(x1 - x0) / np.linalg.norm(x0)))
            bd = band(name, method, {}, perm) if name == "cvxqp1_m" else None
            for k in dev:
                rule = max(1e-8, 10 * bd[k]) if bd else 1e-8
                print(f"{name:10s} {method:10s} {k:16s} deviation {dev[k]:.2e}  band {bd[k] if bd else float('nan'):.2e}  "
                      f"rule {rule:.2e}  inside {dev[k] <= rule}  integers equal {same}")


if __name__ == "__main__":
    main()
