"""Time the lockstep block solve (cpk_method_solve_multi_device: one Krylov product and one panel
apply per iteration for a panel of 8 columns) against the k single-column solves it replaces.

Systems: a mid-sized synthetic.saddle_system, the benchmark's S10 system with the +-4 B window, and
a band_g-sized case of 2 000 dofs, where the launch count dominates.  Methods: cpminres and cpcg
with the example options, atol = rtol = 0 and itmax = --itmax (default 50), so that every column
runs the same number of iterations -- as long as no residual reaches rounding level before itmax
(see equal_work below; the committed profile uses --itmax 12 for that reason).  For k in
{1, 2, 4, 7, 8, 16}, after a warm-up of both legs (which also captures their iteration graphs),
--rounds (default 5) alternating rounds of
  (a) k calls of cpk_method_solve_device             (the single-column solver, fused cpminres)
  (b) one cpk_method_solve_multi_device of k columns (ceil(k / 8) panels)
each round timed between stream synchronisations.  Prints one JSON line: per system, method and k
the median and the [min, max] of the rounds (ms for the whole block), the ratio (a)/(b), whether
(b) beat (a) in every round, the columns' iteration counts and the distinct return codes of both
legs, and equal_work: every column of both legs ran exactly itmax iterations with status 0.  With
a zero tolerance a column whose residual has reached rounding level stops before itmax on the
reference's indefinite / complex-norm test (a squared quantity that is pure rounding comes out
negative; which iteration depends on the summation order, so the legs differ, and a single-column
solve that stops so reports no count: null below): rows with equal_work false compare legs that
did unequal work.  The times are also given per iteration: ms_per_iteration = time / itmax where
equal_work holds.
Leg (a) is what a caller of the single-column device entry pays: its solver cache holds four
solvers keyed by the vectors' addresses, so for k > 4 the calls evict each other and capture their
graphs again (its time is not linear in k; DESIGN.md discusses it).
Per system it also reports the panel product's device time for 1, 2, 4, 7 and 8 columns against
the single-column Krylov product measured in the same run (cpk_debug_spmm_time), each with its
model GB/s: 12 nnz + 4 (N + 1) bytes of the matrix once, 16 N per column of vectors.  The crossover
k (the smallest k from which (b) wins in every round on a system) is derived from the rows.

  python tools/solve_multi_timing.py [--mid N] [--size N] [--rounds R] [--itmax I] > profiles/solve_multi_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch  # before libcpk initialises HIP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.api import _as_matrix  # noqa: E402
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402

KS = (1, 2, 4, 7, 8, 16)
OPTS = dict(print=False, atol=0.0, rtol=0.0, residual_update=True, nitref=1, force_itref=True, itref_tol=1.0e-8)


def window(ctx, fn):
    ctx.synchronize()
    t = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t) * 1e3


def measure(ctx, name, S, rounds, itmax):
    M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
    M._set(nitref=1, force_itref=True, itref_tol=1e-8, residual_update=True)
    A, Cm = _as_matrix(S["Q"], ctx), _as_matrix(S["C"], ctx)
    n, N = S["n"], M.info["N"]
    nnz = S["Q"].nnz + S["C"].nnz
    kmax = max(KS)
    g = torch.Generator(device="cuda").manual_seed(7)
    B = torch.randn(kmax * n, dtype=torch.float64, device="cuda", generator=g)
    Xa = torch.zeros(kmax * N, dtype=torch.float64, device="cuda")
    Xb = torch.zeros(kmax * N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pb, pa, pm = B.data_ptr(), Xa.data_ptr(), Xb.data_ptr()
    o = _lib.make_opts(dict(OPTS, itmax=itmax))
    out = dict(system=name, N=N, n=n, nnz_krylov=nnz, nnz_l=M.info["nnz_l"], product=[], methods=[])
    for kc in (1, 2, 4, 7, 8):
        a, b = C.c_double(), C.c_double()
        _lib.check(_lib.lib.cpk_debug_spmm_time(ctx.h, A.h, Cm.h, M.h, kc, 20, C.byref(a), C.byref(b)))
        by_p, by_s = 12.0 * nnz + 4.0 * (N + 1) + kc * 16.0 * N, 12.0 * nnz + 4.0 * (N + 1) + 16.0 * N
        out["product"].append(dict(columns=kc, panel_ms=round(a.value, 4), single_ms=round(b.value, 4),
                                   panel_gbs=round(by_p / (a.value * 1e-3) / 1e9, 1),
                                   single_gbs=round(by_s / (b.value * 1e-3) / 1e9, 1),
                                   ratio_k_singles_over_panel=round(kc * b.value / a.value, 3)))
    for method in ("minres", "cg"):
        mid = _lib.METHODS[method]
        rows = []
        for k in KS:
            sts = (_lib.Stats * k)()
            status = (C.c_int * k)()
            st1 = _lib.Stats()
            codes, its_a = [], []

            def single():
                codes.clear(), its_a.clear()
                for j in range(k):
                    st1.niters = -1  # a solve that stops on the error test leaves it untouched
                    codes.append(_lib.lib.cpk_method_solve_device(ctx.h, mid, C.c_void_p(pb + 8 * n * j), A.h, Cm.h, M.h,
                                                                  C.byref(o), C.c_void_p(pa + 8 * N * j), C.byref(st1)))
                    its_a.append(int(st1.niters) if st1.niters >= 0 else None)

            def multi():
                return _lib.lib.cpk_method_solve_multi_device(ctx.h, mid, k, C.c_void_p(pb), n, A.h, Cm.h, M.h, C.byref(o),
                                                              C.c_void_p(pm), N, sts, status)

            single(), multi()  # warm-up of both (and the capture of their graphs)
            ctx.synchronize()
            its = [int(sts[j].niters) for j in range(k)]
            ta, tb = [], []
            for _ in range(rounds):  # alternating, so a drift of the machine hits both
                ta.append(window(ctx, single))
                tb.append(window(ctx, multi))
            a, b = statistics.median(ta), statistics.median(tb)
            known = [v for v in its_a if v is not None]
            equal = (not any(codes) and not any(status) and all(v == itmax for v in its_a) and all(v == itmax for v in its))
            rows.append(dict(k=k, rounds=rounds, single_ms=round(a, 3), single_range=[round(min(ta), 3), round(max(ta), 3)],
                             multi_ms=round(b, 3), multi_range=[round(min(tb), 3), round(max(tb), 3)],
                             ratio_single_over_multi=round(a / b, 3),
                             multi_faster_in_every_round=all(y < x for x, y in zip(ta, tb)), equal_work=equal,
                             single_niters=dict(min=min(known) if known else None, max=max(known) if known else None,
                                                unreported=len(its_a) - len(known)),
                             multi_niters=dict(min=min(its), max=max(its), sum=sum(its)),
                             single_ms_per_iteration=round(a / itmax, 4) if equal else None,
                             multi_ms_per_iteration=round(b / itmax, 4) if equal else None,
                             single_status=sorted(set(codes)), multi_column_status=sorted(set(status))))
            print(f"[solve_multi_timing] {name}: {method}: k={k} single {a:.2f} ms, multi {b:.2f} ms, "
                  f"equal work: {equal}", file=sys.stderr, flush=True)
        win = [r["k"] for r in rows if r["multi_faster_in_every_round"]]
        cross = next((k for k in KS if all(q in win for q in KS if q >= k)), None)
        out["methods"].append(dict(method=method, by_k=rows, crossover_k=cross))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window)")
    ap.add_argument("--small", type=int, default=2_000, help="dofs of the launch-bound case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--itmax", type=int, default=50, help="iterations every column is asked to run")
    a = ap.parse_args()
    ctx = cpk.default_context()
    res = []
    if a.small > 0:
        res.append(measure(ctx, f"saddle_system(N={a.small})", saddle_system(N=a.small), a.rounds, a.itmax))
    if a.mid > 0:
        res.append(measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, a.itmax))
    if a.size > 0:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4),
                           a.rounds, a.itmax))
    print(json.dumps(dict(tool="tools/solve_multi_timing.py", device=torch.cuda.get_device_name(0), itmax=a.itmax,
                          opts=dict(OPTS, itmax=a.itmax), systems=res)))


if __name__ == "__main__":
    main()
