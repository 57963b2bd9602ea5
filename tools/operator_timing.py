"""Time the operator-valued A (cpk_op) against the matrix path it stands beside.

Systems: synthetic.saddle_system at --mid dofs (default 10^6) and the benchmark's S10 system with
the +-4 B window.  Methods: cpminres and cpcg with the example options, atol = rtol = 0 and
itmax = --itmax (default 12), so every leg runs the same iterations (equal_work below: every leg
returned status 0 and ran exactly itmax iterations).  After a warm-up of every leg (which also
captures the graphs), --rounds (default 5) alternating rounds of
  (a) the matrix path with engine option no_minres_fuse (the sequence an operator solve runs)
  (b) the matrix path by default (cpminres with the fused update), for context
  (c) a capturable operator whose callback is cpk_mat_spmv_device on a handle of the same A
  (d) the same operator, eager (one Python callback and one state read-back per iteration)
each round timed between stream synchronisations, through the device entries on fixed device
vectors (cpk_method_solve_device / cpk_method_solve_op_device), so the cached solvers are reused.
Prints one JSON line: per system and method the median and [min, max] of every leg (ms per solve and
per iteration), the ratios (c)/(a) and (d)/(a), and the byte model's prediction for (c)/(a): the
operator path moves 24 n more bytes per product (the copy of the Krylov vector to the callback's
input, the read of its output) plus what the callback moves -- here the SpMV of A alone,
12 nnz(A) + 4 (n + 1) + 16 n, where the matrix path streams A inside blkdiag(A, C); the prediction
is (stats.bytes_moved of (c) + the callback's bytes) / stats.bytes_moved of (a).

  python tools/operator_timing.py [--mid N] [--size N] [--rounds R] [--itmax I] > profiles/operator_timing.json
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

OPTS = dict(print=False, atol=0.0, rtol=0.0, residual_update=True, nitref=1, force_itref=True, itref_tol=1.0e-8)
LEGS = ("a_matrix_unfused", "b_matrix_default", "c_operator_capturable", "d_operator_eager")


def window(ctx, fn):
    ctx.synchronize()
    t = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t) * 1e3


def spmv_operator(A, ctx, capturable):
    def fn(x, y, n, stream):
        return _lib.lib.cpk_mat_spmv_device(A.h, x, y)
    return cpk.Operator(A.shape[0], fn, ctx=ctx, capturable=capturable)


def measure(ctx, name, S, rounds, itmax, methods):
    M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
    M._set(nitref=1, force_itref=True, itref_tol=1e-8, residual_update=True)
    A, Cm = _as_matrix(S["Q"], ctx), _as_matrix(S["C"], ctx)
    n, N = S["n"], M.info["N"]
    g = torch.Generator(device="cuda").manual_seed(7)
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    X = torch.zeros(4 * N, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib.cpk_mat_spmv_device(A.h, C.c_void_p(b.data_ptr()), C.c_void_p(y.data_ptr())))  # the device copy
    ops = {True: spmv_operator(A, ctx, True), False: spmv_operator(A, ctx, False)}
    o = _lib.make_opts(dict(OPTS, itmax=itmax))
    pb = C.c_void_p(b.data_ptr())
    px = [C.c_void_p(X.data_ptr() + 8 * N * j) for j in range(4)]
    cb_bytes = 12.0 * S["Q"].nnz + 4.0 * (n + 1) + 16.0 * n
    out = dict(system=name, N=N, n=n, nnz_A=int(S["Q"].nnz), nnz_C=int(S["C"].nnz), nnz_l=M.info["nnz_l"],
               callback_bytes_per_product=cb_bytes, extra_bytes_per_product=24.0 * n, methods=[])
    for method in methods:
        mid = _lib.METHODS[method]
        st = {k: _lib.Stats() for k in LEGS}
        rc = {}

        def matrix(leg, j, unfused):
            def run():
                ctx.set_option("no_minres_fuse", unfused)
                rc[leg] = _lib.lib.cpk_method_solve_device(ctx.h, mid, pb, A.h, Cm.h, M.h, C.byref(o), px[j], C.byref(st[leg]))
                ctx.set_option("no_minres_fuse", False)
            return run

        def operator(leg, j, capturable):
            def run():
                rc[leg] = _lib.lib.cpk_method_solve_op_device(ctx.h, mid, pb, ops[capturable].h, Cm.h, M.h, C.byref(o),
                                                              px[j], C.byref(st[leg]))
            return run

        legs = dict(zip(LEGS, (matrix(LEGS[0], 0, True), matrix(LEGS[1], 1, False), operator(LEGS[2], 2, True),
                               operator(LEGS[3], 3, False))))
        for f in legs.values():  # warm-up of every leg (and the capture of its graphs)
            f()
        ctx.synchronize()
        times = {k: [] for k in LEGS}
        for _ in range(rounds):  # alternating, so a drift of the machine hits every leg
            for k, f in legs.items():
                times[k].append(window(ctx, f))
        equal = all(rc[k] == 0 and int(st[k].niters) == itmax for k in LEGS)
        med = {k: statistics.median(v) for k, v in times.items()}
        row = dict(method=method, rounds=rounds, equal_work=equal, status={k: rc[k] for k in LEGS},
                   niters={k: int(st[k].niters) for k in LEGS},
                   bytes_moved={k: st[k].bytes_moved for k in LEGS},
                   device_loop_ms={k: round(st[k].loop_ms, 3) for k in LEGS},
                   ms={k: round(med[k], 3) for k in LEGS},
                   ms_range={k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
                   ms_per_iteration={k: round(med[k] / itmax, 4) for k in LEGS} if equal else None,
                   ratio_c_over_a=round(med[LEGS[2]] / med[LEGS[0]], 3), ratio_d_over_a=round(med[LEGS[3]] / med[LEGS[0]], 3),
                   ratio_a_over_b=round(med[LEGS[0]] / med[LEGS[1]], 3),
                   model_c_over_a=round((st[LEGS[2]].bytes_moved + itmax * cb_bytes) / st[LEGS[0]].bytes_moved, 3)
                   if st[LEGS[0]].bytes_moved else None,
                   operator_calls={("capturable" if k else "eager"): ops[k].info()["calls"] for k in ops})
        out["methods"].append(row)
        print(f"[operator_timing] {name}: {method}: " + ", ".join(f"{k[0]} {med[k]:.2f} ms" for k in LEGS) +
              f", equal work: {equal}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system (0: skip)")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system, +-4 window (0: skip)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--itmax", type=int, default=12, help="iterations every leg is asked to run")
    ap.add_argument("--methods", default="minres,cg")
    a = ap.parse_args()
    ctx = cpk.default_context()
    methods = a.methods.split(",")
    res = []
    if a.mid > 0:
        res.append(measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, a.itmax, methods))
    if a.size > 0:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4),
                           a.rounds, a.itmax, methods))
    print(json.dumps(dict(tool="tools/operator_timing.py", device=torch.cuda.get_device_name(0), itmax=a.itmax,
                          opts=dict(OPTS, itmax=a.itmax), systems=res)))


if __name__ == "__main__":
    main()
