"""Time an interior-point outer iteration three ways (profiles/ipm_sequence_timing.json).

One outer iteration: new values of the same sparsity for A, C and G (reg_cpkrylov.m:131 rebuilds
opLDL2 once per outer iteration), a refactorization, one cpminres solve with the example options.

  (a) new `Matrix` objects per iteration -- the only way without cpk_mat_set_values; uses no new
      entry, so it also runs on a tree that lacks them (`--legs a`);
  (b) `Matrix.set_values` from host arrays;
  (c) `Matrix.set_values` from device tensors (torch).

Per phase, wall time around a context synchronisation: the value hand-over, the refactor call, the
solve.  The Krylov operator blkdiag(A, C) is built (a) or refreshed (b, c) lazily inside the first
solve after an update, so the solve is run twice on the same values: the first includes the
operator (and, in (a), the capture of new graphs), the second is the solve alone; their difference
is reported as the operator's share.  An iteration's total is hand-over + refactor + first solve.
A warm-up iteration per leg, then `--rounds` rounds with the legs
interleaved, every leg of a round on the same values.  Also the rate of the value kernel itself
against its byte model ("Value refresh"), from the wall time of the blocking
call.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch  # before libcpk initialises HIP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402

OPTS = dict(print=False, atol=1.0e-6, rtol=1.0e-6, itmax=500, residual_update=True, nitref=1, force_itref=True,
            itref_tol=1.0e-8)  # the example options (examples/cpk_exprog1.m:79-90)
HAVE = hasattr(cpk.Matrix, "set_values")


def window(ctx, fn):
    ctx.synchronize()
    t = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def canon(M):
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return M


def values(S, it):
    """iteration `it`'s values of (Q, C, G, -C), canonical CSR order: G rescaled in (0.5, 2), C by a
    constant, Q scaled symmetrically (D Q D, D in (0.9, 1.1): still symmetric positive definite)"""
    rng = np.random.default_rng(100 + it)
    Q, G, Cm = S["Q"], S["G"], S["C"]
    d = rng.uniform(0.9, 1.1, Q.shape[0])
    q = Q.data * d[np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))] * d[Q.indices]
    c = Cm.data * (1.0 + 0.1 * (it % 7))
    return dict(Q=q, C=c, G=G.data * rng.uniform(0.5, 2.0, G.nnz), Cn=-c)


class Leg:
    """one set of handles, one opLDL2, fixed device vectors"""

    def __init__(self, ctx, S, kind):
        self.ctx, self.S, self.kind = ctx, S, kind
        self.pat = {k: S[k] for k in ("Q", "C", "G")}
        self.pat["Cn"] = S["C"]
        self.h = {k: cpk.Matrix(M, ctx=ctx) for k, M in (("Q", S["Q"]), ("C", S["C"]), ("G", S["G"]), ("Cn", -S["C"]))}
        self.B = cpk.Matrix(S["B"], ctx=ctx)
        self.M = cpk.opLDL2(self.h["G"], self.B, self.h["Cn"], ctx=ctx)
        self.M._set(**{k: OPTS[k] for k in ("nitref", "itref_tol", "force_itref", "residual_update")})
        self.n, self.N = S["n"], self.M.info["N"]
        self.b = torch.from_numpy(S["rhs"][:self.n].copy()).cuda()
        self.xy = torch.zeros(self.N, dtype=torch.float64, device="cuda")
        self.o = _lib.make_opts(OPTS)
        torch.cuda.synchronize()

    def inst(self):
        return self.M.solver_info()["graph_instantiations"] if hasattr(self.M, "solver_info") else None

    def iteration(self, host, dev):
        ctx = self.ctx
        if self.kind == "a":
            def hand():
                for k in ("Q", "C", "G", "Cn"):
                    P = self.pat[k]
                    self.h[k] = cpk.Matrix(sp.csr_matrix((host[k], P.indices, P.indptr), shape=P.shape), ctx=ctx)
        elif self.kind == "b":
            def hand():
                for k in ("Q", "C", "G", "Cn"):
                    self.h[k].set_values(host[k])
        else:
            def hand():
                for k in ("Q", "C", "G", "Cn"):
                    self.h[k].set_values(dev[k])
        t_hand, _ = window(ctx, hand)
        t_ref, ptime = window(ctx, lambda: self.M.refactor(self.h["G"], self.B, self.h["Cn"]))
        i0 = self.inst()
        st = _lib.Stats()

        def solve():
            _lib.check(_lib.lib.cpk_method_solve_device(ctx.h, _lib.METHODS["minres"], C.c_void_p(self.b.data_ptr()),
                                                        self.h["Q"].h, self.h["C"].h, self.M.h, C.byref(self.o),
                                                        C.c_void_p(self.xy.data_ptr()), C.byref(st)))
        t_solve, _ = window(ctx, solve)  # builds or refreshes blkdiag(A, C) first
        i1 = self.inst()
        t_again, _ = window(ctx, solve)  # the solve alone
        return dict(handover_ms=t_hand, refactor_wall_ms=t_ref, refactor_ptime_ms=ptime * 1e3, solve_ms=t_solve,
                    solve_again_ms=t_again, operator_ms=t_solve - t_again, total_ms=t_hand + t_ref + t_solve,
                    niters=int(st.niters), loop_ms=st.loop_ms,
                    graphs_instantiated_in_solve=None if i0 is None else i1 - i0)


def kernel_rate(ctx, S, reps=10):
    """the value kernel alone: a CSC-created handle (a 32-bit permutation) and a CSR one (identity)"""
    out = []
    Q = S["Q"]
    for name, csc, bpe in (("permutation (CSC input)", True, 20.0), ("identity (sorted CSR input)", False, 16.0)):
        h = cpk.Matrix(Q, ctx=ctx, csc=csc)
        h @ np.zeros(Q.shape[1])  # the device copy
        v = torch.rand(Q.nnz, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        h.set_values(v)  # uploads the map
        ts = [window(ctx, lambda: h.set_values_device(v.data_ptr(), Q.nnz))[0] for _ in range(reps)]
        t = min(ts)
        out.append(dict(map=name, nnz=int(Q.nnz), model_bytes=bpe * Q.nnz, call_ms_min=round(t, 4),
                        call_ms_median=round(statistics.median(ts), 4), gbs_of_model_at_min=round(bpe * Q.nnz / (t * 1e-3) / 1e9, 1)))
    return out


def measure(ctx, name, S, rounds, legs):
    S = dict(S, Q=canon(S["Q"]), C=canon(S["C"]), G=canon(S["G"]), B=canon(S["B"]))
    print(f"[ipm_sequence_timing] {name}: building the legs", file=sys.stderr, flush=True)
    L = {k: Leg(ctx, S, k) for k in legs}
    rows = {k: [] for k in legs}
    for it in range(rounds + 1):  # iteration 0 warms every leg up (graph capture, the device maps)
        host = values(S, it)
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        torch.cuda.synchronize()
        for k in legs:
            r = L[k].iteration(host, dev)
            if it:
                rows[k].append(r)
    out = dict(system=name, N=int(S["n"] + S["m"]), nnz=dict(Q=int(S["Q"].nnz), C=int(S["C"].nnz), G=int(S["G"].nnz), B=int(S["B"].nnz)),
               rounds=rounds, legs={})
    for k in legs:
        med = {f: round(statistics.median(r[f] for r in rows[k]), 3) for f in rows[k][0] if f.endswith("_ms")}
        out["legs"][k] = dict(median=med, rounds=[{f: (round(v, 3) if isinstance(v, float) else v) for f, v in r.items()} for r in rows[k]])
    if "a" in legs:
        for k in legs:
            if k != "a":
                out["legs"][k]["beats_a_in_every_round"] = all(x["total_ms"] < y["total_ms"] for x, y in zip(rows[k], rows["a"]))
                out["legs"][k]["same_niters_as_a"] = all(x["niters"] == y["niters"] for x, y in zip(rows[k], rows["a"]))
    for k in legs:
        m = out["legs"][k]["median"]
        print(f"[ipm_sequence_timing] {name}: ({k}) hand-over {m['handover_ms']:.2f}, refactor {m['refactor_wall_ms']:.2f} "
              f"(ptime {m['refactor_ptime_ms']:.2f}), first solve {m['solve_ms']:.2f}, solve alone {m['solve_again_ms']:.2f}, "
              f"total {m['total_ms']:.2f} ms", file=sys.stderr, flush=True)
    if HAVE:
        out["value_kernel"] = kernel_rate(ctx, S)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system (0: skip)")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system, +-4 window (0: skip)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="abc" if HAVE else "a")
    ap.add_argument("--label", default="", help="recorded with the result (e.g. the commit the tree is at)")
    a = ap.parse_args()
    legs = [k for k in a.legs if k == "a" or HAVE]
    ctx = cpk.default_context()
    res = []
    if a.mid > 0:
        res.append(measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, legs))
    if a.size > 0:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4), a.rounds, legs))
    print(json.dumps(dict(tool="tools/ipm_sequence_timing.py", label=a.label, device=torch.cuda.get_device_name(0),
                          in_place_entries=HAVE, opts=OPTS, systems=res)))


if __name__ == "__main__":
    main()
