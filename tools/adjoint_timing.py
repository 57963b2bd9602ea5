"""Time the adjoint solve's pieces (profiles/adjoint_timing.json): one MI355X, the 10^6-dof system
and S10 with the +-4 window, `--rounds` alternating rounds, medians with ranges.

  (a) the kernel alone: cpk_mat_sample_outer_device with k = 1 and k = 2 on A and on B against the
      same handle's cpk_mat_spmv_device in the same process and round, each enqueued `--reps` times
      between two synchronisations; the ratio to the SpMV and the achieved fraction of 8 TB/s on the
      byte model 4 nnz + 4 (nrows + 1) + 8 k (nrows + ncols) + 8 count (+ 4 nnz for a perm map); and
      the same on a handle with a perm map (B handed over column-compressed), whose store scatters;
  (b) one backward: K.adjoint on device tensors (the adjoint solve plus the three passes) against one
      forward K.solve with the same options, and the three passes alone.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import scipy.sparse as sp
import torch  # before libcpk initialises HIP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402
from ipm_sequence_timing import OPTS, canon, window  # noqa: E402

PEAK = 8.0e12  # bytes/s


def vp(t):
    return C.c_void_p(t.data_ptr())


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=list(v))


def measure(ctx, label, S, rounds, reps):
    S = {k: (canon(v) if sp.issparse(v) else v) for k, v in S.items()}
    n, m = S["n"], S["m"]
    N = n + m
    A, Bm, Cm, G, Cn = (cpk.Matrix(X, ctx=ctx) for X in (S["Q"], S["B"], S["C"], S["G"], -S["C"]))
    Bp = cpk.Matrix(S["B"], ctx=ctx, csc=True)  # values in column order: a perm map
    M = cpk.opLDL2(G, Bm, Cn, ctx=ctx)
    M._set(**{k: OPTS[k] for k in ("nitref", "itref_tol", "force_itref", "residual_update")})
    K = cpk.KKT(A, Bm, Cm)
    lib = _lib.lib
    rng = np.random.default_rng(3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    x, gx = dev(S["rhs"]), dev(rng.standard_normal(N))
    sol, lam = torch.zeros_like(x), torch.zeros_like(x)

    def timed(fn):
        fn()
        ms, _ = window(ctx, lambda: [fn() for _ in range(reps)])
        return ms / reps

    print(f"{label}: operators built", file=sys.stderr, flush=True)
    handles = {"A": (A, False), "B": (Bm, False), "B_perm_map": (Bp, True)}
    legs = {}
    for name, (H, perm) in handles.items():
        nr, nc = H.shape
        info = H.info()
        U, V = dev(rng.standard_normal((2, nr))), dev(rng.standard_normal((2, nc)))
        out, y = torch.zeros(info["entries"], dtype=torch.float64, device="cuda"), torch.zeros(nr, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        legs[name] = dict(H=H, U=U, V=V, out=out, y=y, nr=nr, nc=nc, nnz=info["nnz"], count=info["entries"], perm=perm,
                          spmv=[], k1=[], k2=[])
    for _ in range(rounds):
        for L in legs.values():
            H = L["H"]
            L["spmv"].append(timed(lambda: _lib.check(lib.cpk_mat_spmv_device(H.h, vp(L["V"]), vp(L["y"])))))
            for k in (1, 2):
                L[f"k{k}"].append(timed(lambda: _lib.check(lib.cpk_mat_sample_outer_device(
                    H.h, k, vp(L["U"]), L["nr"], vp(L["V"]), L["nc"], -1.0, vp(L["out"]), L["count"]))))
    kernel = {}
    for name, L in legs.items():
        rec = dict(nrows=L["nr"], ncols=L["nc"], nnz=L["nnz"], perm_map=L["perm"], spmv_ms=summary(L["spmv"]),
                   spmv_model_bytes=12.0 * L["nnz"] + 4.0 * (L["nr"] + 1) + 8.0 * (L["nr"] + L["nc"]))
        rec["spmv_round_spread"] = (max(L["spmv"]) - min(L["spmv"])) / statistics.median(L["spmv"])
        for k in (1, 2):
            model = 4.0 * L["nnz"] + 4.0 * (L["nr"] + 1) + 8.0 * k * (L["nr"] + L["nc"]) + 8.0 * L["count"] + \
                (4.0 * L["nnz"] if L["perm"] else 0.0)
            t = L[f"k{k}"]
            rec[f"k{k}"] = dict(ms=summary(t), model_bytes=model, fraction_of_8TBs=model / (statistics.median(t) * 1e-3) / PEAK,
                                ratio_to_spmv=statistics.median(t) / statistics.median(L["spmv"]),
                                ratio_per_round=[a / b for a, b in zip(t, L["spmv"])])
        kernel[name] = rec
    print(f"{label}: kernel legs done", file=sys.stderr, flush=True)
    # ---- (b) one backward against one forward -------------------------------------------------
    K.solve("minres", x, M, OPTS, out=sol)  # warm the cached solver and its graphs
    out = {"db": lam, "dA": legs["A"]["out"], "dB": legs["B"]["out"],
           "dC": torch.zeros(Cm.info()["entries"], dtype=torch.float64, device="cuda")}
    K.adjoint("minres", sol, gx, M, OPTS, out=out)
    LB = legs["B"]  # gB's two columns lie in two vectors (lam and x): timed on stand-in columns of B's shapes
    fwd, bwd, passes, its = [], [], [], []
    for _ in range(rounds):
        t, (_, sf, _) = window(ctx, lambda: K.solve("minres", x, M, OPTS, out=sol))
        fwd.append(t)
        t, r = window(ctx, lambda: K.adjoint("minres", sol, gx, M, OPTS, out=out))
        bwd.append(t)
        its.append((sf["niters"], r["stats"]["niters"]))

        def three():
            _lib.check(lib.cpk_mat_sample_outer_device(A.h, 1, vp(lam), N, vp(sol), N, -1.0, vp(out["dA"]), out["dA"].numel()))
            _lib.check(lib.cpk_mat_sample_outer_device(Bm.h, 2, vp(LB["U"]), LB["nr"], vp(LB["V"]), LB["nc"], -1.0, vp(out["dB"]),
                                                       out["dB"].numel()))
            _lib.check(lib.cpk_mat_sample_outer_device(Cm.h, 1, vp(lam[n:]), N, vp(sol[n:]), N, 1.0, vp(out["dC"]), out["dC"].numel()))

        passes.append(timed(three))
    med = statistics.median
    return dict(system=label, n=n, m=m, kernel=kernel,
                backward=dict(forward_solve_ms=summary(fwd), adjoint_ms=summary(bwd), three_passes_ms=summary(passes),
                              niters_forward_adjoint=its, passes_share_of_backward=med(passes) / med(bwd),
                              backward_over_forward=med(bwd) / med(fwd)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=32)
    a = ap.parse_args()
    ctx = cpk.default_context()
    res = [measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, a.reps)]
    if a.size:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4),
                           a.rounds, a.reps))
    note = ("times are wall time around calls enqueued between two synchronisations; the operand vectors of a leg stay in "
            "the last-level cache across repetitions, for the SpMV and the sampled pass alike; three_passes_ms uses stand-in "
            "columns of the right shapes for gB's second term (the pass's traffic does not depend on which vectors they are)")
    print(json.dumps(dict(tool="adjoint_timing", note=note, device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK,
                          systems=res)))


if __name__ == "__main__":
    main()
