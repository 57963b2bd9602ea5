"""Time the saddle-point operator K = [A B'; B -C] (profiles/kkt_timing.json): one MI355X, the
10^6-dof system and S10 with the +-4 window.

  * single residual: device time of r = b - K z with its four sums (enqueued `--reps` times
    between two synchronisations), the achieved fraction of 8 TB/s on the byte model
    12 nnz(K) + 4 (N + 1) + 24 N, and beside it, in the same process and round, the refinement
    residual spmv_stream<EpiResidSched> on Kp (cpk_profile_kernels): the yardstick;
  * block: one call with k = 1, 2, 4, 7, 8, 16 columns on the panel path (forced) against k
    single-column calls, both legs rotating through a pool of 32 columns so that no repetition
    meets vectors left in the last-level cache: the routing crossover kKktPanelMinCols is the smallest k from which the
    panel wins in every round on both systems;
  * outer iteration (tools/ipm_sequence_timing.py's device-values leg): new values of A and C,
    then the added cost of the device check (the first K.residual after the update, which
    regathers K's values, and K.residual alone) against the host check (download x, scipy K @ x);
  * warm start: iterations of K.solve warm from the previous outer iteration's x against cold,
    over a sequence of value updates (reported, not judged).

Rounds alternate the legs.  Prints one JSON line."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402
from ipm_sequence_timing import OPTS, canon, values, window  # noqa: E402

PEAK = 8.0e12  # bytes/s
KS = (1, 2, 4, 7, 8, 16)
POOL = 32  # columns of the rotating pool (768 MB of vectors at 10^6 dofs: beyond the last-level cache)


def vp(t):
    return C.c_void_p(t.data_ptr())


def measure(ctx, label, S, rounds, reps, outer):
    S = {k: (canon(v) if sp.issparse(v) else v) for k, v in S.items()}
    n, m = S["n"], S["m"]
    N = n + m
    A, Bm, Cm, G, Cn = (cpk.Matrix(X, ctx=ctx) for X in (S["Q"], S["B"], S["C"], S["G"], -S["C"]))
    M = cpk.opLDL2(G, Bm, Cn, ctx=ctx)
    M._set(**{k: OPTS[k] for k in ("nitref", "itref_tol", "force_itref", "residual_update")})
    K = cpk.KKT(A, Bm, Cm)
    nnz = K.info()["nnz"]
    model = 12.0 * nnz + 4.0 * (N + 1) + 24.0 * N
    rng = np.random.default_rng(3)
    kmax = POOL  # the block legs rotate through a pool of columns, so no repetition meets warm vectors
    Z = torch.from_numpy(rng.standard_normal((kmax, N))).cuda()  # row j = column j of the N x k block
    Bt = torch.from_numpy(np.tile(S["rhs"], (kmax, 1))).cuda()
    Rt = torch.empty_like(Z)
    nr = torch.zeros(4 * kmax, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = _lib.lib

    def resid(k, j0=0):
        _lib.check(lib.cpk_kkt_residual_device(K.h, k, vp(Z[j0]), N, vp(Bt[j0]), N, vp(Rt[j0]), N, vp(nr[4 * j0:])))

    def timed(fn, count):
        fn()
        ms, _ = window(ctx, lambda: [fn() for _ in range(count)])
        return ms / count

    def rotated(fn, k, count):
        """fn(j0) on `count` successive groups of k columns of the pool (both legs walk the same groups)"""
        starts = [(i * k) % (POOL - k + 1) for i in range(count)]
        fn(starts[-1])
        ms, _ = window(ctx, lambda: [fn(j0) for j0 in starts])
        return ms / count

    single, yard, block = [], [], {k: [] for k in KS}
    for _ in range(rounds):
        single.append(timed(lambda: resid(1), reps))
        prof = _lib.Profile()
        _lib.check(lib.cpk_profile_kernels(ctx.h, A.h, Cm.h, M.h, reps, C.byref(prof)))
        yard.append((prof.resid_ms, prof.resid_bytes))
        for k in KS:  # the panel path forced against k single-column calls
            K.set_route("panel")
            one = rotated(lambda j0: resid(k, j0), k, max(reps // k, 8))
            K.set_route("loop")
            loop = rotated(lambda j0: [resid(1, j0 + j) for j in range(k)], k, max(reps // k, 8))
            block[k].append((one, loop))
        K.set_route("auto")
    med = statistics.median
    out = dict(system=label, n=n, m=m, nnz_K=nnz, model_bytes=model,
               single_ms=dict(median=med(single), min=min(single), max=max(single), rounds=single),
               single_fraction_of_8TBs=model / (med(single) * 1e-3) / PEAK,
               yardstick_resid_sched=dict(ms=[y[0] for y in yard], bytes=yard[0][1],
                                          fraction_of_8TBs=yard[0][1] / (med([y[0] for y in yard]) * 1e-3) / PEAK),
               block={str(k): dict(panel_ms=med([b[0] for b in block[k]]), singles_ms=med([b[1] for b in block[k]]),
                                   panel_wins_every_round=all(b[0] < b[1] for b in block[k])) for k in KS})
    # ---- the outer iteration's check, and the warm start ------------------------------------------
    b = Bt[0]
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    xc = torch.zeros_like(x)
    checks = []
    for it in range(outer):
        v = values(S, it)
        q, c, g, cn = (torch.from_numpy(np.ascontiguousarray(v[k])).cuda() for k in ("Q", "C", "G", "Cn"))
        t_set, _ = window(ctx, lambda: (A.set_values(q), Cm.set_values(c), G.set_values(g), Cn.set_values(cn)))
        t_ref, _ = window(ctx, lambda: M.refactor(G, Bm, Cn))
        t_cold, (_, sc, _) = window(ctx, lambda: K.solve("minres", b, M, OPTS, out=xc))
        rec = dict(hand_over_ms=t_set, refactor_ms=t_ref, cold_solve_ms=t_cold, cold_niters=sc["niters"],
                   cold_true_rel=sc["true_resid"]["rnorm"] / sc["true_resid"]["bnorm"])
        if it > 0:
            t_warm, (_, sw, fw) = window(ctx, lambda: K.solve("minres", b, M, OPTS, x0=x, out=x))
            rec.update(warm_solve_ms=t_warm, warm_niters=sw["niters"], warm_solved=fw["solved"],
                       warm_start_rel=sw["true_resid0"]["rnorm"] / sw["true_resid0"]["bnorm"],
                       warm_true_rel=sw["true_resid"]["rnorm"] / sw["true_resid"]["bnorm"])
        else:
            x.copy_(xc)
            torch.cuda.synchronize()
        t_dev, (_, nd) = window(ctx, lambda: K.residual(xc, b, want_r=False))
        t_dev2, _ = window(ctx, lambda: K.residual(xc, b, want_r=False))

        t_down, xh = window(ctx, lambda: xc.cpu().numpy())
        # the host's own copy of K on this iteration's values (its assembly is not counted: a host
        # checker would update values in place)
        Kv = sp.bmat([[sp.csr_matrix((v["Q"], S["Q"].indices, S["Q"].indptr), shape=S["Q"].shape), S["B"].T],
                      [S["B"], sp.csr_matrix((v["Cn"], S["C"].indices, S["C"].indptr), shape=S["C"].shape)]]).tocsr()
        t0 = time.perf_counter()
        rh = float(np.linalg.norm(S["rhs"] - Kv @ xh))
        t_mul = (time.perf_counter() - t0) * 1e3
        del Kv
        rec.update(device_check_first_ms=t_dev, device_check_ms=t_dev2, host_download_ms=t_down, host_product_ms=t_mul,
                   device_rnorm=nd["rnorm"], host_rnorm=rh)
        checks.append(rec)
    out["outer_iterations"] = checks
    out["host_check_minus_device_check_ms"] = med([c["host_download_ms"] + c["host_product_ms"] - c["device_check_first_ms"]
                                                   for c in checks])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--outer", type=int, default=3)
    a = ap.parse_args()
    ctx = cpk.default_context()
    res = [measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, a.reps, a.outer)]
    if a.size:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4),
                           a.rounds, a.reps, a.outer))
    note = ("the outer iteration is timed as one device-values leg plus the added costs of the device check and of "
            "the host check (download, scipy product; the host's assembly of K is not counted), not as three "
            "separate legs; single_ms is wall time around enqueued calls, the yardstick HIP-event time")
    print(json.dumps(dict(tool="kkt_timing", note=note, device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, systems=res)))


if __name__ == "__main__":
    main()
