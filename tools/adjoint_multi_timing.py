"""Time the block adjoint's pieces (profiles/adjoint_multi_timing.json): one MI355X, the 10^6-dof
system and S10 with the +-4 window, both legs of every comparison in one process, `--rounds`
alternating rounds, medians with ranges.

  (a) the sampler: the panel kernel (cpk_kkt_sample_multi_device forming one gradient: the transposing
      pass over X and Lam plus sample_panel_kernel) against the run-time-k kernel it replaces
      (cpk_mat_sample_outer_device fed the same k columns as a column-major block; for B the 2k columns
      [ly_0, xy_0, ...] x [xx_0, lx_0, ...], staged once outside the timed region), on A and on B at
      k = 8 and 16; the two legs' bits are compared once.  The expectation: at k = 8 on S10 +-4 the
      panel leg's median is not above the other leg's by more than that leg's own round-to-round
      spread.  The achieved fraction of 8 TB/s is on the byte model 4 nnz + 4 (nrows + 1) + 8 count
      + 64 ceil(k / 8) (rows + columns touched) for the panels (+ 16 N k read and 128 N ceil(k / 8)
      written by the transposing pass, which the entry runs once per call).
      Then what the entry's routing is decided by: all three gradients of one call on either route
      (`K.set_sample_route`; the run-time-k route stages gB's 2k columns inside the call) at
      k = 2 ... 24, and whether the panel route wins in every round.
  (b) one backward: K.adjoint_block of k = 8 on device tensors against eight K.adjoint calls that
      reuse one pair of buffers (so M's cached solver is found again), `--itmax` iterations per
      column in both legs, and the gradient passes' share of the block backward.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import scipy.sparse as sp
import torch  # before libcpk initialises HIP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402
from ipm_sequence_timing import OPTS, canon, window  # noqa: E402

PEAK = 8.0e12  # bytes/s
NULL = C.c_void_p(None)


def vp(t):
    return C.c_void_p(t.data_ptr())


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=list(v))


def measure(ctx, label, S, rounds, reps, itmax, expect):
    S = {k: (canon(v) if sp.issparse(v) else v) for k, v in S.items()}
    n, m = S["n"], S["m"]
    N = n + m
    A, Bm, Cm, G, Cn = (cpk.Matrix(X, ctx=ctx) for X in (S["Q"], S["B"], S["C"], S["G"], -S["C"]))
    M = cpk.opLDL2(G, Bm, Cn, ctx=ctx)
    M._set(**{k: OPTS[k] for k in ("nitref", "itref_tol", "force_itref", "residual_update")})
    K = cpk.KKT(A, Bm, Cm)
    lib = _lib.lib
    gen = torch.Generator(device="cuda").manual_seed(3)
    new = lambda *shape: torch.randn(*shape, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    print(f"{label}: operators built", file=sys.stderr, flush=True)

    def timed(fn):
        fn()
        ms, _ = window(ctx, lambda: [fn() for _ in range(reps)])
        return ms / reps

    legs = {}
    for k in (8, 16):
        X, L = new(k, N), new(k, N)  # (k, N) row-major: the N x k block, ld N
        for name, H in (("A", A), ("B", Bm)):
            info = H.info()
            nr, nc = H.shape
            out_new, out_old = (torch.zeros(info["entries"], dtype=torch.float64, device="cuda") for _ in range(2))
            if name == "A":
                U, V, kk, ldu, ldv = L, X, k, N, N  # lx = L[:, :n], xx = X[:, :n]: the blocks' own columns
                g = (vp(out_new), info["entries"], NULL, 0, NULL, 0)
            else:
                U, V = torch.empty(2 * k, m, dtype=torch.float64, device="cuda"), torch.empty(2 * k, n, dtype=torch.float64, device="cuda")
                U[0::2], U[1::2], V[0::2], V[1::2] = L[:, n:], X[:, n:], X[:, :n], L[:, :n]
                kk, ldu, ldv = 2 * k, m, n
                g = (NULL, 0, vp(out_new), info["entries"], NULL, 0)
            torch.cuda.synchronize()
            f_new = lambda X=X, L=L, g=g, k=k: _lib.check(lib.cpk_kkt_sample_multi_device(K.h, k, vp(X), N, vp(L), N, *g))  # noqa: E731
            f_old = lambda H=H, U=U, V=V, kk=kk, ldu=ldu, ldv=ldv, o=out_old, c=info["entries"]: _lib.check(  # noqa: E731
                lib.cpk_mat_sample_outer_device(H.h, kk, vp(U), ldu, vp(V), ldv, -1.0, vp(o), c))
            f_new(), f_old()
            ctx.synchronize()
            same = bool(torch.equal(out_new.view(torch.int64), out_old.view(torch.int64)))
            np_ = -(-k // 8)
            base = 4.0 * info["nnz"] + 4.0 * (nr + 1) + 8.0 * info["entries"]
            terms = 2 if name == "B" else 1
            legs[(name, k)] = dict(new=f_new, old=f_old, t_new=[], t_old=[], same_bits=same, keep=(X, L, U, V, out_new, out_old),
                                   model_panel=base + 64.0 * np_ * terms * (nr + nc), model_pack=16.0 * N * k + 128.0 * N * np_,
                                   model_outer=base + 8.0 * kk * (nr + nc), nnz=info["nnz"], nrows=nr, ncols=nc)
    K.set_sample_route("panel")
    for _ in range(rounds):
        for Lg in legs.values():
            Lg["t_old"].append(timed(Lg["old"]))
            Lg["t_new"].append(timed(Lg["new"]))
    med = statistics.median
    # the entry's own quantity: all three gradients of one call, on either route
    three = {}
    grads = [torch.zeros(H.info()["entries"], dtype=torch.float64, device="cuda") for H in (A, Bm, Cm)]
    gargs = [a for g in grads for a in (vp(g), g.numel())]
    X, L = new(24, N), new(24, N)
    for k in (2, 4, 6, 7, 8, 9, 12, 15, 16, 24):
        f = lambda k=k, X=X, L=L: _lib.check(lib.cpk_kkt_sample_multi_device(K.h, k, vp(X), N, vp(L), N, *gargs))  # noqa: E731
        t = {"panel": [], "outer": []}
        for _ in range(rounds):
            for route in ("outer", "panel"):
                K.set_sample_route(route)
                t[route].append(timed(f))
        three[f"k{k}"] = dict(panel_ms=summary(t["panel"]), outer_ms=summary(t["outer"]),
                              panel_over_outer=med(t["panel"]) / med(t["outer"]),
                              panel_wins_every_round=bool(all(p < o for p, o in zip(t["panel"], t["outer"]))))
    K.set_sample_route("auto")
    sampler = {}
    for (name, k), Lg in legs.items():
        tn, to = Lg["t_new"], Lg["t_old"]
        spread = max(to) - min(to)
        rec = dict(nrows=Lg["nrows"], ncols=Lg["ncols"], nnz=Lg["nnz"], same_bits=Lg["same_bits"], panel_ms=summary(tn),
                   run_time_k_ms=summary(to), run_time_k_round_spread_ms=spread, panel_over_run_time_k=med(tn) / med(to),
                   panel_not_slower_beyond_spread=bool(med(tn) <= med(to) + spread),
                   panel_model_bytes=Lg["model_panel"], pack_model_bytes=Lg["model_pack"], run_time_k_model_bytes=Lg["model_outer"],
                   panel_fraction_of_8TBs=(Lg["model_panel"] + Lg["model_pack"]) / (med(tn) * 1e-3) / PEAK,
                   run_time_k_fraction_of_8TBs=Lg["model_outer"] / (med(to) * 1e-3) / PEAK)
        sampler[f"{name}_k{k}"] = rec
    holds = None
    if expect:
        holds = all(sampler[f"{h}_k8"]["panel_not_slower_beyond_spread"] for h in "AB")
    print(f"{label}: sampler legs done", file=sys.stderr, flush=True)
    legs.clear()
    # ---- (b) one block backward against eight single-column ones ----------------------------------
    k = 8
    opts = dict(OPTS, itmax=itmax)
    Xb, GX, Lam = new(k, N), new(k, N), torch.zeros(k, N, dtype=torch.float64, device="cuda")
    out = {"db": Lam, "dA": torch.zeros(A.info()["entries"], dtype=torch.float64, device="cuda"),
           "dB": torch.zeros(Bm.info()["entries"], dtype=torch.float64, device="cuda"),
           "dC": torch.zeros(Cm.info()["entries"], dtype=torch.float64, device="cuda")}
    x1, g1 = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
    out1 = dict(out, db=torch.zeros(N, dtype=torch.float64, device="cuda"))

    def block():
        return K.adjoint_block("minres", Xb, GX, M, opts, out=out)

    def singles():
        its = []
        for j in range(k):
            x1.copy_(Xb[j]), g1.copy_(GX[j])
            its.append(K.adjoint("minres", x1, g1, M, opts, out=out1)["stats"]["niters"])
        return its

    def passes():
        _lib.check(lib.cpk_kkt_sample_multi_device(K.h, k, vp(Xb), N, vp(Lam), N, vp(out["dA"]), out["dA"].numel(),
                                                   vp(out["dB"]), out["dB"].numel(), vp(out["dC"]), out["dC"].numel()))

    block(), singles()
    tb, ts, tp, its = [], [], [], []
    for _ in range(rounds):
        t, r = window(ctx, block)
        tb.append(t)
        t, i1 = window(ctx, singles)
        ts.append(t)
        its.append(([s["niters"] for s in r["stats"]], i1))
        tp.append(timed(passes))
    backward = dict(k=k, itmax=itmax, adjoint_block_ms=summary(tb), eight_adjoints_ms=summary(ts), gradient_passes_ms=summary(tp),
                    niters_block_singles=its[-1], block_over_singles=med(tb) / med(ts),
                    passes_share_of_block_backward=med(tp) / med(tb))
    return dict(system=label, n=n, m=m, sampler=sampler, expectation_k8_holds=holds, three_gradients=three,
                sample_route=K.sample_route_info(), backward=backward)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system (0: skip)")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window; 0: skip)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--itmax", type=int, default=12)
    a = ap.parse_args()
    ctx = cpk.default_context()
    res = []
    if a.mid:
        res.append(measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, a.reps, a.itmax, False))
    if a.size:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4),
                           a.rounds, a.reps, a.itmax, True))
    note = ("times are wall time around calls enqueued between two synchronisations; cpk_kkt_sample_multi_device waits for "
            "its stream before it returns and the run-time-k leg does not, so the panel leg carries one synchronisation per "
            "call that the other leg does not; the panel leg includes the transposing pass over all of X and Lam although "
            "one gradient reads only part of the panels")
    print(json.dumps(dict(tool="adjoint_multi_timing", note=note, device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK,
                          systems=res)))


if __name__ == "__main__":
    main()
