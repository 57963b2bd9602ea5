"""Time and compare the float-compressed Krylov basis (engine option basis_f32) against the double
one (profiles/basis_f32_timing.json): one MI355X.

  s50       config 5 of bench.py (nonsym_system(N), cpdqgmres(40), `--itmax` iterations per call on the
            shifted right-hand side): it/s of both bases, the legs alternating within each of `--rounds`
            rounds after a warm-up call each, medians; then one profiled call per basis (engine option
            profile_passes, cpk_debug_pass_times) for the five pass times, each window pass as a
            fraction of 8 TB/s on its own byte model, and the ring bytes allocated.
            Byte models per iteration with windows of nv (dots, orthogonalisation) and nv' (direction)
            vectors, E the ring element size (8 or 4), VNEW / VCUR the float basis's double work vectors:
              dots        nv E N + 8N (ut) + 8N (w) + 8N (new vector written) + E m (old y-part read)
              orth        nv E N + 16N (new vector read and written) + 8N (ut)
              direction   nv' E N + E N (v_k) + 16N (xy) + E N (direction stored), and the new vector:
                          double 16N (read and written in its slot); float 8N (VNEW read) + 4N (slot) + 8N (VCUR)
  converge  cvxqp2_s (tests/golden), nonsym_system(20000) and the s50 system (first `--itmax` iterations),
            K.solve("dqgmres") with both bases: niters, solved, the largest deviation between the two
            histories relative to history[0], and the true relative residual |b - K x| / |b| of both.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before libcpk initialises HIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.synthetic import nonsym_system  # noqa: E402

PEAK = 8.0e12  # bytes/s
OPTS = dict(print=False, atol=1.0e-6, rtol=1.0e-6, itmax=500, residual_update=True, nitref=1, force_itref=True,
            itref_tol=1.0e-8)
MEM = 40


def pad64(N):
    return (N + 63) // 64 * 64


def build(ctx, S):
    A, B, Cm, G = (cpk.Matrix(S[k], ctx) for k in ("Q", "B", "C", "G"))
    M = cpk.opLDL2(G, B, -S["C"], ctx=ctx)
    M.nitref, M.itref_tol = OPTS["nitref"], OPTS["itref_tol"]
    M.residual_update, M.force_itref = OPTS["residual_update"], OPTS["force_itref"]
    return A, B, Cm, M


def pass_model(E, N, m, its, wd, wr):
    new = 16.0 * N if E == 8 else 20.0 * N
    return {"dots": wd * E * N + (24.0 * N + E * m) * its, "orth": wd * E * N + 24.0 * N * its,
            "direction": wr * E * N + (2.0 * E * N + 16.0 * N + new) * its}


def s50(ctx, S, A, B, Cm, M, itmax, rounds, steps):
    n, m, N = S["n"], S["m"], S["N"]
    b = torch.from_numpy(np.ascontiguousarray(S["rhs"])).cuda()
    b1 = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    xy0, xy = torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    shifted = C.c_int()
    _lib.check(_lib.lib.cpk_reg_shift_device(ctx.h, C.c_void_p(b.data_ptr()), A.h, B.h, Cm.h, M.h,
                                             C.c_void_p(b1.data_ptr()), C.c_void_p(xy0.data_ptr()), C.byref(shifted)))
    opts = _lib.make_opts(dict(OPTS, mem=MEM, itmax=itmax))
    hist = np.zeros(itmax + 64)
    st = _lib.Stats()
    st.hist, st.hist_cap = hist.ctypes.data_as(C.POINTER(C.c_double)), itmax + 64

    def step(f32):
        ctx.set_option("basis_f32", f32)
        _lib.check(_lib.lib.cpk_method_solve_device(ctx.h, _lib.METHODS["dqgmres"], C.c_void_p(b1.data_ptr()), A.h, Cm.h,
                                                    M.h, C.byref(opts), C.c_void_p(xy.data_ptr()), C.byref(st)))
        return int(st.niters)

    legs = {"f64": 0, "f32": 1}
    out = {k: {"its_per_s": [], "loop_ms_per_it": []} for k in legs}
    hists = {}
    for k, f in legs.items():  # warm-up: workspace, graphs
        step(f)
        hists[k] = hist[:st.hist_len].copy()
    for _ in range(rounds):
        for k, f in legs.items():  # the legs alternate within a round
            ctx.synchronize()
            t0, its, loop = time.perf_counter(), 0, 0.0
            for _ in range(steps):
                its += step(f)
                loop += st.loop_ms
            ctx.synchronize()
            out[k]["its_per_s"].append(its / (time.perf_counter() - t0))
            out[k]["loop_ms_per_it"].append(loop / its)
    for k, f in legs.items():
        E = 4 if f else 8
        ctx.set_option("profile_passes", 1)
        try:
            step(f)
            v = (C.c_double * 8)()
            _lib.check(_lib.lib.cpk_debug_pass_times(ctx.h, v))
        finally:
            ctx.set_option("profile_passes", 0)
        its, ms, wd, wr = v[0], list(v)[1:6], v[6], v[7]
        model = pass_model(E, N, m, its, wd, wr)
        names = ("krylov_spmv", "mz", "dots", "orth", "direction")
        passes = {nm: {"ms_per_iter": ms[i] / its} for i, nm in enumerate(names)}
        for nm in ("dots", "orth", "direction"):
            passes[nm]["bytes_per_iter"] = model[nm] / its
            passes[nm]["fraction_of_8TBs"] = model[nm] / (ms[names.index(nm)] * 1e-3) / PEAK
        ld = pad64(N) if f else N
        out[k].update(median_its_per_s=statistics.median(out[k]["its_per_s"]),
                      median_loop_ms_per_it=statistics.median(out[k]["loop_ms_per_it"]), passes=passes,
                      profiled_iterations=int(its), mean_window=wd / its, iteration_ms_eager=sum(ms) / its,
                      ring_bytes=2 * (MEM + 1) * ld * E + (2 * ld * 8 if f else 0), niters_per_call=len(hists[k]) - 1)
    L = min(len(hists["f64"]), len(hists["f32"]))
    out["history_deviation"] = float(np.max(np.abs(hists["f64"][:L] - hists["f32"][:L])) / hists["f64"][0])
    out["speedup_f32_over_f64"] = out["f32"]["median_its_per_s"] / out["f64"]["median_its_per_s"]
    ctx.set_option("basis_f32", 0)
    return out


def converge(ctx, label, S, itmax, handles=None):
    A, B, Cm, M = handles or build(ctx, S)
    K = cpk.KKT(A, B, Cm)
    b = np.ascontiguousarray(S["rhs"], dtype=np.float64)
    res = {"system": label, "N": int(S["n"] + S["m"]), "itmax": itmax}
    hs = {}
    for k, f in (("f64", 0), ("f32", 1)):
        with cpk.engine_options(ctx, basis_f32=f):
            try:
                x, stats, flag = K.solve("dqgmres", b, M, dict(OPTS, mem=MEM, itmax=itmax))
            except cpk.CpkError as e:
                res[k] = {"error": str(e)}
                continue
        tr = stats["true_resid"]
        hs[k] = stats["residHistory"]
        res[k] = {"niters": stats["niters"], "solved": flag["solved"], "true_rel_resid": tr["rnorm"] / tr["bnorm"],
                  "last_resid_over_first": float(hs[k][-1] / hs[k][0])}
    if len(hs) == 2:
        L = min(len(hs["f64"]), len(hs["f32"]))
        res["history_deviation"] = float(np.max(np.abs(hs["f64"][:L] - hs["f32"][:L])) / hs["f64"][0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=50_000_000, help="dofs of the S50 system; 0 to skip it")
    ap.add_argument("--itmax", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2, help="calls per leg and round")
    ap.add_argument("--skip-converge", action="store_true", help="the s50 timing alone")
    a = ap.parse_args()
    ctx = cpk.default_context()
    out = dict(tool="basis_f32_timing", device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK, mem=MEM,
               expectation="from the byte model alone, not a requirement: at the full window of 40 vectors the dots and "
                           "the orthogonalisation move (40*4 + 24) N = 184 N bytes instead of (40*8 + 24) N = 344 N "
                           "(1.87x fewer), the direction pass 204 N instead of 368 N (1.80x fewer); at the double "
                           "path's fractions of peak the three passes would take ~4.8 ms of their ~8.8 ms and the "
                           "iteration ~8.6 ms of its ~12.6 ms: ~115 it/s against 83-84")
    conv = []
    if not a.skip_converge:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import fixtures as F
        conv.append(converge(ctx, "cvxqp2_s", F.load("cvxqp2_s"), 500))
        conv.append(converge(ctx, "nonsym_system(N=20000)", nonsym_system(N=20000), 500))
    if a.size:
        S = nonsym_system(N=a.size)
        h = build(ctx, S)
        # the float basis may stop with the reference's error (a negative squared norm) before itmax:
        # that is recorded, and both bases are then timed over the iterations before it
        itmax, stopped = a.itmax, None
        try:
            res = s50(ctx, S, *h, itmax, a.rounds, a.steps)
        except cpk.CpkError as e:
            if e.code != _lib.CPK_ERR_INDEFINITE:
                raise
            import re
            stopped = str(e)
            itmax = max(int(re.search(r"Iter (\d+)", stopped).group(1)) * 3 // 4, 1)
            ctx.set_option("profile_passes", 0)
            res = s50(ctx, S, *h, itmax, a.rounds, a.steps)
        out["s50"] = dict(system=f"nonsym_system(N={a.size})", n=S["n"], m=S["m"], itmax_asked=a.itmax,
                          float_basis_stopped_with=stopped, itmax=itmax, rounds=a.rounds, steps=a.steps, **res)
        if not a.skip_converge:
            conv.append(converge(ctx, f"nonsym_system(N={a.size}), first {a.itmax} iterations", S, a.itmax, h))
    out["converge"] = conv
    print(json.dumps(out))


if __name__ == "__main__":
    main()
