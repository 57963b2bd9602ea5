"""Time the refined block apply Y = M*X (cpk_pc_apply_multi_device on its panel kernels,
multiapply.hip + multisweep.hip) against the loop of single-column applies it has to beat.

Two systems: a mid-sized synthetic.saddle_system and the benchmark's S10 system with the +-4 B
window, each built with the engine option apply_multi_panel (the panel kernels at every k; the
single-column apply does not read the option).  Two settings: nitref = 3 under force_itref, and
the default data-dependent one (nitref = 3, itref_tol = 1e-8).  For k in {1, 2, 4, 6, 7, 8, 64}, after a
warm-up of both, ROUNDS alternating rounds of
  (a) k calls of cpk_pc_apply_device                (the tuned single-column apply)
  (b) one cpk_pc_apply_multi_device with k columns  (ceil(k / 8) panels)
each round timing `reps` repetitions between stream synchronisations (reps chosen so that a round
lasts about a quarter of a second).  Prints one JSON line: per system, setting and k the median
and the [min, max] of the rounds' times per repetition (ms), the ratio (a)/(b) of the medians,
whether (b) beat (a) in every round, the step counts the block apply reported, whether its columns
equal the single-column ones bit for bit, and the effective GB/s of (b) against this byte model
(KP = 8 columns per panel, kc of them the user's, l = nnz(L), N rows):
  sweep, forward + backward:  the factor twice, 2 * 12 l, its row pointers 2 * 4 (N + 1), D 8 N,
                              perm twice 2 * 4 N, the sweep panel written and read 2 * 64 N
  first solve:                + X gathered 8 kc N + the solution panel written 64 N
  refinement solve:           + the residual panel read 64 N + the solution panel read and
                              written 2 * 64 N
  residual:                   Kp once, 12 nnz(Kp) + 4 (N + 1), X read 8 kc N, the solution panel
                              gathered 64 N, the residual panel written 64 N
  store:                      the solution panel read 64 N, Y written 8 kc N
A panel takes s refinement solves, s the largest step count among its columns (every step under
force_itref), and min(nitref, s + 1) residuals.  Break-even is the only threshold: the entry
routes a panel of kc columns to the panel kernels only where (b) is faster than (a) on both
systems (kApplyMultiMinCols in dev.hpp).

  python tools/apply_multi_timing.py [--mid N] [--size N] > profiles/apply_multi_timing.json
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
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402

KP = 8
KS = (1, 2, 4, 6, 7, 8, 64)  # 6 and 7: the break-even lies between 4 and 8
ROUNDS = 5
NITREF = 3


def model_bytes(N, nnz_l, nnz_kp, k, nit, nitref):
    """algorithmic HBM bytes of one block apply of k columns with the step counts nit"""
    sweep = 2 * 12.0 * nnz_l + 2 * 4.0 * (N + 1) + 8.0 * N + 2 * 4.0 * N + 2 * 64.0 * N
    total = 0.0
    for j0 in range(0, k, KP):
        kc = min(KP, k - j0)
        s = max(nit[j0:j0 + kc])
        first = sweep + 8.0 * kc * N + 64.0 * N
        refine = sweep + 64.0 * N + 2 * 64.0 * N
        resid = 12.0 * nnz_kp + 4.0 * (N + 1) + 8.0 * kc * N + 2 * 64.0 * N
        total += first + s * refine + min(nitref, s + 1) * resid + 64.0 * N + 8.0 * kc * N
    return total


def window(ctx, fn, reps):
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def measure(ctx, name, S):
    with cpk.engine_options(ctx, apply_multi_panel=1):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
    N, nnz_l, nnz_kp = M.info["N"], M.info["nnz_l"], M.info["nnz_kp"]
    kmax = max(KS)
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randn(kmax * N, dtype=torch.float64, device="cuda", generator=g)
    Ya = torch.zeros(kmax * N, dtype=torch.float64, device="cuda")
    Yb = torch.zeros(kmax * N, dtype=torch.float64, device="cuda")
    nit = torch.zeros(kmax, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    px, pa, pb, pn = X.data_ptr(), Ya.data_ptr(), Yb.data_ptr(), nit.data_ptr()
    out = dict(system=name, N=N, nnz_l=nnz_l, nnz_kp=nnz_kp, rounds=M.sweep_info()["rounds"], settings=[])
    for setting, force in (("nitref=3, force_itref", True), ("nitref=3, itref_tol=1e-8 (default)", False)):
        M.nitref, M.itref_tol, M.force_itref = NITREF, 1e-8, force
        rows = []
        for k in KS:
            def single():
                for j in range(k):
                    _lib.check(_lib.lib.cpk_pc_apply_device(M.h, C.c_void_p(px + 8 * N * j), C.c_void_p(pa + 8 * N * j)))

            def multi():
                _lib.check(_lib.lib.cpk_pc_apply_multi_device(M.h, k, C.c_void_p(px), N, C.c_void_p(pb), N, C.c_void_p(pn)))

            Ya.zero_(), Yb.zero_()
            single(), multi()  # warm-up of both
            ctx.synchronize()
            same = bool(torch.equal(Ya[:k * N], Yb[:k * N]))
            steps = nit[:k].cpu().tolist()
            reps = int(min(200, max(5, 0.25e3 / max(window(ctx, multi, 2), 1e-3))))
            ta, tb = [], []
            for _ in range(ROUNDS):  # alternating, so a drift of the machine hits both
                ta.append(window(ctx, single, reps))
                tb.append(window(ctx, multi, reps))
            a, b = statistics.median(ta), statistics.median(tb)
            by = model_bytes(N, nnz_l, nnz_kp, k, steps, NITREF)
            rows.append(dict(k=k, reps=reps, rounds=ROUNDS, single_ms=round(a, 4),
                             single_ms_range=[round(min(ta), 4), round(max(ta), 4)], multi_ms=round(b, 4),
                             multi_ms_range=[round(min(tb), 4), round(max(tb), 4)], ratio_single_over_multi=round(a / b, 3),
                             multi_faster_in_every_round=all(y < x for x, y in zip(ta, tb)),
                             steps=steps if k <= KP else dict(min=min(steps), max=max(steps)),
                             model_bytes=by, multi_gbs=round(by / (b * 1e-3) / 1e9, 1), columns_bit_equal=same))
            print(f"[apply_multi_timing] {name}: {setting}: k={k} single {a:.3f} ms, multi {b:.3f} ms", file=sys.stderr,
                  flush=True)
        out["settings"].append(dict(setting=setting, by_k=rows))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window)")
    a = ap.parse_args()
    ctx = cpk.default_context()
    res = [measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid)),
           measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4))]
    # the panel kernels win at k on both systems and both settings, in every round
    wins = {k: all(r["multi_faster_in_every_round"] for s in res for st in s["settings"] for r in st["by_k"] if r["k"] == k)
            for k in KS}
    line = dict(tool="tools/apply_multi_timing.py", device=torch.cuda.get_device_name(0), kp=KP, nitref=NITREF, systems=res,
                panel_wins_at_k=wins)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
