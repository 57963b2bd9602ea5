"""Time cpk_pc_refactor with device values on three builds / settings, to price the factor report
(ldl_report_kernel: one pass over D after every numeric phase) and the pivot_min instantiations of
the row kernels (profiles/factor_report_timing.json).

  (a) a tree built from the parent commit (--parent-root: a checkout with its libcpk.so built);
  (b) this tree with pivot_min = 0 (the default: the parent's row kernels plus the report);
  (c) this tree with pivot_min = 1e-9 on data where no pivot is hit (the REG row kernels, E zeroed
      and read by the report).

Systems: S10 with the +-4 B window (saddle_system(N=10M, window=4)) and saddle_system(N=1M).  One
measurement = a process of its own (under its own time limit) that builds the system and the
preconditioner, warms up with two refactorizations, then times --reps refactorizations, each on
new device values of G (Matrix.set_values from a torch tensor, outside the timed window), wall time
between two context synchronisations around the refactor call alone.  The processes of the legs
alternate, --rounds rounds of (a), (b), (c), so a drift of the machine hits all of them.  Per
system and leg: the median and the [min, max] of all timed calls, and per process medians (the
round-to-round spread).  Acceptance is against the parent, never against the code under test:
`b_within_parent_spread` says whether leg (b)'s median is at most the highest of leg (a)'s process
medians (the strictest reading of "within the parent's own round-to-round spread"); the differences
of the medians and the parent's spread are printed beside it.  Prints one JSON line.

  python tools/factor_report_timing.py --parent-root DIR [--sizes 10000000,1000000] > profiles/factor_report_timing.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = (("a", "parent commit", None), ("b", "this tree, pivot_min=0", 0.0), ("c", "this tree, pivot_min=1e-9", 1e-9))


def leg(a):
    """One measuring process: prints one JSON line with the timed calls (ms)."""
    sys.path.insert(0, a.root)
    import numpy as np
    import torch  # before libcpk initialises HIP

    import cpkrylov_amd as cpk
    from cpkrylov_amd.synthetic import saddle_system

    ctx = cpk.default_context()
    if a.pivot_min is not None:
        ctx.set_option("pivot_min", a.pivot_min)
    S = saddle_system(N=a.size, window=4)
    G = S["G"].tocsr()
    hG, hB, hC = (cpk.Matrix(M, ctx=ctx) for M in (G, S["B"], -S["C"]))
    M = cpk.opLDL2(hG, hB, hC, ctx=ctx)
    g0 = torch.as_tensor(np.ascontiguousarray(G.data), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(11)
    times = []
    for it in range(2 + a.reps):  # G rescaled in (0.5, 2): positive, no pivot near zero
        v = (g0 * (0.5 + 1.5 * torch.rand(g0.numel(), dtype=torch.float64, device="cuda", generator=gen))).contiguous()
        hG.set_values(v)
        ctx.synchronize()
        t = time.perf_counter()
        M.refactor(hG, hB, hC)
        ctx.synchronize()
        if it >= 2:
            times.append((time.perf_counter() - t) * 1e3)
    out = dict(leg=a.leg, size=a.size, N=M.info["N"], nnz_l=M.info["nnz_l"], ms=[round(t, 4) for t in times])
    if hasattr(M, "factor_report"):
        r = M.factor_report()
        out["report"] = dict(n_perturbed=r["n_perturbed"], n_wrong=r["n_wrong"], pivot_min=r["pivot_min"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--sizes", default="10000000,1000000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per measuring process")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--pivot-min", type=float, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    systems = []
    for size in [int(s) for s in a.sizes.split(",") if s]:
        runs = {k: [] for k, _, _ in LEGS}
        info = {}
        for rnd in range(a.rounds):
            for k, _, pm in LEGS:
                if k == "a" and not a.parent_root:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", k, "--size", str(size), "--reps", str(a.reps),
                       "--root", a.parent_root if k == "a" else ROOT]
                if pm is not None:
                    cmd += ["--pivot-min", repr(pm)]
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    print(f"[factor_report_timing] size {size} leg {k} round {rnd}: time limit", file=sys.stderr, flush=True)
                    return 1  # a hung process: nothing more is started
                if p.returncode != 0:
                    print(f"[factor_report_timing] size {size} leg {k} round {rnd}: exit {p.returncode}\n{p.stderr[-2000:]}",
                          file=sys.stderr, flush=True)
                    return 1
                r = json.loads(p.stdout.strip().splitlines()[-1])
                runs[k].append(r["ms"])
                info = dict(N=r["N"], nnz_l=r["nnz_l"])
                if "report" in r:
                    info["report_" + k] = r["report"]
                print(f"[factor_report_timing] size {size} leg {k} round {rnd}: median {statistics.median(r['ms']):.3f} ms",
                      file=sys.stderr, flush=True)
        legs = {}
        for k, what, _ in LEGS:
            if not runs[k]:
                continue
            allms = [t for r in runs[k] for t in r]
            legs[k] = dict(what=what, median_ms=round(statistics.median(allms), 4),
                           range_ms=[round(min(allms), 4), round(max(allms), 4)],
                           process_medians_ms=[round(statistics.median(r), 4) for r in runs[k]], calls=len(allms))
        row = dict(size=size, **info, legs=legs)
        if "a" in legs and "b" in legs:
            pa = legs["a"]["process_medians_ms"]
            row["parent_round_to_round_spread_ms"] = round(max(pa) - min(pa), 4)
            row["b_minus_a_median_ms"] = round(legs["b"]["median_ms"] - legs["a"]["median_ms"], 4)
            row["b_within_parent_spread"] = bool(legs["b"]["median_ms"] <= max(pa))
        if "c" in legs and "b" in legs:
            row["c_minus_b_median_ms"] = round(legs["c"]["median_ms"] - legs["b"]["median_ms"], 4)
        systems.append(row)
    print(json.dumps(dict(tool="tools/factor_report_timing.py", rounds=a.rounds, reps=a.reps, systems=systems)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
