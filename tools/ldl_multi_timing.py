"""Time the multi-column factor apply (cpk_pc_apply_ldl_multi_device, multisweep.hip) against the
single-column sweeps it has to beat.

Two systems: a mid-sized synthetic.saddle_system and the benchmark's S10 system with the +-4 B
window.  On each, after a warm-up and between stream synchronisations, REPS repetitions of
  (a) 8 calls of cpk_pc_apply_ldl_device           (the tuned single-column sweeps, 8 columns)
  (b) one cpk_pc_apply_ldl_multi_device, k = 8     (one panel)
  (c) one cpk_pc_apply_ldl_multi_device, k = 64    (eight panels)
Prints one JSON line: the times per repetition (ms), the ratio (a)/(b), and the effective GB/s
of (b) and (c) against the byte model of DESIGN.md section 5 (multi-column sweep) -- per panel of
KP = 8 columns the factor streamed once forward and once backward, 2 * 12 * nnz(L) bytes, plus
the vectors (X gathered and Y scattered, 2 * 8 * 8 N, with perm twice, 2 * 4 N), the panel
written forward and read backward (2 * 8 * 8 N), the row pointers and D -- beside the GB/s of (a)
against the single-column sweeps' model (section 5), which streams the factor once per column.
Break-even is the only threshold: (b) must be faster than (a) on both systems.

  python tools/ldl_multi_timing.py [--mid N] [--size N] [--reps R] > profiles/ldl_multi_timing.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # before libcpk initialises HIP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpkrylov_amd as cpk  # noqa: E402
from cpkrylov_amd import _lib  # noqa: E402
from cpkrylov_amd.synthetic import saddle_system  # noqa: E402

KP = 8


def panel_bytes(N, nnz_l):
    """algorithmic HBM bytes of one panel solve (forward + backward)"""
    factor = 2 * 12.0 * nnz_l + 2 * 4.0 * (N + 1) + 8.0 * N  # entries both ways, row pointers, D
    vectors = 2 * 8.0 * KP * N + 2 * 4.0 * N                 # X gathered, Y scattered, perm twice
    panel = 2 * 8.0 * KP * N                                 # W written forward, read backward
    return factor + vectors + panel


def single_bytes(N, nnz_l):
    """the single-column model of one LDL solve (Precond::apply_bytes, nitref = 0, int32 columns)"""
    fwd = 12.0 * nnz_l + 4.0 * (N + 1) + 16.0 * N + 4.0 * N
    return fwd + fwd + 16.0 * N  # backward: also D and the scatter


def timed(ctx, fn, reps):
    fn()
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def measure(ctx, name, S, reps):
    M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
    N, nnz_l = M.info["N"], M.info["nnz_l"]
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randn(64 * N, dtype=torch.float64, device="cuda", generator=g)
    Y = torch.zeros(64 * N, dtype=torch.float64, device="cuda")
    Y1 = torch.zeros(8 * N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    px, py, py1 = X.data_ptr(), Y.data_ptr(), Y1.data_ptr()

    def single8():
        for j in range(8):
            _lib.check(_lib.lib.cpk_pc_apply_ldl_device(M.h, C.c_void_p(px + 8 * N * j), C.c_void_p(py1 + 8 * N * j)))

    def multi(k):
        return lambda: _lib.check(_lib.lib.cpk_pc_apply_ldl_multi_device(M.h, k, C.c_void_p(px), N, C.c_void_p(py), N))

    a = timed(ctx, single8, reps)
    b = timed(ctx, multi(8), reps)
    same = bool(torch.equal(Y[:8 * N], Y1))  # the panel's columns equal the single-column ones, bit for bit
    c = timed(ctx, multi(64), reps)
    pb = panel_bytes(N, nnz_l)
    info = M.multi_info()
    out = dict(system=name, N=N, nnz_l=nnz_l, rounds=M.sweep_info()["rounds"], staged_blocks=info["staged_blocks"],
               direct_blocks=info["direct_blocks"], launches_per_panel=info["launches"], reps=reps,
               single8_ms=round(a, 4), multi8_ms=round(b, 4), multi64_ms=round(c, 4),
               ratio_single8_over_multi8=round(a / b, 3), ratio_8x_single8_over_multi64=round(8 * a / c, 3),
               single8_gbs=round(8 * single_bytes(N, nnz_l) / (a * 1e-3) / 1e9, 1), panel_model_bytes=pb, multi8_gbs=round(pb / (b * 1e-3) / 1e9, 1),
               multi64_gbs=round(8 * pb / (c * 1e-3) / 1e9, 1), columns_bit_equal=same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window)")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    ctx = cpk.default_context()
    res = [measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.reps),
           measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4), a.reps)]
    line = dict(tool="tools/ldl_multi_timing.py", device=torch.cuda.get_device_name(0), kp=KP, systems=res,
                break_even=all(r["single8_ms"] > r["multi8_ms"] for r in res))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
