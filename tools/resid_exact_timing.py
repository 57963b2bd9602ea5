"""Time the exactly rounded residual against the plain one (profiles/resid_exact_timing.json): one
MI355X, the 10^6-dof system and S10 with the +-4 window, one column, the same K, z and b.

Both legs are the _device entries with R stored and no sums (`r`), and with the four sums
(`r_sums`; the exact entry takes them in a second pass over r and b, kkt_sums_kernel).  A leg is
`--reps` calls enqueued between two synchronisations after a warm-up call; rounds alternate the
legs and the medians are reported.  The byte model of a single-column pass is the plain residual's,
12 nnz(K) + 4 (N + 1) + 24 N (the sums pass adds 16 N + 4 (nblk + 1), counted for the exact leg with
sums): the exact kernel moves the same bytes and adds arithmetic only, so its fraction of 8 TB/s
says how far it is from the memory bound.  Prints one JSON line."""
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
from ipm_sequence_timing import canon, window  # noqa: E402

PEAK = 8.0e12  # bytes/s


def vp(t):
    return C.c_void_p(t.data_ptr())


def measure(ctx, label, S, rounds, reps):
    S = {k: (canon(v) if sp.issparse(v) else v) for k, v in S.items()}
    n, m = S["n"], S["m"]
    N = n + m
    K = cpk.KKT(cpk.Matrix(S["Q"], ctx=ctx), cpk.Matrix(S["B"], ctx=ctx), cpk.Matrix(S["C"], ctx=ctx))
    nnz = K.info()["nnz"]
    model = 12.0 * nnz + 4.0 * (N + 1) + 24.0 * N
    rng = np.random.default_rng(3)
    z = torch.from_numpy(rng.standard_normal(N)).cuda()
    b = torch.from_numpy(np.ascontiguousarray(S["rhs"], dtype=np.float64)).cuda()
    r = torch.empty_like(z)
    nr = torch.zeros(4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = _lib.lib
    legs = {
        "plain_r": lambda: lib.cpk_kkt_residual_device(K.h, 1, vp(z), N, vp(b), N, vp(r), N, None),
        "exact_r": lambda: lib.cpk_kkt_residual_exact_device(K.h, 1, vp(z), N, vp(b), N, vp(r), N, None),
        "plain_r_sums": lambda: lib.cpk_kkt_residual_device(K.h, 1, vp(z), N, vp(b), N, vp(r), N, vp(nr)),
        "exact_r_sums": lambda: lib.cpk_kkt_residual_exact_device(K.h, 1, vp(z), N, vp(b), N, vp(r), N, vp(nr)),
    }
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():  # the legs alternate within a round
            _lib.check(fn())
            t, _ = window(ctx, lambda: [_lib.check(fn()) for _ in range(reps)])
            ms[k].append(t / reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the two residuals of this operand, so that the record says what was timed
    _lib.check(legs["plain_r"]())
    ctx.synchronize()
    rp = r.clone()
    _lib.check(legs["exact_r"]())
    ctx.synchronize()
    differ = int((rp != r).sum().item())
    return dict(system=label, n=n, m=m, nnz_K=nnz, model_bytes=model, rounds=rounds, reps=reps,
                ms={k: dict(median=med[k], min=min(v), max=max(v), rounds=v) for k, v in ms.items()},
                fraction_of_8TBs={k: (model + (16.0 * N if k == "exact_r_sums" else 0.0)) / (med[k] * 1e-3) / PEAK for k in med},
                exact_over_plain=dict(r=med["exact_r"] / med["plain_r"], r_sums=med["exact_r_sums"] / med["plain_r_sums"]),
                rows_where_the_two_residuals_differ=differ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=1_000_000, help="dofs of the mid-sized system")
    ap.add_argument("--size", type=int, default=10_000_000, help="dofs of the S10 system (+-4 window); 0 to skip")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=32)
    a = ap.parse_args()
    ctx = cpk.default_context()
    res = [measure(ctx, f"saddle_system(N={a.mid})", saddle_system(N=a.mid), a.rounds, a.reps)]
    if a.size:
        res.append(measure(ctx, f"S10 +-4 (saddle_system(N={a.size}, window=4))", saddle_system(N=a.size, window=4),
                           a.rounds, a.reps))
    note = ("ms is wall time around enqueued calls divided by reps; one column; the exact entry's sums are a second "
            "pass (kkt_sums_kernel) over r and b")
    print(json.dumps(dict(tool="resid_exact_timing", note=note, device=torch.cuda.get_device_name(0),
                          peak_bytes_per_s=PEAK, systems=res)))


if __name__ == "__main__":
    main()
