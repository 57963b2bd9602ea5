"""The reference of the compressed basis (arnoldi_f32_ref.py) on the CPU, before it is used with
rd = f32 against the device (test_gpu_basis_f32_step.py, test_gpu_basis_f32_solve.py).

  * rd the identity: the step equals arnoldi_ref.py's, array for array;
  * rd the identity: the solves equal oracle.method("gmres" | "dqgmres", ...) in exact mode bit for
    bit -- niters, solved, history, x, y -- on the tiny members and on cvxqp2_s, over several restart
    cycles and ring wraps; so the Krylov product (Spmv), the start, the loops, the back substitution
    and the wrap-up are the oracle's;
  * rd = f32 is IEEE round-to-nearest-even with subnormals and infinities, and a solve with it
    differs from the double one (the deviation is printed);
  * the systems of the default-mode GPU comparison: the reference's iteration count does not move
    under 1e-15 perturbations of the rhs (test_gpu_basis_f32_solve.py relies on it)."""
import numpy as np
import pytest

import arnoldi_f32_ref as RF
import arnoldi_ref as R
import basis_f32_cases as BC
import xacc_cases as X
from oracle import oracle as O


# ---- the step with rd the identity is arnoldi_ref's -------------------------------------------------------
@pytest.mark.parametrize("method,win,kk", (("gmres", 5, 5), ("gmres", 9, 3), ("dqgmres", 4, 7), ("dqgmres", 1, 4),
                                           ("dqgmres", 6, 2)))
def test_identity_step_is_arnoldi_ref(method, win, kk):
    N, n = 130, 57
    rng = np.random.default_rng([3, win, kk])
    dq = method == "dqgmres"
    V, PV, xy = rng.standard_normal((N, win + 1)), rng.standard_normal((N, win + 1)), rng.standard_normal(N)
    w, ut = rng.standard_normal(N), rng.standard_normal(N)
    c, s, g = rng.uniform(-1, 1, win), rng.uniform(-1, 1, win), rng.standard_normal(win + 1)
    S = dict(n=n, kk=kk, running=1, stopTol=0.0, residNorm=1.0, itmax=10 ** 6, **{("mem" if dq else "restart"): win})
    outs = []
    for step in ((R.dqgmres_step, R.gmres_step), (RF.dqgmres_step, RF.gmres_step)):
        A = [np.array(a, order="F", copy=True) for a in (V, PV, xy, c, s, g)]
        if dq:
            H = {j: rng.standard_normal(win + 2) * 0 + 0.25 * j for j in R.hd_rows(kk, win) if j >= 1}
            o = step[0](S, A[0], A[1], A[2], w, ut, H, A[3], A[4], A[5], rational=False)
            A.append(R.pack_hd(H, win))
        else:
            H = np.full((win + 1, win), 0.5)
            o = step[1](S, A[0], w, ut, H, A[3], A[4], A[5], rational=False)
            A.append(R.pack_hg(H))
        outs.append((o, A))
    (o1, A1), (o2, A2) = outs
    assert all(X.same_bits(a, b) for a, b in zip(A1, A2))
    for k in ("hk1", "residNorm", "stop", "err", "hn2"):
        assert X.same_bits(o1[k], o2[k]), k
    assert X.same_bits(o1["hwin"], o2["hwin"]) and X.same_bits(o1["hist"], o2["hist"])


def test_not_running_and_error_store_nothing():
    """rd is applied where the step stored, nowhere else: a step that does not run, or stops with
    err = 4, leaves the rings to arnoldi_ref.py"""
    N, n, win = 40, 17, 3
    rng = np.random.default_rng(5)
    V = rng.standard_normal((N, win + 1))
    w, ut = rng.standard_normal(N), rng.standard_normal(N)
    S = dict(n=n, kk=1, restart=win, running=0, stopTol=0.0, residNorm=1.0)
    V2 = V.copy()
    RF.gmres_step(S, V2, w, ut, np.zeros((win + 1, win)), np.zeros(win), np.zeros(win), np.ones(win + 1), rd=RF.f32)
    assert X.same_bits(V2, V)


# ---- the solves with rd the identity are the oracle's ----------------------------------------------------------
def _same_solve(got, want):
    (x, y, s), (xo, yo, so) = got, want
    h, ho = s["residHistory"], so["residHistory"]
    assert s["niters"] == so["niters"] and s["solved"] == so["solved"], (s["niters"], so["niters"])
    assert len(h) == len(ho)
    bad = np.flatnonzero(X.bits(h) != X.bits(ho))
    assert bad.size == 0, (bad[:5], h[bad[:3]], ho[bad[:3]])
    assert X.same_bits(x, xo) and X.same_bits(y, yo)


@pytest.mark.parametrize("method,window", BC.WINDOWS)
@pytest.mark.parametrize("name", BC.SYSTEMS)
def test_identity_solve_is_the_oracle(name, method, window):
    S, b = BC.system(name)
    Mo = BC.oracle_M(S)
    opts = BC.opts(method, window)
    with O.exact():
        want = O.method(method, b, S["Q"], S["C"], Mo, opts)
        got = RF.solve(method, BC.ref_system(S, Mo, rational=S["N"] <= 8), b, window)
    _same_solve(got, want)
    if name == "cvxqp2_s":  # the runs the GPU test relies on: several cycles, ring wraps
        assert want[2]["niters"] > {5: 12, 40: 82, 20: 60, 100: 100}[window]


# ---- rd = f32 --------------------------------------------------------------------------------------------------
def test_f32_is_ieee_rounding():
    t = 2.0 ** -24
    v = np.array([1 + t, 1 + 3 * t, 1 + 2 * t, 2.0 ** -140, -0.0, 2.0 ** -160, 3.4028234e38, 3.4028236e38, 1e39,
                  -(1 + t), 2.0 ** -149 * 1.5, 2.0 ** -150])
    want = np.array([1.0, 1 + 4 * t, 1 + 2 * t, 2.0 ** -140, -0.0, 0.0, float(np.float32(3.4028234e38)), np.inf,
                     np.inf, -1.0, 2.0 ** -148, 0.0])  # ties to even; subnormals kept; beyond the range inf
    got = RF.f32(v)
    assert X.same_bits(got, want), (got, want)
    assert X.same_bits(RF.f32(got), got)  # the image is fixed


@pytest.mark.parametrize("method,window", (("gmres", 100), ("dqgmres", 40)))
def test_f32_solve_differs_from_the_double_one(method, window):
    S, b = BC.system("cvxqp2_s")
    Mo = BC.oracle_M(S)
    with O.exact():
        x64, y64, s64 = RF.solve(method, BC.ref_system(S, Mo), b, window)
        x32, y32, s32 = RF.solve(method, BC.ref_system(S, Mo), b, window, rd=RF.f32)
    assert not X.same_bits(s64["residHistory"], s32["residHistory"])
    L = min(len(s64["residHistory"]), len(s32["residHistory"]))
    dev = np.max(np.abs(s64["residHistory"][:L] - s32["residHistory"][:L])) / s64["residHistory"][0]
    print(f"{method}({window}) cvxqp2_s: niters f64 {s64['niters']} f32 {s32['niters']}, largest history deviation "
          f"{dev:.3e} of the initial residual, solved {s64['solved']} / {s32['solved']}")
    assert s32["solved"] == s64["solved"] and (method != "gmres" or s32["solved"])
    assert 0 < dev < 1e-2  # report only; a rounding rule gone wrong (to bfloat16, say) is far above


# ---- the default-mode cases are stable -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,window", BC.DEFAULT_CASES)
def test_default_cases_have_a_stable_count(name, method, window):
    band = BC.band(name, method, window)
    assert band["stable"], (name, method, window, band)
