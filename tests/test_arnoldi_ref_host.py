"""The step reference of the Arnoldi kernels (arnoldi_ref.py) against the oracle, on the CPU.

Starting from the oracle's operators on cvxqp2_s in exact mode (Q, C and oracle.LDL2 for M), the
step functions iterated by the loops of cpgmres.m / cpdqgmres.m reproduce the oracle's residHistory,
x and y with ==, over several restart cycles and ring wraps.  A mismatch here is a bug in the
reference."""
import numpy as np
import pytest

import arnoldi_ref as R
import fixtures as F
import xacc_cases as X
from oracle import oracle as O
from test_oracle import SYMGIVENS_TABLE

ITERS = 60
TOL = dict(atol=1.0e-10, rtol=1.0e-10)


@pytest.fixture(scope="module")
def system():
    P = F.load("cvxqp2_s")
    M = O.LDL2(P["G"], P["B"], -P["C"])
    M.set(nitref=1, force_itref=1)
    return P, M, P["rhs"][:P["n"]].copy()


def _start(P, M, b, x, y, first):
    """cpgmres.m:159-180 / cpdqgmres.m:146-164: u, t, the first basis vector and the residual norm"""
    n = P["n"]
    u = b.copy() if first else b - P["Q"] @ x
    t = np.zeros(P["m"]) if first else P["C"] @ y
    w = M @ np.concatenate([u, -t])
    v1 = np.concatenate([w[:n], -w[n:] if first else y - w[n:]])
    ut = np.concatenate([u, t])
    rn2 = R.window_sum(ut, v1, n, rational=False)
    assert rn2 >= 0
    rn = float(np.sqrt(rn2))
    if rn != 0:
        v1 = v1 / rn
    return v1, rn


def _apply(P, M, v):
    """[u; t] = blkdiag(A, C) * v and w = M * [u; -t]"""
    n = P["n"]
    u, t = P["Q"] @ v[:n], P["C"] @ v[n:]
    return M @ np.concatenate([u, -t]), np.concatenate([u, t])


def ref_gmres(P, M, b, restart, itmax):
    n, N = P["n"], P["n"] + P["m"]
    x, y = np.zeros(n), np.zeros(P["m"])
    hist, outer, finished = [], 0, False
    stopTol = 0.0
    while not finished and outer < -(-itmax // restart):
        outer += 1
        V = np.zeros((N, restart + 1), order="F")
        V[:, 0], rn = _start(P, M, b, x, y, outer == 1)
        if outer == 1:
            stopTol = TOL["atol"] + TOL["rtol"] * rn
            hist.append(rn)
        H, c, s, g = np.zeros((restart + 1, restart)), np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        g[0] = rn
        k = 0
        while rn > stopTol and k < restart:
            k += 1
            w, ut = _apply(P, M, V[:, k - 1])
            S = dict(n=n, kk=k, restart=restart, running=1, stopTol=stopTol, residNorm=rn)
            out = R.gmres_step(S, V, w, ut, H, c, s, g, rational=(outer == 1 and k <= 2))
            assert out["err"] == 0
            rn = out["residNorm"]
            hist += out["hist"]
            assert out["stop"] == int(not (rn > stopTol and k < restart))
        z = g[:k].copy()  # z = H(1:k,1:k) \ g(1:k), column oriented (cpgmres.m:257)
        for j in range(k - 1, -1, -1):
            z[j] = z[j] / H[j, j]
            z[:j] = z[:j] - z[j] * H[:j, j]
        tmp = np.zeros(N)
        for j in range(k):
            tmp = tmp + V[:, j] * z[j]
        x = x + tmp[:n]
        y = y - (np.zeros(P["m"]) + tmp[n:])
        finished = rn <= stopTol
    return x, y, np.array(hist)


def ref_dqgmres(P, M, b, mem, itmax):
    n, N = P["n"], P["n"] + P["m"]
    mem = max(1, min(mem, itmax))
    V, PV, xy = np.zeros((N, mem + 1), order="F"), np.zeros((N, mem + 1), order="F"), np.zeros(N)
    V[:, 0], rn = _start(P, M, b, None, None, True)  # (cpdqgmres.m:157 takes dot(u, V1) alone: t = 0 adds +0)
    stopTol = TOL["atol"] + TOL["rtol"] * rn
    hist = [rn]
    H, c, s, g = {}, np.zeros(mem), np.zeros(mem), np.zeros(mem + 1)
    g[0] = rn
    k = 0
    while rn > stopTol and k < itmax:
        k += 1
        w, ut = _apply(P, M, V[:, (k - 1) % (mem + 1)])
        S = dict(n=n, kk=k, mem=mem, itmax=itmax, running=1, stopTol=stopTol, residNorm=rn)
        out = R.dqgmres_step(S, V, PV, xy, w, ut, H, c, s, g, rational=(k <= 2))
        assert out["err"] == 0
        rn = out["residNorm"]
        hist += out["hist"]
        for j in [j for j in H if j < k - mem - 1]:  # what the engine's ring of mem + 2 rows has dropped
            del H[j]
        # the engine's storage holds exactly these rows: the round trip is the identity
        back = R.unpack_hd(R.pack_hd(H, mem), mem, k)
        assert all(np.array_equal(back[j], H[j]) for j in H)
    return xy[:n], xy[n:], np.array(hist)


def _same(got, want):
    x, y, h = got
    xo, yo, so = want
    ho = so["residHistory"]
    assert len(h) == len(ho) and len(h) > 1
    bad = np.flatnonzero(h != ho)
    assert bad.size == 0, (bad[:5], h[bad[:3]], ho[bad[:3]])
    assert np.array_equal(x, xo) and np.array_equal(y, yo)


@pytest.mark.parametrize("restart", (5, 20))
def test_gmres_steps_reproduce_the_oracle(system, restart):
    P, M, b = system
    opts = dict(TOL, itmax=ITERS, restart=restart, print=False)
    with O.exact():
        want = O.method("gmres", b, P["Q"], P["C"], M, opts)
        got = ref_gmres(P, M, b, restart, ITERS)
    assert len(want[2]["residHistory"]) > 2 * restart  # several cycles
    _same(got, want)


@pytest.mark.parametrize("mem", (1, 3, 20))
def test_dqgmres_steps_reproduce_the_oracle(system, mem):
    P, M, b = system
    opts = dict(TOL, itmax=ITERS, mem=mem, print=False)
    with O.exact():
        want = O.method("dqgmres", b, P["Q"], P["C"], M, opts)
        got = ref_dqgmres(P, M, b, mem, ITERS)
    assert len(want[2]["residHistory"]) > 2 * (mem + 1) + 2  # the ring wrapped twice
    _same(got, want)


def test_hg_pack_round_trip():
    H = np.arange(30.0).reshape(6, 5)
    flat = R.pack_hg(H)
    assert flat[2 + 3 * 6] == H[2, 3]  # H(3, 4) at (3 - 1) + (4 - 1) * (restart + 1)
    assert np.array_equal(R.unpack_hg(flat, 5), H)


@pytest.mark.parametrize("a,b,exp", SYMGIVENS_TABLE)
def test_sym_givens_equals_the_oracle(a, b, exp):
    assert X.same_bits(R.sym_givens(a, b), O.symgivens(a, b))
    assert np.allclose(R.sym_givens(a, b), exp, rtol=1e-15, atol=0)
    assert X.same_bits(R.sym_givens(-a, -b), O.symgivens(-a, -b))
