"""The reference of the compressed basis (engine option basis_f32): arnoldi_ref.py's step with a
rounding hook, and whole cpgmres / cpdqgmres solves built on it.

rd is the rounding of a ring store (DESIGN.md "Compressed basis"): the identity for the double basis,
f32 for the float one.  One rule defines every value:

  * a basis vector [V(:, j); Q(:, j)] and a direction [PV(:, j); PQ(:, j)] are formed and normalised in
    double, exactly as arnoldi_ref.py forms them, and rounded ONCE when they are stored in their ring
    slot; the rings here are float64 arrays that hold rd's image, so every ring read sees the rounded
    value converted exactly to double;
  * everything that works on the vector under construction (the window sums against [u; t], the
    orthogonalisation, H(k+1, k) = sqrt(<u, vnew> + <t, qnew>)) sees the unrounded vector;
  * cpdqgmres updates x and y with the unrounded direction.

Within a step nothing reads a slot after it has been stored, so the step is arnoldi_ref.py's step
followed by rd on the slots it stored -- the hook sits at the stores and nowhere else.

The solves are the loops of kernels/cpgmres.m and kernels/cpdqgmres.m around that step, each piece
from what exists already: the Krylov product is the project's SpMV definition (per row, 0 + a1 x1 +
a2 x2 + ... in entry order, one rounded operation at a time: spmv below), M*z is whatever the caller
passes (the oracle's LDL2, on the product's exported factors when the device is compared), window sums
are oracle.xdot (with the rational check where xacc_cases.a_applies).  With rd the identity a solve
equals oracle.method(...) in exact mode bit for bit (test_arnoldi_f32_ref_host.py), which pins this
module before it is used with rd = f32.

A plain module (not a conftest); test infrastructure only."""
import math

import numpy as np
import scipy.sparse as sp

import arnoldi_ref as R


def ident(v):
    return v


def f32(v):
    """IEEE round-to-nearest-even to binary32, subnormals kept, beyond the range +-inf; back as float64"""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


# ---- the step ------------------------------------------------------------------------------------
def gmres_step(S, V, w, ut, H, c, s, g, rd=ident, **kw):
    """arnoldi_ref.gmres_step; the new basis vector V(:, k+1) goes to its slot through rd"""
    out = R.gmres_step(S, V, w, ut, H, c, s, g, **kw)
    if S["running"] and not out["err"]:
        V[:, S["kk"]] = rd(V[:, S["kk"]])
    return out


def dqgmres_step(S, V, PV, xy, w, ut, H, c, s, g, rd=ident, **kw):
    """arnoldi_ref.dqgmres_step; V(:, kp1pos) and PV(:, kpos) go to their slots through rd (x and y
    have been updated with the unrounded direction)"""
    out = R.dqgmres_step(S, V, PV, xy, w, ut, H, c, s, g, **kw)
    if S["running"] and not out["err"]:
        M1 = S["mem"] + 1
        V[:, S["kk"] % M1] = rd(V[:, S["kk"] % M1])
        PV[:, (S["kk"] - 1) % M1] = rd(PV[:, (S["kk"] - 1) % M1])
    return out


# ---- the Krylov product -------------------------------------------------------------------------------
class Spmv:
    """y = A x by the project's definition: per row acc = 0; acc = acc + a_p * x_p over the row's
    entries in storage order, every product and every sum rounded.  (Entry rank by entry rank over all
    rows at once: the same operations in the same order per row.)"""

    def __init__(self, A):
        A = sp.csr_matrix(A)
        A.sum_duplicates()
        A.sort_indices()
        self.shape = A.shape
        ptr = A.indptr.astype(np.int64)
        cnt = np.diff(ptr)
        self.ranks = []
        for r in range(int(cnt.max()) if cnt.size else 0):
            rows = np.flatnonzero(cnt > r)
            p = ptr[rows] + r
            self.ranks.append((rows, A.indices[p].astype(np.int64), A.data[p].astype(np.float64)))

    def __matmul__(self, x):
        y = np.zeros(self.shape[0])
        with np.errstate(all="ignore"):
            for rows, cols, vals in self.ranks:
                y[rows] = y[rows] + vals * x[cols]
        return y


class System:
    """the operators of a solve: A and C (scipy), M (anything with M @ z), and the stopping options"""

    def __init__(self, A, C, M, atol, rtol, itmax, rational=False):
        self.n, self.m = A.shape[0], C.shape[0]
        self.N = self.n + self.m
        self.A, self.C, self.M = Spmv(A), Spmv(C), M
        self.atol, self.rtol, self.itmax = float(atol), float(rtol), float(itmax)
        self.rational = rational

    def apply(self, v):
        """[u; t] = blkdiag(A, C) * v and w = M * [u; -t]"""
        u, t = self.A @ v[:self.n], self.C @ v[self.n:]
        return self.M @ np.concatenate([u, -t]), np.concatenate([u, t])

    def start(self, b, x, y, first, dq=False):
        """cpgmres.m:159-180 / cpdqgmres.m:146-164: the unrounded, normalised first basis vector and the
        residual norm (None: dot(u, V1) + dot(t, Q1) < 0, the reference's error)"""
        n = self.n
        u = b.copy() if first else b - self.A @ x
        t = np.zeros(self.m) if first else self.C @ y
        w = self.M @ np.concatenate([u, -t])
        v1 = np.concatenate([w[:n], -w[n:] if first else y - w[n:]])
        rn2 = R.part_sum(u, v1[:n], self.rational)
        rn2 = rn2 + (0.0 if dq else R.part_sum(t, v1[n:], self.rational))
        if rn2 < 0:
            return v1, None
        rn = math.sqrt(rn2)
        if rn != 0:
            v1 = v1 / rn
        return v1, rn


class Indefinite(Exception):
    """the reference's error: a negative squared norm at iteration `iter` (0: of the first vector)"""

    def __init__(self, it, val):
        super().__init__(f"Iter {it}: negative squared norm {val!r}")
        self.iter, self.val = it, val


def _result(x, y, hist, niters, solved):
    return x, y, dict(niters=int(niters), solved=bool(solved), residHistory=np.array(hist))


def gmres(Sy, b, restart, rd=ident):
    """kernels/cpgmres.m on the step above -- x, y, dict(niters, solved, residHistory)"""
    n, m, N = Sy.n, Sy.m, Sy.N
    restart = int(restart)
    assert restart >= 1 and math.ceil(Sy.itmax / restart) >= 1
    x, y = np.zeros(n), np.zeros(m)
    hist, outer, finished, stopTol, k, rn = [], 0, False, 0.0, 0, 0.0
    while not finished and outer < math.ceil(Sy.itmax / restart):
        outer += 1
        V = np.zeros((N, restart + 1), order="F")
        v1, rn = Sy.start(b, x, y, outer == 1)
        if rn is None:
            raise Indefinite(0, float("nan"))
        V[:, 0] = rd(v1)
        if outer == 1:
            stopTol = Sy.atol + Sy.rtol * rn
            hist.append(rn)
        H, c, s, g = np.zeros((restart + 1, restart)), np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        g[0] = rn
        k = 0
        while rn > stopTol and k < restart:
            k += 1
            w, ut = Sy.apply(V[:, k - 1])
            St = dict(n=n, kk=k, restart=restart, running=1, stopTol=stopTol, residNorm=rn)
            out = gmres_step(St, V, w, ut, H, c, s, g, rd=rd, rational=Sy.rational)
            if out["err"]:
                raise Indefinite((outer - 1) * restart + out["err_iter"], out["err_val"])
            rn = out["residNorm"]
            hist += out["hist"]
        z = g[:k].copy()  # z = H(1:k,1:k) \ g(1:k), column oriented (cpgmres.m:257)
        with np.errstate(all="ignore"):
            for j in range(k - 1, -1, -1):
                z[j] = z[j] / H[j, j]
                z[:j] = z[:j] - z[j] * H[:j, j]
            tmp = np.zeros(N)
            for j in range(k):
                tmp = tmp + V[:, j] * z[j]
            x = x + tmp[:n]
            y = y - (np.zeros(m) + tmp[n:])
        finished = rn <= stopTol
    return _result(x, y, hist, (outer - 1) * restart + k, rn <= stopTol)


def dqgmres(Sy, b, mem, rd=ident):
    """kernels/cpdqgmres.m on the step above -- x, y, dict(niters, solved, residHistory)"""
    n, N = Sy.n, Sy.N
    mem = max(1, int(min(float(mem), Sy.itmax)))
    M1 = mem + 1
    V, PV, xy = np.zeros((N, M1), order="F"), np.zeros((N, M1), order="F"), np.zeros(N)
    v1, rn = Sy.start(b, None, None, True, dq=True)
    if rn is None:
        raise Indefinite(0, float("nan"))
    V[:, 0] = rd(v1)
    stopTol = Sy.atol + Sy.rtol * rn
    hist = [rn]
    H, c, s, g = {}, np.zeros(mem), np.zeros(mem), np.zeros(M1)
    g[0] = rn
    k = 0
    while rn > stopTol and k < Sy.itmax:
        k += 1
        w, ut = Sy.apply(V[:, (k - 1) % M1])
        St = dict(n=n, kk=k, mem=mem, itmax=Sy.itmax, running=1, stopTol=stopTol, residNorm=rn)
        out = dqgmres_step(St, V, PV, xy, w, ut, H, c, s, g, rd=rd, rational=Sy.rational)
        if out["err"]:
            raise Indefinite(out["err_iter"], out["err_val"])
        rn = out["residNorm"]
        hist += out["hist"]
        for j in [j for j in H if j < k - mem - 1]:  # rows the engine's ring of mem + 2 has dropped
            del H[j]
    return _result(xy[:n].copy(), xy[n:].copy(), hist, k, rn <= stopTol)


def solve(method, Sy, b, window, rd=ident):
    return (gmres if method == "gmres" else dqgmres)(Sy, b, window, rd=rd)
