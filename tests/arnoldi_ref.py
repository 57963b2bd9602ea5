"""One Arnoldi step of cpgmres and of cpdqgmres on numpy arrays: the reference of
cpk_debug_arnoldi_step (test_gpu_arnoldi_step.py), pinned to the oracle by test_arnoldi_ref_host.py.

Written from the algorithm (kernels/cpgmres.m:212-247, kernels/cpdqgmres.m:208-269,
util/SymGivens.m), in the reference's own 1-based (i, j) indexing of H:

  * every vector is the stacked [V(:, j); Q(:, j)] of length N, rows [0, n) the x-part;
  * a window sum is fl(x-part) + fl(y-part), each part the correctly rounded exact sum of its
    products: oracle.xdot always, and rational arithmetic (xacc_cases.ref_exact) as well wherever it
    is the definition (xacc_cases.a_applies); the two must agree;
  * the vector updates are elementwise numpy, one rounded operation at a time (v = v - h * Vj is a
    product and then a difference, never a fused operation);
  * the rotations, SymGivens, g, residNorm and stop are Python floats.

H of cpgmres is a (restart + 1) x restart array, H[i - 1, j - 1] = H(i, j).  H of cpdqgmres is a
dict of rows, H[j][col - 1] = H(j, col) with col = 2 + k - j the reference's diagonal-compressed
column (cpdqgmres.m:133-137), so a step at k = 10^6 holds mem + 2 rows and not 10^6.  pack_* and
unpack_* map both to the engine's storage (include/cpk.h, cpk_debug_arnoldi_step).

hwin / hk1: the window sums and H(k+1, k) to use in place of the reference's own (the default
mode's sums are not exact; everything downstream of them is still checked bit for bit).

A plain module (not a conftest); test infrastructure only."""
import math

import numpy as np

import xacc_cases as X
from oracle import oracle as O


# ---- the engine's storage of H -----------------------------------------------------------------
def pack_hg(H):
    """cpgmres: H(i, j) at [(i - 1) + (j - 1) * (restart + 1)] (column-major)"""
    return np.ascontiguousarray(H.reshape(-1, order="F"))


def unpack_hg(flat, restart):
    return np.array(flat, dtype=np.float64).reshape((restart + 1, restart), order="F")


def hd_rows(kk, mem):
    """the rows j that the ring of mem + 2 rows holds at step kk (labels <= 0: slots not yet used)"""
    return range(kk - mem - 1, kk + 1)


def pack_hd(rows, mem):
    """cpdqgmres: row j at ring row j % (mem + 2), H(j, col) at [(j % (mem + 2)) * (mem + 2) + col - 1]"""
    W = mem + 2
    flat = np.zeros(W * W)
    assert len({j % W for j in rows}) == len(rows)
    for j, row in rows.items():
        flat[(j % W) * W:(j % W + 1) * W] = row
    return flat


def unpack_hd(flat, mem, kk):
    W = mem + 2
    return {j: np.array(flat[(j % W) * W:(j % W + 1) * W], dtype=np.float64) for j in hd_rows(kk, mem)}


# ---- the pieces ----------------------------------------------------------------------------------
def part_sum(a, b, rational=True):
    """the correctly rounded exact sum of a[i] * b[i]"""
    v = O.xdot(a, b)
    if rational and X.a_applies(a, b):
        r = X.ref_exact(a, b)
        assert X.same_bits(v, r), (v, r)
    return v


def window_sum(a, b, n, rational=True):
    return part_sum(a[:n], b[:n], rational) + part_sum(a[n:], b[n:], rational)


def sign(a):
    return float((a > 0) - (a < 0))


def _div(a, b):
    """a / b as IEEE defines it (x / 0 is an infinity or a NaN, where Python raises)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def sym_givens(a, b):
    """util/SymGivens.m"""
    if b == 0:
        c = 1.0 if a == 0 else sign(a)
        return c, 0.0, abs(a)
    if a == 0:
        return 0.0, sign(b), abs(b)
    if abs(b) > abs(a):
        t = _div(a, b)
        s = _div(sign(b), math.sqrt(1 + t * t))
        return s * t, s, _div(b, s)
    t = _div(b, a)
    c = _div(sign(a), math.sqrt(1 + t * t))
    return c, c * t, _div(a, c)


def _sub_scaled(v, h, x):
    """v - h * x, two rounded operations per element"""
    p = h * x
    return v - p


def _out(S):
    return dict(hk1=S.get("hk1"), residNorm=S["residNorm"], stop=0, err=0, err_val=0.0, err_iter=0, hist=[], hwin=[])


def _norm2(S, out, ut, vnew, n, kk, rational):
    """H(k+1, k)^2 (cpgmres.m:219, cpdqgmres.m:218); negative: the step stops with err = 4"""
    hn2 = window_sum(ut, vnew, n, rational)
    out["hn2"], out["vnew"] = hn2, vnew.copy()  # vnew: orthogonalised, not yet normalised
    if hn2 < 0:
        out.update(err=4, err_val=hn2, err_iter=kk, stop=1)
        return False
    return True


# ---- cpgmres.m:212-247 ------------------------------------------------------------------------------
def gmres_step(S, V, w, ut, H, c, s, g, hwin=None, hk1=None, rational=True):
    """S: n, kk, restart, running, stopTol, residNorm (and hk1, passed through when nothing runs).
    V (N x (restart + 1)), H, c, s, g are updated in place.  Returns hk1, residNorm, stop, err,
    err_val, err_iter, hist (the values pushed), hwin (the window sums) and hn2."""
    out = _out(S)
    if not S["running"]:
        return out
    n, k, restart = S["n"], S["kk"], S["restart"]
    with np.errstate(all="ignore"):
        vnew = np.concatenate([w[:n], V[n:, k - 1] - w[n:]])
        for j in range(1, k + 1):
            H[j - 1, k - 1] = window_sum(V[:, j - 1], ut, n, rational) if hwin is None else hwin[j - 1]
            out["hwin"].append(H[j - 1, k - 1])
        for j in range(1, k + 1):
            vnew = _sub_scaled(vnew, H[j - 1, k - 1], V[:, j - 1])
        V[:, k] = vnew
        if not _norm2(S, out, ut, vnew, n, k, rational):
            return out
        h = math.sqrt(out["hn2"]) if hk1 is None else hk1
        out["hk1"] = h
        H[k, k - 1] = h
        if h != 0:
            V[:, k] = V[:, k] / h
    for j in range(1, k):
        a, b = float(H[j - 1, k - 1]), float(H[j, k - 1])
        cj, sj = float(c[j - 1]), float(s[j - 1])
        H[j - 1, k - 1] = cj * a + sj * b
        H[j, k - 1] = sj * a - cj * b
    ck, sk, d = sym_givens(float(H[k - 1, k - 1]), float(H[k, k - 1]))
    c[k - 1], s[k - 1], H[k - 1, k - 1] = ck, sk, d
    H[k, k - 1] = 0.0
    gk = float(g[k - 1])
    g[k] = sk * gk
    g[k - 1] = ck * gk
    out["residNorm"] = abs(float(g[k]))
    out["hist"].append(out["residNorm"])
    out["stop"] = int(not (out["residNorm"] > S["stopTol"] and k < restart))
    return out


# ---- cpdqgmres.m:208-269 ---------------------------------------------------------------------------
def dqgmres_step(S, V, PV, xy, w, ut, H, c, s, g, hwin=None, hk1=None, rational=True):
    """S: n, kk, mem, itmax, running, stopTol, residNorm.  V, PV (N x (mem + 1) ring slots), xy, the
    rows of H (a dict, see the module's docstring), c, s, g are updated in place."""
    out = _out(S)
    if not S["running"]:
        return out
    n, k, mem = S["n"], S["kk"], S["mem"]
    M1 = mem + 1
    kpos, kp1pos, rotpos = (k - 1) % M1, k % M1, (k - 1) % mem  # 0-based slots
    with np.errstate(all="ignore"):
        vnew = np.concatenate([w[:n], V[n:, kpos] - w[n:]])
        H[k] = np.zeros(mem + 2)  # the reference's H starts as zeros; row k is first written here
        win = range(max(1, k - mem + 1), k + 1)
        for q, j in enumerate(win):
            H[j][2 + k - j - 1] = window_sum(V[:, (j - 1) % M1], ut, n, rational) if hwin is None else hwin[q]
            out["hwin"].append(H[j][2 + k - j - 1])
        for j in win:
            vnew = _sub_scaled(vnew, H[j][2 + k - j - 1], V[:, (j - 1) % M1])
        V[:, kp1pos] = vnew
        if not _norm2(S, out, ut, vnew, n, k, rational):
            return out
        h = math.sqrt(out["hn2"]) if hk1 is None else hk1
        out["hk1"] = h
        H[k][0] = h
        if h != 0:
            V[:, kp1pos] = V[:, kp1pos] / h
    for j in range(max(1, k - mem), k):
        jr, kk, kk1 = (j - 1) % mem, k - j + 1, k - j + 2
        a, b = float(H[j][kk1 - 1]), float(H[j + 1][kk - 1])
        cj, sj = float(c[jr]), float(s[jr])
        H[j][kk1 - 1] = cj * a + sj * b
        H[j + 1][kk - 1] = sj * a - cj * b
    ck, sk, d = sym_givens(float(H[k][1]), float(H[k][0]))
    c[rotpos], s[rotpos], H[k][1] = ck, sk, d
    H[k][0] = 0.0
    gk = float(g[kpos])
    g[kp1pos] = sk * gk
    g[kpos] = ck * gk
    with np.errstate(all="ignore"):
        pv = V[:, kpos].copy()
        for j in range(max(1, k - mem), k):
            pv = _sub_scaled(pv, H[j][2 + k - j - 1], PV[:, (j - 1) % M1])
        pv = pv / H[k][1]
        PV[:, kpos] = pv
        gk = g[kpos]
        p = gk * pv
        xy[:n] = xy[:n] + p[:n]
        xy[n:] = xy[n:] - p[n:]
    out["residNorm"] = abs(float(g[kp1pos]))
    out["hist"].append(out["residNorm"])
    out["stop"] = int(not (out["residNorm"] > S["stopTol"] and k < S["itmax"]))
    return out
