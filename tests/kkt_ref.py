"""The reference of the saddle-point operator tests: K = [A B'; B -C] in the product's entry
order, its product and residual by scalar float64 operations in that order, and the exact sums of
squares from the oracle.  Test infrastructure only (a plain module); no product code."""
import numpy as np
import scipy.sparse as sp

MEMBERS = ("tiny1x1", "tiny2x1", "tiny65x63", "zero_c", "empty_rows", "arrow_row", "cvxqp1_m", "cvxqp2_s")
TINY = ("tiny1x1", "tiny2x1", "tiny65x63")

_CACHE = {}


def system(name):
    """dict(A, B, C, G, rhs, n, m) of a member: A is the (1,1) block the solvers take (Q)."""
    if name not in _CACHE:
        if name.startswith("cvxqp"):
            import fixtures as F
            P = F.load(name)
        else:
            import structures as S
            P = S.get(name)
        _CACHE[name] = dict(A=_canon(P["Q"]), B=_canon(P["B"]), C=_canon(P["C"]), G=_canon(P["G"]),
                            rhs=np.array(P["rhs"], dtype=np.float64), n=int(P["n"]), m=int(P["m"]))
    return _CACHE[name]


def _canon(M):
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return M


def assemble(A, B, C):
    """K as CSR arrays (indptr, indices, data): row i < n is A's row, then B''s entries by
    ascending constraint; row n + i is B's row, then -C's row.  Explicit zeros are kept."""
    A, B, C = _canon(A), _canon(B), _canon(C)
    n, m = A.shape[0], C.shape[0]
    Bt = _canon(B.T)  # rows of B' with the constraints ascending
    ptr, ind, val = [0], [], []
    for i in range(n):
        for M, shift, sign in ((A, 0, 1.0), (Bt, n, 1.0)):
            lo, hi = M.indptr[i], M.indptr[i + 1]
            ind.append(M.indices[lo:hi].astype(np.int64) + shift)
            val.append(sign * M.data[lo:hi])
        ptr.append(ptr[-1] + len(ind[-1]) + len(ind[-2]))
    for i in range(m):
        for M, shift, sign in ((B, 0, 1.0), (C, n, -1.0)):
            lo, hi = M.indptr[i], M.indptr[i + 1]
            ind.append(M.indices[lo:hi].astype(np.int64) + shift)
            val.append(sign * M.data[lo:hi])
        ptr.append(ptr[-1] + len(ind[-1]) + len(ind[-2]))
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)  # noqa: E731
    return np.array(ptr, np.int64), cat(ind, np.int64), cat(val, np.float64)


def operator(name):
    """(indptr, indices, data) of a member's K, built once."""
    key = ("K", name)
    if key not in _CACHE:
        P = system(name)
        _CACHE[key] = assemble(P["A"], P["B"], P["C"])
    return _CACHE[key]


def as_scipy(K):
    ptr, ind, val = K
    N = len(ptr) - 1
    return sp.csr_matrix((val, ind, ptr), shape=(N, N))


def matvec(K, z):
    """s_i from 0.0, adding the separately rounded products K_ij * z_j in entry order: a plain
    loop of scalar float64 operations (Python floats: IEEE doubles, no FMA)."""
    ptr, ind, val = K
    zl, vl, il = [float(v) for v in z], val.tolist(), ind.tolist()
    out = np.zeros(len(ptr) - 1)
    for i in range(len(ptr) - 1):
        s = 0.0
        for e in range(ptr[i], ptr[i + 1]):
            p = vl[e] * zl[il[e]]
            s = s + p
        out[i] = s
    return out


def residual(K, z, b):
    return np.asarray(b, dtype=np.float64) - matvec(K, z)


def sums(r, b, n):
    """The four exact sums of squares [r(1:n), r(n+1:N), b(1:n), b(n+1:N)] (the oracle's xdot)."""
    from oracle import oracle as O
    return np.array([O.xdot(r[:n], r[:n]), O.xdot(r[n:], r[n:]), O.xdot(b[:n], b[:n]), O.xdot(b[n:], b[n:])])


def gamma(q):
    u = 2.0 ** -53
    return q * u / (1.0 - q * u)


def same_bits(a, b):
    """Equality with ==, a NaN equal to a NaN at the same place."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def operands(name, seed=0):
    """The z operands of the product tests: seeded random, a unit vector, zero, one NaN."""
    P = system(name)
    N = P["n"] + P["m"]
    rng = np.random.default_rng(1000 + seed)
    zr = rng.standard_normal(N)
    zu = np.zeros(N)
    zu[N // 2] = 1.0
    zn = zr.copy()
    zn[N // 3] = np.nan
    return {"random": zr, "unit": zu, "zero": np.zeros(N), "nan": zn}
