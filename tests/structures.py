"""A deterministic family of saddle-point structures that pin kernel paths by construction.

The reference examples and the benchmark generators all have diagonal G, at most three entries
per row of B, no empty row and no dense row or column, so how deep their elimination trees get
depends on the ordering's quality.  The members here force a path through their structure alone:
a dense row stays a dense row, a clique stays a clique and an isolated node stays isolated under
any ordering.  Each member is a function returning dict(Q, G, B, C, rhs, n, m), the layout of
fixtures._synthetic; every seed is fixed.  Test infrastructure only (a plain module)."""
import numpy as np
import scipy.sparse as sp

from cpkrylov_amd.synthetic import saddle_system

TINY_SHAPES = [(1, 1), (2, 1), (3, 2), (65, 63)]


def _pack(Q, G, B, C, rhs):
    Q, G, B, C = (sp.csr_matrix(M, dtype=np.float64) for M in (Q, G, B, C))
    for M in (Q, G, B, C):
        M.sum_duplicates()
        M.sort_indices()
    m, n = B.shape
    return dict(Q=Q, G=G, B=B, C=C, rhs=np.asarray(rhs, dtype=np.float64), n=n, m=m)


def _signed(rng, size, lo=1.0 / 3.0):
    return rng.uniform(lo, 1.0, size=size) * np.where(rng.random(size) < 0.5, -1.0, 1.0)


def _band(N):
    S = saddle_system(N=N)
    G = 0.5 * (S["Q"] + sp.diags(S["Q"].diagonal()))  # tridiagonal: the whole-graph orderings
    return _pack(S["Q"], G, S["B"], S["C"], S["rhs"])


def band_g():
    """G tridiagonal at N = 3000: minimum degree on the whole graph of Kp (ordering 4)."""
    return _band(3000)


def band_g_nd():
    """The same at N = 70000: nested dissection on the whole graph (ordering 3).  For the apply
    only, not for solves."""
    return _band(70000)


def band_g_zero_c():
    """band_g with C = 0: no 1x1-pivot LDL' of the whole graph's order exists in general; the
    documented limit (CPK_ERR_FACTOR), not a working member."""
    S = band_g()
    S["C"] = sp.csr_matrix((S["m"], S["m"]))
    return S


ARROW_ROW = 1800  # the dense constraint of arrow_row
DENSE_COL = 192  # the variable of dense_col that every constraint holds


def arrow_row():
    """saddle_system(8000) with one fully dense row of B: a Kp row of n + 1 = 4401 entries (the
    SpMV long-row path, 3 chunks) and a factor row of nearly N entries, above every LDS cap."""
    S = saddle_system(N=8000)
    n = S["n"]
    B = S["B"].tolil()
    B[ARROW_ROW, :] = _signed(np.random.default_rng(8001), n)
    return _pack(S["Q"], S["G"], B, S["C"], S["rhs"])


def dense_col():
    """saddle_system(700) with one variable in every constraint: the Schur complement is a dense
    m-clique (m = 315) under any ordering -- a dense chain of upper rounds."""
    S = saddle_system(N=700)
    m = S["m"]
    B = S["B"].tolil()
    B[:, DENSE_COL] = _signed(np.random.default_rng(701), m).reshape(m, 1)
    return _pack(S["Q"], S["G"], B, S["C"], S["rhs"])


def empty_rows():
    """saddle_system(3000) with 30 consecutive zero rows of B: isolated C nodes."""
    S = saddle_system(N=3000)
    B = S["B"].tolil()
    B[600:630, :] = 0.0
    B = B.tocsr()
    B.eliminate_zeros()
    return _pack(S["Q"], S["G"], B, S["C"], S["rhs"])


def zero_c():
    """Diagonal G with C = 0 (ordering 2): the Schur complement B G^-1 B' alone carries the
    constraint block."""
    S = saddle_system(N=3000)
    return _pack(S["Q"], S["G"], S["B"], sp.csr_matrix((S["m"], S["m"])), S["rhs"])


def blocks8():
    """Eight disconnected copies of saddle_system(400) (one seed each)."""
    parts = [saddle_system(N=400, seed=8400 + k) for k in range(8)]
    n = parts[0]["n"]
    return _pack(sp.block_diag([p["Q"] for p in parts]), sp.block_diag([p["G"] for p in parts]),
                 sp.block_diag([p["B"] for p in parts]), sp.block_diag([p["C"] for p in parts]),
                 np.concatenate([p["rhs"][:n] for p in parts] + [p["rhs"][n:] for p in parts]))


# On systems this small the Krylov iteration ends after one or two steps with a residual that is
# pure rounding, and the reference's methods stop with an error when such a quantity comes out
# below zero (sqrt of a negative beta or squared norm) -- about half of all seeds, for one method
# or another.  The seeds below are the first at which the CPU oracle (no product code) solves
# with all six methods; (2, 1)'s is the first that also takes two iterations.
TINY_SEED = {(1, 1): 1, (2, 1): 6, (3, 2): 1, (65, 63): 1}
TINY_INDEFINITE = ((2, 1), 9)  # ... and the first seed at which every method of the reference stops so


def tiny(n, m, seed=None):
    """Systems smaller than one wave: G = diag(1..n), dense B in U(0.3, 1), C = 1e-8 I and
    Q = G + 0.1 * ones (for solves)."""
    rng = np.random.default_rng(TINY_SEED[(n, m)] if seed is None else seed)
    G = sp.diags(np.arange(1.0, n + 1.0))
    Q = G.toarray() + 0.1 * np.ones((n, n))
    B = rng.uniform(0.3, 1.0, size=(m, n))
    return _pack(Q, G, B, 1e-8 * sp.identity(m), rng.standard_normal(n + m))


def tiny_indefinite():
    """Not a member: the (2, 1) system on which the reference's six methods all raise their
    indefinite-preconditioner / complex-norm error at iteration 1 or 2 (a squared quantity that
    is pure rounding comes out below zero)."""
    (n, m), seed = TINY_INDEFINITE
    return tiny(n, m, seed)


def _tiny(n, m):
    return lambda: tiny(n, m)


MEMBERS = dict(band_g=band_g, band_g_nd=band_g_nd, arrow_row=arrow_row, dense_col=dense_col,
               empty_rows=empty_rows, zero_c=zero_c, blocks8=blocks8,
               **{f"tiny{n}x{m}": _tiny(n, m) for n, m in TINY_SHAPES})

# the solves: every method on the tiny members, band_g and arrow_row (not band_g_nd)
SOLVE_MEMBERS = [f"tiny{n}x{m}" for n, m in TINY_SHAPES] + ["band_g", "arrow_row"]
SOLVE_METHODS = [("minres", {}), ("cg", {}), ("cglanczos", {}), ("symmlq", {}), ("gmres", {"restart": 20}),
                 ("dqgmres", {"mem": 5})]

_CACHE = {}


def get(name):
    """The member `name`, built once; the matrices are shared, treat them as read-only."""
    if name not in _CACHE:
        _CACHE[name] = MEMBERS[name]()
    return _CACHE[name]


def kp(S):
    Kp = sp.bmat([[S["G"], S["B"].T], [S["B"], -S["C"]]]).tocsr()
    Kp.sum_duplicates()
    Kp.sort_indices()
    return Kp


def hub(S):
    """The dof with the longest row of Kp (arrow_row: its dense constraint; dense_col: the
    variable every constraint holds)."""
    return int(np.argmax(np.diff(kp(S).indptr)))
