"""The systems of the factor-report tests (host: test_factor_report_host.py, device:
test_gpu_factor_report.py) and the checks both share.  Every case is (G, B, C22, options): the
blocks of Kp = [G B'; B C22] and the engine options of the factorization."""
import functools

import numpy as np
import scipy.sparse as sp

import fixtures as F
import structures as ST
from cpkrylov_amd.synthetic import saddle_system

U = 2.0 ** -53
DELTA = 1e-9  # cvxqp2_s holds entries equal to 1e-8: a threshold of 1e-8 would sit on a tie
REPORT_FIELDS = ("n_pos", "n_neg", "n_wrong", "first_wrong", "n_perturbed", "argmin_abs", "min_abs", "max_abs",
                 "max_shift", "pivot_min")


def _fixture(name):
    P = F.load(name)
    return P["G"].tocsr(), P["B"].tocsr(), (-P["C"]).tocsr()


def _set_diag(G, dofs, fn):
    """A copy of G whose stored diagonal entries at `dofs` are fn(value): same sparsity."""
    G = G.copy()
    for j in dofs:
        lo, hi = G.indptr[j], G.indptr[j + 1]
        k = np.flatnonzero(G.indices[lo:hi] == j)
        assert len(k) == 1, "the diagonal entry must be stored"
        G.data[lo + k[0]] = fn(G.data[lo + k[0]])
    return G


def touched_dofs(B):
    """The fixed rule of the modified cvxqp2_s cases: of the columns B touches, in ascending
    order, the first, the one a third of the way and the one two thirds of the way."""
    t = np.unique(B.tocsr().indices)
    return t[[0, len(t) // 3, 2 * len(t) // 3]]


@functools.lru_cache(maxsize=None)
def zeroed():
    """cvxqp2_s with three stored diagonal entries of G set to 0 (dofs that B touches)."""
    G, B, C22 = _fixture("cvxqp2_s")
    dofs = touched_dofs(B)
    return G, _set_diag(G, dofs, lambda v: 0.0), B, C22, dofs


@functools.lru_cache(maxsize=None)
def negated():
    """cvxqp2_s with one diagonal entry of G negated: the first dof no constraint holds, so the
    matrix gains exactly one negative eigenvalue (a dof B touches can trade signs with a constraint's
    pivot: two wrong-signed pivots and the inertia unchanged, which is no less correct)."""
    G, B, C22 = _fixture("cvxqp2_s")
    dof = int(np.setdiff1d(np.arange(G.shape[0]), np.unique(B.indices))[0])
    return _set_diag(G, [dof], lambda v: -v), B, C22, dof


@functools.lru_cache(maxsize=None)
def defaults():
    out = {name: _fixture(name) for name in ("cvxqp1_m", "cvxqp2_s")}
    S = saddle_system(N=20000)
    out["synthetic20k"] = (S["G"].tocsr(), S["B"].tocsr(), (-S["C"]).tocsr())
    return out


DEFAULT_NAMES = ("cvxqp1_m", "cvxqp2_s", "synthetic20k")


@functools.lru_cache(maxsize=None)
def band_zero_c():
    S = ST.band_g_zero_c()
    return S["G"].tocsr(), S["B"].tocsr(), (-S["C"]).tocsr()


@functools.lru_cache(maxsize=None)
def dense_col():
    S = ST.get("dense_col")
    return S["G"].tocsr(), S["B"].tocsr(), (-S["C"]).tocsr()


def kp_of(G, B, C22):
    return sp.bmat([[G, B.T], [B, C22]]).tocsr()


def recomputed_report(D, perm, n, E, pivot_min):
    """Every report field from the exported D and perm (and E in dof order), in numpy."""
    s = np.where(perm < n, 1.0, -1.0)
    wrong = np.flatnonzero(s * D < 0)
    Ek = E[perm]
    return dict(n_pos=int((D > 0).sum()), n_neg=int((D < 0).sum()), n_wrong=len(wrong),
                first_wrong=int(wrong[0]) if len(wrong) else -1, n_perturbed=int((Ek != 0).sum()),
                argmin_abs=int(np.argmin(np.abs(D))), min_abs=float(np.abs(D).min()), max_abs=float(np.abs(D).max()),
                max_shift=float(np.abs(Ek).max()), pivot_min=float(pivot_min))


def identity_excess(Kp, L, D, perm, E):
    """max over the entries of |P'(Kp + diag(E))P - L D L'| - gamma_q |L||D||L'| (<= 0: the
    identity holds), gamma_q = q u / (1 - q u) with q = the longest row pattern of L plus 2: the
    standard backward-error bound of the up-looking recurrence (each entry of row k is an inner
    product of at most that many terms and one division)."""
    N = len(D)
    q = int(np.diff(L.tocsr().indptr).max()) + 2 if L.nnz else 2
    gamma = q * U / (1 - q * U)
    L1 = (L + sp.eye(N)).tocsc()
    A = (Kp + sp.diags(E)).tocsr()[perm][:, perm]
    R = abs(A - L1 @ sp.diags(D) @ L1.T)
    S = abs(L1) @ sp.diags(np.abs(D)) @ abs(L1).T
    return (R - gamma * S).max(), q


def same_report(a, b):
    return all(a[k] == b[k] for k in REPORT_FIELDS)
