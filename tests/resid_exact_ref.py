"""The reference of the exactly rounded residual (cpk_kkt_residual_exact): r_i = RN(b_i - sum_e
K_ie z_col(e)), the exact sum of b_i and the TwoProd pairs of (-K_ie) * z_col(e), rounded once.

Two references for a row:
  ref_row       the oracle's exact inner product xdot([b_i, -vals...], [1.0, z...]) (b_i * 1.0 is an
                exact TwoProd), for every input: where a product under- or overflows both sides
                perform the same IEEE operations.
  ref_row_exact rational arithmetic (xacc_cases.ref_exact), the definition wherever
                xacc_cases.a_applies holds.
The hand-built system HAND forces each path of the kernel with chosen rows of A.  A plain module
(not a conftest); test infrastructure only, no product code."""
import numpy as np
import scipy.sparse as sp

import kkt_ref as R
import xacc_cases as X

SYSTEMS = ("tiny1x1", "tiny3x2", "tiny65x63", "empty_rows", "zero_c", "cvxqp1_m", "cvxqp2_s", "arrow_row")
_CACHE = {}


def ref_row(b_i, vals, z_cols):
    from oracle import oracle as O
    a = np.concatenate([[b_i], -np.asarray(vals, np.float64)])
    return O.xdot(a, np.concatenate([[1.0], np.asarray(z_cols, np.float64)]))


def ref_row_exact(b_i, vals, z_cols):
    """(applies, value) by rational arithmetic"""
    a = np.concatenate([[b_i], -np.asarray(vals, np.float64)])
    w = np.concatenate([[1.0], np.asarray(z_cols, np.float64)])
    if not X.a_applies(a, w):
        return False, None
    return True, X.ref_exact(a, w)


def residual(K, z, b):
    """the reference residual of K = (indptr, indices, data), row by row (the oracle)"""
    ptr, ind, val = K
    z, b = np.asarray(z, np.float64), np.asarray(b, np.float64)
    out = np.empty(len(ptr) - 1)
    for i in range(len(ptr) - 1):
        lo, hi = ptr[i], ptr[i + 1]
        out[i] = ref_row(b[i], val[lo:hi], z[ind[lo:hi]])
    return out


def residual_exact(K, z, b):
    """(mask of the rows where rational arithmetic is the definition, their values)"""
    ptr, ind, val = K
    ok, out = np.zeros(len(ptr) - 1, bool), np.zeros(len(ptr) - 1)
    for i in range(len(ptr) - 1):
        lo, hi = ptr[i], ptr[i + 1]
        ok[i], v = ref_row_exact(b[i], val[lo:hi], z[ind[lo:hi]])
        if ok[i]:
            out[i] = v
    return ok, out


def same(a, b):
    """== with NaN positions equal (kkt_ref.same_bits)"""
    return R.same_bits(a, b)


def operands(name):
    """{key: (z, b)} of a system: a random z against the system's right-hand side, and the same z
    against b = the plain product K*z, where the plain residual is 0.0 in every row and the exact
    one is the product's own rounding error."""
    if ("ops", name) not in _CACHE:
        P, K = R.system(name), R.operator(name)
        z = np.random.default_rng(4242).standard_normal(P["n"] + P["m"])
        _CACHE[("ops", name)] = {"random": (z, P["rhs"]), "cancel": (z, R.matvec(K, z))}
    return _CACHE[("ops", name)]


def reference(name, key):
    """(exact residual, plain residual) of an operand, computed once and shared"""
    if ("ref", name, key) not in _CACHE:
        z, b = operands(name)[key]
        K = R.operator(name)
        _CACHE[("ref", name, key)] = (residual(K, z, b), R.residual(K, z, b))
    return _CACHE[("ref", name, key)]


# ---- the hand-built system: n = 10, m = 3; the rows of A are the cases ----------------------------
HAND_N, HAND_M = 10, 3
_T = 2.0 ** 1023
# z: columns 0-3 are 1.0 (terms are the negated values themselves), 4-7 full significands
HAND_Z = np.array([1.0, 1.0, 1.0, 1.0, 1.0 / 3.0, -0.7, 1.1, 2.0 / 7.0, 0.0, 0.9, 0.0, 0.0, 0.0])
# row -> (name, {column: value}, b_i); a term is -value * z[column]
HAND_ROWS = [
    ("cancel_to_last_bit", {4: 3.3, 5: 0.17, 6: -2.9, 7: 1e-3}, None),  # b_i = RN(sum): set below
    ("tie_down", {0: 2.0 ** 60, 1: -2.0 ** 60, 2: -2.0 ** -53}, 1.0),  # 1 + 2^-53 -> 1 (even)
    ("tie_up", {0: 2.0 ** 60, 1: -2.0 ** 60, 2: -2.0 ** -53}, 1.0 + 2.0 ** -52),  # 1 + 3 2^-53 -> 1 + 2^-51
    ("wide_exponents", {0: -2.0 ** 1000, 1: -1.0, 2: -2.0 ** -500, 3: 2.0 ** 1000, 4: -3.0 * 2.0 ** -1000},
     2.0 ** -53),  # four live magnitudes: the cascade leaves a residue; 1 + 2^-53 + tiny -> 1 + 2^-52
    ("partial_overflow", {0: -1.5 * _T, 1: -1.5 * _T, 2: 1.5 * _T, 5: 0.3}, 1.0),  # total 1.5 2^1023 + ...
    ("subnormal", {0: 2.0 ** -1022 * (1 - 2.0 ** -52)}, 2.0 ** -1022),  # r = 2^-1074
    ("subnormal_sum", {0: -3 * 2.0 ** -1074, 1: 2.0 ** -1074, 4: 0.0}, 5 * 2.0 ** -1074),
    ("reads_nonfinite", {6: 0.5, 7: 0.25, 0: 1.0}, 1.0),  # finite with HAND_Z; NaN with HAND_Z_NONFINITE
    ("empty", {}, 0.75),
    ("plain", {9: 2.0, 0: 1.0}, 0.1),
]
HAND_Z_NONFINITE = HAND_Z.copy()
HAND_Z_NONFINITE[6], HAND_Z_NONFINITE[7] = np.inf, np.nan


def hand():
    """dict(A, B, C, n, m, K, z, z_nonfinite, b, names): variable 8 is isolated (row 8 of K is empty)"""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    n, m = HAND_N, HAND_M
    rows, cols, vals = [], [], []
    for i, (_, ent, _) in enumerate(HAND_ROWS):
        for c in sorted(ent):
            rows.append(i), cols.append(c), vals.append(ent[c])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))  # explicit zeros kept
    B = sp.csr_matrix(([0.5, -0.25, 1.5, 0.75, -1.25, 2.0], ([0, 0, 1, 1, 2, 2], [0, 1, 2, 6, 4, 5])), shape=(m, n))
    Cm = sp.csr_matrix(sp.diags([1e-3, 2e-3, 3e-3]))
    K = R.assemble(A, B, Cm)
    b = np.array([row[2] if row[2] is not None else 0.0 for row in HAND_ROWS] + [0.3, -0.6, 0.9])
    # cancellation to the last bit: b_0 is the correctly rounded sum of row 0's products
    lo, hi = K[0][0], K[0][1]
    b[0] = -ref_row(0.0, K[2][lo:hi], HAND_Z[K[1][lo:hi]])
    _CACHE["hand"] = dict(A=A, B=B, C=Cm, n=n, m=m, K=K, z=HAND_Z, z_nonfinite=HAND_Z_NONFINITE, b=b,
                          names=[r[0] for r in HAND_ROWS])
    return _CACHE["hand"]
