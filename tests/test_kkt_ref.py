"""The reference of the saddle-point operator tests (tests/kkt_ref.py) proved on its own: against
exact rational arithmetic on the tiny members, against scipy's product within the rounding bound of
any summation order on the others, and that a transposed (1,1) block cannot pass (no GPU)."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_ref as R


def _fraction_matvec(K, z):
    """Every operation rounded once, the rounding done by Fraction -> float (correctly rounded):
    p = fl(K_ij * z_j), s = fl(s + p), in entry order from 0."""
    ptr, ind, val = K
    out = np.zeros(len(ptr) - 1)
    for i in range(len(ptr) - 1):
        s = 0.0
        for e in range(ptr[i], ptr[i + 1]):
            p = float(Fraction(float(val[e])) * Fraction(float(z[ind[e]])))
            s = float(Fraction(s) + Fraction(p))
        out[i] = s
    return out


@pytest.mark.parametrize("name", R.TINY)
def test_reference_equals_rational_arithmetic(name):
    K = R.operator(name)
    P = R.system(name)
    for key, z in R.operands(name).items():
        if key == "nan":
            continue
        s = R.matvec(K, z)
        assert R.same_bits(s, _fraction_matvec(K, z)), key
        r = R.residual(K, z, P["rhs"])
        want = np.array([float(Fraction(float(b)) - Fraction(float(v))) for b, v in zip(P["rhs"], s)])
        assert R.same_bits(r, want), key


@pytest.mark.parametrize("name", [n for n in R.MEMBERS if n not in R.TINY])
def test_reference_within_rounding_of_scipy(name):
    K = R.operator(name)
    Ks = R.as_scipy(K)
    P = R.system(name)
    want = sp.bmat([[P["A"], P["B"].T], [P["B"], -P["C"]]]).tocsr()
    assert (abs(Ks - want)).max() == 0 and Ks.nnz == P["A"].nnz + 2 * P["B"].nnz + P["C"].nnz
    q = int(np.max(np.diff(K[0])))
    z = R.operands(name)["random"]
    bound = R.gamma(q) * (abs(Ks) @ np.abs(z))
    assert np.all(np.abs(R.matvec(K, z) - Ks @ z) <= bound)


def test_entry_order_is_the_assembly_order():
    """Row i < n: A's entries (columns < n ascending), then B''s by ascending constraint; row n + i:
    B's entries, then -C's: every row ascending, explicit zeros of C kept (zero_c has none)."""
    for name in ("tiny2x1", "empty_rows", "zero_c"):
        ptr, ind, val = R.operator(name)
        P = R.system(name)
        for i in range(len(ptr) - 1):
            assert np.all(np.diff(ind[ptr[i]:ptr[i + 1]]) > 0)
        n = P["n"]
        assert ptr[n] == P["A"].nnz + P["B"].nnz


def test_transposed_block_cannot_pass():
    K = R.operator("cvxqp2_s")
    Ks = R.as_scipy(K)
    z = R.operands("cvxqp2_s")["random"]
    assert np.any(Ks @ z != Ks.T @ z)
    n = R.system("cvxqp2_s")["n"]
    assert np.any((Ks @ z)[:n] != (Ks.T @ z)[:n])


def test_nan_stays_in_its_rows():
    K = R.operator("tiny65x63")
    z = R.operands("tiny65x63")["nan"]
    s = R.matvec(K, z)
    j = int(np.flatnonzero(np.isnan(z))[0])
    touched = np.array([j in K[1][K[0][i]:K[0][i + 1]] for i in range(len(s))])
    assert np.array_equal(np.isnan(s), touched)
