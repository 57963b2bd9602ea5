"""The references of the exactly rounded residual against each other, on the CPU: the oracle's exact
inner product (resid_exact_ref.ref_row) equals rational arithmetic wherever that is the definition,
on every system and hand-built row the GPU test uses; and every system has rows whose exactly
rounded value differs from the plain entry-order residual, so the GPU comparison can tell the two
apart."""
import numpy as np
import pytest

import kkt_ref as R
import resid_exact_ref as E


@pytest.mark.parametrize("name", E.SYSTEMS)
def test_references_agree_and_differ_from_the_plain_sum(name):
    K = R.operator(name)
    for key, (z, b) in E.operands(name).items():
        exact, plain = E.reference(name, key)
        rows = np.arange(len(exact))
        if len(rows) > 600:  # rational arithmetic on a seeded sample of the large systems, the long row included
            rows = np.unique(np.concatenate([np.random.default_rng(7).choice(len(exact), 600, replace=False),
                                             [int(np.argmax(np.diff(K[0])))]]))
        sub = (K[0], K[1], K[2])
        for i in rows:
            lo, hi = sub[0][i], sub[0][i + 1]
            ok, v = E.ref_row_exact(b[i], sub[2][lo:hi], z[sub[1][lo:hi]])
            assert ok, (key, i)  # these systems neither under- nor overflow
            assert E.same(exact[i], v), (key, i, exact[i], v)
        assert np.all(np.isfinite(exact))
    # b = the plain product: the plain residual is zero everywhere, the exact one is not
    exact, plain = E.reference(name, "cancel")
    assert not np.any(plain) and np.any(exact != plain), name
    exact, plain = E.reference(name, "random")
    assert np.any(exact != plain), name


def test_long_row_is_in_the_family():
    """arrow_row's dense constraint is longer than the staging capacity (kSpmvCap = 2048)"""
    assert int(np.max(np.diff(R.operator("arrow_row")[0]))) > 2048


def test_hand_built_rows():
    H = E.hand()
    K, b, names = H["K"], H["b"], H["names"]
    row = {nm: i for i, nm in enumerate(names)}
    r = E.residual(K, H["z"], b)
    ok, v = E.residual_exact(K, H["z"], b)
    assert np.all(ok) and E.same(r, v)  # no product of the finite operand under- or overflows
    plain = R.residual(K, H["z"], b)
    # cancellation to the last bit: the plain sum loses the residual, the exact one keeps it
    i = row["cancel_to_last_bit"]
    assert r[i] != plain[i] and abs(r[i]) <= 2.0 ** -52 * abs(b[i]) and r[i] != 0.0
    # the ties, to even both ways
    assert r[row["tie_down"]] == 1.0 and r[row["tie_up"]] == 1.0 + 2.0 ** -51
    # 2^1000 and 2^-1000 in one row: the tiny term breaks the tie the plain sum never sees
    assert r[row["wide_exponents"]] == 1.0 + 2.0 ** -52 and plain[row["wide_exponents"]] != r[row["wide_exponents"]]
    # a partial sum beyond 2^1023, a finite total
    i = row["partial_overflow"]
    assert np.isfinite(r[i]) and r[i] == 1.5 * 2.0 ** 1023 and not np.isfinite(plain[i])
    assert r[row["subnormal"]] == 2.0 ** -1074 and r[row["subnormal_sum"]] == 7 * 2.0 ** -1074
    assert r[row["empty"]] == 0.75 and K[0][row["empty"] + 1] == K[0][row["empty"]]
    # inf and NaN in z: NaN exactly in the rows that store column 6 or 7
    rn = E.residual(K, H["z_nonfinite"], b)
    reads = np.array([bool(np.isin(K[1][K[0][i]:K[0][i + 1]], (6, 7)).any()) for i in range(len(rn))])
    assert reads.any() and not reads.all()
    assert np.array_equal(np.isnan(rn), reads) and E.same(rn[~reads], r[~reads])
