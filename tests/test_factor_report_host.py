"""The factor report and the static pivot perturbation of the host numeric phase (cpk.analyze):
the inertia and pivot information MA57's ldl returns with the factors (ops/opLDL2.m:81-82), and
the rule d -> s*delta for a pivot with s*d < delta under the engine option pivot_min = delta."""
import numpy as np
import pytest

import cpkrylov_amd as cpk
import factor_report_cases as FC


def _analyze(G, B, C22, **opts):
    return cpk.analyze(G, B, C22, options=opts or None)


def _check_report(an, n, pivot_min):
    want = FC.recomputed_report(an["D"], an["perm"], n, an["E"], pivot_min)
    assert an["report"] == want  # every field, ==


@pytest.mark.parametrize("name", FC.DEFAULT_NAMES)
def test_default_factor_report(name):
    G, B, C22 = FC.defaults()[name]
    n, m = G.shape[0], B.shape[0]
    an = _analyze(G, B, C22)
    _check_report(an, n, 0.0)
    r = an["report"]
    assert (r["n_pos"], r["n_neg"], r["n_wrong"], r["n_perturbed"]) == (n, m, 0, 0)
    assert r["first_wrong"] == -1 and r["max_shift"] == 0.0
    assert an["E"].shape == (n + m,) and not an["E"].any()
    a0 = _analyze(G, B, C22, pivot_min=0)  # given explicitly: the same bits
    assert np.array_equal(a0["perm"], an["perm"]) and np.array_equal(a0["D"], an["D"])
    assert np.array_equal(a0["L"].indptr, an["L"].indptr) and np.array_equal(a0["L"].data, an["L"].data)
    assert a0["report"] == r


def test_zeroed_g_entries_are_perturbed():
    G, G0, B, C22, dofs = FC.zeroed()
    n, m = G.shape[0], B.shape[0]
    Kp = FC.kp_of(G0, B, C22)
    sv = np.linalg.svd(Kp.toarray(), compute_uv=False)
    assert sv[-1] > 1e-9 * sv[0]  # Kp is nonsingular (cond ~ 1.7e6)
    with pytest.raises(cpk.CpkError) as e:
        _analyze(G0, B, C22)
    assert e.value.code == 6 and "pivot" in str(e.value)
    an = _analyze(G0, B, C22, pivot_min=FC.DELTA)
    r = an["report"]
    _check_report(an, n, FC.DELTA)
    assert r["n_perturbed"] == 3 and r["max_shift"] == FC.DELTA
    assert np.array_equal(np.flatnonzero(an["E"]), np.sort(dofs))
    assert np.all(an["E"][dofs] == FC.DELTA)  # d = 0 exactly: E = delta - 0
    assert (r["n_pos"], r["n_neg"], r["n_wrong"]) == (n, m, 0)
    excess, q = FC.identity_excess(Kp, an["L"], an["D"], an["perm"], an["E"])
    assert excess <= 0, (excess, q)


def test_negated_g_entry_is_reported_not_refused():
    G1, B, C22, dof = FC.negated()
    n = G1.shape[0]
    an = _analyze(G1, B, C22)  # no error
    r = an["report"]
    _check_report(an, n, 0.0)
    ev = np.linalg.eigvalsh(FC.kp_of(G1, B, C22).toarray())
    assert (r["n_pos"], r["n_neg"]) == (int((ev > 0).sum()), int((ev < 0).sum()))
    assert r["n_wrong"] == 1 and r["n_perturbed"] == 0
    assert r["first_wrong"] == int(np.flatnonzero(an["perm"] == dof)[0])


def test_delta_above_every_pivot_perturbs_all():
    G, B, C22 = FC.defaults()["cvxqp2_s"]
    n, m = G.shape[0], B.shape[0]
    delta = 2.0 * _analyze(G, B, C22)["report"]["max_abs"]
    an = _analyze(G, B, C22, pivot_min=delta)
    r = an["report"]
    _check_report(an, n, delta)
    assert r["n_perturbed"] == n + m
    assert np.array_equal(an["D"], np.where(an["perm"] < n, delta, -delta))
    excess, q = FC.identity_excess(FC.kp_of(G, B, C22), an["L"], an["D"], an["perm"], an["E"])
    assert excess <= 0, (excess, q)


def test_band_g_zero_c_factors_under_pivot_min():
    """No accuracy claim for the apply: the option does not substitute for C > 0."""
    G, B, C22 = FC.band_zero_c()
    n = G.shape[0]
    with pytest.raises(cpk.CpkError) as e:
        _analyze(G, B, C22)
    assert e.value.code == 6
    an = _analyze(G, B, C22, pivot_min=FC.DELTA)
    r = an["report"]
    _check_report(an, n, FC.DELTA)
    assert r["n_perturbed"] == np.count_nonzero(an["E"]) > 0
    excess, q = FC.identity_excess(FC.kp_of(G, B, C22), an["L"], an["D"], an["perm"], an["E"])
    assert excess <= 0, (excess, q)
