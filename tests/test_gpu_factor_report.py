"""The factor report and the static pivot perturbation on the device (ldl.hip: the REG
instantiations of the row kernels, ldl_report_kernel) against the host numeric phase, bit for bit;
refactorization, refinement against the unperturbed Kp, a solve end to end, the distributed
preconditioner and the MEX gateway.  Stands in for the inertia and pivot information MA57's ldl
returns with the factors (ops/opLDL2.m:81-82)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import factor_report_cases as FC
import fixtures as F
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _dense_col_delta():
    """The quantile of |D| of dense_col's default factor at which both row kernels see perturbed
    and unperturbed pivots (the median perturbs every long row)."""
    import cpkrylov_amd as cpk
    G, B, C22 = FC.dense_col()
    return float(np.quantile(np.abs(cpk.analyze(G, B, C22)["D"]), 0.25))


def _cases():
    out = [(name,) + FC.defaults()[name] + ({},) for name in FC.DEFAULT_NAMES]
    G, G0, B, C22, _ = FC.zeroed()
    out.append(("zeroed", G0, B, C22, dict(pivot_min=FC.DELTA)))
    G1, B1, C1, _ = FC.negated()
    out.append(("negated", G1, B1, C1, {}))
    out.append(("band_g_zero_c", *FC.band_zero_c(), dict(pivot_min=FC.DELTA)))
    return out


CASES = _cases()


def _device(G, B, C22, opts):
    import cpkrylov_amd as cpk
    with cpk.engine_options(**opts):
        return cpk.opLDL2(G, B, C22)


def _assert_equals_host(M, G, B, C22, opts):
    import cpkrylov_amd as cpk
    H = cpk.analyze(G, B, C22, options=opts or None)
    L, D, perm = M.export_factors()
    assert np.array_equal(perm, H["perm"])
    assert np.array_equal(L.indptr, H["L"].indptr) and np.array_equal(L.indices, H["L"].indices)
    assert np.array_equal(L.data, H["L"].data)
    assert np.array_equal(D, H["D"])
    assert np.array_equal(M.pivot_shift(), H["E"])
    assert M.factor_report() == H["report"]
    return H, L


@pytest.mark.parametrize("name,G,B,C22,opts", CASES, ids=[c[0] for c in CASES])
def test_device_equals_host(gpu_ctx, name, G, B, C22, opts):
    _assert_equals_host(_device(G, B, C22, opts), G, B, C22, opts)


def test_device_equals_host_all_perturbed(gpu_ctx):
    import cpkrylov_amd as cpk
    G, B, C22 = FC.defaults()["cvxqp2_s"]
    opts = dict(pivot_min=2.0 * cpk.analyze(G, B, C22)["report"]["max_abs"])
    M = _device(G, B, C22, opts)
    _assert_equals_host(M, G, B, C22, opts)
    assert M.factor_report()["n_perturbed"] == M.n


def test_device_equals_host_both_kernels(gpu_ctx):
    """dense_col: rows of at least 48 pattern entries (one wave per row) and shorter ones (one
    thread per row) each hold perturbed and unperturbed pivots."""
    G, B, C22 = FC.dense_col()
    opts = dict(pivot_min=_dense_col_delta())
    M = _device(G, B, C22, opts)
    H, L = _assert_equals_host(M, G, B, C22, opts)
    rows = np.diff(L.tocsr().indptr)
    pert = H["E"][H["perm"]] != 0
    for long in (rows >= 48, rows < 48):
        assert (pert & long).any() and (~pert & long).any()


def test_fresh_option_string(gpu_ctx):
    import cpkrylov_amd as cpk
    ctx = cpk.Context()
    try:
        assert "pivot_min=0;" in ctx.options_string() and ctx.get_option("pivot_min") == "0"
        ctx.set_option("pivot_min", 1e-9)
        assert "pivot_min=1.0000000000000001e-09;" in ctx.options_string()
        for bad in ("-1", "nan", "inf", "abc"):
            with pytest.raises(cpk.CpkError) as e:
                ctx.set_option("pivot_min", bad)
            assert e.value.code == 3
    finally:
        ctx.close()


def _state(M, z):
    L, D, _ = M.export_factors()
    return L.data.copy(), D, M.pivot_shift(), M.factor_report(), M * z


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and np.array_equal(a[4], b[4])


def test_refactor_under_pivot_min(gpu_ctx):
    import cpkrylov_amd as cpk
    G, G0, B, C22, dofs = FC.zeroed()
    z = np.random.default_rng(4).standard_normal(G.shape[0] + B.shape[0])
    M = cpk.opLDL2(G, B, C22)
    M.nitref, M.force_itref = 1, True
    assert M.factor_report()["pivot_min"] == 0.0 and not M.pivot_shift().any()
    with cpk.engine_options(pivot_min=FC.DELTA):
        M.refactor(G0, B, C22)
        M2 = cpk.opLDL2(G0, B, C22)
        M2.nitref, M2.force_itref = 1, True
        s1 = _state(M, z)
        assert _same_state(s1, _state(M2, z))  # a fresh construction on those values, bit for bit
        assert s1[3]["n_perturbed"] == 3 and s1[3]["pivot_min"] == FC.DELTA
    # the option raised between two refactorizations of the same handle
    with cpk.engine_options(pivot_min=1e-7):
        M.refactor(G0, B, C22)
        s2 = _state(M, z)
        assert s2[3]["pivot_min"] == 1e-7 and s2[3]["n_perturbed"] > 3
        assert s2[3]["n_perturbed"] == np.count_nonzero(s2[2])
        # a NaN in G: raises, and everything stays
        Gn = G0.copy()
        Gn.data[Gn.indptr[dofs[0]]] = np.nan
        with pytest.raises(cpk.CpkError) as e:
            M.refactor(Gn, B, C22)
        assert e.value.code == 6 and "pivot" in str(e.value)
        assert _same_state(s2, _state(M, z))
    # back to the default: the shifts are gone with the option
    M.refactor(G, B, C22)
    assert not M.pivot_shift().any() and M.factor_report()["n_perturbed"] == 0
    M0 = cpk.opLDL2(G, B, C22)
    M0.nitref, M0.force_itref = 1, True
    assert _same_state(_state(M, z), _state(M0, z))


def test_refinement_uses_the_unperturbed_kp(gpu_ctx):
    G, G0, B, C22, _ = FC.zeroed()
    Kp = FC.kp_of(G0, B, C22)
    z = np.random.default_rng(9).standard_normal(Kp.shape[0])
    M = _device(G0, B, C22, dict(pivot_min=FC.DELTA))
    M.nitref, M.force_itref = 1, True
    y1 = M * z
    Mo = O.LDL2(G0, B, C22, factors=M.export_factors())  # its own Kp from the unperturbed blocks
    Mo.set(nitref=1.0, force_itref=1.0)
    assert np.array_equal(y1, Mo @ z)
    Kc = Kp.tocsr()
    Kc.sort_indices()
    kz = np.zeros(Kc.shape[0])  # MATLAB order: per row, 0 + a1*x1 + a2*x2 + ... (no FMA)
    for i in range(Kc.shape[0]):
        acc = 0.0
        for p in range(Kc.indptr[i], Kc.indptr[i + 1]):
            acc = acc + Kc.data[p] * z[Kc.indices[p]]
        kz[i] = acc
    assert np.array_equal(M.divide(z), kz)
    M.nitref = 0
    y0 = M * z
    x = spla.spsolve(Kp.tocsc(), z)
    e0, e1 = (np.linalg.norm(y - x) / np.linalg.norm(x) for y in (y0, y1))
    print(f"relative error of M*z against spsolve(Kp, z): nitref=0 {e0:.3e}, one forced step {e1:.3e}")
    assert e1 < e0


def test_solve_end_to_end_exact(gpu_ctx):
    import cpkrylov_amd as cpk
    G, G0, B, C22, _ = FC.zeroed()
    P = dict(F.load("cvxqp2_s"))
    P["G"] = G0
    opts = dict(F.EXPROG_OPTS)
    with cpk.engine_options(exact_dots=1, pivot_min=FC.DELTA):
        x, stats, flag = cpk.reg_cpkrylov(cpk.cpminres, P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts)
        factors = stats["M"].export_factors()
        assert stats["M"].factor_report()["n_perturbed"] == 3
    Mo = O.LDL2(P["G"], P["B"], -P["C"], factors=factors)
    Mo.set(**{k: float(opts[k]) for k in ("nitref", "itref_tol", "force_itref", "residual_update") if k in opts})
    with O.exact():
        xo, so = O.reg_solve("minres", P["rhs"], P["Q"], P["B"], P["C"], Mo, opts)
    assert stats["niters"] == so["niters"] and flag["solved"] == so["solved"]
    for k in [k for k in so if k.endswith("History")]:
        assert np.array_equal(stats[k], so[k]), k
    assert np.array_equal(x, xo)


def test_distributed_report_equals_single_gpu(gpu_ctx):
    import cpkrylov_amd as cpk
    from test_gpu_dist import _run_ranks
    G, G0, B, C22, _ = FC.zeroed()
    z = np.random.default_rng(5).standard_normal(G.shape[0] + B.shape[0])
    opts = dict(pivot_min=FC.DELTA)

    def work(ctx, r):
        M = cpk.opLDL2(G0, B, C22, ctx=ctx)
        M.nitref, M.force_itref = 1, True
        return M.factor_report(), M.pivot_shift(), M * z

    res = _run_ranks(2, work, opts)
    M1 = _device(G0, B, C22, opts)
    M1.nitref, M1.force_itref = 1, True
    rep, E, y = M1.factor_report(), M1.pivot_shift(), M1 * z
    assert rep["n_perturbed"] == 3
    for rr, Er, yr in res:
        assert rr == rep and np.array_equal(Er, E) and np.array_equal(yr, y)


def test_mex_factor_report(gpu_ctx):
    import cpkrylov_amd as cpk
    from test_mex_shim import _gpu_mex
    mex = _gpu_mex()
    G1, B, C22, _ = FC.negated()  # a report with a wrong-signed pivot under the gateway's default options
    h = mex.value(mex(1, "pc_create", G1, B, C22)[0])
    try:
        rep, E = mex(2, "pc_factor_report", h)
        M = cpk.opLDL2(G1, B, C22)
        want = M.factor_report()
        assert want["n_wrong"] == 1
        for k in FC.REPORT_FIELDS:
            assert mex.field(rep, k)[0] == want[k], k
        assert np.array_equal(mex.value(E), M.pivot_shift())
        mex.L.shim_destroy(rep), mex.L.shim_destroy(E)
        (rep,) = mex(1, "pc_factor_report", h)  # the report alone
        assert mex.field(rep, "n_neg")[0] == want["n_neg"]
        mex.L.shim_destroy(rep)
    finally:
        mex(0, "pc_destroy", h)
        mex.L.shim_destroy(h.a)
