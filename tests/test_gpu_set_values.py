"""In-place value updates on the device (cpk_mat_set_values, cpk_mat_set_values_device): the outer
iteration of an interior-point method, which rebuilds opLDL2 from new values of the same sparsity
once per iteration (reg_cpkrylov.m:131), on one set of handles.

Every comparison is bit for bit against handles freshly created from the new values on the same
device: the same layout and the same grids give the same bits.

  1. A @ x (cpk_mat_spmv) after a host update before and after the first device use and after a
     device update (a DeviceArray and, where torch sees the GPU, a torch tensor), for handles created
     from CSC, unsorted CSR and CSR with duplicates;
  2. three outer iterations on one set of handles and one opLDL2: factors, M * z, x, y, niters and
     the history of cpminres and cpcg through the device entries equal a fresh construction's, the
     cached solvers instantiate no further graph from the second iteration on, and the handle
     keeps one Krylov operator -- for the single-column and the block entry, and once under
     exact_dots;
  3. pairings: one C with two A handles, one handle as both A and G, an update without a
     refactorization, and a new opLDL2 from device-updated handles (the host copy follows);
  4. a failed refactorization after a good update, and the refusals (a wrong count, a distributed
     context), which leave everything untouched.

The iteration limit of case 2: the solvers replay captured graphs of 16 iterations and, once a
first batch has not converged, choose later batch sizes from the observed convergence rate
(solvers.hip, SolveCore::loop), so under new values a new batch size is a legitimately new graph.
With at most 12 iterations every solve is exactly one batch of 16, so the set of graphs is fixed by
construction and "no further instantiation" is a property of the cache alone.  The last iteration
also solves to convergence (itmax = 500), compared for equality only."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

try:  # before libcpk initialises HIP
    import torch
    _TORCH = torch.cuda.is_available()
except Exception:  # noqa: BLE001
    _TORCH = False

import fixtures as F
import structures as ST
from devbuf import DeviceArray
from rawmat import duplicated_csr, raw_matrix, unsorted_csr

pytestmark = pytest.mark.gpu

SYSTEMS = ("tiny1x1", "tiny65x63", "zero_c", "arrow_row", "cvxqp1_m")
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
OPTS = dict(F.EXPROG_OPTS)
SHORT = dict(OPTS, itmax=12)
K = 8


def system(name):
    return F.load(name) if name == "cvxqp1_m" else ST.get(name)


def new_values(S, it):
    """Iteration `it`'s matrices: seeded, the same sparsity, still factorable -- the update of
    test_gpu_factor.py::test_refactor_equals_fresh_construction (G's diagonal rescaled in
    (0.5, 2), B's entries in (0.8, 1.25), C times a constant), and Q scaled symmetrically, D Q D
    with D in (0.8, 1.25), which keeps it symmetric positive definite"""
    rng = np.random.default_rng(1700 + it)
    G, B, Cm, Q = (S[k].copy() for k in ("G", "B", "C", "Q"))
    G.data = G.data * rng.uniform(0.5, 2.0, G.nnz)
    B.data = B.data * rng.uniform(0.8, 1.25, B.nnz)
    Cm.data = Cm.data * (1.5 + it)
    d = rng.uniform(0.8, 1.25, Q.shape[0])
    Q = sp.csr_matrix(Q, dtype=np.float64)
    Q.data = Q.data * d[np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))] * d[Q.indices]
    return dict(G=G, B=B, C=Cm, Q=Q)


def canon(M):
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return M


def neg(M):
    M = canon(M)
    return sp.csr_matrix((-M.data, M.indices, M.indptr), shape=M.shape)


def give(h, v, mode, keep):
    """hand the values v (the creating call's order) to handle h: "host", "dev" (a DeviceArray's
    pointer) or "torch" (a tensor, where torch sees the GPU; else the DeviceArray)"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    if mode == "host":
        h.set_values(v)
    elif mode == "torch" and _TORCH:
        t = torch.from_numpy(v.copy()).cuda()
        h.set_values(t)
        t.zero_()  # the call has consumed it
    else:
        d = DeviceArray.of(v)
        keep.append(d)
        h.set_values_device(d.p.value, v.size)


# ---- 1. A @ x --------------------------------------------------------------------------------------
def _raw(kind, S, v, rng_seed):
    """(kind, shape, ptr, ind, values in the creating call's order) of scipy CSR S carrying v"""
    S = canon(S)
    if kind == "csc":
        T = sp.csr_matrix((np.arange(S.nnz, dtype=np.float64), S.indices, S.indptr), shape=S.shape).tocsc()
        T.sort_indices()
        order = T.data.astype(np.int64)
        return "csc", S.shape, T.indptr, T.indices, v[order]
    if kind == "unsorted":
        ptr, ind, order = unsorted_csr(S)
        return "csr", S.shape, ptr, ind, v[order]
    ptr, ind, split = duplicated_csr(S, np.random.default_rng(5))
    return "csr", S.shape, ptr, ind, split(v, np.random.default_rng(rng_seed))


def _spmv_matrix(name):
    S = system(name)
    return S["C"] if name == "zero_c" else S["B"]  # zero_c: a matrix without entries (count == 0)


@pytest.mark.parametrize("kind", ("csc", "unsorted", "duplicates"))
@pytest.mark.parametrize("name", SYSTEMS)
def test_spmv_after_update(gpu_ctx, name, kind):
    S = canon(_spmv_matrix(name))
    rng = np.random.default_rng(11)
    x = rng.standard_normal(S.shape[1])
    vals = [S.data * rng.uniform(0.5, 2.0, S.nnz) for _ in range(5)]
    raws = [_raw(kind, S, v, 20 + i) for i, v in enumerate(vals)]
    k, shape, ptr, ind, v0 = raws[0]
    fresh = [raw_matrix(k, shape, ptr, ind, r[4], ctx=gpu_ctx) @ x for r in raws]
    keep = []
    h = raw_matrix(k, shape, ptr, ind, v0, ctx=gpu_ctx)
    give(h, raws[1][4], "host", keep)  # before the first device use
    assert h.info()["device_copy"] is False
    assert np.array_equal(h @ x, fresh[1])
    assert h.info()["device_copy"] is True
    give(h, raws[2][4], "host", keep)  # after it
    assert np.array_equal(h @ x, fresh[2])
    give(h, raws[3][4], "dev", keep)
    assert np.array_equal(h @ x, fresh[3])
    give(h, raws[4][4], "torch", keep)
    assert np.array_equal(h @ x, fresh[4])
    give(h, raws[0][4], "host", keep)  # a host update over values that came from the device
    assert np.array_equal(h @ x, fresh[0])
    assert h.info()["values_generation"] == 5
    # a device update before the first device use
    h2 = raw_matrix(k, shape, ptr, ind, v0, ctx=gpu_ctx)
    give(h2, raws[3][4], "dev", keep)
    assert np.array_equal(h2 @ x, fresh[3])
    if S.nnz and kind != "duplicates":  # (a lone 1e16, w, -1e16 triple may sum to 0 both times)
        assert not np.array_equal(fresh[0], fresh[1])


def test_many_sources_and_block_edges(gpu_ctx):
    """the value kernel's shapes: an entry summed from 1000 sources, and stored entry counts
    around its block size (256) and a multiple of it"""
    import cpkrylov_amd as cpk
    rng = np.random.default_rng(9)
    x = np.ones(1)
    ind = np.zeros(1000, np.int32)
    h = raw_matrix("csr", (1, 1), [0, 1000], ind, np.ones(1000), ctx=gpu_ctx)
    assert h @ x == 1000.0
    v = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    d = DeviceArray.of(v)
    h.set_values_device(d.p.value, 1000)
    assert np.array_equal(h @ x, raw_matrix("csr", (1, 1), [0, 1000], ind, v, ctx=gpu_ctx) @ x)
    for nnz in (1, 255, 256, 257, 1024, 1031):
        rows, cols = np.divmod(rng.permutation(1600)[:nnz], 40)
        D = canon(sp.csr_matrix((np.ones(nnz), (rows, cols)), shape=(40, 40)))
        T = D.tocsc()
        v = rng.standard_normal(nnz)
        xx = rng.standard_normal(40)
        h = cpk.Matrix(D, ctx=gpu_ctx, csc=True)
        dv = DeviceArray.of(v)
        h.set_values_device(dv.p.value, nnz)
        want = cpk.Matrix(sp.csc_matrix((v, T.indices, T.indptr), shape=T.shape), ctx=gpu_ctx, csc=True) @ xx
        assert np.array_equal(h @ xx, want), nnz


# ---- 2. outer iterations ---------------------------------------------------------------------------
class Outer:
    """the handles of one system, its preconditioner and its fixed device buffers"""

    def __init__(self, cpk, ctx, V, b, kb):
        self.cpk, self.ctx = cpk, ctx
        self.A, self.Cm, self.G, self.B, self.Cn = (cpk.Matrix(M, ctx=ctx) for M in (V["Q"], V["C"], V["G"], V["B"], neg(V["C"])))
        self.M = cpk.opLDL2(self.G, self.B, self.Cn, ctx=ctx)
        self.M._set(**{k: OPTS[k] for k in PC_PROPS})
        self.n, self.m, self.N = self.A.shape[0], self.Cm.shape[0], self.M.n
        # zeroed, so that a solve the reference's error stops (CPK_ERR_INDEFINITE on a residual that
        # is pure rounding, structures.py) compares equal too: such a solve writes nothing
        self.db, self.dxy = DeviceArray.of(b), DeviceArray.of(np.zeros(self.N))
        self.dB, self.dXY = DeviceArray.of(kb.T), DeviceArray.of(np.zeros(self.N * K))

    def solve(self, method, opts):
        """(rc, xy, niters, history) through cpk_method_solve_device on the fixed buffers"""
        from cpkrylov_amd import _lib, api
        st, hist, _, _ = api._new_stats(api._hist_cap(method, opts, self.n, self.m))
        rc = _lib.lib.cpk_method_solve_device(self.ctx.h, _lib.METHODS[method], self.db.p, self.A.h, self.Cm.h, self.M.h,
                                              C.byref(_lib.make_opts(opts)), self.dxy.p, C.byref(st))
        self.ctx.synchronize()
        return rc, self.dxy.numpy(), int(st.niters), hist[:st.hist_len].copy()

    def solve_block(self, method, opts):
        from cpkrylov_amd import _lib, api
        cap = api._hist_cap(method, opts, self.n, self.m)
        sts = (_lib.Stats * K)()
        hists = [np.zeros(cap) for _ in range(K)]
        for j in range(K):
            sts[j].hist, sts[j].hist_cap = hists[j].ctypes.data_as(C.POINTER(C.c_double)), cap
        status = (C.c_int * K)()
        rc = _lib.lib.cpk_method_solve_multi_device(self.ctx.h, _lib.METHODS[method], K, self.dB.p, max(self.n, 1), self.A.h,
                                                    self.Cm.h, self.M.h, C.byref(_lib.make_opts(opts)), self.dXY.p,
                                                    max(self.N, 1), sts, status)
        self.ctx.synchronize()
        return (rc, list(status), self.dXY.numpy(), [int(s.niters) for s in sts],
                [hists[j][:sts[j].hist_len].copy() for j in range(K)])


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def rhs(S):
    n = S["n"]
    rng = np.random.default_rng(23)
    b = S["rhs"][:n].copy()
    if n <= 65:  # the tiny members: a seeded first column, as test_gpu_solve_multi.py's TINY_COLUMNS
        b = np.random.default_rng(1013).standard_normal(n) if n > 1 else np.array([7.0])
    kb = np.column_stack([b, 1e-3 * b] + [rng.standard_normal(n) for _ in range(K - 2)])
    return b, np.asfortranarray(kb)


def run_outer(cpk, ctx, name, block):
    S = system(name)
    b, kb = rhs(S)
    z = np.random.default_rng(31).standard_normal(S["n"] + S["m"])
    keep = []
    O = Outer(cpk, ctx, {k: canon(S[k]) for k in ("Q", "C", "G", "B")}, b, kb)
    solve = O.solve_block if block else O.solve
    counts = []
    for it, mode in enumerate(("host", "dev", "torch")):
        V = new_values(S, it)
        give(O.A, canon(V["Q"]).data, mode, keep)
        give(O.Cm, canon(V["C"]).data, mode, keep)
        give(O.Cn, neg(V["C"]).data, mode, keep)
        give(O.G, canon(V["G"]).data, mode, keep)
        if it == 1:
            give(O.B, canon(V["B"]).data, mode, keep)
        else:
            V["B"] = new_values(S, 1)["B"] if it > 1 else S["B"]
        O.M.refactor(O.G, O.B, O.Cn)
        Fr = Outer(cpk, ctx, V, b, kb)  # fresh matrices, a fresh opLDL2, fresh buffers
        fsolve = Fr.solve_block if block else Fr.solve
        (L, D, perm), (L2, D2, perm2) = O.M.export_factors(), Fr.M.export_factors()
        assert np.array_equal(perm, perm2) and np.array_equal(L.data, L2.data) and np.array_equal(D, D2), it
        assert np.array_equal(O.M * z, Fr.M * z), it
        for method in ("minres", "cg"):
            got, want = solve(method, SHORT), fsolve(method, SHORT)
            assert same(got, want), (it, method, got[0], want[0])
            if name in ("cvxqp1_m", "arrow_row"):  # these solve: the comparison is of real iterations
                assert got[0] == 0 and np.min(got[-2]) >= 1, (it, method, got[0], got[-2])
        info = O.M.solver_info()
        counts.append((info["graph_instantiations"], info["block_graph_instantiations"]))
        assert O.A.info()["krylov_operators"] == 1 and O.A.info()["values_generation"] == it + 1
        if it == 2:  # to convergence, for equality
            for method in ("minres", "cg"):
                assert same(solve(method, OPTS), fsolve(method, OPTS)), method
    used = counts[0][1 if block else 0]
    if name != "tiny1x1":  # (one dof: a solve may stop before its first batch)
        assert used >= 1, counts  # graphs were captured in the first iteration ...
    assert counts[1] == counts[0] and counts[2] == counts[0], counts  # ... and none later
    info = O.M.solver_info()
    assert (info["block_solvers"] == 2) if block else (info["solvers"] == 2), info


@pytest.mark.parametrize("block", (False, True), ids=("single", "block"))
@pytest.mark.parametrize("name", SYSTEMS)
def test_outer_iterations(gpu_ctx, name, block):
    import cpkrylov_amd as cpk
    run_outer(cpk, gpu_ctx, name, block)


def test_outer_iterations_exact_dots(gpu_ctx):
    import cpkrylov_amd as cpk
    with cpk.engine_options(exact_dots=1):
        run_outer(cpk, gpu_ctx, "tiny65x63", False)
        run_outer(cpk, gpu_ctx, "tiny65x63", True)


# ---- 3. pairings and preconditioners ------------------------------------------------------------------
def test_one_c_paired_with_two_a(gpu_ctx):
    import cpkrylov_amd as cpk
    S = system("cvxqp1_m")
    b, kb = rhs(S)
    V0, V1 = {k: canon(S[k]) for k in ("Q", "C", "G", "B")}, new_values(S, 0)
    O = Outer(cpk, gpu_ctx, V0, b, kb)
    A1, A2 = O.A, cpk.Matrix(V1["Q"], ctx=gpu_ctx)
    before = {}
    for key, A in (("a1", A1), ("a2", A2)):
        O.A = A
        before[key] = O.solve("minres", OPTS)
    assert A1.info()["krylov_operators"] == 1 and A2.info()["krylov_operators"] == 1
    keep = []
    give(O.Cm, canon(V1["C"]).data, "dev", keep)  # C alone, neither A; the preconditioner follows C
    give(O.Cn, neg(V1["C"]).data, "dev", keep)    # (a constraint preconditioner holds the operator's -C)
    O.M.refactor(O.G, O.B, O.Cn)
    Fr = Outer(cpk, gpu_ctx, dict(V0, C=V1["C"]), b, kb)
    Fr.M, Fr.Cn = O.M, O.Cn
    for key, A, Q in (("a1", A1, V0["Q"]), ("a2", A2, V1["Q"])):
        O.A, Fr.A = A, cpk.Matrix(Q, ctx=gpu_ctx)
        got, want = O.solve("minres", OPTS), Fr.solve("minres", OPTS)
        assert same(got, want) and got[0] == 0, (key, got[0], want[0])
        assert not np.array_equal(got[1], before[key][1]), key  # C's new values did reach this pairing
    assert A1.info()["krylov_operators"] == 1 and A2.info()["krylov_operators"] == 1


def test_one_handle_as_a_and_g(gpu_ctx):
    import cpkrylov_amd as cpk
    S = system("cvxqp1_m")
    b, kb = rhs(S)
    V0, V1 = {k: canon(S[k]) for k in ("Q", "C", "G", "B")}, new_values(S, 0)
    O = Outer(cpk, gpu_ctx, dict(V0, Q=V0["G"]), b, kb)
    O.A = O.G  # the same handle in the Krylov operator and in the preconditioner
    O.solve("cg", OPTS)
    keep = []
    give(O.G, canon(V1["G"]).data, "dev", keep)
    O.M.refactor(O.G, O.B, O.Cn)
    Fr = Outer(cpk, gpu_ctx, dict(V0, Q=V1["G"], G=V1["G"]), b, kb)
    for method in ("minres", "cg"):
        got = O.solve(method, OPTS)
        assert same(got, Fr.solve(method, OPTS)) and got[0] == 0, (method, got[0])
    assert same(O.M.export_factors()[1], Fr.M.export_factors()[1])


def test_update_without_refactor_leaves_the_preconditioner(gpu_ctx):
    import cpkrylov_amd as cpk
    S = system("cvxqp1_m")
    b, kb = rhs(S)
    V0, V1 = {k: canon(S[k]) for k in ("Q", "C", "G", "B")}, new_values(S, 0)
    O = Outer(cpk, gpu_ctx, V0, b, kb)
    z = np.random.default_rng(2).standard_normal(O.N)
    y0, k0, (L0, D0, _) = O.M * z, O.M.divide(z), O.M.export_factors()
    keep = []
    for mode in ("host", "dev"):
        give(O.G, canon(V1["G"]).data, mode, keep)
        give(O.B, canon(V1["B"]).data, mode, keep)
        L1, D1, _ = O.M.export_factors()
        assert np.array_equal(O.M * z, y0) and np.array_equal(O.M.divide(z), k0)
        assert np.array_equal(L1.data, L0.data) and np.array_equal(D1, D0)
    O.M.refactor(O.G, O.B, O.Cn)
    assert not np.array_equal(O.M * z, y0)


@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_new_preconditioner_from_device_updated_handles(gpu_ctx, name):
    """the host-coherence case: cpk_pc_create, cpk_analyze and a first blkdiag(A, C) read the host
    copies, which an update from device memory left behind"""
    import cpkrylov_amd as cpk
    S = system(name)
    b, kb = rhs(S)
    V0, V1 = {k: canon(S[k]) for k in ("Q", "C", "G", "B")}, new_values(S, 0)
    keep = []
    hs = {k: cpk.Matrix(M, ctx=gpu_ctx) for k, M in (("Q", V0["Q"]), ("C", V0["C"]), ("G", V0["G"]), ("B", V0["B"]),
                                                     ("Cn", neg(V0["C"])))}
    for k, M in (("Q", V1["Q"]), ("C", V1["C"]), ("G", V1["G"]), ("B", V1["B"]), ("Cn", neg(V1["C"]))):
        give(hs[k], canon(M).data, "dev", keep)
    Fr = Outer(cpk, gpu_ctx, V1, b, kb)
    O = Outer.__new__(Outer)
    O.__dict__.update(Fr.__dict__)
    O.A, O.Cm, O.G, O.B, O.Cn = hs["Q"], hs["C"], hs["G"], hs["B"], hs["Cn"]
    O.M = cpk.opLDL2(O.G, O.B, O.Cn, ctx=gpu_ctx)
    O.M._set(**{k: OPTS[k] for k in PC_PROPS})
    O.db, O.dxy = DeviceArray.of(b), DeviceArray(O.N)
    assert same([x for x in O.M.export_factors()[1:]], [x for x in Fr.M.export_factors()[1:]])
    assert np.array_equal(O.M.export_factors()[0].data, Fr.M.export_factors()[0].data)
    assert same(O.solve("minres", OPTS), Fr.solve("minres", OPTS))  # the first blkdiag(A, C) of the pairing
    a, f = cpk.analyze(O.G, O.B, O.Cn), cpk.analyze(V1["G"], V1["B"], neg(V1["C"]))
    assert np.array_equal(a["L"].data, f["L"].data) and np.array_equal(a["D"], f["D"])


# ---- 4. errors and refusals ---------------------------------------------------------------------------
def test_failed_refactor_after_a_good_update(gpu_ctx):
    """a zero pivot, provoked as test_gpu_factor.py::test_refactor_zero_pivot_reported does"""
    import cpkrylov_amd as cpk
    S = F.load("cvxqp2_s")
    G, B, Cn = canon(S["G"]), canon(S["B"]), neg(S["C"])
    hG, hB, hCn = (cpk.Matrix(M, ctx=gpu_ctx) for M in (G, B, Cn))
    M = cpk.opLDL2(hG, hB, hCn)
    M.nitref, M.force_itref = 1, True
    z = np.random.default_rng(4).standard_normal(M.n)
    x = np.random.default_rng(5).standard_normal(G.shape[1])
    y0, k0 = M * z, M.divide(z)
    L0, D0, _ = M.export_factors()
    keep = []
    give(hG, G.data * 0.0, "dev", keep)  # the update itself succeeds
    with pytest.raises(cpk.CpkError) as e:
        M.refactor(hG, hB, hCn)
    assert "pivot" in str(e.value)
    L1, D1, _ = M.export_factors()
    assert np.array_equal(L1.data, L0.data) and np.array_equal(D1, D0)  # the preconditioner is as before
    assert np.array_equal(M * z, y0) and np.array_equal(M.divide(z), k0)
    assert np.array_equal(hG @ x, np.zeros(G.shape[0])) and hG.info()["values_generation"] == 1  # the matrix holds the new values
    G2 = G.copy()
    G2.data = G.data * np.random.default_rng(6).uniform(0.5, 2.0, G.nnz)
    give(hG, G2.data, "dev", keep)
    M.refactor(hG, hB, hCn)
    M2 = cpk.opLDL2(G2, B, Cn)
    M2.nitref, M2.force_itref = 1, True
    (L, D, perm), (L2, D2, perm2) = M.export_factors(), M2.export_factors()
    assert np.array_equal(perm, perm2) and np.array_equal(L.data, L2.data) and np.array_equal(D, D2)
    assert np.array_equal(M * z, M2 * z)


def test_wrong_count_leaves_everything(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S = canon(system("tiny65x63")["B"])
    x = np.random.default_rng(8).standard_normal(S.shape[1])
    h = cpk.Matrix(S, ctx=gpu_ctx)
    y0, info = h @ x, h.info()
    d = DeviceArray.of(np.ones(S.nnz + 1))
    for fn, args in ((h.set_values, (np.ones(S.nnz + 1),)), (h.set_values, (np.ones(S.nnz - 1),)),
                     (h.set_values_device, (d.p.value, S.nnz + 1)), (h.set_values_device, (d.p.value, S.nnz - 1))):
        with pytest.raises(cpk.CpkError) as e:
            fn(*args)
        assert e.value.code == _lib.CPK_ERR_DIM
        assert h.info() == info and np.array_equal(h @ x, y0)
    with pytest.raises(cpk.CpkError) as e:
        h.set_values_device(0, S.nnz)
    assert e.value.code == _lib.CPK_ERR_ARGS and h.info() == info


def test_distributed_context_is_refused(gpu_ctx):
    """SimGroup(1) with dist1, as test_gpu_solve_multi.py::test_distributed_preconditioner_is_refused"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S = canon(system("tiny65x63")["B"])
    x = np.random.default_rng(8).standard_normal(S.shape[1])
    g = cpk.SimGroup(1)
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=g, options=dict(dist1=1))
    try:
        h = cpk.Matrix(S, ctx=ctx)
        y0, info = h @ x, h.info()
        d = DeviceArray.of(2.0 * S.data)
        for fn, args in ((h.set_values, (2.0 * S.data,)), (h.set_values_device, (d.p.value, S.nnz))):
            with pytest.raises(cpk.CpkError) as e:
                fn(*args)
            assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
            assert h.info() == info and np.array_equal(h @ x, y0)
        del h
    finally:
        ctx.close()
