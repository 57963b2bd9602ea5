"""The HIP paths on the structure family (tests/structures.py): inputs whose structure forces a
kernel path whatever the ordering does -- whole-graph orderings, a factor row longer than every
LDS image, a dense clique (a dense chain of upper rounds), isolated nodes, C = 0, disconnected
blocks, systems smaller than one wave -- and the SpMV's long-row path and block-closing edges.

Everything is compared bit for bit: the apply with the oracle's opLDL2 multiply on the exported
factors, the device factorization with the host's, the exact_dots solves with the oracle's
exact mode, the SpMV with the sequential row sum from 0.0.  Each test also asserts that the
path it is there for was taken."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import structures as ST
from dist_emul import seq_rowsum
from fixtures import EXPROG_OPTS
from oracle import oracle as O
from test_gpu_dist import _run_ranks
from test_gpu_exact import _assert_same, _oracle

pytestmark = pytest.mark.gpu

NAMES = list(ST.MEMBERS)
PROPS = [dict(nitref=0), dict(nitref=1, force_itref=True), dict(nitref=2, force_itref=False, itref_tol=1e-30)]
PROP_IDS = ["plain", "forced1", "live2"]
HUBBED = ["dense_col", "arrow_row"]
OPTION_SETS = [dict(no_chain=1), dict(chain_wide=2 ** 24), dict(no_dataflow=1, no_colsweep=1),
               dict(all_dataflow=1, no_colsweep=1), dict(all_colsweep=1), dict(no_fuse_last=1), dict(no_col16=1),
               dict(no_fused_resid=1), dict(no_sched_resid=1), dict(sweep="64,128,64")]


def _zs(S):
    """standard normal, all zeros, the unit vector of the hub dof"""
    N = S["n"] + S["m"]
    e = np.zeros(N)
    e[ST.hub(S)] = 1.0
    return [np.random.default_rng(7).standard_normal(N), np.zeros(N), e]


def _apply_check(M, S, props_list):
    L, D, perm = M.export_factors()
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=(L, D, perm))
    for props in props_list:
        for k, v in props.items():
            setattr(M, k, v)
        Mo.set(**{k: float(v) for k, v in props.items()})
        for i, z in enumerate(_zs(S)):
            y, yo = M * z, Mo @ z
            assert np.array_equal(y, yo), (props, i, np.max(np.abs(y - yo)))


# ---- 1. apply -----------------------------------------------------------------------------------
@pytest.mark.parametrize("props", PROPS, ids=PROP_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_apply_bitexact(gpu_ctx, name, props):
    import cpkrylov_amd as cpk
    S = ST.get(name)
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    _apply_check(M, S, [props])


@pytest.mark.parametrize("options", OPTION_SETS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in OPTION_SETS])
@pytest.mark.parametrize("name", HUBBED)
def test_apply_bitexact_engine_options(gpu_ctx, name, options):
    import cpkrylov_amd as cpk
    S = ST.get(name)
    with cpk.engine_options(**options):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    _apply_check(M, S, PROPS)


# ---- 2. the paths the members are there for -------------------------------------------------------
def test_paths_taken(gpu_ctx):
    import cpkrylov_amd as cpk
    Ms = {k: cpk.opLDL2(ST.get(k)["G"], ST.get(k)["B"], -ST.get(k)["C"]) for k in NAMES}
    assert Ms["band_g"].info["ordering"] == 4  # minimum degree on the whole graph
    assert Ms["band_g_nd"].info["ordering"] == 3  # nested dissection on the whole graph
    for k in NAMES:
        if not k.startswith("band_g"):
            assert Ms[k].info["ordering"] == 2, k
    L = Ms["arrow_row"].export_factors()[0]
    assert np.diff(L.tocsr().indptr).max() > 3072  # a factor row above the upper rounds' LDS cap
    info = Ms["dense_col"].sweep_info()
    assert info["rounds"] >= 10 and info["chain_tasks"] > 0, info
    assert Ms["dense_col"].info["nrounds"] == info["rounds"]
    # one block in one round.  tiny65x63 is two waves of rows with a dense factor of 6048
    # entries, more than one block stages: it runs in several rounds
    for k in ("tiny1x1", "tiny2x1", "tiny3x2"):
        info = Ms[k].sweep_info()
        assert info["rounds"] == 1 and info["round0_blocks"] == 1 and info["upper_blocks"] == 0, (k, info)


def test_zero_c_with_band_g_reports_factor_error(gpu_ctx):
    """C = 0 with a non-diagonal G: the documented limit of static 1x1 pivots, CPK_ERR_FACTOR."""
    import cpkrylov_amd as cpk
    S = ST.band_g_zero_c()
    with pytest.raises(cpk.CpkError) as e:
        cpk.opLDL2(S["G"], S["B"], -S["C"])
    assert e.value.code == 6


# ---- 3. device factorization ----------------------------------------------------------------------
FACTOR_NAMES = ["band_g", "arrow_row", "dense_col"]


@pytest.mark.parametrize("name", FACTOR_NAMES)
def test_device_factor_equals_host(gpu_ctx, name):
    import cpkrylov_amd as cpk
    S = ST.get(name)
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    L, D, perm = M.export_factors()
    H = cpk.analyze(S["G"], S["B"], -S["C"])
    assert np.array_equal(perm, H["perm"])
    assert np.array_equal(L.indptr, H["L"].indptr) and np.array_equal(L.indices, H["L"].indices)
    assert np.array_equal(L.data, H["L"].data), np.max(np.abs(L.data - H["L"].data))
    assert np.array_equal(D, H["D"])


@pytest.mark.parametrize("name", FACTOR_NAMES)
def test_device_factor_independent_checks(gpu_ctx, name):
    import cpkrylov_amd as cpk
    S = ST.get(name)
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    L, D, perm = M.export_factors()
    Lo, Do, permo = O.LDL2(S["G"], S["B"], -S["C"], perm=perm).factors()
    assert np.array_equal(permo, perm)
    assert np.array_equal(Lo.indptr, L.indptr) and np.array_equal(Lo.indices, L.indices)
    assert np.max(np.abs(L.data - Lo.data)) <= 1e-10 * max(np.max(np.abs(L.data)), 1.0)
    assert np.max(np.abs(D - Do) / np.abs(Do)) <= 1e-10
    K = ST.kp(S)[perm][:, perm]
    Lu = L + sp.identity(K.shape[0], format="csc")
    R = K - Lu @ sp.diags(D) @ Lu.T
    assert abs(R).max() <= 1e-12 * abs(K).max() * max(1.0, abs(Lu).max() ** 2)


@pytest.mark.parametrize("name", FACTOR_NAMES)
def test_refactor_equals_fresh_construction(gpu_ctx, name):
    import cpkrylov_amd as cpk
    S = ST.get(name)
    rng = np.random.default_rng(17)
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    M.nitref, M.force_itref = 1, True
    # new values, same sparsity: G -> E G E with a positive diagonal E (symmetric and positive
    # definite whether G is diagonal or a band), rescaled B and C
    E = sp.diags(rng.uniform(0.7, 1.4, S["n"]))
    G2 = (E @ S["G"] @ E).tocsr()
    G2.sort_indices()
    assert np.array_equal(G2.indices, S["G"].indices)
    B2 = S["B"].copy()
    B2.data = B2.data * rng.uniform(0.8, 1.25, B2.data.shape[0])
    C2 = S["C"] * 3.0
    assert M.refactor(G2, B2, -C2) > 0
    M2 = cpk.opLDL2(G2, B2, -C2)
    M2.nitref, M2.force_itref = 1, True
    (L, D, perm), (L2, D2, perm2) = M.export_factors(), M2.export_factors()
    assert np.array_equal(perm, perm2) and np.array_equal(L.data, L2.data) and np.array_equal(D, D2)
    z = rng.standard_normal(M.n)
    y = M * z
    assert np.array_equal(y, M2 * z)
    assert np.array_equal(M.divide(z), M2.divide(z))
    Mo = O.LDL2(G2, B2, -C2, factors=(L, D, perm))
    Mo.set(nitref=1.0, force_itref=1.0)
    assert np.array_equal(y, Mo @ z)


# ---- 4. solves, exact inner products ---------------------------------------------------------------
@pytest.mark.parametrize("method,extra", ST.SOLVE_METHODS, ids=[m for m, _ in ST.SOLVE_METHODS])
@pytest.mark.parametrize("name", ST.SOLVE_MEMBERS)
def test_exact_solve_bitexact(gpu_ctx, name, method, extra):
    """exact_dots against the oracle's exact mode on the product's factors (that the oracle
    itself solves each case in 1-11 iterations: test_structures_host.py)."""
    import cpkrylov_amd as cpk
    S = ST.get(name)
    opts = dict(EXPROG_OPTS, **extra)
    with cpk.engine_options(exact_dots=1):
        x, stats, flag = cpk.reg_cpkrylov(getattr(cpk, "cp" + method), S["rhs"], S["Q"], S["B"], S["C"], S["G"], opts)
        factors = stats["M"].export_factors()
    xo, so = _oracle(S, method, opts, factors)
    assert so["solved"]
    _assert_same(x, stats, flag, xo, so)


def _iter_and_value(msg):
    """the iteration and the offending value (as %g prints it) of an indefinite-error message"""
    import re
    it = re.search(r"Iter (\d+)", msg)
    val = re.search(r"-\d(?:\.\d+)?e[-+]\d+", msg)
    assert it and val, msg
    return int(it.group(1)), val.group(0)


@pytest.mark.parametrize("method,extra", ST.SOLVE_METHODS, ids=[m for m, _ in ST.SOLVE_METHODS])
def test_exact_solve_raises_as_the_reference(gpu_ctx, method, extra):
    """Where the reference stops with its indefinite / complex-norm error (a squared quantity that
    is pure rounding comes out negative), the product in exact mode stops with CPK_ERR_INDEFINITE
    at the same iteration on the same value."""
    import cpkrylov_amd as cpk
    S = ST.tiny_indefinite()
    opts = dict(EXPROG_OPTS, **extra)
    with cpk.engine_options(exact_dots=1):
        factors = cpk.opLDL2(S["G"], S["B"], -S["C"]).export_factors()
        with pytest.raises(O.OracleError) as eo:
            _oracle(S, method, opts, factors)
        assert eo.value.code == 1
        with pytest.raises(cpk.CpkError) as e:
            cpk.reg_cpkrylov(getattr(cpk, "cp" + method), S["rhs"], S["Q"], S["B"], S["C"], S["G"], opts)
    assert e.value.code == 1, str(e.value)
    assert _iter_and_value(str(e.value)) == _iter_and_value(eo.value.msg), (str(e.value), eo.value.msg)


@pytest.mark.parametrize("P", [2, 4])
def test_dist_apply_small_blocks_cvxqp1_m(gpu_ctx, P):
    """cvxqp1_m on P ranks with small sweep blocks (many rounds), chained and one launch per
    round: the oracle's bits.  (test_gpu_dist.test_dist_apply_sweep_chain_bitexact ran this until
    the corrected ordering left no rank of cvxqp1_m a chain to assert; the comparison stays.)"""
    import cpkrylov_amd as cpk
    import fixtures as F
    S = F.load("cvxqp1_m")
    rng = np.random.default_rng(53)
    zs = [rng.standard_normal(S["n"] + S["m"]) for _ in range(3)]

    def work(ctx, r):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        M.nitref, M.force_itref = 1, True
        return [M * z for z in zs], M.export_factors() if r == 0 else None

    res = {off: _run_ranks(P, work, dict(sweep="64,192,64,128,512,512", no_chain=off)) for off in (False, True)}
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=res[False][0][1])
    Mo.set(nitref=1.0, force_itref=1.0)
    for i, z in enumerate(zs):
        yo = Mo @ z
        for off in (False, True):
            for ys, _ in res[off]:
                assert np.array_equal(ys[i], yo), (off, np.max(np.abs(ys[i] - yo)))


# ---- 5. SpMV ---------------------------------------------------------------------------------------
CAP, MAXROWS = 2048, 1024  # kSpmvCap entries, kSpmvMaxRows rows per workgroup block (dev.hpp)
# workgroups of a launch (spmv_grid): min(blocks, resident), resident = 6 per CU (24 waves per CU
# under amdgpu_waves_per_eu(6), 4 waves each; the 16 KB of LDS would allow 10) x 256 CUs.  The
# wide cases below put their long block on a shared walk for any grid of 101..1600 workgroups.
GRID = 6 * 256


def _csr(lens, ncols, seed=0):
    """rows of the given lengths, sorted distinct columns, values in +-U(1/3, 1)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(ptr[-1], dtype=np.int32)
    for i, k in enumerate(lens):
        if k:
            col[ptr[i]:ptr[i + 1]] = np.arange(ncols) if k == ncols else np.sort(rng.choice(ncols, k, replace=False))
    val = rng.uniform(1.0 / 3.0, 1.0, ptr[-1]) * np.where(rng.random(ptr[-1]) < 0.5, -1.0, 1.0)
    return sp.csr_matrix((val, col, ptr), shape=(len(lens), ncols))


def _blocks(ptr):
    """the row blocks the device matrix is cut into (make_dmat): a block closes before a row
    that would take it over CAP entries, and at MAXROWS rows"""
    blk, r0 = [0], 0
    for r in range(len(ptr) - 1):
        if r > r0 and (r - r0 >= MAXROWS or ptr[r + 1] - ptr[r0] > CAP):
            blk.append(r)
            r0 = r
    return blk + [len(ptr) - 1]


SPMV_CASES = {}
for _L in (2048, 2049, 4096, 4097, 6000):
    SPMV_CASES[f"row{_L}"] = ([7, _L, 3], _L + 13)
SPMV_CASES.update({
    "long_first": ([5000, 4, 9], 5003),
    "long_last": ([4, 9, 5000], 5003),
    "long_adjacent": ([3, 2500, 4097, 2], 4100),
    "block2048": ([8] * 256 + [3], 100),  # the first block holds exactly CAP entries
    "block2049": ([8] * 255 + [9, 3], 100),  # one more: the ninth entry's row opens the next block
    "block2x1024": ([1024, 1024, 5], 1500),
    "block1024_1025": ([1024, 1025, 5], 1500),
    "nnz0": ([0] * 1500, 7),
    "1x1": ([1], 1),
    "1x5000": ([5000], 5000),
    "5000x1": ([1] * 5000, 1),
    # 1700 rows of 1100 entries, a block each, and one 5000-entry row: more blocks than resident
    # workgroups (GRID), so workgroup w walks blocks w, w + GRID, ...; the long block shares a
    # walk with a staged one, before it (block 100, then 100 + GRID) and after it (1600 - GRID,
    # then 1600): prod[] and the loop-top barrier are reused across the two branches
    "wide_long_then_staged": ([1100] * 100 + [5000] + [1100] * 1600, 5000),
    "wide_staged_then_long": ([1100] * 1600 + [5000] + [1100] * 100, 5000),
})
for _K in (1023, 1024, 1025):
    SPMV_CASES[f"empty{_K}"] = ([2] + [0] * _K + [2], 9)
    SPMV_CASES[f"empty{_K}_long"] = ([1] + [0] * _K + [3000] + [0] * _K + [1], 3001)


def _spmv_check(A, x):
    import cpkrylov_amd as cpk
    y = cpk.Matrix(A) @ x
    prod = A.data * x[A.indices]  # the rounded products, as the device forms them (no FMA)
    ref = seq_rowsum(A.indptr, prod)
    assert y.shape == ref.shape
    assert np.array_equal(y, ref, equal_nan=True), np.flatnonzero(y != ref)[:5]
    # independent of the summation order: within the bound of a recursive sum of the row
    for i in range(A.shape[0]):
        p = prod[A.indptr[i]:A.indptr[i + 1]]
        assert abs(y[i] - math.fsum(p)) <= len(p) * 2.0 ** -53 * math.fsum(np.abs(p)), i


@pytest.mark.parametrize("case", list(SPMV_CASES))
def test_spmv_bitexact(gpu_ctx, case):
    lens, ncols = SPMV_CASES[case]
    A = _csr(lens, ncols, seed=len(case))
    # the case is what its name says: the blocks the device cuts
    blk = _blocks(A.indptr)
    ents = np.diff(A.indptr[blk])
    nrow = np.diff(blk)
    assert nrow.max() <= MAXROWS and np.all((ents <= CAP) | (nrow == 1))
    if case.startswith(("row", "long", "1x5000", "wide", "empty")) and max(lens) > CAP:
        assert ents.max() > CAP  # the long-row path
    if case in ("block2048", "block2x1024", "row2048"):
        assert CAP in ents
    if case == "block2049":
        assert ents[0] == CAP - 8 and blk[1] == 255
    if case.startswith("empty") or case in ("nnz0", "5000x1"):
        assert nrow.max() == MAXROWS
    if case.startswith("wide"):
        assert len(ents) == 1701
        grid = min(len(ents), GRID)
        (b,) = np.flatnonzero(ents > CAP)
        walk = [x for x in range(b % grid, len(ents), grid)]  # the blocks of b's workgroup, in order
        i = walk.index(b)
        nxt = case == "wide_long_then_staged"
        assert (i + 1 < len(walk)) if nxt else (i > 0), walk
        assert 0 < ents[walk[i + 1] if nxt else walk[i - 1]] <= CAP  # a staged block on the same walk
    _spmv_check(A, np.random.default_rng(3).standard_normal(ncols))


def test_spmv_special_values(gpu_ctx):
    """x with +-0, subnormals and 1e300 (no overflow: at most 6000 * 1e300 per row)."""
    A = _csr([5, 6000, 0, 2049, 2048, 17], 6100, seed=9)
    x = np.random.default_rng(4).standard_normal(6100)
    x[0::7] = 0.0
    x[1::7] = -0.0
    x[2::7] = 5e-324
    x[3::7] = -2.5e-310
    x[4::7] = 1e300
    x[5::7] = -1e300
    _spmv_check(A, x)


# ---- 6. distributed apply -----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("name", ["band_g", "arrow_row", "dense_col", "tiny3x2"])
def test_dist_apply_bitexact(gpu_ctx, name, P):
    """P simulated ranks; tiny3x2 has ranks that own nothing."""
    import cpkrylov_amd as cpk
    S = ST.get(name)
    zs = _zs(S)

    def work(ctx, r):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        ys = []
        for props in PROPS[:2]:
            for k, v in props.items():
                setattr(M, k, v)
            ys.append([M * z for z in zs])
        d, nl = M.local_dofs()
        return ys, M.export_factors() if r == 0 else None, d, nl

    res = _run_ranks(P, work)
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=res[0][1])
    for j, props in enumerate(PROPS[:2]):
        Mo.set(**{k: float(v) for k, v in props.items()})
        for i, z in enumerate(zs):
            yo = Mo @ z
            for ys, _, _, _ in res:
                assert np.array_equal(ys[j][i], yo), (props, i, np.max(np.abs(ys[j][i] - yo)))
    alld = np.concatenate([d for _, _, d, _ in res])
    assert np.array_equal(np.sort(alld), np.arange(S["n"] + S["m"]))
    if name == "tiny3x2":
        assert min(len(d) for _, _, d, _ in res) == 0


@pytest.mark.parametrize("extra", [{}, {"nitref": 3, "force_itref": False}], ids=["forced1", "live3"])
@pytest.mark.parametrize("P", [2, 3])
def test_dist_exact_solve_ranks_without_rows(gpu_ctx, P, extra):
    """cpminres on tiny3x2 over P ranks: all but one own nothing (empty solver vectors, empty
    SpMV row slices, the accumulating backward sweep of the live refinement with no rows).  With
    exact inner products every rank returns the serial oracle's bits."""
    import cpkrylov_amd as cpk
    S = ST.get("tiny3x2")
    opts = dict(EXPROG_OPTS, **extra)

    def work(ctx, r):
        x, stats, flag = cpk.reg_cpkrylov(cpk.cpminres, S["rhs"], S["Q"], S["B"], S["C"], S["G"], opts, ctx=ctx)
        M = stats["M"]
        return (x, {k: v for k, v in stats.items() if k != "M"}, flag, M.export_factors() if r == 0 else None,
                len(M.local_dofs()[0]))

    res = _run_ranks(P, work, dict(exact_dots=1))
    assert sorted(n for *_, n in res)[0] == 0
    xo, so = _oracle(S, "minres", opts, res[0][3])
    assert so["solved"]
    for x, stats, flag, _, _ in res:
        _assert_same(x, stats, flag, xo, so)
