"""The block forms of the verified solve and of its adjoint (cpk_kkt_solve_multi,
cpk_kkt_sample_multi, cpk_kkt_adjoint_multi; KKT.solve_block, sample_block, adjoint_block).

  sampler     dA, dB, dC of a block X, Lam equal the scalar loop `sampled()` on the stacked columns
              BIT FOR BIT (for B the 2k columns [ly_0, xy_0, ...] x [xx_0, lx_0, ...]), for k at and
              around the panel width, on structures that take every path of the kernel, through every
              value map, with leading dimensions above N, with NaN / 1e300 / zero columns, from host
              and device operands, in both modes; k = 1 gives K.adjoint's bits.
  solve       under exact_dots column j of solve_block is K.solve on that column bit for bit (x,
              niters, solved, histories, the eight sums), cold and warm; in the default mode a
              column's bits do not depend on k, its position or its neighbours, and its true residual
              stays within SAFETY of the single-column solve's.
  adjoint     db and stats are solve_block's on GX, the gradients the loop's on X and the returned
              Lam; under exact_dots they agree with the sum of K.adjoint's single-column gradients
              within the reassociation bound; against a dense direct solve within the bound of
              test_gpu_kkt_adjoint.test_against_a_direct_solve summed over the columns; a column
              whose driver stops leaves the gradients untouched; refusals write nothing.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import fixtures as F
import structures as ST
from rawmat import raw_matrix
from test_gpu_kkt_adjoint import DENSE_LIMIT, bits_equal, sampled
from test_gpu_kkt_adjoint import system as member
from test_gpu_sample_outer import pattern, raw
from test_gpu_solve_multi import longrow

pytestmark = pytest.mark.gpu

SAFETY = 10.0  # tests/test_gpu_parity.py
EPS = 2.0 ** -52
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
OPTS = dict(F.EXPROG_OPTS)
METHODS = ("minres", "cg")
PD = C.POINTER(C.c_double)
SAMPLER_SYSTEMS = ("tiny3x2", "tiny65x63", "arrow_row", "longrow", "cvxqp1_m")
SAMPLER_K = (0, 1, 2, 7, 8, 9, 17)  # the panel boundary, a padded last panel, two panels and one column
SOLVE_SYSTEMS = ("tiny3x2", "tiny65x63", "cvxqp1_m")
SOLVE_K = (1, 2, 7, 8, 9)
# On the tiny members an iteration ends with a residual that is pure rounding, and the reference's
# methods stop with an error when such a quantity comes out below zero (structures.py, TINY_SEED).
# Per member and method: the first nine seeds at which the single-column K.solve of a standard normal
# right-hand side runs through cold and from x0 = 0.9 x, in both modes (the members' own rhs,
# 1e-3 * rhs and the zero column do so for both methods).  test_columns_are_solved_alone keeps
# checking it.
TINY_SEEDS = {("tiny3x2", "minres"): (0, 1, 2, 4, 5, 7, 8, 9, 10), ("tiny3x2", "cg"): (0, 1, 2, 5, 7, 8, 9, 10, 11),
              ("tiny65x63", "minres"): (1, 3, 4, 6, 8, 10, 11, 12, 13), ("tiny65x63", "cg"): (0, 1, 2, 3, 4, 6, 8, 9, 10)}


def _dp(a):
    return a.ctypes.data_as(PD) if a.size else None


@functools.lru_cache(maxsize=None)
def load(name):
    """dict(Q, G, B, C, rhs, n, m) with canonical CSR blocks"""
    if name not in ("longrow", "cvxqp1_m"):
        return member(name)
    P = dict(longrow() if name == "longrow" else F.load(name))
    for key in ("Q", "G", "B", "C"):
        M = sp.csr_matrix(P[key], dtype=np.float64)
        M.sum_duplicates()
        M.sort_indices()
        P[key] = M
    return P


_K = {}


def kkt(name, ctx):
    """K on handles of its own, built once per system (the sampler needs no preconditioner)"""
    import cpkrylov_amd as cpk
    if name not in _K:
        P = load(name)
        _K[name] = cpk.KKT(*(cpk.Matrix(P[k], ctx=ctx) for k in ("Q", "B", "C")), ctx=ctx)
    return _K[name]


_KM = {}


def solver(name, ctx):
    """(K, M) with the example properties, built once per system"""
    import cpkrylov_amd as cpk
    if name not in _KM:
        P = load(name)
        M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=ctx)
        M._set(**{k: OPTS[k] for k in PC_PROPS})
        _KM[name] = (kkt(name, ctx), M)
    return _KM[name]


def operands(N, k, seed):
    """Two N x k blocks with wide exponents (the order of a sum shows) and signed zeros"""
    rng = np.random.default_rng(seed)

    def one():
        a = rng.uniform(1.0, 2.0, (N, k)) * 2.0 ** rng.integers(-40, 40, (N, k)) * rng.choice([-1.0, 1.0], (N, k))
        a[rng.random((N, k)) < 0.08] = 0.0
        a[rng.random((N, k)) < 0.04] = -0.0
        return np.asfortranarray(a)

    return one(), one()


def stacked(P, X, L):
    """(dA, dB, dC) of the scalar loop on the stacked columns: the definition"""
    n, k = P["n"], X.shape[1]
    U, V = np.empty((P["m"], 2 * k)), np.empty((n, 2 * k))
    U[:, 0::2], U[:, 1::2], V[:, 0::2], V[:, 1::2] = L[n:], X[n:], X[:n], L[:n]
    return sampled(P["Q"], L[:n], X[:n], -1.0), sampled(P["B"], U, V, -1.0), sampled(P["C"], L[n:], X[n:], 1.0)


def same_gradients(got, want):
    for key, w in zip(("dA", "dB", "dC"), want):
        assert bits_equal(got[key], w), key


# ---- 1. the sampler, bit for bit -----------------------------------------------------------------
ROUTES = ("panel", "outer")  # the panel kernel and the run-time-k kernel: the same bits on either


class routed:
    """K.set_sample_route(route) for a block of a test, "auto" again afterwards; `.panels` counts the
    calls that took the panel kernel inside it"""

    def __init__(self, K, route):
        self.K, self.route = K, route

    def __enter__(self):
        self.K.set_sample_route(self.route)
        self.before = self.K.sample_route_info()["panel_calls"]
        return self

    def __exit__(self, *exc):
        self.panels = self.K.sample_route_info()["panel_calls"] - self.before
        self.K.set_sample_route("auto")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k", SAMPLER_K)
@pytest.mark.parametrize("name", SAMPLER_SYSTEMS)
def test_sampler_equals_the_scalar_loop(gpu_ctx, name, k, route):
    P, K = load(name), kkt(name, gpu_ctx)
    X, L = operands(K.N, k, 100 + k)
    with routed(K, route) as r:
        got = K.sample_block(X, L)
    assert r.panels == (1 if route == "panel" and k >= 2 else 0)  # k < 2 has the adjoint's own kernels only
    same_gradients(got, stacked(P, X, L))


def test_the_default_route_is_the_measured_rule(gpu_ctx):
    """"auto" takes the panel kernel where at most `max_pad` columns of the last panel are padding
    (DESIGN.md "The block adjoint"), and never below two columns"""
    K = kkt("tiny65x63", gpu_ctx)
    info = K.sample_route_info()
    assert info["route"] == "auto" and info["panel_columns"] == 8 and 0 <= info["max_pad"] < 8
    for k in (0, 1, 2, 7, 8, 9, 16, 17):
        X, L = operands(K.N, k, 5)
        with routed(K, "auto") as r:
            K.sample_block(X, L)
        assert r.panels == int(k >= 2 and -k % 8 <= info["max_pad"]), k


def test_the_structures_take_the_long_row_paths():
    assert np.diff(load("arrow_row")["B"].indptr).max() >= 4400 > 2048
    assert np.diff(load("longrow")["Q"].indptr).max() >= 2101 > 2048
    assert load("tiny65x63")["n"] > 64


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SAMPLER_SYSTEMS)
def test_sampler_operand_forms_agree(gpu_ctx, request, name, route):
    """k = 9: device tensors, leading dimensions above N (the padding rows hold NaN), absent gradients
    and exact_dots all give the loop's bits"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    assert torch is not None and torch.cuda.is_available()
    P, K = load(name), kkt(name, gpu_ctx)
    request.addfinalizer(lambda: K.set_sample_route("auto"))
    K.set_sample_route(route)
    N, k = K.N, 9
    X, L = operands(N, k, 7)
    ref = dict(zip(("dA", "dB", "dC"), stacked(P, X, L)))
    same_gradients(K.sample_block(X, L), [ref[key] for key in ("dA", "dB", "dC")])
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        same_gradients(K.sample_block(X, L), [ref[key] for key in ("dA", "dB", "dC")])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda()  # noqa: E731  (k, N): the N x k block
    out = {key: torch.full((ref[key].size,), -1.5, dtype=torch.float64, device="cuda") for key in ("dA", "dB", "dC")}
    got = K.sample_block(dev(X), dev(L), out=out)
    assert got["dB"] is out["dB"]
    same_gradients({key: v.cpu().numpy() for key, v in out.items()}, [ref[key] for key in ("dA", "dB", "dC")])
    only = K.sample_block(dev(X), dev(L), out={"dC": torch.empty(ref["dC"].size, dtype=torch.float64, device="cuda")})
    assert only["dA"] is None and only["dB"] is None and bits_equal(only["dC"].cpu().numpy(), ref["dC"])
    ldx, ldl = N + 3, N + 5
    Xp, Lp = np.full((ldx, k), np.nan, order="F"), np.full((ldl, k), np.nan, order="F")
    Xp[:N], Lp[:N] = X, L
    g = [np.full(ref[key].size, -2.5) for key in ("dA", "dB", "dC")]
    _lib.check(_lib.lib.cpk_kkt_sample_multi(K.h, k, _dp(Xp), ldx, _dp(Lp), ldl, _dp(g[0]), g[0].size, _dp(g[1]), g[1].size,
                                             _dp(g[2]), g[2].size))
    same_gradients(dict(zip(("dA", "dB", "dC"), g)), [ref[key] for key in ("dA", "dB", "dC")])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k", (2, 9))
def test_sampler_special_values_stay_in_their_entries(gpu_ctx, k, route):
    """columns of X holding NaN, 1e300 and zeros: an entry's bits depend on its own row's and column's
    values alone, so the block still equals the loop entry by entry"""
    name = "tiny65x63"
    P, K = load(name), kkt(name, gpu_ctx)
    X, L = operands(K.N, k, 55)
    X[::7, 0] = np.nan
    X[:, 1] = 0.0
    X[1::5, k - 1] = 1e300
    L[2::9, k - 1] = -1e300
    want = stacked(P, X, L)
    assert np.isnan(want[0]).any() and np.isinf(want[1]).any() and np.isfinite(want[0]).any()
    with routed(K, route):
        same_gradients(K.sample_block(X, L), want)


@pytest.mark.parametrize("case", (("tiny65x63_B", "csc"), ("tiny65x63_B", "dup_csr"), ("arrow_row_B", "csc"),
                                  ("arrow_row_B", "dup_csc")))
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k", (2, 9))
def test_sampler_value_maps(gpu_ctx, case, k, route):
    """B handed over column-compressed (perm map) and with summed duplicates (sptr/src): every raw
    entry gets the bits of its stored entry, both sources of a duplicate the same"""
    import cpkrylov_amd as cpk
    pname, way = case
    name = pname[:-2]
    P = load(name)
    Bc = pattern(pname)
    assert (Bc != P["B"]).nnz == 0
    kind, ptr, ind, rows, cols = raw(pname, way)
    Bh = raw_matrix(kind, Bc.shape, ptr, ind, np.ones(len(rows)), ctx=gpu_ctx)
    K = cpk.KKT(cpk.Matrix(P["Q"], ctx=gpu_ctx), Bh, cpk.Matrix(P["C"], ctx=gpu_ctx), ctx=gpu_ctx)
    X, L = operands(K.N, k, 31 + k)
    wA, wB, wC = stacked(P, X, L)
    stored = {(int(i), int(j)): q for q, (i, j) in enumerate(zip(np.repeat(np.arange(Bc.shape[0]), np.diff(Bc.indptr)),
                                                                Bc.indices))}
    want_raw = np.array([wB[stored[(int(i), int(j))]] for i, j in zip(rows, cols)])
    if way.startswith("dup"):
        assert len(rows) > Bc.nnz
    K.set_sample_route(route)
    got = K.sample_block(X, L)
    assert bits_equal(got["dB"], want_raw) and bits_equal(got["dA"], wA) and bits_equal(got["dC"], wC)


@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_one_column_is_the_adjoints_three_passes(gpu_ctx, name):
    K, M = solver(name, gpu_ctx)
    P = load(name)
    x, _, _ = K.solve("minres", P["rhs"], M, OPTS)
    gx = np.random.default_rng(TINY_SEEDS.get((name, "minres"), (0,))[0]).standard_normal(K.N)
    r = K.adjoint("minres", x, gx, M, OPTS)
    same_gradients(K.sample_block(x, r["db"]), [r[key] for key in ("dA", "dB", "dC")])


# ---- 2. solve_block under exact_dots: every column is the single-column solve ---------------------
@functools.lru_cache(maxsize=None)
def columns(name, method, k):
    """N x k: the fixture's rhs, 1e-3 * rhs, a seeded standard normal vector (a new seed at every
    turn), a zero column, and round again"""
    P = load(name)
    N = P["n"] + P["m"]
    seeds = iter(TINY_SEEDS.get((name, method), tuple(range(9))))
    cols = []
    for j in range(k):
        cols.append((P["rhs"], 1e-3 * P["rhs"], None, np.zeros(N))[j % 4])
        if cols[-1] is None:
            cols[-1] = np.random.default_rng(next(seeds)).standard_normal(N)
    return np.asfortranarray(np.column_stack(cols)) if k else np.zeros((N, 0), order="F")


_SINGLE = {}


def single(ctx, name, method, exact, j, warm):
    """K.solve of column j (warm: from 0.9 times its own cold solution), run once"""
    import cpkrylov_amd as cpk
    key = (name, method, exact, j, warm)
    if key not in _SINGLE:
        K, M = solver(name, ctx)
        b = columns(name, method, max(SOLVE_K))[:, j].copy()
        x0 = 0.9 * single(ctx, name, method, exact, j, False)[0] if warm else None
        with cpk.engine_options(ctx, exact_dots=exact):
            _SINGLE[key] = K.solve(method, b, M, OPTS, x0=x0)
    return _SINGLE[key]


def same_column(X, stats, flags, j, ref):
    x, s, f = ref
    assert bits_equal(X[:, j], x), j
    assert stats[j]["niters"] == s["niters"] and flags[j]["solved"] == f["solved"], j
    hists = [key for key in s if key.endswith("History")]
    assert hists
    for key in hists:
        assert bits_equal(stats[j][key], s[key]), (j, key)
    assert stats[j]["true_resid0"] == s["true_resid0"] and stats[j]["true_resid"] == s["true_resid"], j


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", SOLVE_SYSTEMS)
def test_columns_are_solved_alone(gpu_ctx, name, method):
    """every column the block tests use is solved by the single-column path, cold and warm, in both
    modes (so no comparison below is with an error), and a block holds columns that stop at different
    iterations"""
    for exact in (0, 1):
        its = []
        for j in range(max(SOLVE_K)):
            for warm in (False, True):
                x, s, f = single(gpu_ctx, name, method, exact, j, warm)
                assert f["solved"] and np.all(np.isfinite(x)), (exact, j, warm)
            its.append(single(gpu_ctx, name, method, exact, j, False)[1]["niters"])
        assert len(set(its)) > 1 and its[3] == 0, its


@pytest.mark.parametrize("k", SOLVE_K)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", SOLVE_SYSTEMS)
def test_solve_block_exact_is_the_single_column_solve(gpu_ctx, name, method, k):
    import cpkrylov_amd as cpk
    K, M = solver(name, gpu_ctx)
    Bk = columns(name, method, k)
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        X, stats, flags = K.solve_block(method, Bk, M, OPTS)
        X0 = np.asfortranarray(0.9 * X)
        Xw, sw, fw = K.solve_block(method, Bk, M, OPTS, X0=X0)
    assert len(stats) == len(flags) == k and bits_equal(X0, 0.9 * X)
    for j in range(k):
        same_column(X, stats, flags, j, single(gpu_ctx, name, method, 1, j, False))
        same_column(Xw, sw, fw, j, single(gpu_ctx, name, method, 1, j, True))


def test_solve_block_device_tensors(gpu_ctx):
    """B and out= as (k, N) device tensors, X0 = out: the bits of the host call"""
    assert torch is not None and torch.cuda.is_available()
    name, method, k = "cvxqp1_m", "minres", 3
    K, M = solver(name, gpu_ctx)
    Bk = columns(name, method, k)
    X, stats, _ = K.solve_block(method, Bk, M, OPTS)
    Bd = torch.from_numpy(np.ascontiguousarray(Bk.T)).cuda()
    out = torch.full((k, K.N), np.nan, dtype=torch.float64, device="cuda")
    Xd, sd, _ = K.solve_block(method, Bd, M, OPTS, out=out)
    assert Xd is out and bits_equal(out.cpu().numpy().T, X)
    assert [s["true_resid"] for s in sd] == [s["true_resid"] for s in stats]
    Xw, sw, _ = K.solve_block(method, Bk, M, OPTS, X0=0.9 * X)
    out.mul_(0.9)
    K.solve_block(method, Bd, M, OPTS, X0=out, out=out)
    assert bits_equal(out.cpu().numpy().T, Xw)


# ---- 3. solve_block in the default mode ----------------------------------------------------------
def _solve_anyway(K, M, method, Bk):
    import cpkrylov_amd as cpk
    try:
        return K.solve_block(method, Bk, M, OPTS)
    except cpk.CpkError as e:  # a NaN neighbour may stop with its own error: the others are written
        return e.partial


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_position_independence(gpu_ctx, name, method):
    """a column's bits for k = 2, 8 and 9, first and last, beside NaN, zero and 1e300 * rhs columns"""
    K, M = solver(name, gpu_ctx)
    P = load(name)
    col = P["rhs"]
    X, stats, _ = K.solve_block(method, np.asfortranarray(col.reshape(-1, 1)), M, OPTS)
    ref = (X[:, 0].copy(), stats[0]["residHistory"], stats[0]["niters"], stats[0]["true_resid"])
    for label, other in (("nan", np.full(K.N, np.nan)), ("zeros", np.zeros(K.N)), ("huge", 1e300 * col)):
        for k in (2, 8, 9):
            for pos in (0, k - 1):
                Bk = np.asfortranarray(np.tile(other.reshape(-1, 1), (1, k)))
                Bk[:, pos] = col
                X, stats, _ = _solve_anyway(K, M, method, Bk)
                assert bits_equal(X[:, pos], ref[0]), (label, k, pos)
                assert bits_equal(stats[pos]["residHistory"], ref[1]) and stats[pos]["niters"] == ref[2], (label, k, pos)
                assert stats[pos]["true_resid"] == ref[3], (label, k, pos)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", SOLVE_SYSTEMS)
def test_default_mode_true_residuals(gpu_ctx, name, method):
    """each column's true relative residual within SAFETY of the single-column K.solve's"""
    K, M = solver(name, gpu_ctx)
    k = 9
    X, stats, flags = K.solve_block(method, columns(name, method, k), M, OPTS)
    for j in range(k):
        s = single(gpu_ctx, name, method, 0, j, False)[1]
        got, ref = stats[j]["true_resid"], s["true_resid"]
        print(f"{name} {method} column {j}: block {got['rnorm']:.3e} single {ref['rnorm']:.3e} ||b|| {ref['bnorm']:.3e}")
        assert got["bnorm"] == ref["bnorm"]
        if ref["bnorm"] == 0.0:
            assert got["rnorm"] == 0.0
        else:
            assert got["rnorm"] / got["bnorm"] <= SAFETY * ref["rnorm"] / ref["bnorm"], j


# ---- 4. adjoint_block ----------------------------------------------------------------------------
def grad_columns(name, method, k):
    """GX: k seeded standard normal columns the single-column solve runs through on"""
    seeds = TINY_SEEDS.get((name, method), tuple(range(9)))
    N = load(name)["n"] + load(name)["m"]
    return np.asfortranarray(np.column_stack([np.random.default_rng(s).standard_normal(N) for s in seeds[:k]]))


def same_solve(r, Lam, stats, flags):
    assert bits_equal(r["db"], Lam)
    for j, (a, b) in enumerate(zip(r["stats"], stats)):
        assert a["niters"] == b["niters"] and r["flags"][j]["solved"] == flags[j]["solved"], j
        assert bits_equal(a["residHistory"], b["residHistory"]), j
        assert a["true_resid0"] == b["true_resid0"] and a["true_resid"] == b["true_resid"], j


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("exact", (0, 1))
@pytest.mark.parametrize("k", (2, 9))
@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_adjoint_block_is_solve_block_then_the_loop(gpu_ctx, request, name, k, exact, route):
    import cpkrylov_amd as cpk
    method = "minres"
    K, M = solver(name, gpu_ctx)
    request.addfinalizer(lambda: K.set_sample_route("auto"))
    K.set_sample_route(route)
    P = load(name)
    GX = grad_columns(name, method, k)
    X = np.asfortranarray(np.random.default_rng(77).standard_normal((K.N, k)))
    with cpk.engine_options(gpu_ctx, exact_dots=exact):
        r = K.adjoint_block(method, X, GX, M, OPTS)
        same_solve(r, *K.solve_block(method, GX, M, OPTS))
        same_gradients(r, stacked(P, X, r["db"]))
        Lam0 = np.asfortranarray(0.9 * r["db"])
        out = {"dB": np.zeros(P["B"].nnz), "db": np.zeros((K.N, k), order="F")}
        rw = K.adjoint_block(method, X, GX, M, OPTS, Lam0=Lam0, out=out)
        same_solve(rw, *K.solve_block(method, GX, M, OPTS, X0=Lam0))
        assert rw["dB"] is out["dB"] and rw["db"] is out["db"] and bits_equal(Lam0, 0.9 * r["db"])
        same_gradients(rw, stacked(P, X, rw["db"]))


@pytest.mark.parametrize("k", (3, 9))
@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_block_gradients_are_the_sum_of_the_single_column_ones(gpu_ctx, name, k):
    """exact_dots: Lam's columns are the single-column bits, so the block gradients and the sum over j
    of K.adjoint's are sums of the same k (B: 2k) products per entry in another association; each is
    within (terms + 1) eps sum|products| of the exact sum, so |delta| <= 2 (terms + 1) eps sum|products|"""
    import cpkrylov_amd as cpk
    method = "minres"
    K, M = solver(name, gpu_ctx)
    P = load(name)
    n = P["n"]
    GX = grad_columns(name, method, k)
    X = np.asfortranarray(np.random.default_rng(78).standard_normal((K.N, k)))
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        r = K.adjoint_block(method, X, GX, M, OPTS)
        singles = [K.adjoint(method, X[:, j].copy(), GX[:, j].copy(), M, OPTS) for j in range(k)]
    L = r["db"]
    for j in range(k):
        assert bits_equal(L[:, j], singles[j]["db"]), j
    aX, aL = np.abs(X), np.abs(L)
    U, V = np.empty((P["m"], 2 * k)), np.empty((n, 2 * k))
    U[:, 0::2], U[:, 1::2], V[:, 0::2], V[:, 1::2] = aL[n:], aX[n:], aX[:n], aL[:n]
    mags = (sampled(P["Q"], aL[:n], aX[:n], 1.0), sampled(P["B"], U, V, 1.0), sampled(P["C"], aL[n:], aX[n:], 1.0))
    for key, mag, terms in zip(("dA", "dB", "dC"), mags, (k, 2 * k, k)):
        total = np.zeros_like(r[key])
        for s in singles:
            total = total + s[key]
        delta, bound = np.abs(r[key] - total), 2.0 * (terms + 1) * EPS * mag
        print(f"{name} k={k} {key}: max |delta| / bound {np.max(delta / np.where(bound > 0, bound, 1.0)):.3e}")
        assert np.all(delta <= bound), key


@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_against_a_direct_solve(gpu_ctx, name):
    """test_gpu_kkt_adjoint.test_against_a_direct_solve for a block: X_ref = K \\ B and Lam_ref = K \\ GX
    by a direct solve of K (dense LU up to DENSE_LIMIT dofs, a sparse LU above), g_ref the loop on them.  Column by column lam x' - lam_ref x_ref' = dlam x_ref' +
    lam_ref dx' + dlam dx', a sampled block's 2-norm is at most the Frobenius norm of the whole, and an
    entry's own rounding (per column two products, one sum; alpha) is below 4 k eps of the sum of its
    products' magnitudes: per handle

        ||g - g_ref||_2 <= sum_c (e_x,c + e_lam,c + e_x,c e_lam,c) ||lam_ref,c|| ||x_ref,c|| w + 4 k eps ||terms||_1

    with w = 1 for A and C and 2 for B's two terms"""
    method, k = "minres", 3
    K, M = solver(name, gpu_ctx)
    P = load(name)
    n = P["n"]
    Bk = np.asfortranarray(np.column_stack([P["rhs"]] + [np.random.default_rng(s).standard_normal(K.N)
                                                         for s in TINY_SEEDS.get((name, method), tuple(range(9)))[3:5]]))
    GX = grad_columns(name, method, k)
    X, sx, _ = K.solve_block(method, Bk, M, OPTS)
    r = K.adjoint_block(method, X, GX, M, OPTS)
    Ks = sp.bmat([[P["Q"], P["B"].T], [P["B"], -P["C"]]]).tocsc()
    if K.N <= DENSE_LIMIT:
        Kd = Ks.toarray()
        X_ref, L_ref = np.linalg.solve(Kd, Bk), np.linalg.solve(Kd.T, GX)
    else:  # as that test does above the limit: a sparse direct LU of the same K
        lu = spl.splu(Ks)
        X_ref, L_ref = lu.solve(Bk), lu.solve(GX, trans="T")
    norm = lambda A: np.linalg.norm(A, axis=0)  # noqa: E731
    e_x, e_l = norm(X - X_ref) / norm(X_ref), norm(r["db"] - L_ref) / norm(L_ref)
    for j in range(k):
        fwd = sx[j]["true_resid"]["rnorm"] / sx[j]["true_resid"]["bnorm"]
        adj = r["stats"][j]["true_resid"]["rnorm"] / r["stats"][j]["true_resid"]["bnorm"]
        print(f"{name} column {j}: e_x {e_x[j]:.3e} e_lam {e_l[j]:.3e} true relative residual forward {fwd:.3e} adjoint {adj:.3e}")
    scale = float(np.sum((e_x + e_l + e_x * e_l) * norm(L_ref) * norm(X_ref)))
    aX, aL = np.abs(X_ref), np.abs(L_ref)
    U, V = np.empty((P["m"], 2 * k)), np.empty((n, 2 * k))
    U[:, 0::2], U[:, 1::2], V[:, 0::2], V[:, 1::2] = aL[n:], aX[n:], aX[:n], aL[:n]
    mags = (sampled(P["Q"], aL[:n], aX[:n], 1.0), sampled(P["B"], U, V, 1.0), sampled(P["C"], aL[n:], aX[n:], 1.0))
    for key, ref, mag, w in zip(("dA", "dB", "dC"), stacked(P, X_ref, L_ref), mags, (1.0, 2.0, 1.0)):
        err, bound = np.linalg.norm(r[key] - ref), scale * w + 4.0 * k * EPS * np.sum(mag)
        print(f"{name}: {key} error {err:.3e} bound {bound:.3e} (|g_ref| {np.linalg.norm(ref):.3e})")
        assert err <= bound, (key, err, bound)


def test_a_driver_stop_leaves_the_gradients_untouched(gpu_ctx):
    """structures.tiny_indefinite under exact_dots, its rhs between two zero columns: the call raises
    the column's error, `columns` names it, Lam is written and the sentinel-filled gradients stay"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P = member("indefinite")
    K = cpk.KKT(*(cpk.Matrix(P[k], ctx=gpu_ctx) for k in ("Q", "B", "C")), ctx=gpu_ctx)
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=gpu_ctx)
    M._set(**{k: OPTS[k] for k in PC_PROPS})
    GX = np.asfortranarray(np.column_stack([np.zeros(K.N), P["rhs"], np.zeros(K.N)]))
    sent = -3.75
    out = {k: np.full(c, sent) for k, c in (("dA", P["Q"].nnz), ("dB", P["B"].nnz), ("dC", P["C"].nnz))}
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        with pytest.raises(cpk.IndefiniteError) as es:
            K.solve("minres", P["rhs"], M, OPTS)
        with pytest.raises(cpk.IndefiniteError) as ea:
            K.adjoint_block("minres", np.ones((K.N, 3)), GX, M, OPTS, out=out)
    assert ea.value.code == es.value.code == _lib.CPK_ERR_INDEFINITE
    assert ea.value.columns == [0, _lib.CPK_ERR_INDEFINITE, 0] and "column 1" in str(ea.value)
    Lam, stats, flags = ea.value.partial
    assert flags[0]["solved"] and flags[2]["solved"] and not flags[1]["solved"] and flags[1]["error"] == _lib.CPK_ERR_INDEFINITE
    assert np.all(Lam[:, 0] == 0.0) and np.all(Lam[:, 2] == 0.0)
    assert all(np.all(v == sent) for v in out.values())


def test_refusals_write_nothing(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    lib = _lib.lib
    name = "tiny65x63"
    K, M = solver(name, gpu_ctx)
    P = load(name)
    N, k, sent = K.N, 2, 6.5
    X = np.asfortranarray(np.ones((N, k)))
    cnt = [P[key].nnz for key in ("Q", "B", "C")]
    mk = lambda: ([np.full(c, sent) for c in cnt], np.full((N, k), sent, order="F"), np.full(8 * k, sent),  # noqa: E731
                  (C.c_int * k)(*([-9] * k)))
    o = _lib.make_opts(OPTS)

    def adjoint(method=2, Kh=K.h, ldx=N, ldg=N, ldl=N, counts=cnt, kk=k, xp=True):
        g, lam, res, status = mk()
        rc = lib.cpk_kkt_adjoint_multi(Kh, method, kk, _dp(X) if xp else None, ldx, _dp(X), ldg, M.h, C.byref(o), _dp(lam), ldl,
                                       0, _dp(g[0]), counts[0], _dp(g[1]), counts[1], _dp(g[2]), counts[2], None, status,
                                       _dp(res))
        assert all(np.all(v == sent) for v in g + [lam, res]) and list(status) == [-9] * k
        return rc

    assert adjoint(method=_lib.METHODS["gmres"]) == _lib.CPK_ERR_UNSUPPORTED
    assert adjoint(counts=[cnt[0], cnt[1] - 1, cnt[2]]) == _lib.CPK_ERR_DIM
    assert adjoint(ldx=N - 1) == _lib.CPK_ERR_DIM and adjoint(ldg=N - 1) == _lib.CPK_ERR_DIM
    assert adjoint(ldl=N - 1) == _lib.CPK_ERR_DIM and adjoint(kk=-1) == _lib.CPK_ERR_DIM
    assert adjoint(xp=False) == _lib.CPK_ERR_ARGS and adjoint(Kh=None) == _lib.CPK_ERR_ARGS
    g, lam, res, status = mk()
    assert lib.cpk_kkt_solve_multi(K.h, _lib.METHODS["gmres"], k, _dp(X), N, M.h, C.byref(o), _dp(lam), N, 0, None, status,
                                   _dp(res)) == _lib.CPK_ERR_UNSUPPORTED
    assert lib.cpk_kkt_solve_multi(K.h, 2, k, _dp(X), N - 1, M.h, C.byref(o), _dp(lam), N, 0, None, status,
                                   _dp(res)) == _lib.CPK_ERR_DIM
    assert lib.cpk_kkt_solve_multi(K.h, 2, k, None, N, M.h, C.byref(o), _dp(lam), N, 0, None, status, _dp(res)) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_sample_multi(K.h, k, _dp(X), N, _dp(X), N - 1, _dp(g[0]), cnt[0], None, 0, None, 0) == _lib.CPK_ERR_DIM
    assert lib.cpk_kkt_sample_multi(K.h, k, _dp(X), N, _dp(X), N, _dp(g[0]), cnt[0] + 1, None, 0, None, 0) == _lib.CPK_ERR_DIM
    assert lib.cpk_kkt_sample_multi(K.h, k, None, N, _dp(X), N, _dp(g[0]), cnt[0], None, 0, None, 0) == _lib.CPK_ERR_ARGS
    assert all(np.all(v == sent) for v in g + [lam, res]) and list(status) == [-9] * k
    # the Python methods raise the same codes
    for fn, code in ((lambda: K.solve_block("gmres", X, M, OPTS), _lib.CPK_ERR_UNSUPPORTED),
                     (lambda: K.adjoint_block("gmres", X, X, M, OPTS), _lib.CPK_ERR_UNSUPPORTED),
                     (lambda: K.adjoint_block("minres", X, X, M, OPTS, out={"dB": np.zeros(cnt[1] - 1)}), _lib.CPK_ERR_DIM)):
        with pytest.raises(cpk.CpkError) as e:
            fn()
        assert e.value.code == code
    # a one-rank sim context that runs the distributed path: K was built before the option was set
    grp = cpk.SimGroup(1)
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=grp)
    try:
        P3 = load("tiny3x2")
        K3 = cpk.KKT(*(cpk.Matrix(P3[key], ctx=ctx) for key in ("Q", "B", "C")), ctx=ctx)
        M3 = cpk.opLDL2(P3["G"], P3["B"], -P3["C"], ctx=ctx)
        ctx.set_option("dist1", 1)
        X3 = np.ones((K3.N, 2), order="F")
        out = {key: np.full(P3[h].nnz, sent) for key, h in (("dA", "Q"), ("dB", "B"), ("dC", "C"))}
        out["db"] = np.full((K3.N, 2), sent, order="F")
        grads = {key: out[key] for key in ("dA", "dB", "dC")}
        for fn in (lambda: K3.solve_block("minres", X3, M3, OPTS, out=out["db"]), lambda: K3.sample_block(X3, X3, out=grads),
                   lambda: K3.adjoint_block("minres", X3, X3, M3, OPTS, out=out)):
            with pytest.raises(cpk.CpkError) as e:
                fn()
            assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
        assert all(np.all(v == sent) for v in out.values())
        del fn, K3, M3
    finally:
        ctx.close()
