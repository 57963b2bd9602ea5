"""The lockstep block solve (cpk_method_solve_multi, cpcg and cpminres on an n x k block): column j
is the reference's method(b(:, j), A, C, M, opts) (kernels/cpcg.m:1, kernels/cpminres.m:1), whatever
the other columns hold.

The reference has no block solve, so the oracle run once per column is the specification.  Every
system gets five base columns whose iteration counts differ -- the fixture's rhs, 1e-3 * rhs, a
seeded random vector, a unit vector and an all-zero column (it stops at iteration 0, solved) -- and
a block of k columns cycles through them, so frozen columns sit beside running ones in every
panel.  The oracle's result of a base column is computed once and shared.

  exact mode      every column's niters, solved, history, x and y == the oracle's exact mode on the
                  product's exported factors, and == the single-column GPU solve of that column
                  (the unfused and the fused cpminres): the panel product's row sums, the per-column
                  reductions, the freezing and the panel apply at once.
  default mode    the project's band (test_gpu_parity.py: FLOOR, SAFETY) around the oracle, the band
                  being that column's own spread under 1e-15 perturbations of its rhs.
  position        a column's bits do not depend on k, its position or its neighbours (NaN, zeros,
                  1e300 * rhs).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import fixtures as F
import structures as ST
from oracle import oracle as O
from xacc_cases import ref_exact

pytestmark = pytest.mark.gpu

FLOOR = 1e-8  # tests/test_gpu_parity.py
SAFETY = 10.0
METHODS = ("minres", "cg")
FIXTURES = ("cvxqp1_m", "syn_symm20k")
TINY = ("tiny1x1", "tiny2x1", "tiny3x2", "tiny65x63")
MEMBERS = TINY + ("band_g", "arrow_row")
LONGROW = "longrow"
SYSTEMS = FIXTURES + MEMBERS + (LONGROW,)
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
OPTS = dict(F.EXPROG_OPTS)
NBASE = 5
# On the tiny members a residual that is pure rounding may come out below zero, where the reference
# stops with its error (structures.py TINY_SEED), and a member's rhs(1:n) without reg_cpkrylov's
# shift is such a column on some of them.  There the first column is a seeded random vector too:
# (seed, unit index) below is the first pair at which the oracle solves every base column with both
# methods in both modes; test_oracle_columns_differ_and_are_stable keeps checking it.
TINY_COLUMNS = {"tiny1x1": (0, 0, 7.0), "tiny2x1": (0, 0, 1.0), "tiny3x2": (5, 0, 1.0), "tiny65x63": (13, 0, 1.0)}
LONG_ARROW = 2100  # entries of the long row of the Krylov operator's A (above kSpmvCap = 2048)


def sizes(name):
    return (1, 2, 7, 8, 9, 17) if name in TINY else (2, 7, 8, 9)


@functools.lru_cache(maxsize=None)
def longrow():
    """saddle_system(4000) with a symmetric arrow in Q: row / column 0 holds LONG_ARROW small
    entries, so the Krylov operator blkdiag(Q, C) has a row above kSpmvCap (the long-row path of
    the panel product; arrow_row's long row is in Kp only).  The entries are small enough to keep
    Q strictly diagonally dominant where it was: Q stays SPD."""
    S = ST.saddle_system(N=4000)
    n = S["n"]
    rng = np.random.default_rng(4001)
    v = np.zeros(n)
    v[1:LONG_ARROW + 1] = 1e-4 * rng.uniform(0.5, 1.0, LONG_ARROW) * np.where(rng.random(LONG_ARROW) < 0.5, -1, 1)
    arrow = sp.lil_matrix((n, n))
    arrow[0, :] = v
    arrow[:, 0] = v.reshape(n, 1)
    Q = (S["Q"] + arrow.tocsr()).tocsr()
    Q[0, 0] = Q[0, 0] + 1.0  # the arrow's row sum is below 0.21
    return ST._pack(Q, sp.diags(Q.diagonal()), S["B"], S["C"], S["rhs"])


def system(name):
    if name == LONGROW:
        return longrow()
    if name in FIXTURES:
        return F.load(name)
    return ST.get(name)


@functools.lru_cache(maxsize=None)
def base_columns(name):
    """n x NBASE: rhs(1:n), 1e-3 * rhs(1:n), a seeded random vector, a unit vector, zeros (the tiny
    members: TINY_COLUMNS -- a seeded first column, and the unit vector scaled where n = 1 leaves no
    other choice)"""
    S = system(name)
    n = S["n"]
    b = S["rhs"][:n]
    seed, unit, uval = TINY_COLUMNS.get(name, (7, n // 2, 1.0))
    rng = np.random.default_rng(seed)
    if name in TINY_COLUMNS:
        b = np.random.default_rng(1000 + seed).standard_normal(n)
    e = np.zeros(n)
    e[unit] = uval
    return np.asfortranarray(np.column_stack([b, 1e-3 * b, rng.standard_normal(n), e, np.zeros(n)]))


def block(name, k):
    Bc = base_columns(name)
    return np.asfortranarray(Bc[:, [j % NBASE for j in range(k)]])


def _oracle_M(S, factors):
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=factors)
    Mo.set(**{k: float(OPTS[k]) for k in PC_PROPS})
    return Mo


_FACTORS = {}


def gpu_M(name):
    """the product's preconditioner of a system (built once) with the example properties"""
    import cpkrylov_amd as cpk
    if name not in _FACTORS:
        S = system(name)
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        M._set(**{k: OPTS[k] for k in PC_PROPS})
        _FACTORS[name] = (M, M.export_factors())
    return _FACTORS[name]


@functools.lru_cache(maxsize=None)
def oracle_column(name, method, j, exact):
    """(x, y, stats) of the oracle on base column j with the product's factors"""
    S = system(name)
    Mo = _oracle_M(S, gpu_M(name)[1])
    with O.exact(exact):
        return O.method(method, base_columns(name)[:, j].copy(), S["Q"], S["C"], Mo, OPTS)


@functools.lru_cache(maxsize=None)
def column_band(name, method, j, trials=4, eps=1e-15):
    """tests/sensitivity.py for one column at the method level: the oracle's spread (histories
    relative to history[0], x relative to the norm of x) under relative perturbations of 1e-15 of
    that column, and whether niters moved"""
    S = system(name)
    Mo = _oracle_M(S, gpu_M(name)[1])
    b = base_columns(name)[:, j]
    x1, y1, s1 = oracle_column(name, method, j, False)
    out = {"hist": 0.0, "x": 0.0, "stable": True}
    rng = np.random.default_rng(12345)
    for _ in range(trials):
        x2, y2, s2 = O.method(method, b * (1 + eps * rng.standard_normal(b.shape[0])), S["Q"], S["C"], Mo, OPTS)
        h1, h2 = s1["residHistory"], s2["residHistory"]
        out["stable"] = out["stable"] and s1["niters"] == s2["niters"]
        L = min(len(h1), len(h2))
        if h1[0] > 0:
            out["hist"] = max(out["hist"], float(np.max(np.abs(h1[:L] - h2[:L])) / h1[0]))
        if np.linalg.norm(x1) > 0:
            out["x"] = max(out["x"], float(np.linalg.norm(x1 - x2) / np.linalg.norm(x1)))
    return out


def solve_block(name, method, Bk, raise_on_error=True):
    """the block entry on Bk; k = 1 goes through it too (the Python solvers keep an n x 1 array on
    the single-column path)"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import api
    S = system(name)
    M = gpu_M(name)[0]
    if Bk.shape[1] == 1:
        return api._method_block(method, Bk, api._as_matrix(S["Q"], M.ctx), api._as_matrix(S["C"], M.ctx), M, OPTS,
                                 raise_on_error)
    return getattr(cpk, "cp" + method)(Bk, S["Q"], S["C"], M, OPTS, raise_on_error=raise_on_error)


_SINGLE = {}


def single_column(name, method, j, exact, fused):
    """the single-column GPU solve of base column j (the code this change does not touch)"""
    import cpkrylov_amd as cpk
    key = (name, method, j, exact, fused)
    if key not in _SINGLE:
        S = system(name)
        with cpk.engine_options(exact_dots=int(exact), no_minres_fuse=int(not fused)):
            _SINGLE[key] = getattr(cpk, "cp" + method)(base_columns(name)[:, j].copy(), S["Q"], S["C"], gpu_M(name)[0],
                                                       OPTS)
    return _SINGLE[key]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- the columns are what the tests need them to be (CPU: the oracle alone decides) -------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", SYSTEMS)
def test_oracle_columns_differ_and_are_stable(gpu_ctx, name, method):
    """the oracle solves every base column, its iteration counts are not all equal (so a block
    holds frozen columns beside running ones), the zero column stops at 0 solved, and the counts
    do not move under the perturbations the band is made of"""
    its = []
    for j in range(NBASE):
        for exact in (False, True):
            x, y, s = oracle_column(name, method, j, exact)
        its.append(s["niters"])
        assert column_band(name, method, j)["stable"], (name, method, j)
    assert len(set(its)) > 1, its
    x, y, s = oracle_column(name, method, NBASE - 1, False)
    assert s["niters"] == 0 and s["solved"] and not x.any() and not y.any()


# ---- 1. exact mode, bit for bit -----------------------------------------------------------------
def _assert_column(got, want, what):
    (x, y, st, fl), (xo, yo, so) = got, want
    assert st["niters"] == so["niters"], what
    assert fl["solved"] == so["solved"], what
    assert len(st["residHistory"]) == len(so["residHistory"]), what
    bad = np.flatnonzero(st["residHistory"] != so["residHistory"])
    assert bad.size == 0, (what, bad[:5])
    assert np.array_equal(x, xo), (what, np.max(np.abs(x - xo)))
    assert np.array_equal(y, yo), (what, np.max(np.abs(y - yo)))


CASES = [(n, m, k) for n in SYSTEMS for m in METHODS for k in sizes(n)]


@pytest.mark.parametrize("name,method,k", CASES)
def test_exact_block_bitexact(gpu_ctx, name, method, k):
    import cpkrylov_amd as cpk
    with cpk.engine_options(exact_dots=1):
        X, Y, stats, flag = solve_block(name, method, block(name, k))
    assert X.shape == (system(name)["n"], k) and Y.shape == (system(name)["m"], k) and len(stats) == len(flag) == k
    for j in range(k):
        got = (X[:, j], Y[:, j], stats[j], flag[j])
        _assert_column(got, oracle_column(name, method, j % NBASE, True), (name, method, k, j, "oracle"))
        for fused in ((False, True) if method == "minres" else (False,)):
            xs, ys, ss, fs = single_column(name, method, j % NBASE, True, fused)
            ss = dict(ss, solved=fs["solved"])
            _assert_column(got, (xs, ys, ss), (name, method, k, j, "single", fused))


# ---- 2. default mode, the project's band --------------------------------------------------------
@pytest.mark.parametrize("name,method,k", CASES)
def test_default_block_in_band(gpu_ctx, name, method, k):
    X, Y, stats, flag = solve_block(name, method, block(name, k))
    for j in range(k):
        b = j % NBASE
        xo, yo, so = oracle_column(name, method, b, False)
        what = (name, method, k, j)
        assert stats[j]["niters"] == so["niters"], what
        assert flag[j]["solved"] == so["solved"], what
        h, ho = stats[j]["residHistory"], so["residHistory"]
        assert len(h) == len(ho), what
        if b == NBASE - 1:  # the all-zero column
            assert np.array_equal(h, ho) and not X[:, j].any() and not Y[:, j].any(), what
            continue
        bd = column_band(name, method, b)
        dev = float(np.max(np.abs(h - ho)) / ho[0])
        print(what, "history", dev, "band", bd["hist"])
        assert dev <= max(FLOOR, SAFETY * bd["hist"]), (what, dev, bd["hist"])
        if not xo.any():  # a column that stops at iteration 0: the zero solution, nothing to scale by
            assert not yo.any() and not X[:, j].any() and not Y[:, j].any(), what
            continue
        dx = float(np.linalg.norm(X[:, j] - xo) / np.linalg.norm(xo))
        print(what, "x", dx, "band", bd["x"])
        assert dx <= max(FLOOR, SAFETY * bd["x"]), (what, dx, bd["x"])


# ---- 3. position independence, default mode -------------------------------------------------------
def _fill(name, k, pos, col, other):
    n = system(name)["n"]
    Bk = np.empty((n, k), order="F")
    Bk[:] = other.reshape(n, 1)
    Bk[:, pos] = col
    return Bk


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ("cvxqp1_m", "tiny65x63"))
def test_position_independence(gpu_ctx, name, method):
    n = system(name)["n"]
    col = base_columns(name)[:, 0].copy()
    X, Y, st, fl = solve_block(name, method, block(name, 8))
    ref = (X[:, 0].copy(), Y[:, 0].copy(), st[0]["residHistory"], st[0]["niters"])
    others = {"nan": np.full(n, np.nan), "zeros": np.zeros(n), "huge": 1e300 * col}
    for k, pos in ((8, 5), (3, 0), (9, 8), (17, 16), (17, 3)):
        for label, other in others.items():
            X, Y, st, fl = solve_block(name, method, _fill(name, k, pos, col, other), raise_on_error=False)
            what = (name, method, k, pos, label)
            assert st[pos]["niters"] == ref[3], what
            assert np.array_equal(X[:, pos], ref[0]) and np.array_equal(Y[:, pos], ref[1]), what
            assert np.array_equal(st[pos]["residHistory"], ref[2]), what
    # the NaN column itself: what the single-column solve returns for it
    import cpkrylov_amd as cpk
    S = system(name)
    with cpk.engine_options(no_minres_fuse=1):
        xs, ys, ss, fs = getattr(cpk, "cp" + method)(others["nan"], S["Q"], S["C"], gpu_M(name)[0], OPTS)
    X, Y, st, fl = solve_block(name, method, _fill(name, 8, 5, col, others["nan"]), raise_on_error=False)
    for j in (0, 7):
        assert st[j]["niters"] == ss["niters"] and fl[j]["solved"] == fs["solved"]
        assert _same_bits(st[j]["residHistory"], ss["residHistory"])
        assert _same_bits(X[:, j], xs) and _same_bits(Y[:, j], ys)


# ---- 4. batching and leading dimensions -----------------------------------------------------------
@pytest.mark.parametrize("exact", (0, 1))
@pytest.mark.parametrize("method", METHODS)
def test_batching_changes_no_bit(gpu_ctx, method, exact):
    import cpkrylov_amd as cpk
    name = "cvxqp1_m"
    runs = []
    for o in ({}, dict(batch=1), dict(batch=16), dict(no_graph=1)):
        with cpk.engine_options(exact_dots=exact, **o):
            X, Y, st, fl = solve_block(name, method, block(name, 9))
        runs.append((X, Y, [s["residHistory"] for s in st]))
    for X, Y, hs in runs[1:]:
        assert np.array_equal(X, runs[0][0]) and np.array_equal(Y, runs[0][1])
        assert all(np.array_equal(a, b) for a, b in zip(hs, runs[0][2]))


@pytest.mark.parametrize("method", METHODS)
def test_leading_dimensions_leave_padding_untouched(gpu_ctx, method):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _as_matrix, _dptr
    name, k = "cvxqp1_m", 9
    S = system(name)
    n, m = S["n"], S["m"]
    M = gpu_M(name)[0]
    A, Cm = _as_matrix(S["Q"], M.ctx), _as_matrix(S["C"], M.ctx)
    ldb, ldx, ldy = n + 3, n + 5, m + 2
    Bp = np.full((ldb, k), 7.25, order="F")
    Bp[:n] = block(name, k)
    Xp, Yp = np.full((ldx, k), -3.5, order="F"), np.full((ldy, k), -4.5, order="F")
    status = (C.c_int * k)()
    rc = _lib.lib.cpk_method_solve_multi(M.ctx.h, _lib.METHODS[method], k, _dptr(Bp), ldb, A.h, Cm.h, M.h,
                                         C.byref(_lib.make_opts(OPTS)), _dptr(Xp), ldx, _dptr(Yp), ldy, None, status)
    assert rc == 0 and not any(status)
    X, Y, st, fl = solve_block(name, method, block(name, k))
    assert np.array_equal(Xp[:n], X) and np.array_equal(Yp[:m], Y)
    assert np.all(Xp[n:] == -3.5) and np.all(Yp[m:] == -4.5) and np.all(Bp[n:] == 7.25)


# ---- 5. the Krylov product alone ----------------------------------------------------------------------
def _spmm(name, X):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _as_matrix, _dptr
    S = system(name)
    M = gpu_M(name)[0]
    A, Cm = _as_matrix(S["Q"], M.ctx), _as_matrix(S["C"], M.ctx)
    N, k = X.shape
    Y, dots = np.full((N, k), np.nan, order="F"), np.zeros(2 * k)
    _lib.check(_lib.lib.cpk_debug_spmm(M.ctx.h, A.h, Cm.h, M.h, k, _dptr(X), N, _dptr(Y), N, _dptr(dots)))
    return Y, dots.reshape(k, 2), A, Cm


_xround = ref_exact  # the correctly rounded exact inner product (xacc_cases.py, reference A)


@pytest.mark.parametrize("k", (1, 7, 8))
@pytest.mark.parametrize("name", SYSTEMS)
def test_spmm_equals_spmv(gpu_ctx, name, k):
    import cpkrylov_amd as cpk
    S = system(name)
    n, N = S["n"], S["n"] + S["m"]
    rng = np.random.default_rng(100 + k)
    X = np.asfortranarray(rng.standard_normal((N, k)) * np.exp(rng.uniform(-3, 3, (N, 1))))
    Y, dots, A, Cm = _spmm(name, X)
    for j in range(k):
        y = np.concatenate([A @ X[:n, j], Cm @ X[n:, j]])
        assert np.array_equal(Y[:, j], y), (name, k, j)
        for h, (lo, hi) in enumerate(((0, n), (n, N))):
            want = float(np.dot(y[lo:hi], X[lo:hi, j]))
            scale = float(np.dot(np.abs(y[lo:hi]), np.abs(X[lo:hi, j])))
            assert abs(dots[j, h] - want) <= 4 * N * np.finfo(float).eps * scale, (name, k, j, h)
    # the exact sums against correctly rounded rational arithmetic, every system and column
    with cpk.engine_options(exact_dots=1):
        Ye, de, _, _ = _spmm(name, X)
    assert np.array_equal(Ye, Y)
    for j in range(k):
        assert de[j, 0] == _xround(Y[:n, j], X[:n, j]), (name, k, j)
        assert de[j, 1] == _xround(Y[n:, j], X[n:, j]), (name, k, j)


# ---- 6. the reg level -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ("cvxqp1_m", "tiny65x63"))
def test_exact_reg_block_bitexact(gpu_ctx, name, method):
    """reg_cpkrylov on an N x k block whose columns are shifted (b(n+1:N) != 0) or not"""
    import cpkrylov_amd as cpk
    S = system(name)
    n, N = S["n"], S["n"] + S["m"]
    rhs = S["rhs"]
    unshifted = rhs.copy()
    unshifted[n:] = 0.0
    rng = np.random.default_rng(5)
    cols = [rhs, unshifted, 1e-3 * rhs, np.concatenate([rng.standard_normal(n), np.zeros(N - n)]), np.zeros(N),
            rhs, unshifted, 2.0 * rhs, rhs]
    Bk = np.asfortranarray(np.column_stack(cols))
    with cpk.engine_options(exact_dots=1):
        X, stats, flag = cpk.reg_cpkrylov(getattr(cpk, "cp" + method), Bk, S["Q"], S["B"], S["C"], S["G"], OPTS,
                                          raise_on_error=False)
        M = stats[0]["M"]
        Mo = _oracle_M(S, M.export_factors())
        solved = 0
        for j, b in enumerate(cols):
            what = (name, method, j)
            try:
                with O.exact():
                    xo, so = O.reg_solve(method, b, S["Q"], S["B"], S["C"], Mo, OPTS)
            except O.OracleError as e:  # the reference stops with its error on this column: so does the product
                assert e.code == 1 and flag[j].get("error") == 1, what
                continue
            solved += 1
            assert "error" not in flag[j], what
            assert stats[j]["niters"] == so["niters"] and flag[j]["solved"] == so["solved"], what
            assert np.array_equal(stats[j]["residHistory"], so["residHistory"]), what
            assert np.array_equal(X[:, j], xo), (what, np.max(np.abs(X[:, j] - xo)))
        assert solved >= 5  # the columns the test is about are solved, shifted and unshifted
        # one operator, reusable
        assert all("M" not in s for s in stats[1:])
        x1, y1, s1, f1 = getattr(cpk, "cp" + method)(unshifted[:n], S["Q"], S["C"], M, OPTS)
        assert np.array_equal(np.concatenate([x1, y1]), X[:, 1])


# ---- 7. errors and refusals -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_indefinite_columns_report_per_column(gpu_ctx, method):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S = ST.tiny_indefinite()
    Bk = np.asfortranarray(np.column_stack([S["rhs"], 2.0 * S["rhs"], 0.5 * S["rhs"]]))
    fn = getattr(cpk, "cp" + method)
    with cpk.engine_options(exact_dots=1):
        with pytest.raises(cpk.CpkError) as e:
            cpk.reg_cpkrylov(fn, Bk, S["Q"], S["B"], S["C"], S["G"], OPTS)
        assert e.value.code == _lib.CPK_ERR_INDEFINITE and "column 0" in str(e.value)
        assert e.value.columns == [_lib.CPK_ERR_INDEFINITE] * 3
        assert e.value.partial[0].shape == Bk.shape
        X, stats, flag = cpk.reg_cpkrylov(fn, Bk, S["Q"], S["B"], S["C"], S["G"], OPTS, raise_on_error=False)
        assert [f["error"] for f in flag] == [_lib.CPK_ERR_INDEFINITE] * 3 and not any(f["solved"] for f in flag)


@pytest.mark.parametrize("method", METHODS)
def test_indefinite_message_is_the_single_columns(gpu_ctx, method):
    """one formatter writes both texts: the block entry's message for its first failing column is
    "column 0: " and what the single-column entry raises on that column (exact mode: both stop at
    the same iteration with the same value)"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S = ST.tiny_indefinite()
    Bk = np.asfortranarray(np.column_stack([S["rhs"], 2.0 * S["rhs"], 0.5 * S["rhs"]]))
    fn = getattr(cpk, "cp" + method)
    with cpk.engine_options(exact_dots=1):
        with pytest.raises(cpk.CpkError) as single:
            cpk.reg_cpkrylov(fn, S["rhs"].copy(), S["Q"], S["B"], S["C"], S["G"], OPTS)
        with pytest.raises(cpk.CpkError) as blk:
            cpk.reg_cpkrylov(fn, Bk, S["Q"], S["B"], S["C"], S["G"], OPTS)
    assert single.value.code == blk.value.code == _lib.CPK_ERR_INDEFINITE
    print(repr(str(single.value)), repr(str(blk.value)))
    assert str(blk.value) == "column 0: " + str(single.value)


def test_refusals_leave_outputs_untouched(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _as_matrix, _dptr
    name, k = "tiny65x63", 3
    S = system(name)
    n, m = S["n"], S["m"]
    Bk = block(name, k)
    # methods other than cpcg and cpminres
    for fn in (cpk.cpgmres, cpk.cpdqgmres, cpk.cpsymmlq, cpk.cpcglanczos):
        with pytest.raises(cpk.CpkError) as e:
            fn(Bk, S["Q"], S["C"], gpu_M(name)[0], OPTS)
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
    # the handle semantics of residual_update in effect: the condition cpk_pc_apply_multi refuses
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    M._set(**{p: OPTS[p] for p in PC_PROPS})
    M.handle_semantics = True
    A, Cm = _as_matrix(S["Q"], M.ctx), _as_matrix(S["C"], M.ctx)
    X, Y = np.full((n, k), -3.5, order="F"), np.full((m, k), -4.5, order="F")
    status = (C.c_int * k)(9, 9, 9)
    for method in (_lib.METHODS["minres"], _lib.METHODS["gmres"]):
        rc = _lib.lib.cpk_method_solve_multi(M.ctx.h, method, k, _dptr(Bk), n, A.h, Cm.h, M.h,
                                             C.byref(_lib.make_opts(OPTS)), _dptr(X), n, _dptr(Y), m, None, status)
        assert rc == _lib.CPK_ERR_UNSUPPORTED
        assert np.all(X == -3.5) and np.all(Y == -4.5) and list(status) == [9, 9, 9]
    M.handle_semantics = False
    rc = _lib.lib.cpk_method_solve_multi(M.ctx.h, _lib.METHODS["gmres"], k, _dptr(Bk), n, A.h, Cm.h, M.h,
                                         C.byref(_lib.make_opts(OPTS)), _dptr(X), n, _dptr(Y), m, None, status)
    assert rc == _lib.CPK_ERR_UNSUPPORTED and np.all(X == -3.5) and list(status) == [9, 9, 9]
    # k == 0 does nothing
    rc = _lib.lib.cpk_method_solve_multi(M.ctx.h, _lib.METHODS["minres"], 0, _dptr(Bk), n, A.h, Cm.h, M.h,
                                         C.byref(_lib.make_opts(OPTS)), _dptr(X), n, _dptr(Y), m, None, status)
    assert rc == 0 and np.all(X == -3.5) and np.all(Y == -4.5)


def test_distributed_preconditioner_is_refused(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    name, k = "tiny65x63", 3
    S = system(name)
    g = cpk.SimGroup(1)
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=g, options=dict(dist1=1))
    try:
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        with pytest.raises(cpk.CpkError) as e:
            cpk.cpminres(block(name, k), S["Q"], S["C"], M, OPTS)
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
        del M
    finally:
        ctx.close()
