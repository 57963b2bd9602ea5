"""The operator-valued A (cpk.Operator / cpk_op): the (1,1) block given as a product on device memory.

Unless a test says otherwise the callback is the library's own SpMV (cpk_mat_spmv_device) on a
handle of the same A, so the operator path and the matrix path compute the same u = A*v bit for bit
and differ only in where the two inner products of the Krylov product are summed:
  - under exact_dots the sums are the correctly rounded exact sums, which have no order, so every
    result must equal the matrix path's bit for bit (case 1);
  - by default the sums are fixed-order sums over another grid, so the results agree with the CPU
    oracle within the project's rule max(1e-8, 10 x band), the band being the oracle's own spread
    under 1e-15 perturbations of the right-hand side (tests/sensitivity.py), as in
    tests/test_gpu_parity.py (case 2).

Systems: cvxqp1_m for the four symmetric methods, cvxqp2_s for cpgmres and cpdqgmres, tiny1x1 (a
one-element gather), tiny65x63 (one past a wave), and zero_c, whose blkdiag(0, C) has no entry at
all.  On the tiny members the right-hand side is the column tests/test_gpu_solve_multi.py
established the oracle solves (TINY_COLUMNS); the CPU oracle solves every (system, method) pair
below in both modes (one iteration on the tiny members, ten on zero_c).

Calls of fn, from the loops of solvers.hip (eager operator, where the count is exact): one per
iteration that ran (niters), one for cpsymmlq's pre-step (it runs whenever the initial residual
is above the tolerance), one per cpgmres restart (the cycle's [A*x; C*y]), one for reg_cpkrylov's
shift when b(n+1:N) != 0:
    calls = niters + [symmlq] + [gmres] (max(1, ceil(niters / restart)) - 1) + [shift]
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import fixtures as F
import structures as ST
from devbuf import DeviceArray
from oracle import oracle as O
from sensitivity import band

pytestmark = pytest.mark.gpu

FLOOR = 1e-8  # tests/test_gpu_parity.py
SAFETY = 10.0
OPTS = dict(F.EXPROG_OPTS)
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
TINY_COLUMNS = {"tiny1x1": (0, 0, 7.0), "tiny65x63": (13, 0, 1.0)}  # tests/test_gpu_solve_multi.py
SYM = [("cg", {}), ("cglanczos", {}), ("minres", {}), ("symmlq", {})]
# cvxqp2_s without the shift converges slowly (cpgmres(20): 415 iterations, cpdqgmres: none in 500);
# 60 iterations are three restart cycles and a full DQGMRES window, and keep the cases quick
NONSYM = [("gmres", {"restart": 20, "itmax": 60}), ("dqgmres", {"mem": 20, "itmax": 60})]
SMALL = SYM + [("gmres", {"restart": 20}), ("dqgmres", {"mem": 5})]
CASES = [("cvxqp1_m", m, e) for m, e in SYM] + [("cvxqp2_s", m, e) for m, e in NONSYM] + \
        [(s, m, e) for s in ("tiny1x1", "tiny65x63", "zero_c") for m, e in SMALL]
HISTS = ("residHistory", "cgresidHistory", "lqresidHistory", "qrresidHistory")


def system(name):
    return F.load(name) if name in ("cvxqp1_m", "cvxqp2_s", "syn_symm20k") else ST.get(name)


def column(name):
    S = system(name)
    if name in TINY_COLUMNS:
        return np.random.default_rng(1000 + TINY_COLUMNS[name][0]).standard_normal(S["n"])
    return S["rhs"][:S["n"]].copy()


_HANDLES = {}


def handles(name):
    """(A, C as Matrix handles, M with the examples' properties, its factors), built once"""
    import cpkrylov_amd as cpk
    if name not in _HANDLES:
        S = system(name)
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        M._set(**{k: OPTS[k] for k in PC_PROPS})
        Am, Cm = cpk.Matrix(S["Q"], M.ctx), cpk.Matrix(S["C"], M.ctx)
        Am @ np.zeros(S["n"])  # the device copy exists before any capture calls the SpMV
        _HANDLES[name] = (Am, Cm, M, M.export_factors())
    return _HANDLES[name]


def spmv_operator(Am, capturable, fail_at=0, exc=None, rc=7):
    """cpk.Operator around cpk_mat_spmv_device on Am; call number fail_at returns rc or raises exc"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    seen = [0]

    def fn(x, y, n, stream):
        seen[0] += 1
        if seen[0] == fail_at:
            if exc is not None:
                raise exc
            return rc
        return _lib.lib.cpk_mat_spmv_device(Am.h, x, y)

    return cpk.Operator(Am.shape[0], fn, ctx=Am.ctx, capturable=capturable)


def solve(name, method, extra, A, exact, itmax=None):
    import cpkrylov_amd as cpk
    _, Cm, M, _ = handles(name)
    opts = dict(OPTS, **extra)
    if itmax is not None:
        opts["itmax"] = itmax
    with cpk.engine_options(exact_dots=int(exact)):
        return getattr(cpk, "cp" + method)(column(name), A, Cm, M, opts)


_MATRIX = {}


def matrix_solve(name, method, extra, exact, itmax=None):
    """the matrix path's solve (the code this feature leaves alone), computed once"""
    key = (name, method, tuple(sorted(extra.items())), exact, itmax)
    if key not in _MATRIX:
        _MATRIX[key] = solve(name, method, extra, handles(name)[0], exact, itmax)
    return _MATRIX[key]


def assert_same_bits(got, want, what):
    (x, y, st, fl), (xo, yo, so, fo) = got, want
    assert st["niters"] == so["niters"], what
    assert fl == fo, what
    for k in HISTS:
        assert (k in st) == (k in so), (what, k)
        if k in so:
            assert np.array_equal(st[k], so[k]), (what, k)
    if "status" in so:
        assert st["status"] == so["status"], what
    assert np.array_equal(x, xo) and np.array_equal(y, yo), what


# ---- 1. exact mode: bit for bit the matrix path ----------------------------------------------------
@pytest.mark.parametrize("capturable", [True, False], ids=["capturable", "eager"])
@pytest.mark.parametrize("name,method,extra", CASES)
def test_exact_mode_equals_matrix_path(gpu_ctx, name, method, extra, capturable):
    """u is cpk_mat_spmv's bits, t is unchanged and exact sums have no order: niters, solved, every
    history, x and y equal the matrix-path solve, also when itmax stops the solve inside a batch."""
    A = spmv_operator(handles(name)[0], capturable)
    for itmax in (None, 1, 2, 7):
        got = solve(name, method, extra, A, True, itmax)
        assert_same_bits(got, matrix_solve(name, method, extra, True, itmax), (name, method, itmax))


# ---- 2. default mode: in the oracle's band; capturable == eager ---------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_solve(name, method, extra_items, b_bytes=None):
    S = system(name)
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=handles(name)[3])
    Mo.set(**{k: float(OPTS[k]) for k in PC_PROPS})
    b = column(name) if b_bytes is None else np.frombuffer(b_bytes)
    return O.method(method, b.copy(), S["Q"], S["C"], Mo, dict(OPTS, **dict(extra_items)))


@functools.lru_cache(maxsize=None)
def method_band(name, method, extra_items, trials=4, eps=1e-15):
    """tests/sensitivity.py at the method level: the oracle's spread under relative perturbations
    of 1e-15 of b (histories relative to history[0], [x; y] relative to its norm).  On the tiny
    members a solve ends after one iteration with a residual that is pure rounding, and a perturbed
    b can take the reference to its complex-norm stop (structures.py, TINY_SEED); such a trial has
    no result and adds nothing to the band, which only matters above the rule's floor of 1e-8."""
    x1, y1, s1 = oracle_solve(name, method, extra_items)
    out = {k: 0.0 for k in s1 if k.endswith("History")}
    out["x"] = 0.0
    rng = np.random.default_rng(12345)
    b = column(name)
    h0 = s1.get("residHistory", s1.get("cgresidHistory"))[0]
    for _ in range(trials):
        b2 = b * (1 + eps * rng.standard_normal(b.shape[0]))
        try:
            x2, y2, s2 = oracle_solve(name, method, extra_items, b2.tobytes())
        except O.OracleError:
            continue  # see the docstring
        for k in [k for k in out if k != "x"]:
            L = min(len(s1[k]), len(s2[k]))
            out[k] = max(out[k], float(np.max(np.abs(s1[k][:L] - s2[k][:L])) / h0))
        z1, z2 = np.concatenate([x1, y1]), np.concatenate([x2, y2])
        out["x"] = max(out["x"], float(np.linalg.norm(z1 - z2) / np.linalg.norm(z1)))
    return out


@pytest.mark.parametrize("name,method,extra", [c for c in CASES if c[0] != "cvxqp2_s"])
def test_default_mode_in_band_of_the_oracle(gpu_ctx, name, method, extra):
    """The method-level solve against the oracle on the product's factors: integers equal,
    histories, x and y within max(1e-8, 10 x band); capturable and eager run the same kernels on
    the same grids, so they equal each other bit for bit."""
    Am = handles(name)[0]
    cap = solve(name, method, extra, spmv_operator(Am, True), False)
    eag = solve(name, method, extra, spmv_operator(Am, False), False)
    assert_same_bits(cap, eag, (name, method))
    items = tuple(sorted(extra.items()))
    xo, yo, so = oracle_solve(name, method, items)
    bd = method_band(name, method, items)
    x, y, st, fl = cap
    assert st["niters"] == so["niters"] and fl["solved"] == so["solved"]
    h0 = so.get("residHistory", so.get("cgresidHistory"))[0]
    for k in [k for k in so if k.endswith("History")]:
        assert len(st[k]) == len(so[k]), k
        dev = np.max(np.abs(st[k] - so[k])) / h0
        print(name, method, k, "deviation", dev, "band", bd[k])
        assert dev <= max(FLOOR, SAFETY * bd[k]), (k, dev, bd[k])
    if method == "cglanczos":
        assert st["status"] == so["status"]
    z, zo = np.concatenate([x, y]), np.concatenate([xo, yo])
    dz = np.linalg.norm(z - zo) / np.linalg.norm(zo)
    print(name, method, "[x; y] deviation", dz, "band", bd["x"])
    assert dz <= max(FLOOR, SAFETY * bd["x"]), (dz, bd["x"])


PARITY = [("cvxqp1_m", m, e) for m, e in SYM] + [("cvxqp2_s", "gmres", {"restart": 20}), ("cvxqp2_s", "dqgmres", {"mem": 20})]


def reg_against_oracle(name, method, extra, A, scale=1.0, widen=None):
    """reg_cpkrylov with the operator A against the oracle's, tests/test_gpu_parity.py's rule"""
    import cpkrylov_amd as cpk
    P = F.load(name)
    opts = dict(OPTS, **extra)
    x, stats, flag = cpk.reg_cpkrylov(method, P["rhs"], A, P["B"], P["C"], P["G"], opts)
    perm = stats["M"].export_factors()[2]
    xo, so = O.reg_cpkrylov(method, P["rhs"], P["Q"], P["B"], P["C"], P["G"], opts, perm=perm)
    assert stats["niters"] == so["niters"] and flag["solved"] == so["solved"]
    bd = band(name, method, extra, perm)
    h0 = so.get("residHistory", so.get("cgresidHistory"))[0]
    for k in [k for k in so if k.endswith("History")]:
        assert len(stats[k]) == len(so[k]), k
        dev = np.max(np.abs(stats[k] - so[k])) / h0
        print(name, method, k, "deviation", dev, "band", bd[k])
        assert dev <= max(FLOOR, SAFETY * bd[k]), (k, dev, bd[k])
    dx = np.linalg.norm(x - xo) / np.linalg.norm(xo)
    print(name, method, "x deviation", dx, "band", bd["x"])
    assert dx <= max(FLOOR, SAFETY * bd["x"]), (dx, bd["x"])
    return x, stats, flag


@pytest.mark.parametrize("name,method,extra", PARITY)
def test_reg_cpkrylov_with_operator_matches_oracle(gpu_ctx, name, method, extra):
    """The driver (shift included: the fixtures' b(n+1:N) is not zero) with a capturable operator,
    held to tests/test_gpu_parity.py's bar for the matrix path."""
    import cpkrylov_amd as cpk
    P = F.load(name)
    Am = cpk.Matrix(P["Q"], gpu_ctx)
    Am @ np.zeros(P["n"])
    A = spmv_operator(Am, True)
    reg_against_oracle(name, method, extra, A)
    assert A.info()["failed"] == 0 and A.info()["calls"] >= 2


# ---- 3. genuinely matrix-free: a dense torch product ------------------------------------------------
@pytest.mark.parametrize("method", [m for m, _ in SYM])
@pytest.mark.parametrize("name", ["cvxqp1_m", "tiny65x63"])
def test_from_torch_dense_product(gpu_ctx, name, method):
    """Operator.from_torch with torch.mv on the dense A, default mode, against the oracle on the
    sparse A with the band rule: the dense row sums round differently and nothing else differs.

    CPU check before relying on it (tools/operator_dense_check.py, no GPU): a row sum taken in
    another order is the exact sum of entries perturbed by relative amounts of at most (row
    length) x 2^-53 (the backward-error bound of recursive summation), so the oracle was run on A
    with every entry perturbed by 2^-53 x (its row's length) x U(-1, 1), four seeds.  The integers
    never moved, and the largest deviations stayed inside max(1e-8, 10 x band) everywhere:
    cvxqp1_m through reg_cpkrylov, histories / x against the rule's bound: cg 2.2e-12 / 1.6e-12
    (1e-8), cglanczos 4.7e-10 / 3.9e-10 (2.7e-8 / 2.2e-8), minres 1.2e-10 / 9.3e-15 (1e-8), symmlq
    at most 1.6e-9 (lqresid, bound 8.9e-8) / 3.9e-10 (2.2e-8); tiny65x63 on this test's column, at
    most 6.7e-11 (histories) / 6.0e-10 ([x; y], symmlq) against the floor of 1e-8.  No case is
    widened."""
    import torch

    import cpkrylov_amd as cpk
    if name == "cvxqp1_m":
        P = F.load(name)
        Ad = torch.tensor(P["Q"].toarray(), dtype=torch.float64, device="cuda")
        A = cpk.Operator.from_torch(P["n"], lambda v: torch.mv(Ad, v), ctx=gpu_ctx)
        reg_against_oracle(name, method, {}, A)
        return
    S = system(name)
    _, Cm, M, _ = handles(name)
    Ad = torch.tensor(S["Q"].toarray(), dtype=torch.float64, device="cuda")
    A = cpk.Operator.from_torch(S["n"], lambda v: torch.mv(Ad, v), ctx=M.ctx)
    x, y, st, fl = getattr(cpk, "cp" + method)(column(name), A, Cm, M, OPTS)
    xo, yo, so = oracle_solve(name, method, ())
    bd = method_band(name, method, ())
    assert st["niters"] == so["niters"] and fl["solved"] == so["solved"]
    h0 = so.get("residHistory", so.get("cgresidHistory"))[0]
    for k in [k for k in so if k.endswith("History")]:
        assert len(st[k]) == len(so[k]), k
        dev = np.max(np.abs(st[k] - so[k])) / h0
        print(name, method, k, "deviation", dev, "band", bd[k])
        assert dev <= max(FLOOR, SAFETY * bd[k]), (k, dev, bd[k])
    z, zo = np.concatenate([x, y]), np.concatenate([xo, yo])
    dz = np.linalg.norm(z - zo) / np.linalg.norm(zo)
    print(name, method, "[x; y] deviation", dz, "band", bd["x"])
    assert dz <= max(FLOOR, SAFETY * bd["x"]), (dz, bd["x"])
    assert A.info()["calls"] == st["niters"] + (1 if method == "symmlq" else 0)


# ---- 4. the driver in exact mode -----------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [True, False], ids=["capturable", "eager"])
@pytest.mark.parametrize("name,method", [("cvxqp1_m", "minres"), ("cvxqp1_m", "cg"), ("cvxqp1_m", "symmlq"),
                                         ("tiny65x63", "minres"), ("tiny65x63", "gmres")])
def test_reg_cpkrylov_exact_equals_matrix_path(gpu_ctx, name, method, capturable):
    """b(n+1:N) != 0, so the shift calls fn once; under exact_dots x, the histories and the
    integers equal the matrix path's."""
    import cpkrylov_amd as cpk
    S = system(name)
    b = S["rhs"].copy()  # the members' own rhs: the reg_cpkrylov solves of tests/test_gpu_structures.py
    assert np.any(b[S["n"]:] != 0)
    Am = cpk.Matrix(S["Q"], gpu_ctx)
    Am @ np.zeros(S["n"])
    A = spmv_operator(Am, capturable)
    with cpk.engine_options(exact_dots=1):
        x, st, fl = cpk.reg_cpkrylov(method, b, A, S["B"], S["C"], S["G"], OPTS)
        xm, sm, fm = cpk.reg_cpkrylov(method, b, Am, S["B"], S["C"], S["G"], OPTS)
    assert st["niters"] == sm["niters"] and fl == fm
    for k in HISTS:
        if k in sm:
            assert np.array_equal(st[k], sm[k]), k
    assert np.array_equal(x, xm)
    if not capturable:
        R = 50
        want = st["niters"] + (1 if method == "symmlq" else 0) + 1 + \
            ((max(1, -(-st["niters"] // R)) - 1) if method == "gmres" else 0)
        assert A.info()["calls"] == want, (A.info(), st["niters"])


# ---- 5. call counts and caching ----------------------------------------------------------------------
def expected_calls(method, extra, niters, shift=0):
    R = int(extra.get("restart", 50))
    return niters + (1 if method == "symmlq" else 0) + \
        ((max(1, -(-niters // R)) - 1) if method == "gmres" else 0) + shift


@pytest.mark.parametrize("name,method,extra", [c for c in CASES if c[0] in ("cvxqp1_m", "cvxqp2_s", "zero_c")])
def test_eager_call_count_is_exact(gpu_ctx, name, method, extra):
    """An eager operator is called once per running Krylov product (the formula in the module
    docstring) and its solves never instantiate a graph."""
    _, _, M, _ = handles(name)
    A = spmv_operator(handles(name)[0], False)
    inst = M.solver_info()["graph_instantiations"]
    x, y, st, fl = solve(name, method, extra, A, False)
    assert st["niters"] > 0
    assert A.info() == {"n": system(name)["n"], "capturable": False,
                        "calls": expected_calls(method, extra, st["niters"]), "failed": 0}
    assert M.solver_info()["graph_instantiations"] == inst


def device_solve(name, method, A, d_b, d_xy, opts, Cm=None, M=None):
    """cpk_method_solve_op_device on fixed device vectors (the cached solver is keyed by them)"""
    from cpkrylov_amd import _lib, api
    if M is None:
        _, Cm, M, _ = handles(name)
    S = system(name)
    st, hist, lq, qr = api._new_stats(api._hist_cap(method, opts, S["n"], S["m"]))
    rc = _lib.lib.cpk_method_solve_op_device(M.ctx.h, _lib.METHODS[method], d_b.p, A.h, Cm.h, M.h,
                                             C.byref(_lib.make_opts(opts)), d_xy.p, C.byref(st))
    return rc, api._stats_from(method, st, hist, lq, qr), d_xy.numpy()


@pytest.mark.parametrize("method", ["minres", "cg", "symmlq"])
def test_capturable_second_solve_replays(gpu_ctx, method):
    """A second identical solve with a capturable operator replays the cached graphs: no further
    call of fn from an iteration, no instantiation, the same bits.  cpsymmlq's pre-step is not part
    of an iteration: it runs outside the graphs and calls fn once per solve."""
    name = "cvxqp1_m"
    S = system(name)
    _, _, M, _ = handles(name)
    A = spmv_operator(handles(name)[0], True)
    d_b, d_xy = DeviceArray.of(column(name)), DeviceArray(S["n"] + S["m"])
    rc, (st1, fl1), xy1 = device_solve(name, method, A, d_b, d_xy, OPTS)
    assert rc == 0 and fl1["solved"]
    calls, info = A.info()["calls"], M.solver_info()
    assert calls > 0 and info["graph_instantiations"] > 0
    rc, (st2, fl2), xy2 = device_solve(name, method, A, d_b, d_xy, OPTS)
    assert rc == 0
    assert A.info()["calls"] == calls + (1 if method == "symmlq" else 0)
    assert M.solver_info() == info
    assert st1["niters"] == st2["niters"] and fl1 == fl2 and np.array_equal(xy1, xy2)
    for k in HISTS:
        if k in st1:
            assert np.array_equal(st1[k], st2[k]), k


# ---- 6. C refresh ------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [True, False], ids=["capturable", "eager"])
def test_operator_follows_set_values_on_C(gpu_ctx, capturable):
    """After set_values on C the operator's blkdiag(0, C) holds the new values at the same address:
    the solve (cached graphs included) has the bits of one on fresh handles."""
    import cpkrylov_amd as cpk
    name = "cvxqp1_m"
    S = system(name)
    Am = handles(name)[0]
    ctx = Am.ctx

    def precond(Cmat):  # a constraint preconditioner holds K's own C: it follows the update by a refactor
        M = cpk.opLDL2(S["G"], S["B"], -Cmat, ctx=ctx)
        M._set(**{k: OPTS[k] for k in PC_PROPS})
        return M

    C2 = (S["C"] * 1.5).tocsr()
    Cm, M = cpk.Matrix(S["C"], ctx), precond(S["C"])
    A = spmv_operator(Am, capturable)
    b = column(name)
    d_b, d_xy = DeviceArray.of(b), DeviceArray(S["n"] + S["m"])  # fixed vectors: the solver stays cached
    rc, _, before = device_solve(name, "minres", A, d_b, d_xy, OPTS, Cm, M)
    assert rc == 0
    info = M.solver_info()
    Cm.set_values(C2)
    M.refactor(S["G"], S["B"], -C2)
    rc, (st, fl), after = device_solve(name, "minres", A, d_b, d_xy, OPTS, Cm, M)
    assert rc == 0 and M.solver_info() == info  # the cached solver and its graphs, on the refreshed operator
    x, y, sf, ff = cpk.cpminres(b, spmv_operator(Am, capturable), cpk.Matrix(C2, ctx), precond(C2), OPTS)
    assert st["niters"] == sf["niters"] and fl == ff and np.array_equal(st["residHistory"], sf["residHistory"])
    assert np.array_equal(after, np.concatenate([x, y]))
    assert not np.array_equal(before, after)  # C entered the solve


# ---- 7. failures -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["minres", "cg"])
@pytest.mark.parametrize("capturable,fail_at", [(False, 3), (True, 2)], ids=["eager-third", "capture-second"])
def test_callback_failure_is_a_status(gpu_ctx, method, capturable, fail_at):
    """fn returning nonzero (the eager one on its third call, the capturable one on its second,
    which is inside a capture) gives CPK_ERR_CALLBACK naming the call; afterwards a sound operator
    on the same M gives case 1's bits: no capture is left open, no solver is poisoned."""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    name = "cvxqp1_m"
    Am = handles(name)[0]
    bad = spmv_operator(Am, capturable, fail_at=fail_at)
    with pytest.raises(cpk.CpkError) as e:
        solve(name, method, {}, bad, True)
    assert e.value.code == _lib.CPK_ERR_CALLBACK == 9
    assert f"call {fail_at}" in str(e.value) and e.value.__cause__ is None
    assert bad.info()["calls"] == fail_at and bad.info()["failed"] == 1
    good = solve(name, method, {}, spmv_operator(Am, capturable), True)
    assert_same_bits(good, matrix_solve(name, method, {}, True), (method, "after a failure"))
    # the failed handle itself stays usable once its callback is sound again (call fail_at is past)
    assert_same_bits(solve(name, method, {}, bad, True), matrix_solve(name, method, {}, True), "same handle")


@pytest.mark.parametrize("capturable", [True, False], ids=["capturable", "eager"])
def test_python_exception_is_the_cause(gpu_ctx, capturable):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    name = "cvxqp1_m"
    boom = ValueError("no product today")
    bad = spmv_operator(handles(name)[0], capturable, fail_at=2, exc=boom)
    with pytest.raises(cpk.CpkError) as e:
        solve(name, "minres", {}, bad, False)
    assert e.value.code == _lib.CPK_ERR_CALLBACK and e.value.__cause__ is boom
    assert_same_bits(solve(name, "minres", {}, spmv_operator(handles(name)[0], capturable), True),
                     matrix_solve(name, "minres", {}, True), "after an exception")


# ---- 8. refusals leave the outputs untouched -------------------------------------------------------------
def raw_solve(ctx, A_h, Cm, M, n, m):
    """cpk_method_solve_op on sentinel-filled outputs: (rc, x, y)"""
    from cpkrylov_amd import _lib, api
    b, x, y = np.ones(n), np.full(n, -3.5), np.full(max(m, 1), -4.5)
    st, *_ = api._new_stats(api._hist_cap("minres", OPTS, n, m))
    rc = _lib.lib.cpk_method_solve_op(ctx.h, _lib.METHODS["minres"], api._dptr(b), A_h, Cm.h, M.h,
                                      C.byref(_lib.make_opts(OPTS)), api._dptr(x), api._dptr(y), C.byref(st))
    return rc, x, y


def test_refusals_write_nothing(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    name = "tiny65x63"
    S = system(name)
    n, m = S["n"], S["m"]
    Am, Cm, M, _ = handles(name)
    # an n that differs from M's
    wrong = cpk.Operator(n + 1, lambda *a: 0, ctx=M.ctx)
    rc, x, y = raw_solve(M.ctx, wrong.h, Cm, M, n, m)
    assert rc == _lib.CPK_ERR_DIM and np.all(x == -3.5) and np.all(y == -4.5)
    # a NULL fn
    h = C.c_void_p()
    assert _lib.lib.cpk_op_create(M.ctx.h, n, _lib.OpFn(), None, 0, C.byref(h)) == 0
    try:
        rc, x, y = raw_solve(M.ctx, h, Cm, M, n, m)
        assert rc == _lib.CPK_ERR_ARGS and np.all(x == -3.5) and np.all(y == -4.5)
        d = DeviceArray(n)
        assert _lib.lib.cpk_op_apply_device(h, d.p, d.p) == _lib.CPK_ERR_ARGS
    finally:
        _lib.lib.cpk_op_destroy(h)
    assert wrong.info()["calls"] == 0
    # a block b, and K with an Operator: refused in Python, before any C entry
    A = spmv_operator(Am, False)
    for call in (lambda: cpk.cpminres(np.ones((n, 2)), A, Cm, M, OPTS),
                 lambda: cpk.reg_cpkrylov("minres", np.ones((n + m, 2)), A, S["B"], S["C"], S["G"], OPTS),
                 lambda: cpk.KKT(A, S["B"], S["C"], ctx=M.ctx),
                 lambda: cpk.opLDL2(A, S["B"], -S["C"], ctx=M.ctx)):
        with pytest.raises(cpk.CpkError) as e:
            call()
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
    K = cpk.KKT(Am, S["B"], Cm, ctx=M.ctx)
    with pytest.raises(cpk.CpkError) as e:
        K.solve("minres", np.ones(n + m), A)
    assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
    assert A.info()["calls"] == 0


def test_distributed_preconditioner_is_refused(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S = system("tiny65x63")
    n, m = S["n"], S["m"]
    g = cpk.SimGroup(1)
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=g, options=dict(dist1=1))
    try:
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        Cm = cpk.Matrix(S["C"], ctx)
        A = cpk.Operator(n, lambda *a: 0, ctx=ctx)
        rc, x, y = raw_solve(ctx, A.h, Cm, M, n, m)
        assert rc == _lib.CPK_ERR_UNSUPPORTED and np.all(x == -3.5) and np.all(y == -4.5)
        assert A.info()["calls"] == 0
        del M, Cm, A
    finally:
        ctx.close()


# ---- 9. cpk_mat_spmv_device ---------------------------------------------------------------------------
def spmv_matrices():
    E = ST.get("empty_rows")
    return {"cvxqp1_m": F.load("cvxqp1_m")["Q"], "cvxqp2_s": F.load("cvxqp2_s")["Q"],
            "syn_symm20k": F.load("syn_symm20k")["Q"], "empty_rows_B": E["B"],
            "zero_c_C": ST.get("zero_c")["C"], "tiny1x1": ST.get("tiny1x1")["Q"],
            "cvxqp1_m_blkdiag0C": sp.block_diag([sp.csr_matrix((3, 3)), F.load("cvxqp1_m")["C"]]).tocsr()}


@pytest.mark.parametrize("which", ["cvxqp1_m", "cvxqp2_s", "syn_symm20k", "empty_rows_B", "zero_c_C", "tiny1x1",
                                   "cvxqp1_m_blkdiag0C"])
def test_spmv_device_equals_spmv(gpu_ctx, which):
    """The same kernel on the same row blocks: device vectors in, the host entry's bits out."""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    A = spmv_matrices()[which]
    Am = cpk.Matrix(A, gpu_ctx)
    x = np.random.default_rng(5).standard_normal(A.shape[1])
    want = Am @ x
    d_x, d_y = DeviceArray.of(x), DeviceArray.of(np.full(A.shape[0], np.nan))
    assert _lib.lib.cpk_mat_spmv_device(Am.h, d_x.p, d_y.p) == 0
    gpu_ctx.synchronize()
    assert np.array_equal(d_y.numpy(), want)
    if which == "empty_rows_B":
        assert np.any(np.diff(A.indptr) == 0)
