"""The refined apply Y = M*X for a block of right-hand sides on the GPU (cpk_pc_apply_multi, the
panel kernels of multiapply.hip and multisweep.hip): column j of Y is M * X[:, j] -- opLDL2.multiply
(ops/opLDL2.m:161-188) on that column, as the reference's double(op) forms it -- bit for bit, each
column with its own refinement predicate.

Reference: the oracle's LDL2 on the product's exported factors with the same properties, applied
column by column and compared with np.array_equal.  The step counts come from replaying the loop
of opLDL2.m:174-185 on the oracle's iterates (y after s forced steps); every decision the replay
meets must have ||r|| / ||x|| at least 4x away from itref_tol on either side, else the test
fails as mis-specified (the all-zero column's 0 >= 0 is exempt).

Systems and tolerances (the ratios before the first step and after one step, measured with the
oracle on the host analysis' factors, fix the tolerances so that columns of one panel provably
stop at different steps):
  band_g     normal 4.7e-8...1.1e-7 -> ~2e-10, hub 1.2e-14, Kp*v 3.4e-12   itref_tol 1e-8 (default)
  band_g_nd  normal 2.7e-8...3.5e-8 -> ~2e-10, hub 7.8e-14, Kp*v 1.8e-12   itref_tol 2e-9 (1e-8 would
             sit within 4x of the normal columns' ratio)
  cvxqp1_m   normal >= 1.1e-11, hub 2.0e-16, Kp*v 1.3e-16                  itref_tol 1e-13
  dense_col  normal >= 2.1e-11, hub 3.4e-16, Kp*v 5.2e-16                  itref_tol 1e-13
  arrow_row  normal >= 1.3e-10, hub 1.2e-13, Kp*v 1.3e-16                  itref_tol 1e-12
  zero_c     normal >= 4.6e-10, hub 1.2e-16, Kp*v 1.1e-16                  itref_tol 1e-12
  tiny members: rounding-level ratios, so force_itref only (3 steps everywhere)
Columns: those of test_gpu_ldl_factor.py -- standard normal (seed 7), one all-zero column, the
hub unit vector -- and a column Kp*v.  The operators of _case are built with the engine option
that forces the panel kernels, so every k runs them whatever the routing; the routed entry has
its own test."""
import ctypes as C

import numpy as np
import pytest

import fixtures as F
import structures as ST
from devbuf import DeviceArray
from oracle import oracle as O
from test_gpu_dist import _run_ranks
from test_gpu_ldl_factor import Mex2
from test_mex_shim import _expect_error, _factors, _gpu_mex

pytestmark = pytest.mark.gpu

TINY = ["tiny1x1", "tiny2x1", "tiny3x2", "tiny65x63"]
NAMES = TINY + ["band_g", "dense_col", "arrow_row", "zero_c", "band_g_nd", "cvxqp1_m"]
TOL = dict(band_g=1e-8, band_g_nd=2e-9, cvxqp1_m=1e-13, dense_col=1e-13, arrow_row=1e-12, zero_c=1e-12)
KS = [1, 2, 7, 8, 9, 17]  # below, at and just above one panel of 8; two panels plus one
KMAX = max(KS)
MARGIN = 4.0
_CACHE = {}
_ITER = {}


def _system(name):
    return F.load(name) if name == "cvxqp1_m" else ST.get(name)


def _props(name):
    """the properties a system is tested under (module docstring)"""
    if name in TOL:
        return dict(nitref=3.0, itref_tol=TOL[name], force_itref=False)
    return dict(nitref=3.0, itref_tol=1e-8, force_itref=True)


def _columns(S):
    """N x 17: standard normal (seed 7) with column 1 all zero, column 2 the hub's unit vector and
    column 3 = Kp*v, so every k >= 4 holds all four kinds"""
    N = S["n"] + S["m"]
    X = np.random.default_rng(7).standard_normal((N, KMAX))
    X[:, 1] = 0.0
    X[:, 2] = 0.0
    X[ST.hub(S), 2] = 1.0
    X[:, 3] = ST.kp(S) @ np.random.default_rng(8).standard_normal(N)
    return X


def _set(M, Mo, props):
    for k, v in props.items():
        setattr(M, k, v)
    Mo.set(**{k: float(v) for k, v in props.items()})


def _ratio(name, j, s):
    """||x - Kp*y_s|| / ||x|| for column j, y_s the oracle's iterate after s forced steps"""
    key = (name, j, s)
    if key not in _ITER:
        S, _, Mo, X, _, _ = _case(name)
        saved = Mo.props()
        Mo.set(nitref=float(s), force_itref=1.0)
        y = Mo @ X[:, j]
        Mo.set(**saved)
        x = X[:, j]
        _ITER[key] = np.linalg.norm(x - ST.kp(S) @ y) / np.linalg.norm(x)
    return _ITER[key]


def _replay(name, j, nitref, tol, force):
    """opLDL2.m:174-185 for column j: the refinement solves it takes.  A decision within MARGIN of
    the tolerance makes the test mis-specified (a failure, not a pass by luck)."""
    X = _case(name)[3]
    nit = 0
    while nit < nitref:
        if not force:
            if np.any(X[:, j]):
                q = _ratio(name, j, nit)
                assert q >= MARGIN * tol or q <= tol / MARGIN, \
                    f"mis-specified: {name} column {j} step {nit}: ||r||/||x|| = {q:.3e} against itref_tol {tol:.1e}"
                if q < tol:
                    break
            # the all-zero column: 0 >= tol * 0 holds at every step
        nit += 1
    return nit


def _case(name):
    """(system, operator on the panel kernels, oracle operator, X, oracle's Y, replayed counts)
    under _props(name), built once per member; read-only (a test that changes properties puts
    them back)"""
    if name not in _CACHE:
        import cpkrylov_amd as cpk
        S = _system(name)
        with cpk.engine_options(apply_multi_panel=1):
            M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
        p = _props(name)
        _set(M, Mo, p)
        X = _columns(S)
        kmax = 9 if name == "band_g_nd" else KMAX  # band_g_nd: one k only
        Yo = np.column_stack([Mo @ X[:, j] for j in range(kmax)])
        X.setflags(write=False), Yo.setflags(write=False)
        _CACHE[name] = [S, M, Mo, X, Yo, None]
        _CACHE[name][5] = np.array([_replay(name, j, 3, p["itref_tol"], p["force_itref"]) for j in range(kmax)], np.int32)
    return _CACHE[name]


def _multi_device(M, X, ldx, ldy, sentinel=-7.25, nit=True):
    """cpk_pc_apply_multi_device on padded column-major buffers; returns (rc, Y as ldy x k, counts)"""
    from cpkrylov_amd import _lib
    N, k = X.shape
    Xp = np.full((k, ldx), np.nan)  # row j of this C array = column j with leading dimension ldx
    Xp[:, :N] = X.T
    dX, dY = DeviceArray.of(Xp), DeviceArray.of(np.full((k, ldy), sentinel))
    dn = DeviceArray.of(np.full(k + 2 - k % 2, -1, np.int32).view(np.float64))  # int32 counts, sentinel -1
    rc = _lib.lib.cpk_pc_apply_multi_device(M.h, k, dX.p, ldx, dY.p, ldy, dn.p if nit else None)
    return rc, dY.numpy().reshape(k, ldy).T, dn.numpy().view(np.int32)[:k]


def _check_block(M, X, Yo, nit_o, ks, what):
    N = X.shape[0]
    for k in ks:
        for order in ("C", "F"):
            Y, nit = M.apply_block(np.array(X[:, :k], order=order), return_steps=True)
            assert Y.shape == (N, k) and nit.shape == (k,) and nit.dtype == np.int32
            for j in range(k):
                assert np.array_equal(Y[:, j], Yo[:, j]), (what, k, order, j, np.max(np.abs(Y[:, j] - Yo[:, j])))
            assert np.array_equal(nit, nit_o[:k]), (what, k, order, nit, nit_o[:k])
            assert np.array_equal(M @ np.array(X[:, :k], order=order), Y) or k == 1
        rc, Yd, nd = _multi_device(M, X[:, :k], N + 3, N + 5)
        assert rc == 0
        assert np.array_equal(Yd[:N], Yo[:, :k]), (what, k)
        assert np.all(Yd[N:] == -7.25), (what, k)  # the padding rows of Y are untouched
        assert np.array_equal(nd, nit_o[:k]), (what, k, nd, nit_o[:k])


# ---- 1. bit equality ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bit_equal_to_the_column_loop(gpu_ctx, name):
    S, M, Mo, X, Yo, nit_o = _case(name)
    N = S["n"] + S["m"]
    if name == "band_g_nd":  # the large member: a single apply
        Y, nit = M.apply_block(X[:, :9], return_steps=True)
        for j in range(9):
            assert np.array_equal(Y[:, j], Yo[:, j]), (name, j)
        assert list(nit) == list(nit_o) and list(nit[:4]) == [1, 3, 0, 0]
        return
    _check_block(M, X, Yo, nit_o, KS, name)
    # the product's own single-column apply, and the (N, 1) and 1-D forms, which keep their path
    for j in range(min(4, Yo.shape[1])):
        assert np.array_equal(M * X[:, j], Yo[:, j]), (name, j)
    y1 = M @ X[:, :1]
    assert y1.shape == (N,) and np.array_equal(y1, Yo[:, 0])
    if name in TOL:  # the table's counts for (normal, zero, hub): columns stop at different steps
        want = [1, 3, 0] if name in ("band_g", "band_g_nd") else [3, 3, 0]
        assert list(nit_o[:3]) == want and nit_o[3] == 0, (name, nit_o)
    else:
        assert np.all(nit_o == 3)


@pytest.mark.parametrize("name", ["cvxqp1_m", "band_g", "tiny65x63"])
def test_routed_entry(gpu_ctx, name):
    """an operator built without the forcing option: whatever path a panel takes, the same bits"""
    import cpkrylov_amd as cpk
    S, M, Mo, X, Yo, nit_o = _case(name)
    M2 = cpk.opLDL2(S["G"], S["B"], -S["C"])
    for k, v in _props(name).items():
        setattr(M2, k, v)
    _check_block(M2, X, Yo, nit_o, KS, name)


# ---- 2. mixed step counts in one panel ----------------------------------------------------------
def test_mixed_step_counts(gpu_ctx):
    S, M, Mo, X, Yo, nit_o = _case("band_g")
    assert M.itref_tol == 1e-8 and not M.force_itref and M.nitref == 3  # the defaults
    Y, nit = M.apply_block(X[:, :8], return_steps=True)
    assert list(nit[:4]) == [1, 3, 0, 0] and set(nit) == {0, 1, 3}
    Y0 = M.H @ X[:, :8]  # nitref = 0: no refinement
    M.force_itref = True
    try:
        Y3 = M.apply_block(X[:, :8])  # three steps everywhere
    finally:
        M.force_itref = False
    # the normal column took one step: neither the unrefined nor the fully refined result
    assert not np.array_equal(Y[:, 0], Y0[:, 0]) and not np.array_equal(Y[:, 0], Y3[:, 0])
    assert np.array_equal(Y[:, 2], Y0[:, 2])  # the hub column never refined
    assert np.array_equal(Y[:, 1], Y3[:, 1]) and not np.any(Y[:, 1])  # the zero column: all steps, still zero
    assert np.array_equal(Y, Yo[:, :8])


# ---- 3. property grid ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cvxqp1_m", "tiny65x63"])
def test_property_grid(gpu_ctx, name):
    S, M, Mo, X, Yo, _ = _case(name)
    k = 9
    YH = M.H @ X[:, :k]
    try:
        for nitref in (0, 1, 3):
            for force in (False, True):
                for tol in sorted({1e-8, TOL.get(name, 1e-8)}):
                    props = dict(nitref=nitref, itref_tol=tol, force_itref=force)
                    _set(M, Mo, props)
                    Y, nit = M.apply_block(X[:, :k], return_steps=True)
                    want = [_replay(name, j, nitref, tol, force) for j in range(k)]
                    assert list(nit) == want, (props, nit, want)
                    for j in range(k):
                        assert np.array_equal(Y[:, j], Mo @ X[:, j]), (props, j)
                        if j < 4:
                            assert np.array_equal(Y[:, j], M * X[:, j]), (props, j)
                    if nitref == 0:
                        assert np.array_equal(Y, YH), props
                    M.residual_update = True  # without handle semantics: the no-op it already is
                    try:
                        Yr, nr = M.apply_block(X[:, :k], return_steps=True)
                    finally:
                        M.residual_update = False
                    assert np.array_equal(Yr, Y) and np.array_equal(nr, nit), props
    finally:
        _set(M, Mo, _props(name))


# ---- 4. engine options --------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(sweep="64,128,64"), dict(no_chain=1), dict(chain_wide=2 ** 24), dict()],
                         ids=["sweep=64,128,64", "no_chain", "chain_wide", "panel_only"])
def test_engine_options(gpu_ctx, options):
    """the panel kernels read the schedule these options built: still bit-equal to the oracle, and
    the forcing option runs them at k = 1 and 2 as well"""
    import cpkrylov_amd as cpk
    S, _, _, X, Yo, nit_o = _case("dense_col")
    with cpk.engine_options(apply_multi_panel=1, **options) as ctx:
        assert ctx.get_option("apply_multi_panel") == "1"
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    assert cpk.default_context().get_option("apply_multi_panel") == "0"
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
    _set(M, Mo, _props("dense_col"))
    if "sweep" in options:  # the clique's rows of up to 314 entries are above a cap of 128
        assert M.multi_info()["direct_blocks"] >= 1
    for k in (1, 2, 9):
        Y, nit = M.apply_block(X[:, :k], return_steps=True)
        for j in range(k):
            assert np.array_equal(Y[:, j], Mo @ X[:, j]), (options, k, j)
            assert np.array_equal(Y[:, j], M * X[:, j]), (options, k, j)
        assert np.array_equal(nit, nit_o[:k]), (options, k, nit)
    M.force_itref = True
    Mo.set(force_itref=1.0)
    Y = M.apply_block(X[:, :9])
    for j in range(9):
        assert np.array_equal(Y[:, j], Mo @ X[:, j]), (options, "forced", j)


# ---- 5. isolation -------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True], ids=["predicate", "forced"])
def test_a_nan_stays_in_its_column(gpu_ctx, force):
    S, M, Mo, X, Yo, nit_o = _case("band_g")
    Xn = np.array(X[:, :9])
    Xn[17, 4] = np.nan
    M.force_itref = force
    Mo.set(force_itref=float(force))
    try:
        Y, nit = M.apply_block(Xn, return_steps=True)
        yn = M * Xn[:, 4]
        for j in range(9):
            if j != 4:
                assert np.array_equal(Y[:, j], Mo @ X[:, j]), (force, j)
    finally:
        M.force_itref = False
        Mo.set(force_itref=0.0)
    assert np.isnan(Y[:, 4]).any() and np.array_equal(Y[:, 4], yn, equal_nan=True)
    assert nit[4] == (3 if force else 0)  # NaN >= tol * NaN is false: the column never refines
    if not force:
        assert np.array_equal(np.delete(nit, 4), np.delete(nit_o[:9], 4))


# ---- 6. state -----------------------------------------------------------------------------------
def test_handle_state_is_refused_and_untouched(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S, _, _, X, _, _ = _case("cvxqp1_m")
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    props = dict(nitref=1, itref_tol=1e-9, force_itref=True, residual_update=True)
    for k, v in props.items():
        setattr(M, k, v)
    M.handle_semantics = True
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
    Mo.set(**{k: float(v) for k, v in props.items()})
    Mo.set_handle(True)
    z1, z2 = X[:, 0], X[:, 4]
    yo1, yo2 = Mo @ z1, Mo @ z2
    y1 = M * z1
    with pytest.raises(_lib.CpkError) as e:
        M.apply_block(X[:, :9])
    assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
    rc, Yd, _ = _multi_device(M, X[:, :2], M.n, M.n)
    assert rc == _lib.CPK_ERR_UNSUPPORTED and np.all(Yd == -7.25)
    y2 = M * z2
    assert np.array_equal(y1, yo1) and np.array_equal(y2, yo2)  # nothing was moved
    assert not np.array_equal(yo2, Mo @ z2)  # the oracle's state does move: the check above can fail
    assert (M.nitref, M.itref_tol, M.force_itref, M.residual_update) == (1.0, 1e-9, True, 1.0)
    # residual_update off: the block apply runs again, handle semantics or not
    M.residual_update = False
    Mo.set(residual_update=0.0)
    Y = M.apply_block(X[:, :3])
    for j in range(3):
        assert np.array_equal(Y[:, j], Mo @ X[:, j]), j


def test_properties_and_the_bare_operator_after_a_block_apply(gpu_ctx):
    S, M, Mo, X, Yo, nit_o = _case("cvxqp1_m")
    before = (M.nitref, M.itref_tol, M.force_itref, M.residual_update)
    YH = M.H @ X[:, :9]
    Y = M.apply_block(X[:, :9])
    assert (M.nitref, M.itref_tol, M.force_itref, M.residual_update) == before == (3.0, 1e-13, False, 0.0)
    # the sweeps' work array is shared with the bare block apply
    assert np.array_equal(M.H @ X[:, :9], YH) and np.array_equal(M.apply_block(X[:, :9]), Y)
    assert not np.array_equal(Y[:, 0], YH[:, 0]) and np.array_equal(Y[:, 2], YH[:, 2])
    Mo.set(nitref=0.0)
    try:
        for j in range(3):
            assert np.array_equal(YH[:, j], Mo @ X[:, j]), j
    finally:
        Mo.set(nitref=3.0)


# ---- 7. errors ----------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    from cpkrylov_amd import _lib
    S, M, Mo, X, Yo, _ = _case("tiny65x63")
    N = S["n"] + S["m"]
    rc, Yd, nd = _multi_device(M, X[:, :0], N, N)  # k = 0 does nothing
    assert rc == 0
    Y, nit = M.apply_block(np.zeros((N, 0)), return_steps=True)
    assert Y.shape == (N, 0) and nit.shape == (0,)
    assert (M @ np.zeros((N, 0))).shape == (N, 0)
    dX, dY = DeviceArray.of(X[:, :2].T), DeviceArray.of(np.full(2 * N, -7.25))
    L = _lib.lib
    assert L.cpk_pc_apply_multi_device(M.h, -1, dX.p, N, dY.p, N, None) == _lib.CPK_ERR_DIM
    assert L.cpk_pc_apply_multi_device(M.h, 2, dX.p, N - 1, dY.p, N, None) == _lib.CPK_ERR_DIM
    assert L.cpk_pc_apply_multi_device(M.h, 2, dX.p, N, dY.p, N - 1, None) == _lib.CPK_ERR_DIM
    assert L.cpk_pc_apply_multi_device(M.h, 2, dX.p, N, dX.p, N, None) == _lib.CPK_ERR_ARGS  # X aliases Y
    half = C.c_void_p(dX.p.value + 8 * N)  # Y starts at the second column of X
    assert L.cpk_pc_apply_multi_device(M.h, 2, dX.p, N, half, N, None) == _lib.CPK_ERR_ARGS  # a partial overlap
    assert L.cpk_pc_apply_multi_device(M.h, 1, dX.p, N, half, N, None) == 0  # one column each: disjoint
    assert np.all(dY.numpy() == -7.25)  # the refused calls wrote nothing
    Xh, Yh = np.asfortranarray(X[:, :2]), np.full((N, 2), -7.25, order="F")
    P = C.POINTER(C.c_double)
    assert L.cpk_pc_apply_multi(M.h, 2, Xh.ctypes.data_as(P), N - 1, Yh.ctypes.data_as(P), N, None) == _lib.CPK_ERR_DIM
    assert L.cpk_pc_apply_multi(M.h, 2, Xh.ctypes.data_as(P), N, Xh.ctypes.data_as(P), N, None) == _lib.CPK_ERR_ARGS
    assert np.all(Yh == -7.25) and np.array_equal(Xh, X[:, :2])
    for bad in (np.ones((N + 1, 2)), np.ones((N - 1, 3))):
        with pytest.raises(_lib.CpkError) as e:
            M @ bad
        assert e.value.code == _lib.CPK_ERR_DIM
        with pytest.raises(_lib.CpkError) as e:
            M.apply_block(bad)
        assert e.value.code == _lib.CPK_ERR_DIM
    with pytest.raises(_lib.CpkError) as e:
        M.apply_block(np.ones(N))  # a block is two-dimensional
    assert e.value.code == _lib.CPK_ERR_DIM


def test_distributed_is_refused(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S, _, _, X, _, _ = _case("dense_col")
    N = S["n"] + S["m"]
    P = C.POINTER(C.c_double)

    def work(ctx, r):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        Xh, Yh = np.asfortranarray(X[:, :2]), np.full((N, 2), -7.25, order="F")
        rc = _lib.lib.cpk_pc_apply_multi(M.h, 2, Xh.ctypes.data_as(P), N, Yh.ctypes.data_as(P), N, None)
        return rc, bool(np.all(Yh == -7.25))

    for rc, untouched in _run_ranks(2, work):
        assert rc == _lib.CPK_ERR_UNSUPPORTED and untouched


# ---- 8. to_dense --------------------------------------------------------------------------------
def test_to_dense(gpu_ctx):
    S, M, Mo, _, _, _ = _case("tiny65x63")
    N = S["n"] + S["m"]
    A = M.to_dense()
    assert A.shape == (N, N)
    I = np.eye(N)
    assert np.array_equal(A, np.column_stack([M * I[:, j] for j in range(N)]))
    assert np.array_equal(M.to_dense(chunk=5), A)
    assert np.array_equal(A, np.column_stack([Mo @ I[:, j] for j in range(N)]))


# ---- 9. MEX gateway -----------------------------------------------------------------------------
def test_mex_pc_apply_multi(gpu_ctx):
    _gpu_mex()  # the gateway's context, made as the other gateway tests make it
    mex = Mex2()
    S, _, _, X, _, _ = _case("cvxqp1_m")
    N = S["n"] + S["m"]
    h = mex.value(mex(1, "pc_create", S["G"], S["B"], -S["C"])[0])
    mex(0, "pc_set", h, dict(nitref=3, itref_tol=TOL["cvxqp1_m"], force_itref=0))
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=_factors(S))
    Mo.set(nitref=3.0, itref_tol=TOL["cvxqp1_m"], force_itref=0.0)
    y0 = mex.value(mex(1, "pc_apply", h, X[:, 0])[0])
    assert np.array_equal(y0, Mo @ X[:, 0])
    out = mex(1, "pc_apply_multi", h, X[:, :1])[0]
    assert (mex.L.mxGetM(out), mex.L.mxGetN(out)) == (N, 1)
    assert np.array_equal(mex.value(out), y0)
    out = mex(1, "pc_apply_multi", h, X[:, :9])[0]
    assert (mex.L.mxGetM(out), mex.L.mxGetN(out)) == (N, 9)
    Y = mex.value(out).reshape(9, N).T
    for j in range(9):
        assert np.array_equal(Y[:, j], Mo @ X[:, j]), j
    _expect_error(mex, "cpk:dim", "pc_apply_multi", h, X[:-1, :2])
    _expect_error(mex, "cpk:dim", "pc_apply_multi", h, S["G"])  # sparse
    assert np.array_equal(mex.value(mex(1, "pc_apply", h, X[:, 0])[0]), y0)
    mex(0, "pc_destroy", h)
    mex.L.shim_destroy(h.a)
