"""The bare factor operator M' = conj(M) = P*L'^-1*D^-1*L^-1*P' (ops/opLDL2.m:127-136) on the GPU:
single column (cpk_pc_apply_ldl, the tuned sweeps) and a block of right-hand sides
(cpk_pc_apply_ldl_multi, the panel sweep of multisweep.hip).

Reference: the oracle's LDL2 on the product's exported factors with nitref = 0 -- the bare
composite on the same factors -- applied column by column and compared with np.array_equal.
Systems: every member of the structure family (tests/structures.py) and the cvxqp1_m fixture.
Columns: standard normal (seed 7), one all-zero column, the hub unit vector."""
import ctypes as C

import numpy as np
import pytest

import fixtures as F
import structures as ST
from devbuf import DeviceArray
from oracle import oracle as O
from test_gpu_dist import _run_ranks
from test_mex_shim import Mex, _expect_error, _factors, _gpu_mex

pytestmark = pytest.mark.gpu

NAMES = list(ST.MEMBERS) + ["cvxqp1_m"]
KS = [1, 2, 7, 8, 9, 17]  # below, at and just above one panel of 8; two panels plus one
KMAX = max(KS)
_CACHE = {}


def _system(name):
    return F.load(name) if name == "cvxqp1_m" else ST.get(name)


def _columns(S):
    """N x 17: standard normal (seed 7) with column 1 all zero and column 2 the hub's unit vector,
    so every k >= 3 holds all three kinds, k = 2 the first two and k = 1 the normal column"""
    N = S["n"] + S["m"]
    X = np.random.default_rng(7).standard_normal((N, KMAX))
    X[:, 1] = 0.0
    X[:, 2] = 0.0
    X[ST.hub(S), 2] = 1.0
    return X


def _case(name):
    """(system, operator, oracle operator, X, oracle's Y), built once per member; read-only"""
    if name not in _CACHE:
        import cpkrylov_amd as cpk
        S = _system(name)
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
        Mo.set(nitref=0.0)
        X = _columns(S)
        Yo = np.column_stack([Mo @ X[:, j] for j in range(KMAX)])
        X.setflags(write=False), Yo.setflags(write=False)
        _CACHE[name] = (S, M, Mo, X, Yo)
    return _CACHE[name]


def _multi_device(M, X, ldx, ldy, sentinel=-7.25):
    """cpk_pc_apply_ldl_multi_device on padded column-major buffers; returns (rc, Y as ldy x k)"""
    from cpkrylov_amd import _lib
    N, k = X.shape
    Xp = np.full((k, ldx), np.nan)  # row j of this C array = column j with leading dimension ldx
    Xp[:, :N] = X.T
    dX, dY = DeviceArray.of(Xp), DeviceArray.of(np.full((k, ldy), sentinel))
    rc = _lib.lib.cpk_pc_apply_ldl_multi_device(M.h, k, dX.p, ldx, dY.p, ldy)
    return rc, dY.numpy().reshape(k, ldy).T


# ---- 1. single column ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_single_column(gpu_ctx, name):
    from cpkrylov_amd import _lib
    S, M, Mo, X, Yo = _case(name)
    N = S["n"] + S["m"]
    assert M.T is M and M.transpose() is M
    H = M.H
    assert H.H is H and H.T is H and H.conj() is H and H.ctranspose() is H
    assert H.shape == (N, N) and H.n == N
    saved = (M.nitref, M.itref_tol, M.force_itref, M.residual_update)
    assert saved[0] == 3  # the default: the refined operator M would run its loop
    for props in (dict(), dict(force_itref=True, residual_update=True)):
        for k, v in props.items():
            setattr(M, k, v)
        for j in range(3):
            z = X[:, j]
            assert np.array_equal(M.H * z, Yo[:, j]), (props, j)
            assert np.array_equal(M.conj() * z, Yo[:, j]), (props, j)
            assert np.array_equal(M.ctranspose() @ z, Yo[:, j]), (props, j)
            dx, dy = DeviceArray.of(z), DeviceArray(N)
            assert _lib.lib.cpk_pc_apply_ldl_device(M.h, dx.p, dy.p) == 0
            assert np.array_equal(dy.numpy(), Yo[:, j]), (props, j)
    M.force_itref, M.residual_update = saved[2], saved[3]
    with pytest.raises(_lib.CpkError) as e:
        M.H * np.ones(N + 1)
    assert e.value.code == _lib.CPK_ERR_DIM


def test_factor_operator_is_not_the_refined_operator(gpu_ctx):
    """on cvxqp1_m three forced refinement steps change M*z: the test tells M' from M"""
    S, M, Mo, X, Yo = _case("cvxqp1_m")
    M.force_itref = True
    try:
        assert M.nitref == 3
        y = M * X[:, 0]
    finally:
        M.force_itref = False
    assert not np.array_equal(y, Yo[:, 0])
    assert np.array_equal(M.H * X[:, 0], Yo[:, 0])


# ---- 2. multi column ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_multi_column(gpu_ctx, name):
    from cpkrylov_amd import _lib
    S, M, Mo, X, Yo = _case(name)
    N = S["n"] + S["m"]
    for k in KS:
        for order in ("C", "F"):
            Y = M.H @ np.array(X[:, :k], order=order)
            assert Y.shape == (N, k)
            for j in range(k):
                assert np.array_equal(Y[:, j], Yo[:, j]), (k, order, j, np.max(np.abs(Y[:, j] - Yo[:, j])))
        rc, Yd = _multi_device(M, X[:, :k], N + 3, N + 5)
        assert rc == 0
        assert np.array_equal(Yd[:N], Yo[:, :k]), k
        assert np.all(Yd[N:] == -7.25), k  # the padding rows of Y are untouched
    # k = 0 does nothing; a leading dimension below N is refused
    rc, Yd = _multi_device(M, X[:, :0], N, N)
    assert rc == 0
    assert (M.H @ np.zeros((N, 0))).shape == (N, 0)
    dX, dY = DeviceArray.of(X[:, :2].T), DeviceArray(2 * N)
    if N > 1:
        assert _lib.lib.cpk_pc_apply_ldl_multi_device(M.h, 2, dX.p, N - 1, dY.p, N) == _lib.CPK_ERR_DIM
        assert _lib.lib.cpk_pc_apply_ldl_multi_device(M.h, 2, dX.p, N, dY.p, N - 1) == _lib.CPK_ERR_DIM
    assert _lib.lib.cpk_pc_apply_ldl_multi_device(M.h, -1, dX.p, N, dY.p, N) == _lib.CPK_ERR_DIM
    Xh, Yh = np.asfortranarray(X[:, :2]), np.empty((N, 2), order="F")
    P = C.POINTER(C.c_double)
    assert _lib.lib.cpk_pc_apply_ldl_multi(M.h, 2, Xh.ctypes.data_as(P), N - 1, Yh.ctypes.data_as(P), N) == _lib.CPK_ERR_DIM
    with pytest.raises(_lib.CpkError) as e:
        M.H @ np.ones((N + 1, 2))
    assert e.value.code == _lib.CPK_ERR_DIM


# ---- 3. the paths taken -------------------------------------------------------------------------
def test_paths_taken(gpu_ctx):
    info = _case("arrow_row")[1].multi_info()
    assert info["kp"] == 8 and info["direct_blocks"] >= 1 and info["staged_blocks"] >= 1, info
    M = _case("dense_col")[1]
    info = M.multi_info()
    assert info["staged_blocks"] >= 1 and info["launches"] == 2 * M.sweep_info()["rounds"], info
    assert info["staged_blocks"] + info["direct_blocks"] == M.info["nblocks"], info
    for name in ("tiny1x1", "tiny2x1", "tiny3x2"):
        info = _case(name)[1].multi_info()
        assert info == dict(kp=8, launches=2, staged_blocks=1, direct_blocks=0), (name, info)


@pytest.mark.parametrize("options", [dict(sweep="64,128,64"), dict(no_chain=1), dict(chain_wide=2 ** 24)],
                         ids=["sweep=64,128,64", "no_chain", "chain_wide"])
def test_multi_column_engine_options(gpu_ctx, options):
    """the multi sweep reads the schedule these options built: still bit-equal to the oracle"""
    import cpkrylov_amd as cpk
    S, _, _, X, _ = _case("dense_col")
    with cpk.engine_options(**options):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
    Mo.set(nitref=0.0)
    info = M.multi_info()
    assert info["launches"] == 2 * M.sweep_info()["rounds"]
    if "sweep" in options:  # the clique's rows of up to 314 entries are above a cap of 128
        assert info["direct_blocks"] >= 1, info
    Y = M.H @ X[:, :9]
    for j in range(9):
        assert np.array_equal(Y[:, j], Mo @ X[:, j]), (options, j)
        if j < 3:
            assert np.array_equal(M.H * X[:, j], Y[:, j]), (options, j)


# ---- 4. no state leak ---------------------------------------------------------------------------
def test_factor_apply_leaves_the_handle_state_alone(gpu_ctx):
    import cpkrylov_amd as cpk
    S, _, _, X, Yo = _case("cvxqp1_m")
    M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    props = dict(nitref=1, itref_tol=1e-9, force_itref=True, residual_update=True)
    for k, v in props.items():
        setattr(M, k, v)
    M.handle_semantics = True
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
    Mo.set(**{k: float(v) for k, v in props.items()})
    Mo.set_handle(True)
    z1, z2 = X[:, 0], X[:, 3]
    yo1, yo2 = Mo @ z1, Mo @ z2
    y1 = M * z1
    Y = M.H @ X[:, :9]
    yh = M.H * X[:, 4]
    y2 = M * z2
    assert np.array_equal(y1, yo1) and np.array_equal(y2, yo2)
    assert not np.array_equal(yo2, Mo @ z2)  # the oracle's state does move: the check above can fail
    assert np.array_equal(Y, Yo[:, :9]) and np.array_equal(yh, Yo[:, 4])
    assert (M.nitref, M.itref_tol, M.force_itref, M.residual_update) == (1.0, 1e-9, True, 1.0)


# ---- 5. to_dense --------------------------------------------------------------------------------
def test_to_dense(gpu_ctx):
    S, M, Mo, _, _ = _case("tiny65x63")
    N = S["n"] + S["m"]
    A = M.H.to_dense()
    assert A.shape == (N, N)
    I = np.eye(N)
    Ao = np.column_stack([Mo @ I[:, j] for j in range(N)])
    assert np.array_equal(A, Ao)
    assert np.array_equal(M.H.to_dense(chunk=5), Ao)
    # a sanity bound on an exactly symmetric operator computed in two triangular passes
    assert np.max(np.abs(A - A.T)) <= 1e-10 * np.max(np.abs(A))


# ---- 6. distributed -----------------------------------------------------------------------------
def test_distributed(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S, _, _, X, _ = _case("dense_col")
    N = S["n"] + S["m"]
    P = C.POINTER(C.c_double)

    def work(ctx, r):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        ys = [M.H * X[:, j] for j in range(3)]
        Xh, Yh = np.asfortranarray(X[:, :2]), np.empty((N, 2), order="F")
        rc = _lib.lib.cpk_pc_apply_ldl_multi(M.h, 2, Xh.ctypes.data_as(P), N, Yh.ctypes.data_as(P), N)
        return ys, rc, M.export_factors() if r == 0 else None

    res = _run_ranks(2, work)
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=res[0][2])
    Mo.set(nitref=0.0)
    for ys, rc, _ in res:
        assert rc == _lib.CPK_ERR_UNSUPPORTED
        for j in range(3):
            assert np.array_equal(ys[j], Mo @ X[:, j]), j


# ---- 7. MEX gateway -----------------------------------------------------------------------------
class Mex2(Mex):
    """Mex whose dense 2-D arrays stay matrices (MATLAB's column-major N x k)"""

    def arr(self, v):
        if isinstance(v, np.ndarray) and v.ndim == 2:
            a = np.asfortranarray(v, dtype=np.float64)
            return self.L.shim_dense(a.shape[0], a.shape[1], a.ctypes.data_as(C.POINTER(C.c_double)))
        return super().arr(v)


def test_mex_pc_apply_ldl(gpu_ctx):
    _gpu_mex()  # the gateway's context, made as the other gateway tests make it
    mex = Mex2()
    S, _, _, X, _ = _case("cvxqp1_m")
    N = S["n"] + S["m"]
    h = mex.value(mex(1, "pc_create", S["G"], S["B"], -S["C"])[0])
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=_factors(S))
    Mo.set(nitref=0.0)
    y0 = mex.value(mex(1, "pc_apply", h, X[:, 0])[0])
    out = mex(1, "pc_apply_ldl", h, X[:, :1])[0]
    assert (mex.L.mxGetM(out), mex.L.mxGetN(out)) == (N, 1)
    assert np.array_equal(mex.value(out), Mo @ X[:, 0])
    out = mex(1, "pc_apply_ldl", h, X[:, :9])[0]
    assert (mex.L.mxGetM(out), mex.L.mxGetN(out)) == (N, 9)
    Y = mex.value(out).reshape(9, N).T
    for j in range(9):
        assert np.array_equal(Y[:, j], Mo @ X[:, j]), j
    _expect_error(mex, "cpk:dim", "pc_apply_ldl", h, X[:-1, :2])
    _expect_error(mex, "cpk:dim", "pc_apply_ldl", h, S["G"])  # sparse
    assert np.array_equal(mex.value(mex(1, "pc_apply", h, X[:, 0])[0]), y0)
    mex(0, "pc_destroy", h)
    mex.L.shim_destroy(h.a)
