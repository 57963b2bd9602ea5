"""The MEX gateway's saddle-point operator commands end to end (through the mx stand-in,
tests/mex_shim): kkt_create, kkt_apply, kkt_residual, kkt_solve and kkt_destroy return what the
scalar reference (tests/kkt_ref.py) and the Python class give, bit for bit, and leave nothing
behind -- also on their error paths."""
import numpy as np
import pytest

import fixtures as F
import kkt_ref as R
from test_gpu_solve_multi_mex import BlockMex
from test_mex_shim import Func, _expect_error, _gpu_mex

pytestmark = pytest.mark.gpu

PROPS = dict(nitref=1, force_itref=1, itref_tol=1e-8)
OPTS = dict(atol=1e-6, rtol=1e-6, itmax=500)


def _mex():
    _gpu_mex()  # the gateway's context, made in exact mode
    return BlockMex()


@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp2_s"))
def test_mex_kkt_product_and_residual(name):
    mex = _mex()
    P, Kr = R.system(name), R.operator(name)
    N, n, k = P["n"] + P["m"], P["n"], 3
    rng = np.random.default_rng(21)
    Z = np.asfortranarray(rng.standard_normal((N, k)))
    Z[N // 2, 1] = np.nan
    Bm = np.asfortranarray(np.column_stack([P["rhs"], rng.standard_normal((N, k - 1))]))
    h = mex.value(mex(1, "kkt_create", P["A"], P["B"], P["C"])[0])
    assert mex.live()["mats"] == 3  # the handle owns its three device matrices
    out = mex(1, "kkt_apply", h, Z)
    Y = mex.matrix(out[0])
    out += mex(2, "kkt_residual", h, Z, Bm)
    Rm, sums = mex.matrix(out[1]), mex.matrix(out[2])
    assert Y.shape == (N, k) and Rm.shape == (N, k) and sums.shape == (4, k)
    for j in range(k):
        s = R.matvec(Kr, Z[:, j])
        assert R.same_bits(Y[:, j], s), j
        assert R.same_bits(Rm[:, j], Bm[:, j] - s), j
        assert R.same_bits(sums[:, j], R.sums(Bm[:, j] - s, Bm[:, j], n)), j  # the gateway's context is exact
    one = mex(1, "kkt_apply", h, Z[:, 0])  # a vector is an N x 1 matrix
    assert R.same_bits(mex.matrix(one[0])[:, 0], Y[:, 0])
    # the commands' own errors leave nothing behind and the handle stays good
    _expect_error(mex, "cpk:dim", "kkt_apply", h, Z[:-1])
    _expect_error(mex, "cpk:dim", "kkt_residual", h, Z, Bm[:, :2], nlhs=2)
    _expect_error(mex, "cpk:args", "kkt_residual", h, Z, nlhs=2)
    _expect_error(mex, "cpk:args", "kkt_apply", 1.0, Z)
    _expect_error(mex, "cpk:error", "kkt_create", P["B"], P["B"], P["C"])  # opLDL2's dimension error
    for a in out + one:
        mex.L.shim_destroy(a)
    mex(0, "kkt_destroy", h)
    mex.L.shim_destroy(h.a)
    live = mex.live()
    assert live["mats"] == 0 and live["calloc"] == 0 and live["pcs"] == 0


@pytest.mark.parametrize("method", ("minres", "cg"))
def test_mex_kkt_solve_matches_python(method):
    import cpkrylov_amd as cpk
    mex = _mex()
    P = R.system("cvxqp1_m")
    b = P["rhs"]
    k = mex.value(mex(1, "kkt_create", P["A"], P["B"], P["C"])[0])
    h = mex.value(mex(1, "pc_create", P["G"], P["B"], -P["C"])[0])
    mex(0, "pc_set", h, PROPS)
    with cpk.engine_options(exact_dots=1):
        K = cpk.KKT(P["A"], P["B"], P["C"])
        M = cpk.opLDL2(P["G"], P["B"], -P["C"])
        M._set(**PROPS)
        xp, sp_, fp = K.solve(method, b, M, OPTS)
        x0 = 0.9 * xp
        xw, sw, fw = K.solve(method, b, M, OPTS, x0=x0)
    outs = []
    for want, st, fl, extra in ((xp, sp_, fp, ()), (xw, sw, fw, (x0,))):
        out = mex(4, "kkt_solve", k, Func("@cp" + method), b, h, OPTS, *extra)
        outs += out
        assert R.same_bits(mex.value(out[0]), want)
        assert mex.field(out[1], "niters")[0] == st["niters"] and mex.field(out[2], "solved") == fl["solved"]
        assert R.same_bits(mex.field(out[1], "residHistory"), st["residHistory"])
        res = mex.value(out[3])
        tr0, tr = st["true_resid0"], st["true_resid"]
        assert R.same_bits(res, [tr0["rr_x"], tr0["rr_y"], tr0["bb_x"], tr0["bb_y"],
                                 tr["rr_x"], tr["rr_y"], tr["bb_x"], tr["bb_y"]])
    _expect_error(mex, "cpk:dim", "kkt_solve", k, Func("@cp" + method), b[:-1], h, OPTS, nlhs=4)
    _expect_error(mex, "cpk:dim", "kkt_solve", k, Func("@cp" + method), b, h, OPTS, x0[:-1], nlhs=4)
    _expect_error(mex, "cpk:args", "kkt_solve", k, Func("@cpnothing"), b, h, OPTS, nlhs=4)
    for a in outs:
        mex.L.shim_destroy(a)
    mex(0, "kkt_destroy", k)
    mex(0, "pc_destroy", h)
    mex.L.shim_destroy(k.a), mex.L.shim_destroy(h.a)
    live = mex.live()
    assert live["mats"] == 0 and live["calloc"] == 0 and live["pcs"] == 0
