"""The MEX gateway's block command end to end (through the mx stand-in, tests/mex_shim):
[X, Y, stats, flag] = cpk_mex('method_solve_multi', @cpminres, B, A, C, h, opts) returns what the
Python block call returns (kernels/cpminres.m:1, kernels/cpcg.m:1 column by column), column for
column and bit for bit, and leaves nothing behind -- also when a column stops on the reference's
error, which the command reports in stats.status instead of raising."""
import ctypes as C

import numpy as np
import pytest

import fixtures as F
import structures as ST
from test_mex_shim import Func, Mex, _expect_error, _gpu_mex

pytestmark = pytest.mark.gpu

PROPS = dict(nitref=1, force_itref=1, itref_tol=1e-8)


class BlockMex(Mex):
    """Mex whose dense 2-D arguments stay matrices (column-major, as MATLAB stores them)"""

    def arr(self, v):
        if isinstance(v, np.ndarray) and v.ndim == 2:
            a = np.asfortranarray(v, dtype=np.float64)
            self._keep_dense = a
            return self.L.shim_dense(a.shape[0], a.shape[1], a.ctypes.data_as(C.POINTER(C.c_double)))
        return super().arr(v)

    def matrix(self, a):
        L = self.L
        m, n = L.mxGetM(a), L.mxGetN(a)
        flat = np.ctypeslib.as_array(L.mxGetPr(a), shape=(m * n,)).copy() if m * n else np.zeros(0)
        return flat.reshape((m, n), order="F")


def _mex():
    _gpu_mex()  # the gateway's context, made in exact mode
    return BlockMex()


def _python_block(S, method, Bk, opts):
    import cpkrylov_amd as cpk
    with cpk.engine_options(exact_dots=1):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        M._set(**PROPS)
        return getattr(cpk, "cp" + method)(Bk, S["Q"], S["C"], M, opts, raise_on_error=False)


@pytest.mark.parametrize("method", ("minres", "cg"))
def test_mex_method_solve_multi_matches_python_block(method):
    mex = _mex()
    P = F.load("cvxqp1_m")
    n, k = P["n"], 9  # two panels, the second of one column
    opts = dict(atol=1e-6, rtol=1e-6, itmax=500)
    rng = np.random.default_rng(11)
    Bk = np.asfortranarray(rng.standard_normal((n, k)))
    Bk[:, 3] = 0.0          # stops at iteration 0
    Bk[:, 5] *= 1e-3        # another iteration count
    h = mex.value(mex(1, "pc_create", P["G"], P["B"], -P["C"])[0])
    mex(0, "pc_set", h, PROPS)
    out = mex(4, "method_solve_multi", Func("@cp" + method), Bk, P["Q"], P["C"], h, opts)
    X, Y = mex.matrix(out[0]), mex.matrix(out[1])
    niters, hlen = mex.field(out[2], "niters"), mex.field(out[2], "histLen")
    status, solved = mex.field(out[2], "status"), mex.field(out[3], "solved")
    hist = mex.matrix(mex.L.shim_field(out[2], b"residHistory"))
    Xp, Yp, sp_, fp = _python_block(P, method, Bk, opts)
    assert X.shape == Xp.shape and Y.shape == Yp.shape and hist.shape == (opts["itmax"] + 4, k)
    assert np.array_equal(X, Xp) and np.array_equal(Y, Yp)
    assert len(set(niters)) > 1 and niters[3] == 0
    for j in range(k):
        assert niters[j] == sp_[j]["niters"] and status[j] == 0 and bool(solved[j]) == fp[j]["solved"], j
        L = len(sp_[j]["residHistory"])
        assert hlen[j] == L and np.array_equal(hist[:L, j], sp_[j]["residHistory"]) and not hist[L:, j].any(), j
    # a row mismatch of B is the command's own dimension error; the handle stays good
    _expect_error(mex, "cpk:dim", "method_solve_multi", Func("@cp" + method), Bk[:-1], P["Q"], P["C"], h, opts, nlhs=4)
    # the methods without a block solve are refused by the library (nothing written, nothing left)
    _expect_error(mex, "cpk:error", "method_solve_multi", Func("@cpgmres"), Bk, P["Q"], P["C"], h, opts, nlhs=4)
    for a in out:
        mex.L.shim_destroy(a)
    mex(0, "pc_destroy", h)
    mex.L.shim_destroy(h.a)
    live = mex.live()
    assert live["mats"] == 0 and live["calloc"] == 0 and live["pcs"] == 0


def test_mex_method_solve_multi_reports_failing_columns():
    """tiny_indefinite: columns on which the reference stops with its error come back with
    stats.status = 1 (CPK_ERR_INDEFINITE), no MATLAB error, and agree with the Python block call"""
    mex = _mex()
    S = ST.tiny_indefinite()
    n = S["n"]
    opts = dict(atol=1e-6, rtol=1e-6, itmax=500)
    rng = np.random.default_rng(2)
    Bk = np.asfortranarray(np.column_stack([S["rhs"][:n], rng.standard_normal((n, 6)), np.zeros(n)]))
    Xp, Yp, sp_, fp = _python_block(S, "minres", Bk, opts)
    want = [f.get("error", 0) for f in fp]
    assert 0 < sum(1 for w in want if w) < len(want)  # failing columns beside solved ones (the oracle: 2, 3, 4)
    h = mex.value(mex(1, "pc_create", S["G"], S["B"], -S["C"])[0])
    mex(0, "pc_set", h, PROPS)
    out = mex(4, "method_solve_multi", "cpminres", Bk, S["Q"], S["C"], h, opts)
    assert list(mex.field(out[2], "status")) == want
    assert list(mex.field(out[2], "niters")) == [s["niters"] for s in sp_]
    assert np.array_equal(mex.matrix(out[0]), Xp, equal_nan=True) and np.array_equal(mex.matrix(out[1]), Yp, equal_nan=True)
    for a in out:
        mex.L.shim_destroy(a)
    mex(0, "pc_destroy", h)
    mex.L.shim_destroy(h.a)
    live = mex.live()
    assert live["mats"] == 0 and live["calloc"] == 0 and live["pcs"] == 0
