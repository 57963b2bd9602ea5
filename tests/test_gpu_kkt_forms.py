"""The two forms of every K entry, host arrays and device memory, give identical bits: the outputs,
the sums, the stats and, where the driver stops, the error and what it carries.  On tiny2x1 and
tiny65x63, the smallest members with an empty and with a ragged last wave; blocks of k = 0, 1, 3, 9
columns (none, one, the loop below the crossover, a full panel plus a ragged one).  The C host forms
also run with leading dimensions N + 3, whose padding rows (NaN) must come back untouched.  Then the
error paths of the three single-column solves on the indefinite fixture, and the solver cache of M
over a sequence of K's solves.

Already asserted elsewhere and not repeated here: residual at k = 3 on tiny65x63
(test_gpu_kkt.test_device_operands), sample_block at k = 9 on tiny65x63, device tensors and padded
leading dimensions (test_gpu_kkt_block.test_sampler_operand_forms_agree), and the indefinite stop of
`solve` itself against the driver (test_gpu_kkt.test_indefinite_stop_surfaces_with_the_drivers_message).
"""
import ctypes as C

import numpy as np
import pytest

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import fixtures as F
import kkt_ref as R
import structures as S
from devbuf import DeviceArray
from test_gpu_kkt_adjoint import bits_equal

pytestmark = pytest.mark.gpu

MEMBERS = ("tiny2x1", "tiny65x63")
KS = (0, 1, 3, 9)
PAD = 3
OPTS = dict(F.EXPROG_OPTS)
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
PD = C.POINTER(C.c_double)
_KM = {}


def _dp(a):
    return a.ctypes.data_as(PD)


def _precond(P, ctx):
    import cpkrylov_amd as cpk
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=ctx)
    M._set(**{k: OPTS[k] for k in PC_PROPS})
    return M


def km(name, ctx):
    """(P, K, M) of a member, built once"""
    import cpkrylov_amd as cpk
    if name not in _KM:
        P = R.system(name)
        _KM[name] = (P, cpk.KKT(P["A"], P["B"], P["C"], ctx=ctx), _precond(P, ctx))
    return _KM[name]


def block(N, k, seed):
    """N x k: seeded standard normal columns"""
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((N, k)))


def dev(a):
    """A host vector or N x k block as a device tensor ((k, N) row-major)"""
    a = np.asarray(a, dtype=np.float64)
    return torch.from_numpy(a.copy() if a.ndim == 1 else np.ascontiguousarray(a.T)).cuda()


def host(v):
    """A result as host data: a (k, N) device tensor as the N x k block"""
    if torch is not None and isinstance(v, torch.Tensor):
        a = v.cpu().numpy()
        return a.T if a.ndim == 2 else a
    return v


def same(a, b, where="result"):
    """a and b, results of the two forms, agree: arrays bit for bit, dicts but for the wall times"""
    a, b = host(a), host(b)
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), where
        for key in a:
            if key not in ("ptime", "stime", "loop_ms"):
                same(a[key], b[key], f"{where}[{key!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert bits_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), where
    elif isinstance(a, float) and isinstance(b, float):
        assert a == b or (np.isnan(a) and np.isnan(b)), (where, a, b)
    else:
        assert a == b, (where, a, b)


def outcome(fn):
    """What a call gave: its result, or the error's code, message, partial and columns"""
    import cpkrylov_amd as cpk
    try:
        return ("ok", fn())
    except cpk.CpkError as e:
        return ("error", e.code, str(e), getattr(e, "partial", None), getattr(e, "columns", None))


def padded(Bk, fill=None):
    """The N x k block in an (N + PAD) x k array whose padding rows hold NaN"""
    N, k = Bk.shape
    A = np.full((N + PAD, max(k, 1)), np.nan, order="F")[:, :k]
    A[:N] = Bk if fill is None else fill
    return A


def padding_untouched(*blocks):
    return all(np.all(np.isnan(A[A.shape[0] - PAD:])) for A in blocks)


# ---- the residual entries ------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS[1:])  # the front end takes no host block of no columns
@pytest.mark.parametrize("entry", ("residual", "residual_exact"))
@pytest.mark.parametrize("name", MEMBERS)
def test_residual_forms(gpu_ctx, name, entry, k):
    from cpkrylov_amd import _lib
    P, K, _ = km(name, gpu_ctx)
    N = K.N
    Z, Bm = block(N, k, 10 + k), block(N, k, 20 + k)
    rh, nh = getattr(K, entry)(Z, Bm)
    if (name, entry, k) != ("tiny65x63", "residual", 3):  # test_gpu_kkt.test_device_operands
        out = dev(np.zeros((N, k)))
        rd, nd = getattr(K, entry)(dev(Z), dev(Bm), out=out)
        same((rd, nd), (rh, nh), "device form")
    Zp, Bp, Rp, nr = padded(Z), padded(Bm), padded(Z, np.nan), np.zeros(4 * max(k, 1))
    fn = getattr(_lib.lib, "cpk_kkt_" + entry)
    _lib.check(fn(K.h, k, _dp(Zp), N + PAD, _dp(Bp), N + PAD, _dp(Rp), N + PAD, _dp(nr)))
    assert bits_equal(Rp[:N], rh) and padding_untouched(Zp, Bp, Rp)
    assert bits_equal(nr[:4 * k].reshape(k, 4), np.stack([nh[q] for q in ("rr_x", "rr_y", "bb_x", "bb_y")], axis=1))


@pytest.mark.parametrize("name", MEMBERS)
def test_residual_entries_of_no_columns(gpu_ctx, name):
    """k = 0 through the six C entries themselves: CPK_OK, and R and the sums stay as they were"""
    from cpkrylov_amd import _lib
    _, K, _ = km(name, gpu_ctx)
    N = K.N
    for exact in ("", "_exact"):
        Z, Bm, Rm, nr = np.ones(N), np.ones(N), np.full(N, np.nan), np.full(4, np.nan)
        fn = getattr(_lib.lib, f"cpk_kkt_residual{exact}")
        assert fn(K.h, 0, _dp(Z), N, _dp(Bm), N, _dp(Rm), N, _dp(nr)) == _lib.CPK_OK
        assert np.all(np.isnan(Rm)) and np.all(np.isnan(nr)) and np.all(Z == 1.0) and np.all(Bm == 1.0)
        dZ, dB, dR, dn = DeviceArray.of(Z), DeviceArray.of(Bm), DeviceArray.of(Rm), DeviceArray.of(nr)
        fn = getattr(_lib.lib, f"cpk_kkt_residual{exact}_device")
        assert fn(K.h, 0, dZ.p, N, dB.p, N, dR.p, N, dn.p) == _lib.CPK_OK
        fn = getattr(_lib.lib, f"cpk_kkt_residual{exact}_device_sums")
        assert fn(K.h, 0, dZ.p, N, dB.p, N, dR.p, N, _dp(nr)) == _lib.CPK_OK
        assert np.all(np.isnan(dR.numpy())) and np.all(np.isnan(dn.numpy())) and np.all(np.isnan(nr))
        assert np.all(dZ.numpy() == 1.0) and np.all(dB.numpy() == 1.0)


# ---- the three single-column solves --------------------------------------------------------------
@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("name", MEMBERS)
def test_solve_forms(gpu_ctx, name, warm):
    P, K, M = km(name, gpu_ctx)
    b, x0 = P["rhs"], (block(K.N, 1, 31)[:, 0] if warm else None)
    oh = outcome(lambda: K.solve("minres", b, M, OPTS, x0=x0))
    xd = dev(x0 if warm else np.full(K.N, np.nan))
    od = outcome(lambda: K.solve("minres", dev(b), M, OPTS, x0=xd if warm else None, out=xd))
    same(od, oh)


@pytest.mark.parametrize("max_steps", (0, 2))
@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("name", MEMBERS)
def test_solve_refined_forms(gpu_ctx, name, warm, max_steps):
    P, K, M = km(name, gpu_ctx)
    b, x0 = P["rhs"], (block(K.N, 1, 32)[:, 0] if warm else None)
    oh = outcome(lambda: K.solve_refined("minres", b, M, OPTS, x0=x0, max_steps=max_steps))
    xd = dev(x0 if warm else np.full(K.N, np.nan))
    od = outcome(lambda: K.solve_refined("minres", dev(b), M, OPTS, x0=xd if warm else None, max_steps=max_steps, out=xd))
    same(od, oh)


@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("name", MEMBERS)
def test_adjoint_forms(gpu_ctx, name, warm):
    P, K, M = km(name, gpu_ctx)
    x, gx, lam0 = block(K.N, 1, 33)[:, 0], P["rhs"], (block(K.N, 1, 34)[:, 0] if warm else None)
    oh = outcome(lambda: K.adjoint("minres", x, gx, M, OPTS, lam0=lam0))
    out = {"db": dev(lam0 if warm else np.full(K.N, np.nan))}
    out.update({key: dev(np.full(h.info()["entries"], np.nan)) for key, h in (("dA", K.A), ("dB", K.B), ("dC", K.C))})
    od = outcome(lambda: K.adjoint("minres", dev(x), dev(gx), M, OPTS, lam0=out["db"] if warm else None, out=out))
    same(od, oh)


# ---- the block entries ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("name", MEMBERS)
def test_solve_block_forms(gpu_ctx, name, warm, k):
    from cpkrylov_amd import _lib, api
    P, K, M = km(name, gpu_ctx)
    N = K.N
    Bk, X0 = block(N, k, 40 + k) * P["rhs"][:, None], (block(N, k, 50 + k) if warm else None)
    oh = outcome(lambda: K.solve_block("minres", Bk, M, OPTS, X0=X0))
    if k:
        Xd = dev(X0 if warm else np.full((N, k), np.nan))
        od = outcome(lambda: K.solve_block("minres", dev(Bk), M, OPTS, X0=Xd if warm else None, out=Xd))
        same(od, oh)
    else:  # a tensor of no elements has no address and the entry refuses NULL: the C device form itself
        dB, dX = DeviceArray(N), DeviceArray.of(np.full(N, np.nan))
        assert oh[0] == "ok" and _lib.lib.cpk_kkt_solve_multi_device(
            K.h, _lib.METHODS["minres"], 0, dB.p, N, M.h, C.byref(_lib.make_opts(OPTS)), dX.p, N, int(warm), None, None,
            None) == _lib.CPK_OK
        assert np.all(np.isnan(dX.numpy()))
    # the C host form with padded leading dimensions: X, the sums and the column statuses
    Bp, Xp, res = padded(Bk), padded(Bk, X0 if warm else np.nan), np.zeros(8 * max(k, 1))
    sts, stats, flags, _ = api._block_call("minres", k, OPTS, K.n, K.m, lambda st, status: _lib.lib.cpk_kkt_solve_multi(
        K.h, _lib.METHODS["minres"], k, _dp(Bp), N + PAD, M.h, C.byref(_lib.make_opts(OPTS)), _dp(Xp), N + PAD, int(warm),
        st, status, _dp(res)), False)
    K._block_stats(sts, stats, res, k)
    Xh, sh, fh = oh[1] if oh[0] == "ok" else oh[3]
    assert bits_equal(Xp[:N], Xh) and padding_untouched(Bp, Xp)
    same((stats, flags), (sh, fh), "padded form")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", MEMBERS)
def test_sample_block_forms(gpu_ctx, name, k):
    from cpkrylov_amd import _lib
    P, K, _ = km(name, gpu_ctx)
    N = K.N
    X, L = block(N, k, 60 + k), block(N, k, 70 + k)
    gh = K.sample_block(X, L)
    if (name, k) == ("tiny65x63", 9):  # test_gpu_kkt_block.test_sampler_operand_forms_agree
        return
    counts = [h.info()["entries"] for h in (K.A, K.B, K.C)]
    out = {key: dev(np.full(c, np.nan)) for key, c in zip(("dA", "dB", "dC"), counts)}
    same(K.sample_block(dev(X), dev(L), out=out), gh, "device form")
    Xp, Lp, g = padded(X), padded(L), [np.full(max(c, 1), np.nan)[:c] for c in counts]
    args = [v for a, c in zip(g, counts) for v in (_dp(a) if c else None, c)]
    _lib.check(_lib.lib.cpk_kkt_sample_multi(K.h, k, _dp(Xp), N + PAD, _dp(Lp), N + PAD, *args))
    same(dict(zip(("dA", "dB", "dC"), g)), gh, "padded form")
    assert padding_untouched(Xp, Lp)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("name", MEMBERS)
def test_adjoint_block_forms(gpu_ctx, name, warm, k):
    from cpkrylov_amd import _lib, api
    P, K, M = km(name, gpu_ctx)
    N = K.N
    X, GX, L0 = block(N, k, 80 + k), block(N, k, 90 + k) * P["rhs"][:, None], (block(N, k, 100 + k) if warm else None)
    oh = outcome(lambda: K.adjoint_block("minres", X, GX, M, OPTS, Lam0=L0))
    counts = [h.info()["entries"] for h in (K.A, K.B, K.C)]
    out = {key: dev(np.full(c, np.nan)) for key, c in zip(("dA", "dB", "dC"), counts)}
    if k:
        out["db"] = dev(L0 if warm else np.full((N, k), np.nan))
        od = outcome(lambda: K.adjoint_block("minres", dev(X), dev(GX), M, OPTS, Lam0=out["db"] if warm else None, out=out))
        same(od, oh)
    else:  # no columns: the C device form itself, as in test_solve_block_forms
        dX, dG, dL = DeviceArray(N), DeviceArray(N), DeviceArray.of(np.full(N, np.nan))
        dg = [DeviceArray.of(np.full(c, np.nan)) for c in counts]
        assert oh[0] == "ok" and _lib.lib.cpk_kkt_adjoint_multi_device(
            K.h, _lib.METHODS["minres"], 0, dX.p, N, dG.p, N, M.h, C.byref(_lib.make_opts(OPTS)), dL.p, N, int(warm),
            dg[0].p, counts[0], dg[1].p, counts[1], dg[2].p, counts[2], None, None, None) == _lib.CPK_OK
        same({key: d.numpy() for key, d in zip(("dA", "dB", "dC"), dg)}, {key: oh[1][key] for key in ("dA", "dB", "dC")})
        assert np.all(np.isnan(dL.numpy()))
    # the C host form with padded leading dimensions
    Xp, Gp, Lp, res = padded(X), padded(GX), padded(X, L0 if warm else np.nan), np.zeros(8 * max(k, 1))
    g = [np.full(max(c, 1), np.nan)[:c] for c in counts]
    args = [v for a, c in zip(g, counts) for v in (_dp(a) if c else None, c)]
    sts, stats, flags, _ = api._block_call("minres", k, OPTS, K.n, K.m, lambda st, status: _lib.lib.cpk_kkt_adjoint_multi(
        K.h, _lib.METHODS["minres"], k, _dp(Xp), N + PAD, _dp(Gp), N + PAD, M.h, C.byref(_lib.make_opts(OPTS)), _dp(Lp),
        N + PAD, int(warm), *args, st, status, _dp(res)), False)
    K._block_stats(sts, stats, res, k)
    assert padding_untouched(Xp, Gp, Lp)
    if oh[0] == "ok":
        same(dict(db=Lp[:N], dA=g[0], dB=g[1], dC=g[2], stats=stats, flags=flags), oh[1], "padded form")
    else:  # a column's driver stopped: Lam and the stats as far as they went, the gradients untouched
        same((Lp[:N], stats, flags), oh[3], "padded form")
        assert all(np.all(np.isnan(a)) for a in g)


# ---- the error paths of the three single-column solves -------------------------------------------
def test_indefinite_stop_of_every_single_column_solve(gpu_ctx):
    """structures.tiny_indefinite under exact_dots (test_gpu_kkt's fixture): solve_refined and adjoint
    raise solve's code and message; partial[0] is finite and is, bit for bit, what the device form
    leaves in out; adjoint leaves NaN-filled dA, dB, dC untouched"""
    import cpkrylov_amd as cpk
    P = S.tiny_indefinite()
    b = P["rhs"]
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        K = cpk.KKT(P["Q"], P["B"], P["C"], ctx=gpu_ctx)
        M = _precond(P, gpu_ctx)
        with pytest.raises(cpk.IndefiniteError) as es:
            K.solve("minres", b, M, OPTS)
        counts = [h.info()["entries"] for h in (K.A, K.B, K.C)]
        new = lambda: {key: np.full(c, np.nan) for key, c in zip(("dA", "dB", "dC"), counts)}  # noqa: E731
        gh, gd = new(), {key: dev(v) for key, v in new().items()}
        calls = {
            "solve": lambda **kw: K.solve("minres", kw.get("b", b), M, OPTS, out=kw.get("out")),
            "solve_refined": lambda **kw: K.solve_refined("minres", kw.get("b", b), M, OPTS, max_steps=2, out=kw.get("out")),
            "adjoint": lambda **kw: K.adjoint("minres", kw.get("x", np.ones(K.N)), kw.get("b", b), M, OPTS,
                                              out=dict(gd, db=kw["out"]) if "out" in kw else gh),
        }
        for entry, call in calls.items():
            with pytest.raises(cpk.IndefiniteError) as eh:
                call()
            assert eh.value.code == es.value.code and str(eh.value) == str(es.value), entry
            xh = eh.value.partial[0]
            assert np.all(np.isfinite(xh)), entry
            out = dev(np.full(K.N, np.nan))
            with pytest.raises(cpk.IndefiniteError) as ed:
                call(b=dev(b), x=dev(np.ones(K.N)), out=out)
            assert ed.value.code == es.value.code and str(ed.value) == str(es.value), entry
            assert ed.value.partial[0] is out and bits_equal(host(out), xh), entry
            same(ed.value.partial[1], eh.value.partial[1], entry)
    assert all(np.all(np.isnan(v)) for v in gh.values()) and all(np.all(np.isnan(host(v))) for v in gd.values())


# ---- the solver cache ----------------------------------------------------------------------------
def cached_solvers_of_the_sequence(name, ctx):
    """The solvers M caches over two cold K.solve, one K.solve_refined and one more K.solve on fresh K
    and M, after each call; b and x are device tensors that stay, so the only addresses that can move
    are K's own"""
    import cpkrylov_amd as cpk
    P = R.system(name)
    K, M = cpk.KKT(P["A"], P["B"], P["C"], ctx=ctx), _precond(P, ctx)
    b, x = dev(P["rhs"]), dev(np.zeros(K.N))
    counts = [M.solver_info()["solvers"]]
    for entry, kw in ((K.solve, {}), (K.solve, {}), (K.solve_refined, {"max_steps": 2}), (K.solve, {})):
        outcome(lambda: entry("minres", b, M, OPTS, out=x, **kw))
        counts.append(M.solver_info()["solvers"])
    return counts


def test_the_solves_find_the_cached_solver_again():
    """K's vectors keep their addresses from call to call, except where the refined solve's third part
    makes them grow, so M's cached solver is found again exactly as before the drivers moved to
    kkt_driver.cpp: the counts are those measured on that commit's parent, 01dc9a0.

    The sequence runs in a process of its own, as the parent's was measured.  When the refined solve
    makes K's vectors grow, whether the larger allocation comes back at the address of the one it
    replaces -- so that the solver's key, which holds those addresses, does not move -- is up to the
    device allocator and to what the process freed before: in a fresh process it does ([0, 1, 1, 1, 1]),
    after this module's other tests it may not ([0, 1, 1, 2, 2], as legitimate on the parent).  So do
    not read more into the counts than this: a preamble that sized the vectors wrongly could give the
    same ones; what they do catch is a solve that hands the method other vectors than K's own."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_gpu_kkt_forms as T, cpkrylov_amd as cpk; "
            "print(json.dumps({n: T.cached_solvers_of_the_sequence(n, cpk.default_context()) for n in T.MEMBERS}))"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == PARENT_COUNTS


PARENT_COUNTS = {"tiny2x1": [0, 1, 1, 1, 1], "tiny65x63": [0, 1, 1, 1, 1]}  # measured on 01dc9a0
