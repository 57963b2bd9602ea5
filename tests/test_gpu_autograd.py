"""cpk.autograd.kkt_solve: the verified solve as a torch.autograd.Function on device tensors.  The
gradients loss.backward() leaves are K.adjoint's arrays bit for bit and agree with torch's own
dense autograd within the bound derived in tests/test_gpu_kkt_adjoint.py; a System's handles are
reused from call to call; tensors of the wrong kind are refused."""
import numpy as np
import pytest
import scipy.sparse as sp

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import fixtures as F
import structures as ST

pytestmark = pytest.mark.gpu

SAFETY = 10.0
EPS = 2.0 ** -52
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
OPTS = dict(F.EXPROG_OPTS)
METHOD = "minres"
# seed of the loss's w: the first at which the adjoint solve of a standard normal w runs through on
# these members (tests/test_gpu_kkt_adjoint.py, SYSTEMS)
W_SEED = {"tiny3x2": 0, "tiny65x63": 1}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)))


def canon(M):
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return M


def blocks(name):
    P = F.load(name) if name.startswith("cvxqp") else ST.get(name)
    return {k: canon(P[k]) for k in ("Q", "B", "C", "G")}, np.array(P["rhs"]), P["n"], P["m"]


def leaves(vals):
    assert torch is not None and torch.cuda.is_available()
    return [torch.from_numpy(np.array(v)).cuda().requires_grad_(True) for v in vals]


def run(S, vals, w, method=METHOD, opts=OPTS):
    """forward and backward of loss = w . x on fresh leaf tensors: (x, leaves)"""
    import cpkrylov_amd as cpk
    ts = leaves(vals)
    x = cpk.autograd.kkt_solve(S.K, S.M, method, *ts, opts=opts)
    (torch.from_numpy(w).cuda() * x).sum().backward()
    return x, ts


@pytest.mark.parametrize("name", ("tiny3x2", "tiny65x63"))
def test_gradients_are_the_adjoints_and_match_dense_autograd(gpu_ctx, name):
    import cpkrylov_amd as cpk
    Bk, rhs, n, m = blocks(name)
    N = n + m
    w = np.random.default_rng(W_SEED[name]).standard_normal(N)
    vals = (Bk["Q"].data, Bk["B"].data, Bk["C"].data, Bk["G"].data, rhs)
    S = cpk.autograd.System(Bk["Q"], Bk["B"], Bk["C"], Bk["G"], ctx=gpu_ctx)
    x, (ta, tb, tc, tg, tr) = run(S, vals, w)
    assert tg.grad is None
    # K.adjoint on handles of their own
    K = cpk.KKT(Bk["Q"], Bk["B"], Bk["C"], ctx=gpu_ctx)
    M = cpk.opLDL2(Bk["G"], Bk["B"], -Bk["C"], ctx=gpu_ctx)
    M._set(**{k: OPTS[k] for k in PC_PROPS if k in OPTS})
    xh, sx, _ = K.solve(METHOD, rhs, M, OPTS)
    assert bits_equal(x.detach().cpu().numpy(), xh)
    r = K.adjoint(METHOD, xh, w, M, OPTS)
    for t, key in ((ta, "dA"), (tb, "dB"), (tc, "dC"), (tr, "db")):
        assert bits_equal(t.grad.cpu().numpy(), r[key]), key
    # torch's own dense autograd on the same leaves' values
    da, db_, dc, _, dr = leaves(vals)
    Kd = torch.zeros((N, N), dtype=torch.float64, device="cuda")

    def idx(Mx, r0, c0):
        rows = np.repeat(np.arange(Mx.shape[0]), np.diff(Mx.indptr))
        return torch.from_numpy(rows + r0).cuda(), torch.from_numpy(Mx.indices.astype(np.int64) + c0).cuda()

    (ia, ja), (ib, jb), (ic, jc) = idx(Bk["Q"], 0, 0), idx(Bk["B"], n, 0), idx(Bk["C"], n, n)
    Kd = Kd.index_put((ia, ja), da).index_put((ib, jb), db_).index_put((jb, ib), db_).index_put((ic, jc), -dc)
    x_ref = torch.linalg.solve(Kd, dr)
    (torch.from_numpy(w).cuda() * x_ref).sum().backward()
    x_ref = x_ref.detach().cpu().numpy()
    lam_ref = dr.grad.cpu().numpy()
    e_x = np.linalg.norm(xh - x_ref) / np.linalg.norm(x_ref)
    e_l = np.linalg.norm(r["db"] - lam_ref) / np.linalg.norm(lam_ref)
    fwd = sx["true_resid"]["rnorm"] / sx["true_resid"]["bnorm"]
    adj = r["stats"]["true_resid"]["rnorm"] / r["stats"]["true_resid"]["bnorm"]
    print(f"{name}: e_x {e_x:.3e} e_lam {e_l:.3e} true relative residual forward {fwd:.3e} adjoint {adj:.3e}")
    assert adj <= SAFETY * fwd, (adj, fwd)
    scale = (e_x + e_l + e_x * e_l) * np.linalg.norm(lam_ref) * np.linalg.norm(x_ref)
    for t, ref, c, key in ((ta, da, 1.0, "A"), (tb, db_, 2.0, "B"), (tc, dc, 1.0, "C")):
        g, g_ref = t.grad.cpu().numpy(), ref.grad.cpu().numpy()
        err, bound = np.linalg.norm(g - g_ref), scale * c + 4.0 * EPS * np.sum(np.abs(g_ref))
        print(f"{name}: d{key} error {err:.3e} bound {bound:.3e} (|g_ref| {np.linalg.norm(g_ref):.3e})")
        assert err <= bound, (key, err, bound)


def test_handles_are_reused(gpu_ctx):
    """Two forwards with different values on one System: every handle's values generation rises by
    one per forward, M holds no solver beyond the first call's, and the second result and
    gradients equal a fresh System's on the second values bit for bit"""
    import cpkrylov_amd as cpk
    Bk, rhs, n, m = blocks("cvxqp2_s")  # 725 dofs: real iterations, no stop on a residual that is pure rounding
    w = np.random.default_rng(5).standard_normal(n + m)
    rng = np.random.default_rng(21)
    v1 = (Bk["Q"].data, Bk["B"].data, Bk["C"].data, Bk["G"].data, rhs)
    # the fixture's (1,1) block is nonsymmetric: the System keeps A' and KT, and the method is cpgmres
    assert abs(Bk["Q"] - Bk["Q"].T).max() > 0
    method, opts = "gmres", dict(OPTS, restart=20)
    q2 = Bk["Q"].copy()
    q2.data = q2.data * rng.uniform(0.9, 1.1, q2.nnz)
    v2 = (q2.data, Bk["B"].data * rng.uniform(0.9, 1.1, Bk["B"].nnz), Bk["C"].data * 2.0, q2.diagonal(), rhs * 0.5)
    S = cpk.autograd.System(Bk["Q"], Bk["B"], Bk["C"], Bk["G"], ctx=gpu_ctx, symmetric=False)
    hs = S.handles()
    g0 = [h.info()["values_generation"] for h in hs]
    run(S, v1, w, method, opts)
    g1 = [h.info()["values_generation"] for h in hs]
    info1 = S.M.solver_info()
    ids = [id(o) for o in hs + (S.K, S.M)]
    x2, t2 = run(S, v2, w, method, opts)
    g2 = [h.info()["values_generation"] for h in hs]
    assert [b - a for a, b in zip(g0, g1)] == [1] * 5 and [b - a for a, b in zip(g1, g2)] == [1] * 5
    assert S.AT.info()["values_generation"] == 2 and S.KT is not None
    assert S.M.solver_info() == info1 and ids == [id(o) for o in S.handles() + (S.K, S.M)]
    fresh = cpk.autograd.System(Bk["Q"], Bk["B"], Bk["C"], Bk["G"], ctx=gpu_ctx, symmetric=False)
    xf, tf = run(fresh, v2, w, method, opts)
    assert bits_equal(x2.detach().cpu().numpy(), xf.detach().cpu().numpy())
    for a, b, key in zip(t2, tf, ("a", "b", "c", "g", "rhs")):
        if key == "g":
            assert a.grad is None and b.grad is None
        else:
            assert bits_equal(a.grad.cpu().numpy(), b.grad.cpu().numpy()), key
    # the warm-started backward: lambda of the first values starts the second values' adjoint solve,
    # whose stop test then runs on the correction system -- the forward is untouched, and the adjoint
    # solve's true residual is held to the cold one's
    S.warm_adjoint = True
    run(S, v1, w, method, opts)
    x3, t3 = run(S, v2, w, method, opts)
    assert bits_equal(x3.detach().cpu().numpy(), xf.detach().cpu().numpy())
    warm, cold = (s.last_backward[0]["true_resid"] for s in (S, fresh))
    print(f"adjoint solve, true relative residual: warm {warm['rnorm'] / warm['bnorm']:.3e} cold {cold['rnorm'] / cold['bnorm']:.3e}")
    assert warm["rnorm"] / warm["bnorm"] <= SAFETY * cold["rnorm"] / cold["bnorm"]
    assert warm == S.KT.residual(t3[4].grad.cpu().numpy(), w)[1]


def test_wrong_tensors_are_refused(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    Bk, rhs, n, m = blocks("tiny3x2")
    S = cpk.autograd.System(Bk["Q"], Bk["B"], Bk["C"], Bk["G"], ctx=gpu_ctx)
    good = leaves((Bk["Q"].data, Bk["B"].data, Bk["C"].data, Bk["G"].data, rhs))
    gens = [h.info()["values_generation"] for h in S.handles()]
    bad = [lambda t: t.float(), lambda t: torch.stack([t, t], dim=1)[:, 0], lambda t: t.detach().cpu()]
    for pos in (0, 4):
        for make in bad:
            args = list(good)
            args[pos] = make(good[pos])
            with pytest.raises(cpk.CpkError) as e:
                cpk.autograd.kkt_solve(S.K, S.M, METHOD, *args, opts=OPTS)
            assert e.value.code == _lib.CPK_ERR_ARGS
    with pytest.raises(cpk.CpkError) as e:  # a K that is no System's
        cpk.autograd.kkt_solve(cpk.KKT(Bk["Q"], Bk["B"], Bk["C"], ctx=gpu_ctx), S.M, METHOD, *good, opts=OPTS)
    assert e.value.code == _lib.CPK_ERR_ARGS
    assert gens == [h.info()["values_generation"] for h in S.handles()]  # nothing was written
