"""The adjoint of the verified solve (cpk_kkt_adjoint, KKT.adjoint): lambda = K' \\ gx is the
verified solve itself, bit for bit; the value gradients are the sampled outer products of the x and
the lambda the call itself used, bit for bit against a scalar Python loop; against a direct solve
they stay within a bound derived from the two solves' own errors; KT is used where A is
nonsymmetric; a stop inside the driver leaves the gradient arrays untouched; exact_dots changes
none of the equalities."""
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

pytestmark = pytest.mark.gpu

SAFETY = 10.0  # tests/test_gpu_parity.py
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
EPS = 2.0 ** -52
# (method, extra options, with KT, seed of gx).  On the tiny members an iteration ends with a residual
# that is pure rounding, and the reference's methods stop with an error when such a quantity comes
# out below zero (structures.py, TINY_SEED): the seeds are the first at which the adjoint solve of
# a standard normal gx runs through in both modes.
SYSTEMS = {"tiny3x2": ("minres", {}, False, 0), "tiny65x63": ("minres", {}, False, 1),
           "cvxqp2_s": ("gmres", {"restart": 20}, True, 0), "syn_nonsym20k": ("gmres", {"restart": 40}, True, 0)}
DENSE_LIMIT = 4000  # dofs up to which K is formed densely; above it a sparse direct LU of the same K


def bits_equal(a, b):
    """The same bit patterns (so -0.0 differs from 0.0), a NaN equal to a NaN at the same place"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)))


def sampled(S, U, V, alpha):
    """alpha * sum_c U[i, c] * V[j, c] on the entries of the canonical CSR matrix S, in its data order:
    the scalar loop of tests/test_gpu_sample_outer.py"""
    out = np.zeros(S.nnz)
    k = U.shape[1]
    q = 0
    for i in range(S.shape[0]):
        for j in S.indices[S.indptr[i]:S.indptr[i + 1]].tolist():
            s = 0.0
            for c in range(k):
                s = s + float(U[i, c]) * float(V[j, c])
            out[q] = float(alpha) * s
            q += 1
    return out


def gradients(P, x, lam):
    """(dA, dB, dC) of the loop for an x and a lambda"""
    n = P["n"]
    xx, xy, lx, ly = x[:n], x[n:], lam[:n], lam[n:]
    col = lambda *v: np.stack(v, axis=1)  # noqa: E731
    return (sampled(P["Q"], col(lx), col(xx), -1.0), sampled(P["B"], col(ly, xy), col(xx, lx), -1.0),
            sampled(P["C"], col(ly), col(xy), 1.0))


@functools.lru_cache(maxsize=None)
def system(name):
    P = F.load(name) if name in ("cvxqp2_s", "syn_nonsym20k") else (ST.tiny_indefinite() if name == "indefinite" else ST.get(name))
    P = dict(P)
    for key in ("Q", "G", "B", "C"):
        M = sp.csr_matrix(P[key], dtype=np.float64)
        M.sum_duplicates()
        M.sort_indices()
        P[key] = M
    return P


def setup(name, ctx):
    """K, KT (or None), M, method, opts and gx on fresh handles"""
    import cpkrylov_amd as cpk
    P = system(name)
    method, extra, with_kt, seed = SYSTEMS.get(name, ("minres", {}, False, 0))
    opts = dict(F.EXPROG_OPTS, **extra)
    A, B, Cm = (cpk.Matrix(P[k], ctx=ctx) for k in ("Q", "B", "C"))
    K = cpk.KKT(A, B, Cm, ctx=ctx)
    KT = cpk.KKT(cpk.Matrix(P["Q"].T.tocsr(), ctx=ctx), B, Cm, ctx=ctx) if with_kt else None
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=ctx)
    M._set(**{k: opts[k] for k in PC_PROPS if k in opts})
    gx = np.random.default_rng(seed).standard_normal(K.N)
    return P, K, KT, M, method, opts, gx


def _same_solve(r, lam, stats, flag):
    assert bits_equal(r["db"], lam)
    assert r["stats"]["niters"] == stats["niters"] and r["flag"]["solved"] == flag["solved"]
    for k in [k for k in stats if k.endswith("History")]:
        assert bits_equal(r["stats"][k], stats[k]), k
    assert r["stats"]["true_resid0"] == stats["true_resid0"] and r["stats"]["true_resid"] == stats["true_resid"]


@pytest.mark.parametrize("exact", (0, 1))
@pytest.mark.parametrize("name", tuple(SYSTEMS))
def test_plumbing_and_lambda_bit_for_bit(gpu_ctx, name, exact):
    """dA, dB, dC are the loop's, fed the x and the lambda = db the call returned; db, the stats and
    the eight sums are K.solve's on K (or KT), cold and with lam0; in both modes"""
    import cpkrylov_amd as cpk
    with cpk.engine_options(gpu_ctx, exact_dots=exact):
        P, K, KT, M, method, opts, gx = setup(name, gpu_ctx)
        x, _, _ = K.solve(method, P["rhs"], M, opts)
        r = K.adjoint(method, x, gx, M, opts, KT=KT)
        lam, stats, flag = (KT or K).solve(method, gx, M, opts)
        _same_solve(r, lam, stats, flag)
        for got, want, key in zip((r["dA"], r["dB"], r["dC"]), gradients(P, x, r["db"]), "ABC"):
            assert bits_equal(got, want), key
        # warm from a perturbed lambda; a caller's arrays are filled in place, lam0 is not written
        lam0 = 0.9 * lam
        out = {"dB": np.zeros(P["B"].nnz), "db": np.zeros(K.N)}
        rw = K.adjoint(method, x, gx, M, opts, KT=KT, lam0=lam0, out=out)
        lw, sw, fw = (KT or K).solve(method, gx, M, opts, x0=lam0)
        _same_solve(rw, lw, sw, fw)
        assert rw["dB"] is out["dB"] and rw["db"] is out["db"] and bits_equal(lam0, 0.9 * lam)
        for got, want, key in zip((rw["dA"], rw["dB"], rw["dC"]), gradients(P, x, rw["db"]), "ABC"):
            assert bits_equal(got, want), key


@pytest.mark.parametrize("name", tuple(SYSTEMS))
def test_against_a_direct_solve(gpu_ctx, name):
    """x_ref = K \\ b, lam_ref = K' \\ gx by a direct solve of K (dense LU up to DENSE_LIMIT dofs; the
    20 000-dof system by a sparse LU of the same K, which a dense one cannot do in a test's time), g_ref
    the sampled -lam_ref x_ref' per block.  With e_x, e_lam the relative 2-norm errors of the device's
    x and lambda, per handle

        ||g - g_ref||_2 <= (e_x + e_lam + e_x e_lam) ||lam_ref|| ||x_ref|| c + 4 eps ||g_ref||_1

    (c = 1 for A and C, 2 for B's two terms): lam x' - lam_ref x_ref' = dlam x_ref' + lam_ref dx' + dlam dx',
    a sampled block's 2-norm is at most the Frobenius norm of the whole, and each entry's own
    rounding -- two products, one sum, alpha -- is below 4 eps of its magnitude.  The adjoint solve is
    held to the project's bound on a solve: a true relative residual within SAFETY of the one the
    forward solve reaches on the same system with the same options."""
    P, K, KT, M, method, opts, gx = setup(name, gpu_ctx)
    n = P["n"]
    x, sx, _ = K.solve(method, P["rhs"], M, opts)
    r = K.adjoint(method, x, gx, M, opts, KT=KT)
    lam = r["db"]
    Ks = sp.bmat([[P["Q"], P["B"].T], [P["B"], -P["C"]]]).tocsc()
    if K.N <= DENSE_LIMIT:
        Kd = Ks.toarray()
        x_ref, lam_ref = np.linalg.solve(Kd, P["rhs"]), np.linalg.solve(Kd.T, gx)
    else:
        lu = spl.splu(Ks)
        x_ref, lam_ref = lu.solve(P["rhs"]), lu.solve(gx, trans="T")
    e_x = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    e_l = np.linalg.norm(lam - lam_ref) / np.linalg.norm(lam_ref)
    fwd = sx["true_resid"]["rnorm"] / sx["true_resid"]["bnorm"]
    adj = r["stats"]["true_resid"]["rnorm"] / r["stats"]["true_resid"]["bnorm"]
    print(f"{name}: e_x {e_x:.3e} e_lam {e_l:.3e} true relative residual forward {fwd:.3e} adjoint {adj:.3e}")
    assert adj <= SAFETY * fwd, (adj, fwd)
    scale = (e_x + e_l + e_x * e_l) * np.linalg.norm(lam_ref) * np.linalg.norm(x_ref)
    for got, ref, c, key in zip((r["dA"], r["dB"], r["dC"]), gradients(P, x_ref, lam_ref), (1.0, 2.0, 1.0), "ABC"):
        err, bound = np.linalg.norm(got - ref), scale * c + 4.0 * EPS * np.sum(np.abs(ref))
        print(f"{name}: d{key} error {err:.3e} bound {bound:.3e} (|g_ref| {np.linalg.norm(ref):.3e})")
        assert err <= bound, (key, err, bound)
    assert x_ref.shape == (n + P["m"],)


def test_kt_is_used_where_a_is_nonsymmetric(gpu_ctx):
    """cpgmres on syn_nonsym20k: with KT the lambda solves K' lam = gx; without it, K lam = gx, a
    different vector -- so the argument is not ignored"""
    name = "syn_nonsym20k"
    P, K, KT, M, method, opts, gx = setup(name, gpu_ctx)
    assert abs(P["Q"] - P["Q"].T).max() > 0
    x, _, _ = K.solve(method, P["rhs"], M, opts)
    with_kt = K.adjoint(method, x, gx, M, opts, KT=KT)
    without = K.adjoint(method, x, gx, M, opts)
    lk, _, _ = K.solve(method, gx, M, opts)
    assert bits_equal(without["db"], lk)
    diff = np.linalg.norm(with_kt["db"] - without["db"]) / np.linalg.norm(with_kt["db"])
    print(f"relative difference of lambda with and without KT: {diff:.3e}")
    assert diff > 1e3 * opts["rtol"]
    Ks = sp.bmat([[P["Q"], P["B"].T], [P["B"], -P["C"]]]).tocsr()
    res_t = np.linalg.norm(gx - Ks.T @ with_kt["db"]) / np.linalg.norm(gx)
    res_n = np.linalg.norm(gx - Ks.T @ without["db"]) / np.linalg.norm(gx)
    print(f"||gx - K' lam|| / ||gx||: with KT {res_t:.3e}, without {res_n:.3e}")
    assert res_t < res_n


def test_refusals(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P, K, _, M, method, opts, gx = setup("tiny65x63", gpu_ctx)
    P3, K3, _, _, _, _, _ = setup("tiny3x2", gpu_ctx)
    x = np.ones(K.N)
    sent = 6.5
    out = {k: np.full(c, sent) for k, c in (("db", K.N), ("dA", P["Q"].nnz), ("dB", P["B"].nnz), ("dC", P["C"].nnz))}
    with pytest.raises(cpk.CpkError) as e:  # KT of other dimensions
        K.adjoint(method, x, gx, M, opts, KT=K3, out=out)
    assert e.value.code == _lib.CPK_ERR_ARGS
    with pytest.raises(cpk.CpkError) as e:  # a short gradient array
        K.adjoint(method, x, gx, M, opts, out=dict(out, dB=np.full(P["B"].nnz - 1, sent)))
    assert e.value.code == _lib.CPK_ERR_DIM
    with pytest.raises(cpk.CpkError) as e:
        K.adjoint(method, x[:-1], gx, M, opts, out=out)
    assert e.value.code == _lib.CPK_ERR_DIM
    with pytest.raises(cpk.CpkError) as e:
        K.adjoint("nosuch", x, gx, M, opts, out=out)
    assert e.value.code == _lib.CPK_ERR_ARGS
    assert all(np.all(v == sent) for v in out.values())


def test_a_driver_stop_leaves_the_gradients_untouched(gpu_ctx):
    """structures.tiny_indefinite under exact_dots: the call raises the error of K.solve on the same
    right-hand side, carrying the driver's lambda, and sentinel-filled gradient arrays stay as they
    were"""
    import cpkrylov_amd as cpk
    opts = dict(F.EXPROG_OPTS)
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        P, K, _, M, method, opts, _ = setup("indefinite", gpu_ctx)
        gx = P["rhs"]
        with pytest.raises(cpk.IndefiniteError) as es:
            K.solve(method, gx, M, opts)
        sent = -3.75
        out = {k: np.full(c, sent) for k, c in (("dA", P["Q"].nnz), ("dB", P["B"].nnz), ("dC", P["C"].nnz))}
        with pytest.raises(cpk.IndefiniteError) as ea:
            K.adjoint(method, np.ones(K.N), gx, M, opts, out=out)
    assert ea.value.code == es.value.code and str(ea.value) == str(es.value)
    assert bits_equal(ea.value.partial[0], es.value.partial[0]) and bits_equal(ea.value.partial[1], es.value.partial[1])
    assert all(np.all(v == sent) for v in out.values())


def test_device_tensors(gpu_ctx):
    """x, gx and out= as device tensors: the bits of the host path; an absent gradient is not formed;
    lam0 is out['db'] itself"""
    assert torch is not None and torch.cuda.is_available()
    import cpkrylov_amd as cpk
    P, K, KT, M, method, opts, gx = setup("cvxqp2_s", gpu_ctx)
    x, _, _ = K.solve(method, P["rhs"], M, opts)
    r = K.adjoint(method, x, gx, M, opts, KT=KT)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    new = lambda c: torch.full((c,), -1.5, dtype=torch.float64, device="cuda")  # noqa: E731
    out = {"db": new(K.N), "dA": new(P["Q"].nnz), "dC": new(P["C"].nnz)}
    rd = K.adjoint(method, dev(x), dev(gx), M, opts, KT=KT, out=out)
    assert rd["db"] is out["db"] and rd["dB"] is None
    for key in ("db", "dA", "dC"):
        assert bits_equal(out[key].cpu().numpy(), r[key]), key
    assert rd["stats"]["true_resid"] == r["stats"]["true_resid"]
    out["db"].mul_(0.9)
    torch.cuda.synchronize()
    lam0 = out["db"].cpu().numpy()
    rw = K.adjoint(method, x, gx, M, opts, KT=KT, lam0=lam0)
    out["dB"] = new(P["B"].nnz)
    K.adjoint(method, dev(x), dev(gx), M, opts, KT=KT, lam0=out["db"], out=out)
    for key in ("db", "dA", "dB", "dC"):
        assert bits_equal(out[key].cpu().numpy(), rw[key]), key
    with pytest.raises(cpk.CpkError) as e:
        K.adjoint(method, dev(x), dev(gx), M, opts, out={"db": new(K.N).float()})
    assert e.value.code == cpk._lib.CPK_ERR_ARGS
