"""cpk.autograd.kkt_solve_batch: the verified solve with a batch dimension on rhs.  The forward is
K.solve_block; under exact_dots the value gradients of loss = sum_j w_j . x_j are the sums of the
per-column kkt_solve gradients within the reassociation bound of tests/test_gpu_kkt_block.py and
rhs.grad's rows are the per-column ones bit for bit; a System's handles are reused; the backward of a
call has to run before the next forward."""
import numpy as np
import pytest

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

from test_gpu_kkt_adjoint import bits_equal, sampled
from test_gpu_kkt_block import EPS, OPTS, PC_PROPS, TINY_SEEDS, load

pytestmark = pytest.mark.gpu

METHOD = "minres"


def leaves(vals):
    assert torch is not None and torch.cuda.is_available()
    return [torch.from_numpy(np.ascontiguousarray(v)).cuda().requires_grad_(True) for v in vals]


def problem(name, k):
    """the System's matrices, the value arrays, rhs (k, N) and the loss's weights W (k, N): rows the
    single-column solve runs through on (TINY_SEEDS)"""
    P = load(name)
    N = P["n"] + P["m"]
    seeds = TINY_SEEDS.get((name, METHOD), tuple(range(9)))
    W = np.stack([np.random.default_rng(s).standard_normal(N) for s in seeds[:k]])
    rhs = np.stack([(P["rhs"], 1e-3 * P["rhs"], W[(j + 1) % k])[j % 3] for j in range(k)])
    return P, (P["Q"].data, P["B"].data, P["C"].data, P["G"].data), rhs, W


@pytest.mark.parametrize("k", (3, 9))
@pytest.mark.parametrize("name", ("tiny65x63", "cvxqp1_m"))
def test_forward_is_solve_block_and_gradients_are_the_columns_sums(gpu_ctx, name, k):
    import cpkrylov_amd as cpk
    P, vals, rhs, W = problem(name, k)
    n = P["n"]
    S = cpk.autograd.System(P["Q"], P["B"], P["C"], P["G"], ctx=gpu_ctx)
    S1 = cpk.autograd.System(P["Q"], P["B"], P["C"], P["G"], ctx=gpu_ctx)
    K = cpk.KKT(P["Q"], P["B"], P["C"], ctx=gpu_ctx)
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=gpu_ctx)
    M._set(**{key: OPTS[key] for key in PC_PROPS})
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        ta, tb, tc, tg, tr = leaves(vals + (rhs,))
        X = cpk.autograd.kkt_solve_batch(S.K, S.M, METHOD, ta, tb, tc, tg, tr, opts=OPTS)
        assert tuple(X.shape) == rhs.shape
        (torch.from_numpy(W).cuda() * X).sum().backward()
        Xh, _, _ = K.solve_block(METHOD, np.asfortranarray(rhs.T), M, OPTS)
        assert bits_equal(X.detach().cpu().numpy().T, Xh)
        assert tg.grad is None
        # the per-column function on a System of its own
        total = [np.zeros(v.size) for v in vals[:3]]
        lam = []
        for j in range(k):
            sa, sb, sc, sg, sr = leaves(vals + (rhs[j],))
            x = cpk.autograd.kkt_solve(S1.K, S1.M, METHOD, sa, sb, sc, sg, sr, opts=OPTS)
            assert bits_equal(x.detach().cpu().numpy(), Xh[:, j])
            (torch.from_numpy(W[j]).cuda() * x).sum().backward()
            assert bits_equal(tr.grad[j].cpu().numpy(), sr.grad.cpu().numpy()), j
            lam.append(sr.grad.cpu().numpy())
            for t, s in zip(total, (sa, sb, sc)):
                t += s.grad.cpu().numpy()
    aX, aL = np.abs(Xh), np.abs(np.column_stack(lam))
    U, V = np.empty((P["m"], 2 * k)), np.empty((n, 2 * k))
    U[:, 0::2], U[:, 1::2], V[:, 0::2], V[:, 1::2] = aL[n:], aX[n:], aX[:n], aL[:n]
    mags = (sampled(P["Q"], aL[:n], aX[:n], 1.0), sampled(P["B"], U, V, 1.0), sampled(P["C"], aL[n:], aX[n:], 1.0))
    for t, tot, mag, terms, key in zip((ta, tb, tc), total, mags, (k, 2 * k, k), "ABC"):
        delta, bound = np.abs(t.grad.cpu().numpy() - tot), 2.0 * (terms + 1) * EPS * mag
        print(f"{name} k={k} d{key}: max |delta| / bound {np.max(delta / np.where(bound > 0, bound, 1.0)):.3e}")
        assert np.all(delta <= bound), key


def test_handles_are_reused_and_a_second_forward_blocks_the_first_backward(gpu_ctx):
    """no Matrix, KKT or opLDL2 per call: every handle's values generation rises by one per forward and
    the objects stay; a backward after a later forward on the same System raises CPK_ERR_ARGS"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P, vals, rhs, W = problem("cvxqp1_m", 3)
    S = cpk.autograd.System(P["Q"], P["B"], P["C"], P["G"], ctx=gpu_ctx)
    hs = S.handles()
    ids = [id(o) for o in hs + (S.K, S.M)]
    gens = [[h.info()["values_generation"] for h in hs]]
    outs = []
    for scale in (1.0, 0.5):
        ts = leaves(vals + (scale * rhs,))
        outs.append((cpk.autograd.kkt_solve_batch(S.K, S.M, METHOD, *ts, opts=OPTS), ts))
        gens.append([h.info()["values_generation"] for h in hs])
    assert [b - a for a, b in zip(gens[0], gens[1])] == [1] * 5 and [b - a for a, b in zip(gens[1], gens[2])] == [1] * 5
    assert ids == [id(o) for o in S.handles() + (S.K, S.M)] and list(S._blocks) == [3]
    with pytest.raises(cpk.CpkError) as e:
        outs[0][0].sum().backward()
    assert e.value.code == _lib.CPK_ERR_ARGS
    outs[1][0].sum().backward()  # the latest forward's backward runs
    assert all(t.grad is not None for t in outs[1][1][:3] + outs[1][1][4:])


def test_wrong_tensors_are_refused(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P, vals, rhs, W = problem("tiny65x63", 3)
    S = cpk.autograd.System(P["Q"], P["B"], P["C"], P["G"], ctx=gpu_ctx)
    good = leaves(vals + (rhs,))
    gens = [h.info()["values_generation"] for h in S.handles()]
    for make, code in ((lambda t: t.float(), _lib.CPK_ERR_ARGS), (lambda t: t.t(), _lib.CPK_ERR_DIM),
                       (lambda t: t[0], _lib.CPK_ERR_DIM), (lambda t: t.detach().cpu(), _lib.CPK_ERR_ARGS),
                       (lambda t: torch.stack([t, t], dim=2)[:, :, 0], _lib.CPK_ERR_ARGS)):
        with pytest.raises(cpk.CpkError) as e:
            cpk.autograd.kkt_solve_batch(S.K, S.M, METHOD, *good[:4], make(good[4]), opts=OPTS)
        assert e.value.code == code
    with pytest.raises(cpk.CpkError) as e:
        cpk.autograd.kkt_solve_batch(S.K, S.M, "gmres", *good, opts=OPTS)
    assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
    assert gens == [h.info()["values_generation"] for h in S.handles()]  # nothing was written
