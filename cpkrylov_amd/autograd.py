"""The verified solve of K x = b as a differentiable torch function (implicit differentiation).

    S = cpk.autograd.System(A, B, C, G)                  # once: the handles, K, M
    x = cpk.autograd.kkt_solve(S.K, S.M, "minres", a_vals, b_vals, c_vals, g_vals, rhs, opts)
    loss(x).backward()                                    # a_vals.grad, b_vals.grad, c_vals.grad, rhs.grad

Forward: the values go into the System's handles on the device (`Matrix.set_values`), M is
refactored and `K.solve` runs on device tensors.  Backward: one more solve with the same factors
(`K.adjoint`): lambda = K' \\ gx = dL/d(rhs), and dL/d(values) = the sampled -lambda x' on each
handle's own sparsity.  g_vals gets no gradient: the preconditioner does not change the solution.
Second derivatives are not formed.  `kkt_solve_batch` is the same function for a (k, N) batch of
right-hand sides: one `K.solve_block` forward, one `K.adjoint_block` backward that sums the value
gradients over the batch in one pass per handle.  torch is imported when a function of this module is
first used.
"""
import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import CpkError
from .api import BLOCK_METHODS, KKT, Matrix, default_context, opLDL2

_PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")


def _canonical(M):
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return M


class System:
    """The handles one differentiable solve works on, created once and reused by every call:
    the `Matrix` handles of A, B, C (K's blocks), G and -C (the preconditioner's), K = KKT(A, B, C)
    and M = opLDL2(G, B, -C).  A, B, C, G are scipy (or dense) matrices giving the sparsity and the
    first values; the value tensors of `kkt_solve` are in the order of their canonical CSR data.

    symmetric=False also builds the handle of A' and KT = KKT(A', B, C) for the adjoint solve (a
    method for nonsymmetric A, cpgmres or cpdqgmres, is then the caller's choice); with the
    default the caller asserts that A is symmetric, which is not checked.

    warm_adjoint = True starts each backward solve from the previous backward's lambda: that
    solve's stop test then runs on the correction system (KKT.solve)."""

    def __init__(self, A, B, C, G, ctx=None, symmetric=True):
        self.ctx = ctx or default_context()
        A, B, C, G = (_canonical(M) for M in (A, B, C, G))
        self.A, self.B, self.C, self.G = (Matrix(M, self.ctx) for M in (A, B, C, G))
        self.negC = Matrix(-C, self.ctx)
        self.K = KKT(self.A, self.B, self.C, ctx=self.ctx)
        self.M = opLDL2(self.G, self.B, self.negC, ctx=self.ctx)
        self.AT = self.KT = self._tperm = None
        if not symmetric:
            # A' in canonical CSR: entry q of it is entry tperm[q] of A
            T = sp.csr_matrix((np.arange(1.0, A.nnz + 1.0), A.indices, A.indptr), shape=A.shape).T.tocsr()
            T.sort_indices()
            self._tperm = (T.data - 1.0).astype(np.int64)
            self.AT = Matrix(sp.csr_matrix((A.data[self._tperm], T.indices, T.indptr), shape=T.shape), self.ctx)
            self.KT = KKT(self.AT, self.B, self.C, ctx=self.ctx)
        self.K._system = self
        self.N = self.K.N
        self.warm_adjoint = False
        self._lam = self._rhs = self._sol = self._tperm_dev = None
        self._blocks, self._lamb = {}, None  # kkt_solve_batch: (rhs, solution) blocks by batch size, the last Lambda

    def handles(self):
        return (self.A, self.B, self.C, self.G, self.negC)


def _check_tensor(t, what, count):
    if not all(hasattr(t, a) for a in ("is_cuda", "data_ptr", "dtype", "is_contiguous")) or not t.is_cuda or \
            "float64" not in str(t.dtype) or not t.is_contiguous():
        raise CpkError(_lib.CPK_ERR_ARGS, f"{what}: a contiguous float64 CUDA tensor expected")
    if t.numel() != count:
        raise CpkError(_lib.CPK_ERR_DIM, f"{what}: {count} values expected")


_FN = None


def _function():
    """The torch.autograd.Functions (kkt_solve's, kkt_solve_batch's), defined when first used (torch is
    imported here)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    def load_values(S, opts, refactor, a, b, c, g):
        """The values into the System's handles on the device, M's properties, one refactor"""
        S.A.set_values(a), S.B.set_values(b), S.C.set_values(c)
        S.G.set_values(g), S.negC.set_values(-c)
        if S.AT is not None:
            if S._tperm_dev is None:
                S._tperm_dev = torch.from_numpy(S._tperm).to(a.device)
            S.AT.set_values(a[S._tperm_dev].contiguous())
        S.M._set(**{k: opts[k] for k in _PC_PROPS if k in (opts or {})})
        if refactor:
            S.M.refactor(S.G, S.B, S.negC)

    def generations(S):
        return tuple(h.info()["values_generation"] for h in S.handles())

    class KktSolve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, S, method, opts, refactor, a_vals, b_vals, c_vals, g_vals, rhs):
            a, b, c, g, r = (t.detach() for t in (a_vals, b_vals, c_vals, g_vals, rhs))
            load_values(S, opts, refactor, a, b, c, g)
            # the solves run on the System's own two vectors: M keys its cached solvers (workspace,
            # captured graphs) by the operand addresses too, so they are found again at every call
            if S._rhs is None:
                S._rhs = torch.empty(S.N, dtype=torch.float64, device=r.device)
                S._sol = torch.empty_like(S._rhs)
            S._rhs.copy_(r)
            _, stats, flag = S.K.solve(method, S._rhs, S.M, opts, out=S._sol)
            x = S._sol.clone()
            S.last_forward = (stats, flag)
            ctx.S, ctx.method, ctx.opts = S, method, opts
            ctx.gens = generations(S)
            ctx.save_for_backward(x)
            return x

        @staticmethod
        def backward(ctx, gx):
            S = ctx.S
            (x,) = ctx.saved_tensors
            if generations(S) != ctx.gens:
                raise CpkError(_lib.CPK_ERR_ARGS, "kkt_solve backward: the System's handles hold the values of a later "
                               "forward (run each backward before the next forward on the same System)")
            S._rhs.copy_(gx.detach())
            need = ctx.needs_input_grad[4:7]
            out = {"db": S._sol}
            for key, h, want in zip(("dA", "dB", "dC"), (S.A, S.B, S.C), need):
                if want:
                    out[key] = torch.empty(h.info()["entries"], dtype=torch.float64, device=x.device)
            lam0 = None
            if S.warm_adjoint and S._lam is not None:
                S._sol.copy_(S._lam)
                lam0 = S._sol
            r = S.K.adjoint(ctx.method, x, S._rhs, S.M, ctx.opts, KT=S.KT, lam0=lam0, out=out)
            S.last_backward = (r["stats"], r["flag"])
            lam = S._sol.clone()
            S._lam = lam if S.warm_adjoint else None
            return (None, None, None, None, out.get("dA"), out.get("dB"), out.get("dC"), None, lam)

    class KktSolveBatch(torch.autograd.Function):
        """kkt_solve for a (k, N) batch of right-hand sides: one solve_block, one adjoint_block"""

        @staticmethod
        def forward(ctx, S, method, opts, refactor, a_vals, b_vals, c_vals, g_vals, rhs):
            a, b, c, g, r = (t.detach() for t in (a_vals, b_vals, c_vals, g_vals, rhs))
            load_values(S, opts, refactor, a, b, c, g)
            # the System's own block buffers, one pair per batch size (as _rhs and _sol above)
            k = r.shape[0]
            if k not in S._blocks:
                S._blocks[k] = (torch.empty((k, S.N), dtype=torch.float64, device=r.device),
                                torch.empty((k, S.N), dtype=torch.float64, device=r.device))
            rhsb, solb = S._blocks[k]
            rhsb.copy_(r)
            _, stats, flags = S.K.solve_block(method, rhsb, S.M, opts, out=solb)
            x = solb.clone()
            S.last_forward = (stats, flags)
            ctx.S, ctx.method, ctx.opts = S, method, opts
            ctx.gens = generations(S)
            ctx.save_for_backward(x)
            return x

        @staticmethod
        def backward(ctx, gx):
            S = ctx.S
            (x,) = ctx.saved_tensors
            if generations(S) != ctx.gens:
                raise CpkError(_lib.CPK_ERR_ARGS, "kkt_solve_batch backward: the System's handles hold the values of a "
                               "later forward (run each backward before the next forward on the same System)")
            rhsb, solb = S._blocks[x.shape[0]]
            rhsb.copy_(gx.detach())
            out = {"db": solb}
            for key, h, want in zip(("dA", "dB", "dC"), (S.A, S.B, S.C), ctx.needs_input_grad[4:7]):
                if want:
                    out[key] = torch.empty(h.info()["entries"], dtype=torch.float64, device=x.device)
            lam0 = None
            if S.warm_adjoint and S._lamb is not None and S._lamb.shape == solb.shape:
                solb.copy_(S._lamb)
                lam0 = solb
            r = S.K.adjoint_block(ctx.method, x, rhsb, S.M, ctx.opts, Lam0=lam0, out=out)
            S.last_backward = (r["stats"], r["flags"])
            lam = solb.clone()
            S._lamb = lam if S.warm_adjoint else None
            return (None, None, None, None, out.get("dA"), out.get("dB"), out.get("dC"), None, lam)

    _FN = (KktSolve, KktSolveBatch)
    return _FN


def kkt_solve(K, M, method, a_vals, b_vals, c_vals, g_vals, rhs, opts=None, refactor=True):
    """x = K \\ rhs with K = [A B'; B -C] on the values a_vals, b_vals, c_vals and the preconditioner
    M = opLDL2(G, B, -C) on g_vals, b_vals, c_vals, differentiable with respect to a_vals, b_vals,
    c_vals and rhs.  K and M are a `System`'s (S.K, S.M): its handles take the values, and nothing
    is created per call.  All tensors are contiguous float64 CUDA tensors (CPK_ERR_ARGS otherwise),
    the values in the order of the canonical CSR data of the System's matrices.  refactor=False
    keeps M's factors (M need not follow K for the solve to be right, only to be fast).  Run the
    backward of a call before the next forward on the same System."""
    S = getattr(K, "_system", None)
    if not isinstance(S, System) or M is not S.M:
        raise CpkError(_lib.CPK_ERR_ARGS, "kkt_solve: K and M are the K and M of one cpk.autograd.System")
    name = getattr(method, "_cpk_method", method)
    if name not in _lib.METHODS:
        raise CpkError(_lib.CPK_ERR_ARGS, f"unknown method {method!r}")
    for t, what, h in ((a_vals, "a_vals", S.A), (b_vals, "b_vals", S.B), (c_vals, "c_vals", S.C), (g_vals, "g_vals", S.G)):
        _check_tensor(t, what, h.info()["entries"])
    _check_tensor(rhs, "rhs", S.N)
    return _function()[0].apply(S, name, dict(opts) if opts else None, bool(refactor), a_vals, b_vals, c_vals, g_vals, rhs)


def kkt_solve_batch(K, M, method, a_vals, b_vals, c_vals, g_vals, rhs, opts=None, refactor=True):
    """`kkt_solve` with a batch dimension on rhs: a contiguous (k, N) float64 CUDA tensor, row j one
    right-hand side (the N x k block of `KKT.solve_block`).  Returns X (k, N), X[j] = K \\ rhs[j].
    Forward: the values into the System's handles, one refactor, one `K.solve_block` on the System's
    own block buffers.  Backward: one `K.adjoint_block`: a_vals.grad, b_vals.grad and c_vals.grad are
    the sums over the batch, formed in one pass per handle, and rhs.grad is Lambda (k, N).  The block
    methods are cpcg and cpminres and there is no KT, so the System is a symmetric one.  The
    generation check and `warm_adjoint` are `kkt_solve`'s."""
    S = getattr(K, "_system", None)
    if not isinstance(S, System) or M is not S.M:
        raise CpkError(_lib.CPK_ERR_ARGS, "kkt_solve_batch: K and M are the K and M of one cpk.autograd.System")
    name = getattr(method, "_cpk_method", method)
    if name not in _lib.METHODS:
        raise CpkError(_lib.CPK_ERR_ARGS, f"unknown method {method!r}")
    if name not in BLOCK_METHODS:
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED, f"cp{name} takes one right-hand side; the block solve covers cpcg and cpminres")
    if S.KT is not None:
        raise CpkError(_lib.CPK_ERR_UNSUPPORTED, "kkt_solve_batch: the block adjoint has no KT (a symmetric System only)")
    for t, what, h in ((a_vals, "a_vals", S.A), (b_vals, "b_vals", S.B), (c_vals, "c_vals", S.C), (g_vals, "g_vals", S.G)):
        _check_tensor(t, what, h.info()["entries"])
    if getattr(rhs, "ndim", 0) != 2 or rhs.shape[1] != S.N:
        raise CpkError(_lib.CPK_ERR_DIM, f"rhs: a (k, N) tensor with N = {S.N} expected")
    _check_tensor(rhs, "rhs", rhs.shape[0] * S.N)
    return _function()[1].apply(S, name, dict(opts) if opts else None, bool(refactor), a_vals, b_vals, c_vals, g_vals, rhs)
