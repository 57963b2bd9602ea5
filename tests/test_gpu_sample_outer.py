"""cpk_mat_sample_outer[_device] (adjoint.hip) against a scalar Python loop, BIT FOR BIT: a sum of
outer products sampled on a handle's sparsity and handed back through the handle's value map, for
handles created from canonical CSR (identity map), CSR with unsorted columns (perm), CSR and CSC
with duplicate entries (sptr/src) and canonical CSC, on patterns that take every path of the
kernel: one entry, several row blocks, empty rows, no entry at all, a long row inside a block's
cap and one above it.  Then the refusals, each leaving its output untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import fixtures as F
import structures as ST
from devbuf import DeviceArray
from rawmat import raw_matrix, unsorted_csr

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
LONG_ARROW = 2100  # entries of the long row of longrow's A: above kSpmvCap = 2048
SENT = -4321.125


def _dp(a):
    return a.ctypes.data_as(PD) if a.size else None


def bits_equal(a, b):
    """The same bit patterns (so -0.0 differs from 0.0), a NaN equal to a NaN at the same place"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)))


# ---- the reference ---------------------------------------------------------------------------
def reference(rows, cols, U, V, alpha):
    """out[e] for the raw entries e = (rows[e], cols[e]) of a creating call.  The stored entries are
    the distinct (i, j) in row-major order; g_q of each is the scalar loop below, and the value map
    -- raw entry e went into the stored entry of its own (i, j) -- takes it back to every e."""
    k = U.shape[1]
    stored = sorted(set(zip(rows.tolist(), cols.tolist())))
    g = {}
    for (i, j) in stored:
        s = 0.0
        for c in range(k):
            s = s + float(U[i, c]) * float(V[j, c])
        g[(i, j)] = float(alpha) * s
    return np.array([g[(i, j)] for i, j in zip(rows.tolist(), cols.tolist())], dtype=np.float64)


# ---- the patterns ----------------------------------------------------------------------------
def _longrow_A():
    """saddle_system(4000)'s Q with a symmetric arrow: row 0 holds LONG_ARROW + 1 entries"""
    S = ST.saddle_system(N=4000)
    n = S["n"]
    v = np.zeros(n)
    v[1:LONG_ARROW + 1] = 1e-4
    arrow = sp.lil_matrix((n, n))
    arrow[0, :] = v
    arrow[:, 0] = v.reshape(n, 1)
    return (S["Q"] + arrow.tocsr()).tocsr()


def _holes():
    """40 x 30, rows 3 ... 10, 17 and the last row empty"""
    rng = np.random.default_rng(40)
    M = sp.random(40, 30, density=0.2, random_state=rng, format="lil")
    for r in list(range(3, 11)) + [17, 39]:
        M[r, :] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    return M


@functools.lru_cache(maxsize=None)
def pattern(name):
    M = {"tiny1x1_A": lambda: ST.get("tiny1x1")["Q"], "tiny65x63_B": lambda: ST.get("tiny65x63")["B"],
         "holes": _holes, "nnz0": lambda: sp.csr_matrix((5, 4)), "arrow_row_B": lambda: ST.get("arrow_row")["B"],
         "longrow_A": _longrow_A, "syn_symm20k_A": lambda: F.load("syn_symm20k")["Q"]}[name]()
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    M.sort_indices()
    return M


def _row_of(S):
    return np.repeat(np.arange(S.shape[0]), np.diff(S.indptr)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def raw(name, way):
    """(kind, ptr, ind, rows, cols) of the creating call: the index arrays handed over and each raw
    entry's (row, column)"""
    S = pattern(name)
    rows, cols = _row_of(S), S.indices.astype(np.int64)
    if way == "csr":
        return "csr", S.indptr.astype(np.int64), S.indices.astype(np.int32), rows, cols
    if way == "unsorted":
        ptr, ind, order = unsorted_csr(S)
        return "csr", ptr, ind, rows[order], cols[order]
    if way == "dup_csr":  # every row reversed, then every third entry of it once more at the row's end
        ptr, ind, rr = [0], [], []
        for i in range(S.shape[0]):
            e = S.indices[S.indptr[i]:S.indptr[i + 1]][::-1].tolist()
            e = e + e[::3]
            ind += e
            rr += [i] * len(e)
            ptr.append(len(ind))
        return "csr", np.array(ptr, np.int64), np.array(ind, np.int32), np.array(rr, np.int64), np.array(ind, np.int64)
    T = S.tocsc()
    T.sort_indices()
    if way == "csc":
        return "csc", T.indptr, T.indices, T.indices.astype(np.int64), \
            np.repeat(np.arange(T.shape[1]), np.diff(T.indptr)).astype(np.int64)
    assert way == "dup_csc"  # every column reversed, every third entry of it once more at its end
    ptr, ind, cc = [0], [], []
    for j in range(T.shape[1]):
        e = T.indices[T.indptr[j]:T.indptr[j + 1]][::-1].tolist()
        e = e + e[::3]
        ind += e
        cc += [j] * len(e)
        ptr.append(len(ind))
    return "csc", np.array(ptr, np.int64), np.array(ind, np.int64), np.array(ind, np.int64), np.array(cc, np.int64)


def handle(name, way, ctx):
    kind, ptr, ind, rows, cols = raw(name, way)
    return raw_matrix(kind, pattern(name).shape, ptr, ind, np.ones(len(rows)), ctx=ctx), rows, cols


def operands(shape, k, seed):
    """Wide exponents (the order of a sum shows), signed zeros"""
    rng = np.random.default_rng(seed)

    def one(n):
        a = rng.uniform(1.0, 2.0, (n, k)) * 2.0 ** rng.integers(-140, 140, (n, k)) * rng.choice([-1.0, 1.0], (n, k))
        a[rng.random((n, k)) < 0.08] = 0.0
        a[rng.random((n, k)) < 0.04] = -0.0
        return np.asfortranarray(a)

    return one(shape[0]), one(shape[1])


def call_host(M, U, V, alpha, count, ldu=None, ldv=None, out=None):
    from cpkrylov_amd import _lib
    out = np.full(count, SENT) if out is None else out
    k = U.shape[1]
    rc = _lib.lib.cpk_mat_sample_outer(M.h, k, _dp(U), ldu or max(M.shape[0], 1), _dp(V), ldv or max(M.shape[1], 1),
                                       float(alpha), _dp(out), count)
    return rc, out


SMALL = ("tiny1x1_A", "tiny65x63_B", "holes")
CASES = [(n, w) for n in SMALL for w in ("csr", "unsorted", "dup_csr", "dup_csc", "csc")] + \
        [("nnz0", "csr"), ("nnz0", "csc"), ("arrow_row_B", "csr"), ("arrow_row_B", "unsorted"), ("arrow_row_B", "csc"),
         ("longrow_A", "csr"), ("longrow_A", "dup_csr"), ("syn_symm20k_A", "csr"), ("syn_symm20k_A", "csc")]


@pytest.mark.parametrize("name,way", CASES)
def test_against_the_python_loop(gpu_ctx, name, way):
    """Host and device variants, every k and alpha (the large patterns: each k and each alpha
    once), leading dimensions above the row counts with NaN padding that is neither read nor
    written"""
    from cpkrylov_amd import _lib
    M, rows, cols = handle(name, way, gpu_ctx)
    count = len(rows)
    info = M.info()
    assert info["entries"] == count and info["nnz"] == pattern(name).nnz
    if way in ("dup_csr", "dup_csc") and count:
        assert count > info["nnz"]
    combos = [(k, a) for k in (0, 1, 2, 3) for a in (1.0, -1.0, 0.3)] if name in SMALL or name == "nnz0" else \
        [(0, -1.0), (1, -1.0), (2, 0.3), (3, 1.0)]
    nr, nc = M.shape
    for k, alpha in combos:
        U, V = operands(M.shape, k, 100 * k + 7)
        want = reference(rows, cols, U, V, alpha)
        rc, got = call_host(M, U, V, alpha, count)
        assert rc == 0 and bits_equal(got, want), (k, alpha)
        if k == 0 and count:
            assert bits_equal(got, np.full(count, alpha * 0.0))
        # the device variant on padded operands
        ldu, ldv = nr + 3, nc + 5
        Up, Vp = np.full((ldu, k), np.nan, order="F"), np.full((ldv, k), np.nan, order="F")
        Up[:nr], Vp[:nc] = U, V
        dU, dV, dO = DeviceArray.of(Up.ravel("F")), DeviceArray.of(Vp.ravel("F")), DeviceArray.of(np.full(count, SENT))
        _lib.check(_lib.lib.cpk_mat_sample_outer_device(M.h, k, dU.p, ldu, dV.p, ldv, alpha, dO.p, count))
        gpu_ctx.synchronize()
        assert bits_equal(dO.numpy(), want), (k, alpha)
        assert bits_equal(dU.numpy(), Up.ravel("F")) and bits_equal(dV.numpy(), Vp.ravel("F"))
        # the host variant with the same leading dimensions
        rc, got = call_host(M, Up, Vp, alpha, count, ldu, ldv)
        assert rc == 0 and bits_equal(got, want), (k, alpha)


@pytest.mark.parametrize("way", ("dup_csr", "dup_csc"))
def test_a_duplicated_pair_gets_the_same_bits_twice(gpu_ctx, way):
    M, rows, cols = handle("tiny65x63_B", way, gpu_ctx)
    U, V = operands(M.shape, 2, 5)
    rc, got = call_host(M, U, V, -1.0, len(rows))
    assert rc == 0
    seen = {}
    twice = 0
    for e, key in enumerate(zip(rows.tolist(), cols.tolist())):
        if key in seen:
            twice += 1
            assert bits_equal(got[e:e + 1], got[seen[key]:seen[key] + 1])
        seen[key] = e
    assert twice > 1000


@pytest.mark.parametrize("name,way", (("holes", "unsorted"), ("longrow_A", "csr"), ("arrow_row_B", "csc")))
def test_a_nan_stays_in_its_row(gpu_ctx, name, way):
    M, rows, cols = handle(name, way, gpu_ctx)
    r = 0 if name == "longrow_A" else (ST.ARROW_ROW if name == "arrow_row_B" else int(np.argmax(np.bincount(rows))))
    assert np.count_nonzero(rows == r) > 0
    rng = np.random.default_rng(3)
    U, V = np.asfortranarray(rng.standard_normal((M.shape[0], 2))), np.asfortranarray(rng.standard_normal((M.shape[1], 2)))
    U[r, 1] = np.nan
    rc, got = call_host(M, U, V, 0.3, len(rows))
    assert rc == 0 and np.array_equal(np.isnan(got), rows == r)
    assert bits_equal(got, reference(rows, cols, U, V, 0.3))


def test_python_front_end(gpu_ctx):
    """Matrix.sample_outer on NumPy arrays (a vector is one column; out=) and on device tensors"""
    import cpkrylov_amd as cpk
    S = pattern("holes")
    M = cpk.Matrix(S, ctx=gpu_ctx)
    rows, cols = _row_of(S), S.indices.astype(np.int64)
    U, V = operands(S.shape, 2, 11)
    want = reference(rows, cols, U, V, -1.0)
    assert bits_equal(M.sample_outer(U, V, alpha=-1.0), want)
    assert bits_equal(M.sample_outer(U[:, 0], V[:, 0]), reference(rows, cols, U[:, :1], V[:, :1], 1.0))
    out = np.full(S.nnz, SENT)
    assert M.sample_outer(U, V, alpha=-1.0, out=out) is out and bits_equal(out, want)
    Mc = cpk.Matrix(S, ctx=gpu_ctx, csc=True)  # values in CSC order
    T = S.tocsc()
    T.sort_indices()
    tc = np.repeat(np.arange(T.shape[1]), np.diff(T.indptr))
    assert bits_equal(Mc.sample_outer(U, V, alpha=-1.0), reference(T.indices.astype(np.int64), tc, U, V, -1.0))
    with pytest.raises(cpk.CpkError) as e:
        M.sample_outer(U[:-1], V)
    assert e.value.code == cpk._lib.CPK_ERR_DIM
    assert torch is not None and torch.cuda.is_available()
    tu, tv = torch.from_numpy(U.T.copy()).cuda(), torch.from_numpy(V.T.copy()).cuda()
    to = torch.full((S.nnz,), SENT, dtype=torch.float64, device="cuda")
    assert M.sample_outer(tu, tv, alpha=-1.0, out=to) is to and bits_equal(to.cpu().numpy(), want)
    with pytest.raises(cpk.CpkError) as e:
        M.sample_outer(tu.float(), tv, out=to)
    assert e.value.code == cpk._lib.CPK_ERR_ARGS


def test_refusals_leave_the_output_untouched(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    lib = _lib.lib
    M, rows, cols = handle("tiny65x63_B", "dup_csr", gpu_ctx)
    count = len(rows)
    nr, nc = M.shape
    U, V = operands(M.shape, 2, 1)
    out = np.full(count + 1, SENT)
    dU, dV, dO = DeviceArray.of(U.ravel("F")), DeviceArray.of(V.ravel("F")), DeviceArray.of(out)

    def both(k, u, ldu, v, ldv, o, cnt, mat=M):
        """the two variants' codes for the same arguments (u, v, o: True for the array, None for NULL)"""
        rh = lib.cpk_mat_sample_outer(mat.h if mat else None, k, _dp(U) if u else None, ldu, _dp(V) if v else None, ldv, 1.0,
                                      _dp(out) if o else None, cnt)
        rd = lib.cpk_mat_sample_outer_device(mat.h if mat else None, k, dU.p if u else None, ldu, dV.p if v else None, ldv,
                                             1.0, dO.p if o else None, cnt)
        return rh, rd

    E = _lib
    assert both(2, True, nr, True, nc, True, count - 1) == (E.CPK_ERR_DIM,) * 2      # a wrong count
    assert both(2, True, nr, True, nc, True, count + 1) == (E.CPK_ERR_DIM,) * 2
    assert both(-1, True, nr, True, nc, True, count) == (E.CPK_ERR_DIM,) * 2
    assert both(2, True, nr - 1, True, nc, True, count) == (E.CPK_ERR_DIM,) * 2      # short leading dimensions
    assert both(2, True, nr, True, nc - 1, True, count) == (E.CPK_ERR_DIM,) * 2
    assert both(2, None, nr, True, nc, True, count) == (E.CPK_ERR_ARGS,) * 2         # NULL pointers
    assert both(2, True, nr, None, nc, True, count) == (E.CPK_ERR_ARGS,) * 2
    assert both(2, True, nr, True, nc, None, count) == (E.CPK_ERR_ARGS,) * 2
    assert both(2, True, nr, True, nc, True, count, mat=None) == (E.CPK_ERR_ARGS,) * 2
    kind, ptr, ind, _, _ = raw("tiny65x63_B", "dup_csr")
    H = raw_matrix(kind, M.shape, ptr, ind, np.ones(count), ctx=None)                # a host-only matrix
    assert both(2, True, nr, True, nc, True, count, mat=H) == (E.CPK_ERR_ARGS,) * 2
    g = cpk.SimGroup(1)
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=g, options=dict(dist1=1))  # a one-rank sim context
    try:
        D = raw_matrix(kind, M.shape, ptr, ind, np.ones(count), ctx=ctx)
        assert both(2, True, nr, True, nc, True, count, mat=D) == (E.CPK_ERR_UNSUPPORTED,) * 2
        del D
    finally:
        ctx.close()
    gpu_ctx.synchronize()
    assert np.all(out == SENT) and np.all(dO.numpy() == SENT)
    # and the same arguments without a fault go through
    assert both(2, True, nr, True, nc, True, count) == (0, 0)
    gpu_ctx.synchronize()
    assert bits_equal(out[:count], reference(rows, cols, U, V, 1.0)) and bits_equal(dO.numpy()[:count], out[:count])
    assert out[count] == SENT and dO.numpy()[count] == SENT
