"""In-place value updates of a matrix handle (cpk_mat_set_values, cpk_mat_set_values_device,
cpk_mat_get_info, cpk_pc_solver_info) without a device: an interior-point outer iteration rebuilds
opLDL2 from new values of the same sparsity (reg_cpkrylov.m:131), and the handles take those values
in place.

  * the four entries exist with the header's signatures and the ABI version is unchanged;
  * every refusal that needs no device, each leaving the handle's info and a following analysis
    (cpk_analyze / cpk_analysis_export) exactly as they were;
  * on host-only matrices created from sorted CSR, unsorted CSR, CSR with duplicates (among them
    triples 1e16, w, -1e16 whose float sum depends on the order), CSC, explicit zeros, an empty
    matrix and 1 x 1: after set_values the exported factors equal those of handles freshly created
    from the same index arrays and the new values, bit for bit;
  * the values generation counts successful updates only."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib
from rawmat import duplicated_csr, raw_matrix, unsorted_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpk_mat_set_values", "cpk_mat_set_values_device", "cpk_mat_get_info", "cpk_pc_solver_info")
PD = C.POINTER(C.c_double)


def _ctype(param):
    """the ctypes type _SIGS must hold for one parameter of a declaration in cpk.h"""
    param = " ".join(param.split())
    name = re.search(r"(\w+)(\[\d*\])?$", param).group(1)
    pointer = "*" in param or param.endswith("]")
    if re.match(r"(const )?cpk_(mat|pc|ctx)\b", param):
        return C.c_void_p
    if "double" in param and pointer:
        return C.c_void_p if name.startswith("d_") else PD  # device pointers travel as void *
    if "int64_t" in param:
        return C.POINTER(C.c_int64) if pointer else C.c_int64
    raise AssertionError(f"unmapped parameter {param!r}")


def test_signatures_match_the_header():
    src = open(os.path.join(ROOT, "include", "cpk.h")).read()
    for n in NEW:
        m = re.search(r"^int\s+" + n + r"\s*\(([^)]*)\)\s*;", src, re.M)
        assert m, f"{n} is not declared in cpk.h"
        want = [_ctype(p) for p in m.group(1).split(",")]
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTED, n
        args, res = _lib._SIGS[n]
        assert res is C.c_int and args == want, (n, args, want)
    assert _lib.lib.cpk_abi_version() == 3


# ---- the systems: G (n x n, diagonal > 0), B (m x n, the case's kind), C22 (m x m, diagonal < 0) --
def _diag(v):
    n = len(v)
    return ("csr", (n, n), np.arange(n + 1), np.arange(n), np.asarray(v, dtype=np.float64))


def _sparse_b(m, n, rng, density=0.45):
    B = sp.random(m, n, density=density, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
    B.data = rng.uniform(0.3, 1.0, B.nnz) * np.where(rng.random(B.nnz) < 0.5, -1.0, 1.0)
    B.sum_duplicates()
    B.sort_indices()
    return B


def _case(name):
    """(G, B, C22) as (kind, shape, ptr, ind, val) and the three new value arrays, in the creating
    calls' order: seeded, the same sparsity, still factorable (G > 0 > C22 diagonal: Kp is
    quasi-definite whatever B holds)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    n, m = (1, 1) if name == "1x1" else (9, 0) if name == "zero_rows" else (9, 6)
    S = sp.csr_matrix(np.array([[0.7]])) if name == "1x1" else _sparse_b(m, n, rng) if m else sp.csr_matrix((0, n))
    v2 = S.data * rng.uniform(0.5, 2.0, S.nnz)
    if name in ("sorted_csr", "1x1", "zero_rows"):
        B, b2 = ("csr", (m, n), S.indptr, S.indices, S.data), v2
    elif name == "unsorted_csr":
        ptr, ind, order = unsorted_csr(S)
        B, b2 = ("csr", (m, n), ptr, ind, S.data[order]), v2[order]
    elif name == "duplicates":
        ptr, ind, split = duplicated_csr(S, rng)
        B, b2 = ("csr", (m, n), ptr, ind, split(S.data, np.random.default_rng(1))), split(v2, np.random.default_rng(2))
    elif name == "csc":
        T = S.tocsc()
        T.sort_indices()
        B, b2 = ("csc", (m, n), T.indptr, T.indices, T.data), T.data * rng.uniform(0.5, 2.0, T.nnz)
    elif name == "explicit_zeros":
        v1 = S.data.copy()
        v1[::3] = 0.0
        v2[1::4] = 0.0
        B, b2 = ("csr", (m, n), S.indptr, S.indices, v1), v2
    elif name == "empty":
        B, b2 = ("csr", (m, n), np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)), np.zeros(0)
    else:
        raise KeyError(name)
    G, Cn = _diag(rng.uniform(1.0, 3.0, n)), _diag(-rng.uniform(0.5, 1.5, m))
    return (G, B, Cn), (G[4] * rng.uniform(0.5, 2.0, n), b2, Cn[4] * rng.uniform(0.5, 2.0, m))


CASES = ("sorted_csr", "unsorted_csr", "duplicates", "csc", "explicit_zeros", "empty", "zero_rows", "1x1")


def _handles(mats, vals=None):
    return [raw_matrix(k, shape, ptr, ind, val if vals is None else vals[i]) for i, (k, shape, ptr, ind, val) in enumerate(mats)]


def _factors(hs):
    a = cpk.analyze(*hs)
    return a["perm"], a["L"].indptr, a["L"].indices, a["L"].data, a["D"]


def _same(f, g):
    return all(np.array_equal(x, y) for x, y in zip(f, g))


def test_duplicate_triples_depend_on_the_order():
    """the duplicates case does hold sums that another order changes: the check below is not vacuous"""
    assert (1e16 + 1.0) + -1e16 != (1e16 + -1e16) + 1.0
    (_, B, _), (_, b2, _) = _case("duplicates")
    assert np.sum(np.abs(B[4]) == 1e16) >= 2 and np.sum(np.abs(b2) == 1e16) >= 2


@pytest.mark.parametrize("name", CASES)
def test_set_values_equals_fresh_handles(name):
    mats, new = _case(name)
    hs = _handles(mats)
    before = _factors(hs)
    for h, v in zip(hs, new):
        assert h.info()["values_generation"] == 0 and h.info()["entries"] == len(v)
        h.set_values(v)
        assert h.info()["values_generation"] == 1
    after = _factors(hs)
    fresh = _factors(_handles(mats, new))
    assert _same(after, fresh)
    assert not np.array_equal(after[4], before[4])  # D changed: the update did reach the analysis
    # and back: the first values again give the first factors
    for h, m in zip(hs, mats):
        h.set_values(m[4])
    assert _same(_factors(hs), before)
    assert [h.info()["values_generation"] for h in hs] == [2, 2, 2]


def test_info_fields():
    mats, _ = _case("duplicates")
    B = _handles(mats)[1]
    i = B.info()
    assert (i["nrows"], i["ncols"]) == mats[1][1] and i["entries"] == len(mats[1][4]) and i["nnz"] < i["entries"]
    assert i["values_generation"] == 0 and i["device_copy"] is False and i["krylov_operators"] == 0
    assert _lib.lib.cpk_mat_get_info(None, (C.c_int64 * 8)()) == _lib.CPK_ERR_ARGS
    assert _lib.lib.cpk_mat_get_info(B.h, None) == _lib.CPK_ERR_ARGS
    assert _lib.lib.cpk_pc_solver_info(None, (C.c_int64 * 4)()) == _lib.CPK_ERR_ARGS


@pytest.mark.parametrize("name", ("duplicates", "csc", "sorted_csr"))
def test_refusals_leave_the_handle_untouched(name):
    L = _lib.lib
    mats, new = _case(name)
    hs = _handles(mats)
    B, v = hs[1], np.ascontiguousarray(new[1])
    cnt = len(v)
    longer = np.concatenate([v, [1.0]])
    infos, before = [h.info() for h in hs], _factors(hs)
    fake_dev = C.c_void_p(v.ctypes.data)  # stands for a device address; never dereferenced
    for rc, want in ((L.cpk_mat_set_values(None, v.ctypes.data_as(PD), cnt), _lib.CPK_ERR_ARGS),
                     (L.cpk_mat_set_values(B.h, None, cnt), _lib.CPK_ERR_ARGS),
                     (L.cpk_mat_set_values(B.h, longer.ctypes.data_as(PD), cnt + 1), _lib.CPK_ERR_DIM),
                     (L.cpk_mat_set_values(B.h, v.ctypes.data_as(PD), cnt - 1), _lib.CPK_ERR_DIM),
                     (L.cpk_mat_set_values(B.h, None, 0), _lib.CPK_ERR_DIM),
                     (L.cpk_mat_set_values_device(None, fake_dev, cnt), _lib.CPK_ERR_ARGS),
                     (L.cpk_mat_set_values_device(B.h, None, cnt), _lib.CPK_ERR_ARGS),
                     (L.cpk_mat_set_values_device(B.h, fake_dev, cnt + 1), _lib.CPK_ERR_DIM),
                     (L.cpk_mat_set_values_device(B.h, fake_dev, cnt), _lib.CPK_ERR_ARGS)):  # host-only matrix
        assert rc == want, (rc, want, L.cpk_last_error())
        assert [h.info() for h in hs] == infos
        assert _same(_factors(hs), before)
    with pytest.raises(cpk.CpkError) as e:
        B.set_values(longer)
    assert e.value.code == _lib.CPK_ERR_DIM
    with pytest.raises(cpk.CpkError) as e:
        B.set_values_device(v.ctypes.data, cnt)
    assert e.value.code == _lib.CPK_ERR_ARGS and "host-only" in str(e.value)
    assert [h.info() for h in hs] == infos and _same(_factors(hs), before)
    # the generation counts successes only
    B.set_values(v)
    assert B.info()["values_generation"] == 1
    assert _same(_factors(hs), _factors(_handles(mats, [mats[0][4], v, mats[2][4]])))


def test_empty_values_are_fine():
    """count == 0 with NULL values: a matrix without entries (C = 0) takes the update"""
    Z = cpk.Matrix(sp.csr_matrix((4, 4)), host_only=True)
    assert _lib.lib.cpk_mat_set_values(Z.h, None, 0) == _lib.CPK_OK
    Z.set_values(np.zeros(0))
    assert Z.info()["values_generation"] == 2 and Z.info()["entries"] == 0


def test_python_set_values_takes_a_sparse_matrix_of_the_same_pattern():
    rng = np.random.default_rng(3)
    S = _sparse_b(6, 9, rng)
    for csc in (False, True):
        M = cpk.Matrix(S, host_only=True, csc=csc)
        S2 = S.copy()
        S2.data = S.data * rng.uniform(0.5, 2.0, S.nnz)
        M.set_values(S2.tocoo())  # any format: canonicalised as the constructor does
        want = (S2.tocsc() if csc else S2).data
        assert np.array_equal(M._val, want) and M.info()["values_generation"] == 1
        T = S2.tolil()
        i, j = np.argwhere(S.toarray() == 0)[0]
        T[i, j] = 0.5
        with pytest.raises(cpk.CpkError) as e:
            M.set_values(T.tocsr())
        assert e.value.code == _lib.CPK_ERR_ARGS and M.info()["values_generation"] == 1
        with pytest.raises(cpk.CpkError) as e:
            M.set_values(sp.csr_matrix((6, 8)))
        assert e.value.code == _lib.CPK_ERR_ARGS
