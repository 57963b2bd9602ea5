"""Matrix handles created from raw index arrays, as a C caller would hand them over: unsorted
columns, duplicate entries and CSC input, none of which `cpk.Matrix` passes down (it canonicalises
with scipy first).  Test infrastructure for the value-update tests (a plain module)."""
import ctypes as C

import numpy as np

import cpkrylov_amd as cpk
from cpkrylov_amd import _lib

_P = C.POINTER


def raw_matrix(kind, shape, ptr, ind, val, ctx=None):
    """A `cpk.Matrix` around cpk_mat_create_csr (kind "csr") or cpk_mat_create_csc ("csc") on the
    arrays exactly as given; ctx None: host-only.  `set_values` then takes values in the order of
    `val`."""
    M = cpk.Matrix.__new__(cpk.Matrix)
    M.ctx, M.shape, M._csc = ctx, tuple(shape), kind == "csc"
    M._val = np.ascontiguousarray(val, dtype=np.float64)
    h = C.c_void_p()
    cx = ctx.h if ctx is not None else None
    pv = M._val.ctypes.data_as(_P(C.c_double)) if M._val.size else None
    if kind == "csc":
        M._ptr = np.ascontiguousarray(ptr, dtype=np.uintp)
        M._ind = np.ascontiguousarray(ind, dtype=np.uintp)
        rc = _lib.lib.cpk_mat_create_csc(cx, shape[0], shape[1], M._ptr.ctypes.data_as(_P(C.c_size_t)),
                                         M._ind.ctypes.data_as(_P(C.c_size_t)) if M._ind.size else None, pv, C.byref(h))
    else:
        M._ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        M._ind = np.ascontiguousarray(ind, dtype=np.int32)
        rc = _lib.lib.cpk_mat_create_csr(cx, shape[0], shape[1], M._ptr.ctypes.data_as(_P(C.c_int64)),
                                         M._ind.ctypes.data_as(_P(C.c_int32)) if M._ind.size else None, pv, C.byref(h))
    _lib.check(rc)
    M.h = h
    return M


def unsorted_csr(S):
    """(ptr, ind, entry order) of the canonical scipy CSR matrix S with every row's entries
    reversed: values in this order are S.data[order]"""
    order = np.concatenate([np.arange(S.indptr[i], S.indptr[i + 1])[::-1] for i in range(S.shape[0])] +
                           [np.zeros(0, np.int64)]).astype(np.int64)
    return S.indptr.astype(np.int64), S.indices[order].astype(np.int32), order


def duplicated_csr(S, rng):
    """(ptr, ind, split) of the canonical scipy CSR matrix S with every third entry given three
    times (beside each other or not, rows shuffled): split(v) spreads values v of S's entries over
    the raw entries so that they sum back to v up to rounding -- the triples as (1e16, w, -1e16)
    in a seeded order, whose float sum depends on that order"""
    ptr, ind, owner, role = [0], [], [], []
    for i in range(S.shape[0]):
        ents = []
        for p in range(S.indptr[i], S.indptr[i + 1]):
            for r in ((0, 1, 2) if p % 3 == 0 else (0,)):
                ents.append((S.indices[p], p, r if p % 3 == 0 else -1))
        ents = [ents[k] for k in rng.permutation(len(ents))]
        ind += [e[0] for e in ents]
        owner += [e[1] for e in ents]
        role += [e[2] for e in ents]
        ptr.append(len(ind))
    owner, role = np.array(owner, np.int64), np.array(role, np.int64)

    def split(v, srng):
        out = np.asarray(v, dtype=np.float64)[owner].copy() if owner.size else np.zeros(0)
        for p in np.unique(owner[role >= 0]):
            slots = np.flatnonzero(owner == p)  # in raw order: the order they are summed in
            out[slots] = np.array([1e16, v[p], -1e16])[srng.permutation(3)]
        return out

    return np.array(ptr, np.int64), np.array(ind, np.int32), split
