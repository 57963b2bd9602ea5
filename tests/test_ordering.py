"""The minimum-degree ordering (csrc/ordering.cpp min_degree) against a plain set-based minimum
degree: exact degrees in the elimination graph, ties broken by the lowest index.  The product's
pivot order must EQUAL the reference's -- every other test takes the product's own perm, so a
wrong ordering (still a permutation) would pass them all.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import cpkrylov_amd as cpk
import fixtures as F
import structures as ST
from cpkrylov_amd.synthetic import saddle_system


def min_degree_reference(A):
    """Eliminate the node of least degree (lowest index among equals); its neighbours become a
    clique."""
    A = sp.csr_matrix(A)
    nv = A.shape[0]
    adj = [set(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist()) - {i} for i in range(nv)]
    deg = np.array([len(a) for a in adj], dtype=np.int64)
    order = []
    for _ in range(nv):
        v = int(np.argmin(deg))  # the first of the minima
        order.append(v)
        nb = adj[v]
        for u in nb:
            adj[u] |= nb
            adj[u] -= {u, v}
            deg[u] = len(adj[u])
        adj[v] = set()
        deg[v] = nv + 1  # eliminated
    return np.array(order)


def _pattern(M):
    M = sp.csr_matrix(M).copy()
    M.data[:] = 1.0
    return M


def _check(G, B, C):
    """G diagonal: the Schur-complement graph C + B*B' of the constraint block, after the G
    block; otherwise the whole graph of Kp."""
    an = cpk.analyze(G, B, -C)
    n, m = G.shape[0], B.shape[0]
    perm = an["perm"]
    if an["info"]["ordering"] == 2:
        assert np.array_equal(perm[:n], np.arange(n))
        S = _pattern(C) + _pattern(B) @ _pattern(B).T
        assert np.array_equal(perm[n:] - n, min_degree_reference(S))
    else:
        assert an["info"]["ordering"] == 4
        Kp = sp.bmat([[_pattern(G), _pattern(B).T], [_pattern(B), _pattern(C)]])
        assert np.array_equal(perm, min_degree_reference(Kp))
    return an


@pytest.mark.parametrize("name", ["cvxqp1_m", "cvxqp2_s"])
def test_min_degree_examples(name):
    P = F.load(name)
    _check(P["G"], P["B"], P["C"])


def test_min_degree_synthetic3k():
    S = saddle_system(N=3000)
    _check(S["G"], S["B"], S["C"])


def test_min_degree_band_g():
    S = ST.get("band_g")
    _check(S["G"], S["B"], S["C"])


def _graph_system(edges, nv):
    """A system whose Schur-complement graph is the given graph: C carries it (diagonally
    dominant), and B = e_1 e_1' adds no edge."""
    r, c = np.array(edges).T
    A = sp.coo_matrix((np.full(len(r), -1.0), (r, c)), shape=(nv, nv))
    A = A + A.T
    C = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)).tocsr()
    B = sp.csr_matrix(([1.0], ([0], [0])), shape=(nv, 1))
    return sp.identity(1, format="csr"), B, C


# star: hub 0, leaves 1..6.  The first leaf's elimination updates the hub; the second update of
# the hub is where a mark left by the first would drop the hub's live leaves.
STAR = [(0, k) for k in range(1, 7)]
GRAPHS = {"star": (STAR, 7),
          "star_hub_last": ([(6, k) for k in range(6)], 7),
          "star_plus_path": (STAR + [(6, 7), (7, 8), (8, 9), (9, 10)], 11),
          "star_and_path": (STAR + [(7, 8), (8, 9), (9, 10)], 11)}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_min_degree_star_and_path(name):
    edges, nv = GRAPHS[name]
    G, B, C = _graph_system(edges, nv)
    an = _check(G, B, C)
    assert an["info"]["nnz_l"] == len(edges) + 1  # a tree: minimum degree leaves no fill (+ B's entry)


def test_fill_guard_cvxqp1_m():
    """The reference order's fill is 13 743 entries; the bound allows for other tie-breaking."""
    P = F.load("cvxqp1_m")
    assert cpk.analyze(P["G"], P["B"], -P["C"])["info"]["nnz_l"] <= 15000


def test_fill_guard_arrow_row():
    """One dense constraint: eliminated last it costs one dense factor row and nothing else."""
    S = ST.get("arrow_row")
    info = cpk.analyze(S["G"], S["B"], -S["C"])["info"]
    assert info["nnz_l"] <= 2 * info["nnz_kp"], info
