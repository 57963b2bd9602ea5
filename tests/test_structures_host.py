"""The host half of the preconditioner and the distributed plans on the structure family
(tests/structures.py), no GPU: the checks of test_host_analysis.test_factor_and_schedule and the
numpy replays of test_dist_plan, on inputs whose structure forces the path -- whole-graph
orderings, a dense row, a dense clique, isolated nodes, C = 0, disconnected blocks and systems
smaller than one wave (ranks that own nothing)."""
import numpy as np
import pytest
import scipy.sparse as sp

import cpkrylov_amd as cpk
import structures as ST
from dist_emul import dist_spmv, halo_payload
from fixtures import EXPROG_OPTS
from oracle import oracle as O
from test_dist_plan import _apply_all, _global_rowsum, _plans
from test_host_analysis import replay

NAMES = list(ST.MEMBERS)
ORDERING = dict(band_g=4, band_g_nd=3)  # every other member: G first, minimum degree (2)


@pytest.mark.parametrize("name", NAMES)
def test_factor_and_schedule(name):
    S = ST.get(name)
    G, B, C22 = S["G"], S["B"], -S["C"]
    an = cpk.analyze(G, B, C22)
    N = an["info"]["N"]
    assert N == S["n"] + S["m"]
    assert an["info"]["ordering"] == ORDERING.get(name, 2)
    perm = an["perm"]
    assert np.array_equal(np.sort(perm), np.arange(N))  # P is a permutation (P*P' = I)
    Kp = ST.kp(S)
    L1 = an["L"] + sp.eye(N)
    R = Kp[perm][:, perm] - L1 @ sp.diags(an["D"]) @ L1.T
    scale = abs(L1) @ sp.diags(np.abs(an["D"])) @ abs(L1).T  # componentwise backward error
    assert abs(R).max() <= 1e-14 * max(abs(scale).max(), abs(Kp).max())
    # schedule covers every row once, rounds/blocks/levels consistent
    assert an["lvl_row"][0] >= 0 and an["lvl_row"][-1] == N
    assert np.all(np.diff(an["lvl_row"]) > 0)
    assert an["blk_lvl"][-1] == len(an["lvl_row"]) - 1
    x = np.random.default_rng(5).standard_normal(N)
    y = replay(an, x)
    Mo = O.LDL2(G, B, C22, factors=(an["L"], an["D"], perm))
    Mo.set(nitref=0)
    assert np.array_equal(y, Mo @ x)
    assert np.linalg.norm(Kp @ y - x) <= 1e-6 * np.linalg.norm(x)


def test_paths_by_structure():
    """What each member is for, read from the analysis: it holds for any pivot order."""
    info = {k: cpk.analyze(ST.get(k)["G"], ST.get(k)["B"], -ST.get(k)["C"]) for k in
            ("arrow_row", "dense_col", "empty_rows", "tiny1x1", "tiny2x1", "tiny3x2")}
    rows = np.diff(info["arrow_row"]["L"].tocsr().indptr)
    assert rows.max() > 3072  # above the largest LDS image of the upper rounds
    assert np.diff(ST.kp(ST.get("arrow_row")).indptr).max() == ST.get("arrow_row")["n"] + 1 > 2 * 2048
    assert info["dense_col"]["info"]["nrounds"] >= 10  # the 315-clique: a dense chain
    assert info["dense_col"]["info"]["nnz_l"] >= 315 * 314 // 2
    L = info["empty_rows"]["L"]
    lone = np.flatnonzero((np.diff(L.tocsr().indptr) == 0) & (np.diff(L.indptr) == 0))
    assert np.isin(ST.get("empty_rows")["n"] + np.arange(600, 630), info["empty_rows"]["perm"][lone]).all()
    # (tiny65x63's dense factor, 6048 entries, is more than one block stages: several rounds)
    for k in ("tiny1x1", "tiny2x1", "tiny3x2"):
        assert info[k]["info"]["nrounds"] == 1 and info[k]["info"]["nblocks"] == 1


def test_zero_c_needs_diagonal_g():
    """C = 0 works with G diagonal (the Schur complement B G^-1 B' is definite); with a
    non-diagonal G the whole-graph order meets a zero 1x1 pivot: the documented limit,
    reported as CPK_ERR_FACTOR."""
    S = ST.band_g_zero_c()
    with pytest.raises(cpk.CpkError) as e:
        cpk.analyze(S["G"], S["B"], -S["C"])
    assert e.value.code == 6


@pytest.mark.parametrize("name", ST.SOLVE_MEMBERS)
def test_oracle_solves_the_solve_members(name):
    """The cases of test_gpu_structures.test_exact_solve_bitexact are ones the reference itself
    solves (exact mode, the host factors): one or two iterations on the tiny members, 7 on
    band_g and 11 on arrow_row, with every method."""
    S = ST.get(name)
    an = cpk.analyze(S["G"], S["B"], -S["C"])
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=(an["L"], an["D"], an["perm"]))
    Mo.set(nitref=1.0, itref_tol=1e-8, force_itref=1.0, residual_update=1.0)
    want = {"band_g": (7, 7), "arrow_row": (11, 11)}.get(name, (1, 2))
    for method, extra in ST.SOLVE_METHODS:
        with O.exact():
            _, so = O.reg_solve(method, S["rhs"], S["Q"], S["B"], S["C"], Mo, dict(EXPROG_OPTS, **extra))
        assert so["solved"] and want[0] <= so["niters"] <= want[1], (method, so["niters"])


def test_oracle_raises_on_tiny_indefinite():
    """... and ST.tiny_indefinite() is a system on which every method of the reference stops with
    its indefinite / complex-norm error (test_gpu_structures.test_exact_solve_raises_as_the_reference)."""
    S = ST.tiny_indefinite()
    an = cpk.analyze(S["G"], S["B"], -S["C"])
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=(an["L"], an["D"], an["perm"]))
    Mo.set(nitref=1.0, itref_tol=1e-8, force_itref=1.0, residual_update=1.0)
    for method, extra in ST.SOLVE_METHODS:
        with pytest.raises(O.OracleError) as e, O.exact():
            O.reg_solve(method, S["rhs"], S["Q"], S["B"], S["C"], Mo, dict(EXPROG_OPTS, **extra))
        assert e.value.code == 1 and "Iter" in e.value.msg, (method, e.value.msg)


@pytest.mark.parametrize("P", [2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_distributed_apply_bitexact(name, P):
    S = ST.get(name)
    Q, B, Cm, G = S["Q"], S["B"], S["C"], S["G"]
    plans = _plans(Q, B, Cm, G, P)
    n, N = plans[0]["n"], plans[0]["N"]
    allg = np.concatenate([p["dofs"] for p in plans])
    assert np.array_equal(np.sort(allg), np.arange(N))
    for p in plans:
        assert np.all(p["dofs"][:p["n_loc"]] < n) and np.all(p["dofs"][p["n_loc"]:] >= n)
    an = cpk.analyze(G, B, -Cm)
    Mo = O.LDL2(G, B, -Cm, factors=(an["L"], an["D"], an["perm"]))
    Mo.set(nitref=0)
    x = np.random.default_rng(P).standard_normal(N)
    for negate in (False, True):
        xs = [x[p["dofs"]] for p in plans]
        negs = [p["n_loc"] if negate else p["N_loc"] for p in plans]
        ys = _apply_all(plans, xs, negs)
        y = np.empty(N)
        for p, yl in zip(plans, ys):
            y[p["dofs"]] = yl
        xin = np.concatenate([x[:n], -x[n:]]) if negate else x
        assert np.array_equal(y, Mo @ xin), f"{name} P={P} negate={negate}"


@pytest.mark.parametrize("P", [2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_distributed_spmv_bitexact(name, P):
    S = ST.get(name)
    Q, B, Cm, G = S["Q"], S["B"], S["C"], S["G"]
    plans = _plans(Q, B, Cm, G, P)
    n, N = plans[0]["n"], plans[0]["N"]
    AC = sp.block_diag([Q, Cm]).tocsr()
    AB = sp.hstack([Q, B.T]).tocsr()
    x = np.random.default_rng(11).standard_normal(N)
    for kind, K, rows in (("kp", ST.kp(S), N), ("ac", AC, N), ("ab", AB, n)):
        ref = _global_rowsum(K, x)
        xs = [x[p["dofs"]] for p in plans]
        recv = np.concatenate([halo_payload(p, kind, xl) for p, xl in zip(plans, xs)])
        got = np.empty(rows)
        for p, xl in zip(plans, xs):
            yl = dist_spmv(p, kind, xl, recv)
            got[p["dofs"][:len(yl)]] = yl
        assert np.array_equal(got, ref), kind
