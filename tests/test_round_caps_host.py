"""Per-round block caps of the sweep schedule (engine option round_caps), checked on the CPU.

round_caps = 0 is the uniform schedule; 1 (the default) gives the rounds above round 1 the largest
cap of a ladder derived from the LDS limit whose blocks stay resident, for a tree whose round 1 is
wider than the device holds at once; N > 1 puts every round above round 1 at N entries (what the
small systems here use).  Round 1 keeps 512 rows / 3072 entries, a tall round holds at most 128
rows per block.  Systems: the 60 000-dof +-64 system (seed 5), the same generator at 250 000 and
1.5 M dofs (a top deep enough for fewer rounds; a round 1 of more than 1024 blocks), and the
structure family."""
import hashlib
import json
import os

import numpy as np
import pytest

import cpkrylov_amd as cpk
import structures
from cpkrylov_amd.synthetic import saddle_system

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "round_caps_uniform_schedule.json")
DEFAULT_SWEEP = "192,576,64,512,3072,256,480"
NAMES = ["w64"] + sorted(structures.MEMBERS)
_SYS = {}


def _system(name):
    if name not in _SYS:
        _SYS[name] = saddle_system(N=int(name[4:] or 60000), window=64, seed=5) if name.startswith("w64") else structures.get(name)
    return _SYS[name]


def _analyze(name, **opts):
    S = _system(name)
    return cpk.analyze(S["G"], S["B"], -S["C"], options=opts)


def _sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def _blocks(a):
    """per block: round, rows, forward and backward entries; and the block of every schedule row"""
    rp, brow, order = a["round_ptr"], a["lvl_row"][a["blk_lvl"]], a["order"]
    L = a["L"].tocsc()
    fwd, bwd = np.diff(L.tocsr().indptr)[order], np.diff(L.indptr)[order]
    cf, cb = np.concatenate([[0], np.cumsum(fwd)]), np.concatenate([[0], np.cumsum(bwd)])
    nb = len(brow) - 1
    rnd = np.searchsorted(rp, np.arange(nb), side="right") - 1
    return rnd, np.diff(brow), cf[brow[1:]] - cf[brow[:-1]], cb[brow[1:]] - cb[brow[:-1]], brow


@pytest.mark.parametrize("name", NAMES)
def test_option_off_is_the_uniform_schedule(name):
    """round_caps = 0: round_ptr and the order recorded from the schedule before per-round caps
    existed (tests/golden/round_caps_uniform_schedule.json); the default leaves these systems --
    a round 1 the device holds at once -- as they are, and so does an explicit sweep"""
    g = json.load(open(GOLDEN))[name]
    for opts in (dict(round_caps=0), dict(), dict(sweep=DEFAULT_SWEEP, round_caps=7000)):
        a = _analyze(name, **opts)
        assert a["round_ptr"].tolist() == g["round_ptr"], opts
        assert _sha(a["order"], np.int32) == g["order_sha256"], opts
        assert np.all(a["round_cap"][1:] == 3072) and np.all(a["round_rows"][1:] == 512)
        assert a["round_cap"][0] == 576 and a["round_rows"][0] == 192


@pytest.mark.parametrize("name,caps", [(n, c) for n in NAMES + ["w64_250000"] for c in (3100, 7000, 16384)])
def test_forced_caps_give_a_valid_schedule(name, caps):
    a0, a = _analyze(name, round_caps=0), _analyze(name, round_caps=caps)
    rnd, rows, fe, be, brow = _blocks(a)
    R = len(a["round_ptr"]) - 1
    top = min(caps, 15651)  # the ladder's top: one image of 512 + 1 rows within 160 KB less 64 bytes
    if R > 2 and np.all(a["round_cap"][1:] == 3072):
        # a chain-like tree (the peeling gives up and the bottom-up clustering takes over: arrow_row's
        # and dense_col's kind): the whole schedule keeps uniform caps
        assert name in ("arrow_row", "dense_col", "band_g", "band_g_nd", "blocks8", "empty_rows", "zero_c"), name
        assert np.array_equal(a["round_ptr"], a0["round_ptr"]) and np.array_equal(a["order"], a0["order"])
    else:
        assert a["round_cap"].tolist() == [576, 3072][:R] + [top] * max(R - 2, 0)
        assert a["round_rows"].tolist() == [192, 512][:R] + [128] * max(R - 2, 0)
    # every block within its round's rows and entries, both directions (a single row may exceed
    # any cap: arrow_row's dense row is a block of its own, on the kernels' direct path)
    cap, lim = a["round_cap"][rnd], a["round_rows"][rnd]
    one = rows == 1
    assert np.all(rows <= lim) and np.all((fe <= cap) | one) and np.all((be <= cap) | one)
    # every entry's column lies in the row's block or an earlier one: L's entry (i, j), i > j in the
    # pivot order, is a forward term of row i on column j
    n = len(a["order"])
    pos = np.empty(n, np.int64)
    pos[a["order"]] = np.arange(n)
    blk = np.searchsorted(brow, np.arange(n), side="right") - 1
    L = a["L"].tocoo()
    assert np.all(blk[pos[L.col]] <= blk[pos[L.row]])
    assert np.all(rnd[blk[pos[L.col]]] <= rnd[blk[pos[L.row]]])
    same_round = rnd[blk[pos[L.col]]] == rnd[blk[pos[L.row]]]
    assert np.all(blk[pos[L.col]][same_round] == blk[pos[L.row]][same_round])  # a round's blocks are independent
    # never more rounds; the pivot order and the factor are the option-off ones
    assert R <= len(a0["round_ptr"]) - 1
    assert np.array_equal(a["perm"], a0["perm"]) and (a["L"] != a0["L"]).nnz == 0
    # the block kernels' int16 fields: entry offsets (S.p, S.ps, the fold counts) and local rows
    multi = ~one
    assert np.all(fe[multi] <= np.iinfo(np.int16).max) and np.all(be[multi] <= np.iinfo(np.int16).max)


def test_fewer_rounds_where_the_top_is_deep():
    """250 000 dofs: 8 rounds with uniform caps; the forced ladder top folds the narrow top's
    stack of 16-row blocks into fewer, taller rounds.  (The 60 000-dof system's top holds 192 rows in
    three blocks of at most 3019 entries: the 128-row limit, not the entry cap, is what cuts it, and
    its round count stays 4.)"""
    r0 = len(_analyze("w64_250000", round_caps=0)["round_ptr"]) - 1
    r1 = len(_analyze("w64_250000", round_caps=16384)["round_ptr"]) - 1
    assert r1 < r0 and r0 >= 8
    assert len(_analyze("w64", round_caps=16384)["round_ptr"]) == len(_analyze("w64", round_caps=0)["round_ptr"])


def test_default_ladder_on_a_wide_round1():
    """1.5 M dofs: round 1 has more than 1024 blocks (four 38 KB images on each of 256 CUs), so the
    default applies the ladder: fewer rounds, round 1 untouched, every tall round's blocks within
    the residency its cap allows (256 CUs x images of that cap in 160 KB less 64 bytes)"""
    a0, a1 = _analyze("w64_1500000", round_caps=0), _analyze("w64_1500000")
    rp0, rp1 = a0["round_ptr"], a1["round_ptr"]
    assert rp0[2] - rp0[1] > 1024 and rp1[:3].tolist() == rp0[:3].tolist()
    assert len(rp1) < len(rp0)
    cap, rows = a1["round_cap"], a1["round_rows"]
    assert cap[1] == 3072 and rows[1] == 512 and np.all(cap[2:] >= 3072) and cap[-1] == 15651
    assert np.all(np.diff(cap[2:]) >= 0)  # the rounds narrow going up, so their caps grow
    for r in range(2, len(cap)):
        if cap[r] > 3072:
            image = (8 * 513 + 10 * (int(cap[r]) + 8) + 6 * 513 + 15) & ~15
            assert rows[r] == 128 and rp1[r + 1] - rp1[r] <= 256 * ((160 * 1024 - 64) // image)
    rnd, nrows, fe, be, _ = _blocks(a1)
    assert np.all(nrows <= rows[rnd]) and np.all(fe <= cap[rnd]) and np.all(be <= cap[rnd])
    assert np.any(fe > 3072) and np.any(fe > 6144)


@pytest.mark.parametrize("name", ["w64", "dense_col"])
def test_rowspan_eligibility_refuses_what_does_not_fit(name):
    """The row-span layouts of a forced-cap schedule: a block of more than 128 rows, an image over
    its round's cap or a table over 2048 bytes is refused, never truncated; an eligible block's
    slots fit int16 and its image its round's entries"""
    S = _system(name)
    a = _analyze(name, round_caps=7000)
    rp, cap = a["round_ptr"], a["round_cap"]
    tall = 0
    for r in cpk.rowspan_layouts(S["G"], S["B"], -S["C"], options=dict(round_caps=7000)):
        rnd = int(np.searchsorted(rp, r["block"], side="right")) - 1
        if r["nr"] > 128:
            assert not r["eligible"]
        if r["eligible"]:
            assert r["slots"] <= np.iinfo(np.int16).max and r["ndr"] * r["nrp"] <= 2048
            assert 8 * r["slots"] + r["ndr"] * r["nrp"] <= 10 * (int(cap[rnd]) + 8)
            assert r["dest"].max(initial=0) < r["slots"] and np.all(r["tab"] <= 255)
            tall += rnd >= 2
    assert tall > 0
    # a small image refuses every block over it, in the tall rounds too
    for r in cpk.rowspan_layouts(S["G"], S["B"], -S["C"], options=dict(round_caps=7000), cap_entries=64):
        if r["eligible"]:
            assert 8 * r["slots"] + r["ndr"] * r["nrp"] <= 10 * (64 + 8)


def test_distributed_plan_is_unchanged():
    """The distributed preconditioner schedules each rank's subtrees with uniform caps: its plan
    does not depend on the option"""
    S = _system("w64")
    plans = [cpk.dist_plan(S["G"], S["B"], -S["C"], S["Q"], S["C"], 4, 1, options=dict(round_caps=c)) for c in (0, 1, 7000)]
    for p in plans[1:]:
        assert p.keys() == plans[0].keys()
        for k, v in plans[0].items():
            assert np.array_equal(np.asarray(v), np.asarray(p[k])), k


def test_option_value_is_checked_and_reported():
    S = structures.get("tiny3x2")
    for bad in ("-1", "16385", "x"):
        with pytest.raises(cpk.CpkError):
            cpk.analyze(S["G"], S["B"], -S["C"], options=f"round_caps={bad}")
