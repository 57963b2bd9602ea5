"""Per-round block caps (engine option round_caps) on the GPU: tall blocks staged in chunks.

A round above round 1 may hold blocks of more entries than the block kernels stage in one pass
(12 x 256 = 3072 for the round and chain kernels, 8 x 512 = 4096 for the fused last round's own
launch); the staging then loops over chunks into one LDS image.  Rows keep their terms and their
order, so M*z with forced refinement and the bare LDL' apply must equal the oracle's on the
exported factors exactly (np.array_equal), and a cpminres solve must repeat the option-off solve.

Systems: the 60 000-dof +-64 system (seed 5) and hub_system, 100 constraints coupled densely
through C (a separator clique) over 60 private variables each (the leaves).  The caps are forced
(round_caps = N puts every round above round 1 at N entries), and extra leaves on one constraint
move one block's entry count by one each, which gives blocks of exactly 3071, 3072 and 3073
entries, in a middle round (upper_block) and in the last (last_block), and blocks of more than
6144.  The host analysis states the counts; the tests assert them before they run the GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from fixtures import EXPROG_OPTS
from cpkrylov_amd.synthetic import saddle_system
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_CACHE = {}
FORCED = dict(nitref=1, force_itref=True)
LOOPS = [{}, {"no_chain": 1}, {"all_rowspan": 1}, {"all_colsweep": 1}, {"all_dataflow": 1, "no_colsweep": 1},
         {"no_dataflow": 1}, {"all_rowspan": 1, "no_chain": 1}]


def hub_system(extra=0, which=99, hubs=100, leaves=60, seed=3):
    key = ("hub", extra, which)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        d = np.full(hubs, leaves)
        d[which] += extra
        n = int(d.sum())
        G = sp.diags(rng.uniform(1.0, 2.0, n), 0, format="csr")
        B = sp.csr_matrix((rng.uniform(1 / 3, 1.0, n) * rng.choice([-1.0, 1.0], n), (np.repeat(np.arange(hubs), d), np.arange(n))),
                          shape=(hubs, n))
        R = 0.01 * rng.uniform(-1.0, 1.0, (hubs, hubs))
        C = sp.csr_matrix(R @ R.T + np.eye(hubs))
        rhs = rng.standard_normal(n + hubs)
        _CACHE[key] = dict(G=G, Q=G, B=B, C=C, n=n, m=hubs, rhs=rhs)
    return _CACHE[key]


def _w64():
    if "w64" not in _CACHE:
        _CACHE["w64"] = saddle_system(N=60000, window=64, seed=5)
    return _CACHE["w64"]


def block_entries(S, **opts):
    """[(round, rows, forward entries, backward entries)] of the upper rounds' blocks (host analysis)"""
    import cpkrylov_amd as cpk
    a = cpk.analyze(S["G"], S["B"], -S["C"], options=opts)
    rp, brow, order = a["round_ptr"], a["lvl_row"][a["blk_lvl"]], a["order"]
    L = a["L"].tocsc()
    fwd, bwd = np.diff(L.tocsr().indptr)[order], np.diff(L.indptr)[order]
    return [(r, int(brow[b + 1] - brow[b]), int(fwd[brow[b]:brow[b + 1]].sum()), int(bwd[brow[b]:brow[b + 1]].sum()))
            for r in range(1, len(rp) - 1) for b in range(rp[r], rp[r + 1])]


def _check_applies(S, opts, seed=71, multi=True):
    """M*z with forced refinement, the bare LDL' apply (one column and a panel of three) twice
    each, against the oracle on the exported factors"""
    import cpkrylov_amd as cpk
    with cpk.engine_options(**opts):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=M.export_factors())
    rng = np.random.default_rng(seed)
    z, Z = rng.standard_normal(M.n), rng.standard_normal((M.n, 3))
    Mo.set(nitref=0.0)
    yo = Mo @ z
    for _ in range(2):  # repeated applies: the chain's epochs, the image reused
        assert np.array_equal(M.H * z, yo)
    if multi:
        assert np.array_equal(M.H @ Z, np.column_stack([Mo @ Z[:, j] for j in range(3)]))
    for k, v in FORCED.items():
        setattr(M, k, v)
    Mo.set(**{k: float(v) for k, v in FORCED.items()})
    yo = Mo @ z
    for _ in range(2):
        assert np.array_equal(M * z, yo)
    return M


@pytest.mark.parametrize("extra", [33, 34, 35])
def test_middle_round_block_at_one_chunk(gpu_ctx, extra):
    """round 2's block (upper_block, in the chain and in a launch of its own) holds 3071, 3072 and
    3073 forward entries: one chunk, exactly one chunk, one entry into the second"""
    S = hub_system(extra, which=40)
    be = block_entries(S, round_caps=3100)
    assert [b[2] for b in be if b[0] == 2] == [3038 + extra] and len({b[0] for b in be}) >= 3, be
    for mode in ({}, {"no_chain": 1}):
        _check_applies(S, dict(mode, round_caps=3100), multi=not mode)


@pytest.mark.parametrize("extra", [81, 82, 83])
def test_last_round_block_at_one_chunk(gpu_ctx, extra):
    """the last round's block (last_block: the chain's, 3072 entries a chunk, and the fused launch's
    own, 4096) holds 3071, 3072 and 3073 forward entries behind a round-2 block of 5265 (two chunks)"""
    S = hub_system(extra, which=99)
    be = block_entries(S, round_caps=5300)
    assert [b[2] for b in be] == [2635, 5265, 2990 + extra], be
    for mode in ({}, {"no_chain": 1}, {"no_chain": 1, "no_fuse_last": 1}):
        _check_applies(S, dict(mode, round_caps=5300), multi=False)


@pytest.mark.parametrize("caps,want", [(7000, 6860), (16384, 8255)])
@pytest.mark.parametrize("mode", LOOPS, ids=lambda m: "+".join(m) or "model")
def test_three_chunks_every_loop(gpu_ctx, caps, want, mode):
    """blocks of more than 6144 entries (three chunks): 6860 in a middle round, 8255 in the last
    (the fused last round over more than one chunk), on every level loop, chained and per round"""
    import cpkrylov_amd as cpk
    S = hub_system()
    be = block_entries(S, round_caps=caps)
    assert max(b[2] for b in be) == want > 6144 and max(b[1] for b in be if b[0] >= 2) <= 128, be
    M = _check_applies(S, dict(mode, round_caps=caps), multi=not mode)
    mo = M.block_model()
    tall = mo[:, 2] > 34  # the tall rounds' blocks hold more rows than round 1's
    if mode == {"all_rowspan": 1}:
        assert np.all(mo[tall & (mo[:, 8] == 1), 7] == 4)
    if mode == {"no_dataflow": 1}:
        assert not np.any(mo[:, 7] == 1)
    with cpk.engine_options(round_caps=0):  # the option off: the same bits from the uniform schedule
        M0 = cpk.opLDL2(S["G"], S["B"], -S["C"])
    z = np.random.default_rng(5).standard_normal(M.n)
    assert np.array_equal(M.H * z, M0.H * z)


@pytest.mark.parametrize("mode", [{}, {"no_chain": 1}, {"all_rowspan": 1}, {"all_colsweep": 1}, {"chain_wide": 2 ** 24}],
                         ids=lambda m: "+".join(m) or "model")
def test_w64_forced_caps(gpu_ctx, mode):
    """The 60 000-dof +-64 system with every round above round 1 at 7000 entries: round 1 keeps its
    blocks of up to 168 rows (two rows per lane), the tall rounds hold at most 128 (one and two
    rows per lane of the wave-wide loops)"""
    S = _w64()
    be = block_entries(S, round_caps=7000)
    assert max(b[1] for b in be if b[0] == 1) > 128 and max(b[1] for b in be if b[0] >= 2) <= 128
    assert any(64 < b[1] for b in be if b[0] >= 2) and any(b[1] <= 64 for b in be if b[0] >= 2)
    _check_applies(S, dict(mode, round_caps=7000), multi=not mode)


@pytest.mark.parametrize("which", ["hub", "w64"])
def test_cpminres_repeats_the_option_off_solve(gpu_ctx, which):
    """cpminres with forced caps: the iteration count and every history entry of the option-off
    solve, and the same x"""
    import cpkrylov_amd as cpk
    S = hub_system() if which == "hub" else _w64()
    opts = dict(EXPROG_OPTS)
    out = []
    for caps in (0, 16384 if which == "hub" else 7000):
        with cpk.engine_options(round_caps=caps):
            x, stats, flag = cpk.reg_cpkrylov(cpk.cpminres, S["rhs"], S["Q"], S["B"], S["C"], S["G"], opts)
        out.append((x, stats["niters"], np.asarray(stats["residHistory"]), bool(flag["solved"])))
    (x0, n0, h0, s0), (x1, n1, h1, s1) = out
    assert n0 == n1 and s0 == s1 and np.array_equal(h0, h1) and np.array_equal(x0, x1)
