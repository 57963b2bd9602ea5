"""The upper rounds' row-span level loop (levels_rowspan) on the GPU: every way the oracle's bits.

The loop keeps each row's terms and their order -- a row's in-block values stored dense by step,
a register mask saying which steps it has, the outside runs drained at the layout's steps -- so
M*z must equal the oracle's LDL2 on the exported factors exactly (np.array_equal), forced on every
eligible block (all_rowspan), off (no_rowspan) and where the host model picks it."""
import numpy as np
import pytest

import structures
from cpkrylov_amd.synthetic import saddle_system
from oracle import oracle as O
from test_gpu_dist import _run_ranks

pytestmark = pytest.mark.gpu

_W64 = {}
PROPS = [dict(nitref=0), dict(nitref=1, force_itref=True), dict(nitref=2, force_itref=False, itref_tol=1e-30)]
MODES = [{}, {"all_rowspan": 1}, {"all_rowspan": 1, "no_chain": 1}, {"all_rowspan": 1, "chain_wide": 2 ** 24},
         {"no_rowspan": 1}]


def _w64():
    if "s" not in _W64:
        _W64["s"] = saddle_system(N=60000, window=64, seed=5)
    return _W64["s"]


def _oracle(G, B, C, M, props):
    L, D, perm = M.export_factors()
    Mo = O.LDL2(G, B, -C, factors=(L, D, perm))
    Mo.set(**{k: float(v) for k, v in props.items()})
    return Mo


@pytest.mark.parametrize("props", PROPS)
@pytest.mark.parametrize("sweep", ["", "64,192,64,128,512,512"])
def test_rowspan_modes_w64(gpu_ctx, sweep, props):
    """The 60 000-dof +-64 system: blocks of up to 168 rows in the first upper round, so one and
    two rows per lane, forward runs, and blocks the loop must refuse; chained and per round."""
    import cpkrylov_amd as cpk
    S = _w64()
    G, B, C = S["G"], S["B"], S["C"]
    z = np.random.default_rng(37).standard_normal(G.shape[0] + B.shape[0])
    ys = []
    for mode in MODES:
        opts = dict(mode)
        if sweep:
            opts["sweep"] = sweep
        with cpk.engine_options(**opts):
            M = cpk.opLDL2(G, B, -C)
        for k, v in props.items():
            setattr(M, k, v)
        ys.append(M * z)
        mo = M.block_model()
        if mode == {"all_rowspan": 1}:
            for d in (0, 1):
                assert np.any((mo[:, 1] == d) & (mo[:, 7] == 4)), "no block on the row-span loop"
            big = mo[:, 2] > 128
            if not sweep:  # the default blocks: some hold more than 128 rows
                assert np.any(big)
            assert not np.any(big & (mo[:, 7] == 4)) and np.all(mo[big, 8] == 0)
        if mode == {"no_rowspan": 1}:
            assert not np.any(mo[:, 7] == 4)
    yo = _oracle(G, B, C, M, props) @ z
    for y in ys:
        assert np.array_equal(y, yo)


@pytest.mark.parametrize("mode,loops", [({"all_colsweep": 1}, (2, 3)), ({"all_dataflow": 1, "no_colsweep": 1}, (1,)),
                                        ({"all_colsweep": 1, "no_rowspan": 1}, (2, 3)),
                                        ({"all_colsweep": 1, "all_rowspan": 1}, (4,))])
def test_forced_loops_stay_forced(gpu_ctx, mode, loops):
    """all_colsweep and all_dataflow keep their loop on the blocks they force: the model's pick of
    the row-span loop does not displace them (the older tests of those loops rely on it), only
    all_rowspan does.  Every way the oracle's bits."""
    import cpkrylov_amd as cpk
    S = _w64()
    G, B, C = S["G"], S["B"], S["C"]
    z = np.random.default_rng(59).standard_normal(G.shape[0] + B.shape[0])
    with cpk.engine_options(**mode):
        M = cpk.opLDL2(G, B, -C)
    props = dict(nitref=1, force_itref=True)
    for k, v in props.items():
        setattr(M, k, v)
    mo = M.block_model()
    if loops == (4,):
        el = mo[:, 8] == 1
        assert np.any(el) and np.all(mo[el, 7] == 4)
    elif loops == (1,):
        assert np.all(mo[:, 7] == 1)
    else:
        valid = mo[:, 6] == 1
        assert np.any(valid) and np.all(np.isin(mo[valid, 7], loops)) and not np.any(mo[:, 7] == 4)
        assert np.any(valid & (mo[:, 2] <= 64)) and np.any(valid & (mo[:, 2] > 64))  # one and two rows per lane
    assert np.array_equal(M * z, _oracle(G, B, C, M, props) @ z)


@pytest.mark.parametrize("name", ["dense_col", "arrow_row"] + [f"tiny{n}x{m}" for n, m in structures.TINY_SHAPES])
def test_rowspan_structures(gpu_ctx, name):
    import cpkrylov_amd as cpk
    S = structures.get(name)
    z = np.random.default_rng(41).standard_normal(S["n"] + S["m"])
    with cpk.engine_options(all_rowspan=1):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
    props = dict(nitref=1, force_itref=True)
    for k, v in props.items():
        setattr(M, k, v)
    assert np.array_equal(M * z, _oracle(S["G"], S["B"], S["C"], M, props) @ z)


def test_rowspan_zeros_and_subnormals(gpu_ctx):
    """Inputs with +0.0, -0.0 and subnormals, and an all-(-0.0) vector: an absent slot subtracts
    +0.0 and a present term its true product, so the signs of zeros come out as the oracle's."""
    import cpkrylov_amd as cpk
    S = _w64()
    G, B, C = S["G"], S["B"], S["C"]
    N = G.shape[0] + B.shape[0]
    rng = np.random.default_rng(43)
    z = rng.standard_normal(N)
    kind = rng.integers(0, 6, N)
    z[kind == 0] = 0.0
    z[kind == 1] = -0.0
    z[kind == 2] = 5e-324 * rng.integers(1, 1 << 20, N)[kind == 2]
    with cpk.engine_options(all_rowspan=1):
        M = cpk.opLDL2(G, B, -C)
    for props in (dict(nitref=0), dict(nitref=1, force_itref=True)):
        for k, v in props.items():
            setattr(M, k, v)
        Mo = _oracle(G, B, C, M, props)
        for x in (z, np.full(N, -0.0)):
            y, yo = M * x, Mo @ x
            assert np.array_equal(y, yo, equal_nan=True)
            assert np.array_equal(np.signbit(y), np.signbit(yo))


def test_rowspan_refactor(gpu_ctx):
    """New values on the same layout (the layout is structure only): equal to a fresh construction
    and to the oracle."""
    import cpkrylov_amd as cpk
    S = _w64()
    rng = np.random.default_rng(47)
    G2 = S["G"].copy()
    G2.data = G2.data * rng.uniform(0.5, 2.0, G2.data.shape[0])
    B2 = S["B"].copy()
    B2.data = B2.data * rng.uniform(0.8, 1.25, B2.data.shape[0])
    C2 = S["C"].copy()
    C2.data = C2.data * 3.0
    props = dict(nitref=1, force_itref=True)
    with cpk.engine_options(all_rowspan=1):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        assert M.refactor(G2, B2, -C2) > 0
        M2 = cpk.opLDL2(G2, B2, -C2)
    for Mx in (M, M2):
        for k, v in props.items():
            setattr(Mx, k, v)
    z = rng.standard_normal(M.n)
    y = M * z
    assert np.array_equal(y, M2 * z)
    assert np.array_equal(y, _oracle(G2, B2, C2, M, props) @ z)


def test_rowspan_dist_tsweep():
    """SimComm P = 2 with the separator solved by the block sweeps: the T sweep's upper rounds and
    the ranks' own on the row-span loop."""
    import cpkrylov_amd as cpk
    S = _w64()
    z = np.random.default_rng(53).standard_normal(S["n"] + S["m"])

    def work(ctx, r):
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        M.nitref, M.force_itref = 1, True
        return M * z, M.export_factors() if r == 0 else None, M.block_model(), M.sep_info()

    res = _run_ranks(2, work, {"tsolve_sweep": 1, "all_rowspan": 1})
    for _, _, mo, info in res:  # the loop runs: in the rank's own upper rounds and in the T sweep's (directions 2, 3)
        assert info["tsweep"] == 1
        for d in (0, 1, 2, 3):
            assert np.any((mo[:, 1] == d) & (mo[:, 7] == 4)), (d, mo[mo[:, 1] == d][:, [2, 7, 8]])
    L, D, perm = res[0][1]
    Mo = O.LDL2(S["G"], S["B"], -S["C"], factors=(L, D, perm))
    Mo.set(nitref=1.0, force_itref=1.0)
    yo = Mo @ z
    for y, *_ in res:
        assert np.array_equal(y, yo), np.max(np.abs(y - yo))
