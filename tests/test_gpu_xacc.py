"""The device's exact-dot accumulator (engine option exact_dots, xacc.hpp) at edge values, through
the diagnostic entries cpk_debug_dot / cpk_debug_xnorm2 / cpk_debug_spmm.

The mode promises "the correctly rounded value of the exact sum of the TwoProd pairs", the same
bits on any grid, any rank count and in the oracle.  The oracle's side of that is checked against
rational arithmetic in test_oracle.py and test_xacc_cases.py; this module holds the device's
separate implementation to it: the per-thread TwoSum expansion (XAcc), xdeposit, the shuffle / LDS
merges of block_deposit and wave_hand, gather_digits, xround, xround_kernel behind the int64
allreduce, and xnorm2.  Inputs and references: xacc_cases.py (reference A: rational arithmetic,
where no product under- or overflows; reference B: the oracle, bit for bit, always).

Out of scope here: arnoldi_dots_exact_kernel and its own index arithmetic (% nsum, groups of 4,
chunks of 16).  test_gpu_arnoldi_step.py drives it, and the rest of the Arnoldi step, directly
(cpk_debug_arnoldi_step), with these families in its window sums; the pieces it shares with the
rest (XAcc::add, block_deposit, gather_digits, xround) are covered here.

Found by this module (the values before the fix): finite terms whose partial sum overflowed in a
thread or a merge step (H + H with H = 1.7e308) went through the TwoSum as inf - inf and the sum
came back NaN, where the definition gives +-inf (family 5), DBL_MAX (family 5) or 3.0 (family 6).
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

import xacc_cases as X
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097, 5000)  # 4097: 17 workgroups, two share sub-accumulator 0
GRIDS = ((1, 1280), (2, 1280), (15, 4097), (16, 4097), (17, 5000))  # (grid override, n): below, at, above kXSub
TILED = (1, 257, 1023, 1024, 1025)
WRAP = 262144 + 257  # the default grid (1024 workgroups) wrapped: a second element in 257 threads


def _cols(cols):
    n = len(cols[0][0])
    ld = max(n, 1)
    A, B = np.zeros((ld, len(cols)), order="F"), np.zeros((ld, len(cols)), order="F")
    for j, (a, b) in enumerate(cols):
        A[:n, j], B[:n, j] = a, b
    return n, ld, A, B


def gpu_dot(ctx, cols, kind=0, grid=0):
    """cpk_debug_dot on the columns [(a, b), ...] (nv of them, one length)"""
    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _dptr
    n, ld, A, B = _cols(cols)
    out = np.full(len(cols), -7.0)
    _lib.check(_lib.lib.cpk_debug_dot(ctx.h, kind, n, len(cols), _dptr(A), ld, _dptr(B), ld, grid, _dptr(out)))
    return out


@pytest.fixture(scope="module")
def xctx():
    """a context of its own in exact mode (the session's default context stays in default mode)"""
    import cpkrylov_amd as cpk
    ctx = cpk.Context(options=dict(exact_dots=1))
    yield ctx
    ctx.close()


_REF = {}


def refs(name, a, b):
    """(reference B, reference A or None) of a case, computed once"""
    key = (name, len(a))
    if key not in _REF:
        _REF[key] = (O.xdot(a, b), X.ref_exact(a, b) if X.a_applies(a, b) else None)
    return _REF[key]


def check_exact(got, name, a, b, where):
    rb, ra = refs(name, a, b)
    print(f"{where} {name}: device {got!r} oracle {rb!r} rational {ra!r}")
    assert X.same_bits(got, rb), (where, name, got, rb)
    if ra is not None:
        assert X.same_bits(got, ra), (where, name, got, ra)


def groups(cs, nv):
    """the cases nv at a time, each group's columns from different families where there are enough"""
    order = [cs[(7 * i) % len(cs)] for i in range(len(cs))] if len(cs) % 7 else list(cs)
    order += [order[i % len(order)] for i in range((-len(order)) % nv)]
    return [order[i:i + nv] for i in range(0, len(order), nv)]


def run_cases(ctx, cs, nv, kind=0, grid=0, where=""):
    for g in groups(cs, nv):
        out = gpu_dot(ctx, [(a, b) for _, a, b in g], kind, grid)
        for (name, a, b), v in zip(g, out):
            check_exact(v, name, a, b, f"{where} nv={nv} kind={kind} grid={grid} n={len(a)}")


# ---- exact mode: every family, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_exact_every_family(xctx, n):
    cs = X.cases(n)
    for nv in (1, 2, 4):
        run_cases(xctx, cs, nv)


@pytest.mark.parametrize("grid,n", GRIDS)
def test_exact_grid_override(xctx, grid, n):
    """one workgroup with several elements per thread, fewer workgroups than sub-accumulators, as
    many, more: the same bits"""
    cs = X.cases(n)
    run_cases(xctx, cs, 1, grid=grid)
    run_cases(xctx, cs, 4, grid=grid)


@pytest.mark.parametrize("n", TILED)
def test_exact_tiled_form(xctx, n):
    cs = X.cases(n)
    for nv in (1, 2, 4):
        run_cases(xctx, cs, nv, kind=1)
    if n == 1025:
        run_cases(xctx, cs, 2, kind=1, grid=1)


def test_exact_default_grid_wraps(xctx):
    cs = [(name, *X.case(name, WRAP)) for name in ("wide40", "wide1000", "cancel0", "sticky_1070_neg", "sub_terms",
                                                    "dblmax_half", "mid_ovf", "prod_unf")]
    run_cases(xctx, cs, 4)
    run_cases(xctx, cs[:2], 1)


def test_exact_cascade_remainder_is_deposited(xctx):
    """the overflow-deposit path by construction: the launch model shows thread 0's three-term
    expansion leaving two remainders with one workgroup (and none with five)"""
    a, b = X.cascade_terms()
    assert X.launch_model(a, b, grid=1) == (2, 0) and X.launch_model(a, b, grid=1, kind=1) == (2, 0)
    for kind, grid in ((0, 1), (1, 1), (0, 5), (0, 0)):
        check_exact(gpu_dot(xctx, [(a, b)], kind, grid)[0], "cascade", a, b, f"kind={kind} grid={grid}")
    # the wide family leaves remainders in many threads when each thread takes ~20 elements
    a, b = X.case("wide1000", 5000)
    assert X.launch_model(a, b, grid=1)[0] > 0
    check_exact(gpu_dot(xctx, [(a, b)], 0, 1)[0], "wide1000", a, b, "grid=1")


PLACEMENTS = [("one thread", 1, (0, 256)), ("two waves", 0, (0, 64)), ("two workgroups", 0, (0, 256))] + \
             [(f"lanes {d} apart", 0, (0, d)) for d in (1, 2, 4, 8, 16, 32)]


@pytest.mark.parametrize("h", (X.H, 2.0 ** 1023), ids=("H", "2p1023"))
@pytest.mark.parametrize("what,grid,plus", PLACEMENTS, ids=[p[0].replace(" ", "_") for p in PLACEMENTS])
def test_exact_intermediate_overflow(xctx, what, grid, plus, h):
    """h, h, -h, -h, 3.0: the two +h meet in one thread, in one shuffle step, in the LDS merge or
    only in the digits, before either meets a -h (other waves).  The sum is 3.0 wherever they meet.
    h = 1.7e308, and h = 2^1023, which a thread's expansion holds until the second one arrives."""
    n = 1280
    a, b = X.intermediate(n, plus, (700, 900), 5, h)
    if what == "one thread":
        assert X.launch_model(a, b, grid=1)[1] == (4 if h == X.H else 1)
    for nv in (1, 4):
        out = gpu_dot(xctx, [(a, b)] * nv, 0, grid)
        print(what, nv, out)
        for v in out:
            check_exact(v, f"mid_ovf {what} {h!r}", a, b, what)
            assert X.same_bits(v, 3.0)


MERGED_AT = [("shuffle steps", 64, 0, (16, 48, 0)),       # lane 16 takes lane 48 at offset 32, lane 0 takes it at 16
             ("shuffle then LDS", 256, 0, (80, 112, 0)),  # wave 1 merges them, thread 0 adds wave 1's sum
             ("one thread", 1280, 1, (0, 256, 512)),
             ("two workgroups", 1280, 0, (16, 48, 300))]


@pytest.mark.parametrize("sign", (1.0, -1.0), ids=("pos", "neg"))
@pytest.mark.parametrize("what,n,grid,at", MERGED_AT, ids=[p[0].replace(" ", "_") for p in MERGED_AT])
def test_exact_merged_partial_near_dblmax(xctx, what, n, grid, at, sign):
    """2^1023 and 2^1023 - 2^971 merge to exactly DBL_MAX; adding -3 2^970 to that gives a finite
    sum, but a TwoSum recovers its operand as (DBL_MAX - 2^971) + 3 2^970, which rounds to inf.
    The expansion's leading term therefore never exceeds 2^1023; the result is finite wherever
    the three terms meet, and so is its negation."""
    a, b = X.merged(n, *at, sign=sign)
    want = sign * (X.DBL_MAX - 2.0 ** 971)  # the tie at DBL_MAX - 3 2^970, to even
    assert X.same_bits(X.ref_exact(a, b), want)
    for nv in (1, 4):
        for v in gpu_dot(xctx, [(a, b)] * nv, 0, grid):
            check_exact(v, f"merged {what} {sign}", a, b, what)
            assert X.same_bits(v, want)


# ---- buffer hygiene ------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,then", ((4, 1), (1, 4)))
def test_exact_buffers_are_clean_after_nan_and_inf(xctx, first, then):
    """after a NaN and after a +-inf result the next call on the same context is right:
    gather_digits re-zeroed the count word and every digit, for another number of sums too"""
    n = 4097
    benign = [(name, *X.case(name, n)) for name in ("wide40", "cancel4", "tie_even_up", "sub_terms")]
    for dirty in ("nan_term", "inf_term", "prod_ovf", "ovf_inf", "ovf_inf_neg", "ovf_inf_held", "dblmax_half"):
        a, b = X.case(dirty, n)
        out = gpu_dot(xctx, [(a, b)] * first)
        for v in out:
            check_exact(v, dirty, a, b, f"dirty nv={first}")
        out = gpu_dot(xctx, [(x, y) for _, x, y in benign[:then]])
        for (name, x, y), v in zip(benign, out):
            check_exact(v, name, x, y, f"after {dirty} nv={then}")


# ---- default mode ---------------------------------------------------------------------------------------
def check_default(ctx, cs, nv, kind=0, grid=0):
    """the fixed-tree sums: |out - exact| <= gamma_n sum |a b| (gamma_n = n u / (1 - n u), u = 2^-53:
    n - 1 additions and one product rounding per term, any order), where its premises hold (no
    product under- or overflows and sum |a b| is finite, so no partial sum overflows); two calls
    return the same bits"""
    assert ctx.get_option("exact_dots") == "0"
    cs = [(name, a, b) for name, a, b in cs if X.default_mode_ok(a, b)]
    assert cs
    for g in groups(cs, nv):
        out = gpu_dot(ctx, [(a, b) for _, a, b in g], kind, grid)
        again = gpu_dot(ctx, [(a, b) for _, a, b in g], kind, grid)
        assert X.same_bits(out, again)
        for (name, a, b), v in zip(g, out):
            assert math.isfinite(v), (name, len(a), v)
            err, bound = X.error_and_bound(v, a, b)
            print(f"n={len(a)} nv={nv} kind={kind} grid={grid} {name}: error {float(err):.3e} bound {float(bound):.3e}")
            assert err <= bound, (name, len(a), nv, kind, grid, float(err), float(bound))


@pytest.mark.parametrize("n", SIZES)
def test_default_mode_bound(gpu_ctx, n):
    for nv in (1, 2, 4):
        check_default(gpu_ctx, X.cases(n), nv)


@pytest.mark.parametrize("grid,n", GRIDS)
def test_default_grid_override(gpu_ctx, grid, n):
    check_default(gpu_ctx, X.cases(n), 1, grid=grid)
    check_default(gpu_ctx, X.cases(n), 4, grid=grid)


@pytest.mark.parametrize("n", TILED)
def test_default_tiled_form(gpu_ctx, n):
    for nv in (1, 2, 4):
        check_default(gpu_ctx, X.cases(n), nv, kind=1)
    if n == 1025:
        check_default(gpu_ctx, X.cases(n), 2, kind=1, grid=1)


def test_default_grid_wraps(gpu_ctx):
    cs = [(name, *X.case(name, WRAP)) for name in ("wide40", "wide1000", "cancel0", "sticky_1070_neg")]
    check_default(gpu_ctx, cs, 4)
    check_default(gpu_ctx, cs[:1], 1)


# ---- distributed: the int64 allreduce and xround_kernel ----------------------------------------------
def _run_ranks(P, fn, options):
    import cpkrylov_amd as cpk
    g = cpk.SimGroup(P)

    def one(r):
        ctx = cpk.Context(device=0, rank=r, nranks=P, simgroup=g, options=dict(options))
        try:
            return fn(ctx, r)
        finally:
            ctx.close()

    with ThreadPoolExecutor(P) as ex:
        return [f.result(timeout=600) for f in [ex.submit(one, r) for r in range(P)]]


def _dist_cases():
    n = 1500
    cs = X.cases(n, families=(1, 2, 5, 6, 7))
    # family 6 with the two +H on different ranks (the cuts below), and within one rank
    cs.append(("mid_ovf two ranks", *X.intermediate(n, (3, 1400), (700, 900), 5)))
    cs.append(("mid_ovf one rank", *X.intermediate(n, (1300, 1301), (2, 700), 5)))
    cs.append(("merged two ranks", *X.merged(n, 16, 1300, 0)))
    cs.append(("merged one rank", *X.merged(n, 1216, 1248, 1280, sign=-1.0)))
    return n, cs


@pytest.mark.parametrize("exact", (1, 0))
@pytest.mark.parametrize("P", (2, 3))
def test_dist_global_sums(P, exact):
    """every rank passes its rows (one rank has none) and receives the global sums: reference B's
    bits of the concatenated vectors in exact mode, the gamma_n bound in default mode"""
    n, cs = _dist_cases()
    cuts = [0, 0, 1201, n] if P == 3 else [0, 1201, n]  # P = 3: rank 0 has no rows
    if not exact:
        cs = [c for c in cs if X.default_mode_ok(c[1], c[2])]
    gs = groups(cs, 4) + groups(cs[:3], 1) + groups(cs[:4], 2)

    def work(ctx, r):
        lo, hi = cuts[r], cuts[r + 1]
        return [gpu_dot(ctx, [(a[lo:hi], b[lo:hi]) for _, a, b in g]) for g in gs]

    res = _run_ranks(P, work, dict(exact_dots=exact))
    for r, outs in enumerate(res):
        for i, (g, out) in enumerate(zip(gs, outs)):
            assert X.same_bits(out, res[0][i])  # every rank the same bits
            for (name, a, b), v in zip(g, out):
                if exact:
                    check_exact(v, name, a, b, f"P={P} rank={r}")
                else:
                    err, bound = X.error_and_bound(v, a, b)
                    assert err <= bound, (name, P, r)


# ---- norm([a b]) ------------------------------------------------------------------------------------------
def test_xnorm2_equals_oracle(gpu_ctx):
    """Pythagorean triples, signs and zeros, inf and nan, the scaling thresholds 2^500 and 2^-500 and
    their neighbours, DBL_MAX, subnormal pairs, b^2 underflowing, 4096 random pairs over 2^+-430"""
    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _dptr
    a, b = X.xnorm2_pairs()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.full(len(a), -7.0)
    _lib.check(_lib.lib.cpk_debug_xnorm2(gpu_ctx.h, len(a), _dptr(a), _dptr(b), _dptr(out)))
    want = np.array([O.xnorm2(x, y) for x, y in zip(a, b)])
    bad = np.flatnonzero(~((X.bits(out) == X.bits(want)) | (np.isnan(out) & np.isnan(want))))
    assert bad.size == 0, [(a[i], b[i], out[i], want[i]) for i in bad[:5]]
    assert out[0] == 5.0 and out[1] == 13.0


# ---- the panel path: wave_hand(XAcc&) and the per-column gather_digits ------------------------------------
PN, PM = 1500, 700  # rows of A and of C: three row blocks of blkdiag(A, C), so three workgroups
# signed powers of two (sign, exponent) whose sum is the wanted result, and where they go: False: seeded
# rows; True: the first two at rows 0 and 64 of their part -- one lane of the product's wave, so they
# meet inside a thread; a list: these rows (a row's lane is its index modulo 64 in the A part)
_MERGED = [(1, 1023), (1, 1023), (-1, 971), (-1, 971), (-1, 970)]  # X.MERGED: lane 16, lane 48 (two rows), lane 0
_MERGED_ROWS = [16, 48, 112, 0, 64]
PANEL_TERMS = {
    "cancel_tiny": ([(1, -1074)], False),
    "cancel_minnormal": ([(-1, -1022)], False),
    "cancel_125": ([(-1, 0), (-1, -2)], False),
    "ovf_inf": ([(1, 1023), (1, 1023)], True),
    "ovf_inf_neg": ([(-1, 1023), (-1, 1023)], True),
    "dblmax": ([(1, e) for e in range(971, 1024)], False),           # 2^1023 + ... + 2^971 = DBL_MAX
    "dblmax_half": ([(1, e) for e in range(970, 1024)], False),      # ... + 2^970: the tie at the top, to inf
    "dblmax_below_half": ([(1, e) for e in range(971, 1024)] + [(1, 969)], False),
    "mid_ovf": ([(1, 1023), (1, 1023), (-1, 1023), (-1, 1023), (1, 1), (1, 0)], True),  # = 3.0
    "merged": (_MERGED, _MERGED_ROWS),
    "merged_neg": ([(-s, e) for s, e in _MERGED], _MERGED_ROWS),
}
PANEL_WANT = {"cancel_tiny": 5e-324, "cancel_minnormal": -2.0 ** -1022, "cancel_125": -1.25, "ovf_inf": math.inf,
              "ovf_inf_neg": -math.inf, "dblmax": X.DBL_MAX, "dblmax_half": math.inf, "dblmax_below_half": X.DBL_MAX,
              "mid_ovf": 3.0, "merged": X.DBL_MAX - 2.0 ** 971, "merged_neg": -(X.DBL_MAX - 2.0 ** 971)}
PANEL_NAMES = tuple(PANEL_TERMS)


def _pow2_terms(name, rows, rng):
    """(sign, exponent) per row: the case's terms, and shuffled cancelling pairs in the other rows"""
    t, meet = PANEL_TERMS[name]
    free = rows - len(t)
    k = free // 2
    # (merged: pairs below 2^900 leave the leading terms of the lanes they share as they are)
    e = rng.integers(-1000, 900 if name.startswith("merged") else 1000, k)
    s = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    fs, fe = np.concatenate([s, -s, np.zeros(free - 2 * k)]), np.concatenate([e, e, np.zeros(free - 2 * k, np.int64)])
    perm = rng.permutation(free)
    if meet is True:
        pos = np.array([0, 64] + list(range(1, len(t) - 1)))
    else:
        pos = np.array(meet) if meet else rng.choice(rows, len(t), replace=False)
    rest = np.setdiff1d(np.arange(rows), pos)
    sign, expo = np.zeros(rows), np.zeros(rows, np.int64)
    sign[pos], expo[pos] = [x[0] for x in t], [x[1] for x in t]
    sign[rest], expo[rest] = fs[perm], fe[perm]
    return sign, expo


def _panel_system(name_n, name_m, seed):
    """the diagonal q of blkdiag(A, C) and x, signed powers of two with y = q x finite and the terms
    y x = q x^2 of the two inner products the wanted s 2^e: x = 2^m, q = s 2^(e - 2 m), with
    m = ceil(e / 2) for a large |e| (then |e - 2 m| <= 1 and |e - m| <= 537) and 0 otherwise"""
    rng = np.random.default_rng(seed)
    sn, en = _pow2_terms(name_n, PN, rng)
    sm, em = _pow2_terms(name_m, PM, rng)
    s, e = np.concatenate([sn, sm]), np.concatenate([en, em])
    m = np.where(np.abs(e) > 900, -((-e) // 2), 0)
    return s * np.ldexp(1.0, (e - 2 * m).astype(np.int32)), np.ldexp(1.0, m.astype(np.int32))


@pytest.mark.parametrize("k", (1, 8))
def test_panel_product_exact_sums(gpu_ctx, k):
    """families 2, 5 and 6 (and the three terms that merge past DBL_MAX) through the panel product's own merge (cpk_debug_spmm in exact mode): a
    diagonal operator and x of signed powers of two, so every product and every term of the two
    inner products is a signed power of two and reference A is integer arithmetic.  Y stays finite
    and is compared too.  Odd columns take -x: the same terms, another wave of the workgroup."""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _as_matrix, _dptr
    N = PN + PM
    with cpk.engine_options(exact_dots=1):
        M = cpk.opLDL2(sp.identity(PN, format="csr"), sp.eye(PM, PN, format="csr"), -sp.identity(PM, format="csr"))
        for i, nn in enumerate(PANEL_NAMES):
            nm = PANEL_NAMES[(i + 4) % len(PANEL_NAMES)]
            q, x = _panel_system(nn, nm, 100 * k + i)
            A, Cm = _as_matrix(sp.diags(q[:PN], format="csr"), M.ctx), _as_matrix(sp.diags(q[PN:], format="csr"), M.ctx)
            Xb = np.asfortranarray(np.column_stack([x if j % 2 == 0 else -x for j in range(k)]))
            Y, dots = np.full((N, k), np.nan, order="F"), np.zeros(2 * k)
            _lib.check(_lib.lib.cpk_debug_spmm(M.ctx.h, A.h, Cm.h, M.h, k, _dptr(Xb), N, _dptr(Y), N, _dptr(dots)))
            for j in range(k):
                y = q * Xb[:, j]
                assert np.all(np.isfinite(y)) and np.array_equal(Y[:, j], y)
                for h, (lo, hi, name) in enumerate(((0, PN, nn), (PN, N, nm))):
                    assert X.a_applies(y[lo:hi], Xb[lo:hi, j])
                    ra, rb = X.ref_exact(y[lo:hi], Xb[lo:hi, j]), O.xdot(y[lo:hi], Xb[lo:hi, j])
                    print(f"k={k} col {j} {name}: device {dots[2 * j + h]!r} oracle {rb!r} rational {ra!r}")
                    assert X.same_bits(ra, PANEL_WANT[name]) and X.same_bits(rb, ra)
                    assert X.same_bits(dots[2 * j + h], ra), (k, j, name, dots[2 * j + h], ra)
