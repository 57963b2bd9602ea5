"""Inputs and references for the exact-dot accumulator (engine option exact_dots, xacc.hpp) at the
values where a superaccumulator goes wrong: wide exponents, total cancellation, ties, carries,
subnormals, overflow of the result and of partial sums, non-finite terms, signed zeros.

Two references:
  A  ref_exact(a, b): the correctly rounded sum(a[i] * b[i]) by integer arithmetic over a common
     power of two and one Fraction -> float conversion.  It is the mode's definition only when no
     product under- or overflows (a_applies).
  B  the oracle (oracle.xdot / oracle.xnorm2), for every input: where a product under- or
     overflows both sides still perform the same IEEE operations.  Compared as bit patterns
     (same_bits: +0.0 and -0.0 differ, two NaNs agree).

Every case is a named, seeded generator build(n) -> (a, b).  A plain module (not a conftest);
test infrastructure only."""
import math
from fractions import Fraction

import numpy as np

BLOCK, WAVE, XK, TILE, XSUB, EW_GRID = 256, 64, 3, 4, 16, 1024  # devutil.hpp, xacc.hpp, solver_common.hpp
DBL_MAX = float(np.finfo(np.float64).max)
H = 1.7e308  # H + H overflows
# two terms that merge to exactly DBL_MAX, and a third whose TwoSum with that overflows in the
# recovered operand although the sum is finite: (DBL_MAX - 3 2^970) - (-3 2^970) rounds to inf
MERGED = (2.0 ** 1023, 2.0 ** 1023 - 2.0 ** 971, -3 * 2.0 ** 970)


# ---- references ------------------------------------------------------------------------------
def ref_exact(a, b):
    """reference A: the products summed as integers over a common power of two, then one Fraction
    to float conversion (Python rounds it to nearest even; beyond the range: +-inf)"""
    terms = []
    for p, q in zip(a, b):
        (mp, ep), (mq, eq) = math.frexp(float(p)), math.frexp(float(q))
        terms.append((int(mp * 2 ** 53) * int(mq * 2 ** 53), ep + eq - 106))
    if not terms:
        return 0.0
    e0 = min(e for _, e in terms)
    total = sum(t << (e - e0) for t, e in terms)
    try:
        return float(Fraction(total) * Fraction(2) ** e0)
    except OverflowError:
        return math.inf if total > 0 else -math.inf


def a_applies(a, b):
    """reference A is the definition: every factor finite, no product overflows (p = a * b is
    finite) and none underflows (a * b is a multiple of 2^-1074, so p and fma(a, b, -p) are exact)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return False
    with np.errstate(over="ignore", under="ignore"):
        p = a * b
    if not np.all(np.isfinite(p)):
        return False
    ma, ea = np.frexp(a)
    mb, eb = np.frexp(b)
    # lowest set bit of a[i] * b[i]: 2^(ea - 53 + tz(ma)) * 2^(eb - 53 + tz(mb))
    ia, ib = (np.ldexp(ma, 53)).astype(np.int64), (np.ldexp(mb, 53)).astype(np.int64)
    nz = (ia != 0) & (ib != 0)

    def tz(v):
        v = np.abs(v[nz])
        return np.log2((v & -v).astype(np.float64)).astype(np.int64)
    low = ea[nz] - 53 + tz(ia) + eb[nz] - 53 + tz(ib)
    return bool(np.all(low >= -1074))


def bits(x):
    return np.asarray(x, dtype=np.float64).reshape(-1).view(np.int64)


def same_bits(x, y):
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    return x.shape == y.shape and bool(np.all((bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))))


def _int_sums(a, b):
    """(sum a[i] b[i], sum |a[i] b[i]|) as Fractions, by integer arithmetic over a common power of two"""
    terms = []
    for p, q in zip(a, b):
        (mp, ep), (mq, eq) = math.frexp(float(p)), math.frexp(float(q))
        terms.append((int(mp * 2 ** 53) * int(mq * 2 ** 53), ep + eq - 106))
    if not terms:
        return Fraction(0), Fraction(0)
    e0 = min(e for _, e in terms)
    scale = Fraction(2) ** e0
    return sum(t << (e - e0) for t, e in terms) * scale, sum(abs(t) << (e - e0) for t, e in terms) * scale


def error_and_bound(v, a, b):
    """(|v - sum a[i] b[i]|, gamma_n sum |a[i] b[i]|) as Fractions, gamma_n = n u / (1 - n u),
    u = 2^-53: the bound on |fl(sum) - sum| of any summation order (n - 1 additions and one product
    rounding per term)"""
    n = len(a)
    u = Fraction(1, 2 ** 53)
    total, abs_total = _int_sums(a, b)
    return abs(Fraction(float(v)) - total), n * u / (1 - n * u) * abs_total


def default_mode_ok(a, b):
    """the bound's premises: reference A applies, and sum |a[i] b[i]| is below DBL_MAX, so no
    partial sum overflows in any order"""
    if not a_applies(a, b):
        return False
    with np.errstate(over="ignore"):
        return bool(np.isfinite(np.sum(np.abs(np.asarray(a) * np.asarray(b)))))


# ---- the input families ------------------------------------------------------------------------
def _rng(name, n):
    return np.random.default_rng([sum(name.encode()), len(name), n])


def _filler(rng, k):
    """k slots whose products cancel exactly: shuffled pairs (v, w), (-v, w), and a zero if k is odd"""
    h = k // 2
    v = rng.standard_normal(h) * np.exp(rng.uniform(-40, 40, h))
    w = rng.standard_normal(h) * np.exp(rng.uniform(-40, 40, h))
    a = np.concatenate([v, -v, np.zeros(k - 2 * h)])
    b = np.concatenate([w, w, np.ones(k - 2 * h)])
    p = rng.permutation(k)
    return a[p], b[p]


def _scatter(name, n, ta, tb=None):
    """the terms at seeded positions of an n-vector, a cancelling filler in the other slots"""
    ta = np.asarray(ta, np.float64)
    tb = np.ones(len(ta)) if tb is None else np.asarray(tb, np.float64)
    rng = _rng(name, n)
    a, b = np.empty(n), np.empty(n)
    pos = rng.choice(n, len(ta), replace=False)
    rest = np.setdiff1d(np.arange(n), pos)
    a[pos], b[pos] = ta, tb
    a[rest], b[rest] = _filler(rng, n - len(ta))
    return a, b


def _fixed(family, name, ta, tb=None, negate=True):
    out = [(family, name, len(ta), lambda n, ta=ta, tb=tb, name=name: _scatter(name, n, ta, tb))]
    if negate:
        na = [-x for x in ta]
        out.append((family, name + "_neg", len(ta), lambda n, na=na, tb=tb, name=name: _scatter(name + "_neg", n, na, tb)))
    return out


def _wide40(n):
    rng = _rng("wide40", n)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n)), rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n)))


def _wide1000(n):
    """products from 2^-1000 to 2^1000, each exact (its lowest bit is 2^-1052 or above): a full
    mantissa in [1, 2) times a power of two"""
    rng = _rng("wide1000", n)
    a = np.ldexp(rng.uniform(1, 2, n) * np.where(rng.random(n) < 0.5, -1, 1), rng.integers(-500, 501, n))
    b = np.ldexp(np.where(rng.random(n) < 0.5, -1.0, 1.0), rng.integers(-500, 501, n))
    return a, b


def _sub_terms(n):
    """subnormal terms (integers times 2^-1074); the sum is subnormal or in the lowest binades"""
    rng = _rng("sub_terms", n)
    k = rng.integers(1, 2 ** 52, n).astype(np.float64) * np.where(rng.random(n) < 0.5, -1, 1)
    return np.ldexp(k, -1074), np.ones(n)


def _sub_prod(n):
    """normal factors whose exact products are subnormal: (k 2^-600) * 2^-474 = k 2^-1074"""
    rng = _rng("sub_prod", n)
    k = rng.integers(1, 1024, n).astype(np.float64) * np.where(rng.random(n) < 0.5, -1, 1)
    return np.ldexp(k, -600), np.full(n, 2.0 ** -474)


def _zeros_mixed(n):
    rng = _rng("zeros_mixed", n)
    a = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    b = np.where(rng.random(n) < 0.3, -0.0, rng.standard_normal(n))
    return a, b


CASES = [(1, "wide40", 1, _wide40), (1, "wide1000", 1, _wide1000)]
# 2. cancellation: the residue is the whole result
for _i, _r in enumerate((2.0 ** -1074, -2.0 ** -1074, 2.0 ** -1022, -2.0 ** -1022, -1.25)):
    CASES += _fixed(2, f"cancel{_i}", [_r], negate=False)
# 3. rounding
CASES += _fixed(3, "tie_even_down", [1.0, 2.0 ** -53])
CASES += _fixed(3, "tie_even_up", [1.0, 2.0 ** -52, 2.0 ** -53])
CASES += _fixed(3, "sticky_200", [1.0, 2.0 ** -53, 2.0 ** -200])
CASES += _fixed(3, "sticky_1070", [1.0, 2.0 ** -53, 2.0 ** -1070])
CASES += _fixed(3, "borrow_1070", [1.0, 2.0 ** -53, -2.0 ** -1070])
CASES += _fixed(3, "carry_2", [2.0 - 2.0 ** -52, 2.0 ** -53])
# 4. subnormal terms and results
CASES += [(4, "sub_terms", 1, _sub_terms), (4, "sub_prod", 1, _sub_prod)]
CASES += _fixed(4, "sub_three", [5e-324, 5e-324, -1e-320])
# 5. overflow of the result, and results at the top of the range
CASES += _fixed(5, "ovf_inf", [H, H])
CASES += _fixed(5, "ovf_inf_held", [2.0 ** 1023, 2.0 ** 1023])  # each fits a thread's expansion
CASES += _fixed(5, "dblmax_exact", [2.0 ** 1023, 2.0 ** 1023 - 2.0 ** 971])
CASES += _fixed(5, "dblmax_via_ovf", [DBL_MAX, 2.0 ** 1000, -2.0 ** 1000])
CASES += _fixed(5, "dblmax_below_half", [DBL_MAX, 2.0 ** 970 - 2.0 ** 917])
CASES += _fixed(5, "dblmax_half", [DBL_MAX, 2.0 ** 970])
CASES += _fixed(5, "dblmax_merged", list(MERGED))  # placed deliberately: merged()
# 6. a partial sum overflows, the result is finite (placed deliberately: intermediate())
CASES += _fixed(6, "mid_ovf", [H, H, -H, -H, 3.0], negate=False)
# 7. non-finite terms and products
CASES += _fixed(7, "inf_term", [math.inf], negate=False)
CASES += _fixed(7, "nan_term", [math.nan], negate=False)
CASES += _fixed(7, "inf_times_0", [math.inf], [0.0], negate=False)
CASES += _fixed(7, "prod_ovf", [1e200], [1e200], negate=False)
CASES += _fixed(7, "prod_unf", [1e-160, 3e-170], [1e-160, 7e-150], negate=False)
# 8. zeros
CASES += [(8, "zeros", 1, lambda n: (np.zeros(n), np.zeros(n))), (8, "zeros_mixed", 1, _zeros_mixed)]
NAMES = [c[1] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def cases(n, families=None):
    """[(name, a, b)] of the cases that fit into n elements (n = 0: the empty sum)"""
    if n == 0:
        return [("empty", np.zeros(0), np.zeros(0))]
    return [(name, *build(n)) for fam, name, nmin, build in CASES
            if nmin <= n and (families is None or fam in families)]


def case(name, n):
    fam, _, nmin, build = CASES[NAMES.index(name)]
    assert n >= nmin
    return build(n)


def intermediate(n, plus, minus, three, h=H):
    """family 6 placed: +h at the two indices `plus`, -h at `minus`, 3.0 at `three`, zeros elsewhere.
    h = H = 1.7e308 is above XAcc::add_prod's threshold 2^1023, so a thread hands each one to the
    digits on sight; h = 2^1023 is held in the expansion, and two of them overflow where they meet"""
    a = np.zeros(n)
    a[list(plus)], a[list(minus)], a[three] = h, -h, 3.0
    return a, np.ones(n)


def merged(n, first, second, third, sign=1.0):
    """MERGED placed: the two large terms at `first` and `second`, the small one at `third`, zeros
    elsewhere; sign = -1: the negated form"""
    a = np.zeros(n)
    a[[first, second, third]] = np.array(MERGED) * sign
    return a, np.ones(n)


def cascade_terms(n=1280):
    """2^300, 2^150, 1, 2^-150, 2^-300 at 256 apart: with one workgroup they meet in thread 0,
    whose three-term expansion cannot hold them (launch_model: a non-zero remainder)"""
    a = np.zeros(n)
    a[0:1280:256] = [2.0 ** 300, 2.0 ** 150, 1.0, 2.0 ** -150, 2.0 ** -300]
    return a, np.ones(n)


# ---- a model of the launch -----------------------------------------------------------------------
def default_grid(n):
    return max(1, min((n + BLOCK - 1) // BLOCK, EW_GRID))


def _two_prod(x, y):
    p = x * y
    if not math.isfinite(p):
        return p, 0.0
    return p, float(Fraction(x) * Fraction(y) - Fraction(p))  # exact where a_applies


def launch_model(a, b, grid=0, kind=0):
    """Per-thread accumulation of the reducing kernels (ewred_kernel: thread t of workgroup w takes
    elements w * 256 + t + m * grid * 256; ewtred_kernel: four elements 256 apart per step) through
    XAcc::add's three-term TwoSum cascade.  Returns the number of additions that left a non-zero
    remainder after the cascade (the overflow-deposit path) and of products that XAcc::add_prod's
    range test sent to the digits (|t[0] + p| above 2^1023: the overflowing partial sum, and every
    term that large).  Finite factors only."""
    n = len(a)
    grid = grid or default_grid(n)
    idx = np.flatnonzero((np.asarray(a) != 0) & (np.asarray(b) != 0))
    span = BLOCK * (TILE if kind else 1)
    thread = ((idx // span) % grid) * BLOCK + idx % BLOCK
    remainders = overflows = 0
    for th in np.unique(thread):
        t = [0.0] * XK
        for i in idx[thread == th]:  # ascending i: the kernel's order
            p, e = _two_prod(float(a[i]), float(b[i]))
            if not abs(t[0] + p) <= 2.0 ** 1023:  # XAcc::add_prod's one test for the pair
                overflows += 1  # p and e go to the digits, the expansion stays
                continue
            for x in (p, e):
                for k in range(XK):
                    s = t[k] + x
                    bb = s - t[k]
                    x = (t[k] - (s - bb)) + (x - bb)
                    t[k] = s
                remainders += x != 0
    return remainders, overflows


# ---- norm([a b]) ------------------------------------------------------------------------------------
def hypot_exact(a, b):
    """the correctly rounded sqrt(a^2 + b^2) of finite a, b with a result in the normal range: the
    integer square root of the sum scaled to 2 * 54 + 2 bits and above, then one rounding (the
    remainder's sticky bit appended, so the conversion rounds the true value)"""
    s = Fraction(float(a)) ** 2 + Fraction(float(b)) ** 2
    if s == 0:
        return 0.0
    k = 128 - (s.numerator.bit_length() - s.denominator.bit_length())
    k += k & 1  # even: s * 2^k has 127 bits or more, its root 63 or more
    num, den = (s.numerator << k, s.denominator) if k >= 0 else (s.numerator, s.denominator << -k)
    q, r = divmod(num, den)
    root = math.isqrt(q)
    inexact = root * root != q or r != 0  # then the true root lies strictly inside (root, root + 1)
    try:
        return float(Fraction(2 * root + inexact, 2) * Fraction(2) ** (-(k // 2)))
    except OverflowError:
        return math.inf


def xnorm2_pairs():
    """(a, b) arrays for the device / oracle comparison of xnorm2"""
    rng = np.random.default_rng(2024)
    up, dn = math.nextafter(2.0 ** 500, math.inf), math.nextafter(2.0 ** -500, 0.0)
    fixed = [(3.0, 4.0), (-5.0, 12.0), (8.0, -15.0), (-7.0, -24.0), (4.0, 3.0), (0.0, -2.5), (2.5, 0.0), (0.0, 0.0),
             (-0.0, 0.0), (-0.0, -0.0), (math.inf, 1.0), (1.0, -math.inf), (math.inf, math.nan), (math.nan, 1.0),
             (math.nan, 0.0), (0.0, math.nan), (math.inf, math.inf),
             (2.0 ** 500, 2.0 ** 500), (up, 2.0 ** 500), (up, 1.0), (2.0 ** 500, 3.0 * 2.0 ** 498),
             (2.0 ** -500, 2.0 ** -500), (dn, dn), (dn, 2.0 ** -520), (2.0 ** -500, 3.0 * 2.0 ** -502),
             (DBL_MAX, DBL_MAX), (DBL_MAX, 1.0), (DBL_MAX / 2, DBL_MAX / 2), (1e300, 1e300),
             (5e-324, 5e-324), (3e-310, 4e-310), (2.0 ** -1022, 5e-324), (1e-320, -2e-320),
             (1.0, 1e-200), (1e10, 2.0 ** -1074), (1e300, 1e-300), (1.0, 2.0 ** -27), (1.0, 2.0 ** -26)]
    fa, fb = (np.array(v) for v in zip(*fixed))
    ra = rng.standard_normal(4096) * np.exp(rng.uniform(-300, 300, 4096))
    rb = rng.standard_normal(4096) * np.exp(rng.uniform(-300, 300, 4096))
    rb[::2] = ra[::2] * rng.uniform(0.1, 10, 2048)  # half of them of comparable size
    return np.concatenate([fa, ra]), np.concatenate([fb, rb])
