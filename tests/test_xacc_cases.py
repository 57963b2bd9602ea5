"""The exact-dot test inputs (xacc_cases.py) against the oracle and exact rational arithmetic, and
the argument checks of cpk_debug_dot / cpk_debug_xnorm2 / cpk_debug_arnoldi_step -- all without a device.

Every family goes through the oracle's exact inner product (orc_xdot) and is compared with the
correctly rounded rational sum wherever that is the definition (no product under- or overflows):
the generators and the two references are proved against each other here, before
tests/test_gpu_xacc.py holds the device to them."""
import ctypes as C
import math

import numpy as np
import pytest

import xacc_cases as X
from cpkrylov_amd import _lib
from oracle import oracle as O

PD = C.POINTER(C.c_double)
SIZES = (1, 2, 3, 5, 64, 257, 1280, 5000)


@pytest.mark.parametrize("n", (0,) + SIZES)
def test_oracle_equals_rational_reference(n):
    seen = 0
    for name, a, b in X.cases(n):
        assert len(a) == n and len(b) == n
        got = O.xdot(a, b)
        if X.a_applies(a, b):
            seen += 1
            want = X.ref_exact(a, b)
            assert X.same_bits(got, want), (name, n, got, want)
    assert seen >= 1


def test_reference_a_covers_the_families():
    """reference A applies to every case of families 1-6 and 8, to none of the non-finite ones, and
    not to the underflowing product; every family has cases"""
    fams = {}
    for fam, name, nmin, build in X.CASES:
        a, b = build(max(nmin, 64))
        fams.setdefault(fam, []).append((name, X.a_applies(a, b)))
    assert sorted(fams) == [1, 2, 3, 4, 5, 6, 7, 8]
    for fam, got in fams.items():
        assert all(ok == (fam != 7) for _, ok in got), (fam, got)


def test_known_values():
    """the fixed cases give the values their names promise (both references), whatever the size"""
    one, eps = 1.0, 2.0 ** -52
    want = {"tie_even_down": one, "tie_even_up": one + 2 * eps, "sticky_200": one + eps, "sticky_1070": one + eps,
            "borrow_1070": one, "carry_2": 2.0, "sub_three": 1e-323 - 1e-320, "ovf_inf": math.inf, "ovf_inf_held": math.inf,
            "dblmax_exact": X.DBL_MAX, "dblmax_via_ovf": X.DBL_MAX, "dblmax_below_half": X.DBL_MAX,
            "dblmax_half": math.inf, "dblmax_merged": X.DBL_MAX - 2.0 ** 971, "cancel0": 5e-324,
            "cancel1": -5e-324, "cancel2": 2.0 ** -1022, "cancel3": -2.0 ** -1022, "cancel4": -1.25}
    for n in (8, 4097):
        for name, v in want.items():
            a, b = X.case(name, n)
            assert X.same_bits(X.ref_exact(a, b), v) and X.same_bits(O.xdot(a, b), v), (name, n)
            if name + "_neg" in X.NAMES:
                a, b = X.case(name + "_neg", n)
                assert X.same_bits(X.ref_exact(a, b), -v) and X.same_bits(O.xdot(a, b), -v), (name, n)
        for name in ("zeros", "zeros_mixed"):
            assert X.same_bits(O.xdot(*X.case(name, n)), 0.0)  # the bits of +0.0
        a, b = X.case("mid_ovf", n)
        assert O.xdot(a, b) == 3.0 and X.ref_exact(a, b) == 3.0
        for name in ("inf_term", "nan_term", "inf_times_0", "prod_ovf"):
            assert math.isnan(O.xdot(*X.case(name, n))), name
        assert math.isfinite(O.xdot(*X.case("prod_unf", n)))


def test_intermediate_overflow_placements():
    """family 6 wherever the two +H are put: the oracle and the rational sum say 3.0; the launch
    model confirms that the in-thread placement overflows a thread's level-0 sum"""
    n = 1280
    for plus in ((0, 256), (0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (0, 32), (0, 64), (300, 556)):
        a, b = X.intermediate(n, plus, (700, 900), 5)
        assert O.xdot(a, b) == 3.0 and X.ref_exact(a, b) == 3.0
        a, b = X.intermediate(n, plus, (700, 900), 5, h=2.0 ** 1023)
        assert O.xdot(a, b) == 3.0 and X.ref_exact(a, b) == 3.0
    a, b = X.intermediate(n, (0, 256), (700, 900), 5)
    assert X.launch_model(a, b, grid=1)[1] == 4  # H is above the threshold: each one goes to the digits
    a, b = X.intermediate(n, (0, 256), (700, 900), 5, h=2.0 ** 1023)
    assert X.launch_model(a, b, grid=1)[1] == 1  # one workgroup: elements 0 and 256 meet in thread 0
    assert X.launch_model(a, b, grid=2)[1] == 0  # two: they are in different workgroups


def test_cascade_remainder_by_construction():
    """the terms that no three-term expansion holds: with one workgroup thread 0 deposits a
    remainder; spread over five workgroups nothing is left over"""
    a, b = X.cascade_terms()
    assert X.launch_model(a, b, grid=1) == (2, 0)
    assert X.launch_model(a, b, grid=5) == (0, 0)
    assert X.launch_model(a, b, grid=1, kind=1) == (2, 0)  # tiled: 256 apart are one thread's tile
    assert X.a_applies(a, b) and X.same_bits(O.xdot(a, b), X.ref_exact(a, b))
    # the wide families leave remainders on their own at the tested sizes
    assert X.launch_model(*X.case("wide1000", 5000), grid=1)[0] > 0


def test_xnorm2_within_an_ulp_of_the_exact_root():
    """norm([a b]) of the exact mode: results in the normal range lie within 1 ulp of the correctly
    rounded sqrt(a^2 + b^2) (the figure test_oracle.py asserts against math.hypot), exact on
    Pythagorean triples, and the special values follow a + b"""
    assert X.hypot_exact(3.0, 4.0) == 5.0 and X.hypot_exact(1.0, 1.0) == math.sqrt(2.0)
    assert X.hypot_exact(X.DBL_MAX, X.DBL_MAX) == math.inf
    a, b = X.xnorm2_pairs()
    checked = 0
    for x, y in zip(a, b):
        got = O.xnorm2(x, y)
        if not (math.isfinite(x) and math.isfinite(y)):
            assert math.isnan(got) if (math.isnan(x) or math.isnan(y)) else got == math.inf
            continue
        want = X.hypot_exact(x, y)
        if 2.0 ** -1022 <= want < math.inf:
            checked += 1
            assert abs(got - want) <= math.ulp(want), (x, y, got, want)
        elif want == 0.0:
            assert X.same_bits(got, 0.0)
    assert checked > 4000
    assert O.xnorm2(-5.0, 12.0) == 13.0 and O.xnorm2(8.0, -15.0) == 17.0 and O.xnorm2(0.0, -2.5) == 2.5


# ---- the two diagnostic entries: arguments refused before any device call ------------------------
def test_debug_entries_refuse_bad_arguments():
    L = _lib.lib
    for n in ("cpk_debug_dot", "cpk_debug_xnorm2"):
        assert hasattr(L, n) and n in _lib.EXPORTED
    assert L.cpk_abi_version() == 3
    a, b, out = np.ones(8), np.full(8, 2.0), np.full(4, 7.0)
    pa, pb, po = (v.ctypes.data_as(PD) for v in (a, b, out))
    h = C.c_void_p(a.ctypes.data)  # stands for a context; never dereferenced
    ok = dict(ctx=h, kind=0, n=4, nv=2, A=pa, lda=4, B=pb, ldb=4, grid=0, out=po)
    bad = [dict(ctx=None), dict(A=None), dict(B=None), dict(out=None), dict(nv=0), dict(nv=3), dict(nv=5), dict(nv=8),
           dict(nv=-1), dict(lda=3), dict(ldb=3), dict(kind=2), dict(kind=-1), dict(n=-1), dict(grid=-1)]
    for d in bad:
        v = dict(ok, **d)
        rc = L.cpk_debug_dot(v["ctx"], v["kind"], v["n"], v["nv"], v["A"], v["lda"], v["B"], v["ldb"], v["grid"], v["out"])
        assert rc == _lib.CPK_ERR_ARGS, d
        assert L.cpk_last_error()
    for args in ((None, 4, pa, pb, po), (h, 4, None, pb, po), (h, 4, pa, None, po), (h, 4, pa, pb, None),
                 (h, -1, pa, pb, po)):
        assert L.cpk_debug_xnorm2(*args) == _lib.CPK_ERR_ARGS
    assert np.all(a == 1.0) and np.all(b == 2.0) and np.all(out == 7.0)  # nothing written
    # cpk_debug_arnoldi_step: N = 4, n = 2, restart / mem = 2; V, PV: 4 x 3; H: 16 fits both layouts
    assert hasattr(L, "cpk_debug_arnoldi_step") and "cpk_debug_arnoldi_step" in _lib.EXPORTED
    arrs = {k: np.full(sz, 3.0) for k, sz in (("V", 12), ("PV", 12), ("xy", 4), ("w", 4), ("ut", 4), ("H", 16), ("c", 2),
                                              ("s", 2), ("g", 3), ("H_dots", 16))}
    GM, DQ = _lib.METHODS["gmres"], _lib.METHODS["dqgmres"]
    ok = dict(method=DQ, running=1, grid=0, n=2, N=4, win=2, kk=2, itmax=10, stopTol=1.0, residNorm=2.0, hk1=5.0,
              hist=6.0, ldv=4, ldpv=4, stop=-3, err=-3, err_val=-3.0, err_iter=-3, nh=-3,
              **{k: v.ctypes.data_as(PD) for k, v in arrs.items()})
    bad = [dict(method=0), dict(method=6), dict(V=None), dict(w=None), dict(ut=None), dict(H=None), dict(c=None),
           dict(s=None), dict(g=None), dict(PV=None), dict(xy=None), dict(N=-1), dict(n=-1), dict(n=5), dict(kk=0),
           dict(kk=-1), dict(win=0), dict(win=-1), dict(grid=-1), dict(ldv=3), dict(ldpv=3),
           dict(method=GM, kk=3), dict(method=GM, win=0, kk=1), dict(method=GM, ldv=3), dict(method=GM, V=None)]
    for d in bad:
        io = _lib.ArnoldiStep(**dict(ok, **d))
        assert L.cpk_debug_arnoldi_step(h, C.byref(io)) == _lib.CPK_ERR_ARGS, d
        assert L.cpk_last_error()
        assert (io.stop, io.err, io.err_val, io.err_iter, io.nh, io.hk1, io.hist) == (-3, -3, -3.0, -3, -3, 5.0, 6.0)
    assert L.cpk_debug_arnoldi_step(None, C.byref(_lib.ArnoldiStep(**ok))) == _lib.CPK_ERR_ARGS
    assert L.cpk_debug_arnoldi_step(h, None) == _lib.CPK_ERR_ARGS
    assert all(np.all(v == 3.0) for v in arrs.values())  # nothing written
