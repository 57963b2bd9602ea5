"""The refined solve (cpk_kkt_solve_refined, KKT.solve_refined) on the GPU: max_steps = 0 is the
cold K.solve bit for bit; a call equals the caller's own loop of K.residual_exact, K.solve on r and
one addition, with == in x and in every row of resid_sums, for all six methods; the forward error
against an mpmath solution falls as the CPU oracle says it does; a trial whose residual does not
decrease is dropped; a stop inside the driver comes back with the driver's code."""
import os

import numpy as np
import pytest

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import fixtures as F
import kkt_ref as R
import resid_exact_ref as E
import structures as S

pytestmark = pytest.mark.gpu

PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
KEYS = ("rr_x", "rr_y", "bb_x", "bb_y")
_GOLD = {}


def _gold():
    if not _GOLD:
        _GOLD.update(np.load(os.path.join(F.GOLDEN, "cvxqp1_m_refine.npz")))
    return _GOLD


def _setup(P, ctx, opts):
    import cpkrylov_amd as cpk
    K = cpk.KKT(P["A"] if "A" in P else P["Q"], P["B"], P["C"], ctx=ctx)
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=ctx)
    M._set(**{k: opts[k] for k in PC_PROPS if k in opts})
    return K, M


def _row(nr):
    return np.array([nr[k] for k in KEYS], dtype=np.float64)


def _same_run(stats, flag, so, fo):
    assert stats["niters"] == so["niters"] and flag["solved"] == fo["solved"]
    for k in [k for k in so if k.endswith("History")]:
        assert E.same(stats[k], so[k]), k


def _callers_loop(K, method, b, M, opts, x0, max_steps):
    """cpk_kkt_solve_refined's loop through the public pieces: K.residual_exact, the cold K.solve on
    r, one addition.  Returns (x, rows, refine_steps, (stats, flag) of the last call, the error)"""
    import cpkrylov_amd as cpk
    x = np.zeros(K.N) if x0 is None else np.array(x0, dtype=np.float64)
    r, nr = K.residual_exact(x, b)
    rows, taken, last = [_row(nr)], 0, None
    for j in range(max_steps + 1):
        try:
            dx, st, fl = K.solve(method, r, M, opts)
            last = (st, fl)
        except cpk.CpkError as e:
            return x + e.partial[0], rows, taken, last, e
        trial = x + dx
        if j == max_steps:
            x, taken = trial, taken + 1
            break
        r, nr = K.residual_exact(trial, b)
        rows.append(_row(nr))
        if not rows[-1][0] + rows[-1][1] < rows[-2][0] + rows[-2][1]:
            break  # the trial is dropped
        x, taken = trial, taken + 1
    return x, rows, taken - 1, last, None


@pytest.mark.parametrize("name,method,extra", [("cvxqp1_m", "minres", {}), ("cvxqp2_s", "gmres", {"restart": 20})])
def test_max_steps_zero_is_the_cold_solve(gpu_ctx, name, method, extra):
    P = R.system(name)
    opts = dict(F.EXPROG_OPTS, **extra)
    K, M = _setup(P, gpu_ctx, opts)
    x, stats, flag = K.solve(method, P["rhs"], M, opts)
    xr, sr, fr = K.solve_refined(method, P["rhs"], M, opts, max_steps=0)
    assert E.same(xr, x)
    _same_run(sr, fr, stats, flag)
    assert sr["true_resid"] == stats["true_resid"] and sr["true_resid0"] == stats["true_resid0"]
    assert sr["refine_steps"] == 0 and sr["resid_sums"].shape == (1, 4)
    assert E.same(sr["resid_sums"][0], _row(stats["true_resid0"]))


LOOP_CASES = [("cvxqp1_m", "minres", {}, None, 2), ("cvxqp1_m", "minres", {}, 0.9, 1), ("cvxqp2_s", "gmres", {"restart": 20}, None, 2)]
LOOP_CASES += [("tiny65x63", m, extra, None, 2) for m, extra in S.SOLVE_METHODS]


@pytest.mark.parametrize("name,method,extra,warm,steps", LOOP_CASES)
def test_equals_the_callers_loop(gpu_ctx, name, method, extra, warm, steps):
    """exact_dots on: x, every row of resid_sums, refine_steps and the last call's run equal the
    loop of residual_exact, the driver on r from zero, and one addition (all six methods; cold, and
    warm from 0.9 of the cold solution)"""
    import cpkrylov_amd as cpk
    P = R.system(name)
    opts = dict(F.EXPROG_OPTS, **extra)
    b = P["rhs"]
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        K, M = _setup(P, gpu_ctx, opts)
        x0 = None if warm is None else warm * K.solve(method, b, M, opts)[0]
        x0_in = None if x0 is None else x0.copy()
        xl, rows, nsteps, last, err = _callers_loop(K, method, b, M, opts, x0, steps)
        if err is not None:
            with pytest.raises(cpk.CpkError) as e:
                K.solve_refined(method, b, M, opts, x0=x0, max_steps=steps)
            assert e.value.code == err.code and E.same(e.value.partial[0], xl)
            return
        x, stats, flag = K.solve_refined(method, b, M, opts, x0=x0, max_steps=steps)
        plain = K.residual(x, b, want_r=False)[1]
    assert E.same(x, xl), np.flatnonzero(x != xl)[:5]
    assert stats["refine_steps"] == nsteps and stats["resid_sums"].shape == (len(rows), 4)
    for j, row in enumerate(rows):
        assert E.same(stats["resid_sums"][j], row), j
    _same_run(stats, flag, *last)
    assert stats["true_resid"] == plain
    if x0 is not None:
        assert E.same(x0, x0_in)  # the caller's x0 is not written
    if nsteps == steps:
        assert len(rows) == steps + 1


def test_device_tensors_equal_the_host_entry(gpu_ctx):
    """cpk_kkt_solve_refined_device through the Python front end: b a device tensor, the result in
    out=, cold and warm with x0 = out updated in place; x, refine_steps, resid_sums, true_resid and
    the run equal the host entry's with ==; b is not written"""
    import cpkrylov_amd as cpk
    assert torch is not None and torch.cuda.is_available()
    P = R.system("cvxqp1_m")
    opts = dict(F.EXPROG_OPTS, atol=0.0)
    K, M = _setup(P, gpu_ctx, opts)
    b = P["rhs"]
    tb = torch.from_numpy(b.copy()).cuda()
    out = torch.full((K.N,), 7.0, dtype=torch.float64, device="cuda")
    xh, sh, fh = K.solve_refined("minres", b, M, opts, max_steps=2)
    xd, sd, fd = K.solve_refined("minres", tb, M, opts, max_steps=2, out=out)
    assert xd is out and E.same(out.cpu().numpy(), xh)
    assert sd["refine_steps"] == sh["refine_steps"] and E.same(sd["resid_sums"], sh["resid_sums"])
    assert sd["true_resid"] == sh["true_resid"]
    _same_run(sd, fd, sh, fh)
    # warm, in place from 0.9 x
    out.mul_(0.9)
    torch.cuda.synchronize()
    x0 = out.cpu().numpy()
    xw, sw, fw = K.solve_refined("minres", b, M, opts, x0=x0, max_steps=1)
    xo, so, fo = K.solve_refined("minres", tb, M, opts, x0=out, max_steps=1, out=out)
    assert xo is out and E.same(out.cpu().numpy(), xw) and not E.same(xw, x0)
    assert so["refine_steps"] == sw["refine_steps"] and E.same(so["resid_sums"], sw["resid_sums"])
    assert so["true_resid"] == sw["true_resid"]
    _same_run(so, fo, sw, fw)
    assert E.same(tb.cpu().numpy(), b)
    with pytest.raises(cpk.CpkError):  # x0 must be out itself
        K.solve_refined("minres", tb, M, opts, x0=torch.zeros_like(out), max_steps=1, out=out)
    with pytest.raises(cpk.CpkError):
        K.solve_refined("minres", tb, M, opts, max_steps=1)


def _forward_error(x):
    g = _gold()
    return float(np.linalg.norm((x - g["xstar_hi"]) - g["xstar_lo"]) / np.linalg.norm(g["xstar_hi"]))


# (options beside the example's, half the oracle's gain over the cold solve, half its gain over the plain restarts)
GAIN_CASES = {"example": ({}, 0.5 * 4.455918e-07 / 2.216162e-09, None),
              "atol0": ({"atol": 0.0}, 0.5 * 4.455918e-07 / 3.139598e-17, 0.5 * 1.399716e-15 / 3.139598e-17)}


@pytest.mark.parametrize("tag", sorted(GAIN_CASES))
def test_refinement_gain(gpu_ctx, tag):
    """cvxqp1_m (cond_2(K) = 2.0e7), cpminres, forward error |x - x*| / |x*| against the mpmath
    solution of the same double-precision K and b (tests/golden/make_refine_golden.py, which also
    measured the figures below with the CPU oracle alone, on the product's factors, exact dots).

    example options (atol = rtol = 1e-6):  cold 4.455918e-07;  solve_refined(max_steps=3)
        2.216162e-09 (iterates 4.456e-07, 2.2161616435e-09, 2.2161616418e-09, 2.2161616402e-09);
        three plain warm restarts 2.2161614843e-09, 2.2161660486e-09, 2.2161622050e-09.
        The gain over the cold solve is 201; after the first correction every driver call stops at
        once on atol (0 iterations), so both legs stall at 2.2162e-09 and differ in the 7th digit.
    atol = 0 (rtol = 1e-6 alone, so that a call on a small residual still iterates):  cold
        4.455918e-07;  solve_refined(max_steps=3) 3.139598e-17 (iterates 4.456e-07, 2.703e-13,
        3.1396e-17, 3.1396e-17);  three plain warm restarts 2.706e-13, 1.535e-15, 1.400e-15: the
        plain residual stalls at eps * cond-free level 1.4e-15, the exactly rounded one reaches the
        correctly rounded solution, a gain of 44.6 over the plain restarts and 1.4e10 over the cold solve.
    No rescaling of C was needed (factor 1).  Asserted: the refined error is below the cold solve's
    by at least half the oracle's gain, not above the three plain warm restarts' and, with atol = 0,
    below theirs by at least half the oracle's gain of 44.6."""
    import cpkrylov_amd as cpk
    extra, half_gain_cold, half_gain_plain = GAIN_CASES[tag]
    P = R.system("cvxqp1_m")
    opts = dict(F.EXPROG_OPTS, **extra)
    b = P["rhs"]
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        K, M = _setup(P, gpu_ctx, opts)
        x_cold = K.solve("minres", b, M, opts)[0]
        x_ref, stats, _ = K.solve_refined("minres", b, M, opts, max_steps=3)
        x_plain = x_cold
        for _ in range(3):
            x_plain = K.solve("minres", b, M, opts, x0=x_plain)[0]
    e_cold, e_ref, e_plain = _forward_error(x_cold), _forward_error(x_ref), _forward_error(x_plain)
    print(f"{tag}: forward errors cold {e_cold:.6e} refined {e_ref:.6e} plain restarts {e_plain:.6e}; "
          f"refine_steps {stats['refine_steps']}, sum r^2 {stats['resid_sums'][:, :2].sum(axis=1)}")
    assert e_ref < e_cold and e_ref * half_gain_cold <= e_cold
    assert e_ref <= e_plain
    if half_gain_plain is not None:
        assert e_ref * half_gain_plain <= e_plain


def test_a_trial_that_does_not_decrease_is_dropped(gpu_ctx):
    """exact_dots on (so that the CPU oracle predicts the run).  Example options, max_steps = 6:
    from the second correction on every driver call stops at once on atol and the residual stalls;
    the fourth trial's does not decrease, that dx is not applied and refine_steps says 2.  With
    rtol = 0.5 the cold call's own trial (one iteration) has a larger residual than b: it is
    dropped, x is zero and refine_steps is -1."""
    import cpkrylov_amd as cpk
    P = R.system("cvxqp1_m")
    b = P["rhs"]
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        opts = dict(F.EXPROG_OPTS)
        K, M = _setup(P, gpu_ctx, opts)
        x, stats, _ = K.solve_refined("minres", b, M, opts, max_steps=6)
        xl, rows, nsteps, _, err = _callers_loop(K, "minres", b, M, opts, None, 6)
        assert err is None and E.same(x, xl) and stats["refine_steps"] == nsteps
        rr = stats["resid_sums"][:, :2].sum(axis=1)
        print("sum r^2 per residual formed:", rr, "refine_steps", stats["refine_steps"])
        assert 0 <= nsteps < 6 and len(rr) == nsteps + 3 == len(rows)
        assert np.all(rr[1:-1] < rr[:-2]) and not rr[-1] < rr[-2]
        # the returned x is the iterate before the dropped trial: its exact residual is the row before the last
        assert E.same(_row(K.residual_exact(x, b)[1]), stats["resid_sums"][-2])
        loose = dict(opts, rtol=0.5, atol=0.0)
        x, stats, _ = K.solve_refined("minres", b, M, loose, max_steps=2)
        rr = stats["resid_sums"][:, :2].sum(axis=1)
        assert stats["refine_steps"] == -1 and not np.any(x) and len(rr) == 2 and not rr[1] < rr[0]


def test_driver_error_returns_the_drivers_code(gpu_ctx):
    """structures.tiny_indefinite under exact_dots: the oracle's methods stop with the indefinite
    error, so does K.solve, and solve_refined returns that code and message; x is x_j plus whatever
    the driver wrote (cold: K.solve's partial), and the residuals formed so far are reported"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P = S.tiny_indefinite()
    opts = dict(F.EXPROG_OPTS)
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        K, M = _setup(P, gpu_ctx, opts)
        with pytest.raises(cpk.IndefiniteError) as e0:
            K.solve("minres", P["rhs"], M, opts)
        with pytest.raises(cpk.IndefiniteError) as e:
            K.solve_refined("minres", P["rhs"], M, opts, max_steps=2)
        assert e.value.code == e0.value.code == _lib.CPK_ERR_INDEFINITE and str(e.value) == str(e0.value)
        xp, rows = e.value.partial
        assert E.same(xp, e0.value.partial[0]) and rows.shape == (1, 4)
        assert E.same(rows[0], e0.value.partial[1][:4])
        x0 = np.zeros(K.N)
        x0[0] = 2.0 ** -60
        r, nr = K.residual_exact(x0, P["rhs"])
        with pytest.raises(cpk.IndefiniteError) as er:
            K.solve("minres", r, M, opts)
        with pytest.raises(cpk.IndefiniteError) as ew:
            K.solve_refined("minres", P["rhs"], M, opts, x0=x0, max_steps=2)
        assert ew.value.code == er.value.code and str(ew.value) == str(er.value)
        assert E.same(ew.value.partial[0], x0 + er.value.partial[0]) and E.same(ew.value.partial[1][0], _row(nr))


def test_refusals(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P = R.system("tiny65x63")
    opts = dict(F.EXPROG_OPTS)
    K, M = _setup(P, gpu_ctx, opts)
    with pytest.raises(cpk.CpkError) as e:
        K.solve_refined("minres", P["rhs"], M, opts, max_steps=-1)
    assert e.value.code == _lib.CPK_ERR_ARGS
    with pytest.raises(cpk.CpkError) as e:
        K.solve_refined("minres", P["rhs"][:-1], M, opts)
    assert e.value.code == _lib.CPK_ERR_DIM
    with pytest.raises(cpk.CpkError) as e:
        K.solve_refined("nosuch", P["rhs"], M, opts)
    assert e.value.code == _lib.CPK_ERR_ARGS
    import ctypes as C
    x, steps = np.full(K.N, 4.25), C.c_int(-7)
    pd = C.POINTER(C.c_double)
    rc = _lib.lib.cpk_kkt_solve_refined(K.h, _lib.METHODS["minres"], P["rhs"].ctypes.data_as(pd), M.h,
                                        C.byref(_lib.make_opts(opts)), x.ctypes.data_as(pd), 0, -1, None, None, C.byref(steps))
    assert rc == _lib.CPK_ERR_ARGS and np.all(x == 4.25) and steps.value == -7
    # a preconditioner of other dimensions: refused by the driver's checks, the caller's x as it was
    _, M2 = _setup(R.system("tiny3x2"), gpu_ctx, opts)
    rc = _lib.lib.cpk_kkt_solve_refined(K.h, _lib.METHODS["minres"], P["rhs"].ctypes.data_as(pd), M2.h,
                                        C.byref(_lib.make_opts(opts)), x.ctypes.data_as(pd), 0, 2, None, None, C.byref(steps))
    assert rc != _lib.CPK_OK and np.all(x == 4.25) and steps.value == -7
