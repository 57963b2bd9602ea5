"""Whole cpgmres / cpdqgmres solves under engine option basis_f32 against the reference loops of
arnoldi_f32_ref.py with rd = f32 (pinned to the oracle by test_arnoldi_f32_ref_host.py), on the
product's exported factors, where M*z is the oracle's bit for bit.

  exact mode      niters, solved, history, x and y == the reference, on tiny3x2, tiny65x63 and cvxqp2_s,
                  cpdqgmres with mem = 5 (the ring wraps) and 40, cpgmres with restart = 20 (several
                  cycles) and 100; and where the reference stops with its error (a negative squared
                  norm of the unrounded new vector), the device stops at the same iteration.
  default mode    the project's band (FLOOR, SAFETY) around the reference, the band being the
                  reference's own spread under 1e-15 perturbations of the rhs, on cases whose
                  iteration count that does not move (checked on the CPU).
  the loop        no_graph on and off, batch = 1 against the default: the same bits (the vector under
                  construction and the product's input sit at fixed addresses).
  the operator    cpk.Operator around cpk_mat_spmv_device equals the matrix solve bit for bit.
  elsewhere       the other four methods and a cpminres block do not see the option; basis_f32 = 0
                  set explicitly is the default context.
  K.solve         reports the true residual of the x it returns.
  refusal         a dist1 context refuses both methods with CPK_ERR_UNSUPPORTED and writes nothing."""
import numpy as np
import pytest

import arnoldi_f32_ref as RF
import basis_f32_cases as BC
import xacc_cases as X
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_HANDLES = {}


def handles(name):
    """(A, C as Matrix handles, M with the example's properties, its factors), built once on the
    session's default context"""
    import cpkrylov_amd as cpk
    if name not in _HANDLES:
        S, _ = BC.system(name)
        M = cpk.opLDL2(S["G"], S["B"], -S["C"])
        M._set(**{k: BC.F.EXPROG_OPTS[k] for k in BC.PC_PROPS})
        Am, Cm = cpk.Matrix(S["Q"], M.ctx), cpk.Matrix(S["C"], M.ctx)
        Am @ np.zeros(S["n"])  # the device copy exists before any capture calls the SpMV
        _HANDLES[name] = (Am, Cm, M, M.export_factors())
    return _HANDLES[name]


def solve(name, method, window, A=None, itmax=BC.ITMAX, **options):
    """cp<method> on the system's column under the given engine options"""
    import cpkrylov_amd as cpk
    Am, Cm, M, _ = handles(name)
    _, b = BC.system(name)
    with cpk.engine_options(**options):
        return getattr(cpk, "cp" + method)(b, Am if A is None else A, Cm, M, BC.opts(method, window, itmax=itmax))


_REF = {}


def reference(name, method, window):
    """the reference loop with rd = f32 on the product's factors, in exact mode, computed once"""
    key = (name, method, window)
    if key not in _REF:
        S, b = BC.system(name)
        Sy = BC.ref_system(S, BC.oracle_M(S, handles(name)[3]), rational=S["N"] <= 8)
        with O.exact():
            _REF[key] = RF.solve(method, Sy, b, window, rd=RF.f32)
    return _REF[key]


_F32 = {}


def f32_exact(name, method, window):
    """the device's exact-mode solve with the option on, computed once"""
    key = (name, method, window)
    if key not in _F32:
        _F32[key] = solve(name, method, window, exact_dots=1, basis_f32=1)
    return _F32[key]


def assert_same_bits(got, want, what):
    (x, y, st, fl), (xo, yo, so, fo) = got, want
    assert st["niters"] == so["niters"] and fl["solved"] == fo["solved"], (what, st["niters"], so["niters"])
    h, ho = st["residHistory"], so["residHistory"]
    assert len(h) == len(ho), what
    bad = np.flatnonzero(X.bits(h) != X.bits(ho))
    assert bad.size == 0, (what, bad[:5], h[bad[:3]], ho[bad[:3]])
    assert X.same_bits(x, xo) and X.same_bits(y, yo), (what, np.max(np.abs(x - xo)), np.max(np.abs(y - yo)))


CASES = [(n, m, w) for n in BC.GPU_SYSTEMS for m, w in BC.WINDOWS]


# ---- 1. exact mode, bit for bit the reference ----------------------------------------------------------
@pytest.mark.parametrize("name,method,window", CASES)
def test_exact_mode_is_the_reference(gpu_ctx, name, method, window):
    xo, yo, so = reference(name, method, window)
    got = f32_exact(name, method, window)
    assert_same_bits(got, (xo, yo, so, dict(solved=so["solved"])), (name, method, window))
    if name == "cvxqp2_s":
        assert so["niters"] > {5: 12, 40: 82, 20: 60, 100: 100}[window]  # wraps / cycles happened
        dbl = solve(name, method, window, exact_dots=1)
        assert not X.same_bits(dbl[2]["residHistory"], got[2]["residHistory"])  # the option did something


def test_the_references_error_arrives_at_the_same_iteration(gpu_ctx):
    """cpdqgmres(5) on cvxqp2_s does not converge; with the float basis the squared norm of the
    (unrounded) new vector turns negative.  The device stops where the reference stops, with its
    value."""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    name, method, window, itmax, it = BC.ERROR_CASE
    S, b = BC.system(name)
    Sy = BC.ref_system(S, BC.oracle_M(S, handles(name)[3]), itmax=itmax)
    with O.exact(), pytest.raises(RF.Indefinite) as ref:
        RF.solve(method, Sy, b, window, rd=RF.f32)
    assert ref.value.iter == it and ref.value.val < 0
    with pytest.raises(cpk.CpkError) as dev:
        solve(name, method, window, itmax=itmax, exact_dots=1, basis_f32=1)
    assert dev.value.code == _lib.CPK_ERR_INDEFINITE
    assert f"Iter {it}: negative squared norm {ref.value.val:g}" in str(dev.value), (str(dev.value), ref.value.val)
    x, y, st, fl = solve(name, method, window, itmax=itmax, exact_dots=1)  # the double basis runs on
    assert st["niters"] == itmax and not fl["solved"]


# ---- 2. default mode: the band around the reference ------------------------------------------------------
@pytest.mark.parametrize("name,method,window", BC.DEFAULT_CASES)
def test_default_mode_in_band(gpu_ctx, name, method, window):
    bd = BC.band(name, method, window, factors=handles(name)[3])
    assert bd["stable"], (name, method, window, bd["niters"])  # (the CPU test checks it on the oracle's own factors)
    xo, yo, so = bd["ref"]
    x, y, st, fl = solve(name, method, window, basis_f32=1)
    what = (name, method, window)
    assert st["niters"] == so["niters"] and fl["solved"] == so["solved"], (what, st["niters"], so["niters"])
    h, ho = st["residHistory"], so["residHistory"]
    assert len(h) == len(ho), what
    dev = float(np.max(np.abs(h - ho)) / ho[0])
    z, zo = np.concatenate([x, y]), np.concatenate([xo, yo])
    dx = float(np.linalg.norm(z - zo) / np.linalg.norm(zo))
    print(what, "history", dev, "band", bd["hist"], "x", dx, "band", bd["x"])
    assert dev <= max(BC.FLOOR, BC.SAFETY * bd["hist"]), (what, dev, bd["hist"])
    assert dx <= max(BC.FLOOR, BC.SAFETY * bd["x"]), (what, dx, bd["x"])


# ---- 3. the bits do not depend on how the loop runs ---------------------------------------------------------
@pytest.mark.parametrize("exact", (1, 0), ids=("exact", "default"))
@pytest.mark.parametrize("method,window", (("dqgmres", 5), ("gmres", 20)))
def test_loop_shape_changes_no_bit(gpu_ctx, method, window, exact):
    """graph replay against eager launches, batches of one iteration against the default: VNEW and
    VCUR are at fixed addresses, so a captured batch replays what an eager one runs"""
    name = "cvxqp2_s"
    base = solve(name, method, window, exact_dots=exact, basis_f32=1)
    for extra in (dict(no_graph=1), dict(batch=1), dict(no_graph=1, batch=1)):
        got = solve(name, method, window, exact_dots=exact, basis_f32=1, **extra)
        assert_same_bits(got, base, (method, window, exact, extra))
    again = solve(name, method, window, exact_dots=exact, basis_f32=1)  # the cached solver, replayed
    assert_same_bits(again, base, (method, window, exact, "second call"))


# ---- 4. the operator-valued A ---------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", (True, False), ids=("capturable", "eager"))
@pytest.mark.parametrize("method,window", (("dqgmres", 5), ("gmres", 20)))
def test_operator_equals_matrix_path(gpu_ctx, method, window, capturable):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    name = "cvxqp2_s"
    Am = handles(name)[0]
    A = cpk.Operator(Am.shape[0], lambda x, y, n, stream: _lib.lib.cpk_mat_spmv_device(Am.h, x, y), ctx=Am.ctx,
                     capturable=capturable)
    got = solve(name, method, window, A=A, exact_dots=1, basis_f32=1)
    assert_same_bits(got, f32_exact(name, method, window), (method, window, capturable))


# ---- 5. the option is invisible elsewhere ------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("cg", "cglanczos", "minres", "symmlq"))
def test_other_methods_do_not_see_the_option(gpu_ctx, method):
    import cpkrylov_amd as cpk
    name = "cvxqp2_s"
    Am, Cm, M, _ = handles(name)
    _, b = BC.system(name)
    opts = dict(BC.F.EXPROG_OPTS, itmax=100)
    off = getattr(cpk, "cp" + method)(b, Am, Cm, M, opts)
    with cpk.engine_options(basis_f32=1):
        on = getattr(cpk, "cp" + method)(b, Am, Cm, M, opts)
    assert on[2]["niters"] == off[2]["niters"] and on[3] == off[3]
    for k in off[2]:
        if k.endswith("History"):
            assert X.same_bits(on[2][k], off[2][k]), (method, k)
    assert X.same_bits(on[0], off[0]) and X.same_bits(on[1], off[1])


def test_block_solve_and_apply_do_not_see_the_option(gpu_ctx):
    import cpkrylov_amd as cpk
    name = "cvxqp2_s"
    Am, Cm, M, _ = handles(name)
    S, b = BC.system(name)
    Bk = np.asfortranarray(np.column_stack([b, 1e-3 * b, np.random.default_rng(3).standard_normal(S["n"])]))
    z = np.random.default_rng(4).standard_normal(S["N"])
    off, zoff = cpk.cpminres(Bk, Am, Cm, M, dict(BC.F.EXPROG_OPTS)), M * z
    with cpk.engine_options(basis_f32=1):
        on, zon = cpk.cpminres(Bk, Am, Cm, M, dict(BC.F.EXPROG_OPTS)), M * z
    assert X.same_bits(on[0], off[0]) and X.same_bits(on[1], off[1]) and X.same_bits(zon, zoff)
    for so, sf in zip(on[2], off[2]):
        assert so["niters"] == sf["niters"] and X.same_bits(so["residHistory"], sf["residHistory"])


def test_explicit_zero_is_the_default(gpu_ctx):
    name, method, window = "cvxqp2_s", "dqgmres", 40
    assert gpu_ctx.get_option("basis_f32") == "0"
    base = solve(name, method, window)
    assert_same_bits(solve(name, method, window, basis_f32=0), base, "basis_f32=0")
    on = solve(name, method, window, basis_f32=1)  # (a cached double solver is not reused for it, nor the reverse)
    assert not X.same_bits(on[2]["residHistory"], base[2]["residHistory"])
    assert_same_bits(solve(name, method, window), base, "after a compressed solve")


# ---- 6. K.solve ------------------------------------------------------------------------------------------------------
def test_kkt_solve_reports_the_true_residual(gpu_ctx):
    import cpkrylov_amd as cpk
    name = "cvxqp2_s"
    S, _ = BC.system(name)
    Am, Cm, M, _ = handles(name)
    Bm = cpk.Matrix(S["B"], M.ctx)
    K = cpk.KKT(Am, Bm, Cm)
    b = S["rhs"].copy()
    opts = BC.opts("dqgmres", 40)
    with cpk.engine_options(basis_f32=1):
        x, stats, flag = K.solve("dqgmres", b, M, opts)
        _, norms = K.residual(x, b, want_r=False)
    xd, sd, fd = K.solve("dqgmres", b, M, opts)
    assert not X.same_bits(x, xd)  # K.solve inherited the option
    for k in ("rr_x", "rr_y", "bb_x", "bb_y", "rnorm", "bnorm"):
        assert X.same_bits(stats["true_resid"][k], norms[k]), k
    print("K.solve dqgmres(40) cvxqp2_s: true relative residual, float basis",
          stats["true_resid"]["rnorm"] / stats["true_resid"]["bnorm"], "double basis",
          sd["true_resid"]["rnorm"] / sd["true_resid"]["bnorm"], "niters", stats["niters"], sd["niters"])


# ---- 7. refusal -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
def test_distributed_context_is_refused(method):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    S, b = BC.system("cvxqp2_s")
    group = cpk.SimGroup(1)  # a 1-rank communicator; dist1 makes it run the distributed path
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=group, options=dict(dist1=1, basis_f32=1))
    try:
        assert ctx.info()["distributed"]
        M = cpk.opLDL2(S["G"], S["B"], -S["C"], ctx=ctx)
        Am, Cm = cpk.Matrix(S["Q"], ctx), cpk.Matrix(S["C"], ctx)
        with pytest.raises(cpk.CpkError) as e:
            getattr(cpk, "cp" + method)(b, Am, Cm, M, BC.opts(method, 5))
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED and "basis_f32" in str(e.value)
        # the outputs of the C entry are untouched
        import ctypes as C
        from cpkrylov_amd.api import _dptr, _hist_cap, _new_stats
        from cpkrylov_amd._lib import make_opts
        x, y = np.full(S["n"], -7.5), np.full(S["m"], -7.5)
        st, hist, lq, qr = _new_stats(_hist_cap(method, BC.opts(method, 5), S["n"], S["m"]))
        hist[:] = -7.5
        rc = _lib.lib.cpk_method_solve(ctx.h, _lib.METHODS[method], _dptr(b), Am.h, Cm.h, M.h,
                                       C.byref(make_opts(BC.opts(method, 5))), _dptr(x), _dptr(y), C.byref(st))
        assert rc == _lib.CPK_ERR_UNSUPPORTED
        assert np.all(x == -7.5) and np.all(y == -7.5) and np.all(np.asarray(hist) == -7.5)
        ctx.set_option("basis_f32", 0)  # the same context solves once the option is off
        xs, ys, ss, fs = getattr(cpk, "cp" + method)(b, Am, Cm, M, BC.opts(method, 5, itmax=20))
        assert ss["niters"] == 20 and np.all(np.isfinite(xs))
    finally:
        ctx.close()
