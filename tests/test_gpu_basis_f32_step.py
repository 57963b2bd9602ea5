"""One Arnoldi step through cpk_debug_arnoldi_step under engine option basis_f32 (the float
instantiations of arnoldi_dots_kernel, arnoldi_dots_exact_kernel, ArnoldiOrth, GmresNormalize and
DqgmresDirection) against the reference with rd = f32 (arnoldi_f32_ref.py, pinned to the oracle by
test_arnoldi_f32_ref_host.py).

The entry rounds the caller's V and PV to float on upload and returns the rings as doubles, so the
reference starts from the float image of the same arrays, and whole arrays are compared: every slot
the step does not write comes back as its float image, every other array as it went in.  The rule per
mode is test_gpu_arnoldi_step.py's: exact mode bit for bit in every output; default mode the window
sums within their bound, two calls the same bits, and everything downstream of the device's own sums
and H(k+1, k) bit for bit.

Shapes: the float dots tile is F32_TILE x kBlock elements, read from the library's sources; a slot's stride
is padded to 64 floats, so N = 1, 2, 63, 64, 65 and odd N put slots at padded strides."""
import math

import numpy as np
import pytest

import arnoldi_f32_ref as RF
import arnoldi_ref as R
import test_gpu_arnoldi_step as T
import xacc_cases as X

pytestmark = pytest.mark.gpu



def _dots_tile():
    """(threads per workgroup, elements per thread and step) of the float dots kernel, as the library's
    sources define them: kBlock in devutil.hpp, CPK_DOT_TILE and CPK_DOT_TILE_F32 in solvers.hip (the
    Makefile passes neither on its command line)"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpkrylov_amd", "csrc")
    hip = open(os.path.join(csrc, "solvers.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "CPK_DOT_TILE" not in mk
    tile = int(re.search(r"^#define CPK_DOT_TILE (\d+)$", hip, re.M).group(1))
    f32 = re.search(r"^#define CPK_DOT_TILE_F32 \((.+)\)$", hip, re.M).group(1)
    f32 = int(eval(f32, {"__builtins__": {}}, {"CPK_DOT_TILE": tile}))
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(csrc, "devutil.hpp")).read()).group(1))
    assert 2 <= f32 <= 16 and block in (64, 128, 256, 512, 1024)
    return block, f32


KBLOCK, F32_TILE = _dots_tile()
TILE = KBLOCK * F32_TILE
BIG = 2 * TILE + 515  # an odd N above the tile: two full tiles and a partial one


@pytest.fixture(scope="module")
def fctx():
    """contexts of their own with the option on: exact mode and default mode"""
    import cpkrylov_amd as cpk
    ctxs = {1: cpk.Context(options=dict(exact_dots=1, basis_f32=1)), 0: cpk.Context(options=dict(basis_f32=1))}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(params=(1, 0), ids=("exact", "default"))
def mode(request, fctx):
    return fctx[request.param], request.param


def image(A):
    """the arrays as the entry holds them after the upload: V and PV rounded to float"""
    return dict(A, V=np.asfortranarray(RF.f32(A["V"])), PV=np.asfortranarray(RF.f32(A["PV"])))


def run_ref(S, A, hwin=None, hk1=None, rational=False):
    """test_gpu_arnoldi_step.run_ref on the float image, with the stores through f32"""
    A = image(A)
    dq = S["method"] == "dqgmres"
    out = {k: np.array(A[k], order="F", copy=True) for k in T.ARRAYS}
    St = dict(S, **{("mem" if dq else "restart"): S["win"]})
    if dq:
        H = R.unpack_hd(out["H"], S["win"], S["kk"])
        r = RF.dqgmres_step(St, out["V"], out["PV"], out["xy"], A["w"], A["ut"], H, out["c"], out["s"], out["g"],
                            rd=RF.f32, hwin=hwin, hk1=hk1, rational=rational)
        out["H"] = R.pack_hd(H, S["win"])
    else:
        H = R.unpack_hg(out["H"], S["win"])
        r = RF.gmres_step(St, out["V"], A["w"], A["ut"], H, out["c"], out["s"], out["g"], rd=RF.f32, hwin=hwin,
                          hk1=hk1, rational=rational)
        out["H"] = R.pack_hg(H)
    out.update(hk1=r["hk1"], residNorm=r["residNorm"], stopTol=S["stopTol"], stop=r["stop"], err=r["err"],
               err_val=r["err_val"], err_iter=r["err_iter"], nh=len(r["hist"]),
               hist=r["hist"][0] if r["hist"] else S["hist"], hwin=r["hwin"], vnew=r.get("vnew"), hn2=r.get("hn2"))
    return out


def check(ctx, exact, S, A, grid=0, what=""):
    what = (what, "exact" if exact else "default", S["method"], S["N"], S["n"], S["win"], S["kk"], grid)
    assert ctx.get_option("basis_f32") == "1" and ctx.get_option("exact_dots") == str(exact)
    A32 = image(A)
    dev = T.run_device(ctx, S, A, grid)
    if exact:
        ref = run_ref(S, A, rational=S["N"] <= 65)
        assert ref["err"] == 0, (what, ref["err_val"])
        assert X.same_bits(T.hwin_of(S, dev["H_dots"]), ref["hwin"]), (what, "window sums")
    else:
        again = T.run_device(ctx, S, A, grid)
        T.assert_same(dev, again, (what, "two calls"))
        assert X.same_bits(dev["H_dots"], again["H_dots"])
        js, slot, _ = T.geometry(S)
        hw = T.hwin_of(S, dev["H_dots"])
        n = S["n"]
        for h, j in zip(hw, js):  # the operands are the float images
            err, bound, _ = T.sum_bound(h, A32["V"][:, slot(j)], A["ut"], n)
            assert err <= bound, (what, "window sum", j, float(err), float(bound))
        assert dev["err"] == 0, (what, dev["err"], dev["err_val"])
        ref = run_ref(S, A, hwin=hw, hk1=dev["hk1"])
        # hk1^2 against the exact <ut, vnew> of the UNROUNDED vector orthogonalised with the device's sums
        _, parts, total = T.sum_bound(0.0, A["ut"], ref["vnew"], n)
        bound = parts + T.U * (abs(total) + parts)
        err = abs(T.Fraction(dev["hk1"]) ** 2 - total)
        assert err <= bound + (2 * T.U + T.U * T.U) * (abs(total) + bound), (what, "hk1", float(err), float(bound))
    T.assert_same(dev, ref, what)
    T.assert_untouched(dev, S, A32, what)
    for k in ("V", "PV") if S["method"] == "dqgmres" else ("V",):  # the rings hold float values only
        assert X.same_bits(RF.f32(dev[k]), dev[k]), (what, k, "not a float image")
    return dev, ref


# ---- vector lengths, the padded stride and the [x; y] boundary ------------------------------------------------
@pytest.mark.parametrize("N", (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, BIG))
def test_vector_length_and_boundary(mode, N):
    ctx, exact = mode
    ns = sorted({n for n in (0, 1, N, 700 if N > 700 else N // 2) if 0 <= n <= N})
    for n in ns:
        for method, win, kk in T.both_methods(9):
            check(ctx, exact, *T.make_case(method, N, n, win, kk, seed=21))


# ---- window widths: the groups of 4 and 8 and their tails ------------------------------------------------------
@pytest.mark.parametrize("nv", (1, 4, 5, 8, 9, 17))
def test_window_width(mode, nv):
    ctx, exact = mode
    for method, win, kk in T.both_methods(nv):
        check(ctx, exact, *T.make_case(method, BIG, 700, win, kk, seed=22))


# ---- the ring of cpdqgmres and cpgmres's last column ----------------------------------------------------------------
@pytest.mark.parametrize("mem", (1, 4))
def test_ring_positions(mode, mem):
    ctx, exact = mode
    for kk in sorted({1, mem, mem + 1, 2 * mem + 3}):
        check(ctx, exact, *T.make_case("dqgmres", 600, 250, mem, kk, seed=23))


def test_gmres_last_column(mode):
    """kk = restart: column restart is written and the step reports stop = 1"""
    ctx, exact = mode
    dev, _ = check(ctx, exact, *T.make_case("gmres", 600, 250, 9, 9, seed=24))
    assert dev["stop"] == 1 and dev["nh"] == 1


def test_ring_carried_sequence(fctx):
    """2 (mem + 1) + 2 consecutive steps from kk = 1 in exact mode, each step's output the next one's
    input on the device and in the reference: every slot is stored and read back as a float"""
    ctx, mem = fctx[1], 3
    N, n, M1 = 600, 250, mem + 1
    rng = np.random.default_rng([25, mem])
    S, A = T.make_case("dqgmres", N, n, mem, 1, seed=25)
    resid = abs(A["g"][0])
    for kk in range(1, 2 * M1 + 3):
        S = dict(S, kk=kk, residNorm=resid)
        js, slot, _ = T.geometry(S)
        A["ut"] = rng.standard_normal(N)
        A["w"] = T.fresh_w(rng, A["V"][:, [slot(j) for j in js]], A["V"][:, slot(kk)], A["ut"], n)
        dev, _ = check(ctx, 1, S, A, what=f"carried step {kk}")
        assert dev["nh"] == 1 and dev["stop"] == 0 and dev["err"] == 0
        resid = dev["residNorm"]
        A.update({k: dev[k] for k in T.ARRAYS})


# ---- grids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,N", ((1, BIG), (1, TILE + 1), (1024, 700)))
def test_grid_override(mode, grid, N):
    """one workgroup makes several trips and crosses the boundary inside its loop; a grid larger than
    the work leaves most workgroups without an element"""
    ctx, exact = mode
    for n in (N // 3, N - 1):
        for method, win, kk in T.both_methods(9):
            S, A = T.make_case(method, N, n, win, kk, seed=26)
            dev, _ = check(ctx, exact, S, A, grid=grid)
            if exact:  # the exact sums do not depend on the grid
                assert X.same_bits(dev["H"], T.run_device(ctx, S, A)["H"])


# ---- a step that does not run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,win,kk", T.both_methods(5))
def test_not_running_is_a_noop(mode, method, win, kk):
    """running = 0 leaves every array as uploaded: the rings as their float images, the rest untouched"""
    ctx, _ = mode
    S, A = T.make_case(method, 300, 137, win, kk, seed=27, running=0)
    dev = T.run_device(ctx, S, A)
    A32 = image(A)
    for k in T.ARRAYS:
        assert X.same_bits(dev[k], A32[k]), k
    assert (dev["stop"], dev["err"], dev["err_iter"], dev["nh"]) == (0, 0, 0, 0)
    assert (dev["hk1"], dev["hist"], dev["residNorm"], dev["err_val"]) == (T.HK1_SENT, T.HIST_SENT, T.RESID_SENT, 0.0)
    T.assert_same(dev, run_ref(S, A), "not running")


# ---- the values of the vector that is stored ---------------------------------------------------------------------------
t24 = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
EDGE = [("tie to even, down", 1 + t24, 1.0), ("tie to even, up", 1 + 3 * t24, 1 + 4 * t24),
        ("above a tie", 1 + t24 + 2.0 ** -52, 1 + 2 * t24), ("negative tie", -(1 + t24), -1.0),
        ("float subnormal", 2.0 ** -140, 2.0 ** -140), ("subnormal tie", 1.5 * 2.0 ** -149, 2.0 ** -148),
        ("minus zero", -0.0, -0.0), ("rounds to zero", 2.0 ** -160, 0.0), ("rounds to minus zero", -2.0 ** -160, -0.0),
        ("just below FLT_MAX", FLT_MAX * (1 - 2.0 ** -30), FLT_MAX), ("FLT_MAX", -FLT_MAX, -FLT_MAX)]


@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
def test_edge_values_of_the_stored_vector(mode, method):
    """kk = 1 with V1 = e_1 and ut = e_0: the one window sum is 0, <ut, vnew> = vnew(0) = 1, so
    H(k+1, k) = 1 and the stored vector is f32(vnew) with vnew = [w_x; -w_y] -- the edge values, in the
    x-part and in the y-part, in both normalisation kernels.  No infinity arises."""
    ctx, exact = mode
    N, n, win = 300, 137, 4
    S, A = T.make_case(method, N, n, win, 1, seed=28)
    v1, ut, w = np.zeros(N), np.zeros(N), np.random.default_rng(28).standard_normal(N)
    v1[1], ut[0], w[0] = 1.0, 1.0, 1.0
    vals = np.array([e[1] for e in EDGE])
    w[2:2 + len(vals)] = vals                # x-part: vnew = w
    w[n + 3:n + 3 + len(vals)] = -vals       # y-part: vnew = V1 - w = -w
    A["V"][:, 0], A["ut"], A["w"] = v1, ut, w
    dev, ref = check(ctx, exact, S, A, what="edge values")
    assert dev["hk1"] == 1.0 and T.hwin_of(S, dev["H_dots"]) == [0.0] and dev["err"] == 0
    new = T.geometry(S)[2]
    want = np.array([e[2] for e in EDGE])
    assert X.same_bits(dev["V"][2:2 + len(vals), new], want), (dev["V"][2:2 + len(vals), new], want)
    want_y = np.where(vals == 0, 0.0, want)  # (the y-part is 0 - w: -0.0 cannot arise there from a zero)
    assert X.same_bits(dev["V"][n + 3:n + 3 + len(vals), new], want_y)
    assert np.all(np.isfinite(dev["V"][:, new]))


@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
def test_lucky_breakdown_stores_the_rounded_vector(fctx, method):
    """ut = 0: every sum and H(k+1, k) are zero, the new vector is not normalised -- and is still
    rounded once into its slot (the ring holds nothing else)"""
    S, A = T.make_case(method, 600, 250, 4, 1, seed=29)
    _, slot, new = T.geometry(S)
    A["ut"] = np.zeros(S["N"])
    for exact in (1, 0):
        dev, _ = check(fctx[exact], exact, S, A, what="lucky breakdown")
        assert dev["hk1"] == 0.0 and dev["err"] == 0
        vnew = np.concatenate([A["w"][:S["n"]], RF.f32(A["V"])[S["n"]:, slot(1)] - A["w"][S["n"]:]])
        assert X.same_bits(dev["V"][:, new], RF.f32(vnew))


# ---- the option off: the double basis, as before ----------------------------------------------------------------------
def test_option_off_is_the_double_step(gpu_ctx):
    """the default context (option off) returns what it returned before: the double reference's step,
    no slot rounded (the exact sums of one-product windows make this bit for bit in default mode)"""
    assert gpu_ctx.get_option("basis_f32") == "0"
    S, A = T.scalar_case("gmres", 3.0, 16.0)
    dev, ref = T.check_exact(gpu_ctx, S, A, what="option off")
    assert not X.same_bits(RF.f32(dev["V"]), dev["V"])


# ---- a distributed context refuses -----------------------------------------------------------------------------------------
def test_distributed_context_is_refused():
    from cpkrylov_amd import _lib
    S, A = T.make_case("dqgmres", 128, 70, 4, 5, seed=30)

    def work(ctx, r):
        Sl, Al = T._local(S, A, r * 64, (r + 1) * 64)
        before = {k: np.array(Al[k], copy=True) for k in T.ARRAYS}
        with pytest.raises(_lib.CpkError) as e:
            T.run_device(ctx, Sl, Al, inplace=True)
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
        return all(X.same_bits(Al[k], before[k]) for k in T.ARRAYS)

    assert T._run_ranks(2, work, dict(basis_f32=1)) == [True, True]
