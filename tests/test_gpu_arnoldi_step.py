"""The Arnoldi step kernels of cpgmres / cpdqgmres, driven directly (cpk_debug_arnoldi_step): the window
dots (arnoldi_dots_kernel, arnoldi_dots_exact_kernel, arnoldi_fin_kernel), the orthogonalisation with
its scalar step (ArnoldiOrth) and the normalisation / direction update (GmresNormalize,
DqgmresDirection), against the step reference of arnoldi_ref.py (pinned to the oracle by
test_arnoldi_ref_host.py), at the window widths, vector lengths, grids, ring positions and scalar
branches where these kernels can go wrong and that no solve reaches: windows above the LDS table
(kWinTab = 1024), the last group's empty tail, the [x; y] boundary anywhere in a tile, iterations
far beyond mem.

Exact mode (engine option exact_dots): every output equals the reference bit for bit (NaNs equal).
Default mode: every window sum lies within gamma sum |a b| of the exact sum, two calls return the
same bits, and everything downstream of the sums equals the reference evaluated from the device's
own window sums and H(k+1, k), bit for bit.

Every slot of V, PV, H, c, s and g that the step does not read holds a distinct sentinel, the
reference works on the same arrays, and whole arrays are compared: a wrong ring slot shows as a
changed sentinel or a wrong value.

Not reachable through the step: SymGivens with b < 0 (b is H(k+1, k), a square root); the reference's
sym_givens is held to the oracle's on negated pairs on the CPU.

Found by this module: nothing.  The loops that bypass the LDS table had never run before it; at every
shape here the device equals the reference."""
import math
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import pytest

import arnoldi_ref as R
import xacc_cases as X
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U = Fraction(1, 2 ** 53)
HK1_SENT, HIST_SENT, RESID_SENT = -77.0, -55.0, 123.5
ARRAYS = ("V", "PV", "xy", "H", "c", "s", "g")
SCALARS = ("hk1", "residNorm", "stopTol", "hist", "err_val")
INTS = ("stop", "err", "err_iter", "nh")


@pytest.fixture(scope="module")
def xctx():
    """a context of its own in exact mode (the session's default context stays in default mode)"""
    import cpkrylov_amd as cpk
    ctx = cpk.Context(options=dict(exact_dots=1))
    yield ctx
    ctx.close()


# ---- cases -----------------------------------------------------------------------------------------
def _sent(shape, base):
    size = int(np.prod(shape))
    return np.asfortranarray((-(base + 0.25 * np.arange(size))).reshape(shape, order="F"))


def geometry(S):
    """window iterations j (oldest first), the slot of iteration j's vector, the new vector's slot"""
    kk, win = S["kk"], S["win"]
    if S["method"] == "dqgmres":
        M1 = win + 1
        return range(max(1, kk - win + 1), kk + 1), (lambda j: (j - 1) % M1), kk % M1
    return range(1, kk + 1), (lambda j: j - 1), kk


def fresh_w(rng, Vwin, vk, ut, n):
    """w with <ut, vnew> > 0 after the orthogonalisation: [w_x; vk_y - w_y] = alpha ut + noise and
    alpha |ut|^2 = sum h_j^2 + |<ut, noise>| + |ut|^2"""
    N = len(ut)
    noise = rng.standard_normal(N) / math.sqrt(N)
    h = Vwin.T @ ut
    alpha = (h @ h + abs(ut @ noise)) / (ut @ ut) + 1.0
    base = alpha * ut + noise
    return np.concatenate([base[:n], vk[n:] - base[n:]])


def make_case(method, N, n, win, kk, seed=0, itmax=10 ** 9, stopTol=0.0, running=1):
    """a step on standard-normal data: what the step reads is random, every other slot a sentinel"""
    rng = np.random.default_rng([seed, N, n, win, kk % 100003])
    dq = method == "dqgmres"
    S = dict(method=method, N=N, n=n, win=win, kk=kk, itmax=itmax, stopTol=stopTol, running=running,
             residNorm=RESID_SENT, hk1=HK1_SENT, hist=HIST_SENT)
    js, slot, _ = geometry(S)
    A = dict(V=_sent((N, win + 1), 1.0e6), H=_sent(((win + 2) ** 2 if dq else (win + 1) * win,), 3.0e6),
             c=_sent((win,), 5.0e6), s=_sent((win,), 6.0e6), g=_sent((win + 1,), 7.0e6))
    slots = [slot(j) for j in js]
    A["V"][:, slots] = rng.standard_normal((N, len(slots))) / math.sqrt(N)
    A["ut"] = rng.standard_normal(N)
    A["w"] = fresh_w(rng, A["V"][:, slots], A["V"][:, slot(kk)], A["ut"], n)
    if dq:
        M1, W = win + 1, win + 2
        A["PV"], A["xy"] = _sent((N, M1), 2.0e6), rng.standard_normal(N)
        for j in range(max(1, kk - win), kk):  # what the rotations and the direction update read
            A["PV"][:, (j - 1) % M1] = rng.standard_normal(N) / math.sqrt(N)
            A["c"][(j - 1) % win], A["s"][(j - 1) % win] = rng.uniform(-1, 1, 2)
        A["g"][(kk - 1) % M1] = rng.standard_normal()
        if kk > win:  # H(kk - mem, mem + 2): the fill-in the first rotation reads (a solve left 0 there)
            A["H"][((kk - win) % W) * W + win + 1] = rng.standard_normal()
    else:
        A["PV"], A["xy"] = np.zeros((N, 1), order="F"), np.zeros(N)
        A["c"][:kk - 1], A["s"][:kk - 1] = rng.uniform(-1, 1, kk - 1), rng.uniform(-1, 1, kk - 1)
        A["g"][kk - 1] = rng.standard_normal()
    return S, A


def write_masks(S):
    """where the step may write (everything else must come back as it went in)"""
    kk, win = S["kk"], S["win"]
    m = {k: set() for k in ("V", "PV", "H", "c", "s", "g")}
    if not S["running"]:
        return m, False
    if S["method"] == "dqgmres":
        M1, W = win + 1, win + 2
        m["V"].add(kk % M1), m["PV"].add((kk - 1) % M1)
        m["H"].update((kk % W) * W + q for q in range(W))
        for j in range(max(1, kk - win), kk):
            m["H"].add((j % W) * W + (kk - j + 2) - 1), m["H"].add(((j + 1) % W) * W + (kk - j + 1) - 1)
        m["c"].add((kk - 1) % win), m["s"].add((kk - 1) % win)
        m["g"].update(((kk - 1) % M1, kk % M1))
        return m, True
    m["V"].add(kk)
    m["H"].update(i + (kk - 1) * (win + 1) for i in range(kk + 1))
    m["c"].add(kk - 1), m["s"].add(kk - 1), m["g"].update((kk - 1, kk))
    return m, False


def hwin_of(S, Hflat):
    """the window sums in H's storage as the dots left it"""
    kk, win = S["kk"], S["win"]
    js, _, _ = geometry(S)
    if S["method"] == "dqgmres":
        W = win + 2
        return [float(Hflat[(j % W) * W + (2 + kk - j) - 1]) for j in js]
    return [float(Hflat[(j - 1) + (kk - 1) * (win + 1)]) for j in js]


# ---- the device and the reference, same inputs, same outputs ----------------------------------------
def run_device(ctx, S, A, grid=0, inplace=False):
    """one cpk_debug_arnoldi_step on copies of A's arrays (inplace: on A's own F-ordered arrays)"""
    import ctypes

    from cpkrylov_amd import _lib
    from cpkrylov_amd.api import _dptr
    dq = S["method"] == "dqgmres"
    out = {k: A[k] if inplace else np.array(A[k], order="F", copy=True) for k in ARRAYS}
    w, ut = np.ascontiguousarray(A["w"]), np.ascontiguousarray(A["ut"])
    out["H_dots"] = np.full(out["H"].shape, -9.0)
    ld = max(S["N"], 1)
    io = _lib.ArnoldiStep(method=_lib.METHODS[S["method"]], running=S["running"], grid=grid, n=S["n"], N=S["N"],
                          win=S["win"], kk=S["kk"], itmax=S["itmax"], stopTol=S["stopTol"], residNorm=S["residNorm"],
                          hk1=S["hk1"], hist=S["hist"], V=_dptr(out["V"]), ldv=ld, PV=_dptr(out["PV"]) if dq else None,
                          ldpv=ld, xy=_dptr(out["xy"]) if dq else None, w=_dptr(w), ut=_dptr(ut), H=_dptr(out["H"]),
                          c=_dptr(out["c"]), s=_dptr(out["s"]), g=_dptr(out["g"]), H_dots=_dptr(out["H_dots"]),
                          stop=-3, err=-3, err_val=-3.0, err_iter=-3, nh=-3)
    _lib.check(_lib.lib.cpk_debug_arnoldi_step(ctx.h, ctypes.byref(io)))
    for k in SCALARS + INTS:
        out[k] = getattr(io, k)
    return out


def run_ref(S, A, hwin=None, hk1=None, rational=True):
    dq = S["method"] == "dqgmres"
    out = {k: np.array(A[k], order="F", copy=True) for k in ARRAYS}
    St = dict(S, **{("mem" if dq else "restart"): S["win"]})
    if dq:
        H = R.unpack_hd(out["H"], S["win"], S["kk"])
        r = R.dqgmres_step(St, out["V"], out["PV"], out["xy"], A["w"], A["ut"], H, out["c"], out["s"], out["g"],
                           hwin=hwin, hk1=hk1, rational=rational)
        out["H"] = R.pack_hd(H, S["win"])
    else:
        H = R.unpack_hg(out["H"], S["win"])
        r = R.gmres_step(St, out["V"], A["w"], A["ut"], H, out["c"], out["s"], out["g"], hwin=hwin, hk1=hk1,
                         rational=rational)
        out["H"] = R.pack_hg(H)
    out.update(hk1=r["hk1"], residNorm=r["residNorm"], stopTol=S["stopTol"], stop=r["stop"], err=r["err"],
               err_val=r["err_val"], err_iter=r["err_iter"], nh=len(r["hist"]),
               hist=r["hist"][0] if r["hist"] else S["hist"], hwin=r["hwin"], vnew=r.get("vnew"), hn2=r.get("hn2"))
    return out


def assert_same(dev, ref, what, skip=()):
    for k in INTS:
        assert dev[k] == ref[k], (what, k, dev[k], ref[k])
    for k in SCALARS + ARRAYS:
        if k in skip:
            continue
        a, b = np.asarray(dev[k], np.float64).reshape(-1, order="F"), np.asarray(ref[k], np.float64).reshape(-1, order="F")
        assert a.shape == b.shape, (what, k)
        bad = np.flatnonzero(~((X.bits(a) == X.bits(b)) | (np.isnan(a) & np.isnan(b))))
        assert bad.size == 0, (what, k, bad.size, bad[:5], a[bad[:3]], b[bad[:3]])


def assert_untouched(dev, S, A, what):
    m, xy = write_masks(S)
    for k in ("V", "PV"):
        cols = [q for q in range(A[k].shape[1]) if q not in m[k]]
        assert X.same_bits(dev[k][:, cols], A[k][:, cols]), (what, k)
    for k in ("H", "c", "s", "g"):
        keep = np.ones(A[k].size, bool)
        keep[list(m[k])] = False
        assert X.same_bits(dev[k][keep], A[k][keep]), (what, k, np.flatnonzero(X.bits(dev[k]) != X.bits(A[k]))[:8])
    if not xy:
        assert X.same_bits(dev["xy"], A["xy"]), (what, "xy")


def check_exact(ctx, S, A, grid=0, what="", allow_err=False):
    what = (what, S["method"], S["N"], S["n"], S["win"], S["kk"], grid)
    dev, ref = run_device(ctx, S, A, grid), run_ref(S, A)
    assert allow_err or ref["err"] == 0, (what, ref["err_val"])
    assert X.same_bits(hwin_of(S, dev["H_dots"]), ref["hwin"]) or not S["running"], (what, "window sums")
    # after err = 4 what the last launch leaves in the vectors is not defined (the solve has failed)
    assert_same(dev, ref, what, skip=("V", "PV", "xy") if ref["err"] else ())
    if not ref["err"]:
        assert_untouched(dev, S, A, what)
    return dev, ref


def _gamma(k):
    return k * U / (1 - k * U)


def sum_bound(v, a, b, n):
    """(|v - sum a b|, bound) of a window sum fl(x-part) + fl(y-part) in default mode: the bound of
    xacc_cases.error_and_bound on each part (gamma_len sum |a b|), and the rounding of the final add"""
    assert X.default_mode_ok(a[:n], b[:n]) and X.default_mode_ok(a[n:], b[n:])  # no pair is left out
    (tx, ax), (ty, ay) = X._int_sums(a[:n], b[:n]), X._int_sums(a[n:], b[n:])
    fv = Fraction(float(v))
    return abs(fv - (tx + ty)), _gamma(n) * ax + _gamma(len(a) - n) * ay + U * abs(fv) / (1 - U), tx + ty


def check_default(ctx, S, A, grid=0, what=""):
    what = (what, S["method"], S["N"], S["n"], S["win"], S["kk"], grid)
    assert ctx.get_option("exact_dots") == "0"
    dev, again = run_device(ctx, S, A, grid), run_device(ctx, S, A, grid)
    assert_same(dev, again, (what, "two calls"))
    assert X.same_bits(dev["H_dots"], again["H_dots"])
    js, slot, _ = geometry(S)
    hw = hwin_of(S, dev["H_dots"])
    n = S["n"]
    for h, j in zip(hw, js):
        err, bound, _ = sum_bound(h, A["V"][:, slot(j)], A["ut"], n)
        assert err <= bound, (what, "window sum", j, float(err), float(bound))
    assert dev["err"] == 0, (what, dev["err"], dev["err_val"])
    ref = run_ref(S, A, hwin=hw, hk1=dev["hk1"], rational=False)
    # hk1^2 against the exact <ut, vnew> of the vector orthogonalised with the device's own sums: the
    # sum's bound, and the square root's rounding (hk1 = sqrt(s) (1 + d), |d| <= u) on s <= exact + bound
    _, parts, total = sum_bound(0.0, A["ut"], ref["vnew"], n)  # (v = 0: the two parts' bounds alone)
    bound = parts + U * (abs(total) + parts)  # and the final add's rounding, on |x + y| <= |exact| + parts
    err = abs(Fraction(dev["hk1"]) ** 2 - total)
    assert err <= bound + (2 * U + U * U) * (abs(total) + bound), (what, "hk1", float(err), float(bound))
    assert_same(dev, ref, what)
    assert_untouched(dev, S, A, what)
    return dev, ref


def check(ctx, exact, *a, **k):
    return (check_exact if exact else check_default)(ctx, *a, **k)


@pytest.fixture(params=(1, 0), ids=("exact", "default"))
def mode(request, xctx, gpu_ctx):
    return (xctx, 1) if request.param else (gpu_ctx, 0)


def both_methods(nv, extra=3):
    """(method, win, kk) with a window of nv vectors: cpgmres at kk = nv, cpdqgmres at mem = nv, kk = nv + extra"""
    return (("gmres", nv, nv), ("dqgmres", nv, nv + extra))


# ---- window widths: the groups of 4 and 8, the gather of 16 sums --------------------------------------
@pytest.mark.parametrize("nv", (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33))
def test_window_width(mode, nv):
    ctx, exact = mode
    for method, win, kk in both_methods(nv):
        check(ctx, exact, *make_case(method, 1500, 700, win, kk, seed=1))


# ---- the LDS table's cap: 1025 and 1100 take the untabulated loop ---------------------------------------
@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
@pytest.mark.parametrize("nv", (1023, 1024, 1025, 1100))
def test_table_cap(mode, nv, method):
    """N = 300 is below a tile of the orthogonalisation (4 x 256): the window loop runs in operator()"""
    ctx, exact = mode
    _, win, kk = dict((m[0], m) for m in both_methods(nv))[method]
    check(ctx, exact, *make_case(method, 300, 137, win, kk, seed=2))


@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
def test_table_cap_tiled(mode, method):
    """N = 2100 holds two full tiles: tile()'s own branch for a window above the table"""
    ctx, exact = mode
    _, win, kk = dict((m[0], m) for m in both_methods(1025))[method]
    check(ctx, exact, *make_case(method, 2100, 900, win, kk, seed=3))


# ---- vector lengths and the [x; y] boundary ----------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 3000))
def test_vector_length_and_boundary(mode, N):
    """the dots' tile is 3 x 256, the orthogonalisation's 4 x 256; the boundary at the start, inside
    and at the end of a tile and at both ends of the vector"""
    ctx, exact = mode
    ns = sorted({n for n in (0, 1, N // 2, N - 1, N, 256, 768) if 0 <= n <= N})
    for n in ns:
        for method, win, kk in both_methods(9):
            check(ctx, exact, *make_case(method, N, n, win, kk, seed=4))


# ---- grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,N", ((1, 1025), (1, 3000), (2, 1537)))
def test_grid_override(mode, grid, N):
    """one workgroup makes several trips and crosses the boundary in the middle of its loop; two workgroups"""
    ctx, exact = mode
    for n in (N // 3, 768, N - 1):
        for method, win, kk in both_methods(9):
            S, A = make_case(method, N, n, win, kk, seed=5)
            dev, _ = check(ctx, exact, S, A, grid=grid)
            if exact:  # the exact sums do not depend on the grid
                assert X.same_bits(dev["H"], run_device(ctx, S, A)["H"])


def test_default_grid_wraps(mode):
    """1024 * 768 + 257 elements: the dots' default grid takes a second trip in 257 threads"""
    ctx, exact = mode
    check(ctx, exact, *make_case("gmres", 1024 * 768 + 257, 400000, 2, 2, seed=6))


# ---- the ring of cpdqgmres --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", (1, 2, 3, 8, 9))
def test_ring_carried_sequence(mode, mem):
    """2 (mem + 1) + 2 consecutive steps from kk = 1, each step's output the next one's input, on the
    device and in the reference: every ring slot of V, PV, H, c, s and g is visited twice.  (Default
    mode: the reference takes each step from the device's state, whose sums are not the exact ones.)"""
    ctx, exact = mode
    N, n, M1 = 600, 250, mem + 1
    rng = np.random.default_rng([7, mem])
    S, A = make_case("dqgmres", N, n, mem, 1, seed=7)
    Ar = {k: np.array(v, copy=True) for k, v in A.items()}  # the reference's own carried state (exact mode)
    resid = abs(A["g"][0])
    for kk in range(1, 2 * M1 + 3):
        S = dict(S, kk=kk, residNorm=resid)
        js, slot, _ = geometry(S)
        A["ut"] = Ar["ut"] = rng.standard_normal(N)
        A["w"] = Ar["w"] = fresh_w(rng, A["V"][:, [slot(j) for j in js]], A["V"][:, slot(kk)], A["ut"], n)
        dev, _ = check(ctx, exact, S, A, what=f"carried step {kk}")
        assert dev["nh"] == 1 and dev["stop"] == 0 and dev["err"] == 0
        if exact:
            ref = run_ref(S, Ar, rational=False)
            assert_same(dev, ref, f"carried step {kk}, the reference's own sequence")
            Ar.update({k: ref[k] for k in ARRAYS})
        resid = dev["residNorm"]
        A.update({k: dev[k] for k in ARRAYS})


@pytest.mark.parametrize("mem", (1, 2, 3, 8, 9))
def test_ring_positions(mode, mem):
    ctx, exact = mode
    for kk in (mem, mem + 1, mem + 2, 10 ** 6 + 3):
        check(ctx, exact, *make_case("dqgmres", 600, 250, mem, kk, seed=8))


@pytest.mark.parametrize("kk", (1, 2, 9))
def test_gmres_positions(mode, kk):
    """at kk = restart the step reports stop = 1 whatever the residual"""
    ctx, exact = mode
    dev, _ = check(ctx, exact, *make_case("gmres", 600, 250, 9, kk, seed=9))
    assert dev["residNorm"] > 0 and dev["stop"] == (1 if kk == 9 else 0) and dev["nh"] == 1


# ---- stop values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,win,kk", both_methods(5))
def test_stop_values(mode, method, win, kk):
    ctx, exact = mode
    S, A = make_case(method, 600, 250, win + 3, kk, seed=10)
    dev, _ = check(ctx, exact, S, A)
    r = dev["residNorm"]
    assert r > 0 and dev["stop"] == 0
    for tol, stop in ((r, 1), (math.nextafter(r, 0.0), 0), (math.nextafter(r, math.inf), 1), (1.0e300, 1)):
        dev, _ = check(ctx, exact, dict(S, stopTol=tol), A, what=f"stopTol {tol!r}")
        assert dev["stop"] == stop and X.same_bits(dev["residNorm"], r) and dev["stopTol"] == tol
    if method == "dqgmres":
        dev, _ = check(ctx, exact, dict(S, itmax=kk), A, what="kk == itmax")
        assert dev["stop"] == 1
        dev, _ = check(ctx, exact, dict(S, itmax=kk + 1), A, what="kk < itmax")
        assert dev["stop"] == 0


@pytest.mark.parametrize("method,win,kk", both_methods(5) + both_methods(1100))
def test_not_running_is_a_noop(mode, method, win, kk):
    ctx, exact = mode
    S, A = make_case(method, 300, 137, win, kk, seed=11, running=0)
    dev = run_device(ctx, S, A)
    for k in ARRAYS:
        assert X.same_bits(dev[k], A[k]), k
    assert (dev["stop"], dev["err"], dev["err_iter"], dev["nh"]) == (0, 0, 0, 0)
    assert (dev["hk1"], dev["hist"], dev["residNorm"], dev["err_val"]) == (HK1_SENT, HIST_SENT, RESID_SENT, 0.0)
    assert_same(dev, run_ref(S, A), "not running")


# ---- the scalar step, branch by branch ------------------------------------------------------------------------------
def scalar_case(method, a, b2, seed=12, N=600, n=250, win=4):
    """kk = 1 with H(1,1) = a and H(2,1)^2 = b2 exactly: V1 = e_0 (+ noise where ut is zero), ut = a e_0 +
    e_{N-1}, and w such that vnew(0) = a and vnew(N-1) = b2 before the orthogonalisation takes a e_0 away"""
    S, A = make_case(method, N, n, win, 1, seed=seed)
    rng = np.random.default_rng([seed, 99])
    v1 = rng.standard_normal(N) / math.sqrt(N)
    v1[0], v1[N - 1] = 1.0, 0.0
    ut = np.zeros(N)
    ut[0], ut[N - 1] = a, 1.0
    w = rng.standard_normal(N)
    w[0], w[N - 1] = a, -b2  # vnew(0) = w(0) - a * 1 = 0 ; vnew(N-1) = v1(N-1) - w(N-1) = b2
    A["V"][:, 0], A["ut"], A["w"] = v1, ut, w
    return S, A


GIVENS = [("a == 0, b > 0", 0.0, 9.0, (0.0, 1.0, 3.0)),
          ("b == 0, a > 0", 2.0, 0.0, (1.0, 0.0, 2.0)),
          ("b == 0, a < 0", -2.0, 0.0, (-1.0, 0.0, 2.0)),
          ("|b| > |a|, a > 0", 3.0, 16.0, None), ("|b| > |a|, a < 0", -3.0, 16.0, None),
          ("|b| <= |a|, a > 0", 4.0, 9.0, None), ("|b| <= |a|, a < 0", -4.0, 9.0, None),
          ("|b| == |a|", 3.0, 9.0, None), ("|b| == |a|, a < 0", -3.0, 9.0, None)]


@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
@pytest.mark.parametrize("what,a,b2,csd", GIVENS, ids=[g[0] for g in GIVENS])
def test_sym_givens_branches(xctx, gpu_ctx, method, what, a, b2, csd):
    """the device's sym_givens through the step at kk = 1, where H(1,1) and H(2,1) are the inputs: every
    sum is exact in either mode (one non-zero product each), so both modes equal the exact reference"""
    S, A = scalar_case(method, a, b2)
    for ctx in (xctx, gpu_ctx):
        dev, ref = check_exact(ctx, S, A, what=what)
        assert dev["err"] == 0 and dev["hk1"] == math.sqrt(b2) and hwin_of(S, dev["H_dots"]) == [a]
        want = csd or R.sym_givens(a, math.sqrt(b2))
        d = dev["H"][0] if method == "gmres" else dev["H"][(1 % (S["win"] + 2)) * (S["win"] + 2) + 1]
        assert X.same_bits((dev["c"][0], dev["s"][0], d), want), (what, dev["c"][0], dev["s"][0], d, want)
        assert X.same_bits(dev["residNorm"], abs(want[1] * A["g"][0]))
        if b2 == 0:  # lucky breakdown: the new vector is not normalised
            assert X.same_bits(dev["V"][:, 1], ref["vnew"])


@pytest.mark.parametrize("method,win,kk", (("gmres", 1, 1), ("gmres", 6, 6), ("dqgmres", 4, 1), ("dqgmres", 6, 5),
                                           ("dqgmres", 1, 4), ("dqgmres", 6, 9)))
def test_zero_step(xctx, gpu_ctx, method, win, kk):
    """ut = 0 and vnew = 0: every window sum and H(k+1, k) are zero, SymGivens(0, 0) = (1, 0, 0), the
    new vector stays as it is, and cpdqgmres divides by H(k, 2) = 0 as the reference does (NaN and
    infinities compared as bits)"""
    S, A = make_case(method, 600, 250, win, kk, seed=13)
    _, slot, new = geometry(S)
    A["ut"] = np.zeros(S["N"])
    A["w"] = np.concatenate([np.zeros(S["n"]), A["V"][S["n"]:, slot(kk)]])
    for ctx in (xctx, gpu_ctx):
        dev, _ = check_exact(ctx, S, A, what="zero step")
        assert dev["hk1"] == 0.0 and dev["err"] == 0 and dev["nh"] == 1 and dev["residNorm"] == 0.0
        assert np.all(dev["V"][:, new] == 0.0)
        rot = (kk - 1) % win if method == "dqgmres" else kk - 1
        # (cpdqgmres at kk > mem: the rotation with row kk - mem carries that row's fill-in into H(k, 2),
        # so SymGivens sees a != 0, b == 0)
        assert dev["s"][rot] == 0.0 and dev["c"][rot] == (1.0 if method == "gmres" else math.copysign(1.0, dev["c"][rot]))
        if method == "dqgmres" and kk <= win:  # H(k, 2) = 0: the direction is V(:, kpos) / 0
            assert dev["c"][rot] == 1.0 and not np.any(np.isfinite(dev["PV"][:, (kk - 1) % (win + 1)]))


@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
def test_negative_squared_norm_stops(xctx, gpu_ctx, method):
    """ut = -vnew with a window whose sums are all zero (V1 and ut on disjoint supports): the squared
    norm is -|vnew|^2 < 0 and the step stops with err = 4 before H(k+1, k) is written.  (What the
    normalisation leaves in the new vector after the error is not defined and not compared.)"""
    S, A = make_case(method, 600, 250, 4, 1, seed=14)
    N, n = S["N"], S["n"]
    rng = np.random.default_rng(14)
    v1, w = np.zeros(N), np.zeros(N)
    v1[0:n:2] = rng.standard_normal(len(range(0, n, 2)))
    w[1:N:2] = rng.standard_normal(len(range(1, N, 2)))
    vnew = np.concatenate([w[:n], v1[n:] - w[n:]])
    A["V"][:, 0], A["w"], A["ut"] = v1, w, -vnew
    want = R.window_sum(A["ut"], vnew, n)
    assert want < 0
    for ctx, exact in ((xctx, 1), (gpu_ctx, 0)):
        dev, ref = run_device(ctx, S, A), run_ref(S, A)
        assert (dev["err"], dev["err_iter"], dev["stop"], dev["nh"]) == (4, 1, 1, 0) == (ref["err"], 1, ref["stop"], 0)
        assert hwin_of(S, dev["H_dots"]) == [0.0]
        if exact:
            assert X.same_bits(dev["err_val"], want) and X.same_bits(ref["err_val"], want)
        else:
            err, bound, _ = sum_bound(dev["err_val"], A["ut"], vnew, n)
            assert err <= bound
        assert (dev["hk1"], dev["hist"], dev["residNorm"]) == (HK1_SENT, HIST_SENT, RESID_SENT)
        # H(k+1, k), the rotations and g are as they went in; the window sum was written
        skip = ("V", "PV", "xy", "err_val")
        assert_same(dev, dict(ref, err_val=dev["err_val"]), "err = 4", skip=skip)
        keepV = [q for q in range(A["V"].shape[1]) if q != geometry(S)[2]]
        assert X.same_bits(dev["V"][:, keepV], A["V"][:, keepV])
        for k in ("c", "s", "g"):
            assert X.same_bits(dev[k], A[k]), k


# ---- edge values in the window sums (exact mode) ---------------------------------------------------------------------
EDGE_N, EDGE_n = 1500, 700


def _edge_pairs():
    """the cases of families 2, 5 and 6 two at a time: one for an x-part (700 elements), one for a y-part (800)"""
    cx, cy = X.cases(EDGE_n, families=(2, 5, 6)), X.cases(EDGE_N - EDGE_n, families=(2, 5, 6))
    assert len(cx) == len(cy) >= 15
    return [(cx[i], cy[(i + 7) % len(cy)]) for i in range(len(cx))]


@pytest.mark.parametrize("nv", (5, 17))
@pytest.mark.parametrize("method", ("gmres", "dqgmres"))
def test_edge_values_in_the_window(xctx, method, nv):
    """cancellation down to the last bit, sums at and above DBL_MAX and a partial sum that overflows, as
    the x-part of one window vector and the y-part of another: each sum equals rational arithmetic
    (where it is the definition) and the oracle, and the whole step equals the reference, in which
    infinities and NaNs then travel as IEEE says"""
    _, win, kk = dict((m[0], m) for m in both_methods(nv))[method]
    for i, ((namex, ax, bx), (namey, ay, by)) in enumerate(_edge_pairs()):
        S, A = make_case(method, EDGE_N, EDGE_n, win, kk, seed=15)
        js, slot, _ = geometry(S)
        jx, jy = js[i % nv], js[(i + 3) % nv]
        A["ut"] = np.concatenate([bx, by])
        A["V"][:, slot(jx)] = np.concatenate([ax, np.zeros(EDGE_N - EDGE_n)])
        A["V"][:, slot(jy)] = np.concatenate([np.zeros(EDGE_n), ay])
        with np.errstate(all="ignore"):  # (the families at the top of the range leave no finite w)
            A["w"] = fresh_w(np.random.default_rng([15, i]), A["V"][:, [slot(j) for j in js]], A["V"][:, slot(kk)],
                             A["ut"], EDGE_n)
        dev, ref = check_exact(xctx, S, A, what=(namex, namey), allow_err=True)
        hw = dict(zip(js, hwin_of(S, dev["H_dots"])))
        for name, a, b, j in ((namex, ax, bx, jx), (namey, ay, by, jy)):
            rb, ra = O.xdot(a, b), X.ref_exact(a, b) if X.a_applies(a, b) else None
            print(f"{method} nv={nv} {name}: device {hw[j]!r} oracle {rb!r} rational {ra!r}")
            assert X.same_bits(hw[j], rb), (name, hw[j], rb)
            assert ra is None or X.same_bits(hw[j], ra), (name, hw[j], ra)


# ---- distributed: the allreduce and arnoldi_fin_kernel -------------------------------------------------------------------
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


def _local(S, A, lo, hi):
    """rows [lo, hi) of the stacked vectors: the rank's x rows, then its y rows, and its own n"""
    nl = min(max(S["n"] - lo, 0), hi - lo)
    Al = {k: (np.asfortranarray(v[lo:hi]) if k in ("V", "PV", "xy", "w", "ut") and v.shape[0] == S["N"] else v)
          for k, v in A.items()}
    if S["method"] != "dqgmres":
        Al["PV"], Al["xy"] = A["PV"], A["xy"]
    return dict(S, N=hi - lo, n=nl), Al


def _check_dist(P, cuts, exact, S, A, what):
    def work(ctx, r):
        Sl, Al = _local(S, A, cuts[r], cuts[r + 1])
        return run_device(ctx, Sl, Al)

    res = _run_ranks(P, work, dict(exact_dots=exact))
    shared = tuple(k for k in SCALARS + ARRAYS if k not in ("V", "PV", "xy"))
    for r in range(P):  # every rank the same bits
        assert_same(res[r], res[0], (what, "rank", r), skip=("V", "PV", "xy"))
        assert X.same_bits(res[r]["H_dots"], res[0]["H_dots"])
    hw = hwin_of(S, res[0]["H_dots"])
    if exact:
        ref = run_ref(S, A)
        assert X.same_bits(hw, ref["hwin"])
    else:
        js, slot, _ = geometry(S)
        for h, j in zip(hw, js):
            err, bound, _ = sum_bound(h, A["V"][:, slot(j)], A["ut"], S["n"])
            assert err <= bound, (what, j)
        ref = run_ref(S, A, hwin=hw, hk1=res[0]["hk1"], rational=False)
    assert_same(res[0], ref, what, skip=("V", "PV", "xy"))
    dq = S["method"] == "dqgmres"
    for r in range(P):  # each rank's rows of the vectors
        lo, hi = cuts[r], cuts[r + 1]
        for k in ("V", "PV", "xy") if dq else ("V",):
            assert X.same_bits(res[r][k], ref[k][lo:hi]), (what, "rank", r, k)
    return shared


LAYOUTS = ((2, (0, 450, 1500)), (3, (0, 450, 1100, 1500)), (3, (0, 0, 1100, 1500)))  # n = 700: cuts in x, in y; no rows


@pytest.mark.parametrize("exact", (1, 0), ids=("exact", "default"))
@pytest.mark.parametrize("P,cuts", LAYOUTS, ids=("P2", "P3", "P3_empty_rank"))
def test_dist_step(P, cuts, exact):
    """every rank passes its rows and its own n and receives the same scalars: the reference's on the
    concatenated vectors in exact mode; the bound and the downstream bits in default mode"""
    for nv in (9, 17):
        for method, win, kk in both_methods(nv):
            S, A = make_case(method, 1500, 700, win, kk, seed=16)
            _check_dist(P, cuts, exact, S, A, (P, cuts, exact, method, nv))


@pytest.mark.parametrize("exact", (1, 0), ids=("exact", "default"))
def test_dist_window_limit(exact):
    """2 maxv sums travel through the 4096-slot reduction buffer: maxv = 2048 is accepted and right
    (64 rows per rank), maxv = 2049 is refused on every rank before anything runs or is written"""
    from cpkrylov_amd import _lib
    P, Nl = 2, 64
    S, A = make_case("gmres", P * Nl, 70, 2048, 2048, seed=17)
    _check_dist(P, (0, Nl, 2 * Nl), exact, S, A, "maxv = 2048")
    for method, kk in (("gmres", 1), ("dqgmres", 5)):
        S, A = make_case(method, P * Nl, 70, 2049, kk, seed=17)

        def work(ctx, r):
            Sl, Al = _local(S, A, r * Nl, (r + 1) * Nl)
            before = {k: np.array(Al[k], copy=True) for k in ARRAYS}
            with pytest.raises(_lib.CpkError) as e:
                run_device(ctx, Sl, Al, inplace=True)
            assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
            return all(X.same_bits(Al[k], before[k]) for k in ARRAYS)

        assert _run_ranks(P, work, dict(exact_dots=exact)) == [True] * P

