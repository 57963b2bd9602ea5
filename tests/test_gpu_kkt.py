"""The saddle-point operator K = [A B'; B -C] on the GPU (cpk_kkt_*, cpkrylov_amd.KKT) against the
scalar reference of tests/kkt_ref.py, BIT FOR BIT: the product, the true residual and its four sums
(exact under exact_dots, within the bound of any summation order otherwise), blocks whose columns
equal the single-column call, values that follow the matrix handles, the cold and the warm-started
verified solve, and the refusals."""
import ctypes as C

import numpy as np
import pytest

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import fixtures as F
import kkt_ref as R
import structures as S
from devbuf import DeviceArray
from oracle import oracle as O
from rawmat import duplicated_csr, raw_matrix

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
PC_PROPS = ("nitref", "itref_tol", "force_itref", "residual_update")
BLOCK_MEMBERS = ("tiny65x63", "arrow_row", "cvxqp1_m")
_REF = {}


def _dp(a):
    return a.ctypes.data_as(PD)


def _kkt(name, ctx):
    import cpkrylov_amd as cpk
    P = R.system(name)
    return cpk.KKT(P["A"], P["B"], P["C"], ctx=ctx)


def _ref(name, key):
    """(s, r, exact sums) of the reference for an operand, computed once and shared"""
    if (name, key) not in _REF:
        P, K = R.system(name), R.operator(name)
        s = R.matvec(K, R.operands(name)[key])
        r = P["rhs"] - s
        _REF[(name, key)] = (s, r, R.sums(r, P["rhs"], P["n"]))
    return _REF[(name, key)]


def _sums_of(nr):
    return np.array([nr["rr_x"], nr["rr_y"], nr["bb_x"], nr["bb_y"]], dtype=np.float64)


@pytest.mark.parametrize("name", R.MEMBERS)
def test_product_and_residual_bit_for_bit(gpu_ctx, name):
    import cpkrylov_amd as cpk
    P = R.system(name)
    K = _kkt(name, gpu_ctx)
    N = P["n"] + P["m"]
    assert K.info()["nnz"] == len(R.operator(name)[1]) and K.shape == (N, N)
    for key, z in R.operands(name).items():
        s, r, exact = _ref(name, key)
        assert R.same_bits(K @ z, s), key
        rd, nr = K.residual(z, P["rhs"])
        assert R.same_bits(rd, r), key
        got = _sums_of(nr)
        # default mode: any summation order stays within gamma_{N+1} of the exact sum of squares
        fin = np.isfinite(exact)
        assert np.array_equal(np.isnan(got), np.isnan(exact)), key
        assert np.all(np.abs(got[fin] - exact[fin]) <= R.gamma(N + 1) * exact[fin]), (key, got, exact)
        assert nr["rnorm"] == np.sqrt(got[0] + got[1]) or np.isnan(nr["rnorm"])
        with cpk.engine_options(gpu_ctx, exact_dots=1):
            rx, nx = K.residual(z, P["rhs"])
            _, n_only = K.residual(z, P["rhs"], want_r=False)
        assert R.same_bits(rx, r), key
        assert R.same_bits(_sums_of(nx), exact), (key, _sums_of(nx), exact)
        assert R.same_bits(_sums_of(n_only), exact), key


@pytest.mark.parametrize("name", ("tiny2x1", "tiny65x63", "arrow_row"))
def test_in_place_padding_and_null_outputs(gpu_ctx, name):
    """R == Bm in place gives the same bits; leading dimensions above N leave the padding rows
    untouched; R or norms may be NULL"""
    from cpkrylov_amd import _lib
    P = R.system(name)
    K = _kkt(name, gpu_ctx)
    N, k, ld = P["n"] + P["m"], 2, P["n"] + P["m"] + 5
    sent = -12345.678
    Z = np.full((ld, k), sent, order="F")
    Bm = np.full((ld, k), sent, order="F")
    zs = [R.operands(name)["random"], R.operands(name)["nan"]]
    for j in range(k):
        Z[:N, j], Bm[:N, j] = zs[j], P["rhs"]
    Rm = np.full((ld, k), sent, order="F")
    nr = np.full(4 * k, sent)
    _lib.check(_lib.lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(Bm), ld, _dp(Rm), ld, _dp(nr)))
    for j, key in enumerate(("random", "nan")):
        assert R.same_bits(Rm[:N, j], _ref(name, key)[1])
    assert np.all(Rm[N:] == sent) and np.all(Z[N:] == sent) and np.all(Bm[N:] == sent)
    # in place, and norms alone, and R alone: the same bits
    B2, n2, R3 = Bm.copy(order="F"), np.full(4 * k, sent), np.full((ld, k), sent, order="F")
    _lib.check(_lib.lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(B2), ld, _dp(B2), ld, _dp(n2)))
    assert R.same_bits(B2, Rm) and R.same_bits(n2, nr)
    n3 = np.full(4 * k, sent)
    _lib.check(_lib.lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(Bm), ld, None, ld, _dp(n3)))
    _lib.check(_lib.lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(Bm), ld, _dp(R3), ld, None))
    assert R.same_bits(n3, nr) and R.same_bits(R3, Rm)
    # the NaN stays in its column
    assert np.all(np.isfinite(Rm[:N, 0])) and np.all(np.isfinite(nr[:4])) and np.any(np.isnan(nr[4:]))


@pytest.mark.parametrize("exact", (0, 1))
@pytest.mark.parametrize("name", BLOCK_MEMBERS)
def test_block_columns_equal_the_single_column_call(gpu_ctx, name, exact):
    """k = 1, 3, 7, 8, 9, 17 with the panel path forced, the loop path forced and the routing left
    to the crossover: every column's R and sums equal the single-column pass (the loop path on that
    column alone), at every position, in both modes; a NaN column leaves the others as they are"""
    import cpkrylov_amd as cpk
    P = R.system(name)
    K = _kkt(name, gpu_ctx)
    N = P["n"] + P["m"]
    rng = np.random.default_rng(77)
    cols = rng.standard_normal((N, 17))
    cols[N // 5, 4] = np.nan
    rhs = np.asfortranarray(P["rhs"][:, None] * (1.0 + np.arange(17.0))[None, :])
    ys = [K @ cols[:, j] for j in range(17)]
    info = K.route_info()
    assert info["panel_columns"] == 8 and 1 <= info["crossover"] <= 9 and info["route"] == "auto"
    with cpk.engine_options(gpu_ctx, exact_dots=exact):
        K.set_route("loop")
        single = [K.residual(cols[:, j], rhs[:, j]) for j in range(17)]
        assert K.route_info()["panels"] == 0
        for route in ("panel", "loop", "auto"):
            K.set_route(route)
            for k in (1, 3, 7, 8, 9, 17):
                for shift in (0, 17 - k):  # the same columns at other positions of the block
                    idx = [(shift + j) % 17 for j in range(k)]
                    before = K.route_info()["panels"]
                    Rm, nr = K.residual(cols[:, idx], rhs[:, idx])
                    ran = K.route_info()["panels"] - before
                    if route == "panel":
                        assert ran == -(-k // 8), (k, ran)
                    elif route == "loop":
                        assert ran == 0
                    else:
                        assert ran == sum(min(8, k - j0) >= info["crossover"] for j0 in range(0, k, 8)), (k, ran)
                    for q, j in enumerate(idx):
                        assert R.same_bits(Rm[:, q], single[j][0]), (route, k, j)
                        for key in ("rr_x", "rr_y", "bb_x", "bb_y"):
                            assert R.same_bits(nr[key][q], single[j][1][key]), (route, k, j, key)
        K.set_route("auto")
        Y = K @ cols
    for j in range(17):
        assert R.same_bits(Y[:, j], ys[j]), j
    # the reference, on a few columns (the product is checked against it in full elsewhere)
    Kr = R.operator(name)
    for j in (0, 4, 16):
        assert R.same_bits(single[j][0], R.residual(Kr, cols[:, j], rhs[:, j]))


@pytest.mark.parametrize("exact", (0, 1))
@pytest.mark.parametrize("name", ("tiny2x1", "arrow_row"))
def test_panel_path_in_place_padding_and_null_outputs(gpu_ctx, name, exact):
    """The forced panel path with leading dimensions above N, R over Bm, R alone and sums alone:
    the loop path's bits, the padding rows untouched"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P = R.system(name)
    K = _kkt(name, gpu_ctx)
    N, k = P["n"] + P["m"], 3
    ld, sent = N + 3, -777.25
    rng = np.random.default_rng(9)
    Z, Bm = np.full((ld, k), sent, order="F"), np.full((ld, k), sent, order="F")
    Z[:N], Bm[:N] = rng.standard_normal((N, k)), rng.standard_normal((N, k))
    Z[N // 2, 1] = np.nan
    lib = _lib.lib
    out = {}
    with cpk.engine_options(gpu_ctx, exact_dots=exact):
        for route in ("loop", "panel"):
            K.set_route(route)
            Rm, nr = np.full((ld, k), sent, order="F"), np.full(4 * k, sent)
            _lib.check(lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(Bm), ld, _dp(Rm), ld, _dp(nr)))
            B2, n2 = Bm.copy(order="F"), np.full(4 * k, sent)
            _lib.check(lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(B2), ld, _dp(B2), ld, _dp(n2)))
            n3, R3 = np.full(4 * k, sent), np.full((ld, k), sent, order="F")
            _lib.check(lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(Bm), ld, None, ld, _dp(n3)))
            _lib.check(lib.cpk_kkt_residual(K.h, k, _dp(Z), ld, _dp(Bm), ld, _dp(R3), ld, None))
            assert R.same_bits(B2, Rm) and R.same_bits(R3, Rm) and R.same_bits(n2, nr) and R.same_bits(n3, nr)
            assert np.all(Rm[N:] == sent) and np.all(Bm[N:] == sent) and np.all(Z[N:] == sent)
            out[route] = (Rm, nr)
    assert K.route_info()["panels"] == 4
    assert R.same_bits(out["panel"][0], out["loop"][0]) and R.same_bits(out["panel"][1], out["loop"][1])
    nr = out["panel"][1].reshape(k, 4)
    assert np.all(np.isfinite(nr[[0, 2]])) and np.any(np.isnan(nr[1]))


def test_device_operands(gpu_ctx):
    """The _device entries on device arrays: the bits of the host entries; sums to device memory
    or, through cpk_kkt_residual_device_sums, to host memory"""
    from cpkrylov_amd import _lib
    name = "tiny65x63"
    P = R.system(name)
    K = _kkt(name, gpu_ctx)
    N, k = P["n"] + P["m"], 3
    rng = np.random.default_rng(5)
    Z = np.asfortranarray(rng.standard_normal((N, k)))
    Bm = np.asfortranarray(rng.standard_normal((N, k)))
    Rh, nh = K.residual(Z, Bm)
    dZ, dB, dR, dn = DeviceArray.of(Z.ravel("F")), DeviceArray.of(Bm.ravel("F")), DeviceArray(N * k), DeviceArray(4 * k)
    _lib.check(_lib.lib.cpk_kkt_residual_device(K.h, k, dZ.p, N, dB.p, N, dR.p, N, dn.p))
    gpu_ctx.synchronize()
    assert R.same_bits(dR.numpy().reshape((N, k), order="F"), Rh)
    assert R.same_bits(dn.numpy().reshape(k, 4), np.stack([nh[q] for q in ("rr_x", "rr_y", "bb_x", "bb_y")], axis=1))
    hn = np.zeros(4 * k)
    _lib.check(_lib.lib.cpk_kkt_residual_device_sums(K.h, k, dZ.p, N, dB.p, N, dB.p, N, _dp(hn)))
    assert R.same_bits(hn, dn.numpy()) and R.same_bits(dB.numpy(), dR.numpy())  # in place, host sums
    dY = DeviceArray(N)
    _lib.check(_lib.lib.cpk_kkt_apply_device(K.h, dZ.p, dY.p))
    gpu_ctx.synchronize()
    assert R.same_bits(dY.numpy(), K @ Z[:, 0])


def test_python_front_end_on_device_tensors(gpu_ctx):
    """K @ z, K.residual and K.solve on device tensors (duck-typed, results in out=): the bits of
    the NumPy path; a block is a (k, N) row-major tensor, one column after the other"""
    assert torch is not None and torch.cuda.is_available()
    name = "cvxqp1_m"
    P = R.system(name)
    K = _kkt(name, gpu_ctx)
    N, k = K.N, 3
    rng = np.random.default_rng(12)
    Z, Bm = rng.standard_normal((N, k)), rng.standard_normal((N, k))
    Rh, nh = K.residual(Z, Bm)
    tz, tb = torch.from_numpy(Z.T.copy()).cuda(), torch.from_numpy(Bm.T.copy()).cuda()
    out = torch.zeros_like(tz)
    ro, nd = K.residual(tz, tb, out=out)
    assert ro is out and R.same_bits(out.cpu().numpy().T, Rh)
    for key in nh:
        assert R.same_bits(nd[key], nh[key]), key
    assert K.residual(tz, tb, want_r=False)[0] is None
    r1, n1 = K.residual(tz[1], tb[1], out=tb[1])  # one column, in place
    assert R.same_bits(tb[1].cpu().numpy(), Rh[:, 1]) and n1["rr_x"] == nh["rr_x"][1]
    K.apply(tz, out=out)
    assert R.same_bits(out.cpu().numpy().T, K @ Z)
    # the solve: cold into out=, then warm in place from 0.9 x
    opts = dict(F.EXPROG_OPTS)
    M = _precond(P, gpu_ctx, opts)
    b = torch.from_numpy(P["rhs"].copy()).cuda()
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    xh, sh, fh = K.solve("minres", P["rhs"], M, opts)
    xd, sd, fd = K.solve("minres", b, M, opts, out=x)
    assert xd is x and R.same_bits(x.cpu().numpy(), xh) and sd["true_resid"] == sh["true_resid"]
    _same_run(sd, fd, dict(sh, solved=fh["solved"]), fh)
    x.mul_(0.9)
    torch.cuda.synchronize()
    x0 = x.cpu().numpy()
    xw, sw, fw = K.solve("minres", P["rhs"], M, opts, x0=x0)
    K.solve("minres", b, M, opts, x0=x, out=x)
    assert R.same_bits(x.cpu().numpy(), xw)


def test_values_follow_the_handles(gpu_ctx):
    """Updates through set_values (host) and cpk_mat_set_values_device, of A alone, C alone and all
    three, one handle built from a CSR with duplicates: K @ z equals a freshly built KKT on the new
    values; the value array keeps its address; no regather when nothing changed"""
    import cpkrylov_amd as cpk
    P = R.system("tiny65x63")
    rng = np.random.default_rng(31)
    A, Cm, Bs = P["A"], P["C"], P["B"]
    ptr, ind, split = duplicated_csr(Bs, np.random.default_rng(32))

    def handles(va, vb_raw, vc):
        return (cpk.Matrix(type(A)((va, A.indices, A.indptr), shape=A.shape), ctx=gpu_ctx),
                raw_matrix("csr", Bs.shape, ptr, ind, vb_raw, ctx=gpu_ctx),
                cpk.Matrix(type(Cm)((vc, Cm.indices, Cm.indptr), shape=Cm.shape), ctx=gpu_ctx))

    va, vb, vc = A.data.copy(), split(Bs.data, np.random.default_rng(33)), Cm.data.copy()
    hA, hB, hC = handles(va, vb, vc)
    K = cpk.KKT(hA, hB, hC)
    z = rng.standard_normal(K.N)
    y0, i0 = K @ z, K.info()
    assert R.same_bits(K @ z, y0) and K.info() == i0 and i0["refreshes"] == 0  # nothing changed: no regather
    fresh0 = cpk.KKT(*handles(va, vb, vc))
    assert R.same_bits(y0, fresh0 @ z)
    gens = [0, 0, 0]
    steps = [("A", "host"), ("C", "device"), ("all", "host"), ("all", "device"), ("B", "device")]
    for step, (which, how) in enumerate(steps):
        if which in ("A", "all"):
            va = va * rng.uniform(0.5, 2.0, va.size)
        if which in ("B", "all"):
            vb = split(Bs.data * rng.uniform(0.5, 2.0, Bs.nnz), np.random.default_rng(40 + step))
        if which in ("C", "all"):
            vc = vc * rng.uniform(0.5, 2.0, vc.size)
        for q, (h, v, tag) in enumerate(((hA, va, "A"), (hB, vb, "B"), (hC, vc, "C"))):
            if which in (tag, "all"):
                if how == "host":
                    h.set_values(v)
                else:
                    d = DeviceArray.of(v)
                    h.set_values_device(d.p.value, v.size)
                gens[q] += 1
        y = K @ z
        info = K.info()
        assert R.same_bits(y, cpk.KKT(*handles(va, vb, vc)) @ z), (which, how)
        assert info["values_generations"] == tuple(gens) and info["values_address"] == i0["values_address"]
        assert info["refreshes"] == step + 1
        assert R.same_bits(K @ z, y) and K.info() == info


def _precond(P, ctx, opts):
    import cpkrylov_amd as cpk
    M = cpk.opLDL2(P["G"], P["B"], -P["C"], ctx=ctx)
    M._set(**{k: opts[k] for k in PC_PROPS if k in opts})
    return M


def _direct_reg_solve(ctx, K, M, method, opts, rhs):
    """cpk_reg_solve_device on K's handles with device arrays: (rc, message, x, stats, flag)"""
    from cpkrylov_amd import _lib, api
    st, hist, lq, qr = api._new_stats(api._hist_cap(method, opts, K.n, K.m))
    db, dx = DeviceArray.of(rhs), DeviceArray.of(np.zeros(K.N))
    rc = _lib.lib.cpk_reg_solve_device(ctx.h, _lib.METHODS[method], db.p, K.A.h, K.B.h, K.C.h, M.h,
                                       C.byref(_lib.make_opts(opts)), dx.p, C.byref(st))
    msg = _lib.lib.cpk_last_error().decode() if rc else ""
    stats, flag = api._stats_from(method, st, hist, lq, qr)
    return rc, msg, dx.numpy(), stats, flag


def _same_run(stats, flag, so, fo):
    assert stats["niters"] == so["niters"] and flag["solved"] == fo["solved"]
    for k in [k for k in so if k.endswith("History")]:
        assert R.same_bits(stats[k], so[k]), k


SOLVE_CASES = [("cvxqp1_m", "minres", {}), ("cvxqp1_m", "cg", {}), ("cvxqp2_s", "gmres", {"restart": 20}),
               ("tiny65x63", "minres", {})]


@pytest.mark.parametrize("name,method,extra", SOLVE_CASES)
def test_cold_and_warm_solve_default_mode(gpu_ctx, name, method, extra):
    """Cold: the bits of cpk_reg_solve_device.  Warm: x == x0 + dx with dx what
    cpk_reg_solve_device returns for the R of cpk_kkt_residual; res[0..3] the sums of x0's
    residual, res[4..7] those of the returned x's"""
    P = R.system(name)
    opts = dict(F.EXPROG_OPTS, **extra)
    K = _kkt(name, gpu_ctx)
    M = _precond(P, gpu_ctx, opts)
    b = P["rhs"]
    x, stats, flag = K.solve(method, b, M, opts)
    rc, _, xd, sd, fd = _direct_reg_solve(gpu_ctx, K, M, method, opts, b)
    assert rc == 0 and R.same_bits(x, xd)
    _same_run(stats, flag, sd, fd)
    r0, n0 = K.residual(np.zeros(K.N), b)
    r1, n1 = K.residual(x, b)
    assert stats["true_resid0"] == n0 and stats["true_resid"] == n1
    assert n0["rr_x"] == n0["bb_x"] and n0["rr_y"] == n0["bb_y"]
    # warm from 0.9 x
    x0 = 0.9 * x
    xw, sw, fw = K.solve(method, b, M, opts, x0=x0)
    rw, nw = K.residual(x0, b)
    rc, _, dx, sdx, fdx = _direct_reg_solve(gpu_ctx, K, M, method, opts, rw)
    assert rc == 0 and R.same_bits(xw, x0 + dx)
    _same_run(sw, fw, sdx, fdx)
    assert sw["true_resid0"] == nw and sw["true_resid"] == K.residual(xw, b)[1]
    assert R.same_bits(x0, 0.9 * x)  # the caller's x0 is not written


@pytest.mark.parametrize("name,method,extra", SOLVE_CASES)
def test_warm_solve_exact_mode_equals_the_oracle(gpu_ctx, name, method, extra):
    """x, niters, solved and every history of the warm-started solve equal the oracle's composition
    on the product's exported factors: the reference residual, O.reg_solve in exact mode, x0 + dx"""
    import cpkrylov_amd as cpk
    P = R.system(name)
    opts = dict(F.EXPROG_OPTS, **extra)
    b = P["rhs"]
    Kr = R.operator(name)
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        K = _kkt(name, gpu_ctx)
        M = _precond(P, gpu_ctx, opts)
        Mo = O.LDL2(P["G"], P["B"], -P["C"], factors=M.export_factors())
        Mo.set(**{k: float(opts[k]) for k in PC_PROPS if k in opts})
        with O.exact():
            x_cold, _ = O.reg_solve(method, b, P["A"], P["B"], P["C"], Mo, opts)
            x0 = 0.9 * x_cold
            r = R.residual(Kr, x0, b)
            dxo, so = O.reg_solve(method, r, P["A"], P["B"], P["C"], Mo, opts)
        xw, sw, fw = K.solve(method, b, M, opts, x0=x0)
    assert sw["niters"] == so["niters"] and fw["solved"] == so["solved"]
    for k in [k for k in so if k.endswith("History")]:
        assert R.same_bits(sw[k], so[k]), k
    assert R.same_bits(xw, x0 + dxo)
    assert R.same_bits(_sums_of(sw["true_resid0"]), R.sums(r, b, P["n"]))
    assert R.same_bits(_sums_of(sw["true_resid"]), R.sums(R.residual(Kr, xw, b), b, P["n"]))


def test_indefinite_stop_surfaces_with_the_drivers_message(gpu_ctx):
    """The reference's indefinite stop inside the driver (structures.tiny_indefinite under
    exact_dots, as tests/test_gpu_structures.py raises it) comes back with the driver's own code
    and message, cold and warm; x is x0 plus whatever the driver wrote"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P = S.tiny_indefinite()
    opts = dict(F.EXPROG_OPTS)
    with cpk.engine_options(gpu_ctx, exact_dots=1):
        K = cpk.KKT(P["Q"], P["B"], P["C"], ctx=gpu_ctx)
        M = _precond(P, gpu_ctx, opts)
        rc, msg, xd, _, _ = _direct_reg_solve(gpu_ctx, K, M, "minres", opts, P["rhs"])
        assert rc == _lib.CPK_ERR_INDEFINITE
        with pytest.raises(cpk.IndefiniteError) as e:
            K.solve("minres", P["rhs"], M, opts)
        assert e.value.code == rc and str(e.value) == msg
        assert R.same_bits(e.value.partial[0], xd)  # cold: what the driver wrote
        # warm from a point whose correction system stops the same way
        x0 = np.zeros(K.N)
        x0[0] = 2.0 ** -60  # r = b - K x0 differs from b in rounding at the most
        r, nr = K.residual(x0, P["rhs"])
        rcw, msgw, dxw, _, _ = _direct_reg_solve(gpu_ctx, K, M, "minres", opts, r)
        assert rcw == _lib.CPK_ERR_INDEFINITE
        with pytest.raises(cpk.IndefiniteError) as e:
            K.solve("minres", P["rhs"], M, opts, x0=x0)
        assert e.value.code == rcw and str(e.value) == msgw
        xw, res = e.value.partial
        assert R.same_bits(xw, x0 + dxw)
        assert R.same_bits(res[:4], _sums_of(nr)) and R.same_bits(res[4:], _sums_of(K.residual(xw, P["rhs"])[1]))


def test_refusals(gpu_ctx):
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    P = R.system("tiny65x63")
    # mismatched dimensions: opLDL2's messages
    with pytest.raises(cpk.CpkError) as e:
        cpk.KKT(P["B"], P["B"], P["C"], ctx=gpu_ctx)
    assert e.value.code == _lib.CPK_ERR_DIM and str(e.value) == "First and last arguments must be square."
    with pytest.raises(cpk.CpkError) as e:
        cpk.KKT(P["A"], P["B"].T.tocsr(), P["C"], ctx=gpu_ctx)
    assert e.value.code == _lib.CPK_ERR_DIM and str(e.value) == "Incompatible dimensions."
    # a distributed (sim) context
    g = cpk.SimGroup(1)
    ctx = cpk.Context(device=0, rank=0, nranks=1, simgroup=g, options=dict(dist1=1))
    try:
        with pytest.raises(cpk.CpkError) as e:
            cpk.KKT(P["A"], P["B"], P["C"], ctx=ctx)
        assert e.value.code == _lib.CPK_ERR_UNSUPPORTED
    finally:
        ctx.close()
    # NULL operands and short leading dimensions leave sentinel-filled outputs untouched
    K = _kkt("tiny65x63", gpu_ctx)
    N, sent = K.N, 4.25
    Z, Bm = np.ones((N, 2), order="F"), np.ones((N, 2), order="F")
    Rm, nr = np.full((N, 2), sent, order="F"), np.full(8, sent)
    lib = _lib.lib
    assert lib.cpk_kkt_residual(K.h, 2, None, N, _dp(Bm), N, _dp(Rm), N, _dp(nr)) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual(K.h, 2, _dp(Z), N, None, N, _dp(Rm), N, _dp(nr)) == _lib.CPK_ERR_ARGS
    for args in ((-1, N, N, N), (2, N - 1, N, N), (2, N, N - 1, N), (2, N, N, N - 1)):
        k, ldz, ldb, ldr = args
        assert lib.cpk_kkt_residual(K.h, k, _dp(Z), ldz, _dp(Bm), ldb, _dp(Rm), ldr, _dp(nr)) == _lib.CPK_ERR_DIM
    assert lib.cpk_kkt_residual(K.h, 0, _dp(Z), N, _dp(Bm), N, _dp(Rm), N, _dp(nr)) == _lib.CPK_OK
    assert np.all(Rm == sent) and np.all(nr == sent) and np.all(Z == 1.0) and np.all(Bm == 1.0)
    assert lib.cpk_kkt_apply(K.h, None, _dp(Rm)) == _lib.CPK_ERR_ARGS and np.all(Rm == sent)
    with pytest.raises(cpk.CpkError) as e:
        K @ np.ones(N + 1)
    assert e.value.code == _lib.CPK_ERR_DIM
