"""The exactly rounded residual on the GPU (cpk_kkt_residual_exact*, KKT.residual_exact) against
tests/resid_exact_ref.py, BIT FOR BIT: r_i = RN(b_i - sum_e K_ie z_col(e)) on the structure family,
both fixtures and a system with a row beyond the staging capacity; hand-built rows that force every
path of the kernel; blocks whose columns do not depend on k or position, in place, with padded
leading dimensions; sums equal to cpk_kkt_residual's on that r and b; the refusals; values that
follow set_values."""
import ctypes as C

import numpy as np
import pytest

try:  # before libcpk initialises HIP
    import torch
except Exception:  # noqa: BLE001
    torch = None

import kkt_ref as R
import resid_exact_ref as E
from devbuf import DeviceArray

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
KEYS = ("rr_x", "rr_y", "bb_x", "bb_y")


def _dp(a):
    return a.ctypes.data_as(PD)


def _kkt(name, ctx):
    import cpkrylov_amd as cpk
    P = R.system(name)
    return cpk.KKT(P["A"], P["B"], P["C"], ctx=ctx)


def _sums_of(nr, q=None):
    return np.array([nr[k] if q is None else nr[k][q] for k in KEYS], dtype=np.float64)


def _plain_sums(K, r, b):
    """cpk_kkt_residual's four sums on (r, b): with z = 0 its residual is its right-hand side, so
    the sums of r come from the call on r and those of b from the call on b, each at its own
    accumulation site"""
    zero = np.zeros(K.N)
    return np.concatenate([_sums_of(K.residual(zero, r, want_r=False)[1])[:2],
                           _sums_of(K.residual(zero, b, want_r=False)[1])[2:]])


@pytest.mark.parametrize("name", E.SYSTEMS)
def test_residual_bit_for_bit(gpu_ctx, name):
    """r == the reference on a random operand and on b = the plain product (where the plain residual
    is zero in every row); the sums are cpk_kkt_residual's on (r, b) in both exact_dots settings"""
    import cpkrylov_amd as cpk
    K = _kkt(name, gpu_ctx)
    for key, (z, b) in E.operands(name).items():
        want, plain = E.reference(name, key)
        r, nr = K.residual_exact(z, b)
        assert E.same(r, want), (key, np.flatnonzero(r != want)[:5])
        assert np.any(r != K.residual(z, b)[0]), key  # the plain pass is another function
        assert E.same(_sums_of(nr), _plain_sums(K, r, b)), key
        with cpk.engine_options(gpu_ctx, exact_dots=1):
            rx, nx = K.residual_exact(z, b)
            assert E.same(rx, want) and E.same(_sums_of(nx), _plain_sums(K, r, b)), key
            assert E.same(_sums_of(nx), R.sums(want, b, R.system(name)["n"])), key


def test_hand_built_rows_force_every_path(gpu_ctx):
    """cancellation to the last bit, ties to even both ways, 2^1000 beside 2^-1000 (a cascade
    residue), a partial sum beyond 2^1023 with a finite total, subnormal results, an empty row; an
    inf and a NaN in z give NaN exactly in the rows that store their columns"""
    import cpkrylov_amd as cpk
    H = E.hand()
    K = cpk.KKT(H["A"], H["B"], H["C"], ctx=gpu_ctx)
    row = {nm: i for i, nm in enumerate(H["names"])}
    want = E.residual(H["K"], H["z"], H["b"])
    r, nr = K.residual_exact(H["z"], H["b"])
    assert E.same(r, want), (r, want)
    assert r[row["tie_down"]] == 1.0 and r[row["tie_up"]] == 1.0 + 2.0 ** -51
    assert r[row["wide_exponents"]] == 1.0 + 2.0 ** -52 and r[row["partial_overflow"]] == 1.5 * 2.0 ** 1023
    assert r[row["subnormal"]] == 2.0 ** -1074 and r[row["empty"]] == 0.75
    assert r[row["cancel_to_last_bit"]] != 0.0 and np.all(np.isfinite(r))
    wn = E.residual(H["K"], H["z_nonfinite"], H["b"])
    Z = np.asfortranarray(np.stack([H["z_nonfinite"], H["z"]], axis=1))
    Rm, nm = K.residual_exact(Z, np.asfortranarray(np.stack([H["b"], H["b"]], axis=1)))
    assert E.same(Rm[:, 0], wn) and np.isnan(wn).any() and not np.isnan(wn).all()
    assert E.same(Rm[:, 1], want)  # the NaN column leaves its neighbour alone
    assert np.isnan(nm["rr_x"][0]) and E.same(_sums_of(nm, 1), _sums_of(nr))


@pytest.mark.parametrize("name", ("tiny65x63", "arrow_row"))
def test_block_form(gpu_ctx, name):
    """k in {0, 1, 3, 9}: a column's bits depend neither on k nor on its position; R == Bm in place;
    leading dimensions above N leave the padding untouched; R or norms may be NULL; the host entry
    and both device entries agree; sums equal cpk_kkt_residual's on (r, b) in both modes"""
    import cpkrylov_amd as cpk
    from cpkrylov_amd import _lib
    lib = _lib.lib
    K = _kkt(name, gpu_ctx)
    N = K.N
    rng = np.random.default_rng(303)
    cols = rng.standard_normal((N, 9))
    cols[N // 4, 2] = np.nan
    rhs = np.asfortranarray(np.stack([R.matvec(R.operator(name), cols[:, j]) if j % 2 else R.system(name)["rhs"] * (1.0 + j)
                                      for j in range(9)], axis=1))
    for exact in (0, 1):
        with cpk.engine_options(gpu_ctx, exact_dots=exact):
            single = [K.residual_exact(cols[:, j], rhs[:, j]) for j in range(9)]
            for j in (0, 1):
                assert E.same(_sums_of(single[j][1]), _plain_sums(K, single[j][0], rhs[:, j])), (exact, j)
            assert np.isnan(single[2][1]["rr_x"]) or np.isnan(single[2][1]["rr_y"])  # the NaN column's own sums
            for k in (0, 1, 3, 9):
                for shift in (0, 9 - k):
                    idx = [(shift + j) % 9 for j in range(k)]
                    ld, sent = N + 3, -321.5
                    Z, Bm = np.full((ld, max(k, 1)), sent, order="F"), np.full((ld, max(k, 1)), sent, order="F")
                    Z[:N, :k], Bm[:N, :k] = cols[:, idx], rhs[:, idx]
                    Rm, nr = np.full((ld, max(k, 1)), sent, order="F"), np.full(4 * max(k, 1), sent)
                    _lib.check(lib.cpk_kkt_residual_exact(K.h, k, _dp(Z), ld, _dp(Bm), ld, _dp(Rm), ld, _dp(nr)))
                    assert np.all(Rm[N:] == sent) and np.all(Z[N:] == sent) and np.all(Bm[N:] == sent)
                    if k == 0:
                        assert np.all(Rm == sent) and np.all(nr == sent)
                        continue
                    for q, j in enumerate(idx):
                        assert E.same(Rm[:N, q], single[j][0]), (exact, k, j)
                        assert E.same(nr[4 * q:4 * q + 4], _sums_of(single[j][1])), (exact, k, j)
                    # in place, sums alone, R alone
                    B2, n2 = Bm.copy(order="F"), np.full(4 * k, sent)
                    _lib.check(lib.cpk_kkt_residual_exact(K.h, k, _dp(Z), ld, _dp(B2), ld, _dp(B2), ld, _dp(n2)))
                    n3, R3 = np.full(4 * k, sent), np.full((ld, k), sent, order="F")
                    _lib.check(lib.cpk_kkt_residual_exact(K.h, k, _dp(Z), ld, _dp(Bm), ld, None, ld, _dp(n3)))
                    _lib.check(lib.cpk_kkt_residual_exact(K.h, k, _dp(Z), ld, _dp(Bm), ld, _dp(R3), ld, None))
                    assert E.same(B2, Rm) and E.same(R3, Rm) and E.same(n2, nr) and E.same(n3, nr)
                    # the device entries on the same padded block: sums to device memory, and to host memory in place
                    dZ, dB, dR, dn = (DeviceArray.of(Z.ravel("F")), DeviceArray.of(Bm.ravel("F")),
                                      DeviceArray.of(np.full(ld * k, sent)), DeviceArray(4 * k))
                    _lib.check(lib.cpk_kkt_residual_exact_device(K.h, k, dZ.p, ld, dB.p, ld, dR.p, ld, dn.p))
                    gpu_ctx.synchronize()
                    assert E.same(dR.numpy().reshape((ld, k), order="F"), Rm) and E.same(dn.numpy(), nr)
                    hn = np.zeros(4 * k)
                    _lib.check(lib.cpk_kkt_residual_exact_device_sums(K.h, k, dZ.p, ld, dB.p, ld, dB.p, ld, _dp(hn)))
                    assert E.same(hn, nr) and E.same(dB.numpy().reshape((ld, k), order="F"), Rm)


def test_device_tensors_through_python(gpu_ctx):
    assert torch is not None and torch.cuda.is_available()
    name = "tiny65x63"
    K = _kkt(name, gpu_ctx)
    z, b = E.operands(name)["cancel"]
    want = E.reference(name, "cancel")[0]
    tz, tb = torch.from_numpy(z.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    out = torch.zeros_like(tz)
    ro, nd = K.residual_exact(tz, tb, out=out)
    assert ro is out and E.same(out.cpu().numpy(), want)
    rh, nh = K.residual_exact(z, b)
    assert nd == nh
    K.residual_exact(tz, tb, out=tb)  # in place
    assert E.same(tb.cpu().numpy(), want)


def test_refusals_in_cpk_kkt_residuals_order(gpu_ctx):
    """NULL arguments, k < 0 and short leading dimensions: cpk_kkt_residual's codes, in its order
    (a NULL operand beside a short leading dimension is the NULL refusal), nothing written"""
    from cpkrylov_amd import _lib
    lib = _lib.lib
    K = _kkt("tiny65x63", gpu_ctx)
    N, sent = K.N, 4.25
    Z, Bm = np.ones((N, 2), order="F"), np.ones((N, 2), order="F")
    Rm, nr = np.full((N, 2), sent, order="F"), np.full(8, sent)
    cases = [(2, None, N, _dp(Bm), N, N), (2, _dp(Z), N, None, N, N), (2, None, N - 1, _dp(Bm), N, N),
             (-1, _dp(Z), N, _dp(Bm), N, N), (2, _dp(Z), N - 1, _dp(Bm), N, N), (2, _dp(Z), N, _dp(Bm), N - 1, N),
             (2, _dp(Z), N, _dp(Bm), N, N - 1)]
    for k, zp, ldz, bp, ldb, ldr in cases:
        want = lib.cpk_kkt_residual(K.h, k, zp, ldz, bp, ldb, _dp(Rm), ldr, _dp(nr))
        assert want in (_lib.CPK_ERR_ARGS, _lib.CPK_ERR_DIM)
        assert lib.cpk_kkt_residual_exact(K.h, k, zp, ldz, bp, ldb, _dp(Rm), ldr, _dp(nr)) == want
    dZ, dB, dR, dn = DeviceArray.of(Z.ravel("F")), DeviceArray.of(Bm.ravel("F")), DeviceArray.of(Rm.ravel("F")), DeviceArray.of(nr)
    for k, ldz, ldb, ldr in ((-1, N, N, N), (2, N - 1, N, N), (2, N, N - 1, N), (2, N, N, N - 1)):
        assert lib.cpk_kkt_residual_exact_device(K.h, k, dZ.p, ldz, dB.p, ldb, dR.p, ldr, dn.p) == _lib.CPK_ERR_DIM
        assert lib.cpk_kkt_residual_exact_device_sums(K.h, k, dZ.p, ldz, dB.p, ldb, dR.p, ldr, _dp(nr)) == _lib.CPK_ERR_DIM
    assert lib.cpk_kkt_residual_exact_device(K.h, 2, None, N, dB.p, N, dR.p, N, dn.p) == _lib.CPK_ERR_ARGS
    assert lib.cpk_kkt_residual_exact_device_sums(K.h, 2, dZ.p, N, dB.p, N, dR.p, N, None) == _lib.CPK_ERR_ARGS
    assert np.all(Rm == sent) and np.all(nr == sent) and np.all(Z == 1.0) and np.all(Bm == 1.0)
    assert np.all(dR.numpy() == sent) and np.all(dn.numpy() == sent) and np.all(dB.numpy() == 1.0)


def test_values_follow_set_values(gpu_ctx):
    """after set_values on A the residual is the new matrix's, by one regather"""
    import cpkrylov_amd as cpk
    P = R.system("tiny65x63")
    A = P["A"]
    hA = cpk.Matrix(A, ctx=gpu_ctx)
    K = cpk.KKT(hA, P["B"], P["C"], ctx=gpu_ctx)
    z, b = E.operands("tiny65x63")["random"]
    assert E.same(K.residual_exact(z, b)[0], E.reference("tiny65x63", "random")[0])
    va = A.data * np.random.default_rng(5).uniform(0.5, 2.0, A.nnz)
    hA.set_values(va)
    A2 = type(A)((va, A.indices, A.indptr), shape=A.shape)
    before = K.info()["refreshes"]
    r = K.residual_exact(z, b)[0]
    assert K.info()["refreshes"] == before + 1
    assert E.same(r, E.residual(R.assemble(A2, P["B"], P["C"]), z, b))
    assert E.same(K.residual_exact(z, b)[0], r) and K.info()["refreshes"] == before + 1
