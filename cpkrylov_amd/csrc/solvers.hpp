// solvers.hpp -- host entry points of the device solvers (solvers.hip).
#pragma once
#include "dev.hpp"

namespace cpk {
// The operator-valued A (cpk_op): the caller's product y(0:n) = A*x(0:n), the
// handle's generation and flags (both enter the solver key) and its two call counters.  xin / uop:
// the fixed-address input and output of the per-iteration product, owned by the cached solver.
// fn == nullptr: A is the matrix inside AC.
struct OpHook {
    cpk_op_fn fn = nullptr;
    void *user = nullptr;
    uint64_t gen = 0;
    int flags = 0;
    int64_t *calls = nullptr, *fails = nullptr;
    double *xin = nullptr, *uop = nullptr;
    bool capturable() const { return (flags & CPK_OP_CAPTURABLE) != 0; }
};
// one call of fn on the context stream; a nonzero return throws CPK_ERR_CALLBACK naming the call
inline void op_call(Ctx &c, const OpHook &op, const double *d_x, double *d_y, int64_t n) {
    const int64_t k = ++*op.calls;
    const int rc = op.fn(op.user, d_x, d_y, n, (void *)c.stream);
    if (rc) {
        ++*op.fails;
        throw Error(CPK_ERR_CALLBACK, "the operator's callback returned " + std::to_string(rc) + " on call " +
                                          std::to_string(k) + " of this operator");
    }
}
// [x, y, stats, flag] = method(b, A, C, M, opts): d_b (n), d_xy (N), AC = blkdiag(A, C)
// op (in all three entries below): A is op's callback; AC is then blkdiag(0, C), n empty rows
// above C's, and Arows is not read.  Single GPU; the callers refuse the rest.
void method_solve_device(Ctx &c, int method, const double *d_b, const DMat &AC, Precond &M, const cpk_opts *opts,
                         double *d_xy, cpk_stats *stats, const OpHook *op = nullptr);
// reg_cpkrylov's shift + method + recovery (reg_cpkrylov.m:150-175): d_b (N), d_x (N)
// The shift's products: rows < n of Arows*xy0 (= A*xy0(1:n)) and of Btrows*xy0 restricted to
// columns >= bt_colmin (= B'*xy0(n+1:N)).
void reg_solve_device(Ctx &c, int method, const double *d_b, const DMat &AC, const DMat &Arows, const DMat &Btrows,
                      int64_t bt_colmin, Precond &M, const cpk_opts *opts, double *d_x, cpk_stats *stats,
                      const OpHook *op = nullptr, double *ws = nullptr);
// ws (optional): device memory for the shift's three vectors in place of the call's own allocations,
// reg_solve_ws(N, n) doubles, each vector on a 256-byte boundary of it.  A caller that keeps it (K of
// cpk_kkt_solve) hands the method the same addresses at every call, so the solver cached by M under
// them, with its captured graphs, is found again
inline size_t reg_solve_ws_part(int64_t len) { return ((size_t)std::max<int64_t>(len, 1) + 31) / 32 * 32; }
inline size_t reg_solve_ws(int64_t N, int64_t n) { return 2 * reg_solve_ws_part(N) + reg_solve_ws_part(n); }
int reg_shift_device(Ctx &c, const double *d_b, const DMat &Arows, const DMat &Btrows, int64_t bt_colmin, Precond &M,
                     double *d_b1, double *d_xy0);
// the same with A*xy0(1:n) made by one direct call of op's callback on xy0 and a buffer of this call
int reg_shift_device(Ctx &c, const double *d_b, const OpHook &op, const DMat &Btrows, int64_t bt_colmin, Precond &M,
                     double *d_b1, double *d_xy0);
// x = x0 + dx (the Recover functor of the shift's recovery; d_x may be d_x0), on the context stream
void launch_recover(Ctx &c, int64_t N, const double *d_x0, const double *d_dx, double *d_x);
// The lockstep block solve: column j of XY (N x k, [x; y]) is method(b(:, j), A, C, M, opts)
// (kernels/cpcg.m, kernels/cpminres.m), panels of kMultiKP columns sharing one Krylov product and
// one panel apply per iteration.  stats / col_status: k entries or null.  Returns CPK_OK or the
// status of the first failing column (its message in *errmsg); every column's outputs are written.
// What the block entries refuse (CPK_ERR_UNSUPPORTED): a distributed context or preconditioner, the
// handle semantics of residual_update, a method other than cpcg / cpminres.  method < 0: the panel
// product alone (the diagnostics), which needs the first only.  The callers check before they run.
void require_block_solve(const Ctx &c, const Precond &M, int method);
int method_solve_multi_device(Ctx &c, int method, int64_t k, const double *d_B, int64_t ldb, const DMat &AC, Precond &M,
                              const cpk_opts *opts, double *d_XY, int64_t ldxy, cpk_stats *stats, int *col_status,
                              std::string *errmsg);
// reg_cpkrylov's shift + method + recovery per column (reg_cpkrylov.m:152-175) of an N x k block
int reg_solve_multi_device(Ctx &c, int method, int64_t k, const double *d_B, int64_t ldb, const DMat &AC,
                           const DMat &Arows, const DMat &Btrows, int64_t bt_colmin, Precond &M, const cpk_opts *opts,
                           double *d_X, int64_t ldx, cpk_stats *stats, int *col_status, std::string *errmsg);
// diagnostic: the panel Krylov product alone (Y = blkdiag(A, C) * X, dots: 2 k inner products)
void debug_spmm(Ctx &c, const DMat &AC, Precond &M, int64_t k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy,
                double *d_dots);
void debug_spmm_time(Ctx &c, const DMat &AC, Precond &M, int kc, int reps, double *ms_panel, double *ms_single);
// diagnostics: nv inner products of n-vectors through the solvers' reducing launches (device
// pointers; collective on a distributed context), and out[i] = xnorm2(a[i], b[i])
void debug_dot(Ctx &c, int kind, int64_t n, int nv, const double *d_A, int64_t lda, const double *d_B, int64_t ldb,
               int grid, double *d_out);
void debug_xnorm2(Ctx &c, int64_t n, const double *d_a, const double *d_b, double *d_out);
// diagnostic (cpk_debug_arnoldi_step): one Arnoldi step of cpgmres / cpdqgmres through the solvers' own
// launches.  s: the caller's description (its scalars are read and written, its H / c / s / g / H_dots
// are host arrays in the engine's storage); the vectors are device arrays with leading dimension
// max(N, 1).  Collective on a distributed context.
void debug_arnoldi_step(Ctx &c, cpk_arnoldi_step &s, double *d_V, double *d_PV, double *d_xy, const double *d_w,
                        const double *d_ut);
void profile_kernels(Ctx &c, const DMat &AC, Precond &M, int reps, cpk_profile *out);
// op: AC is blkdiag(0, C); the product's model adds the gather and the epilogue's read of fn's
// output (24 n), cpminres runs unfused, and fn's own traffic is unknown and not counted
// basis_f32: the solve ran with the float basis (cpgmres / cpdqgmres only)
double method_bytes(int method, const DMat &AC, const Precond &M, int64_t iters, const cpk_opts *opts,
                    const OpHook *op = nullptr, bool basis_f32 = false);
}  // namespace cpk
