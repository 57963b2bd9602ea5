// kkt_driver.cpp -- the drivers of the saddle-point operator K = [A B'; B -C]: assembly, product,
// true residual (plain and exactly rounded), the verified solve with its warm start, the refined
// solve, the adjoint's gradient passes and the block forms.  The cpk_kkt_* entries (capi.cpp) check
// and stage; what runs on the device between is enqueued here.
#include "kkt_driver.hpp"

#include <cstring>
#include <exception>

namespace cpk {

void kkt_assemble(cpk_kkt k) {
    cpk_mat A = k->A, B = k->B, C = k->C;
    HCsr negC = C->host();
    for (auto &v : negC.val) v = -v;
    const HCsr &ha = A->host(), &hb = B->host();
    make_dmat(assemble_kp(ha, hb, negC), k->K);
    const std::vector<int64_t> ks = kp_value_sources(ha, hb, negC);
    const int64_t off[3] = {0, ha.nnz(), ha.nnz() + hb.nnz()};
    std::vector<uint32_t> src(ks.size());
    for (size_t q = 0; q < ks.size(); q++) src[q] = (uint32_t)(off[ks[q] >> 40] + (ks[q] & ((int64_t(1) << 40) - 1)));
    k->src.upload(src);
    k->norms.alloc(8);
    const cpk_mat_s *h[3] = {A, B, C};
    for (int i = 0; i < 3; i++) k->gen[i] = h[i]->gen, k->vgen[i] = h[i]->vgen;
}

void kkt_apply(cpk_kkt K, const double *d_z, double *d_y) { launch_kkt_apply(K->ctx->c, K->current(), d_z, d_y); }

// Panels of kMultiKP columns.  A panel below the measured crossover (or with the loop forced) is a
// loop of single-column passes.  Otherwise K is streamed once for the panel (kkt_panel_kernel: every
// column's R in spmv_stream's row order) and each column's sums are taken from its r and b by
// kkt_sums_kernel in the single-column pass's order -- so either path gives a column the same
// bits, and the routing cannot change one.  r goes to a work array when the caller wants no R or
// wants it over Bm (the sums read b after r exists), and is copied over Bm afterwards.
void kkt_resid_block(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_B, int64_t ldb, double *d_R,
                     int64_t ldr, double *d_norms) {
    const DMat &Kd = K->current();
    Ctx &c = K->ctx->c;
    const int64_t N = K->n + K->m;
    if (!d_R && !d_norms) return;
    for (int64_t j0 = 0; j0 < k; j0 += kMultiKP) {
        const int kc = (int)std::min<int64_t>(kMultiKP, k - j0);
        const bool panel = N > 0 && (K->route == 1 || (K->route == 0 && kc >= kKktPanelMinCols));
        if (!panel) {
            for (int64_t j = j0; j < j0 + kc; j++)
                launch_kkt_resid(c, Kd, K->n, d_Z + j * ldz, d_B + j * ldb, d_R ? d_R + j * ldr : nullptr,
                                 d_norms ? d_norms + 4 * j : nullptr);
            continue;
        }
        const size_t pn = (size_t)N * kMultiKP;
        const bool aside = !d_R || d_R == d_B;
        if (aside && K->Tp.n < pn) K->Tp.alloc(pn);
        double *dst = aside ? K->Tp.p : d_R + j0 * ldr;
        const int64_t ldd = aside ? N : ldr;
        launch_kkt_panel(c, Kd, kc, d_Z + j0 * ldz, ldz, d_B + j0 * ldb, ldb, dst, ldd);
        if (d_norms)
            for (int j = 0; j < kc; j++)
                launch_kkt_sums(c, Kd, K->n, dst + j * ldd, d_B + (j0 + j) * ldb, d_norms + 4 * (j0 + j));
        if (d_R && aside)
            CPK_HIP(hipMemcpy2DAsync(d_R + j0 * ldr, (size_t)ldr * sizeof(double), dst, (size_t)ldd * sizeof(double),
                                     (size_t)N * sizeof(double), (size_t)kc, hipMemcpyDeviceToDevice, c.stream));
        K->panels++;
    }
}

// ---- the exactly rounded residual: cpk_kkt_residual's entries with r_i = RN(exact row sum) --------
// A block is a loop of single-column passes (no panel kernel, no routing): launch_kkt_resid_exact
// forms a column's r, kkt_sums_kernel takes its sums from the stored r and b in the single-column
// pass's order, so they are what cpk_kkt_residual's sums would be on that r and b.  r goes to K's
// work array when the caller wants no R or wants it over Bm (the sums read b after r exists).
void kkt_resid_exact_block(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_B, int64_t ldb, double *d_R,
                           int64_t ldr, double *d_norms) {
    const DMat &Kd = K->current();
    Ctx &c = K->ctx->c;
    const int64_t N = K->n + K->m;
    if (!d_R && !d_norms) return;
    const bool aside = d_norms && (!d_R || d_R == d_B);
    if (aside && K->Tp.n < (size_t)N) K->Tp.alloc((size_t)N * kMultiKP);  // the panel path's size
    for (int64_t j = 0; j < k; j++) {
        const double *b = d_B + j * ldb;
        double *dst = aside ? K->Tp.p : d_R + j * ldr;
        launch_kkt_resid_exact(c, Kd, d_Z + j * ldz, b, dst);
        if (d_norms) launch_kkt_sums(c, Kd, K->n, dst, b, d_norms + 4 * j);
        if (d_R && aside && N)
            CPK_HIP(hipMemcpyAsync(d_R + j * ldr, dst, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    }
}

// What the verified solve and the refined one set up alike: the checks against M, K on current
// values, the Krylov operator, the shift's, and the driver's vectors.  Those live in K, so every call
// hands the method the same addresses and finds the solver M cached under them (solver_key):
// [shift's three; then `parts` of warm residual, warm correction, the refined solve's trial]
struct SolveSetup {
    Precond &p;
    const DMat &Kd, &AC;
    ShiftOps so;
    double *ws, *r;  // the driver's vectors, the parts after them
    size_t part;
};
static SolveSetup solve_setup(cpk_kkt K, cpk_pc M, int parts, cpk_stats *stats, const char *other_ctx) {
    cpk_mat A = K->A, C = K->C;
    need(M->ctx == K->ctx, other_ctx);
    check_method_dims(A, C, M);
    Precond &p = *M->p;
    const int64_t N = K->n + K->m;
    const DMat &Kd = K->current();
    const DMat &AC = A->krylov_op(C, p);
    const ShiftOps so = shift_ops(A, C, p);
    const size_t wsn = reg_solve_ws(N, K->n), part = reg_solve_ws_part(N);
    if (K->ws.n < wsn + parts * part) K->ws.alloc(wsn + parts * part);
    if (stats) stats->ptime = p.ptime;  // also where the driver stops with its error
    return {p, Kd, AC, so, K->ws.p, K->ws.p + wsn, part};
}

// cold: reg_cpkrylov's driver on b (cpk_reg_solve_device's call exactly).  warm: r = b - K*x0, the
// same driver on r (its shift included, reg_cpkrylov.m:152-175), x = x0 + dx.  res (host, 8):
// the four sums of the start residual, then those of b - K*x for the returned x.
void kkt_solve_core(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x, int warm,
                    cpk_stats *stats, double *res) {
    const SolveSetup s = solve_setup(K, M, 2, stats, "kkt_solve: M belongs to another context");
    Ctx &c = K->ctx->c;
    const int64_t N = K->n + K->m;
    double *dn = K->norms.p;
    auto finish = [&] {
        launch_kkt_resid(c, s.Kd, K->n, d_x, d_b, nullptr, dn + 4);
        if (res) CPK_HIP(hipMemcpyAsync(res, dn, 8 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
    };
    if (!warm) {
        // the start residual of x = 0 is b: its sums in the residual pass's order, K not streamed
        if (N) CPK_HIP(hipMemsetAsync(d_x, 0, N * sizeof(double), c.stream));
        launch_kkt_sums(c, s.Kd, K->n, d_b, d_b, dn);
        try {
            reg_solve_device(c, method, d_b, s.AC, *s.so.A, *s.so.Bt, s.so.bt_colmin, s.p, opts, d_x, stats, nullptr, s.ws);
        } catch (...) {
            finish();
            throw;
        }
    } else {
        double *r = s.r, *dx = r + s.part;
        CPK_HIP(hipMemsetAsync(dx, 0, (size_t)std::max<int64_t>(N, 1) * sizeof(double), c.stream));
        launch_kkt_resid(c, s.Kd, K->n, d_x, d_b, r, dn);
        std::exception_ptr err;
        try {
            reg_solve_device(c, method, r, s.AC, *s.so.A, *s.so.Bt, s.so.bt_colmin, s.p, opts, dx, stats, nullptr, s.ws);
        } catch (...) {
            err = std::current_exception();
        }
        launch_recover(c, N, d_x, dx, d_x);  // x0 plus whatever the driver wrote
        if (err) {
            finish();
            std::rethrow_exception(err);
        }
    }
    finish();
}

// ---- iterative refinement on the exactly rounded residual (cpk_kkt_solve_refined) ----------------
// x_0 = x0 (warm) or 0; driver call j = 0 .. max_steps runs reg_solve_device on r_j = the exactly
// rounded b - K*x_j (cold, j = 0: on b itself, which that residual is) from a zero start and gives
// the trial x_j + dx_j, one rounding per entry.  r_{j+1} is formed at the trial: unless its sum of
// squares is below r_j's the trial is dropped and the loop ends with x_j; the last call's trial
// (j = max_steps) is taken as cpk_kkt_solve takes its own, without a further residual.  A driver
// error ends the loop with x_j plus whatever the driver wrote.  The driver's vectors, r, dx and the
// trial live in K (kkt_solve_core's layout plus the trial), at the same addresses on every call.
void kkt_refined_core(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x, int warm,
                      int max_steps, cpk_stats *stats, double *res, int *steps_out, bool *wrote_x) {
    const SolveSetup s = solve_setup(K, M, 3, stats, "kkt_solve_refined: M belongs to another context");
    Ctx &c = K->ctx->c;
    const int64_t N = K->n + K->m;
    const size_t nb = (size_t)N * sizeof(double);
    double *dn = K->norms.p, *r = s.r, *dx = r + s.part, *xt = dx + s.part;
    if (steps_out) *steps_out = 0;
    if (wrote_x) *wrote_x = true;  // every refusal is behind us: from here on d_x holds an iterate
    // the four sums of residual `row` (rv against b), to res; returns sum r^2
    auto sums = [&](const double *rv, int row) {
        double h[4];
        launch_kkt_sums(c, s.Kd, K->n, rv, d_b, dn);
        CPK_HIP(hipMemcpyAsync(h, dn, sizeof h, hipMemcpyDeviceToHost, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
        if (res) std::memcpy(res + 4 * (size_t)row, h, sizeof h);
        return h[0] + h[1];
    };
    auto take_trial = [&] {
        if (N) CPK_HIP(hipMemcpyAsync(d_x, xt, nb, hipMemcpyDeviceToDevice, c.stream));
    };
    double rr;
    if (!warm) {
        if (N) CPK_HIP(hipMemsetAsync(d_x, 0, nb, c.stream));
        rr = sums(d_b, 0);  // the start residual of x = 0 is b
    } else {
        launch_kkt_resid_exact(c, s.Kd, d_x, d_b, r);
        rr = sums(r, 0);
    }
    int applied = 0;
    for (int j = 0; j <= max_steps; j++) {
        const bool on_b = !warm && j == 0;
        double *out = on_b ? xt : dx;
        CPK_HIP(hipMemsetAsync(out, 0, (size_t)std::max<int64_t>(N, 1) * sizeof(double), c.stream));
        std::exception_ptr err;
        try {
            reg_solve_device(c, method, on_b ? d_b : r, s.AC, *s.so.A, *s.so.Bt, s.so.bt_colmin, s.p, opts, out, stats,
                             nullptr, s.ws);
        } catch (...) {
            err = std::current_exception();
        }
        if (!on_b) launch_recover(c, N, d_x, dx, xt);
        if (err || j == max_steps) {
            take_trial();
            applied++;
            CPK_HIP(hipStreamSynchronize(c.stream));
            if (steps_out) *steps_out = applied - 1;
            if (err) std::rethrow_exception(err);
            return;
        }
        launch_kkt_resid_exact(c, s.Kd, xt, d_b, r);
        const double rn = sums(r, j + 1);
        if (!(rn < rr)) break;  // no decrease (or a NaN): this dx is not applied
        take_trial();
        applied++;
        rr = rn;
    }
    CPK_HIP(hipStreamSynchronize(c.stream));
    if (steps_out) *steps_out = applied - 1;
}

// ---- the adjoint of the verified solve: lambda = K' \ gx, then the value gradients sampled on K's
// own handles (adjoint.hip).  A stop inside the driver leaves through kkt_solve_core's exception
// before any gradient pass is enqueued.  d_x, d_lam: N device values each; d_g*: device arrays of
// the handles' entry counts (or null)
void kkt_adjoint_core(cpk_kkt K, cpk_kkt KT, int method, const double *d_x, const double *d_gx, cpk_pc M, const cpk_opts *opts,
                      double *d_lam, int warm, double *d_gA, double *d_gB, double *d_gC, cpk_stats *stats, double *res) {
    kkt_solve_core(KT ? KT : K, method, d_gx, M, opts, d_lam, warm, stats, res);
    if (!d_gA && !d_gB && !d_gC) return;
    Ctx &c = K->ctx->c;
    const int64_t n = K->n;
    // gB's two terms pair x with lambda both ways, U = [lambda_y, x_y] and V = [x_x, lambda_x]: the
    // second column of each lies in the other vector, so the kernel's column stride is the distance
    // between the two vectors in doubles, positive for one operand and negative for the other (two
    // device arrays of doubles; the launcher takes any stride, the public entries only ld >= rows)
    const int64_t lam_to_x = ((int64_t)(intptr_t)d_x - (int64_t)(intptr_t)d_lam) / (int64_t)sizeof(double);
    auto pass = [&](cpk_mat_s *H, int64_t k, const double *U, int64_t ldu, const double *V, int64_t ldv, double alpha,
                    double *out) {
        if (!out) return;
        const DMat &d = H->dev();
        upload_value_map(H->vm, H->dvm);
        launch_sample_outer(c, d, H->vm, H->dvm, k, U, ldu, V, ldv, alpha, out);
    };
    pass(K->A, 1, d_lam, 0, d_x, 0, -1.0, d_gA);                          // -lambda_x * x_x'
    pass(K->B, 2, d_lam + n, lam_to_x, d_x, -lam_to_x, -1.0, d_gB);       // -(lambda_y * x_x' + x_y * lambda_x')
    pass(K->C, 1, d_lam + n, 0, d_x + n, 0, 1.0, d_gC);                   // +lambda_y * x_y' (K holds -C)
}

// ---- the block forms of the verified solve and of its adjoint --------------------------------------
// Column j is cpk_kkt_solve on B(:, j): the driver is reg_solve_multi_device unchanged (no routing by
// k), the start sums are launch_kkt_sums of b_j (cold) or the block residual's (warm), the last four
// those of one block residual of the returned X.  res: host, 8 k (or null).  Returns CPK_OK or the
// first failing column's status (message in *msg)
int kkt_solve_multi_core(cpk_kkt K, int method, int64_t k, const double *d_B, int64_t ldb, cpk_pc M, const cpk_opts *opts,
                         double *d_X, int64_t ldx, int warm, cpk_stats *stats, int *col_status, double *res, std::string *msg) {
    if (k == 0) return CPK_OK;
    cpk_mat A = K->A, C = K->C;
    Ctx &c = K->ctx->c;
    Precond &p = *M->p;
    const int64_t N = K->n + K->m, N1 = std::max<int64_t>(N, 1);
    const DMat &Kd = K->current();
    const DMat &AC = A->krylov_op(C, p);
    const ShiftOps so = shift_ops(A, C, p);
    // [8 k: the call's sums, column by column; 4 k: a block residual's sums before they are spread]
    if (K->normsb.n < 12 * (size_t)k) K->normsb.alloc(12 * (size_t)k);
    double *dn = K->normsb.p, *dt = dn + 8 * k;
    auto spread = [&](int at) {  // dt[4 j ..] -> dn[8 j + at ..]
        CPK_HIP(hipMemcpy2DAsync(dn + at, 8 * sizeof(double), dt, 4 * sizeof(double), 4 * sizeof(double), (size_t)k,
                                 hipMemcpyDeviceToDevice, c.stream));
    };
    int rc;
    if (!warm) {
        for (int64_t j = 0; j < k; j++) {
            if (N) CPK_HIP(hipMemsetAsync(d_X + j * ldx, 0, N * sizeof(double), c.stream));
            launch_kkt_sums(c, Kd, K->n, d_B + j * ldb, d_B + j * ldb, dn + 8 * j);
        }
        rc = reg_solve_multi_device(c, method, k, d_B, ldb, AC, *so.A, *so.Bt, so.bt_colmin, p, opts, d_X, ldx, stats,
                                    col_status, msg);
    } else {
        const size_t blk = (size_t)N1 * (size_t)k;
        if (K->wsb.n < 2 * blk) K->wsb.alloc(2 * blk);
        double *R = K->wsb.p, *dX = R + blk;
        CPK_HIP(hipMemsetAsync(dX, 0, blk * sizeof(double), c.stream));
        kkt_resid_block(K, k, d_X, ldx, d_B, ldb, R, N1, dt);
        spread(0);
        rc = reg_solve_multi_device(c, method, k, R, N1, AC, *so.A, *so.Bt, so.bt_colmin, p, opts, dX, N1, stats, col_status,
                                    msg);
        for (int64_t j = 0; j < k; j++) launch_recover(c, N, d_X + j * ldx, dX + j * N1, d_X + j * ldx);
    }
    kkt_resid_block(K, k, d_X, ldx, d_B, ldb, nullptr, 0, dt);
    spread(4);
    if (res) CPK_HIP(hipMemcpyAsync(res, dn, 8 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
    return rc;
}

// The three gradient passes of a block: X and Lam (N x k) onto the sparsity of K's handles.  From
// kSamplePanelMinCols columns the interleaved panels and the panel kernel (adjoint.hip); k = 1 is the
// single-column adjoint's three launches, k = 0 writes alpha * 0.0
void kkt_sample_core(cpk_kkt K, int64_t k, const double *d_X, int64_t ldx, const double *d_L, int64_t ldl, double *d_gA,
                     double *d_gB, double *d_gC) {
    if (!d_gA && !d_gB && !d_gC) return;
    Ctx &c = K->ctx->c;
    const int64_t n = K->n, N = K->n + K->m;
    auto dev = [&](cpk_mat_s *H) -> const DMat & {
        const DMat &d = H->dev();
        upload_value_map(H->vm, H->dvm);
        return d;
    };
    // k < 2 has no panel path; from there the measured rule (or the forced route) decides, and either
    // path gives every entry the same bits
    const bool panel = k >= 2 && (K->sample_route == 1 || (K->sample_route == 0 && sample_panel_rule(k)));
    if (!panel) {
        auto pass = [&](cpk_mat_s *H, int64_t kk, const double *U, int64_t ldu, const double *V, int64_t ldv, double alpha,
                        double *out) {
            if (out) launch_sample_outer(c, dev(H), H->vm, H->dvm, kk, U, ldu, V, ldv, alpha, out);
        };
        pass(K->A, k, d_L, ldl, d_X, ldx, -1.0, d_gA);
        pass(K->C, k, d_L + n, ldl, d_X + n, ldx, 1.0, d_gC);
        if (!d_gB) return;
        if (k <= 1) {
            // gB's 2 k columns alternate between the two blocks (kkt_adjoint_core): for one column that
            // is a column stride from Lam to X and back
            const int64_t l2x = ((int64_t)(intptr_t)d_X - (int64_t)(intptr_t)d_L) / (int64_t)sizeof(double);
            pass(K->B, 2 * k, d_L + n, l2x, d_X, -l2x, -1.0, d_gB);
            return;
        }
        // for more columns one stride cannot express the alternation: the 2 k columns
        // U = [ly_0, xy_0, ly_1, ...] (m rows) and V = [xx_0, lx_0, xx_1, ...] (n rows) are staged by
        // four strided copies
        const int64_t m = K->m, m1 = std::max<int64_t>(m, 1), n1 = std::max<int64_t>(n, 1);
        const size_t need_d = 2 * (size_t)k * (size_t)(m1 + n1);
        if (K->panel_ops.n < need_d) K->panel_ops.alloc(need_d);
        double *U = K->panel_ops.p, *V = U + 2 * (size_t)k * (size_t)m1;
        auto stage = [&](double *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows) {
            if (rows)
                CPK_HIP(hipMemcpy2DAsync(dst, 2 * (size_t)ldd * sizeof(double), src, (size_t)lds * sizeof(double),
                                         (size_t)rows * sizeof(double), (size_t)k, hipMemcpyDeviceToDevice, c.stream));
        };
        stage(U, m1, d_L + n, ldl, m), stage(U + m1, m1, d_X + n, ldx, m);
        stage(V, n1, d_X, ldx, n), stage(V + n1, n1, d_L, ldl, n);
        pass(K->B, 2 * k, U, m1, V, n1, -1.0, d_gB);
        return;
    }
    K->sample_panels++;
    const int64_t ps = N * kMultiKP;  // one panel of an array
    const size_t per = (size_t)panel_count(k) * (size_t)ps;
    if (K->panel_ops.n < 2 * per) K->panel_ops.alloc(2 * per);
    double *PX = K->panel_ops.p, *PL = PX + per;
    launch_pack_panels(c, N, k, d_X, ldx, d_L, ldl, PX, PL);
    const double *xx = PX, *xy = PX + n * kMultiKP, *lx = PL, *ly = PL + n * kMultiKP;
    auto pass = [&](cpk_mat_s *H, const double *U1, const double *V1, const double *U2, const double *V2, double alpha,
                    double *out) {
        if (out) launch_sample_panel(c, dev(H), H->vm, H->dvm, k, ps, U1, V1, U2, V2, alpha, out);
    };
    pass(K->A, lx, xx, nullptr, nullptr, -1.0, d_gA);  // -sum_c lx_c * xx_c'
    pass(K->B, ly, xx, xy, lx, -1.0, d_gB);            // -sum_c (ly_c * xx_c' then xy_c * lx_c')
    pass(K->C, ly, xy, nullptr, nullptr, 1.0, d_gC);   // +sum_c ly_c * xy_c' (K holds -C)
}

}  // namespace cpk
