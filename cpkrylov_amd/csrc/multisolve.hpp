// multisolve.hpp -- host side of the lockstep block solve and its diagnostics: MultiCore on the shared
// driver (solve_loop.hpp) and the panel kernels (multikrylov.hpp).  Included by solvers.hip after the
// functors and policies the panels are built from.
#pragma once

namespace cpk {

// the panel product alone (cpk_debug_spmm): no solver state is read or written but `running`
struct PolDebugSpmm {
    const double *X;
    double *out;
    __device__ const double *select(DState *, const double *) { return X; }
    __device__ void fin(DState *, const double *tot) { out[0] = tot[0], out[1] = tot[1]; }
};

// ==============================================================================================
// The lockstep block solve (cpk_method_solve_multi): kc <= kMultiKP columns of cpcg / cpminres
// iterate together, one Krylov product for the panel (spmm_krylov_kernel), one panel apply of M
// (Precond::apply_multi) and one launch per element-wise pass (multikrylov.hpp) per iteration.
// Defined column by column: column j is kernels/cpcg.m / kernels/cpminres.m on b(:, j), with its
// own DState (stop test, history, error), so a column that stops freezes while the others run on.
// cpminres runs the unfused sequence (engine option no_minres_fuse): product, M*z, LanczosStep<0>,
// MinresUpdate.  The solver's vectors are N x kMultiKP column-major blocks (leading dimension N),
// the layout apply_multi takes; [x; y] is kept in the solver's own block and copied out at the
// end, so the captured graphs do not depend on the caller's pointers.
struct MultiCore : SolveDriver {
    Precond &M;
    const DMat &AC;
    int64_t n, m, N;
    int method;
    DBuf<double> hist;
    int64_t hcap = 0;
    std::vector<DBuf<double>> vecs;
    DBuf<double> parts, spart;
    DBuf<unsigned> counters;
    DBuf<int64_t> xsub;
    DBuf<int> any;
    size_t pstride = 0;

    MultiCore(Ctx &cc, Precond &MM, const DMat &ACm, int meth)
        : SolveDriver(cc, kMK), M(MM), AC(ACm), n(MM.n), m(MM.m), N(MM.N), method(meth) {
        any.alloc(1);
        pstride = (size_t)std::max<int64_t>(kEwGrid, ewt_grid(N)) * 2;
        parts.alloc(pstride * kMK);
        counters.alloc((size_t)(kMK + 1) * kTicketWords);
        CPK_HIP(hipMemset(counters.p, 0, counters.bytes()));
        if (c.exact()) {
            xsub.alloc(kMultiXStride * kMK);
            CPK_HIP(hipMemset(xsub.p, 0, xsub.bytes()));  // the launches leave them zero
        }
    }
    // block i: `cols` N-vectors per column, column j's at block(i, cols) + j * cols * N
    double *block(size_t i, size_t cols = 1) {
        while (vecs.size() <= i) vecs.emplace_back();
        const size_t want = std::max<size_t>(cols * (size_t)N * kMK, 1);
        if (vecs[i].n != want) vecs[i].alloc(want);
        return vecs[i].p;
    }
    RedBufM rbm() const { return RedBufM{parts.p, pstride, counters.p, xsub.p}; }

    // history: the panel's kc columns only, itmax + 4 entries each (the single-column solver's
    // capacity per column); none for the diagnostics, whose columns record nothing
    void reset(const cpk_opts *o, int kc, bool history = true) {
        resolve(o, (double)M.gn);
        hcap = history ? hist_capacity(itmax) : 0;
        if (hist.n < (size_t)hcap * kc) hist.alloc((size_t)hcap * kc);
        for (int j = 0; j < kMK; j++) {
            const bool records = j < kc && hcap > 0;
            init_state(hs[j], records ? hcap : 0, records ? hist.p + (size_t)j * hcap : nullptr);
            if (j >= kc) hs[j].stop = 1;  // a padding column never runs (and has no history)
        }
        CPK_HIP(hipMemcpyAsync(dst.p, hs, sizeof hs, hipMemcpyHostToDevice, c.stream));
    }

    template <class F, class Mk>
    static Panel<F> panel_of(int kc, const Mk &mk) {
        Panel<F> p{};
        for (int j = 0; j < kMK; j++) p.f[j] = mk(j < kc ? j : 0);  // the padding entries are never launched
        return p;
    }
    template <class F>
    void ew(int kc, const Panel<F> &p) {
        hipLaunchKernelGGL(ew_multi_kernel<F>, dim3(ew_grid(N), kc), dim3(kBlock), 0, c.stream, N, p);
    }
    template <class F>
    void ewt(int kc, const Panel<F> &p) {
        hipLaunchKernelGGL(ewt_multi_kernel<F>, dim3(ewt_grid(N), kc), dim3(kBlock), 0, c.stream, N, p);
    }
    template <int NV, class F>
    void ewred(int kc, const Panel<F> &p) {
        launch_red(c, ewred_multi_kernel<NV, F, double>, ewred_multi_kernel<NV, F, XAcc>, dim3(ew_grid(N), kc), N, p, rbm());
    }
    template <int NV, class F>
    void ewtred(int kc, const Panel<F> &p) {
        launch_red(c, ewtred_multi_kernel<NV, F, double>, ewtred_multi_kernel<NV, F, XAcc>, dim3(ewt_grid(N), kc), N, p, rbm());
    }
    // the resident grid of the product (occupancy x CUs), as spmv_grid: no trailing partial wave
    // of workgroups, and a fixed grid fixes which partials a column's inner products sum
    template <class Pol, class A>
    unsigned spmm_grid() {
        static const int64_t resident = [] {
            int occ = 0, dev = 0, cus = 256;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)spmm_krylov_kernel<Pol, A>, kBlock, 0) != hipSuccess ||
                occ < 1)
                occ = 1;
            (void)hipGetDevice(&dev);
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            return (int64_t)occ * cus;
        }();
        return (unsigned)std::max<int64_t>(1, std::min<int64_t>(AC.nblk, resident));
    }
    // before any capture: the occupancy query and the product's partials
    template <class Pol>
    void spmm_prepare() {
        const unsigned g = c.exact() ? spmm_grid<Pol, XAcc>() : spmm_grid<Pol, double>();
        if (spart.n < (size_t)g * kMK * 2) spart.alloc((size_t)g * kMK * 2);
    }
    template <class Pol, class A>
    void spmm_as(int kc, const Panel<Pol> &p, double *Y, double *Ys) {
        const unsigned g = spmm_grid<Pol, A>();
        hipLaunchKernelGGL((spmm_krylov_kernel<Pol, A>), dim3(g), dim3(kBlock), 0, c.stream, AC.ptr.p, AC.col.p, AC.val.p,
                           AC.blk.p, AC.nblk, dst.p, kc, p, Y, N, Ys, n, spart.p, rbm(), any.p);
    }
    template <class Pol>
    void spmm(int kc, const Panel<Pol> &p, double *Y, double *Ys) {
        if (c.exact()) spmm_as<Pol, XAcc>(kc, p, Y, Ys);
        else spmm_as<Pol, double>(kc, p, Y, Ys);
    }
    // M * z for the panel inside the loop: nothing runs when no column does, and a column that
    // goes through the single-column apply tests its own `running`
    void mapply(int kc, const double *X, double *Y, bool gated) {
        const int *run = &dst.p->running;
        M.apply_multi(kc, X, N, Y, N, nullptr, gated ? any.p : nullptr, gated ? run : nullptr, sizeof(DState) / sizeof(int));
    }

    // replay `body` (one iteration of the panel) in batches until every live column has stopped
    void loop(int kc, const std::function<void()> &body) {
        run_batches(0, kc, M.block_graph_inst, body);
    }

    void cg(int kc, const double *B, int64_t ldb);
    void minres(int kc, const double *B, int64_t ldb);
    double panel_bytes(int kc) const;
};

// cpcg.m:126-192 for every column of the panel
void MultiCore::cg(int kc, const double *B, int64_t ldb) {
    DState *st = dst.p;
    double *GW = block(0), *PQ = block(1), *APCQ = block(2), *RU = block(3), *TT = block(4), *XA = block(5);
    const int64_t N_ = N, n_ = n;
    ew(kc, panel_of<CgInit0>(kc, [&](int j) { return CgInit0{B + j * ldb, GW + j * N_, XA + j * N_, n_}; }));
    mapply(kc, GW, RU, false);
    ewred<1>(kc, panel_of<CgInit1>(kc, [&](int j) { return CgInit1{st + j, RU + j * N_, GW + j * N_, PQ + j * N_, n_}; }));
    CPK_HIP(hipGetLastError());
    const auto pol = panel_of<PolCgSpmv>(kc, [&](int j) { return PolCgSpmv{PQ + j * N_}; });
    const auto step = panel_of<CgStep>(kc, [&](int j) { return CgStep{st + j, XA + j * N_, GW + j * N_, PQ + j * N_, APCQ + j * N_, 0.0}; });
    const auto resid = panel_of<CgResid>(kc, [&](int j) { return CgResid{st + j, XA + j * N_, RU + j * N_, GW + j * N_, TT + j * N_, n_}; });
    const auto dir = panel_of<CgDir>(kc, [&](int j) { return CgDir{st + j, RU + j * N_, TT + j * N_, PQ + j * N_, n_, 0.0}; });
    spmm_prepare<PolCgSpmv>();
    auto body = [&]() {
        spmm(kc, pol, APCQ, nullptr);
        ew(kc, step);
        mapply(kc, GW, RU, true);
        ewred<2>(kc, resid);
        ew(kc, dir);
    };
    loop(kc, body);
}

// cpminres.m:141-252 for every column of the panel
void MultiCore::minres(int kc, const double *B, int64_t ldb) {
    DState *st = dst.p;
    double *VQ = block(0, 3), *W = block(1, 3);  // per column: the three Lanczos slots, the three w slots
    double *UT = block(2), *UTS = block(3), *VPREC = block(4), *XY = block(5);
    const int64_t N_ = N, n_ = n;
    for (int j = 0; j < kc; j++) launch_set_concat(c, UT + j * N_, B + j * ldb, n, m);  // [u; t] = [b; 0]
    mapply(kc, UT, VPREC, false);
    ewred<1>(kc, panel_of<InitLanczos<0>>(kc, [&](int j) {
                 double *v = VQ + j * 3 * N_, *w = W + j * 3 * N_;
                 return InitLanczos<0>{st + j, VPREC + j * N_, B + j * ldb, v + N_, v, w + 2 * N_, XY + j * N_, n_};
             }));
    ew(kc, panel_of<NormalizeCopy>(kc, [&](int j) { return NormalizeCopy{st + j, VQ + j * 3 * N_ + N_, W + j * 3 * N_, 0, 0.0}; }));
    CPK_HIP(hipGetLastError());
    const auto pol = panel_of<PolLanczosSpmv<0>>(kc, [&](int j) { return PolLanczosSpmv<0>{VQ + j * 3 * N_, N_, 0}; });
    const auto ls = panel_of<LanczosStep<0>>(kc, [&](int j) {
        return LanczosStep<0>{st + j, VQ + j * 3 * N_, VPREC + j * N_, UT + j * N_, XY + j * N_, W + j * 3 * N_, n_, N_, 0, 2, 1};
    });
    const auto upd = panel_of<MinresUpdate>(kc, [&](int j) { return MinresUpdate{st + j, VQ + j * 3 * N_, W + j * 3 * N_, XY + j * N_, n_, N_}; });
    spmm_prepare<PolLanczosSpmv<0>>();
    auto body = [&]() {
        spmm(kc, pol, UT, UTS);      // u = A*vk; t = C*qk; alpha; and [u; -t]
        mapply(kc, UTS, VPREC, true);  // vprec = M * [u; -t]
        ewtred<2>(kc, ls);
        ewt(kc, upd);
    };
    loop(kc, body);
}

// Algorithmic HBM bytes of one iteration of a panel of kc columns (DESIGN.md "Lockstep block
// solve"): blkdiag(A, C) once, the panel apply once, the vector passes per column
double MultiCore::panel_bytes(int kc) const {
    const double Nn = (double)N, l = (double)M.dF.nnz, KP = kMK;
    const double spmm = 12.0 * AC.nnz + 4.0 * (Nn + 1) + kc * 16.0 * Nn + (method == CPK_MINRES ? kc * 8.0 * Nn : 0.0);
    double mapply;
    if (kc < kApplyMultiMinCols && !M.multi_panel) {
        mapply = kc * M.apply_bytes();
    } else {
        const double steps = M.nitref > 0 ? M.nitref : 0;
        const double sweep = 12.0 * l + 4.0 * (Nn + 1) + 4.0 * Nn + KP * 16.0 * Nn;  // L once, the panel in and out
        const double resid = 12.0 * (double)M.dKp.nnz + 4.0 * (Nn + 1) + kc * 8.0 * Nn + KP * 16.0 * Nn;
        mapply = 2 * (1 + steps) * sweep + steps * resid + (KP + kc) * 8.0 * Nn;
    }
    const double vec = kc * 8.0 * Nn * (method == CPK_MINRES ? 5 + 8 : 6 + 5 + 4);
    return spmm + mapply + vec;
}

static std::string block_key(const Ctx &c, const Precond &M, const DMat &AC, int method) {
    char buf[512];
    snprintf(buf, sizeof buf, "%d|%llu|%p|%p|%p|%.17g|%.17g|%.17g|%d|%d|%llx", method, (unsigned long long)AC.gen,
             (const void *)c.partials.p, (const void *)c.counter.p, (const void *)c.xsub.p, M.nitref, M.force_itref,
             M.itref_tol, (M.residual_update != 0 && M.handle) ? 1 : 0, M.multi_panel ? 1 : 0,
             (unsigned long long)engine_opts_hash(c.opts));
    return buf;
}

void require_block_solve(const Ctx &c, const Precond &M, int method) {
    if (M.dist || c.dist()) throw Error(CPK_ERR_UNSUPPORTED, "block solve: single-GPU only");
    if (method < 0) return;
    if (M.residual_update != 0 && M.handle)
        throw Error(CPK_ERR_UNSUPPORTED, "block solve: the handle semantics of residual_update keep one state vector");
    if (method != CPK_CG && method != CPK_MINRES)
        throw Error(CPK_ERR_UNSUPPORTED, "block solve: cpcg and cpminres only (the other methods take one right-hand side)");
}

int method_solve_multi_device(Ctx &c, int method, int64_t k, const double *d_B, int64_t ldb, const DMat &AC, Precond &M,
                              const cpk_opts *opts, double *d_XY, int64_t ldxy, cpk_stats *stats, int *col_status,
                              std::string *errmsg) {
    if (k <= 0) return CPK_OK;
    // the reduction workspace of the single-column applies a short panel loops over, sized before
    // any capture (it keys the captured graphs)
    c.ensure_partials(std::max<size_t>((size_t)std::max<int64_t>(AC.nblk, M.dKp.nblk) * 2, (size_t)kEwGrid * 2));
    const std::string key = block_key(c, M, AC, method);
    // one per block method (cpcg, cpminres), so an outer loop that runs both on new values keeps
    // replaying both sets of graphs; a third key (other properties or options) drops the oldest
    auto slot = M.block_solvers.begin();
    while (slot != M.block_solvers.end() && slot->first != key) ++slot;
    if (slot == M.block_solvers.end()) {
        if (M.block_solvers.size() >= 2) M.block_solvers.erase(M.block_solvers.begin());
        M.block_solvers.emplace_back(key, std::shared_ptr<void>(new MultiCore(c, M, AC, method)));
        slot = M.block_solvers.end() - 1;
    }
    MultiCore &s = *static_cast<MultiCore *>(slot->second.get());
    int rc = CPK_OK;
    for (int64_t j0 = 0; j0 < k; j0 += kMK) {
        const int kc = (int)std::min<int64_t>(kMK, k - j0);
        CPK_HIP(hipEventRecord(c.ev0, c.stream));
        s.reset(opts, kc);
        if (method == CPK_CG) s.cg(kc, d_B + j0 * ldb, ldb);
        else s.minres(kc, d_B + j0 * ldb, ldb);
        if (s.N > 0)
            CPK_HIP(hipMemcpy2DAsync(d_XY + j0 * ldxy, (size_t)ldxy * sizeof(double), s.block(5), (size_t)s.N * sizeof(double),
                                     (size_t)s.N * sizeof(double), (size_t)kc, hipMemcpyDeviceToDevice, c.stream));
        CPK_HIP(hipEventRecord(c.ev1, c.stream));
        CPK_HIP(hipEventSynchronize(c.ev1));
        check_chain(M.dF);
        float ms = 0;
        CPK_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        int64_t iters = 0;
        for (int j = 0; j < kc; j++) iters = std::max(iters, s.hs[j].k);
        const double bytes = (double)iters * s.panel_bytes(kc) / kc;
        for (int j = 0; j < kc; j++) {
            const DState &h = s.hs[j];
            int code = CPK_OK;
            if (h.err) {
                code = CPK_ERR_INDEFINITE;
                if (rc == CPK_OK) {
                    rc = code;
                    if (errmsg) *errmsg = "column " + std::to_string(j0 + j) + ": " + indefinite_message(method, h);
                }
            }
            if (col_status) col_status[j0 + j] = code;
            if (!stats) continue;
            cpk_stats &o = stats[j0 + j];
            o.solved = !h.err && h.residNorm <= h.stopTol;
            o.lq_len = o.qr_len = 0;
            o.loop_ms = ms;
            o.bytes_moved = bytes;
            fill_stats(o, h);
        }
    }
    return rc;
}

// reg_cpkrylov.m:152-175 for every column of an N x k block with an existing M: the shift is
// decided per column by any(b(n+1:N, j)); xy0 = M*[0; b2] of the shifted columns goes through
// one block apply; b1 and the recovery are formed per column with the single-column kernels.
// An unshifted column gets xy0 = 0: its solution is the method's, as in reg_solve_device.
int reg_solve_multi_device(Ctx &c, int method, int64_t k, const double *d_B, int64_t ldb, const DMat &AC,
                           const DMat &Arows, const DMat &Btrows, int64_t bt_colmin, Precond &M, const cpk_opts *opts,
                           double *d_X, int64_t ldx, cpk_stats *stats, int *col_status, std::string *errmsg) {
    if (k <= 0) return CPK_OK;
    const int64_t n = M.n, m = M.m, N = M.N;
    auto t0 = std::chrono::steady_clock::now();
    const size_t N1 = (size_t)std::max<int64_t>(N, 1), n1 = (size_t)std::max<int64_t>(n, 1);
    std::vector<int> shift((size_t)k, 0);
    if (m > 0) {  // any(b(n+1:n+m, j)) per column
        DBuf<int> flag;
        flag.alloc((size_t)k);
        c.ensure_partials((size_t)kEwGrid);
        CPK_HIP(hipMemsetAsync(flag.p, 0, flag.bytes(), c.stream));
        for (int64_t j = 0; j < k; j++) launch_ewred<1>(c, m, AnyNonzero{d_B + j * ldb, n, flag.p + j});
        CPK_HIP(hipMemcpyAsync(shift.data(), flag.p, flag.bytes(), hipMemcpyDeviceToHost, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
    }
    std::vector<int64_t> sc;  // the shifted columns
    for (int64_t j = 0; j < k; j++)
        if (shift[(size_t)j]) sc.push_back(j);
    const size_t ks = sc.size();
    DBuf<double> in, xy0, t1, t2, b1, dxy;
    b1.alloc(n1 * (size_t)k), dxy.alloc(N1 * (size_t)k);
    if (ks) {
        in.alloc(N1 * ks), xy0.alloc(N1 * ks), t1.alloc(N1), t2.alloc(N1);
        // xy0 = M * [zeros(n,1); b(n+1:n+m)]   (reg_cpkrylov.m:156), the shifted columns as one block
        for (size_t q = 0; q < ks; q++) {
            if (n) CPK_HIP(hipMemsetAsync(in.p + q * N1, 0, n * sizeof(double), c.stream));
            CPK_HIP(hipMemcpyAsync(in.p + q * N1 + n, d_B + sc[q] * ldb + n, m * sizeof(double), hipMemcpyDeviceToDevice,
                                   c.stream));
        }
        M.apply_multi((int64_t)ks, in.p, (int64_t)N1, xy0.p, (int64_t)N1, nullptr);
        for (size_t q = 0; q < ks; q++) {  // b1 = b(1:n) - A*xy0(1:n) - B'*xy0(n+1:N)   (reg_cpkrylov.m:157)
            launch_spmv(c, Arows, xy0.p + q * N1, t1.p, nullptr);
            launch_spmv_colmask(c, Btrows, bt_colmin, xy0.p + q * N1, t2.p, nullptr);
            launch_ew(c, n, ShiftRhs{d_B + sc[q] * ldb, t1.p, t2.p, b1.p + (size_t)sc[q] * n1});
        }
    }
    for (int64_t j = 0; j < k; j++)
        if (!shift[(size_t)j] && n)
            CPK_HIP(hipMemcpyAsync(b1.p + (size_t)j * n1, d_B + j * ldb, n * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    const int rc = method_solve_multi_device(c, method, k, b1.p, (int64_t)n1, AC, M, opts, dxy.p, (int64_t)N1, stats,
                                             col_status, errmsg);
    size_t q = 0;
    for (int64_t j = 0; j < k; j++) {
        if (shift[(size_t)j]) {  // x = [xy0(1:n) + dx; xy0(n+1:N) + dy]
            launch_ew(c, N, Recover{xy0.p + q * N1, dxy.p + (size_t)j * N1, d_X + j * ldx});
            q++;
        } else if (N) {
            CPK_HIP(hipMemcpyAsync(d_X + j * ldx, dxy.p + (size_t)j * N1, N * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
        }
    }
    CPK_HIP(hipStreamSynchronize(c.stream));
    const double st = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats)
        for (int64_t j = 0; j < k; j++) stats[j].stime = st, stats[j].ptime = M.ptime;
    return rc;
}

// Diagnostic (cpk_debug_spmm): the panel product alone, Y(:, j) = blkdiag(A, C) * X(:, j) and the
// two inner products <y_j(1:n), x_j(1:n)>, <y_j(n+1:N), x_j(n+1:N)> at dots[2 j], dots[2 j + 1]
void debug_spmm(Ctx &c, const DMat &AC, Precond &M, int64_t k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy,
                double *d_dots) {
    require_block_solve(c, M, -1);
    if (k <= 0) return;
    MultiCore s(c, M, AC, CPK_CG);
    const int64_t N = s.N;
    const size_t rowb = (size_t)N * sizeof(double);
    double *Xb = s.block(0), *Yb = s.block(1);
    DBuf<double> dots;
    dots.alloc(2 * kMK);
    s.spmm_prepare<PolDebugSpmm>();
    for (int64_t j0 = 0; j0 < k; j0 += kMK) {
        const int kc = (int)std::min<int64_t>(kMK, k - j0);
        s.reset(nullptr, kc, false);
        if (N) CPK_HIP(hipMemcpy2DAsync(Xb, rowb, d_X + j0 * ldx, (size_t)ldx * sizeof(double), rowb, (size_t)kc,
                                        hipMemcpyDeviceToDevice, c.stream));
        s.spmm(kc, MultiCore::panel_of<PolDebugSpmm>(kc, [&](int j) { return PolDebugSpmm{Xb + j * N, dots.p + 2 * j}; }), Yb,
               nullptr);
        CPK_HIP(hipGetLastError());
        if (N) CPK_HIP(hipMemcpy2DAsync(d_Y + j0 * ldy, (size_t)ldy * sizeof(double), Yb, rowb, rowb, (size_t)kc,
                                        hipMemcpyDeviceToDevice, c.stream));
        CPK_HIP(hipMemcpyAsync(d_dots + 2 * j0, dots.p, (size_t)kc * 2 * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
    }
}

// Diagnostic (cpk_debug_spmm_time): device time per launch (HIP events, `reps` back-to-back
// launches after a warm-up) of the panel product with kc <= kMultiKP columns and, in the same run,
// of the single-column Krylov product spmv_stream<EpiKrylov<PolPlainSpmv>> on one column
void debug_spmm_time(Ctx &c, const DMat &AC, Precond &M, int kc, int reps, double *ms_panel, double *ms_single) {
    require_block_solve(c, M, -1);
    if (kc < 1 || kc > kMK) throw Error(CPK_ERR_DIM, "debug_spmm_time: 1 <= kc <= 8");
    reps = std::max(reps, 1);
    MultiCore s(c, M, AC, CPK_CG);
    const int64_t N = s.N;
    double *Xb = s.block(0), *Yb = s.block(1);
    DBuf<double> dots;
    dots.alloc(2 * kMK);
    std::vector<double> h((size_t)std::max<int64_t>(N, 1) * kMK);
    for (size_t i = 0; i < h.size(); i++) h[i] = 1.0 + 1e-3 * (double)(i % 1000);
    CPK_HIP(hipMemcpy(Xb, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    s.reset(nullptr, kc, false);
    s.spmm_prepare<PolDebugSpmm>();
    c.ensure_partials(std::max<size_t>((size_t)AC.nblk * 2, 4096));
    const auto pol = MultiCore::panel_of<PolDebugSpmm>(kc, [&](int j) { return PolDebugSpmm{Xb + j * N, dots.p + 2 * j}; });
    *ms_panel = time_launches(c, reps, [&]() { s.spmm(kc, pol, Yb, nullptr); });
    *ms_single = time_launches(c, reps, [&]() { launch_krylov_spmv(c, AC, s.dst.p, Yb, s.n, PolPlainSpmv{Xb}); });
    CPK_HIP(hipGetLastError());
}

}  // namespace cpk
