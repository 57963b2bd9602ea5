// capi.cpp -- the extern "C" boundary of libcpk (include/cpk.h).  Every entry point checks, stages host
// arrays and converts C++ exceptions into a cpk_status code plus a thread-local message.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <string>

#include "handles.hpp"
#include "kkt_driver.hpp"
#include "staging.hpp"

struct cpk_analysis_s {
    Analysis an;
    EngineOpts opts;  // the options it was built with (cpk_analysis_plan's split_tol)
    // cpk_analysis_rowspan's last export (a caller asks twice: the sizes, then the arrays)
    RsExport rs_last;
    int64_t rs_key[3] = {-1, -1, -1};
};

struct cpk_plan_s {
    TreeSplit ts;
    DofMap dm;
    RankPlan rp;
    DistCsr kp, ac, ab;
    int64_t n = 0, m = 0;
};

static thread_local std::string g_err;
static std::atomic<uint64_t> g_gen{1};

#define API_BEGIN try {
#define API_END                                                  \
    }                                                            \
    catch (const Error &e) {                                     \
        g_err = e.what();                                        \
        return e.code;                                           \
    }                                                            \
    catch (const std::bad_alloc &) {                             \
        g_err = "out of host memory";                            \
        return CPK_ERR_NOMEM;                                    \
    }                                                            \
    catch (const std::exception &e) {                            \
        g_err = e.what();                                        \
        return CPK_ERR_ARGS;                                     \
    }                                                            \
    return CPK_OK;

// ---- distributed host vectors: global on every rank <-> local slices on the device ----------
static void scatter_global(const Precond &p, const double *h_glob, int64_t len_local, DBuf<double> &d) {
    const std::vector<int32_t> dofs = p.dofmap->dofs(p.ctx->rank);
    std::vector<double> loc((size_t)len_local);
    for (int64_t i = 0; i < len_local; i++) loc[i] = h_glob[dofs[i]];
    d.alloc((size_t)std::max<int64_t>(len_local, 1));
    if (len_local) CPK_HIP(hipMemcpy(d.p, loc.data(), len_local * sizeof(double), hipMemcpyHostToDevice));
}

static void gather_global(Ctx &c, const Precond &p, const double *d_loc, double *h_glob) {
    const DofMap &dm = *p.dofmap;
    int64_t mx = 1;
    for (int r = 0; r < dm.P; r++) mx = std::max<int64_t>(mx, dm.n_loc[r] + dm.m_loc[r]);
    DBuf<double> snd, rcv;
    snd.alloc((size_t)mx), rcv.alloc((size_t)(mx * dm.P));
    CPK_HIP(hipMemsetAsync(snd.p, 0, snd.bytes(), c.stream));
    if (p.N) CPK_HIP(hipMemcpyAsync(snd.p, d_loc, p.N * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    c.comm->allgather(snd.p, rcv.p, (size_t)mx, c.stream);
    std::vector<double> h((size_t)(mx * dm.P));
    CPK_HIP(hipMemcpyAsync(h.data(), rcv.p, rcv.bytes(), hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
    for (int64_t g = 0; g < dm.N; g++) h_glob[g] = h[(size_t)dm.owner[g] * mx + dm.lidx[g]];
}

// a host vector of the preconditioner's layout: the rank's slice (or the whole) up, all of it down
static void stage_up(const Precond &p, const double *h, int64_t len, DBuf<double> &d) {
    if (p.dist) scatter_global(p, h, len, d);
    else h2d(d, h, (size_t)len);
}
static void stage_down(Ctx &c, const Precond &p, const double *d, double *h) {
    if (p.dist) {
        gather_global(c, p, d, h);
    } else {
        CPK_HIP(hipMemcpyAsync(h, d, p.N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
    }
}

extern "C" {

const char *cpk_last_error(void) { return g_err.c_str(); }
int cpk_abi_version(void) { return CPK_ABI_VERSION; }

int cpk_get_unique_id(unsigned char id[128]) {
    API_BEGIN
    need(id != nullptr, "id is NULL");
    rccl_unique_id(id);
    API_END
}

static std::unique_ptr<cpk_ctx_s> ctx_base(int device, int rank, int nranks) {
    need(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank/nranks");
    auto ctx = std::make_unique<cpk_ctx_s>();
    Ctx &c = ctx->c;
    if (device >= 0) CPK_HIP(hipSetDevice(device));
    CPK_HIP(hipGetDevice(&c.device));
    c.rank = rank, c.nranks = nranks;
    c.opts = engine_opts_from_env();
    CPK_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    CPK_HIP(hipEventCreate(&c.ev0));
    CPK_HIP(hipEventCreate(&c.ev1));
    c.ensure_partials(4096);
    c.red.alloc(4096);  // distributed reductions (up to 2047 Arnoldi window pairs)
    return ctx;
}

int cpk_ctx_create(int device, int rank, int nranks, const unsigned char *unique_id, cpk_ctx *out) {
    API_BEGIN
    need(out != nullptr, "out is NULL");
    need(nranks == 1 || unique_id != nullptr, "unique_id required when nranks > 1");
    auto ctx = ctx_base(device, rank, nranks);
    if (unique_id) {  // a 1-rank communicator: the single-GPU path unless engine option dist1
        ctx->comm.reset(make_rccl_comm(nranks, rank, unique_id));
        ctx->c.comm = ctx->comm.get();
    }
    *out = ctx.release();
    API_END
}

int cpk_ctx_create_null(int device, int rank, int nranks, cpk_ctx *out) {
    API_BEGIN
    need(out != nullptr, "out is NULL");
    need(nranks > 1, "the timing stand-in needs nranks > 1");
    auto ctx = ctx_base(device, rank, nranks);
    ctx->comm.reset(make_null_comm(rank, nranks));  // diagnostic (comm.cpp): collectives are no-ops
    ctx->c.comm = ctx->comm.get();
    *out = ctx.release();
    API_END
}

int cpk_ctx_get_info(cpk_ctx ctx, int64_t *info) {
    API_BEGIN
    need(ctx && info, "NULL argument");
    const Ctx &c = ctx->c;
    const int64_t v[8] = {c.device, c.rank, c.nranks, c.comm ? c.comm->kind() : CPK_COMM_NONE,
                          c.comm ? c.comm->count() : 0, c.dist() ? 1 : 0, 0, 0};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_ctx_get_options(cpk_ctx ctx, char *buf, size_t cap) {
    API_BEGIN
    need(ctx && buf && cap > 0, "NULL argument");
    const std::string v = engine_opts_string(ctx->c.opts, ctx->c.dist() && ctx->c.nranks > 1);
    need(v.size() < cap, "buffer too small");
    std::memcpy(buf, v.c_str(), v.size() + 1);
    API_END
}

int cpk_simgroup_create(int nranks, cpk_simgroup *out) {
    API_BEGIN
    need(out && nranks >= 1, "bad argument");
    auto g = std::make_unique<cpk_simgroup_s>();
    g->g = simgroup_create(nranks);
    *out = g.release();
    API_END
}

int cpk_simgroup_destroy(cpk_simgroup g) {
    API_BEGIN
    delete g;
    API_END
}

int cpk_ctx_create_sim(int device, cpk_simgroup group, int rank, int nranks, cpk_ctx *out) {
    API_BEGIN
    need(out && group, "NULL argument");
    auto ctx = ctx_base(device, rank, nranks);
    ctx->comm.reset(make_sim_comm(group->g, rank));
    ctx->c.comm = ctx->comm.get();
    *out = ctx.release();
    API_END
}

int cpk_ctx_destroy(cpk_ctx ctx) {
    API_BEGIN
    if (!ctx) return CPK_OK;
    Ctx &c = ctx->c;
    (void)hipStreamSynchronize(c.stream);
    c.comm = nullptr;
    ctx->comm.reset();
    c.partials.release();
    c.counter.release();
    c.red.release();
    (void)hipEventDestroy(c.ev0);
    (void)hipEventDestroy(c.ev1);
    (void)hipStreamDestroy(c.stream);
    delete ctx;
    API_END
}

int cpk_ctx_set_option(cpk_ctx ctx, const char *name, const char *value) {
    API_BEGIN
    need(ctx && name && value, "NULL argument");
    set_engine_option(ctx->c.opts, name, value);
    API_END
}

int cpk_ctx_get_option(cpk_ctx ctx, const char *name, char *buf, size_t cap) {
    API_BEGIN
    need(ctx && name && buf && cap > 0, "NULL argument");
    const std::string v = get_engine_option(ctx->c.opts, name, ctx->c.dist() && ctx->c.nranks > 1);
    need(v.size() < cap, "buffer too small");
    std::memcpy(buf, v.c_str(), v.size() + 1);
    API_END
}

int cpk_ctx_synchronize(cpk_ctx ctx) {
    API_BEGIN
    need(ctx, "ctx is NULL");
    CPK_HIP(hipStreamSynchronize(ctx->c.stream));
    API_END
}

int cpk_mat_create_csc(cpk_ctx ctx, int64_t nrows, int64_t ncols, const size_t *jc, const size_t *ir,
                       const double *pr, cpk_mat *out) {
    API_BEGIN
    need(out != nullptr, "NULL argument");
    auto m = std::make_unique<cpk_mat_s>();
    m->ctx = ctx;
    m->gen = g_gen++;
    m->h = csr_from_csc(nrows, ncols, jc, ir, pr, &m->vm);
    *out = m.release();
    API_END
}

int cpk_mat_create_csr(cpk_ctx ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr, const int32_t *colind,
                       const double *val, cpk_mat *out) {
    API_BEGIN
    need(out != nullptr, "NULL argument");
    auto m = std::make_unique<cpk_mat_s>();
    m->ctx = ctx;
    m->gen = g_gen++;
    m->h = csr_from_csr(nrows, ncols, rowptr, colind, val, &m->vm);
    *out = m.release();
    API_END
}

int cpk_mat_destroy(cpk_mat A) {
    API_BEGIN
    delete A;
    API_END
}

// the checks of both value updates; nothing is touched before they pass
static void check_set_values(cpk_mat A, const double *val, int64_t count, bool device) {
    need(A != nullptr, "NULL matrix handle");
    need(val != nullptr || count <= 0, "NULL value array");
    if (count != A->vm.count) throw Error(CPK_ERR_DIM, "set_values: count differs from the creating call's entry count");
    if (device && !A->ctx) throw Error(CPK_ERR_ARGS, "host-only matrix (created with ctx == NULL) used on the device");
    if (A->ctx && A->ctx->c.dist())
        throw Error(CPK_ERR_UNSUPPORTED, "set_values: single-GPU only (a distributed preconditioner caches row slices by generation)");
}

int cpk_mat_set_values(cpk_mat A, const double *val, int64_t count) {
    API_BEGIN
    check_set_values(A, val, count, false);
    const int64_t nnz = A->h.nnz();
    if (A->d && nnz) {
        // the device copy follows on the context stream, behind whatever still reads it; staged,
        // so that a failed copy leaves both copies as they were
        Ctx &c = A->ctx->c;
        std::vector<double> v;
        const double *src = val;  // the identity map: the caller's array is the stored order
        if (!A->vm.identity) {
            v.resize((size_t)nnz);
            apply_value_map(A->vm, nnz, val, v.data());
            src = v.data();
        }
        CPK_HIP(hipMemcpyAsync(A->d->val.p, src, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
        if (A->vm.identity) std::memcpy(A->h.val.data(), val, (size_t)nnz * sizeof(double));
        else A->h.val.swap(v);
    } else {
        apply_value_map(A->vm, nnz, val, A->h.val.data());
    }
    A->h_stale = false;
    A->vgen++;
    API_END
}

int cpk_mat_set_values_device(cpk_mat A, const double *d_val, int64_t count) {
    API_BEGIN
    check_set_values(A, d_val, count, true);
    Ctx &c = A->ctx->c;
    const DMat &d = A->dev();
    upload_value_map(A->vm, A->dvm);
    launch_set_values(c, A->vm, A->dvm, d.nnz, d_val, d.val.p);
    CPK_HIP(hipStreamSynchronize(c.stream));  // d_val is the caller's again
    A->h_stale = d.nnz > 0;
    A->vgen++;
    API_END
}

// the checks of both sampled outer products, in set_values_device's order; nothing is touched
// before they pass
static void check_sample_outer(cpk_mat A, int64_t k, const double *U, int64_t ldu, const double *V, int64_t ldv,
                               const double *out, int64_t count) {
    need(A != nullptr, "NULL matrix handle");
    need(out != nullptr || count <= 0, "NULL output array");
    need(k <= 0 || ((U != nullptr || A->h.nrows == 0) && (V != nullptr || A->h.ncols == 0)), "NULL operand");
    if (count != A->vm.count) throw Error(CPK_ERR_DIM, "sample_outer: count differs from the creating call's entry count");
    if (k < 0 || (k > 0 && (ldu < A->h.nrows || ldv < A->h.ncols)))
        throw Error(CPK_ERR_DIM, "sample_outer: k >= 0, ldu >= nrows and ldv >= ncols required");
    if (!A->ctx) throw Error(CPK_ERR_ARGS, "host-only matrix (created with ctx == NULL) used on the device");
    if (A->ctx->c.dist()) throw Error(CPK_ERR_UNSUPPORTED, "sample_outer: single-GPU only");
}

int cpk_mat_sample_outer_device(cpk_mat A, int64_t k, const double *d_U, int64_t ldu, const double *d_V, int64_t ldv,
                                double alpha, double *d_out, int64_t count) {
    API_BEGIN
    check_sample_outer(A, k, d_U, ldu, d_V, ldv, d_out, count);
    const DMat &d = A->dev();
    upload_value_map(A->vm, A->dvm);
    launch_sample_outer(A->ctx->c, d, A->vm, A->dvm, k, d_U, ldu, d_V, ldv, alpha, d_out);
    API_END
}

int cpk_mat_sample_outer(cpk_mat A, int64_t k, const double *U, int64_t ldu, const double *V, int64_t ldv, double alpha,
                         double *out, int64_t count) {
    API_BEGIN
    check_sample_outer(A, k, U, ldu, V, ldv, out, count);
    if (count == 0) return CPK_OK;
    Ctx &c = A->ctx->c;
    const DMat &d = A->dev();
    upload_value_map(A->vm, A->dvm);
    HostBlock dU(A->h.nrows, k), dV(A->h.ncols, k);
    if (k) dU.up(U, ldu), dV.up(V, ldv);
    DBuf<double> dg;
    dg.alloc((size_t)count);
    launch_sample_outer(c, d, A->vm, A->dvm, k, dU.d.p, dU.ld(), dV.d.p, dV.ld(), alpha, dg.p);
    CPK_HIP(hipMemcpyAsync(out, dg.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
    API_END
}

int cpk_mat_get_info(cpk_mat A, int64_t info[8]) {
    API_BEGIN
    need(A && info, "NULL argument");
    const int64_t v[8] = {A->h.nrows, A->h.ncols, A->h.nnz(), A->vm.count, (int64_t)A->vgen, A->d ? 1 : 0,
                          (int64_t)A->ac.size(), 0};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_mat_spmv(cpk_mat A, const double *x, double *y) {
    API_BEGIN
    need(A && (x || !A->h.ncols) && (y || !A->h.nrows), "NULL argument");
    Ctx &c = A->ctx->c;
    const DMat &d = A->dev();
    DBuf<double> dx, dy;
    h2d(dx, x, (size_t)A->h.ncols);
    dy.alloc((size_t)A->h.nrows);
    launch_spmv(c, d, dx.p, dy.p, nullptr);
    if (A->h.nrows) CPK_HIP(hipMemcpyAsync(y, dy.p, A->h.nrows * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
    API_END
}

int cpk_mat_spmv_device(cpk_mat A, const double *d_x, double *d_y) {
    API_BEGIN
    need(A && (d_x || !A->h.ncols) && (d_y || !A->h.nrows), "NULL argument");
    const DMat &d = A->dev();  // refuses a host-only matrix
    launch_spmv(A->ctx->c, d, d_x, d_y, nullptr);
    API_END
}

int cpk_pc_create(cpk_ctx ctx, cpk_mat A11, cpk_mat B, cpk_mat C22, double *ptime, cpk_pc *out) {
    API_BEGIN
    need(ctx && A11 && B && C22 && out, "opLDL2: Invalid number of arguments.");
    auto pc = std::make_unique<cpk_pc_s>();
    pc->ctx = ctx;
    if (ctx->c.dist()) pc->p.reset(precond_create_dist(ctx->c, A11->host(), B->host(), C22->host(), nullptr));
    else pc->p.reset(precond_create(ctx->c, A11->host(), B->host(), C22->host()));
    if (ptime) *ptime = pc->p->ptime;
    *out = pc.release();
    API_END
}

int cpk_pc_create_hint(cpk_ctx ctx, cpk_mat A11, cpk_mat B, cpk_mat C22, cpk_mat Akry, double *ptime,
                       cpk_pc *out) {
    API_BEGIN
    need(ctx && A11 && B && C22 && out, "opLDL2: Invalid number of arguments.");
    auto pc = std::make_unique<cpk_pc_s>();
    pc->ctx = ctx;
    if (ctx->c.dist())
        pc->p.reset(precond_create_dist(ctx->c, A11->host(), B->host(), C22->host(), Akry ? &Akry->host() : nullptr));
    else pc->p.reset(precond_create(ctx->c, A11->host(), B->host(), C22->host()));
    if (ptime) *ptime = pc->p->ptime;
    *out = pc.release();
    API_END
}

int cpk_pc_refactor(cpk_pc M, cpk_mat A11, cpk_mat B, cpk_mat C22, double *ptime) {
    API_BEGIN
    need(M && A11 && B && C22, "opLDL2: Invalid number of arguments.");
    Precond &p = *M->p;
    if (A11->h.nrows != p.gn || C22->h.nrows != p.gm || B->h.nrows != p.gm || B->h.ncols != p.gn)
        throw Error(CPK_ERR_DIM, "Incompatible dimensions.");
    if (!p.dl.ready)
        throw Error(CPK_ERR_UNSUPPORTED, "refactorization needs the device factorization (engine option host_factor off)");
    if (pattern_hash_combine(A11->pattern_hash(), B->pattern_hash(), C22->pattern_hash()) != p.pattern_hash)
        throw Error(CPK_ERR_ARGS, "refactor: the sparsity of A11, B or C22 differs from the factored one");
    const double s = precond_refactor(p, A11->dev(), B->dev(), C22->dev());
    if (ptime) *ptime = s;
    API_END
}

int cpk_pc_destroy(cpk_pc M) {
    API_BEGIN
    delete M;
    API_END
}

static double matlab_round(double v) { return v < 0 ? -std::floor(-v + 0.5) : std::floor(v + 0.5); }

// opLDL2 setters (ops/opLDL2.m:97-115)
static void apply_props(Precond &p, const cpk_opts *o) {
    if (!o) return;
    if (o->has_nitref) p.nitref = std::max(0.0, matlab_round(o->nitref));
    if (o->has_itref_tol) p.itref_tol = o->itref_tol;  // `sef.itref_tol` typo: no clamp in effect
    if (o->has_residual_update) p.residual_update = o->residual_update;
    if (o->has_force_itref) p.force_itref = (o->force_itref != 0 && o->force_itref != 1) ? 0.0 : o->force_itref;
}

int cpk_pc_set(cpk_pc M, const cpk_opts *opts) {
    API_BEGIN
    need(M && opts, "NULL argument");
    apply_props(*M->p, opts);
    API_END
}

int cpk_pc_get(cpk_pc M, double *nitref, double *itref_tol, double *force_itref, double *residual_update) {
    API_BEGIN
    need(M, "NULL argument");
    if (nitref) *nitref = M->p->nitref;
    if (itref_tol) *itref_tol = M->p->itref_tol;
    if (force_itref) *force_itref = M->p->force_itref;
    if (residual_update) *residual_update = M->p->residual_update;
    API_END
}

int cpk_pc_set_handle(cpk_pc M, int on) {
    API_BEGIN
    need(M, "NULL argument");
    M->p->set_handle(on != 0);
    API_END
}

int cpk_pc_apply(cpk_pc M, const double *x, double *y) {
    API_BEGIN
    need(M && x && y, "NULL argument");
    Precond &p = *M->p;
    Ctx &c = M->ctx->c;
    DBuf<double> dx, dy;
    stage_up(p, x, p.N, dx);
    dy.alloc((size_t)std::max<int64_t>(p.N, 1));
    p.apply(dx.p, p.N, dy.p, nullptr);
    stage_down(c, p, dy.p, y);
    check_chain(p.dF);
    check_chain(p.sep.tsw);
    API_END
}

int cpk_pc_apply_device(cpk_pc M, const double *d_x, double *d_y) {
    API_BEGIN
    need(M && d_x && d_y, "NULL argument");
    M->p->apply(d_x, M->p->N, d_y, nullptr);
    API_END
}

// ---- the bare factor composite: opLDL2's M' and conj(M) (opLDL2.m:127-136) ---------------------
// One LDL solve on the device factors: no refinement, no residual update, none of their state.
int cpk_pc_apply_ldl(cpk_pc M, const double *x, double *y) {
    API_BEGIN
    need(M && x && y, "NULL argument");
    Precond &p = *M->p;
    Ctx &c = M->ctx->c;
    DBuf<double> dx, dy;
    stage_up(p, x, p.N, dx);
    dy.alloc((size_t)std::max<int64_t>(p.N, 1));
    p.ldl_solve(dx.p, p.N, dy.p, false, nullptr, nullptr);
    stage_down(c, p, dy.p, y);
    check_chain(p.dF);
    check_chain(p.sep.tsw);
    API_END
}

int cpk_pc_apply_ldl_device(cpk_pc M, const double *d_x, double *d_y) {
    API_BEGIN
    need(M && d_x && d_y, "NULL argument");
    M->p->ldl_solve(d_x, M->p->N, d_y, false, nullptr, nullptr);
    API_END
}

static void check_multi(const Precond &p, int64_t k, int64_t ldx, int64_t ldy) {
    if (k < 0 || ldx < p.gN || ldy < p.gN)
        throw Error(CPK_ERR_DIM, "apply_ldl_multi: k >= 0 and leading dimensions >= N required");
    if (p.dist) throw Error(CPK_ERR_UNSUPPORTED, "multi-column factor apply: single-GPU only");
}

int cpk_pc_apply_ldl_multi_device(cpk_pc M, int64_t k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy) {
    API_BEGIN
    need(M && d_X && d_Y, "NULL argument");
    check_multi(*M->p, k, ldx, ldy);
    M->p->ldl_solve_multi(k, d_X, ldx, d_Y, ldy);
    API_END
}

int cpk_pc_apply_ldl_multi(cpk_pc M, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    API_BEGIN
    need(M && X && Y, "NULL argument");
    Precond &p = *M->p;
    Ctx &c = M->ctx->c;
    check_multi(p, k, ldx, ldy);
    if (k == 0 || p.N == 0) return CPK_OK;
    HostBlock dX(p.N, k), dY(p.N, k);
    dX.up(X, ldx);
    p.ldl_solve_multi(k, dX.d.p, dX.ld(), dY.d.p, dY.ld());
    CPK_HIP(hipStreamSynchronize(c.stream));
    dY.down(Y, ldy);
    API_END
}

// ---- the refined apply for a block: Y(:, j) = M * X(:, j), opLDL2.multiply per column -----------
// the checks of cpk_pc_apply_ldl_multi, and X and Y may not overlap (Y is written while X is
// still read by the refinement residuals)
static void check_apply_multi(const Precond &p, int64_t k, const double *X, int64_t ldx, const double *Y, int64_t ldy) {
    if (k < 0 || ldx < p.gN || ldy < p.gN)
        throw Error(CPK_ERR_DIM, "apply_multi: k >= 0 and leading dimensions >= N required");
    if (p.dist) throw Error(CPK_ERR_UNSUPPORTED, "multi-column apply: single-GPU only");
    if (p.residual_update != 0 && p.handle)
        throw Error(CPK_ERR_UNSUPPORTED, "multi-column apply: the handle semantics of residual_update keep one state vector");
    if (k == 0 || p.N == 0) return;
    const uintptr_t x0 = (uintptr_t)X, y0 = (uintptr_t)Y;
    const uintptr_t x1 = x0 + ((size_t)(k - 1) * (size_t)ldx + (size_t)p.N) * sizeof(double);
    const uintptr_t y1 = y0 + ((size_t)(k - 1) * (size_t)ldy + (size_t)p.N) * sizeof(double);
    if (x0 < y1 && y0 < x1) throw Error(CPK_ERR_ARGS, "apply_multi: X and Y overlap");
}

int cpk_pc_apply_multi_device(cpk_pc M, int64_t k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy,
                              int32_t *d_nit) {
    API_BEGIN
    need(M && d_X && d_Y, "NULL argument");
    check_apply_multi(*M->p, k, d_X, ldx, d_Y, ldy);
    M->p->apply_multi(k, d_X, ldx, d_Y, ldy, d_nit);
    API_END
}

int cpk_pc_apply_multi(cpk_pc M, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, int32_t *nit) {
    API_BEGIN
    need(M && X && Y, "NULL argument");
    Precond &p = *M->p;
    Ctx &c = M->ctx->c;
    check_apply_multi(p, k, X, ldx, Y, ldy);
    if (k == 0 || p.N == 0) return CPK_OK;
    HostBlock dX(p.N, k), dY(p.N, k);
    DBuf<int32_t> dn;
    if (nit) dn.alloc((size_t)k);
    dX.up(X, ldx);
    p.apply_multi(k, dX.d.p, dX.ld(), dY.d.p, dY.ld(), dn.p);
    CPK_HIP(hipStreamSynchronize(c.stream));
    check_chain(p.dF);
    dY.down(Y, ldy);
    if (nit) CPK_HIP(hipMemcpy(nit, dn.p, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost));
    API_END
}

int cpk_pc_multi_info(cpk_pc M, int64_t *info) {
    API_BEGIN
    need(M && info, "NULL argument");
    if (M->p->dist) throw Error(CPK_ERR_UNSUPPORTED, "multi-column factor apply: single-GPU only");
    const MultiPlan &mp = multisweep_plan(M->p->dF);
    const int64_t v[4] = {kMultiKP, mp.launches, mp.staged, mp.direct};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_pc_solver_info(cpk_pc M, int64_t info[4]) {
    API_BEGIN
    need(M && info, "NULL argument");
    const Precond &p = *M->p;
    const int64_t v[4] = {(int64_t)p.solvers.size(), p.graph_inst, (int64_t)p.block_solvers.size(), p.block_graph_inst};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_pc_divide(cpk_pc M, const double *b, double *x) {
    API_BEGIN
    need(M && b && x, "NULL argument");
    Precond &p = *M->p;
    Ctx &c = M->ctx->c;
    DBuf<double> db, dx;
    stage_up(p, b, p.N, db);
    dx.alloc((size_t)std::max<int64_t>(p.N, 1));
    launch_spmv(c, p.dKp, db.p, dx.p, nullptr);
    stage_down(c, p, dx.p, x);
    API_END
}

int cpk_pc_get_info(cpk_pc M, cpk_pc_info *info) {
    API_BEGIN
    need(M && info, "NULL argument");
    const Precond &p = *M->p;
    info->n = p.gn, info->m = p.gm, info->N = p.gN;
    info->nnz_kp = p.Kp.nnz();
    info->nnz_l = (int64_t)p.F.Li.size();
    info->nblocks = (int64_t)p.S.blk_row.size() - 1;
    info->nrounds = (int64_t)p.S.round_ptr.size() - 1;
    info->max_block_levels = p.S.max_levels;
    info->depth = p.S.depth;
    info->ordering = p.ordering;
    API_END
}

int cpk_pc_export(cpk_pc M, int64_t *Lcolptr, int32_t *Lrowind, double *Lval, double *D, int32_t *perm) {
    API_BEGIN
    need(M, "NULL argument");
    const Precond &p = *M->p;
    const Factor &f = p.F;
    if (Lcolptr) std::memcpy(Lcolptr, f.Lp.data(), f.Lp.size() * sizeof(int64_t));
    if (Lrowind) std::memcpy(Lrowind, f.Li.data(), f.Li.size() * sizeof(int32_t));
    if (p.dl.ready) {  // values computed on the device (ldl.hip): CSC order, pivot order
        if (Lval && !f.Li.empty()) CPK_HIP(hipMemcpy(Lval, p.dl.Lx.p, f.Li.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (D && f.N) CPK_HIP(hipMemcpy(D, p.dl.D.p, (size_t)f.N * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        if (Lval) std::memcpy(Lval, f.Lx.data(), f.Lx.size() * sizeof(double));
        if (D) std::memcpy(D, f.D.data(), f.D.size() * sizeof(double));
    }
    if (perm) std::memcpy(perm, f.perm.data(), f.perm.size() * sizeof(int32_t));
    API_END
}

static_assert(sizeof(cpk_factor_report) == sizeof(FactorReport), "cpk_factor_report mirrors FactorReport");
// E in the original dof order from the pivot-order shifts Ek (null: zeros)
static void shift_to_dofs(const Factor &f, const double *Ek, double *E) {
    for (int64_t k = 0; k < f.N; k++) E[f.perm[k]] = Ek ? Ek[k] : 0.0;
}

int cpk_pc_factor_report(cpk_pc M, cpk_factor_report *out) {
    API_BEGIN
    need(M && out, "NULL argument");
    const Precond &p = *M->p;
    const FactorReport &r = p.dl.ready ? p.dl.rep : p.F.rep;
    std::memcpy(out, &r, sizeof r);
    API_END
}

int cpk_pc_pivot_shift(cpk_pc M, double *E) {
    API_BEGIN
    need(M && E, "NULL argument");
    const Precond &p = *M->p;
    const Factor &f = p.F;
    if (p.dl.ready && p.dl.E.n && f.N) {  // shifts computed on the device (ldl.hip), pivot order
        std::vector<double> ek((size_t)f.N);
        CPK_HIP(hipMemcpy(ek.data(), p.dl.E.p, (size_t)f.N * sizeof(double), hipMemcpyDeviceToHost));
        shift_to_dofs(f, ek.data(), E);
    } else {
        shift_to_dofs(f, !p.dl.ready && !f.E.empty() ? f.E.data() : nullptr, E);
    }
    API_END
}

static void check_dist_method(const Ctx &, int) {}

int cpk_method_solve_device(cpk_ctx ctx, int method, const double *d_b, cpk_mat A, cpk_mat C, cpk_pc M,
                            const cpk_opts *opts, double *d_xy, cpk_stats *stats) {
    API_BEGIN
    need(ctx && A && M && (d_xy || !M->p->N) && (d_b || !M->p->n), "NULL argument");
    check_method_dims(A, C, M);
    check_dist_method(ctx->c, method);
    const DMat &AC = A->krylov_op(C, *M->p);
    method_solve_device(ctx->c, method, d_b, AC, *M->p, opts, d_xy, stats);
    API_END
}

int cpk_method_solve(cpk_ctx ctx, int method, const double *b, cpk_mat A, cpk_mat C, cpk_pc M, const cpk_opts *opts,
                     double *x, double *y, cpk_stats *stats) {
    API_BEGIN
    need(ctx && b && x && A && C && M && (y || !C->h.nrows), "NULL argument");
    check_method_dims(A, C, M);
    check_dist_method(ctx->c, method);
    Ctx &c = ctx->c;
    Precond &p = *M->p;
    const int64_t n = p.n, m = p.m, N = n + m;
    const DMat &AC = A->krylov_op(C, p);
    DBuf<double> db, dxy;
    stage_up(p, b, n, db);
    dxy.alloc((size_t)std::max<int64_t>(N, 1));
    auto t0 = std::chrono::steady_clock::now();
    method_solve_device(c, method, db.p, AC, p, opts, dxy.p, stats);
    std::vector<double> g((size_t)p.gN);  // [x; y], split into the caller's two arrays
    stage_down(c, p, dxy.p, g.data());
    std::memcpy(x, g.data(), p.gn * sizeof(double));
    if (p.gm) std::memcpy(y, g.data() + p.gn, p.gm * sizeof(double));
    if (stats) stats->stime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    API_END
}

int cpk_reg_solve_device(cpk_ctx ctx, int method, const double *d_b, cpk_mat A, cpk_mat B, cpk_mat C, cpk_pc M,
                         const cpk_opts *opts, double *d_x, cpk_stats *stats) {
    API_BEGIN
    need(ctx && A && M && B && ((d_b && d_x) || !M->p->N), "NULL argument");
    check_method_dims(A, C, M);
    check_dist_method(ctx->c, method);
    const DMat &AC = A->krylov_op(C, *M->p);
    const ShiftOps so = shift_ops(A, C, *M->p);
    reg_solve_device(ctx->c, method, d_b, AC, *so.A, *so.Bt, so.bt_colmin, *M->p, opts, d_x, stats);
    if (stats) stats->ptime = M->p->ptime;
    API_END
}

int cpk_reg_shift_device(cpk_ctx ctx, const double *d_b, cpk_mat A, cpk_mat B, cpk_mat C, cpk_pc M, double *d_b1,
                         double *d_xy0, int *shifted) {
    API_BEGIN
    need(ctx && A && M && B && ((d_b && d_b1 && d_xy0) || !M->p->N), "NULL argument");
    check_method_dims(A, C, M);
    const ShiftOps so = shift_ops(A, C, *M->p);
    int s = reg_shift_device(ctx->c, d_b, *so.A, *so.Bt, so.bt_colmin, *M->p, d_b1, d_xy0);
    if (shifted) *shifted = s;
    API_END
}

// ---- the operator-valued A (cpk_op) ----------------------------------------------------------
int cpk_op_create(cpk_ctx ctx, int64_t n, cpk_op_fn fn, void *user, int flags, cpk_op *out) {
    API_BEGIN
    need(ctx && out, "NULL argument");
    if (n < 0) throw Error(CPK_ERR_DIM, "op: n must be >= 0");
    need((flags & ~CPK_OP_CAPTURABLE) == 0, "op: unknown flags");
    auto a = std::make_unique<cpk_op_s>();
    a->ctx = ctx, a->n = n, a->fn = fn, a->user = user, a->flags = flags;
    a->gen = g_gen++;
    *out = a.release();
    API_END
}

int cpk_op_destroy(cpk_op A) {
    API_BEGIN
    delete A;
    API_END
}

int cpk_op_get_info(cpk_op A, int64_t info[4]) {
    API_BEGIN
    need(A && info, "NULL argument");
    info[0] = A->n, info[1] = A->flags, info[2] = A->calls, info[3] = A->fails;
    API_END
}

int cpk_op_apply_device(cpk_op A, const double *d_x, double *d_y) {
    API_BEGIN
    need(A && ((d_x && d_y) || !A->n), "NULL argument");
    need(A->fn != nullptr, "op: the callback is NULL");
    op_call(A->ctx->c, A->hook(), d_x, d_y, A->n);
    API_END
}

// what every operator solve refuses, before anything is written
static void check_op_solve(cpk_ctx ctx, cpk_op A, cpk_mat C, const cpk_pc_s *M) {
    need(ctx && A && C && M, "NULL argument");
    need(A->fn != nullptr, "op: the callback is NULL");
    need(A->ctx == ctx && M->ctx == ctx && C->ctx == ctx, "op: the operator, C and M belong to one context");
    if (ctx->c.dist() || M->p->dist)
        throw Error(CPK_ERR_UNSUPPORTED, "an operator-valued A is single-GPU (a distributed context keeps row slices of A)");
    if (C->h.nrows != C->h.ncols) throw Error(CPK_ERR_DIM, "C must be square");
    if (A->n != M->p->gn || C->h.nrows != M->p->gm) throw Error(CPK_ERR_DIM, "A, C and M dimensions disagree");
}

int cpk_method_solve_op_device(cpk_ctx ctx, int method, const double *d_b, cpk_op A, cpk_mat C, cpk_pc M,
                               const cpk_opts *opts, double *d_xy, cpk_stats *stats) {
    API_BEGIN
    check_op_solve(ctx, A, C, M);
    need((d_xy || !M->p->N) && (d_b || !M->p->n), "NULL argument");
    const OpHook h = A->hook();
    method_solve_device(ctx->c, method, d_b, A->krylov_op(C), *M->p, opts, d_xy, stats, &h);
    API_END
}

int cpk_method_solve_op(cpk_ctx ctx, int method, const double *b, cpk_op A, cpk_mat C, cpk_pc M, const cpk_opts *opts,
                        double *x, double *y, cpk_stats *stats) {
    API_BEGIN
    check_op_solve(ctx, A, C, M);
    need(b && x && (y || !C->h.nrows), "NULL argument");
    Ctx &c = ctx->c;
    Precond &p = *M->p;
    const int64_t n = p.n, m = p.m, N = n + m;
    const OpHook h = A->hook();
    const DMat &ZC = A->krylov_op(C);
    DBuf<double> db, dxy;
    h2d(db, b, (size_t)n);
    dxy.alloc((size_t)std::max<int64_t>(N, 1));
    auto t0 = std::chrono::steady_clock::now();
    method_solve_device(c, method, db.p, ZC, p, opts, dxy.p, stats, &h);
    if (n) CPK_HIP(hipMemcpy(x, dxy.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (m) CPK_HIP(hipMemcpy(y, dxy.p + n, m * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) stats->stime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    API_END
}

int cpk_reg_solve_op_device(cpk_ctx ctx, int method, const double *d_b, cpk_op A, cpk_mat B, cpk_mat C, cpk_pc M,
                            const cpk_opts *opts, double *d_x, cpk_stats *stats) {
    API_BEGIN
    check_op_solve(ctx, A, C, M);
    need(B && ((d_b && d_x) || !M->p->N), "NULL argument");
    Precond &p = *M->p;
    const OpHook h = A->hook();
    const DMat &ZC = A->krylov_op(C);
    // the shift's B'*xy0(n+1:N): rows < n of Kp, columns >= n; A's rows are the callback's
    reg_solve_device(ctx->c, method, d_b, ZC, ZC, p.dKp, p.n, p, opts, d_x, stats, &h);
    if (stats) stats->ptime = p.ptime;
    API_END
}

int cpk_reg_solve_op(cpk_ctx ctx, int method, const double *b, cpk_op A, cpk_mat B, cpk_mat C, cpk_pc M,
                     const cpk_opts *opts, double *x, cpk_stats *stats) {
    API_BEGIN
    check_op_solve(ctx, A, C, M);
    need(B && b && x, "NULL argument");
    Precond &p = *M->p;
    const int64_t N = p.N;
    const OpHook h = A->hook();
    const DMat &ZC = A->krylov_op(C);
    DBuf<double> db, dx;
    h2d(db, b, (size_t)N);
    dx.alloc((size_t)std::max<int64_t>(N, 1));
    reg_solve_device(ctx->c, method, db.p, ZC, ZC, p.dKp, p.n, p, opts, dx.p, stats, &h);
    if (N) CPK_HIP(hipMemcpy(x, dx.p, N * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) stats->ptime = p.ptime;
    API_END
}

// ---- the saddle-point operator K = [A B'; B -C]: product, true residual, verified solve ----------
// The drivers are kkt_driver.cpp's; an entry here checks (so a refusal writes nothing), stages and
// copies back.
int cpk_kkt_create(cpk_ctx ctx, cpk_mat A, cpk_mat B, cpk_mat C, cpk_kkt *out) {
    API_BEGIN
    need(ctx && A && B && C && out, "NULL argument");
    need(A->ctx == ctx && B->ctx == ctx && C->ctx == ctx, "kkt: the matrices belong to another context");
    check_kp_dims(A->h, B->h, C->h);
    if (ctx->c.dist())
        throw Error(CPK_ERR_UNSUPPORTED, "kkt: single-GPU only (a distributed context keeps row slices, not K)");
    auto k = std::make_unique<cpk_kkt_s>();
    k->ctx = ctx, k->A = A, k->B = B, k->C = C;
    k->n = A->h.nrows, k->m = C->h.nrows;
    kkt_assemble(k.get());
    *out = k.release();
    API_END
}

int cpk_kkt_destroy(cpk_kkt K) {
    API_BEGIN
    delete K;  // hipFree waits for the device; the context may already be gone
    API_END
}

int cpk_kkt_get_info(cpk_kkt K, int64_t info[8]) {
    API_BEGIN
    need(K && info, "NULL argument");
    const int64_t v[8] = {K->n, K->m, K->K.nnz, (int64_t)K->vgen[0], (int64_t)K->vgen[1], (int64_t)K->vgen[2],
                          K->refreshes, (int64_t)(uintptr_t)K->K.val.p};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_kkt_apply_device(cpk_kkt K, const double *d_z, double *d_y) {
    API_BEGIN
    need(K && ((d_z && d_y) || !(K->n + K->m)), "NULL argument");
    kkt_apply(K, d_z, d_y);
    API_END
}

int cpk_kkt_apply(cpk_kkt K, const double *z, double *y) {
    API_BEGIN
    need(K && ((z && y) || !(K->n + K->m)), "NULL argument");
    Ctx &c = K->ctx->c;
    const int64_t N = K->n + K->m;
    if (N == 0) return CPK_OK;
    DBuf<double> dz, dy;
    h2d(dz, z, (size_t)N);
    dy.alloc((size_t)N);
    kkt_apply(K, dz.p, dy.p);
    CPK_HIP(hipMemcpyAsync(y, dy.p, N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
    API_END
}

int cpk_kkt_set_route(cpk_kkt K, int route) {
    API_BEGIN
    need(K != nullptr, "NULL argument");
    need(route >= 0 && route <= 2, "kkt_set_route: 0 (by the crossover), 1 (panel) or 2 (loop)");
    K->route = route;
    API_END
}

int cpk_kkt_route_info(cpk_kkt K, int64_t info[4]) {
    API_BEGIN
    need(K && info, "NULL argument");
    const int64_t v[4] = {kMultiKP, kKktPanelMinCols, K->route, K->panels};
    std::memcpy(info, v, sizeof v);
    API_END
}

// The residual entries, plain (kkt_resid_block) and exactly rounded (kkt_resid_exact_block), in
// their three forms.  The checks of all of them; nothing is touched before they pass
using ResidBlock = decltype(&kkt_resid_block);
static void check_kkt_resid(cpk_kkt K, int64_t k, const double *Z, int64_t ldz, const double *Bm, int64_t ldb,
                            const double *R, int64_t ldr) {
    need(K && Z && Bm, "NULL argument");
    const int64_t N = K->n + K->m;
    if (k < 0 || ldz < N || ldb < N || (R && ldr < N))
        throw Error(CPK_ERR_DIM, "kkt_residual: k >= 0 and leading dimensions >= N required");
}

static void kkt_residual_device(ResidBlock block, cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm,
                                int64_t ldb, double *d_R, int64_t ldr, double *d_norms) {
    check_kkt_resid(K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr);
    if (k == 0) return;
    block(K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr, d_norms);
}

// device operands, the sums to HOST memory: they are taken in a device buffer, copied back and
// waited for, so a caller without a device allocator (the Python class) can have them
static void kkt_residual_device_sums(ResidBlock block, cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz,
                                     const double *d_Bm, int64_t ldb, double *d_R, int64_t ldr, double *norms) {
    check_kkt_resid(K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr);
    need(norms != nullptr, "NULL argument");
    if (k == 0) return;
    Ctx &c = K->ctx->c;
    DBuf<double> dn;
    dn.alloc(4 * (size_t)k);
    block(K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr, dn.p);
    CPK_HIP(hipMemcpyAsync(norms, dn.p, dn.bytes(), hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
}

static void kkt_residual_host(ResidBlock block, cpk_kkt K, int64_t k, const double *Z, int64_t ldz, const double *Bm,
                              int64_t ldb, double *R, int64_t ldr, double *norms) {
    check_kkt_resid(K, k, Z, ldz, Bm, ldb, R, ldr);
    if (k == 0) return;
    Ctx &c = K->ctx->c;
    const int64_t N = K->n + K->m;
    HostBlock dZ(N, k), dB(N, k);
    DBuf<double> dn;
    if (norms) dn.alloc(4 * (size_t)k);
    dZ.up(Z, ldz), dB.up(Bm, ldb);
    // in place on the staged right-hand sides: a row reads b_i before it writes r_i
    block(K, k, dZ.d.p, dZ.ld(), dB.d.p, dB.ld(), R ? dB.d.p : nullptr, dB.ld(), dn.p);
    CPK_HIP(hipStreamSynchronize(c.stream));
    if (R) dB.down(R, ldr);
    if (norms) CPK_HIP(hipMemcpy(norms, dn.p, 4 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost));
}

int cpk_kkt_residual_device(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm, int64_t ldb,
                            double *d_R, int64_t ldr, double *d_norms) {
    API_BEGIN
    kkt_residual_device(kkt_resid_block, K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr, d_norms);
    API_END
}
int cpk_kkt_residual_device_sums(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm, int64_t ldb,
                                 double *d_R, int64_t ldr, double *norms) {
    API_BEGIN
    kkt_residual_device_sums(kkt_resid_block, K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr, norms);
    API_END
}
int cpk_kkt_residual(cpk_kkt K, int64_t k, const double *Z, int64_t ldz, const double *Bm, int64_t ldb, double *R,
                     int64_t ldr, double *norms) {
    API_BEGIN
    kkt_residual_host(kkt_resid_block, K, k, Z, ldz, Bm, ldb, R, ldr, norms);
    API_END
}
int cpk_kkt_residual_exact_device(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm, int64_t ldb,
                                  double *d_R, int64_t ldr, double *d_norms) {
    API_BEGIN
    kkt_residual_device(kkt_resid_exact_block, K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr, d_norms);
    API_END
}
int cpk_kkt_residual_exact_device_sums(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm,
                                       int64_t ldb, double *d_R, int64_t ldr, double *norms) {
    API_BEGIN
    kkt_residual_device_sums(kkt_resid_exact_block, K, k, d_Z, ldz, d_Bm, ldb, d_R, ldr, norms);
    API_END
}
int cpk_kkt_residual_exact(cpk_kkt K, int64_t k, const double *Z, int64_t ldz, const double *Bm, int64_t ldb, double *R,
                           int64_t ldr, double *norms) {
    API_BEGIN
    kkt_residual_host(kkt_resid_exact_block, K, k, Z, ldz, Bm, ldb, R, ldr, norms);
    API_END
}

// ---- the verified solve, the refined solve and the adjoint: host forms by host_column_solve ------
int cpk_kkt_solve_device(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x, int warm,
                         cpk_stats *stats, double *res) {
    API_BEGIN
    need(K && M && ((d_b && d_x) || !(K->n + K->m)), "NULL argument");
    kkt_solve_core(K, method, d_b, M, opts, d_x, warm, stats, res);
    API_END
}

int cpk_kkt_solve(cpk_kkt K, int method, const double *b, cpk_pc M, const cpk_opts *opts, double *x, int warm,
                  cpk_stats *stats, double *res) {
    API_BEGIN
    need(K && M && ((b && x) || !(K->n + K->m)), "NULL argument");
    host_column_solve(K->ctx->c.stream, K->n + K->m, b, x, warm, nullptr, nullptr, [&](const double *d_b, double *d_x) {
        kkt_solve_core(K, method, d_b, M, opts, d_x, warm, stats, res);
    });
    API_END
}

int cpk_kkt_solve_refined_device(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x,
                                 int warm, int max_steps, cpk_stats *stats, double *res, int *steps_out) {
    API_BEGIN
    need(K && M && ((d_b && d_x) || !(K->n + K->m)), "NULL argument");
    need(max_steps >= 0, "kkt_solve_refined: max_steps >= 0 required");
    kkt_refined_core(K, method, d_b, M, opts, d_x, warm, max_steps, stats, res, steps_out);
    API_END
}

int cpk_kkt_solve_refined(cpk_kkt K, int method, const double *b, cpk_pc M, const cpk_opts *opts, double *x, int warm,
                          int max_steps, cpk_stats *stats, double *res, int *steps_out) {
    API_BEGIN
    need(K && M && ((b && x) || !(K->n + K->m)), "NULL argument");
    need(max_steps >= 0, "kkt_solve_refined: max_steps >= 0 required");
    bool wrote_x = false;  // a refusal leaves the caller's x as it is
    host_column_solve(K->ctx->c.stream, K->n + K->m, b, x, warm, &wrote_x, nullptr, [&](const double *d_b, double *d_x) {
        kkt_refined_core(K, method, d_b, M, opts, d_x, warm, max_steps, stats, res, steps_out, &wrote_x);
    });
    API_END
}

// a gradient array's count is its handle's creating call's entry count (what: the entry's refusal)
static void check_grad_counts(cpk_kkt K, const double *gA, int64_t cA, const double *gB, int64_t cB, const double *gC,
                              int64_t cC, const char *what) {
    const cpk_mat_s *h[3] = {K->A, K->B, K->C};
    const double *g[3] = {gA, gB, gC};
    const int64_t cnt[3] = {cA, cB, cC};
    for (int i = 0; i < 3; i++)
        if (g[i] && cnt[i] != h[i]->vm.count) throw Error(CPK_ERR_DIM, what);
}

static void check_kkt_adjoint(cpk_kkt K, cpk_kkt KT, cpk_pc M, const double *x, const double *gx, const double *lam,
                              const double *gA, int64_t cA, const double *gB, int64_t cB, const double *gC, int64_t cC) {
    need(K && M && ((x && gx && lam) || !(K->n + K->m)), "NULL argument");
    need(!KT || (KT->ctx == K->ctx && KT->n == K->n && KT->m == K->m), "kkt_adjoint: KT's dimensions differ from K's");
    check_grad_counts(K, gA, cA, gB, cB, gC, cC,
                      "kkt_adjoint: a gradient's count differs from its handle's creating call's entry count");
}

int cpk_kkt_adjoint_device(cpk_kkt K, cpk_kkt KT, int method, const double *d_x, const double *d_gx, cpk_pc M,
                           const cpk_opts *opts, double *d_lam, int warm, double *d_gA, int64_t cA, double *d_gB, int64_t cB,
                           double *d_gC, int64_t cC, cpk_stats *stats, double *res) {
    API_BEGIN
    check_kkt_adjoint(K, KT, M, d_x, d_gx, d_lam, d_gA, cA, d_gB, cB, d_gC, cC);
    kkt_adjoint_core(K, KT, method, d_x, d_gx, M, opts, d_lam, warm, d_gA, d_gB, d_gC, stats, res);
    CPK_HIP(hipStreamSynchronize(K->ctx->c.stream));  // the gradients are the caller's
    API_END
}

int cpk_kkt_adjoint(cpk_kkt K, cpk_kkt KT, int method, const double *x, const double *gx, cpk_pc M, const cpk_opts *opts,
                    double *lam, int warm, double *gA, int64_t cA, double *gB, int64_t cB, double *gC, int64_t cC,
                    cpk_stats *stats, double *res) {
    API_BEGIN
    check_kkt_adjoint(K, KT, M, x, gx, lam, gA, cA, gB, cB, gC, cC);
    const int64_t N = K->n + K->m;
    DBuf<double> dx;  // the second input; gx is the solve's right-hand side, lam its x
    h2d(dx, x, (size_t)N);
    HostGrads g(gA, cA, gB, cB, gC, cC);
    host_column_solve(K->ctx->c.stream, N, gx, lam, warm, nullptr, &g, [&](const double *d_gx, double *d_lam) {
        kkt_adjoint_core(K, KT, method, dx.p, d_gx, M, opts, d_lam, warm, g.dev(0), g.dev(1), g.dev(2), stats, res);
    });
    API_END
}

// ---- the lockstep block solve: column j is method(b(:, j), A, C, M, opts) -------------------------
// (kernels/cpcg.m:1, kernels/cpminres.m:1 per column).  Checks in the order of the block applies:
// NULL arguments, then k and the leading dimensions, then what the entry does not support.
static void check_solve_multi(cpk_mat A, cpk_mat C, const cpk_pc_s *M, int method, int64_t k, int64_t ld_n[2],
                              int64_t ld_m, int64_t ld_N[2]) {
    const int64_t n = A->h.nrows, m = C->h.nrows;
    if (k < 0 || ld_n[0] < n || ld_n[1] < n || ld_m < m || ld_N[0] < n + m || ld_N[1] < n + m)
        throw Error(CPK_ERR_DIM, "solve_multi: k >= 0 and leading dimensions >= the column length required");
    check_method_dims(A, C, M);
    require_block_solve(M->ctx->c, *M->p, method);
}
// the first failing column's status and message, after every column's outputs were written
static int solve_multi_result(int rc, const std::string &msg) {
    if (rc != CPK_OK) g_err = msg;
    return rc;
}

int cpk_method_solve_multi_device(cpk_ctx ctx, int method, int64_t k, const double *d_B, int64_t ldb, cpk_mat A, cpk_mat C,
                                  cpk_pc M, const cpk_opts *opts, double *d_XY, int64_t ldxy, cpk_stats *stats,
                                  int *col_status) {
    API_BEGIN
    need(ctx && A && C && M && d_B && d_XY, "NULL argument");
    int64_t ln[2] = {ldb, ldb}, lN[2] = {ldxy, ldxy};
    check_solve_multi(A, C, M, method, k, ln, C->h.nrows, lN);
    if (k == 0) return CPK_OK;
    std::string msg;
    const int rc = method_solve_multi_device(ctx->c, method, k, d_B, ldb, A->krylov_op(C, *M->p), *M->p, opts, d_XY, ldxy,
                                             stats, col_status, &msg);
    return solve_multi_result(rc, msg);
    API_END
}

int cpk_method_solve_multi(cpk_ctx ctx, int method, int64_t k, const double *B, int64_t ldb, cpk_mat A, cpk_mat C, cpk_pc M,
                           const cpk_opts *opts, double *X, int64_t ldx, double *Y, int64_t ldy, cpk_stats *stats,
                           int *col_status) {
    API_BEGIN
    need(ctx && A && C && M && B && X && (Y || !C->h.nrows), "NULL argument");
    int64_t ln[2] = {ldb, ldx}, lN[2] = {A->h.nrows + C->h.nrows, A->h.nrows + C->h.nrows};
    check_solve_multi(A, C, M, method, k, ln, ldy, lN);
    if (k == 0) return CPK_OK;
    Ctx &c = ctx->c;
    Precond &p = *M->p;
    HostBlock dB(p.n, k), dXY(p.N, k);
    dB.up(B, ldb);
    auto t0 = std::chrono::steady_clock::now();
    std::string msg;
    const int rc = method_solve_multi_device(c, method, k, dB.d.p, dB.ld(), A->krylov_op(C, p), p, opts, dXY.d.p, dXY.ld(),
                                             stats, col_status, &msg);
    dXY.down(X, ldx, 0, p.n);
    dXY.down(Y, ldy, p.n, p.m);
    const double st = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats)
        for (int64_t j = 0; j < k; j++) stats[j].stime = st;
    return solve_multi_result(rc, msg);
    API_END
}

// reg_cpkrylov.m:152-175 per column with an existing M: shift, method, recovery
int cpk_reg_solve_multi_device(cpk_ctx ctx, int method, int64_t k, const double *d_B, int64_t ldb, cpk_mat A, cpk_mat B,
                               cpk_mat C, cpk_pc M, const cpk_opts *opts, double *d_X, int64_t ldx, cpk_stats *stats,
                               int *col_status) {
    API_BEGIN
    need(ctx && A && B && C && M && d_B && d_X, "NULL argument");
    int64_t ln[2] = {A->h.nrows, A->h.nrows}, lN[2] = {ldb, ldx};
    check_solve_multi(A, C, M, method, k, ln, C->h.nrows, lN);
    if (k == 0) return CPK_OK;
    const ShiftOps so = shift_ops(A, C, *M->p);
    std::string msg;
    const int rc = reg_solve_multi_device(ctx->c, method, k, d_B, ldb, A->krylov_op(C, *M->p), *so.A, *so.Bt, so.bt_colmin,
                                          *M->p, opts, d_X, ldx, stats, col_status, &msg);
    return solve_multi_result(rc, msg);
    API_END
}

int cpk_reg_solve_multi(cpk_ctx ctx, int method, int64_t k, const double *Bh, int64_t ldb, cpk_mat A, cpk_mat B, cpk_mat C,
                        cpk_pc M, const cpk_opts *opts, double *X, int64_t ldx, cpk_stats *stats, int *col_status) {
    API_BEGIN
    need(ctx && A && B && C && M && Bh && X, "NULL argument");
    int64_t ln[2] = {A->h.nrows, A->h.nrows}, lN[2] = {ldb, ldx};
    check_solve_multi(A, C, M, method, k, ln, C->h.nrows, lN);
    if (k == 0) return CPK_OK;
    Precond &p = *M->p;
    HostBlock dB(p.N, k), dX(p.N, k);
    dB.up(Bh, ldb);
    const ShiftOps so = shift_ops(A, C, p);
    std::string msg;
    const int rc = reg_solve_multi_device(ctx->c, method, k, dB.d.p, dB.ld(), A->krylov_op(C, p), *so.A, *so.Bt,
                                          so.bt_colmin, p, opts, dX.d.p, dX.ld(), stats, col_status, &msg);
    dX.down(X, ldx);
    return solve_multi_result(rc, msg);
    API_END
}

// ---- the block forms of the verified solve and of its adjoint: the checks first ------------------
static void check_kkt_solve_multi(cpk_kkt K, int method, int64_t k, const double *B, int64_t ldb, cpk_pc M, const double *X,
                                  int64_t ldx) {
    need(K && M && ((B && X) || !(K->n + K->m)), "NULL argument");
    const int64_t N = K->n + K->m;
    if (k < 0 || ldb < N || ldx < N)
        throw Error(CPK_ERR_DIM, "kkt_solve_multi: k >= 0 and leading dimensions >= N required");
    need(M->ctx == K->ctx, "kkt_solve_multi: M belongs to another context");
    check_method_dims(K->A, K->C, M);
    require_block_solve(K->ctx->c, *M->p, method);
}

int cpk_kkt_solve_multi_device(cpk_kkt K, int method, int64_t k, const double *d_B, int64_t ldb, cpk_pc M,
                               const cpk_opts *opts, double *d_X, int64_t ldx, int warm, cpk_stats *stats, int *col_status,
                               double *res) {
    API_BEGIN
    check_kkt_solve_multi(K, method, k, d_B, ldb, M, d_X, ldx);
    std::string msg;
    const int rc = kkt_solve_multi_core(K, method, k, d_B, ldb, M, opts, d_X, ldx, warm, stats, col_status, res, &msg);
    return solve_multi_result(rc, msg);
    API_END
}

int cpk_kkt_solve_multi(cpk_kkt K, int method, int64_t k, const double *B, int64_t ldb, cpk_pc M, const cpk_opts *opts,
                        double *X, int64_t ldx, int warm, cpk_stats *stats, int *col_status, double *res) {
    API_BEGIN
    check_kkt_solve_multi(K, method, k, B, ldb, M, X, ldx);
    if (k == 0) return CPK_OK;
    const int64_t N = K->n + K->m;
    HostBlock dB(N, k), dX(N, k);
    dB.up(B, ldb);
    if (warm) dX.up(X, ldx);
    std::string msg;
    const int rc = kkt_solve_multi_core(K, method, k, dB.d.p, dB.ld(), M, opts, dX.d.p, dX.ld(), warm, stats, col_status, res,
                                        &msg);
    dX.down(X, ldx);
    return solve_multi_result(rc, msg);
    API_END
}

static void check_kkt_sample(cpk_kkt K, int64_t k, const double *X, int64_t ldx, const double *L, int64_t ldl,
                             const double *gA, int64_t cA, const double *gB, int64_t cB, const double *gC, int64_t cC) {
    need(K && ((X && L) || !(K->n + K->m) || k == 0), "NULL argument");
    const int64_t N = K->n + K->m;
    if (k < 0 || k > INT32_MAX / 2 || ldx < N || ldl < N)
        throw Error(CPK_ERR_DIM, "kkt_sample_multi: k >= 0 and leading dimensions >= N required");
    check_grad_counts(K, gA, cA, gB, cB, gC, cC,
                      "kkt_sample_multi: a gradient's count differs from its handle's creating call's entry count");
    if (K->ctx->c.dist()) throw Error(CPK_ERR_UNSUPPORTED, "kkt_sample_multi: single-GPU only");
}

int cpk_kkt_set_sample_route(cpk_kkt K, int route) {
    API_BEGIN
    need(K != nullptr, "NULL argument");
    need(route >= 0 && route <= 2, "kkt_set_sample_route: 0 (by the crossover), 1 (panel kernel) or 2 (run-time-k kernel)");
    K->sample_route = route;
    API_END
}

int cpk_kkt_sample_route_info(cpk_kkt K, int64_t info[4]) {
    API_BEGIN
    need(K && info, "NULL argument");
    const int64_t v[4] = {kMultiKP, kSamplePanelMaxPad, K->sample_route, K->sample_panels};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_kkt_sample_multi_device(cpk_kkt K, int64_t k, const double *d_X, int64_t ldx, const double *d_Lam, int64_t ldl,
                                double *d_gA, int64_t cA, double *d_gB, int64_t cB, double *d_gC, int64_t cC) {
    API_BEGIN
    check_kkt_sample(K, k, d_X, ldx, d_Lam, ldl, d_gA, cA, d_gB, cB, d_gC, cC);
    kkt_sample_core(K, k, d_X, ldx, d_Lam, ldl, d_gA, d_gB, d_gC);
    CPK_HIP(hipStreamSynchronize(K->ctx->c.stream));  // the gradients are the caller's
    API_END
}

int cpk_kkt_sample_multi(cpk_kkt K, int64_t k, const double *X, int64_t ldx, const double *Lam, int64_t ldl, double *gA,
                         int64_t cA, double *gB, int64_t cB, double *gC, int64_t cC) {
    API_BEGIN
    check_kkt_sample(K, k, X, ldx, Lam, ldl, gA, cA, gB, cB, gC, cC);
    const int64_t N = K->n + K->m;
    HostBlock dX(N, k), dL(N, k);
    dX.up(X, ldx), dL.up(Lam, ldl);
    HostGrads g(gA, cA, gB, cB, gC, cC);
    kkt_sample_core(K, k, dX.d.p, dX.ld(), dL.d.p, dL.ld(), g.dev(0), g.dev(1), g.dev(2));
    g.down(K->ctx->c.stream);
    API_END
}

// Lam = cpk_kkt_solve_multi(K, GX), then cpk_kkt_sample_multi(K, X, Lam).  A column whose driver
// stopped returns its status before any gradient pass is enqueued (the single-column rule)
static void check_kkt_adjoint_multi(cpk_kkt K, int method, int64_t k, const double *X, int64_t ldx, const double *GX,
                                    int64_t ldg, cpk_pc M, const double *Lam, int64_t ldl, const double *gA, int64_t cA,
                                    const double *gB, int64_t cB, const double *gC, int64_t cC) {
    need(K && M && ((X && GX && Lam) || !(K->n + K->m)), "NULL argument");
    check_kkt_sample(K, k, X, ldx, Lam, ldl, gA, cA, gB, cB, gC, cC);
    check_kkt_solve_multi(K, method, k, GX, ldg, M, Lam, ldl);
}

int cpk_kkt_adjoint_multi_device(cpk_kkt K, int method, int64_t k, const double *d_X, int64_t ldx, const double *d_GX,
                                 int64_t ldg, cpk_pc M, const cpk_opts *opts, double *d_Lam, int64_t ldl, int warm,
                                 double *d_gA, int64_t cA, double *d_gB, int64_t cB, double *d_gC, int64_t cC,
                                 cpk_stats *stats, int *col_status, double *res) {
    API_BEGIN
    check_kkt_adjoint_multi(K, method, k, d_X, ldx, d_GX, ldg, M, d_Lam, ldl, d_gA, cA, d_gB, cB, d_gC, cC);
    std::string msg;
    const int rc = kkt_solve_multi_core(K, method, k, d_GX, ldg, M, opts, d_Lam, ldl, warm, stats, col_status, res, &msg);
    if (rc != CPK_OK) return solve_multi_result(rc, msg);
    kkt_sample_core(K, k, d_X, ldx, d_Lam, ldl, d_gA, d_gB, d_gC);
    CPK_HIP(hipStreamSynchronize(K->ctx->c.stream));
    API_END
}

int cpk_kkt_adjoint_multi(cpk_kkt K, int method, int64_t k, const double *X, int64_t ldx, const double *GX, int64_t ldg,
                          cpk_pc M, const cpk_opts *opts, double *Lam, int64_t ldl, int warm, double *gA, int64_t cA,
                          double *gB, int64_t cB, double *gC, int64_t cC, cpk_stats *stats, int *col_status, double *res) {
    API_BEGIN
    check_kkt_adjoint_multi(K, method, k, X, ldx, GX, ldg, M, Lam, ldl, gA, cA, gB, cB, gC, cC);
    const int64_t N = K->n + K->m;
    HostBlock dX(N, k), dG(N, k), dL(N, k);
    dX.up(X, ldx), dG.up(GX, ldg);
    if (warm) dL.up(Lam, ldl);
    HostGrads g(gA, cA, gB, cB, gC, cC);
    std::string msg;
    const int rc = kkt_solve_multi_core(K, method, k, dG.d.p, dG.ld(), M, opts, dL.d.p, dL.ld(), warm, stats, col_status, res,
                                        &msg);
    dL.down(Lam, ldl);
    if (rc != CPK_OK) return solve_multi_result(rc, msg);
    kkt_sample_core(K, k, dX.d.p, dX.ld(), dL.d.p, dL.ld(), g.dev(0), g.dev(1), g.dev(2));
    g.down(K->ctx->c.stream);
    API_END
}

// diagnostic: the panel Krylov product alone, host arrays (X, Y: N x k; dots: 2 k)
int cpk_debug_spmm(cpk_ctx ctx, cpk_mat A, cpk_mat C, cpk_pc M, int64_t k, const double *X, int64_t ldx, double *Y,
                   int64_t ldy, double *dots) {
    API_BEGIN
    need(ctx && A && C && M && X && Y && dots, "NULL argument");
    check_method_dims(A, C, M);
    Precond &p = *M->p;
    const int64_t N = p.N;
    if (k < 0 || ldx < N || ldy < N) throw Error(CPK_ERR_DIM, "debug_spmm: k >= 0 and leading dimensions >= N required");
    if (k == 0) return CPK_OK;
    HostBlock dX(N, k), dY(N, k);
    DBuf<double> dd;
    dd.alloc(2 * (size_t)k);
    dX.up(X, ldx);
    debug_spmm(ctx->c, A->krylov_op(C, p), p, k, dX.d.p, dX.ld(), dY.d.p, dY.ld(), dd.p);
    dY.down(Y, ldy);
    CPK_HIP(hipMemcpy(dots, dd.p, 2 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost));
    API_END
}

// diagnostic: nv inner products of host n-vectors through the solvers' reducing launches
int cpk_debug_dot(cpk_ctx ctx, int kind, int64_t n, int nv, const double *A, int64_t lda, const double *B, int64_t ldb,
                  int grid, double *out) {
    API_BEGIN
    need(ctx && A && B && out, "NULL argument");
    need(kind == 0 || kind == 1, "debug_dot: kind is 0 (ewred) or 1 (ewtred)");
    need(nv == 1 || nv == 2 || nv == 4, "debug_dot: nv is 1, 2 or 4");
    need(n >= 0 && lda >= n && ldb >= n, "debug_dot: n >= 0 and leading dimensions >= n required");
    need(grid >= 0, "debug_dot: grid >= 0 required");
    HostBlock dA(n, nv), dB(n, nv);
    DBuf<double> dd;
    dd.alloc((size_t)nv);
    dA.up(A, lda), dB.up(B, ldb);
    debug_dot(ctx->c, kind, n, nv, dA.d.p, dA.ld(), dB.d.p, dB.ld(), grid, dd.p);
    CPK_HIP(hipMemcpy(out, dd.p, (size_t)nv * sizeof(double), hipMemcpyDeviceToHost));
    API_END
}

// diagnostic: out[i] = xnorm2(a[i], b[i]) (xacc.hpp) on the device, host arrays
int cpk_debug_xnorm2(cpk_ctx ctx, int64_t n, const double *a, const double *b, double *out) {
    API_BEGIN
    need(ctx && a && b && out, "NULL argument");
    need(n >= 0, "debug_xnorm2: n >= 0 required");
    if (n == 0) return CPK_OK;
    DBuf<double> da, db, dout;
    h2d(da, a, (size_t)n), h2d(db, b, (size_t)n), dout.alloc((size_t)n);
    debug_xnorm2(ctx->c, n, da.p, db.p, dout.p);
    CPK_HIP(hipMemcpy(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    API_END
}

// diagnostic: one Arnoldi step of cpgmres / cpdqgmres on host arrays, through the solvers' launches
int cpk_debug_arnoldi_step(cpk_ctx ctx, cpk_arnoldi_step *io) {
    API_BEGIN
    need(ctx && io, "NULL argument");
    cpk_arnoldi_step &s = *io;
    const bool dq = s.method == CPK_DQGMRES;
    need(dq || s.method == CPK_GMRES, "debug_arnoldi_step: method is CPK_GMRES or CPK_DQGMRES");
    need(s.V && s.w && s.ut && s.H && s.c && s.s && s.g, "NULL argument");
    need(!dq || (s.PV && s.xy), "debug_arnoldi_step: cpdqgmres needs PV and xy");
    need(s.N >= 0 && s.n >= 0 && s.n <= s.N, "debug_arnoldi_step: 0 <= n <= N required");
    need(s.win >= 1 && s.win <= (int64_t)1 << 20, "debug_arnoldi_step: 1 <= restart, mem <= 2^20 required");
    need(s.kk >= 1 && (dq || s.kk <= s.win), "debug_arnoldi_step: kk >= 1 (cpgmres: kk <= restart) required");
    need(s.grid >= 0, "debug_arnoldi_step: grid >= 0 required");
    need(s.ldv >= s.N && (!dq || s.ldpv >= s.N), "debug_arnoldi_step: leading dimensions >= N required");
    if (ctx->c.opts.basis_f32 && ctx->c.dist())  // before any device call, like the argument checks
        throw Error(CPK_ERR_UNSUPPORTED, "engine option basis_f32: the Arnoldi step on a distributed context");
    const int64_t N = s.N, cols = s.win + 1;
    HostBlock dV(N, cols), dPV(N, dq ? cols : 1), dxy(N, 1), dw(N, 1), dut(N, 1);
    dV.up(s.V, s.ldv), dw.up(s.w, N), dut.up(s.ut, N);
    if (dq) dPV.up(s.PV, s.ldpv), dxy.up(s.xy, N);
    debug_arnoldi_step(ctx->c, s, dV.d.p, dPV.d.p, dxy.d.p, dw.d.p, dut.d.p);
    dV.down(s.V, s.ldv);
    if (dq) dPV.down(s.PV, s.ldpv), dxy.down(s.xy, N);
    API_END
}

int cpk_debug_spmm_time(cpk_ctx ctx, cpk_mat A, cpk_mat C, cpk_pc M, int kc, int reps, double *ms_panel, double *ms_single) {
    API_BEGIN
    need(ctx && A && C && M && ms_panel && ms_single, "NULL argument");
    check_method_dims(A, C, M);
    debug_spmm_time(ctx->c, A->krylov_op(C, *M->p), *M->p, kc, reps, ms_panel, ms_single);
    API_END
}

int cpk_profile_kernels(cpk_ctx ctx, cpk_mat A, cpk_mat C, cpk_pc M, int reps, cpk_profile *out) {
    API_BEGIN
    need(ctx && out, "NULL argument");
    check_method_dims(A, C, M);
    profile_kernels(ctx->c, A->krylov_op(C, *M->p), *M->p, reps, out);
    API_END
}

int cpk_debug_pipe_stamps(uint64_t *out, int npairs, int *copied) {
    API_BEGIN
    need(out && copied, "NULL argument");
    *copied = debug_pipe_stamps(out, npairs);
    API_END
}

int cpk_debug_blk_cycles(uint64_t *out, int64_t n, int64_t *copied) {
    API_BEGIN
    need(out && copied, "NULL argument");
    *copied = debug_blk_cycles(out, n);
    API_END
}

int cpk_debug_pass_times(cpk_ctx ctx, double *out) {
    API_BEGIN
    need(ctx && out, "NULL argument");
    std::memcpy(out, ctx->c.pass_ms, sizeof ctx->c.pass_ms);
    API_END
}

int cpk_debug_block_model(cpk_pc M, int64_t *out, int64_t n, int64_t *copied) {
    API_BEGIN
    need(M && copied, "NULL argument");
    // the rank's own sweeps, then (a distributed separator solved by the block sweeps) the T
    // sweep's, its directions reported as 2 (forward) and 3 (backward)
    std::vector<int64_t> h = M->p->dF.hmodel;
    if (M->p->sep.tsweep) {
        const size_t at = h.size();
        h.insert(h.end(), M->p->sep.tsw.hmodel.begin(), M->p->sep.tsw.hmodel.end());
        for (size_t i = at + 1; i < h.size(); i += kBlockModelW) h[i] += 2;
    }
    *copied = std::min<int64_t>(n, (int64_t)h.size());
    if (out && *copied) std::memcpy(out, h.data(), (size_t)*copied * sizeof(int64_t));
    API_END
}

int cpk_pc_sep_info(cpk_pc M, int64_t *info) {
    API_BEGIN
    need(M && info, "NULL argument");
    const Precond &p = *M->p;
    const DSep &T = p.sep;
    const int64_t v[12] = {p.dist ? 1 : 0, T.nT, T.nlev, T.nrec, (int64_t)T.lds, (int64_t)T.lds_g, T.kt, p.tkr ? 1 : 0,
                           p.dsched ? 1 : 0, (p.dsched && p.fused_resid && !p.dF.no_fused_resid) ? 1 : 0,
                           T.tsweep ? 1 : 0, T.tsweep ? (int64_t)T.tsw.round_ptr.size() - 1 : 0};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_pc_sweep_info(cpk_pc M, int64_t *info) {
    API_BEGIN
    need(M && info, "NULL argument");
    const DFactor &F = M->p->dF;
    const int64_t nr = (int64_t)F.round_ptr.size() - 1;
    const int64_t r0 = nr >= 1 ? F.round_ptr[1] - F.round_ptr[0] : 0;
    // the chain the sweeps launch: the full one (last round fused), else the forward one
    const int64_t chain = F.no_chain ? 0
                          : (F.chain[kChainFull].ntask > 0 && fuse_last_ok(F)) ? F.chain[kChainFull].ntask
                                                                               : F.chain[kChainFwd].ntask;
    const int64_t v[8] = {nr, r0, F.nblk - r0, F.agrid[0], F.agrid[1], F.agrid[2], F.pipelined ? 1 : 0, chain};
    std::memcpy(info, v, sizeof v);
    API_END
}

int cpk_pc_local_dofs(cpk_pc M, int64_t *n_loc, int64_t *m_loc, int32_t *dofs) {
    API_BEGIN
    need(M, "NULL argument");
    const Precond &p = *M->p;
    if (n_loc) *n_loc = p.n;
    if (m_loc) *m_loc = p.m;
    if (dofs) {
        if (p.dist) {
            const std::vector<int32_t> d = p.dofmap->dofs(M->ctx->c.rank);
            std::memcpy(dofs, d.data(), d.size() * sizeof(int32_t));
        } else {
            for (int64_t i = 0; i < p.N; i++) dofs[i] = (int32_t)i;
        }
    }
    API_END
}

int cpk_reg_solve(cpk_ctx ctx, int method, const double *b, cpk_mat A, cpk_mat B, cpk_mat C, cpk_mat G,
                  const cpk_opts *opts, double *x, cpk_stats *stats, cpk_pc *M_out) {
    API_BEGIN
    // reg_cpkrylov.m:122-125
    if (!ctx || !b || !A || !B || !C || !G || !x) throw Error(CPK_ERR_ARGS, "reg_cpkrylov: not enough inputs");
    Ctx &c = ctx->c;
    // M = opLDL2(G, B, -C)   (reg_cpkrylov.m:128-132)
    HCsr negC = C->host();
    for (auto &v : negC.val) v = -v;
    check_dist_method(c, method);
    auto pc = std::make_unique<cpk_pc_s>();
    pc->ctx = ctx;
    if (c.dist()) pc->p.reset(precond_create_dist(c, G->host(), B->host(), negC, &A->host()));
    else pc->p.reset(precond_create(c, G->host(), B->host(), negC));
    Precond &p = *pc->p;
    apply_props(p, opts);  // reg_cpkrylov.m:135-148
    check_method_dims(A, C, pc.get());
    const int64_t N = p.N;
    const DMat &AC = A->krylov_op(C, p);
    const ShiftOps so = shift_ops(A, C, p);
    DBuf<double> db, dx;
    if (p.dist) scatter_global(p, b, N, db);
    else h2d(db, b, (size_t)N);
    dx.alloc((size_t)std::max<int64_t>(N, 1));
    reg_solve_device(c, method, db.p, AC, *so.A, *so.Bt, so.bt_colmin, p, opts, dx.p, stats);
    if (p.dist) gather_global(c, p, dx.p, x);
    else CPK_HIP(hipMemcpy(x, dx.p, N * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) stats->ptime = pc->p->ptime;
    if (M_out) *M_out = pc.release();
    API_END
}

int cpk_analyze(cpk_mat A11, cpk_mat B, cpk_mat C22, const char *options, cpk_analysis *out) {
    API_BEGIN
    need(A11 && B && C22 && out, "NULL argument");
    auto a = std::make_unique<cpk_analysis_s>();
    a->opts = engine_opts_from_env();
    if (options) apply_engine_options(a->opts, options);
    a->an = analyze(A11->host(), B->host(), C22->host(), a->opts);
    *out = a.release();
    API_END
}

int cpk_analysis_destroy(cpk_analysis an) {
    API_BEGIN
    delete an;
    API_END
}

int cpk_analysis_get_info(cpk_analysis a, cpk_pc_info *info) {
    API_BEGIN
    need(a && info, "NULL argument");
    const Analysis &an = a->an;
    info->n = an.n, info->m = an.m, info->N = an.N;
    info->nnz_kp = an.Kp.nnz();
    info->nnz_l = (int64_t)an.F0.Li.size();
    info->nblocks = (int64_t)an.S.blk_row.size() - 1;
    info->nrounds = (int64_t)an.S.round_ptr.size() - 1;
    info->max_block_levels = an.S.max_levels;
    info->depth = an.S.depth;
    info->ordering = an.ordering;
    API_END
}

int cpk_analysis_export(cpk_analysis a, int64_t *Lcolptr, int32_t *Lrowind, double *Lval, double *D, int32_t *perm) {
    API_BEGIN
    need(a, "NULL argument");
    const Factor &f = a->an.F0;
    if (Lcolptr) std::memcpy(Lcolptr, f.Lp.data(), f.Lp.size() * sizeof(int64_t));
    if (Lrowind) std::memcpy(Lrowind, f.Li.data(), f.Li.size() * sizeof(int32_t));
    if (Lval) std::memcpy(Lval, f.Lx.data(), f.Lx.size() * sizeof(double));
    if (D) std::memcpy(D, f.D.data(), f.D.size() * sizeof(double));
    if (perm) std::memcpy(perm, f.perm.data(), f.perm.size() * sizeof(int32_t));
    API_END
}

int cpk_analysis_factor_report(cpk_analysis a, cpk_factor_report *out) {
    API_BEGIN
    need(a && out, "NULL argument");
    std::memcpy(out, &a->an.F0.rep, sizeof a->an.F0.rep);
    API_END
}

int cpk_analysis_pivot_shift(cpk_analysis a, double *E) {
    API_BEGIN
    need(a && E, "NULL argument");
    const Factor &f = a->an.F0;
    shift_to_dofs(f, f.E.empty() ? nullptr : f.E.data(), E);
    API_END
}

int cpk_analysis_schedule(cpk_analysis a, int64_t *nlevels, int64_t *round_ptr, int64_t *blk_lvl, int64_t *lvl_row,
                          int32_t *order) {
    API_BEGIN
    need(a, "NULL argument");
    const Schedule &s = a->an.S;
    if (order) std::memcpy(order, s.order.data(), s.order.size() * sizeof(int32_t));
    if (nlevels) *nlevels = (int64_t)s.lvl_row.size() - 1;
    if (round_ptr) std::memcpy(round_ptr, s.round_ptr.data(), s.round_ptr.size() * sizeof(int64_t));
    if (blk_lvl) std::memcpy(blk_lvl, s.blk_lvl.data(), s.blk_lvl.size() * sizeof(int64_t));
    if (lvl_row) std::memcpy(lvl_row, s.lvl_row.data(), s.lvl_row.size() * sizeof(int64_t));
    API_END
}

int cpk_analysis_round_caps(cpk_analysis a, int32_t *cap, int32_t *rows) {
    API_BEGIN
    need(a, "NULL argument");
    const Schedule &s = a->an.S;
    const SweepConfig &sw = a->an.sweep;
    for (size_t r = 0; r + 1 < s.round_ptr.size(); r++) {
        if (cap) cap[r] = r < s.round_cap.size() ? s.round_cap[r] : sw.cap[r == 0 ? 0 : 1];
        if (rows) rows[r] = r < s.round_rows.size() ? s.round_rows[r] : sw.rows[r == 0 ? 0 : 1];
    }
    API_END
}

int cpk_analysis_rowspan(cpk_analysis a, int64_t block, int dir, int64_t cap_entries, cpk_rowspan_info *info,
                         int64_t *rowptr, int32_t *col, double *val, int32_t *dest, int32_t *step, int32_t *lead,
                         uint64_t *mask, int32_t *base, int32_t *first, int32_t *run0, uint8_t *tab) {
    API_BEGIN
    need(a && info, "NULL argument");
    if (a->rs_key[0] != block || a->rs_key[1] != dir || a->rs_key[2] != cap_entries) {
        a->rs_key[0] = -1;
        rowspan_export(a->an.F, a->an.S, block, dir, cap_entries, a->an.sweep.cap[1], a->rs_last);
        a->rs_key[0] = block, a->rs_key[1] = dir, a->rs_key[2] = cap_entries;
    }
    const RsExport &x = a->rs_last;
    info->eligible = x.eligible ? 1 : 0, info->r0 = x.r0, info->nr = x.nr, info->ne = x.ne, info->slots = x.slots;
    info->ndr = x.ndr, info->nrp = x.nrp, info->trips = x.trips, info->dset[0] = x.dset[0], info->dset[1] = x.dset[1];
    auto put = [](auto *dst, const auto &v) {
        if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof v[0]);
    };
    put(rowptr, x.rowptr), put(col, x.col), put(val, x.val), put(step, x.step);
    if (x.eligible) {
        put(dest, x.dest), put(lead, x.lead), put(tab, x.tab);
        for (size_t t = 0; t < x.rows.size(); t++) {
            if (mask) mask[2 * t] = x.rows[t].mlo, mask[2 * t + 1] = x.rows[t].mhi;
            if (base) base[t] = x.rows[t].base;
            if (first) first[t] = x.rows[t].first;
            if (run0) run0[t] = x.rows[t].run0;
        }
    }
    API_END
}

int cpk_analysis_plan(cpk_analysis a, cpk_mat A, cpk_mat C, int nranks, int rank, cpk_plan *out) {
    API_BEGIN
    need(a && A && C && out, "NULL argument");
    need(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
    const Analysis &an = a->an;
    need(A->h.nrows == an.n && A->h.ncols == an.n && C->h.nrows == an.m && C->h.ncols == an.m,
         "A and C must match the analysis' n and m");
    auto p = std::make_unique<cpk_plan_s>();
    p->n = an.n, p->m = an.m;
    p->ts = split_tree(an.F0, nranks, a->opts.split_tol, -1, &A->host());
    p->dm = make_dofmap(an.F0, p->ts, an.n);
    p->rp = make_rank_plan(an.F0, p->ts, p->dm, rank);
    p->kp = dist_csr(an.Kp, p->dm, rank, false);
    p->ac = dist_csr(blkdiag(A->host(), C->host()), p->dm, rank, false);
    p->ab = dist_csr(hstack_ab(A->host(), an.Kp, an.n), p->dm, rank, true);
    *out = p.release();
    API_END
}

int cpk_plan_destroy(cpk_plan p) {
    API_BEGIN
    delete p;
    API_END
}

int cpk_plan_array(cpk_plan p, const char *name, int64_t *count, void *out) {
    API_BEGIN
    need(p && name && count, "NULL argument");
    const RankPlan &r = p->rp;
    const std::string nm(name);
    std::vector<int64_t> iv;
    std::vector<double> dv;
    bool isd = false;
    auto I = [&](const auto &v) { iv.assign(v.begin(), v.end()); };
    auto Dv = [&](const std::vector<double> &v) { dv = v, isd = true; };
    const DistCsr *dc = nm.rfind("kp_", 0) == 0 ? &p->kp : nm.rfind("ac_", 0) == 0 ? &p->ac : nm.rfind("ab_", 0) == 0 ? &p->ab : nullptr;
    const std::string sub = dc ? nm.substr(3) : nm;
    if (dc) {
        if (sub == "ptr") I(dc->a.ptr);
        else if (sub == "col") I(dc->a.ind);
        else if (sub == "val") Dv(dc->a.val);
        else if (sub == "send") I(dc->send);
        else throw Error(CPK_ERR_ARGS, "unknown plan array " + nm);
    } else if (nm == "sizes") {
        const int64_t nl = p->dm.n_loc[r.rank], ml = p->dm.m_loc[r.rank];
        iv = {r.P, r.rank, p->n, p->m, p->n + p->m, nl, ml, nl + ml, r.nsub, r.nT, r.kt, p->kp.kmax, p->ac.kmax, p->ab.kmax};
    } else if (nm == "dofs") I(p->dm.dofs(r.rank));
    else if (nm == "node_rank") I(p->ts.node_rank);
    else if (nm == "T") I(p->ts.T);
    else if (nm == "fsub_Lp") I(r.Fsub.Lp);
    else if (nm == "fsub_Li") I(r.Fsub.Li);
    else if (nm == "fsub_Lx") Dv(r.Fsub.Lx);
    else if (nm == "fsub_D") Dv(r.Fsub.D);
    else if (nm == "fsub_perm") I(r.Fsub.perm);
    else if (nm == "fsub_parent") I(r.Fsub.parent);
    else if (nm == "fsub_key") I(r.key);
    else if (nm == "extra_ptr" || nm == "extra_col" || nm == "extra_key" || nm == "extra_val") {
        std::vector<int64_t> ptr{0}, col, key;
        std::vector<double> val;
        for (const auto &e : r.extra) {
            for (const BwdExtra &x : e) col.push_back(x.col), key.push_back(x.key), val.push_back(x.val);
            ptr.push_back((int64_t)col.size());
        }
        if (nm == "extra_ptr") iv = ptr;
        else if (nm == "extra_col") iv = col;
        else if (nm == "extra_key") iv = key;
        else dv = val, isd = true;
    } else if (nm == "tf_ptr") I(r.tf_ptr);
    else if (nm == "tf_col") I(r.tf_col);
    else if (nm == "tf_val") Dv(r.tf_val);
    else if (nm == "tf_src") I(r.tf_src);
    else if (nm == "tb_ptr") I(r.tb_ptr);
    else if (nm == "tb_col") I(r.tb_col);
    else if (nm == "tb_val") Dv(r.tb_val);
    else if (nm == "DT") Dv(r.DT);
    else if (nm == "tlev_ptr") I(r.tlev_ptr);
    else if (nm == "tlev_rows") I(r.tlev_rows);
    else if (nm == "tsend") I(r.tsend);
    else if (nm == "tdof") I(r.tdof);
    else throw Error(CPK_ERR_ARGS, "unknown plan array " + nm);
    *count = isd ? (int64_t)dv.size() : (int64_t)iv.size();
    if (out) {
        if (isd) std::memcpy(out, dv.data(), dv.size() * sizeof(double));
        else std::memcpy(out, iv.data(), iv.size() * sizeof(int64_t));
    }
    API_END
}

int cpk_symgivens(double a, double b, double *c, double *s, double *d) {
    API_BEGIN
    need(c && s && d, "NULL argument");
    auto sign = [](double v) { return (double)((v > 0) - (v < 0)); };
    if (b == 0) {
        *c = (a == 0) ? 1.0 : sign(a), *s = 0.0, *d = std::fabs(a);
    } else if (a == 0) {
        *c = 0.0, *s = sign(b), *d = std::fabs(b);
    } else if (std::fabs(b) > std::fabs(a)) {
        double t = a / b;
        *s = sign(b) / std::sqrt(1 + t * t), *c = *s * t, *d = b / *s;
    } else {
        double t = b / a;
        *c = sign(a) / std::sqrt(1 + t * t), *s = *c * t, *d = a / *c;
    }
    API_END
}

}  // extern "C"
