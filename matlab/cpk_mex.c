/*
 * cpk_mex.c -- MATLAB MEX gateway over libcpk (include/cpk.h).
 *
 * Build on a MATLAB host (not possible in this container):
 *   mex -largeArrayDims -I../include cpk_mex.c -L../cpkrylov_amd -lcpk
 *
 * Commands (first argument is the command string):
 *   h = cpk_mex('pc_create', G, B, Cneg)        % opLDL2(G, B, Cneg)       (opLDL2.m:60-92)
 *       cpk_mex('pc_set', h, opts)              % M.nitref = ... etc.      (opLDL2.m:97-115)
 *   y = cpk_mex('pc_apply', h, x)               % y = M*x                  (opLDL2.m:161-188)
 *   Y = cpk_mex('pc_apply_ldl', h, X)           % Y = M'*X = conj(M)*X, X dense N x k: the bare
 *                                               % factor composite         (opLDL2.m:127-136)
 *   Y = cpk_mex('pc_apply_multi', h, X)         % Y(:,j) = M*X(:,j), X dense N x k: the refined
 *                                               % apply column by column   (opLDL2.m:138-149, 161-188)
 *   x = cpk_mex('pc_divide', h, b)             % x = Kp*b                 (opLDL2.m:193-195)
 *       cpk_mex('pc_destroy', h)
 *   [x, y, stats, flag] = cpk_mex('method', name, b, A, C, h, opts)
 *                                               % method(b, A, C, M, opts) (kernels/cp*.m)
 *   [x, stats, flag] = cpk_mex('reg_solve', name, b, A, B, C, G, opts)
 *                                               % reg_cpkrylov             (reg_cpkrylov.m:1-180)
 *   [X, Y, stats, flag] = cpk_mex('method_solve_multi', name, B, A, C, h, opts)
 *                                               % method(B(:,j), A, C, M, opts) for every column of
 *                                               % the dense n x k B in lockstep (cpcg, cpminres;
 *                                               % kernels/cpcg.m:1, kernels/cpminres.m:1); stats.niters,
 *                                               % stats.histLen, stats.status and flag.solved are 1 x k,
 *                                               % stats.residHistory is (itmax + 4) x k, column j valid
 *                                               % up to histLen(j) and zero below.  A column on which the
 *                                               % reference stops with its error does not raise: its
 *                                               % stats.status is 1 (CPK_ERR_INDEFINITE), the others 0
 *   k = cpk_mex('kkt_create', A, B, C)          % the operator K = [A B'; B -C] of the system
 *                                               % reg_cpkrylov solves (reg_cpkrylov.m:1-40); the
 *                                               % handle owns device copies of A, B, C
 *   Y = cpk_mex('kkt_apply', k, Z)              % Y = K*Z, Z dense N x c
 *   [R, sums] = cpk_mex('kkt_residual', k, Z, B)   % R = B - K*Z, B and Z dense N x c; sums is 4 x c:
 *                                               % sum r(1:n)^2, r(n+1:N)^2, b(1:n)^2, b(n+1:N)^2 per column
 *   [x, stats, flag, res] = cpk_mex('kkt_solve', k, name, b, h, opts[, x0])
 *                                               % reg_cpkrylov's shift, method and recovery
 *                                               % (reg_cpkrylov.m:152-175) with the preconditioner h,
 *                                               % checked against K: res(1:4) the sums of the start
 *                                               % residual, res(5:8) those of b - K*x.  With x0 the solve
 *                                               % starts there: r = b - K*x0, the driver on r, x = x0 + dx
 *                                               % (atol, rtol then refer to the correction system)
 *       cpk_mex('kkt_destroy', k)
 *
 * Errors: every failure becomes mexErrMsgIdAndTxt after the call's temporaries are freed
 * (mexErrMsgIdAndTxt does not return: it unwinds to MATLAB, so the device matrices this call
 * made are tracked in g_tmp and destroyed first); CPK_ERR_INDEFINITE maps to the reference's
 * identifier CPCGLanczos:IndefiniteError.  tests/test_mex_shim.py drives this file against a
 * stand-in of the mx API (tests/mex_shim/) and counts what the error paths leave behind.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpk.h"
#include "mex.h"

static cpk_ctx g_ctx = NULL;

/* device matrices made by the current call: destroyed on every exit, error or not */
enum { kMaxTmp = 8 };
static cpk_mat g_tmp[kMaxTmp];
static int g_ntmp = 0;

static void release_tmp(void) {
    while (g_ntmp > 0) cpk_mat_destroy(g_tmp[--g_ntmp]);
}

static void cleanup(void) {
    release_tmp();
    if (g_ctx) cpk_ctx_destroy(g_ctx), g_ctx = NULL;
}

/* the one error exit: temporaries first, then MATLAB's error (which does not return) */
static void fail_msg(const char *id, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    release_tmp();
    mexErrMsgIdAndTxt(id, "%s", buf);
}

static void fail(int st) {
    char msg[512];
    snprintf(msg, sizeof msg, "%s", cpk_last_error()); /* before release_tmp can touch it */
    fail_msg(st == CPK_ERR_INDEFINITE ? "CPCGLanczos:IndefiniteError" : "cpk:error", "%s", msg);
}

static cpk_ctx ctx(void) {
    if (!g_ctx) {
        int st = cpk_ctx_create(-1, 0, 1, NULL, &g_ctx);
        if (st) fail(st);
        mexAtExit(cleanup);
    }
    return g_ctx;
}

/* MATLAB sparse (CSC, mwIndex = size_t with -largeArrayDims) -> device matrix */
static cpk_mat to_mat(const mxArray *a) {
    cpk_mat M = NULL;
    int st;
    if (!a || !mxIsSparse(a) || mxIsComplex(a)) fail_msg("cpk:args", "expected a real sparse matrix");
    if (g_ntmp == kMaxTmp) fail_msg("cpk:args", "internal: too many temporaries");
    st = cpk_mat_create_csc(ctx(), (int64_t)mxGetM(a), (int64_t)mxGetN(a), (const size_t *)mxGetJc(a),
                            (const size_t *)mxGetIr(a), mxGetPr(a), &M);
    if (st) fail(st);
    g_tmp[g_ntmp++] = M;
    return M;
}

static cpk_pc to_pc(const mxArray *h) {
    if (!h || !mxIsUint64(h) || mxGetNumberOfElements(h) != 1) fail_msg("cpk:args", "bad handle");
    return (cpk_pc)(uintptr_t)(*(uint64_t *)mxGetData(h));
}

/* a kkt handle: the operator and the device matrices it follows, which must outlive it */
typedef struct {
    cpk_kkt K;
    cpk_mat A, B, C;
    int64_t N;
} kkt_handle;

static kkt_handle *to_kkt(const mxArray *h) {
    if (!h || !mxIsUint64(h) || mxGetNumberOfElements(h) != 1) fail_msg("cpk:args", "bad handle");
    return (kkt_handle *)(uintptr_t)(*(uint64_t *)mxGetData(h));
}

/* a dense real matrix with N rows */
static void need_dense(const mxArray *a, int64_t N, const char *what) {
    if (!a || mxIsSparse(a) || mxIsComplex(a) || (int64_t)mxGetM(a) != N)
        fail_msg("cpk:dim", "%s: expected a dense real matrix with %lld rows", what, (long long)N);
}

/* opts struct -> cpk_opts, honouring isfield() (e.g. cpminres.m:98-111) */
static void to_opts(const mxArray *s, cpk_opts *o) {
    memset(o, 0, sizeof(*o));
    if (!s || !mxIsStruct(s)) return;
#define FIELD(name)                                                      \
    do {                                                                 \
        const mxArray *f = mxGetField(s, 0, #name);                      \
        if (f && !mxIsEmpty(f)) o->name = mxGetScalar(f), o->has_##name = 1; \
    } while (0)
    FIELD(atol); FIELD(rtol); FIELD(btol); FIELD(itmax); FIELD(restart); FIELD(mem); FIELD(print);
    FIELD(nitref); FIELD(itref_tol); FIELD(force_itref); FIELD(residual_update);
#undef FIELD
}

/* @cpminres, 'cpminres' or 'minres'; func2str may also give '@cpminres' or a package-qualified
 * 'pkg.cpminres', so a leading '@' and any prefix up to the last '.' are dropped */
static int method_id(const mxArray *a) {
    static const char *names[] = {"cpcg", "cpcglanczos", "cpminres", "cpsymmlq", "cpgmres", "cpdqgmres"};
    char buf[64];
    const char *nm;
    int i;
    buf[0] = '\0';
    if (!a) fail_msg("cpk:args", "method expected");
    if (mxIsClass(a, "function_handle")) { /* @cpminres -> 'cpminres' */
        mxArray *out = NULL, *in = (mxArray *)a;
        if (mexCallMATLAB(1, &out, 1, &in, "func2str") != 0 || !out) fail_msg("cpk:args", "func2str failed");
        mxGetString(out, buf, sizeof buf);
        mxDestroyArray(out);
    } else if (mxIsChar(a)) {
        mxGetString(a, buf, sizeof buf);
    } else {
        fail_msg("cpk:args", "method must be a function handle or a name");
    }
    nm = buf[0] == '@' ? buf + 1 : buf;
    if (strrchr(nm, '.')) nm = strrchr(nm, '.') + 1;
    for (i = 0; i < 6; i++)
        if (!strcmp(nm, names[i]) || !strcmp(nm, names[i] + 2)) return i;
    fail_msg("cpk:args", "unknown method %s", buf);
    return -1;
}

static mxArray *vec(const double *v, int64_t n) {
    mxArray *a = mxCreateDoubleMatrix((mwSize)n, 1, mxREAL);
    if (n) memcpy(mxGetPr(a), v, (size_t)n * sizeof(double));
    return a;
}

/* stats / flag structs as the reference returns them (cpminres.m:250-252, cpsymmlq.m:363-367) */
static void put_stats(int method, const cpk_stats *st, mxArray **stats, mxArray **flag) {
    const char *sf[] = {"niters", "residHistory", "ptime", "stime"};
    const char *lq[] = {"niters", "cgresidHistory", "lqresidHistory", "qrresidHistory", "ptime", "stime"};
    const char *ff[] = {"solved"};
    if (method == CPK_SYMMLQ) {
        *stats = mxCreateStructMatrix(1, 1, 6, lq);
        mxSetField(*stats, 0, "cgresidHistory", vec(st->hist, st->hist_len));
        mxSetField(*stats, 0, "lqresidHistory", vec(st->hist_lq, st->lq_len));
        mxSetField(*stats, 0, "qrresidHistory", vec(st->hist_qr, st->qr_len));
    } else {
        *stats = mxCreateStructMatrix(1, 1, 4, sf);
        mxSetField(*stats, 0, "residHistory", vec(st->hist, st->hist_len));
    }
    mxSetField(*stats, 0, "niters", mxCreateDoubleScalar((double)st->niters));
    mxSetField(*stats, 0, "ptime", mxCreateDoubleScalar(st->ptime));
    mxSetField(*stats, 0, "stime", mxCreateDoubleScalar(st->stime));
    *flag = mxCreateStructMatrix(1, 1, 1, ff);
    mxSetField(*flag, 0, "solved", mxCreateLogicalScalar(st->solved != 0));
}

/* history buffers of a method call (mxCalloc: MATLAB frees them itself if the call errors) */
static void alloc_hist(cpk_stats *s, int mid, const cpk_opts *o, int64_t n, int64_t m) {
    const double itmax = o->has_itmax ? o->itmax : (double)(mid >= CPK_GMRES ? n + m : n);
    memset(s, 0, sizeof *s);
    s->hist_cap = (int64_t)itmax + 4;
    if (mid == CPK_GMRES) s->hist_cap += o->has_restart ? (int64_t)o->restart : 50;
    s->hist = mxCalloc((size_t)s->hist_cap, sizeof(double));
    s->hist_lq = mxCalloc((size_t)s->hist_cap, sizeof(double));
    s->hist_qr = mxCalloc((size_t)s->hist_cap, sizeof(double));
}
static void free_hist(cpk_stats *s) { mxFree(s->hist), mxFree(s->hist_lq), mxFree(s->hist_qr); }

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    char cmd[32];
    int st = CPK_OK;
#define ARG(i) ((i) < nrhs ? prhs[i] : NULL)
    g_ntmp = 0;
    if (nrhs < 1 || !mxIsChar(prhs[0])) fail_msg("cpk:args", "cpk_mex: command string expected");
    mxGetString(prhs[0], cmd, sizeof cmd);
    {   /* argument counts before anything is converted or a device is touched */
        static const struct { const char *cmd; int nrhs; } need[] = {
            {"pc_create", 4}, {"pc_set", 3}, {"pc_apply", 3}, {"pc_apply_ldl", 3}, {"pc_apply_multi", 3}, {"pc_divide", 3}, {"pc_destroy", 2}, {"pc_factor_report", 2},
            {"method", 6}, {"reg_solve", 7}, {"method_solve_multi", 6},
            {"kkt_create", 4}, {"kkt_apply", 3}, {"kkt_residual", 4}, {"kkt_solve", 6}, {"kkt_destroy", 2}};
        int i;
        for (i = 0; i < (int)(sizeof need / sizeof need[0]); i++)
            if (!strcmp(cmd, need[i].cmd) && nrhs < need[i].nrhs)
                fail_msg("cpk:args", "cpk_mex %s: %d arguments expected, %d given", cmd, need[i].nrhs, nrhs);
    }

    if (!strcmp(cmd, "pc_create")) {
        cpk_mat G = to_mat(ARG(1)), B = to_mat(ARG(2)), C = to_mat(ARG(3));
        cpk_pc M = NULL;
        double ptime = 0;
        st = cpk_pc_create(ctx(), G, B, C, &ptime, &M);
        if (st) fail(st);
        release_tmp();
        plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
        *(uint64_t *)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)M;
    } else if (!strcmp(cmd, "pc_set")) {
        cpk_opts o;
        cpk_pc M = to_pc(ARG(1));
        to_opts(ARG(2), &o);
        if ((st = cpk_pc_set(M, &o))) fail(st);
    } else if (!strcmp(cmd, "pc_apply_ldl") || !strcmp(cmd, "pc_apply_multi")) {
        const int ldl = cmd[9] == 'l';
        cpk_pc M = to_pc(ARG(1));
        cpk_pc_info info;
        int64_t k;
        if ((st = cpk_pc_get_info(M, &info))) fail(st);
        if (!ARG(2) || mxIsSparse(ARG(2)) || mxIsComplex(ARG(2)) || (int64_t)mxGetM(ARG(2)) != info.N)
            fail_msg("cpk:dim", "expected a dense real matrix with %lld rows", (long long)info.N);
        k = (int64_t)mxGetN(ARG(2));
        plhs[0] = mxCreateDoubleMatrix((mwSize)info.N, (mwSize)k, mxREAL);
        if (k == 1)
            st = ldl ? cpk_pc_apply_ldl(M, mxGetPr(ARG(2)), mxGetPr(plhs[0]))
                     : cpk_pc_apply(M, mxGetPr(ARG(2)), mxGetPr(plhs[0]));
        else if (k > 0 && info.N > 0) /* MATLAB stores a dense matrix column-major, leading dimension N */
            st = ldl ? cpk_pc_apply_ldl_multi(M, k, mxGetPr(ARG(2)), info.N, mxGetPr(plhs[0]), info.N)
                     : cpk_pc_apply_multi(M, k, mxGetPr(ARG(2)), info.N, mxGetPr(plhs[0]), info.N, NULL);
        if (st) fail(st);
    } else if (!strcmp(cmd, "pc_apply") || !strcmp(cmd, "pc_divide")) {
        cpk_pc M = to_pc(ARG(1));
        cpk_pc_info info;
        if ((st = cpk_pc_get_info(M, &info))) fail(st);
        if (!ARG(2) || mxIsSparse(ARG(2)) || (int64_t)mxGetNumberOfElements(ARG(2)) != info.N)
            fail_msg("cpk:dim", "expected a dense vector of length %lld", (long long)info.N);
        plhs[0] = mxCreateDoubleMatrix((mwSize)info.N, 1, mxREAL);
        st = cmd[3] == 'a' ? cpk_pc_apply(M, mxGetPr(ARG(2)), mxGetPr(plhs[0]))
                           : cpk_pc_divide(M, mxGetPr(ARG(2)), mxGetPr(plhs[0]));
        if (st) fail(st);
    } else if (!strcmp(cmd, "pc_factor_report")) {
        /* [report, E] = cpk_mex('pc_factor_report', M): the inertia and pivot information MA57's
         * ldl returns with the factors (opLDL2.m:81-82); positions are 0-based pivot positions */
        static const char *rf[] = {"n_pos", "n_neg", "n_wrong", "first_wrong", "n_perturbed", "argmin_abs",
                                   "min_abs", "max_abs", "max_shift", "pivot_min"};
        cpk_pc M = to_pc(ARG(1));
        cpk_factor_report r;
        if ((st = cpk_pc_factor_report(M, &r))) fail(st);
        plhs[0] = mxCreateStructMatrix(1, 1, 10, rf);
        mxSetField(plhs[0], 0, "n_pos", mxCreateDoubleScalar((double)r.n_pos));
        mxSetField(plhs[0], 0, "n_neg", mxCreateDoubleScalar((double)r.n_neg));
        mxSetField(plhs[0], 0, "n_wrong", mxCreateDoubleScalar((double)r.n_wrong));
        mxSetField(plhs[0], 0, "first_wrong", mxCreateDoubleScalar((double)r.first_wrong));
        mxSetField(plhs[0], 0, "n_perturbed", mxCreateDoubleScalar((double)r.n_perturbed));
        mxSetField(plhs[0], 0, "argmin_abs", mxCreateDoubleScalar((double)r.argmin_abs));
        mxSetField(plhs[0], 0, "min_abs", mxCreateDoubleScalar(r.min_abs));
        mxSetField(plhs[0], 0, "max_abs", mxCreateDoubleScalar(r.max_abs));
        mxSetField(plhs[0], 0, "max_shift", mxCreateDoubleScalar(r.max_shift));
        mxSetField(plhs[0], 0, "pivot_min", mxCreateDoubleScalar(r.pivot_min));
        if (nlhs > 1) {
            cpk_pc_info info;
            if ((st = cpk_pc_get_info(M, &info))) fail(st);
            plhs[1] = mxCreateDoubleMatrix((mwSize)info.N, 1, mxREAL);
            if (info.N > 0 && (st = cpk_pc_pivot_shift(M, mxGetPr(plhs[1])))) fail(st);
        }
    } else if (!strcmp(cmd, "pc_destroy")) {
        cpk_pc_destroy(to_pc(ARG(1)));
    } else if (!strcmp(cmd, "method")) {
        const int mid = method_id(ARG(1));
        cpk_mat A = to_mat(ARG(3)), C = to_mat(ARG(4));
        cpk_pc M = to_pc(ARG(5));
        cpk_opts o;
        cpk_stats s;
        const int64_t n = (int64_t)mxGetM(ARG(3)), m = (int64_t)mxGetM(ARG(4));
        mxArray *x, *y;
        if (!ARG(2) || (int64_t)mxGetNumberOfElements(ARG(2)) != n) fail_msg("cpk:dim", "b must have length %lld", (long long)n);
        to_opts(ARG(6), &o);
        alloc_hist(&s, mid, &o, n, m);
        x = mxCreateDoubleMatrix((mwSize)n, 1, mxREAL);
        y = mxCreateDoubleMatrix((mwSize)m, 1, mxREAL);
        st = cpk_method_solve(ctx(), mid, mxGetPr(ARG(2)), A, C, M, &o, mxGetPr(x), mxGetPr(y), &s);
        if (st) fail(st);
        release_tmp();
        plhs[0] = x, plhs[1] = y;
        put_stats(mid, &s, &plhs[2], &plhs[3]);
        free_hist(&s);
    } else if (!strcmp(cmd, "reg_solve")) {
        const int mid = method_id(ARG(1));
        cpk_mat A = to_mat(ARG(3)), B = to_mat(ARG(4)), C = to_mat(ARG(5)), G = to_mat(ARG(6));
        cpk_opts o;
        cpk_stats s;
        const int64_t n = (int64_t)mxGetM(ARG(3)), m = (int64_t)mxGetM(ARG(4));
        if (!ARG(2) || (int64_t)mxGetNumberOfElements(ARG(2)) != n + m)
            fail_msg("cpk:dim", "b must have length %lld", (long long)(n + m));
        to_opts(ARG(7), &o);
        alloc_hist(&s, mid, &o, n, m);
        plhs[0] = mxCreateDoubleMatrix((mwSize)(n + m), 1, mxREAL);
        st = cpk_reg_solve(ctx(), mid, mxGetPr(ARG(2)), A, B, C, G, &o, mxGetPr(plhs[0]), &s, NULL);
        if (st) fail(st);
        release_tmp();
        put_stats(mid, &s, &plhs[1], &plhs[2]);
        free_hist(&s);
    } else if (!strcmp(cmd, "method_solve_multi")) {
        const int mid = method_id(ARG(1));
        const char *sf[] = {"niters", "residHistory", "histLen", "status"};
        const char *ff[] = {"solved"};
        cpk_mat A, C;
        cpk_pc M;
        cpk_opts o;
        cpk_stats *s;
        int *status;
        int64_t n, m, k, cap, j, i;
        mxArray *X, *Y, *nit, *hist, *hlen, *stt, *solved;
        if (!ARG(2) || mxIsSparse(ARG(2)) || mxIsComplex(ARG(2))) fail_msg("cpk:args", "B must be a dense real matrix");
        A = to_mat(ARG(3)), C = to_mat(ARG(4));
        M = to_pc(ARG(5));
        n = (int64_t)mxGetM(ARG(3)), m = (int64_t)mxGetM(ARG(4));
        if ((int64_t)mxGetM(ARG(2)) != n) fail_msg("cpk:dim", "B must have %lld rows", (long long)n);
        k = (int64_t)mxGetN(ARG(2));
        to_opts(ARG(6), &o);
        cap = (int64_t)(o.has_itmax ? o.itmax : (double)n) + 4;
        s = mxCalloc((size_t)(k > 0 ? k : 1), sizeof *s);
        status = mxCalloc((size_t)(k > 0 ? k : 1), sizeof *status);
        hist = mxCreateDoubleMatrix((mwSize)cap, (mwSize)k, mxREAL);
        for (j = 0; j < k; j++) s[j].hist = mxGetPr(hist) + j * cap, s[j].hist_cap = cap;
        X = mxCreateDoubleMatrix((mwSize)n, (mwSize)k, mxREAL);
        Y = mxCreateDoubleMatrix((mwSize)m, (mwSize)k, mxREAL);
        /* MATLAB stores a dense matrix column-major: the leading dimensions are the row counts */
        st = cpk_method_solve_multi(ctx(), mid, k, mxGetPr(ARG(2)), n > 0 ? n : 1, A, C, M, &o, mxGetPr(X), n > 0 ? n : 1,
                                    mxGetPr(Y), m > 0 ? m : 1, s, status);
        for (j = 0, i = 0; j < k; j++) i |= status[j];
        if (st && !i) fail(st); /* refused or failed as a whole; a failing column is reported in stats.status */
        release_tmp();
        nit = mxCreateDoubleMatrix(1, (mwSize)k, mxREAL), hlen = mxCreateDoubleMatrix(1, (mwSize)k, mxREAL);
        stt = mxCreateDoubleMatrix(1, (mwSize)k, mxREAL), solved = mxCreateDoubleMatrix(1, (mwSize)k, mxREAL);
        for (j = 0; j < k; j++) {
            mxGetPr(nit)[j] = (double)s[j].niters, mxGetPr(hlen)[j] = (double)s[j].hist_len;
            mxGetPr(stt)[j] = (double)status[j], mxGetPr(solved)[j] = s[j].solved ? 1.0 : 0.0;
        }
        plhs[0] = X, plhs[1] = Y;
        plhs[2] = mxCreateStructMatrix(1, 1, 4, sf);
        mxSetField(plhs[2], 0, "niters", nit), mxSetField(plhs[2], 0, "residHistory", hist);
        mxSetField(plhs[2], 0, "histLen", hlen), mxSetField(plhs[2], 0, "status", stt);
        plhs[3] = mxCreateStructMatrix(1, 1, 1, ff);
        mxSetField(plhs[3], 0, "solved", solved);
        mxFree(s), mxFree(status);
    } else if (!strcmp(cmd, "kkt_create")) {
        cpk_mat A = to_mat(ARG(1)), B = to_mat(ARG(2)), C = to_mat(ARG(3));
        kkt_handle *k;
        cpk_kkt K = NULL;
        int64_t info[8];
        if ((st = cpk_kkt_create(ctx(), A, B, C, &K))) fail(st);
        if ((st = cpk_kkt_get_info(K, info))) {
            cpk_kkt_destroy(K);
            fail(st);
        }
        k = malloc(sizeof *k);
        if (!k) {
            cpk_kkt_destroy(K);
            fail_msg("cpk:error", "out of host memory");
        }
        k->K = K, k->A = A, k->B = B, k->C = C, k->N = info[0] + info[1];
        g_ntmp = 0; /* the three matrices now belong to the handle */
        plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
        *(uint64_t *)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)k;
    } else if (!strcmp(cmd, "kkt_destroy")) {
        kkt_handle *k = to_kkt(ARG(1));
        if (k) {
            cpk_kkt_destroy(k->K);
            cpk_mat_destroy(k->A), cpk_mat_destroy(k->B), cpk_mat_destroy(k->C);
            free(k);
        }
    } else if (!strcmp(cmd, "kkt_apply")) {
        kkt_handle *k = to_kkt(ARG(1));
        int64_t c, j;
        need_dense(ARG(2), k->N, "Z");
        c = (int64_t)mxGetN(ARG(2));
        plhs[0] = mxCreateDoubleMatrix((mwSize)k->N, (mwSize)c, mxREAL);
        for (j = 0; j < c && k->N > 0; j++)
            if ((st = cpk_kkt_apply(k->K, mxGetPr(ARG(2)) + j * k->N, mxGetPr(plhs[0]) + j * k->N))) fail(st);
    } else if (!strcmp(cmd, "kkt_residual")) {
        kkt_handle *k = to_kkt(ARG(1));
        const int64_t ld = k->N > 0 ? k->N : 1;
        int64_t c;
        mxArray *R, *sums;
        need_dense(ARG(2), k->N, "Z");
        need_dense(ARG(3), k->N, "B");
        c = (int64_t)mxGetN(ARG(2));
        if ((int64_t)mxGetN(ARG(3)) != c) fail_msg("cpk:dim", "B must have Z's %lld columns", (long long)c);
        R = mxCreateDoubleMatrix((mwSize)k->N, (mwSize)c, mxREAL);
        sums = mxCreateDoubleMatrix(4, (mwSize)c, mxREAL);
        /* MATLAB stores a dense matrix column-major: the leading dimensions are the row count */
        st = cpk_kkt_residual(k->K, c, mxGetPr(ARG(2)), ld, mxGetPr(ARG(3)), ld, mxGetPr(R), ld, mxGetPr(sums));
        if (st) fail(st);
        plhs[0] = R, plhs[1] = sums;
    } else if (!strcmp(cmd, "kkt_solve")) {
        kkt_handle *k = to_kkt(ARG(1));
        const int mid = method_id(ARG(2));
        cpk_pc M = to_pc(ARG(4));
        const int warm = ARG(6) && !mxIsEmpty(ARG(6));
        cpk_opts o;
        cpk_stats s;
        int64_t info[8];
        mxArray *x, *res;
        if ((st = cpk_kkt_get_info(k->K, info))) fail(st);
        if (!ARG(3) || mxIsSparse(ARG(3)) || (int64_t)mxGetNumberOfElements(ARG(3)) != k->N)
            fail_msg("cpk:dim", "b must have length %lld", (long long)k->N);
        if (warm && (mxIsSparse(ARG(6)) || (int64_t)mxGetNumberOfElements(ARG(6)) != k->N))
            fail_msg("cpk:dim", "x0 must have length %lld", (long long)k->N);
        to_opts(ARG(5), &o);
        alloc_hist(&s, mid, &o, info[0], info[1]);
        x = mxCreateDoubleMatrix((mwSize)k->N, 1, mxREAL);
        res = mxCreateDoubleMatrix(8, 1, mxREAL);
        if (warm && k->N) memcpy(mxGetPr(x), mxGetPr(ARG(6)), (size_t)k->N * sizeof(double));
        st = cpk_kkt_solve(k->K, mid, mxGetPr(ARG(3)), M, &o, mxGetPr(x), warm, &s, mxGetPr(res));
        if (st) fail(st);
        plhs[0] = x;
        put_stats(mid, &s, &plhs[1], &plhs[2]);
        plhs[3] = res;
        free_hist(&s);
    } else {
        fail_msg("cpk:args", "cpk_mex: unknown command %s", cmd);
    }
#undef ARG
    (void)nlhs;
}
