/*
 * cpk.h -- C ABI of libcpk, the MI355X-native constraint-preconditioned Krylov engine.
 *
 * Drop-in boundary for optimizers/cpkrylov (MATLAB).  Each entry point names the reference
 * interface it replaces; INTEGRATION.md shows the MEX gateway / opSpot subclass / ctypes
 * binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - Every function returns an int status (cpk_status).  On failure cpk_last_error()
 *     returns a message (thread-local, valid until the next call on that thread).
 *     No C++ exception crosses this boundary.
 *   - Input arrays are borrowed read-only for the duration of the call; the library
 *     copies what it keeps (to host memory and HBM).  Output arrays are caller-allocated.
 *   - Handles are owned by the library and freed by the matching *_destroy.
 *   - One host thread per context; a handle is not re-entrant.
 *   - All arithmetic is IEEE fp64.  Vectors are laid out [x-part (n); y-part (m)], as the
 *     reference's [x1; x2] (reg_cpkrylov.m:166-173).
 */
#ifndef CPK_H
#define CPK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPK_ABI_VERSION 3

typedef enum {
    CPK_OK = 0,
    CPK_ERR_INDEFINITE = 1, /* beta < -100*eps, or a negative squared norm (cpminres.m:195-199 etc.) */
    CPK_ERR_DIM = 2,        /* dimension mismatch (opLDL2.m:61-75) */
    CPK_ERR_ARGS = 3,       /* bad argument (reg_cpkrylov.m:122-125 "not enough inputs") */
    CPK_ERR_HIP = 4,        /* HIP runtime failure */
    CPK_ERR_RCCL = 5,       /* RCCL failure */
    CPK_ERR_FACTOR = 6,     /* the static-pivot LDL' (ldl at opLDL2.m:82) met a NaN pivot or, with the
                               engine option pivot_min = 0 (the default), a zero one; a finished
                               factor's signs are in cpk_pc_factor_report, never an error */
    CPK_ERR_NOMEM = 7,
    CPK_ERR_UNSUPPORTED = 8,
    CPK_ERR_CALLBACK = 9    /* the callback of an operator-valued A (cpk_op) returned nonzero */
} cpk_status;

/* Method ids: the function handles @cpcg, @cpcglanczos, @cpminres, @cpsymmlq, @cpgmres,
 * @cpdqgmres passed to reg_cpkrylov (reg_cpkrylov.m:67-68, :163). */
typedef enum {
    CPK_CG = 0,
    CPK_CGLANCZOS = 1,
    CPK_MINRES = 2,
    CPK_SYMMLQ = 3,
    CPK_GMRES = 4,
    CPK_DQGMRES = 5
} cpk_method;

/* The MATLAB `opts` struct.  A field takes effect only when its has_* flag is set
 * (MATLAB isfield(), e.g. cpminres.m:98-111); otherwise each solver's own default applies.
 * nitref/itref_tol/force_itref/residual_update are the fields reg_cpkrylov copies into M
 * (reg_cpkrylov.m:135-148), with opLDL2's setter semantics (opLDL2.m:97-115). */
typedef struct {
    double atol, rtol, btol;
    double itmax, restart, mem;
    double print;
    double nitref, itref_tol, force_itref, residual_update;
    int has_atol, has_rtol, has_btol, has_itmax, has_restart, has_mem, has_print;
    int has_nitref, has_itref_tol, has_force_itref, has_residual_update;
} cpk_opts;

/* stats / flag outputs (cpminres.m:250-252, cpsymmlq.m:363-367, cpcglanczos.m:311-325,
 * reg_cpkrylov.m:177-178).  History buffers are caller-allocated with capacity hist_cap
 * (itmax + 2 suffices for every method); a NULL buffer is skipped. */
typedef struct {
    int64_t niters;
    int solved;          /* flag.solved */
    int status;          /* cpcglanczos stats.status: 0 max iters, 1 residual small, 2 backward error small */
    double *hist;        /* residHistory (cpsymmlq: cgresidHistory) */
    double *hist_lq;     /* cpsymmlq lqresidHistory */
    double *hist_qr;     /* cpsymmlq qrresidHistory */
    int64_t hist_cap;
    int64_t hist_len, lq_len, qr_len;
    double ptime;        /* s, preconditioner setup (reg_cpkrylov.m:128-132) */
    double stime;        /* s, shift + method + recovery (reg_cpkrylov.m:150-175) */
    double loop_ms;      /* device time of the method call (HIP events on the solver stream) */
    double bytes_moved;  /* algorithmic HBM bytes of the method call (DESIGN.md section 5 model) */
} cpk_stats;

/* Factor summary of a preconditioner. */
typedef struct {
    int64_t n, m, N;
    int64_t nnz_kp;      /* nnz(Kp) */
    int64_t nnz_l;       /* nnz of the strict lower factor */
    int64_t nblocks;     /* SpTRSV work blocks */
    int64_t nrounds;     /* kernel launches per triangular sweep */
    int64_t max_block_levels;
    int64_t depth;       /* elimination-tree height */
    int64_t ordering;    /* 0 natural, 1 G-first + nested dissection, 2 G-first + minimum degree,
                            3 nested dissection, 4 minimum degree */
} cpk_pc_info;

typedef struct cpk_ctx_s *cpk_ctx;
typedef struct cpk_mat_s *cpk_mat;
typedef struct cpk_pc_s *cpk_pc;

const char *cpk_last_error(void);
int cpk_abi_version(void);

/* ---- context: device, streams, RCCL communicator ------------------------------------- */
/* Fill `id` (128 bytes) with an RCCL unique id on rank 0; broadcast it to the other ranks. */
int cpk_get_unique_id(unsigned char id[128]);
/* device < 0: use the current device.  nranks == 1 and unique_id == NULL: no communicator.
 * nranks > 1 requires a unique_id and runs the distributed path over RCCL.  A 1-rank RCCL
 * communicator (a torchrun world of one) has nothing to exchange: it runs the single-GPU path
 * unless engine option dist1 is set before the operators are built. */
int cpk_ctx_create(int device, int rank, int nranks, const unsigned char *unique_id, cpk_ctx *out);
/* Diagnostic timing stand-in (no reference counterpart): rank `rank` of an nranks-way
 * distributed context WITHOUT peers.  Every collective is a no-op (an allgather copies the
 * rank's own slot), so results are meaningless, but each kernel is exactly that rank's share of
 * the P-way solve: tools/dist_timing.py times one rank's work on one GPU with it.  Never used by
 * cpk_ctx_create; nranks must be > 1. */
int cpk_ctx_create_null(int device, int rank, int nranks, cpk_ctx *out);
/* Communicator kinds reported by cpk_ctx_get_info. */
enum { CPK_COMM_NONE = 0, CPK_COMM_RCCL = 1, CPK_COMM_SIM = 2, CPK_COMM_NULL = 3 };
/* info[8] = {device, rank, nranks, communicator kind (CPK_COMM_*), ranks the communicator holds
 * (RCCL: ncclCommCount; SimComm: the group's ranks; the timing stand-in: 1; none: 0),
 * distributed path (0/1), 0, 0}. */
int cpk_ctx_get_info(cpk_ctx ctx, int64_t *info);
/* Single-GPU rehearsal of the distributed path: `nranks` ranks as host threads of one process,
 * all on one device, exchanging through a shared HBM buffer instead of RCCL (RCCL refuses two
 * ranks on one GPU).  Each thread creates its context with cpk_ctx_create_sim and then makes
 * the same collective calls as an RCCL rank.  For tests; no hipGraph capture. */
typedef struct cpk_simgroup_s *cpk_simgroup;
int cpk_simgroup_create(int nranks, cpk_simgroup *out);
int cpk_simgroup_destroy(cpk_simgroup g);
int cpk_ctx_create_sim(int device, cpk_simgroup group, int rank, int nranks, cpk_ctx *out);
/* Engine options of a context (no reference counterpart: they choose among execution paths
 * that give identical results, and the sweep schedule / distributed split that every rank
 * must build identically).  A context starts from the CPK_<NAME> environment variables, read
 * once at creation; a change applies to preconditioners and solves created afterwards.
 * Names: sweep ("rows,cap,threads[,rows,cap,threads[,sub0]]"; unset, each path has its own
 * default: a distributed context reports and uses the distributed one), split_tol, pivot_min
 * (delta, a finite number >= 0, default 0 = off: a pivot of the LDL' whose expected sign s gives
 * s * d < delta is replaced by s * delta, see cpk_pc_factor_report; with exact_dots and
 * basis_f32 one of the three options that change results; read at every cpk_pc_create[_hint], cpk_pc_refactor and
 * cpk_analyze), host_factor,
 * no_pipe, no_upper, no_col16, no_dataflow, all_dataflow, no_colsweep, all_colsweep, no_rowspan, all_rowspan
 * (the upper rounds' row-span level loop: never / on every eligible block instead of where the host
 * model picks it; all_rowspan goes before all_dataflow and all_colsweep, which otherwise keep
 * their loop on every block they force), no_chain, chain_wide
 * (rounds of at most this many blocks join the sweep chain, default 256), round_caps (per-round block
 * caps above round 1, single GPU with the default sweep: 0 uniform caps, 1 (default) the largest cap
 * whose blocks stay resident, N > 1 every such round at N entries), exact_dots, no_bcast_analysis
 * (every rank of a distributed preconditioner runs the global analysis instead of receiving rank 0's),
 * apply_multi_panel (cpk_pc_apply_multi always on its panel kernels; set before building operators),
 * no_sched_resid, no_fused_resid, r0_xcd_chunk, tsolve_global, tsolve_sweep,
 * no_piggy, no_halo_merge, no_graph, no_fuse_last, no_tkr, no_minres_fuse, dist_graph, batch,
 * dist1 (a 1-rank communicator runs the distributed kernels; set before building operators),
 * profile_fwd_sched (diagnostic), sweep_set ("0" returns sweep to the per-path default),
 * profile_passes (diagnostic: cpdqgmres runs eagerly with events between its passes, read by
 * cpk_debug_pass_times), fail_inject ("rank:site[:n]", site setup / batch / chain: a test hook
 * that makes one rank of a distributed solve fail at that point).
 * basis_f32 ("0"/"1", default 0, environment CPK_BASIS_F32; read at every solve; with exact_dots and
 * pivot_min the third option that changes results): cpgmres and cpdqgmres keep their rings (V, and PV
 * for cpdqgmres) as float arrays, slots padded to 64 floats.  One rule defines every bit.  A basis
 * vector [V(:,j); Q(:,j)] or a direction [PV(:,j); PQ(:,j)] is built and normalised in double, as
 * without the option, and its final value is rounded ONCE to float (IEEE round to nearest even,
 * subnormals kept, beyond the float range +-inf) when it is stored in its ring slot.  Every read of a
 * ring slot converts the float exactly to double: the window sums, the orthogonalisation, the
 * Q(:,k+1) = Q(:,k) - w recurrence, the direction recurrence, cpgmres's update of x and y, and the
 * vector the Krylov product multiplies.  The vector under construction stays in double, so
 * H(k+1,k) = sqrt(<u, vnew> + <t, qnew>) is taken on the unrounded vector (a stored vector's
 * form-norm is 1 to about 2^-24 only), and cpdqgmres updates x and y with the unrounded direction.
 * Rotations, SymGivens, g, the stop tests, the histories and the errors are unchanged.  The rounding
 * of the basis reaches H(k+1,k)^2: where that is rounding noise (a residual that collapses in a step)
 * its sign is arbitrary at 2^-24 instead of 2^-53 and the methods stop with CPK_ERR_INDEFINITE more
 * often (DESIGN.md "Compressed basis").  The other four methods, the block solves and the
 * preconditioner do not see the option.  On a distributed context or preconditioner cpgmres and
 * cpdqgmres answer CPK_ERR_UNSUPPORTED before anything is written while it is set.
 * Booleans as "0"/"1".  A distributed preconditioner allgathers a hash of its plan and of every
 * option but fail_inject at creation and fails (CPK_ERR_ARGS) on every rank unless all ranks
 * agree. */
int cpk_ctx_set_option(cpk_ctx ctx, const char *name, const char *value);
int cpk_ctx_get_option(cpk_ctx ctx, const char *name, char *buf, size_t cap);
/* Every engine option of the context as "name=value;name=value;..." (the form cpk_analyze's
 * `options` takes), with the sweep this context's path uses. */
int cpk_ctx_get_options(cpk_ctx ctx, char *buf, size_t cap);
int cpk_ctx_destroy(cpk_ctx ctx);
int cpk_ctx_synchronize(cpk_ctx ctx);

/* ---- sparse matrices (MATLAB sparse arrays A, B, C, G; reg_cpkrylov.m:1) -------------- */
/* MATLAB-native CSC: jc[ncols+1], ir[nnz] (0-based, mwIndex = size_t), pr[nnz].
 * ctx may be NULL for a host-only matrix (cpk_analyze); such a matrix cannot be used on a device. */
int cpk_mat_create_csc(cpk_ctx ctx, int64_t nrows, int64_t ncols, const size_t *jc, const size_t *ir,
                       const double *pr, cpk_mat *out);
/* CSR with 64-bit row pointers and 32-bit column indices. */
int cpk_mat_create_csr(cpk_ctx ctx, int64_t nrows, int64_t ncols, const int64_t *rowptr,
                       const int32_t *colind, const double *val, cpk_mat *out);
int cpk_mat_destroy(cpk_mat A);
/* y = A*x on the device (host vectors in/out); replaces MATLAB sparse mtimes A*v. */
int cpk_mat_spmv(cpk_mat A, const double *x, double *y);
/* The same on device vectors: the product is enqueued on the context stream and nothing is waited
 * for.  The same kernel on the same row blocks as cpk_mat_spmv, so the same bits.  Legal while
 * the context stream is capturing, once the handle has its device copy: the first device use of a
 * handle uploads it, so make one call (or any solve with the handle) before relying on that.  This
 * is how a C caller writes a cpk_op callback out of the library's own SpMV. */
int cpk_mat_spmv_device(cpk_mat A, const double *d_x, double *d_y);
/* New values with the same sparsity, written into the handle (an interior-point outer iteration:
 * reg_cpkrylov.m:131 rebuilds opLDL2 from new values once per outer iteration).  val holds the
 * values in the order of the creating call's value array -- pr of cpk_mat_create_csc, val of
 * cpk_mat_create_csr, entry 0 being the first entry that call read (pr[jc[0]], val[rowptr[0]]) --
 * and count is the number of entries it read.  Afterwards A equals, bit for bit, the matrix the
 * creating call would build from the same index arrays and val (the same column sort, duplicates
 * summed left to right).  Everything that hangs off the handle stays valid and sees the new
 * values at its next use: the device copy, the Krylov operators blkdiag(A, C) cached on it, the
 * solvers cached by a preconditioner with their captured graphs.  A preconditioner built or
 * refactored from A keeps its own copies: it changes at its next cpk_pc_refactor.  Works on a
 * host-only matrix.  count == 0 with val == NULL is fine.
 * Errors, all leaving A as it was: CPK_ERR_ARGS for a NULL handle or NULL val with count > 0,
 * CPK_ERR_DIM when count differs from the creating call's entry count, CPK_ERR_UNSUPPORTED on a
 * distributed context. */
int cpk_mat_set_values(cpk_mat A, const double *val, int64_t count);
/* The same from device memory, with no host round trip of the values (CPK_ERR_ARGS on a host-only
 * matrix).  d_val must be complete when the call is made (synchronise the stream that wrote it);
 * the call blocks: on return d_val may be overwritten or freed.  The handle's host copy is
 * downloaded again when a host-side reader next needs it (cpk_pc_create, cpk_analyze, the first
 * blkdiag(A, C) of a pairing). */
int cpk_mat_set_values_device(cpk_mat A, const double *d_val, int64_t count);
/* A sum of k outer products sampled on A's sparsity, handed back in the creating call's value
 * order: the transpose of cpk_mat_set_values (a gradient with respect to the values that call
 * takes).  For every stored entry q = (i, j) of the canonical matrix
 *     g_q = alpha * (U(i,0)*V(j,0) + U(i,1)*V(j,1) + ... + U(i,k-1)*V(j,k-1)),
 * the sum from 0.0 over the separately rounded products in column order (no FMA), alpha applied
 * last with one rounding; k == 0 gives alpha*0.0.  U is nrows x k and V is ncols x k, column-major
 * with ldu >= nrows, ldv >= ncols.  out has count entries, count as for cpk_mat_set_values: entry e
 * receives the g_q of the stored entry it went into, so the entries that were summed into one
 * stored entry all receive that entry's g_q (the derivative of a sum with respect to each summand
 * is 1).  Every entry of out is written exactly once, without atomics: the result is
 * deterministic.  A's values are not read.  The work is done on the device in both variants.
 * Refused before anything is written: a NULL handle, NULL out with count > 0, NULL U or V with
 * k > 0 (CPK_ERR_ARGS); count differing from the creating call's, k < 0 or a short leading dimension
 * (CPK_ERR_DIM); a host-only matrix (CPK_ERR_ARGS); a distributed context (CPK_ERR_UNSUPPORTED).
 * _device: device arrays, enqueued on the context stream; nothing is waited for. */
int cpk_mat_sample_outer(cpk_mat A, int64_t k, const double *U, int64_t ldu, const double *V, int64_t ldv, double alpha,
                         double *out, int64_t count);
int cpk_mat_sample_outer_device(cpk_mat A, int64_t k, const double *d_U, int64_t ldu, const double *d_V, int64_t ldv,
                                double alpha, double *d_out, int64_t count);
/* Diagnostic: info[8] = {nrows, ncols, stored entries, entry count of the creating call, values
 * generation (0 at creation, +1 per successful set), device copy present, Krylov operators
 * cached on this handle, 0}. */
int cpk_mat_get_info(cpk_mat A, int64_t info[8]);

/* ---- preconditioner: M = opLDL2(A, B, C), Kp = [A B'; B C] (ops/opLDL2.m:60-92) ------
 * Distributed contexts (nranks > 1): every rank passes the same global matrices; the library
 * partitions rows by the elimination tree.  Host-vector entry points
 * then take and return GLOBAL vectors on every rank; device-vector entry points take the
 * rank's LOCAL slice in the order cpk_pc_local_dofs reports ([x-part; y-part]). */
int cpk_pc_create(cpk_ctx ctx, cpk_mat A11, cpk_mat B, cpk_mat C22, double *ptime, cpk_pc *out);
/* cpk_pc_create with the Krylov operator's A (n x n) as a placement hint for a distributed
 * context: rows the factor leaves isolated are owned with the dofs A couples them with, so the
 * Krylov SpMV's halo stays small.  reg_cpkrylov (cpk_reg_solve) passes its A itself.  On one
 * GPU identical to cpk_pc_create; Akry may be NULL. */
int cpk_pc_create_hint(cpk_ctx ctx, cpk_mat A11, cpk_mat B, cpk_mat C22, cpk_mat Akry, double *ptime,
                       cpk_pc *out);
int cpk_pc_destroy(cpk_pc M);
/* Refactorization with new values and the same sparsity: opLDL2(G, B, C) rebuilt in an
 * interior-point outer loop (the constructor, opLDL2.m:60-92, called per outer iteration
 * through reg_cpkrylov.m:131).  Kp and the numeric LDL' (opLDL2.m:81-82) are recomputed on
 * the device from the matrices' device copies; ordering, elimination tree and sweep schedule
 * are reused.  The factors equal those of a fresh cpk_pc_create on the same values, bit for
 * bit.  CPK_ERR_ARGS when the sparsity differs, CPK_ERR_FACTOR on a bad pivot (the previous
 * factors, pivot shifts and report then stay).
 * ptime: seconds of the refactorization. */
int cpk_pc_refactor(cpk_pc M, cpk_mat A11, cpk_mat B, cpk_mat C22, double *ptime);
/* M.nitref = ...; M.itref_tol = ...; etc. (opLDL2.m:45-50, 97-115), has_* fields select. */
int cpk_pc_set(cpk_pc M, const cpk_opts *opts);
int cpk_pc_get(cpk_pc M, double *nitref, double *itref_tol, double *force_itref, double *residual_update);
/* Opt-in (not in the reference): handle semantics of the residual-update state.  In the
 * reference, opLDL2 is a Spot value object, so the op.Aty / op.Cy written inside multiply
 * (opLDL2.m:169-171) are lost and residual_update is a functional no-op; cpk_pc_apply matches
 * that by default.  on != 0 keeps [op.Aty; op.Cy] on the device between applies, as the
 * residual update of reg_cpkrylov.m:47-52 (Gould-Hribar-Nocedal) intends; it takes effect while
 * residual_update is set.  Enabling or disabling clears the state.  Single-GPU contexts only
 * (CPK_ERR_UNSUPPORTED on a distributed preconditioner). */
int cpk_pc_set_handle(cpk_pc M, int on);
/* y = M*x (opLDL2.multiply, opLDL2.m:161-188).  Host vectors of length N. */
int cpk_pc_apply(cpk_pc M, const double *x, double *y);
/* Same on device pointers, enqueued on the context stream. */
int cpk_pc_apply_device(cpk_pc M, const double *d_x, double *d_y);
/* y = M'*x = conj(M)*x: the bare factor composite P*L'^-1*D^-1*L^-1*P' (opLDL2.m:127-136), one
 * LDL solve on the device factors.  Unlike cpk_pc_apply it runs no refinement and no residual
 * update: nitref, itref_tol, force_itref, residual_update and the handle-mode state are neither
 * read nor written.  Host vectors of length N (global on a distributed preconditioner). */
int cpk_pc_apply_ldl(cpk_pc M, const double *x, double *y);
/* Same on device pointers (a distributed preconditioner: the rank's local slice). */
int cpk_pc_apply_ldl_device(cpk_pc M, const double *d_x, double *d_y);
/* Y = M'*X for a block of k right-hand sides (the reference's M' * X with an N x k matrix):
 * column-major, column j at X + j*ldx and Y + j*ldy, ldx, ldy >= N and k >= 0 (CPK_ERR_DIM
 * otherwise; k == 0 does nothing).  X and Y must not overlap (not checked).  The columns are
 * solved in panels of 8 by a sweep that streams L once per panel; column j of Y equals
 * cpk_pc_apply_ldl on column j of X bit for bit.  Rows [N, ldy) of Y are not touched.  Single GPU
 * (CPK_ERR_UNSUPPORTED on a distributed preconditioner). */
int cpk_pc_apply_ldl_multi(cpk_pc M, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy);
int cpk_pc_apply_ldl_multi_device(cpk_pc M, int64_t k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy);
/* Diagnostic (not in the reference): the multi-column sweep as the preconditioner's last or next
 * panel solve runs it, info[4] = {columns per panel, kernel launches per panel solve, blocks
 * staged in LDS, blocks on the direct path through global memory} (multi-column sweep). */
int cpk_pc_multi_info(cpk_pc M, int64_t *info);
/* Diagnostic: info[4] = {cached single-column solvers, hipGraph instantiations those made so far,
 * cached block solvers, their instantiations}: a solve that replays cached graphs leaves the
 * instantiation counts as they were. */
int cpk_pc_solver_info(cpk_pc M, int64_t info[4]);
/* Y = M*X for a block of k right-hand sides, DEFINED column by column: column j of Y is what
 * cpk_pc_apply returns for column j of X under the current nitref, itref_tol and force_itref, bit
 * for bit -- the reference's double(op), one op*e per column (opLDL2.m:138-149).  (The reference's
 * own matrix path, multiply on an N x k argument, takes norm(r) as a matrix 2-norm and x(1:n) as
 * a linear index; it is not reproduced.)  Each column runs the loop of opLDL2.m:174-185 with its
 * own predicate: columns of one panel stop refining at different steps, and a column that
 * stopped is not touched again.  Layout and checks as cpk_pc_apply_ldl_multi: column-major,
 * ldx, ldy >= N and k >= 0 (CPK_ERR_DIM otherwise; k == 0 does nothing); rows [N, ldy) of Y are
 * not touched; X and Y may not overlap (CPK_ERR_ARGS).  nit (may be NULL) receives k counts, the
 * refinement solves each column took, 0...nitref; in the device form d_nit is a device pointer.
 * The columns go in panels of 8 through kernels that stream the factor twice per solve and Kp
 * once per residual for the whole panel; a panel below the measured break-even (DESIGN.md
 * section 5, the refined block apply) runs as a loop of single-column applies unless the engine
 * option apply_multi_panel forces the panel kernels -- the bits are the same either way.  The
 * predicate's norms are plain sums in a fixed order (also under exact_dots), so the block apply
 * is deterministic from run to run; their last bits may differ from cpk_pc_apply's, which can
 * matter only at an exact tie ||r|| == itref_tol*||x||.  Single GPU (CPK_ERR_UNSUPPORTED on a
 * distributed preconditioner), and CPK_ERR_UNSUPPORTED, the state untouched, while the handle
 * semantics of residual_update are in effect (cpk_pc_set_handle with residual_update set: one
 * state vector). */
int cpk_pc_apply_multi(cpk_pc M, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, int32_t *nit);
int cpk_pc_apply_multi_device(cpk_pc M, int64_t k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy,
                              int32_t *d_nit);
/* x = Kp*b (opLDL2.divide, opLDL2.m:193-195). */
int cpk_pc_divide(cpk_pc M, const double *b, double *x);
int cpk_pc_get_info(cpk_pc M, cpk_pc_info *info);
/* Local slice of a (distributed) preconditioner: n_loc x-part and m_loc y-part dofs; dofs[i] =
 * global index of local entry i (n_loc + m_loc entries).  One GPU: the identity. */
/* Diagnostic (not in the reference): the separator solve of a distributed preconditioner,
 * info[12] = {distributed, separator rows, levels, step records, LDS bytes with the records
 * staged (0: they do not fit), LDS bytes with the records left in HBM, payload per rank,
 * refinement residual without the Kp halo exchange, refinement in schedule order, its residual
 * fused into the forward sweep, separator solved by the block sweeps (T sweep), the T sweep's
 * rounds}. */
int cpk_pc_sep_info(cpk_pc M, int64_t *info);
/* Diagnostic (not in the reference): the sweep schedule as launched, info[8] = {rounds, round-0
 * blocks, blocks above round 0, grid of the cost-balanced round-0 assignment of the forward /
 * fused-residual forward / backward kernel (0: the launch strides), round 0 persistent, tasks of
 * the sweep chain (every upper round of a solve in one launch; 0: one launch per round)}. */
int cpk_pc_sweep_info(cpk_pc M, int64_t *info);
int cpk_pc_local_dofs(cpk_pc M, int64_t *n_loc, int64_t *m_loc, int32_t *dofs);
/* Export the factors P'*Kp*P = L*D*L': strict-lower L in CSC (Lcolptr[N+1], Lrowind[nnz_l],
 * Lval[nnz_l]), D[N], perm[N] (perm[k] = original index of pivot k).  Any pointer may be NULL. */
int cpk_pc_export(cpk_pc M, int64_t *Lcolptr, int32_t *Lrowind, double *Lval, double *D, int32_t *perm);
/* What the last successful factorization (create or refactor) found.  Stands in for the inertia
 * and pivot information MA57's ldl returns with the factors at opLDL2.m:81-82.  Positions are
 * pivot positions: the index into the exported D and perm, the numbering of CPK_ERR_FACTOR's
 * message.  s_k = +1 where perm[k] < n (a dof of the (1,1) block), -1 otherwise: the pivot signs
 * of a symmetric quasi-definite Kp under any symmetric ordering.
 * Engine option pivot_min = delta > 0: a pivot d with s_k * d < delta is replaced by
 * d' = s_k * delta and E_k = d' - d recorded, so the factors are those of Kp + P*diag(E)*P'
 * exactly; Kp itself (the refinement residual, divide, the solvers) stays the unperturbed matrix,
 * and iterative refinement (nitref, force_itref) corrects towards it.  A refactorization that
 * fails leaves the previous factors, shifts and report in place. */
typedef struct {
    int64_t n_pos, n_neg;      /* signs of D = inertia of the factored matrix (Sylvester) */
    int64_t n_wrong;           /* pivots with s_k * d < 0 */
    int64_t first_wrong;       /* lowest such pivot position, -1 if none */
    int64_t n_perturbed;       /* pivots replaced under pivot_min */
    int64_t argmin_abs;        /* position of min |d|, lowest on ties; -1 if N == 0 */
    double  min_abs, max_abs;  /* over D */
    double  max_shift;         /* max |E_k| */
    double  pivot_min;         /* the value in effect at this factorization */
} cpk_factor_report;
int cpk_pc_factor_report(cpk_pc M, cpk_factor_report *out);
/* The pivot shifts of that factorization (the perturbation MA57's pivoting makes unnecessary at
 * opLDL2.m:81-82): N values in the ORIGINAL dof order, E[perm[k]] = E_k; zeros when none.  On a
 * distributed preconditioner N is the global size and every rank holds the same values. */
int cpk_pc_pivot_shift(cpk_pc M, double *E);

/* ---- host-only analysis (no GPU needed) ------------------------------------------------- */
/* The host half of cpk_pc_create: Kp assembly, fill-reducing ordering, static-pivot LDL' and
 * the triangular-sweep schedule.  Matrices for this call may be created with ctx == NULL.
 * Engine options: the CPK_<NAME> environment (as a new context starts), then `options`
 * ("name=value;...", NULL: none) on top -- pass cpk_ctx_get_options of a context to analyse
 * and plan exactly as that context's preconditioner would (sweep, split_tol). */
typedef struct cpk_analysis_s *cpk_analysis;
int cpk_analyze(cpk_mat A11, cpk_mat B, cpk_mat C22, const char *options, cpk_analysis *out);
int cpk_analysis_destroy(cpk_analysis an);
int cpk_analysis_get_info(cpk_analysis an, cpk_pc_info *info);
int cpk_analysis_export(cpk_analysis an, int64_t *Lcolptr, int32_t *Lrowind, double *Lval, double *D,
                        int32_t *perm);
/* cpk_pc_factor_report / cpk_pc_pivot_shift of the host numeric phase (the inertia and pivot
 * information of MA57's ldl, opLDL2.m:81-82): equal to the device's, bit for bit. */
int cpk_analysis_factor_report(cpk_analysis an, cpk_factor_report *out);
int cpk_analysis_pivot_shift(cpk_analysis an, double *E);
/* Sweep schedule: round_ptr[nrounds+1] (blocks per round), blk_lvl[nblocks+1] (levels per
 * block, indices into lvl_row), lvl_row[nlevels+1] (first position of each level; last = N),
 * order[N] (order[q] = exported-factor row solved at schedule position q).  Each row sums its
 * entries in the exported factor's order: forward by ascending column, backward by
 * descending row -- the order of the reference's column-oriented solves. */
int cpk_analysis_schedule(cpk_analysis an, int64_t *nlevels, int64_t *round_ptr, int64_t *blk_lvl,
                          int64_t *lvl_row, int32_t *order);
/* The caps each round's blocks were built for (engine option round_caps): cap[nrounds] entries of
 * either direction, rows[nrounds] rows per block.  A schedule with uniform caps reports the sweep
 * option's: round 0's pair, then the upper rounds' for every other round. */
int cpk_analysis_round_caps(cpk_analysis an, int32_t *cap, int32_t *rows);

/* ---- distributed plan (host-only) --------------------------------- */
/* The row-block plan of rank `rank` out of `nranks` for the system the analysis was built on
 * (A: n x n, C: m x m the Krylov operator's blocks), with the analysis' engine options
 * (split_tol).  Every rank computes the same global plan deterministically; a distributed
 * cpk_pc_create on a context with the same options builds exactly this.  Exposed for tests and
 * inspection: cpk_plan_array(plan, name, &count, out) copies array `name` (values as double
 * for *_val, fsub_Lx, fsub_D, extra_val, tf_val, tb_val, DT; every other array as int64) into
 * out (NULL: count only).  Names: sizes [P, rank, n, m, N, n_loc, m_loc, N_loc, nsub, nT, kt,
 * kp_kmax, ac_kmax, ab_kmax], dofs, node_rank, T, fsub_{Lp,Li,Lx,D,perm,parent,key},
 * extra_{ptr,col,key,val}, tf_{ptr,col,val,src}, tb_{ptr,col,val}, DT, tlev_{ptr,rows},
 * tsend, tdof, and {kp,ac,ab}_{ptr,col,val,send} for Kp, blkdiag(A,C) and [A B']. */
typedef struct cpk_plan_s *cpk_plan;
int cpk_analysis_plan(cpk_analysis an, cpk_mat A, cpk_mat C, int nranks, int rank, cpk_plan *out);
/* Host-only: the row-span layout (the upper rounds' fourth level loop) of
 * schedule block `block` and direction `dir` (0 forward, 1 backward), so it can be replayed
 * without a GPU.  The layout routine is the device's; the rows' entry order is restated here
 * (single-GPU factor, no entries outside it) and each call scans the factor: for test sizes.  cap_entries: the staged image's entry capacity (<= 0:
 * the schedule's).  info->eligible = 0: the loop refuses the block (more than 128 rows, the rows'
 * in-block terms not at increasing steps before their own, a run over 255 terms, over capacity);
 * the rows and steps are exported all the same.  Any array pointer may be NULL.  The block's rows
 * r0 .. r0 + nr - 1 (relabelled factor): rowptr[nr + 1] into col / val / dest[ne] in the device's
 * entry order (col: relabelled row indices); step[nr] the row's step; lead[nr] its first lead
 * slot; by step: mask[2 nr] (bit t of the pair: an in-block term at step t), base, first, run0[nr];
 * tab[ndr * nrp]: the run length of the row of step s behind its term of the d-th drain step at
 * tab[d * nrp + s]; info->dset: the drain steps. */
typedef struct {
    int64_t eligible, r0, nr, ne, slots, ndr, nrp, trips;
    uint64_t dset[2];
} cpk_rowspan_info;
int cpk_analysis_rowspan(cpk_analysis an, int64_t block, int dir, int64_t cap_entries, cpk_rowspan_info *info,
                         int64_t *rowptr, int32_t *col, double *val, int32_t *dest, int32_t *step, int32_t *lead,
                         uint64_t *mask, int32_t *base, int32_t *first, int32_t *run0, uint8_t *tab);
int cpk_plan_array(cpk_plan plan, const char *name, int64_t *count, void *out);
int cpk_plan_destroy(cpk_plan plan);

/* ---- solvers --------------------------------------------------------------------------- */
/* [x, y, stats, flag] = method(b, A, C, M, opts)   (kernels/cp*.m, e.g. cpminres.m:1).
 * b: n, x: n, y: m (host).  CPK_GMRES with ceil(itmax/restart) < 1 (itmax <= 0) is CPK_ERR_ARGS:
 * the reference's outer loop never runs and cpgmres.m:267 reads a k that was never assigned. */
int cpk_method_solve(cpk_ctx ctx, int method, const double *b, cpk_mat A, cpk_mat C, cpk_pc M,
                     const cpk_opts *opts, double *x, double *y, cpk_stats *stats);
/* Same with device-resident b (n) and xy (N = [x; y]); nothing crosses PCIe except the
 * stop flag polled between iteration batches and the history copied back at the end. */
int cpk_method_solve_device(cpk_ctx ctx, int method, const double *d_b, cpk_mat A, cpk_mat C, cpk_pc M,
                            const cpk_opts *opts, double *d_xy, cpk_stats *stats);
/* [x, stats, flag] = reg_cpkrylov(method, b, A, B, C, G, opts)  (reg_cpkrylov.m:1-180).
 * b: N, x: N (host).  If M_out != NULL the preconditioner built here is returned. */
int cpk_reg_solve(cpk_ctx ctx, int method, const double *b, cpk_mat A, cpk_mat B, cpk_mat C, cpk_mat G,
                  const cpk_opts *opts, double *x, cpk_stats *stats, cpk_pc *M_out);
/* reg_cpkrylov's shift + method + recovery with an existing M, device-resident b and x (N). */
int cpk_reg_solve_device(cpk_ctx ctx, int method, const double *d_b, cpk_mat A, cpk_mat B, cpk_mat C,
                         cpk_pc M, const cpk_opts *opts, double *d_x, cpk_stats *stats);

/* ---- the operator-valued A: the (1,1) block as a device callback ---------------------------- */
/* reg_cpkrylov.m:40 and the header of every kernel (cpcg.m:44, cpminres.m:40, ...): A may be a
 * matrix or a linear operator; only B, C and G must be matrices, since only they are factorized.
 * A cpk_op is that operator: y(0:n) = A*x(0:n) on device memory, all work enqueued on `stream`
 * (the context's hipStream_t).  Returns 0, or nonzero to abort the solve.
 *
 * The contract of fn:
 *  - fn writes y[0:n) and touches nothing else.  In the per-iteration product x and y are two
 *    buffers of the cached solver whose addresses stay fixed for that solver's life (the solver
 *    copies the current Krylov vector into x first); the one product of reg_cpkrylov's shift and
 *    cpk_op_apply_device pass the buffers of that call.
 *  - A capturable op (CPK_OP_CAPTURABLE) may be called while the stream is capturing.  It must
 *    only enqueue on `stream`: no synchronisation, no allocation, no other stream.  What it
 *    enqueues may depend only on its arguments and on device memory contents, never on host state
 *    at call time: fn is then called at capture time, once per captured iteration, and replays of
 *    the graph do not call it.  The iterations run in the usual captured batches.
 *  - A non-capturable op (the default) is called eagerly, once per product, and may do anything
 *    on `stream` (a torch computation, its own synchronisation).  Its solver runs batches of one
 *    iteration without graphs, so fn is never called for an iteration that has already stopped
 *    and cpk_op_get_info's call count is exact: one per iteration, one for cpsymmlq's pre-step,
 *    one per cpgmres restart, one for reg_cpkrylov's shift when b(n+1:N) is not zero.
 *  - A nonzero return aborts the solve with CPK_ERR_CALLBACK; the message names the call count.
 *    An open capture is ended and its graph discarded before the error propagates.  The outputs
 *    are unspecified; every handle stays usable.
 *  - A's symmetry is the caller's responsibility, as it is in the reference.
 * An operator solve of cpminres runs the unfused update (engine option no_minres_fuse's sequence:
 * the same bits).  u = fn's output bit for bit; t = C*q row sums in column order from 0.0 as in
 * the matrix path; <u, v> and <t, q> are fixed-order sums, deterministic per build and device,
 * and the correctly rounded exact sums under engine option exact_dots.
 * stats->bytes_moved counts 12 nnz(C) + 4 (N+1) + 16 N + 24 n for the product (the 24 n: the copy
 * of the Krylov vector to fn's input and the read of fn's output); fn's own traffic is unknown and
 * NOT counted.
 * Block solves, cpk_kkt and distributed contexts stay matrix-only.  THE OP MUST OUTLIVE THE
 * PRECONDITIONERS IT WAS SOLVED WITH, OR THEIR LAST USE. */
typedef int (*cpk_op_fn)(void *user, const double *d_x, double *d_y, int64_t n, void *stream);
typedef struct cpk_op_s *cpk_op;
#define CPK_OP_CAPTURABLE 1
/* n >= 0 (CPK_ERR_DIM); flags: 0 or CPK_OP_CAPTURABLE (CPK_ERR_ARGS otherwise).  A NULL fn makes a
 * handle that every solve and cpk_op_apply_device refuse (CPK_ERR_ARGS). */
int cpk_op_create(cpk_ctx ctx, int64_t n, cpk_op_fn fn, void *user, int flags, cpk_op *out);
int cpk_op_destroy(cpk_op A);
/* info: n, flags, calls of fn so far, calls that returned nonzero */
int cpk_op_get_info(cpk_op A, int64_t info[4]);
/* one call of fn on the context stream (d_x, d_y: n values each); nothing is waited for */
int cpk_op_apply_device(cpk_op A, const double *d_x, double *d_y);
/* cpk_method_solve / cpk_method_solve_device with the operator A.  Refused before anything is
 * written: a distributed context or preconditioner (CPK_ERR_UNSUPPORTED), an n that differs from
 * M's or a C that does not fit (CPK_ERR_DIM), a NULL fn or handle (CPK_ERR_ARGS). */
int cpk_method_solve_op(cpk_ctx ctx, int method, const double *b, cpk_op A, cpk_mat C, cpk_pc M, const cpk_opts *opts,
                        double *x, double *y, cpk_stats *stats);
int cpk_method_solve_op_device(cpk_ctx ctx, int method, const double *d_b, cpk_op A, cpk_mat C, cpk_pc M,
                               const cpk_opts *opts, double *d_xy, cpk_stats *stats);
/* reg_cpkrylov's shift + method + recovery with the operator A and an existing M (as
 * cpk_reg_solve_device): host b and x (N), or device-resident ones.  The same refusals. */
int cpk_reg_solve_op(cpk_ctx ctx, int method, const double *b, cpk_op A, cpk_mat B, cpk_mat C, cpk_pc M,
                     const cpk_opts *opts, double *x, cpk_stats *stats);
int cpk_reg_solve_op_device(cpk_ctx ctx, int method, const double *d_b, cpk_op A, cpk_mat B, cpk_mat C, cpk_pc M,
                            const cpk_opts *opts, double *d_x, cpk_stats *stats);

/* ---- the saddle-point operator itself: product, true residual, verified solve ------------ */
/* K = [A B'; B -C], the matrix of the system reg_cpkrylov solves (reg_cpkrylov.m:1-40): A, B, C
 * are the handles the solvers take, C the positive block, so K holds -C; A may be nonsymmetric
 * and the (1,1) block is A as given.  Row i < n is A's row followed by B''s entries by ascending
 * constraint, row n + i is B's row followed by -C's row (opLDL2.m:81's assembly).  Dimension
 * errors are opLDL2's (CPK_ERR_DIM, opLDL2.m:61-75, same messages); a distributed context is
 * refused with CPK_ERR_UNSUPPORTED, as cpk_mat_set_values is.
 * K follows the handles' values: at each use, if cpk_mat_set_values[_device] moved a handle's
 * values generation, one device pass regathers K's value array from the handles' device values
 * (the array keeps its address; nothing goes through the host).  THE THREE HANDLES MUST OUTLIVE K.
 * cpk_kkt_get_info: {n, m, nnz(K), the values generations of A, B, C that K holds, the number of
 * regather passes so far, the device address of K's value array}. */
typedef struct cpk_kkt_s *cpk_kkt;
int cpk_kkt_create(cpk_ctx ctx, cpk_mat A, cpk_mat B, cpk_mat C, cpk_kkt *out);
int cpk_kkt_destroy(cpk_kkt K);
int cpk_kkt_get_info(cpk_kkt K, int64_t info[8]);
/* y = K*z (N = n + m entries each): y_i = s_i, where the row sum s_i starts at 0.0 and adds the
 * separately rounded products K_ij*z_j in the assembled entry order (no FMA).  Host arrays, or
 * device arrays enqueued on the context stream (_device; nothing is waited for). */
int cpk_kkt_apply(cpk_kkt K, const double *z, double *y);
int cpk_kkt_apply_device(cpk_kkt K, const double *d_z, double *d_y);
/* The true residual of an N x k block: R(:, j) = Bm(:, j) - K*Z(:, j), r_i = b_i - s_i with the
 * row sum above, and norms[4 j .. 4 j + 3] = sum r(1:n)^2, sum r(n+1:N)^2, sum b(1:n)^2,
 * sum b(n+1:N)^2 of column j: sums, not roots; a fixed-order sum each, or under the engine option
 * exact_dots the correctly rounded exact sum of its TwoProd pairs.  Column-major with ldz, ldb,
 * ldr >= N; rows beyond N are not touched.  R or norms may be NULL; R == Bm with ldr == ldb is
 * allowed (a row reads b_i before it writes r_i).  Column j's R and sums do not depend on k, on j
 * or on the other columns (a NaN stays in its column), and equal the single-column call's.
 * Refused before anything is written: NULL K, Z or Bm (CPK_ERR_ARGS); k < 0 or a leading
 * dimension below N (CPK_ERR_DIM).  k == 0 does nothing.  _device: device arrays (d_norms too),
 * enqueued on the context stream, nothing waited for.  _device_sums: the same device operands
 * with the sums returned to HOST memory (4 k doubles, required): the one variant that waits for
 * the stream, for a caller that has no device allocator; not for use during stream capture. */
int cpk_kkt_residual(cpk_kkt K, int64_t k, const double *Z, int64_t ldz, const double *Bm, int64_t ldb, double *R,
                     int64_t ldr, double *norms);
int cpk_kkt_residual_device(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm, int64_t ldb,
                            double *d_R, int64_t ldr, double *d_norms);
int cpk_kkt_residual_device_sums(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm,
                                 int64_t ldb, double *d_R, int64_t ldr, double *norms);
/* Routing of the block residual.  Columns go in panels of 8; a panel streams K once for its
 * columns (one panel product, then each column's sums from its r and b in the single-column
 * pass's order), and a panel of fewer columns than the measured crossover runs as a
 * loop of single-column passes instead.  Either path gives a column the same bits in both modes,
 * so the routing never changes a result.  cpk_kkt_set_route: 0 by the crossover (default), 1
 * always the panel path, 2 always the loop (tests, measurements).  cpk_kkt_route_info:
 * {columns per panel, the crossover, the route in force, panels run on the panel path so far}. */
int cpk_kkt_set_route(cpk_kkt K, int route);
int cpk_kkt_route_info(cpk_kkt K, int64_t info[4]);
/* The verified, optionally warm-started solve of K*x = b with an existing M, one right-hand side.
 * M must be the preconditioner of K's own B and C (opLDL2(G, B, -C)): the driver's shift uses M's
 * copy of B', which the call cannot compare with K's; only M's context and dimensions are checked.
 * warm == 0: cpk_reg_solve_device(ctx, method, b, A, B, C, M, opts, x, stats) on K's handles,
 * unchanged.  warm != 0: x holds x0 on entry, and the call composes reg_cpkrylov's driver
 * (reg_cpkrylov.m:152-175) around the residual: r = b - K*x0 (cpk_kkt_residual), the same driver
 * on r (its shift included when r(n+1:N) is nonzero), x = x0 + dx with one rounding per entry.
 * THE METHOD'S STOP TEST THEN RUNS ON THE CORRECTION SYSTEM: atol and rtol are relative to the
 * initial preconditioned residual of r, not of b.  res (HOST memory in both variants, 8 doubles,
 * may be NULL): res[0..3] the four sums (cpk_kkt_residual's order) of the start residual --
 * warm of b - K*x0, cold of b itself (so res[0..1] == res[2..3]) -- and res[4..7] those of
 * b - K*x for the returned x.  All six methods.  A stop inside the driver (CPK_ERR_INDEFINITE)
 * is returned with the driver's own code and message; x is then x0 plus whatever the driver wrote
 * (cold: what it wrote), and res is still filled.  b, x: N entries, host or (_device) device. */
int cpk_kkt_solve(cpk_kkt K, int method, const double *b, cpk_pc M, const cpk_opts *opts, double *x, int warm,
                  cpk_stats *stats, double *res);
int cpk_kkt_solve_device(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x, int warm,
                         cpk_stats *stats, double *res);
/* The exactly rounded true residual: cpk_kkt_residual's three entries with
 *     r_i = RN( b_i - sum_e K_ie * z_col(e) ),
 * the EXACT sum of b_i and the TwoProd pairs p = -v*z, q = fma(-v, z, -p) of the row's stored
 * entries (p + q = -v*z unless the product under- or overflows, the caveat of the exact inner
 * products), rounded once to nearest even: one definition, whatever the entry order, the grid or
 * the route a row takes through the kernel; an exact zero is +0.0.  A non-finite term (b_i
 * included) makes r_i a NaN, in that row only; an empty row gives RN(b_i) = b_i.  The arguments,
 * the refusals and their order, R == Bm, the NULL outputs and the padding rows are
 * cpk_kkt_residual's.  norms are the four sums cpk_kkt_residual would return on that r and b
 * (exact under exact_dots, fixed-order otherwise).  A block is a loop of single-column passes (no
 * panel kernel, no routing): column j depends neither on k, nor on j, nor on its neighbours. */
int cpk_kkt_residual_exact(cpk_kkt K, int64_t k, const double *Z, int64_t ldz, const double *Bm, int64_t ldb, double *R,
                           int64_t ldr, double *norms);
int cpk_kkt_residual_exact_device(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm, int64_t ldb,
                                  double *d_R, int64_t ldr, double *d_norms);
int cpk_kkt_residual_exact_device_sums(cpk_kkt K, int64_t k, const double *d_Z, int64_t ldz, const double *d_Bm,
                                       int64_t ldb, double *d_R, int64_t ldr, double *norms);
/* Iterative refinement of cpk_kkt_solve on that residual, one right-hand side, all six methods.
 * x_0 = x0 (warm != 0; x holds it on entry) or 0.  Driver call j = 0 .. max_steps runs the driver
 * cpk_kkt_solve's warm path runs, from a zero start, on r_j = the exactly rounded b - K*x_j (cold,
 * j = 0: on b itself, which r_0 then is) and gives the trial x_j + dx_j, one rounding per entry.
 * EACH DRIVER CALL'S STOP TEST RUNS ON ITS CORRECTION SYSTEM: atol and rtol are relative to the
 * initial preconditioned residual of r_j, not of b.  For j < max_steps the next residual r_{j+1}
 * is formed at the trial: if its sum of squares is not below r_j's (a NaN included) the trial is
 * dropped, x = x_j is returned and the loop ends; otherwise x_{j+1} is the trial.  The trial of
 * call j = max_steps is taken without a further residual, so max_steps == 0, cold, is
 * cpk_kkt_solve's cold solve.  steps_out (may be NULL): the corrections in the returned x, that is
 * the driver calls after the first whose trial was taken; -1 when the first call's own trial was
 * dropped and x is x_0.  res (HOST memory in both variants,
 * 4 (max_steps + 1) doubles, may be NULL): row j the four sums (cpk_kkt_residual's order) of r_j
 * for every residual formed, a dropped trial's included: steps_out + 1 rows when the loop ran to
 * its end or stopped inside the driver, steps_out + 3 when a trial was dropped (steps_out <
 * max_steps with CPK_OK: the last two rows are those of the returned x and of the dropped trial);
 * rows beyond are not written.  stats: the last driver call's.  A stop inside the driver
 * (CPK_ERR_INDEFINITE) ends the loop and is returned with the driver's own code; x is then x_j plus
 * whatever the driver wrote.  Refusals are cpk_kkt_solve's (an Operator has no K; a distributed
 * context has none either), and CPK_ERR_ARGS for max_steps < 0; a refusal writes nothing: the host
 * entry leaves x as it was. */
int cpk_kkt_solve_refined(cpk_kkt K, int method, const double *b, cpk_pc M, const cpk_opts *opts, double *x, int warm,
                          int max_steps, cpk_stats *stats, double *res, int *steps_out);
int cpk_kkt_solve_refined_device(cpk_kkt K, int method, const double *d_b, cpk_pc M, const cpk_opts *opts, double *d_x,
                                 int warm, int max_steps, cpk_stats *stats, double *res, int *steps_out);
/* The adjoint of cpk_kkt_solve, one right-hand side: with x = K \ b and gx = dL/dx it returns
 * lam = K' \ gx = dL/db and the gradients with respect to the values of K's own handles, each in
 * its handle's creating call's value order (cpk_mat_sample_outer on that handle; x = [xx; xy],
 * lam = [lx; ly]):
 *     gA (cA entries) = -lx_i * xx_j                     on A's entries (i, j),
 *     gB (cB entries) = -(ly_i * xx_j + xy_i * lx_j)     on B's, one term for each place B sits in K,
 *     gC (cC entries) = +ly_i * xy_j                     on C's (K holds -C).
 * gA, gB, gC may each be NULL; a count must be its handle's entry count (CPK_ERR_DIM).  G gets no
 * gradient: the preconditioner does not change the solution.  Second derivatives are not formed.
 * lam is solved by cpk_kkt_solve[_device](KT ? KT : K, method, gx, M, opts, lam, warm, stats, res):
 * stats and res are that solve's, and warm != 0 takes lam as the start (usually the previous outer
 * iteration's lam), with that call's stop test on the correction system.  KT is the operator of
 * the transposed system, built on A', B, C; KT == NULL solves with K itself, BY WHICH THE CALLER
 * ASSERTS THAT A IS SYMMETRIC: this is not checked.  A stop inside the driver is returned with the
 * driver's own code and message; lam is then whatever the driver wrote, and no gradient array is
 * touched.  Refusals, before anything is written: those of cpk_kkt_solve, and CPK_ERR_ARGS when KT
 * is given and its context or dimensions differ from K's.  The call returns when the gradients are
 * complete.  x, gx, lam: N entries; host arrays, or (_device) device arrays, gradients included. */
int cpk_kkt_adjoint(cpk_kkt K, cpk_kkt KT, int method, const double *x, const double *gx, cpk_pc M, const cpk_opts *opts,
                    double *lam, int warm, double *gA, int64_t cA, double *gB, int64_t cB, double *gC, int64_t cC,
                    cpk_stats *stats, double *res);
int cpk_kkt_adjoint_device(cpk_kkt K, cpk_kkt KT, int method, const double *d_x, const double *d_gx, cpk_pc M,
                           const cpk_opts *opts, double *d_lam, int warm, double *d_gA, int64_t cA, double *d_gB, int64_t cB,
                           double *d_gC, int64_t cC, cpk_stats *stats, double *res);

/* ---- a block of right-hand sides in lockstep (cpcg and cpminres) ------------------------ */
/* [X(:,j), Y(:,j), stats(j), flag(j)] = method(B(:,j), A, C, M, opts) for j < k
 * (kernels/cpcg.m:1, kernels/cpminres.m:1, column by column; the reference has no block solve).
 * The columns iterate together on one GPU in panels of 8, sharing one pass over blkdiag(A, C)
 * and one panel apply of M per iteration; k > 8 runs its panels one after the other.  A column
 * whose own stop test holds freezes while the others run on, so its niters, history, solved, x
 * and y are those of the column solved alone with the same opts (itmax = n by default, stopTol
 * from its own initial residual); a column's result does not depend on k, on its position or on
 * the other columns (a NaN stays in its column).  cpminres runs the unfused update (engine
 * option no_minres_fuse), which the single-column solve equals bit for bit.
 * B: n x k, X: n x k, Y: m x k, column-major with ldb, ldx >= n and ldy >= m; rows beyond the
 * column length are not touched.  stats: k entries (each with its own hist / hist_cap; loop_ms is
 * its panel's device time, bytes_moved the panel's model bytes / its columns) or NULL;
 * col_status: k cpk_status values or NULL.  cpk_stats.status keeps its meaning (cpcglanczos only)
 * and is always 0 here: which columns failed is reported in col_status alone, so pass it to tell
 * them apart (a failed column also has solved = 0).  opts.print is ignored: nothing is printed.
 * Returns CPK_OK when no column failed, else the status of the first failing column (the
 * reference's indefinite / complex-norm stop, CPK_ERR_INDEFINITE: that column stops alone) with
 * its index and message in cpk_last_error; every column's outputs are written either way.
 * Refused before anything is written: NULL arguments (CPK_ERR_ARGS), k < 0 or a leading
 * dimension below the column length (CPK_ERR_DIM), and with CPK_ERR_UNSUPPORTED a distributed
 * preconditioner, the handle semantics of residual_update in effect (as cpk_pc_apply_multi), and
 * methods other than CPK_CG and CPK_MINRES.  k == 0 does nothing.  Small blocks are not routed to
 * single solves (DESIGN.md "Lockstep block solve" has the measured crossover). */
int cpk_method_solve_multi(cpk_ctx ctx, int method, int64_t k, const double *B, int64_t ldb, cpk_mat A, cpk_mat C,
                           cpk_pc M, const cpk_opts *opts, double *X, int64_t ldx, double *Y, int64_t ldy,
                           cpk_stats *stats, int *col_status);
/* Same with device-resident d_B (n x k) and d_XY (N x k, [x; y] per column, ldxy >= N). */
int cpk_method_solve_multi_device(cpk_ctx ctx, int method, int64_t k, const double *d_B, int64_t ldb, cpk_mat A,
                                  cpk_mat C, cpk_pc M, const cpk_opts *opts, double *d_XY, int64_t ldxy,
                                  cpk_stats *stats, int *col_status);
/* reg_cpkrylov's shift + method + recovery (reg_cpkrylov.m:152-175) per column of an N x k block
 * with an existing M: the shift is decided per column by any(b(n+1:N, j)), xy0 = M*[0; b2] of the
 * shifted columns is one block apply, an unshifted column keeps xy0 = 0.  B, X: N x k, ldb, ldx
 * >= N.  Statuses, refusals and stats as cpk_method_solve_multi (stime, ptime in every entry). */
int cpk_reg_solve_multi(cpk_ctx ctx, int method, int64_t k, const double *B, int64_t ldb, cpk_mat A, cpk_mat Bm,
                        cpk_mat C, cpk_pc M, const cpk_opts *opts, double *X, int64_t ldx, cpk_stats *stats,
                        int *col_status);
int cpk_reg_solve_multi_device(cpk_ctx ctx, int method, int64_t k, const double *d_B, int64_t ldb, cpk_mat A,
                               cpk_mat Bm, cpk_mat C, cpk_pc M, const cpk_opts *opts, double *d_X, int64_t ldx,
                               cpk_stats *stats, int *col_status);
/* The block forms of cpk_kkt_solve and cpk_kkt_adjoint: N x k column-major blocks with leading
 * dimensions >= N, as cpk_kkt_residual takes them; host arrays, or (_device) device arrays.
 *
 * cpk_kkt_solve_multi: column j is cpk_kkt_solve on B(:, j).  warm == 0: X(:, j) = 0 and the start
 * sums are those of b_j.  warm != 0 (one flag for the block): X holds X0 on entry, R = B - K*X0 by
 * the block residual, the driver runs on R and X = X0 + dX per column -- EVERY COLUMN'S STOP TEST THEN
 * RUNS ON ITS CORRECTION SYSTEM, as in cpk_kkt_solve.  The driver is cpk_reg_solve_multi_device
 * unchanged: CPK_CG and CPK_MINRES (any other method: CPK_ERR_UNSUPPORTED), never routed by k, so a
 * column's bits do not depend on k, on its position or on its neighbours.  stats: k entries or NULL;
 * col_status: k cpk_status values or NULL; res (HOST memory in both variants, 8 k doubles, may be
 * NULL): res[8 j .. 8 j + 7] are column j's eight sums in cpk_kkt_solve's layout, the last four from
 * one block residual of the returned X.  Errors are per column as in cpk_method_solve_multi: the
 * return value is the first failing column's status, col_status holds all of them, and every
 * column's X and sums are still written.  Refused before anything is written: NULL arguments
 * (CPK_ERR_ARGS), k < 0 or a leading dimension below N (CPK_ERR_DIM), and what
 * cpk_method_solve_multi refuses with CPK_ERR_UNSUPPORTED (a distributed context among them).
 * k == 0 does nothing.  K keeps the block workspace, grown on first use. */
int cpk_kkt_solve_multi(cpk_kkt K, int method, int64_t k, const double *B, int64_t ldb, cpk_pc M, const cpk_opts *opts,
                        double *X, int64_t ldx, int warm, cpk_stats *stats, int *col_status, double *res);
int cpk_kkt_solve_multi_device(cpk_kkt K, int method, int64_t k, const double *d_B, int64_t ldb, cpk_pc M,
                               const cpk_opts *opts, double *d_X, int64_t ldx, int warm, cpk_stats *stats,
                               int *col_status, double *res);
/* The three gradient passes alone, from a block X and a block Lam (x_c = [xx_c; xy_c], lam_c =
 * [lx_c; ly_c]), each gradient in its handle's creating call's value order; a NULL gradient is not
 * formed, a count must be its handle's entry count (CPK_ERR_DIM).  Per stored entry (i, j) the sum
 * starts at 0.0 and adds separately rounded products (no FMA) in column order c = 0 ... k-1, the
 * factor applied last with one rounding:
 *     gA = -1 * sum_c lx_c[i] * xx_c[j]
 *     gB = -1 * sum_c (ly_c[i] * xx_c[j], then xy_c[i] * lx_c[j])
 *     gC = +1 * sum_c ly_c[i] * xy_c[j]
 * -- cpk_mat_sample_outer's sums on the stacked columns (for gB the 2k columns [ly_0, xy_0, ...] and
 * [xx_0, lx_0, ...]), and with k == 1 cpk_kkt_adjoint's bits.  Every entry of each creating call
 * is written exactly once; k == 0 writes factor * 0.0.  The call returns when the gradients are
 * complete.  A distributed context: CPK_ERR_UNSUPPORTED. */
int cpk_kkt_sample_multi(cpk_kkt K, int64_t k, const double *X, int64_t ldx, const double *Lam, int64_t ldl, double *gA,
                         int64_t cA, double *gB, int64_t cB, double *gC, int64_t cC);
int cpk_kkt_sample_multi_device(cpk_kkt K, int64_t k, const double *d_X, int64_t ldx, const double *d_Lam, int64_t ldl,
                                double *d_gA, int64_t cA, double *d_gB, int64_t cB, double *d_gC, int64_t cC);
/* The sampler has two paths with the same bits: the run-time-k kernel of cpk_mat_sample_outer on the
 * column-major blocks (for gB on 2k staged columns), and a panel kernel on interleaved copies of X
 * and Lam (8 columns of a row contiguous).  cpk_kkt_set_sample_route: 0 by the measured rule
 * (default: the panel kernel where the last panel is full, DESIGN.md "The block adjoint"), 1 always
 * the panel kernel (k >= 2), 2 always the run-time-k kernel (tests, measurements).
 * cpk_kkt_sample_route_info: {columns per panel, the padded columns of the last panel up to which
 * the rule takes the panel kernel, the route, the calls that took the panel kernel so far}. */
int cpk_kkt_set_sample_route(cpk_kkt K, int route);
int cpk_kkt_sample_route_info(cpk_kkt K, int64_t info[4]);
/* Lam = cpk_kkt_solve_multi(K, method, GX, M, opts, warm), then cpk_kkt_sample_multi(K, X, Lam): the
 * gradients of a batch, summed over its k columns in one pass per handle.  There is no KT: the block
 * methods are the symmetric ones, BY WHICH THE CALLER ASSERTS THAT A IS SYMMETRIC (not checked).
 * If any column's driver stops with an error the call returns that status (col_status names the
 * columns) before any gradient pass is enqueued: Lam and res are written, no gradient array is
 * touched.  Refusals are those of the two entries, before anything is written. */
int cpk_kkt_adjoint_multi(cpk_kkt K, int method, int64_t k, const double *X, int64_t ldx, const double *GX, int64_t ldg,
                          cpk_pc M, const cpk_opts *opts, double *Lam, int64_t ldl, int warm, double *gA, int64_t cA,
                          double *gB, int64_t cB, double *gC, int64_t cC, cpk_stats *stats, int *col_status, double *res);
int cpk_kkt_adjoint_multi_device(cpk_kkt K, int method, int64_t k, const double *d_X, int64_t ldx, const double *d_GX,
                                 int64_t ldg, cpk_pc M, const cpk_opts *opts, double *d_Lam, int64_t ldl, int warm,
                                 double *d_gA, int64_t cA, double *d_gB, int64_t cB, double *d_gC, int64_t cC,
                                 cpk_stats *stats, int *col_status, double *res);
/* Diagnostic (not in the reference): the block solve's Krylov product alone.  Y(:, j) =
 * blkdiag(A, C) * X(:, j), equal to cpk_mat_spmv on the column bit for bit, and dots[2 j],
 * dots[2 j + 1] = <y_j(1:n), x_j(1:n)>, <y_j(n+1:N), x_j(n+1:N)> as the solvers take them (the
 * exact sums under engine option exact_dots).  Host arrays, X, Y: N x k, ldx, ldy >= N. */
int cpk_debug_spmm(cpk_ctx ctx, cpk_mat A, cpk_mat C, cpk_pc M, int64_t k, const double *X, int64_t ldx, double *Y,
                   int64_t ldy, double *dots);
/* Diagnostic (not in the reference): out[j] = <A(:, j), B(:, j)>, j < nv, taken exactly as the
 * solvers take their sums: a plain dot functor through the element-wise reducing launch (kind 0)
 * or its tiled form (kind 1), nv in {1, 2, 4}; the exact accumulator under engine option
 * exact_dots, the fixed-tree sums otherwise.  grid = 0: the solvers' own grid for n; grid > 0:
 * that many workgroups (at most the streaming kernels' cap).  Host arrays, A, B: n x nv, lda,
 * ldb >= n; n = 0 gives +0.0.  On a context of several ranks the call is collective: every rank
 * passes its local rows and receives the global sums.  Bad arguments: CPK_ERR_ARGS. */
int cpk_debug_dot(cpk_ctx ctx, int kind, int64_t n, int nv, const double *A, int64_t lda, const double *B,
                  int64_t ldb, int grid, double *out);
/* Diagnostic: out[i] = the exact mode's norm([a[i] b[i]]) evaluated on the device, i < n. */
int cpk_debug_xnorm2(cpk_ctx ctx, int64_t n, const double *a, const double *b, double *out);
/* Diagnostic (not in the reference): ONE Arnoldi step of cpgmres (cpgmres.m:212-247) or cpdqgmres
 * (cpdqgmres.m:208-269) on the caller's data, through the launches the solvers make after w = M*[u; -t]:
 * the window dots, the orthogonalisation with its scalar step (rotations, SymGivens, g, residNorm,
 * stop), and the normalisation (cpgmres) or the direction update (cpdqgmres).  Host arrays; every
 * array is uploaded, the step runs, and every array but w and ut is read back.
 *   method   CPK_GMRES or CPK_DQGMRES;  win: restart, resp. mem (>= 1)
 *   n, N     0 <= n <= N: rows [0, n) are the x-part, [n, N) the y-part of every vector
 *   kk       the iteration performed (>= 1; cpgmres: <= restart);  itmax: cpdqgmres's stop
 *   running  0: the step is a no-op and nothing changes
 *   grid     0: the solver's own grid for the window dots; > 0: that many workgroups (capped)
 *   V        N x (win + 1), ldv >= N: cpgmres column j - 1 holds [V(:,j); Q(:,j)], column kk is written;
 *            cpdqgmres ring slot (j - 1) % (mem + 1), slot kk % (mem + 1) is written
 *   PV, xy   cpdqgmres only (N x (mem + 1), ldpv >= N, and N): slot (kk - 1) % (mem + 1) and [x; y]
 *   w, ut    N each: M*[u; -t] and [u; t]
 *   H, c, s, g  the engine's storage.  cpgmres: H(i, j) (1-based) at H[(i - 1) + (j - 1) * (restart + 1)],
 *            (restart + 1) * restart doubles; c, s: restart; g: restart + 1.  cpdqgmres: the reference's
 *            H(j, col), col = 2 + k - j its diagonal-compressed column, at
 *            H[(j % (mem + 2)) * (mem + 2) + (col - 1)], (mem + 2)^2 doubles (a ring of mem + 2 rows, row kk
 *            cleared by the step); c, s at (j - 1) % mem: mem; g at (j - 1) % (mem + 1): mem + 1.
 *   H_dots   optional: H's storage as the window dots left it, before the orthogonalisation reads it
 *   stopTol, residNorm, hk1, hist  in and out (hist: the one history value, written iff nh = 1)
 *   stop, err, err_val, err_iter, nh  out (err = 4: the squared norm err_val of the new vector is negative)
 * On a context of several ranks the call is collective: every rank passes its local rows and its
 * own n, and receives the same scalars.  A window wider than the distributed reduction buffer
 * (2 win sums > 4096): CPK_ERR_UNSUPPORTED.  Bad arguments: CPK_ERR_ARGS, before any device call.
 * Under engine option basis_f32 the call rounds V and PV to float on upload (every slot), runs the
 * float launches and returns the rings as doubles, so every slot comes back as its float image and the
 * written slots hold the once-rounded vectors; the struct and its meaning are unchanged.  A context
 * of several ranks then answers CPK_ERR_UNSUPPORTED. */
typedef struct {
    int method, running, grid;
    int64_t n, N, win, kk, itmax;
    double stopTol, residNorm, hk1, hist;
    double *V;
    int64_t ldv;
    double *PV;
    int64_t ldpv;
    double *xy;
    const double *w, *ut;
    double *H, *c, *s, *g, *H_dots;
    int stop, err;
    double err_val;
    int64_t err_iter, nh;
} cpk_arnoldi_step;
int cpk_debug_arnoldi_step(cpk_ctx ctx, cpk_arnoldi_step *io);

/* Diagnostic: device time per launch (ms, HIP events, `reps` launches after a warm-up) of the
 * panel product with kc <= 8 columns and, in the same run, of the single-column Krylov product
 * on one column (tools/solve_multi_timing.py). */
int cpk_debug_spmm_time(cpk_ctx ctx, cpk_mat A, cpk_mat C, cpk_pc M, int kc, int reps, double *ms_panel,
                        double *ms_single);

/* The driver's shift step alone (reg_cpkrylov.m:152-160): if any(b(n+1:N)), xy0 = M*[0; b2]
 * and b1 = b(1:n) - A*xy0(1:n) - B'*xy0(n+1:N); else b1 = b(1:n), xy0 = 0.  Device pointers:
 * d_b (N), d_b1 (n), d_xy0 (N).  *shifted reports whether the shift was taken. */
int cpk_reg_shift_device(cpk_ctx ctx, const double *d_b, cpk_mat A, cpk_mat B, cpk_mat C, cpk_pc M,
                         double *d_b1, double *d_xy0, int *shifted);

/* ---- measurement ----------------------------------------------------------------------- */
/* Average device time (HIP events on the context stream, `reps` back-to-back launches) and
 * algorithmic HBM bytes per launch of each kernel class of an
 * iteration.  Times in ms. */
typedef struct {
    double spmv_ms, spmv_bytes;      /* Krylov operator blkdiag(A, C) SpMV (u = A*v, t = C*q) */
    double resid_ms, resid_bytes;    /* saddle-point SpMV r = x - Kp*y (refinement residual) */
    double fwd_ms, fwd_bytes;        /* forward sweep w = L \ P'x (all rounds) */
    double bwd_ms, bwd_bytes;        /* backward sweep y = P (L' \ (D \ w)) (all rounds) */
    double apply_ms, apply_bytes;    /* one M*z with the current properties */
    int64_t fwd_launches, bwd_launches;
    double fwd_resid_ms, fwd_resid_bytes;  /* refinement input fused into the forward sweep: r = x - Kp*y,
                                              then w = L \ P'r (0 when the apply does not fuse it) */
    double bwd_dead_store_bytes;     /* (ABI 3) bytes of the work-vector store the profiled backward
                                        sweep skips (round 0's w, dead after the sweep): not in
                                        bwd_bytes; the r03 byte model counted them */
} cpk_profile;
int cpk_profile_kernels(cpk_ctx ctx, cpk_mat A, cpk_mat C, cpk_pc M, int reps, cpk_profile *out);

/* Diagnostic (no reference counterpart): per-workgroup (start, end) s_memrealtime stamps of the
 * last round-0 sweep launch, 100 MHz ticks; *copied = 0 unless the library was built with
 * -DCPK_PIPE_STAMPS (tools/pipe_stamps.py). */
int cpk_debug_pipe_stamps(uint64_t *out, int npairs, int *copied);
/* Diagnostic: per-block s_memtime cycles of the last round-0 launch of each kernel variant,
 * out[v * 131072 + block] for v = forward, forward with the fused refinement residual, backward,
 * backward accumulating; *copied = 0 unless built with -DCPK_PIPE_STAMPS (tools/blk_cycles.py). */
int cpk_debug_blk_cycles(uint64_t *out, int64_t n, int64_t *copied);
/* Diagnostic: the upper-round loop-cost model of a preconditioner's sweeps, 10 int64 per (upper
 * block, direction): block, direction (0 forward), rows, level-loop trips, dataflow trips (-1:
 * not modelled), outside terms behind in-block ones, column sweep valid, loop chosen (0 level,
 * 1 dataflow, 2 column sweep, 3 column sweep with drains, 4 row-span), row-span eligible (-1: the
 * loop is off), its drain trips (-1: not eligible).  A distributed preconditioner whose separator
 * is solved by the block sweeps appends that sweep's records, with directions 2 (forward) and 3.
 * out = NULL: *copied = the total count. */
int cpk_debug_block_model(cpk_pc M, int64_t *out, int64_t n, int64_t *copied);
/* Diagnostic: the last cpdqgmres solve of this context run with engine option profile_passes
 * (eager batches, HIP events between its passes): out[8] = {iterations, Krylov SpMV ms, M*z ms,
 * window dots ms, orthogonalisation ms, direction ms, sum over the iterations of the dots'
 * window size, the same for the direction pass} (bench.py's s50 block: per-pass GB/s). */
int cpk_debug_pass_times(cpk_ctx ctx, double *out);

/* [c, s, d] = SymGivens(a, b)  (util/SymGivens.m:1-29) */
int cpk_symgivens(double a, double b, double *c, double *s, double *d);

#ifdef __cplusplus
}
#endif
#endif
