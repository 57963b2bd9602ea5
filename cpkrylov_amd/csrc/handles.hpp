// handles.hpp -- the structs behind cpk.h's opaque handles, with the device caches they keep, for
// capi.cpp and kkt_driver.cpp.  The handle types are the C header's, so global; like both units this
// header uses namespace cpk.
#pragma once
#include <map>
#include <memory>
#include <utility>

#include "cpk.h"
#include "dev.hpp"
#include "dist.hpp"
#include "solvers.hpp"

using namespace cpk;

struct cpk_ctx_s {
    Ctx c;
    std::unique_ptr<Comm> comm;
};

struct cpk_simgroup_s {
    SimGroup *g = nullptr;
    ~cpk_simgroup_s() {
        if (g) simgroup_destroy(g);
    }
};

// blkdiag(A, C) on the device with the values generations of A and C it holds
struct KrylovOp {
    std::unique_ptr<DMat> m;
    uint64_t va = 0, vc = 0;
};

struct cpk_mat_s {
    cpk_ctx_s *ctx = nullptr;
    uint64_t gen = 0;   // names the handle and its sparsity: never changes
    uint64_t vgen = 0;  // values generation: +1 per successful cpk_mat_set_values[_device]
    HCsr h;             // h.val may lag the device copy (h_stale): read the values through host()
    ValueMap vm;        // stored entry <- entries of the creating call's value array
    DValueMap dvm;      // its device copy, uploaded by the first update from device memory
    bool h_stale = false;
    bool hashed = false;
    uint64_t phash = 0;
    std::unique_ptr<DMat> d;                // lazily uploaded
    std::map<uint64_t, KrylovOp> ac;        // blkdiag(this, C) keyed by C's generation
    // the host copy with current values: downloaded after an update from device memory
    const HCsr &host() {
        if (h_stale) {
            Ctx &c = ctx->c;
            if (d->nnz) CPK_HIP(hipMemcpyAsync(h.val.data(), d->val.p, (size_t)d->nnz * sizeof(double), hipMemcpyDeviceToHost, c.stream));
            CPK_HIP(hipStreamSynchronize(c.stream));
            h_stale = false;
        }
        return h;
    }
    uint64_t pattern_hash() {
        if (!hashed) phash = pattern_hash_one(h), hashed = true;
        return phash;
    }
    const DMat &dev() {
        if (!ctx) throw Error(CPK_ERR_ARGS, "host-only matrix (created with ctx == NULL) used on the device");
        if (!d) {
            d = std::make_unique<DMat>();
            make_dmat(h, *d);  // no device copy yet: h is current
        }
        return *d;
    }
    // distributed rows follow the preconditioner's dof map, so they are
    // cached in the Precond itself (Precond::dist_ops), keyed by the matrices' generations: they
    // die with the preconditioner, and a new preconditioner never sees an old one's rows
    const DMat &krylov_op(cpk_mat_s *C, Precond &M) {
        if (M.dist != ctx->c.dist())
            throw Error(CPK_ERR_ARGS, "engine option dist1 changed after the preconditioner was built");
        if (!M.dist) return blkdiag_with(C);
        auto &slot = M.dist_ops[{'K', gen, C->gen}];
        if (!slot) {
            auto m = std::make_unique<DMat>();
            make_dist_dmat(dist_csr(blkdiag(host(), C->host()), *M.dofmap, ctx->c.rank, false, kKrylovSpare), ctx->c.nranks,
                           *m);
            slot = std::move(m);
        }
        return *slot;
    }
    // shift rows of a distributed preconditioner: A*xy0(1:n) and B'*xy0(n+1:N), x-part rows
    std::pair<const DMat *, const DMat *> shift_ops(Precond &M) {
        auto &sa = M.dist_ops[{'A', gen, 0}];
        auto &sb = M.dist_ops[{'B', gen, 0}];
        if (!sa || !sb) {
            const int64_t n = M.gn, N = M.gN;
            HCsr a = host(), bt;
            a.ncols = N;
            bt.nrows = n, bt.ncols = N;
            bt.ptr.assign(n + 1, 0);
            for (int64_t i = 0; i < n; i++) {
                for (int64_t q = M.Kp.ptr[i]; q < M.Kp.ptr[i + 1]; q++)
                    if (M.Kp.ind[q] >= n) bt.ind.push_back(M.Kp.ind[q]), bt.val.push_back(M.Kp.val[q]);
                bt.ptr[i + 1] = (int64_t)bt.ind.size();
            }
            auto ma = std::make_unique<DMat>(), mb = std::make_unique<DMat>();
            make_dist_dmat(dist_csr(a, *M.dofmap, ctx->c.rank, true), ctx->c.nranks, *ma);
            make_dist_dmat(dist_csr(bt, *M.dofmap, ctx->c.rank, true), ctx->c.nranks, *mb);
            sa = std::move(ma), sb = std::move(mb);
        }
        return {sa.get(), sb.get()};
    }
    // this handle's n rows come first in blkdiag (hostsparse.cpp), C's after them, so the
    // operator's value array is [A's values; C's values]: a refresh is one copy per stale half
    void refresh_half(Ctx &c, cpk_mat_s *src, double *dst) {
        const size_t bytes = (size_t)src->h.nnz() * sizeof(double);
        if (!bytes) return;
        if (src->d) {
            CPK_HIP(hipMemcpyAsync(dst, src->d->val.p, bytes, hipMemcpyDeviceToDevice, c.stream));
        } else {  // never uploaded, so its host copy is current
            CPK_HIP(hipMemcpyAsync(dst, src->h.val.data(), bytes, hipMemcpyHostToDevice, c.stream));
            CPK_HIP(hipStreamSynchronize(c.stream));
        }
    }
    const DMat &blkdiag_with(cpk_mat_s *C) {
        if (!ctx) throw Error(CPK_ERR_ARGS, "host-only matrix (created with ctx == NULL) used on the device");
        auto it = ac.find(C->gen);
        if (it == ac.end()) {
            KrylovOp op;
            op.va = vgen, op.vc = C->vgen;
            op.m = std::make_unique<DMat>();
            make_dmat(blkdiag(host(), C->host()), *op.m);
            it = ac.emplace(C->gen, std::move(op)).first;
        }
        KrylovOp &op = it->second;
        if (op.va != vgen || op.vc != C->vgen) {
            // lazily, at the next use after an update of either matrix; the value array keeps
            // its address, so graphs captured on the operator replay on the new values
            DMat &m = *op.m;
            if (m.nnz != h.nnz() + C->h.nnz() || m.nrows != h.nrows + C->h.nrows || (int64_t)m.val.n != m.nnz)
                throw Error(CPK_ERR_ARGS, "blkdiag(A, C): the cached operator is not [A's entries; C's entries]");
            if (op.va != vgen) refresh_half(ctx->c, this, m.val.p), op.va = vgen;
            if (op.vc != C->vgen) refresh_half(ctx->c, C, m.val.p + h.nnz()), op.vc = C->vgen;
        }
        return *op.m;
    }
};

// The operator-valued A: the caller's callback, and blkdiag(0, C) -- n empty rows, then C's rows
// with their columns moved past n -- keyed by C's generation as cpk_mat_s::ac is.  Its value
// array is C's values, so an update of C is one copy at the next use, to the same address.
struct cpk_op_s {
    cpk_ctx_s *ctx = nullptr;
    int64_t n = 0;
    cpk_op_fn fn = nullptr;
    void *user = nullptr;
    int flags = 0;
    uint64_t gen = 0;
    int64_t calls = 0, fails = 0;
    std::map<uint64_t, KrylovOp> zc;
    OpHook hook() { return OpHook{fn, user, gen, flags, &calls, &fails, nullptr, nullptr}; }
    const DMat &krylov_op(cpk_mat_s *C) {
        auto it = zc.find(C->gen);
        if (it == zc.end()) {
            HCsr Z;
            Z.nrows = Z.ncols = n;
            Z.ptr.assign((size_t)n + 1, 0);
            KrylovOp op;
            op.vc = C->vgen;
            op.m = std::make_unique<DMat>();
            make_dmat(blkdiag(Z, C->host()), *op.m);
            it = zc.emplace(C->gen, std::move(op)).first;
        }
        KrylovOp &op = it->second;
        if (op.vc != C->vgen) {
            DMat &m = *op.m;
            if (m.nnz != C->h.nnz() || m.nrows != n + C->h.nrows || (int64_t)m.val.n != m.nnz)
                throw Error(CPK_ERR_ARGS, "blkdiag(0, C): the cached operator does not hold C's entries");
            C->refresh_half(ctx->c, C, m.val.p), op.vc = C->vgen;
        }
        return *op.m;
    }
};

// K = [A B'; B -C] on the device in assemble_kp's entry order, with the handles' generations it
// holds and the map from their stored values (kp_value_sources' order) to its value array
struct cpk_kkt_s {
    cpk_ctx_s *ctx = nullptr;
    cpk_mat_s *A = nullptr, *B = nullptr, *C = nullptr;  // must outlive K
    uint64_t gen[3] = {0, 0, 0}, vgen[3] = {0, 0, 0};
    int64_t n = 0, m = 0, refreshes = 0;
    DMat K;
    DBuf<uint32_t> src;  // entry q <- entry src[q] of [A's values; B's values; C's values]
    DBuf<double> norms;  // the device side of a call's sums (8: cpk_kkt_solve's res)
    // the block residual's routing (0: by kKktPanelMinCols, 1: always the panel, 2: always the loop),
    // the panels run so far, and the panel path's work array (N * kMultiKP), allocated on first use
    int route = 0;
    int64_t panels = 0;
    DBuf<double> Tp;
    DBuf<double> ws;  // cpk_kkt_solve's vectors (kkt_solve_core), allocated by the first solve and kept
    // the block forms (cpk_kkt_solve_multi, cpk_kkt_sample_multi), each grown on first use and kept:
    // the warm start's residual and correction blocks (2 N k), the device side of the sums (12 k) and
    // the sampler's operands: the interleaved panels of X and Lam (2 * panel_count(k) * 8 N) or, on the
    // other route, gB's staged 2 k columns (2 k N)
    DBuf<double> wsb, normsb, panel_ops;
    // the block sampler's routing (0: by sample_panel_rule, 1: always the panel kernel, 2: always the
    // run-time-k kernel) and the calls that took the panel kernel so far
    int sample_route = 0;
    int64_t sample_panels = 0;
    // the operator on the handles' current values: a device gather where a values generation
    // moved (the value array keeps its address; nothing goes through the host)
    const DMat &current() {
        if (A->gen != gen[0] || B->gen != gen[1] || C->gen != gen[2])
            throw Error(CPK_ERR_ARGS, "kkt: a matrix handle of K was destroyed or replaced");
        if (A->vgen != vgen[0] || B->vgen != vgen[1] || C->vgen != vgen[2]) {
            const DMat &a = A->dev(), &b = B->dev(), &c = C->dev();
            if (a.nnz + 2 * b.nnz + c.nnz != K.nnz || (int64_t)src.n != K.nnz)
                throw Error(CPK_ERR_ARGS, "kkt: the value map does not match the handles");
            launch_kkt_gather(ctx->c, src.p, K.nnz, a.val.p, a.nnz, b.val.p, b.nnz, c.val.p, K.val.p);
            vgen[0] = A->vgen, vgen[1] = B->vgen, vgen[2] = C->vgen;
            refreshes++;
        }
        return K;
    }
};

struct cpk_pc_s {
    cpk_ctx_s *ctx = nullptr;
    std::unique_ptr<Precond> p;
};

inline void need(bool cond, const char *msg) {
    if (!cond) throw Error(CPK_ERR_ARGS, msg);
}

inline void check_method_dims(cpk_mat A, cpk_mat C, const cpk_pc_s *M) {
    need(A && C && M, "NULL argument");
    if (A->h.nrows != A->h.ncols || C->h.nrows != C->h.ncols) throw Error(CPK_ERR_DIM, "A and C must be square");
    if (A->h.nrows != M->p->gn || C->h.nrows != M->p->gm) throw Error(CPK_ERR_DIM, "A, C and M dimensions disagree");
}

// the shift's two products: 1 GPU reads rows < n of blkdiag(A, C) and of Kp (columns >= n);
// distributed mode has dedicated x-part row slices of [A 0] and [0 B']
struct ShiftOps {
    const DMat *A, *Bt;
    int64_t bt_colmin;
};
inline ShiftOps shift_ops(cpk_mat A, cpk_mat C, Precond &p) {
    if (p.dist) {
        auto pr = A->shift_ops(p);
        return {pr.first, pr.second, 0};
    }
    return {&A->blkdiag_with(C), &p.dKp, p.n};
}
