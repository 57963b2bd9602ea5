// solve_loop.hpp -- the host driver of the device solvers (host side only; included by solvers.hip):
// what the single-column solvers (SolveCore) and the lockstep block solve (MultiCore) share.  The
// per-call options and a column's initial DState, the cache of captured iteration graphs, the
// adaptive batch loop over a span of column states (a single-column solve is a span of one), and
// what a finished column reports: the indefinite-error text and the common cpk_stats fields.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <tuple>

#include "solver_common.hpp"

namespace cpk {

// entries of a column's residual history: one per iteration and the initial ones
inline int64_t hist_capacity(double itmax) { return (int64_t)std::min(itmax, 1.0e8) + 4; }

// ---- what a finished column reports ------------------------------------------------------------
// the reference's error text of a column stopped by st.err != 0
inline std::string indefinite_message(int method, const DState &h) {
    char buf[256];
    if (h.err == 1) {
        if (method == CPK_CGLANCZOS)
            snprintf(buf, sizeof buf,
                     "CPCGLanczos:IndefiniteError: Iter %lld, beta (before sqrt) = %g : preconditioner not second-order sufficient",
                     (long long)h.err_iter, h.err_val);
        else
            snprintf(buf, sizeof buf, "Iter %lld, beta (before sqrt) = %g : preconditioner does not behave as a spd matrix.",
                     (long long)h.err_iter, h.err_val);
    } else if (h.err == 3) {
        snprintf(buf, sizeof buf,
                 "Iter 0, 2nd Lanczos vec, beta (before sqrt) = %g : preconditioner does not behave as a spd matrix.",
                 h.err_val);
    } else if (h.err == 2) {
        snprintf(buf, sizeof buf, "Iter %lld, residNorm2 = %g < 0: complex residual norm", (long long)h.err_iter,
                 h.err_val);
    } else {
        snprintf(buf, sizeof buf, "Iter %lld: negative squared norm %g (complex square root)", (long long)h.err_iter,
                 h.err_val);
    }
    return buf;
}
// one history into the caller's buffer (prefix: a leading host value, cpsymmlq's beta1)
inline void copy_history(const cpk_stats &s, double *dstp, const double *d_src, int64_t len, int64_t *outlen,
                         bool prefix = false, double pv = 0) {
    *outlen = len + (prefix ? 1 : 0);
    if (!dstp) return;
    if (*outlen > s.hist_cap) throw Error(CPK_ERR_ARGS, "history buffer too small");
    if (prefix) *dstp++ = pv;
    if (len > 0) CPK_HIP(hipMemcpy(dstp, d_src, len * sizeof(double), hipMemcpyDeviceToHost));
}
// the cpk_stats fields every method and the block solve fill alike
inline void fill_stats(cpk_stats &s, const DState &h, bool prefix = false, double pv = 0) {
    s.niters = h.k;
    s.status = 0;
    copy_history(s, s.hist, h.hist, std::min(h.nh, h.hcap), &s.hist_len, prefix, pv);
}

// ---- captured iteration graphs -----------------------------------------------------------------
// A batch is a captured graph of b iterations, captured once per (loop site, live columns, b) and
// replayed by later calls of the solver that owns the cache.
struct GraphCache {
    std::map<std::tuple<size_t, int, int>, std::pair<hipGraph_t, hipGraphExec_t>> slots;
    ~GraphCache() {
        for (auto &g : slots) {
            if (g.second.second) (void)hipGraphExecDestroy(g.second.second);
            if (g.second.first) (void)hipGraphDestroy(g.second.first);
        }
    }
    // inst: the counter of instantiations this cache reports to.  A failed capture is ended and what
    // exists of it destroyed; a single-GPU context rethrows, a distributed one (a transport that
    // cannot be captured: deterministic, so every rank lands here) returns null: run eagerly
    hipGraphExec_t get(Ctx &c, size_t site, int kc, int b, int64_t &inst, const std::function<void()> &body) {
        auto &slot = slots[{site, kc, b}];
        if (!slot.second) {
            hipGraph_t graph = nullptr;
            try {
                CPK_HIP(hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal));
                for (int i = 0; i < b; i++) body();
                CPK_HIP(hipStreamEndCapture(c.stream, &graph));
                slot.first = graph;
                CPK_HIP(hipGraphInstantiate(&slot.second, graph, nullptr, nullptr, 0));
                inst++;
            } catch (const Error &e) {
                hipGraph_t g2 = nullptr;
                (void)hipStreamEndCapture(c.stream, &g2);
                if (g2) (void)hipGraphDestroy(g2);
                if (graph && graph != g2) (void)hipGraphDestroy(graph);
                slot = {nullptr, nullptr};
                (void)hipGetLastError();
                if (!c.dist()) throw;
                fprintf(stderr, "cpk: iteration-graph capture failed (%s); running batches eagerly\n", e.what());
                return nullptr;
            }
        }
        return slot.second;
    }
};

// ---- the batch loop ----------------------------------------------------------------------------
inline int pow2_at_least(double v, int cap) {
    int b = 1;
    while (b < cap && b < v) b <<= 1;
    return b;
}

// The size of the next batch, a power of two <= the base size.  After the first batch it follows
// the observed convergence rate, so the batch that crosses the tolerance carries few no-op
// iterations; the slowest column still running decides, and no batch runs far past itmax.  Every
// kernel tests the device-side `running` flag, so the size only affects time, never results.
struct BatchPlan {
    int base;
    bool adapt;
    double itmax;
    double res0[kMultiKP];
    int64_t k0[kMultiKP];
    void before(const DState *hs, int kc) {
        for (int j = 0; j < kc; j++) res0[j] = hs[j].residNorm, k0[j] = hs[j].k;
    }
    int after(const DState *hs, int kc) const {
        int want = 1;
        double left = 1;
        for (int j = 0; j < kc; j++) {
            const DState &h = hs[j];
            if (h.stop) continue;
            int bj = base;
            const double res = h.residNorm, tol = h.stopTol;
            if (adapt && h.k > k0[j] && res > 0 && res0[j] > res && tol > 0 && tol < res) {
                // geometric model of the residual over the last batch: iterations still needed
                const double rate = std::log(res / res0[j]) / (double)(h.k - k0[j]);
                const double rem = std::log(tol / res) / rate;
                if (rem > 0 && rem < 1e6) bj = pow2_at_least(std::ceil(rem), bj);
            }
            want = std::max(want, bj);
            left = std::max(left, itmax - (double)h.k);
        }
        return left < want ? pow2_at_least(left, want) : want;
    }
};

// run_batches' default: a batch with nothing around it
struct PlainBatch {
    template <class L, class R>
    void operator()(L &&launch, R &&readback) const { launch(), readback(); }
};

// What both cores are driven by: the per-call options, the columns' states and the graphs.
struct SolveDriver {
    Ctx &c;
    double atol = 1e-6, rtol = 1e-6, btol = 0, itmax = 0;
    int batch = 16;
    bool use_graph = true;
    bool single_step = false;  // every batch is one iteration (an operator-valued A called eagerly)
    // the iterations after which the device ends a loop by itself: itmax, except in a cpgmres cycle,
    // which counts from 0 to restart whatever itmax is (cpgmres.m:203) -- run_batches' guard
    double loop_limit = 0;
    GraphCache graphs;
    DBuf<DState> dst;     // a state per column: nstates travel between host and device,
    DState hs[kMultiKP];  // the first kc of a call are live
    const int nstates;
    SolveDriver(Ctx &cc, int nstates_) : c(cc), nstates(nstates_) { dst.alloc((size_t)nstates); }
    // itmax_default: the method's (size(A,1) in the reference; global sizes, identical on every rank)
    void resolve(const cpk_opts *o, double itmax_default) {
        atol = 1e-6, rtol = 1e-6, btol = 0, itmax = itmax_default;
        if (o) {
            if (o->has_atol) atol = o->atol;
            if (o->has_rtol) rtol = o->rtol;
            if (o->has_btol) btol = o->btol;
            if (o->has_itmax) itmax = o->itmax;
        }
        loop_limit = itmax;
        use_graph = !c.opts.no_graph;
        single_step = false;
        batch = c.opts.batch > 0 ? c.opts.batch : 16;
    }
    // the fields every column's state starts from (all others zero)
    void init_state(DState &h, int64_t hcap, double *hist) const {
        std::memset(&h, 0, sizeof h);
        h.itmax = (int64_t)std::min(itmax, 9.0e15);
        if (h.itmax < 0) h.itmax = 0;
        h.atol = atol, h.rtol = rtol, h.btol = btol;
        h.exact = c.exact() ? 1 : 0;
        h.hcap = hcap, h.hist = hist;
    }

    void pull() {
        CPK_HIP(hipMemcpyAsync(hs, dst.p, sizeof(DState) * nstates, hipMemcpyDeviceToHost, c.stream));
        CPK_HIP(hipStreamSynchronize(c.stream));
    }
    bool stopped(int kc) const {
        for (int j = 0; j < kc; j++)
            if (!hs[j].stop) return false;
        return true;
    }

    // Replay `body` (one iteration of every live column) in batches until the device has set every
    // live column's `stop`; the host only reads the states back between batches.
    // around(launch, readback): what surrounds a batch; it calls both, in that order (SolveCore: the
    // distributed status agreement).  printer (optional): called after every read-back.
    // The loop fails when a column runs loop_limit + 2 batches past its iteration count at entry.
    template <class Batch = PlainBatch>
    void run_batches(size_t site, int kc, int64_t &inst, const std::function<void()> &body,
                     const Batch &around = Batch(), const std::function<void()> &printer = nullptr) {
        pull();
        if (stopped(kc)) return;
        int64_t guard = 0;
        for (int j = 0; j < kc; j++) guard = std::max(guard, hs[j].k);
        guard += (int64_t)std::min(loop_limit, 4.0e9) + 2 * batch + 2;
        BatchPlan plan{single_step ? 1 : pow2_at_least(batch, 64), c.opts.batch <= 0, itmax};
        int b = plan.base;
        for (;;) {
            plan.before(hs, kc);
            around(
                [&] {
                    hipGraphExec_t exec = use_graph ? graphs.get(c, site, kc, b, inst, body) : nullptr;
                    if (use_graph && !exec) use_graph = false;  // this solver's batches run eagerly from here on
                    if (exec) CPK_HIP(hipGraphLaunch(exec, c.stream));
                    else
                        for (int i = 0; i < b; i++) body();
                    CPK_HIP(hipGetLastError());
                },
                [&] { pull(); });
            if (printer) printer();
            if (stopped(kc)) break;
            for (int j = 0; j < kc; j++)
                if (!hs[j].stop && hs[j].k > guard) throw Error(CPK_ERR_HIP, "solver loop did not terminate");
            b = plan.after(hs, kc);
        }
    }
};

// device time per launch of f: HIP events around `reps` back-to-back launches after one warm-up
template <class F>
double time_launches(Ctx &c, int reps, F &&f) {
    f();  // warm
    CPK_HIP(hipEventRecord(c.ev0, c.stream));
    for (int r = 0; r < reps; r++) f();
    CPK_HIP(hipEventRecord(c.ev1, c.stream));
    CPK_HIP(hipEventSynchronize(c.ev1));
    float ms = 0;
    CPK_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    return (double)ms / reps;
}

}  // namespace cpk
