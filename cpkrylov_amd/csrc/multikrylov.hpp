// multikrylov.hpp -- device kernels of the lockstep block solve (cpk_method_solve_multi): kc <=
// kMultiKP independent constraint-preconditioned Krylov solves sharing one pass over
// blkdiag(A, C) and one panel apply of M per iteration (kernels/cpcg.m, kernels/cpminres.m column
// by column).  Included by solvers.hip, whose functors and policies the kernels run unchanged.
//
//   spmm_krylov_kernel   the panel form of spmv_stream<EpiKrylov<Pol, A>>: a workgroup walks the
//                        row blocks of DMat::blk, stages a block's (col, val) in LDS with one
//                        coalesced non-temporal pass, and its four waves then take the columns
//                        (wave w: columns w and w + 4), lanes across the block's rows.  Every
//                        (row, j) sums its separately rounded products val * x_j[col] in column
//                        order from 0.0 -- spmv_stream's order, the same bits.  The two inner
//                        products <y_j(1:n), x_j(1:n)>, <y_j(n+1:N), x_j(n+1:N)> stay inside a
//                        wave, so a wave reduction never mixes columns; the last workgroup sums
//                        each column's partials over the grid and runs the policy's epilogue on
//                        that column's state.
//   *_multi_kernel       the element-wise passes, one launch per panel with blockIdx.y the
//                        column: column j runs the single-column functor built on its own state
//                        and vectors with the single-column thread mapping and its own reduction
//                        slice (partials, tickets, exact sub-accumulators), so a column's
//                        reduction order is the single-column kernel's.
//
// Columns never mix: every value of column j comes from lanes of column j and values of column
// j.  A column whose stop test holds is frozen: its functors' setup() and the product's running
// mask skip it, and nothing of it is written.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "solver_common.hpp"

namespace cpk {

constexpr int kMK = kMultiKP;
constexpr size_t kMultiXStride = (size_t)kXSub * 4 * kXW;  // a column's exact sub-accumulators (<= 4 sums)

// the reduction buffers of a panel: column j's slice of each
struct RedBufM {
    double *partials;
    size_t pstride;
    unsigned *counter;  // [kMK + 1][kTicketWords]; the last one is the product's
    int64_t *xsub;      // [kMK][kMultiXStride] (exact mode, zero between launches)
    __device__ __host__ RedBuf col(int j) const {
        return RedBuf{partials + (size_t)j * pstride, counter + (size_t)j * kTicketWords, nullptr,
                      xsub ? xsub + (size_t)j * kMultiXStride : nullptr, nullptr};
    }
};

// the panel's functors, column j's at f[j] (built by the host on st + j and column j's vectors)
template <class F>
struct Panel {
    F f[kMK];
};

template <class F>
__global__ __launch_bounds__(kBlock) void ew_multi_kernel(int64_t N, Panel<F> p) {
    F f = p.f[blockIdx.y];
    CPK_EW_BODY(N, f);
}
template <int NV, class F, class A>
__global__ __launch_bounds__(kBlock) void ewred_multi_kernel(int64_t N, Panel<F> p, RedBufM rbm) {
    F f = p.f[blockIdx.y];
    const RedBuf rb = rbm.col(blockIdx.y);
    CPK_EWRED_BODY(N, f, rb);
}
template <class F>
__global__ __launch_bounds__(kBlock) void ewt_multi_kernel(int64_t N, Panel<F> p) {
    F f = p.f[blockIdx.y];
    CPK_EWT_BODY(N, f);
}
template <int NV, class F, class A>
__global__ __launch_bounds__(kBlock) void ewtred_multi_kernel(int64_t N, Panel<F> p, RedBufM rbm) {
    F f = p.f[blockIdx.y];
    const RedBuf rb = rbm.col(blockIdx.y);
    CPK_EWTRED_BODY(N, f, rb);
}

// ---- the Krylov product of a panel ---------------------------------------------------------
constexpr int kSpmmWaves = kBlock / kWave;      // 4
constexpr int kSpmmCols = kMK / kSpmmWaves;     // columns per wave: 2
constexpr int kSpmmSub = 256;                   // a long row's products staged per wave at once
static_assert(kMK % kSpmmWaves == 0, "columns map to waves");

// a wave's sum of one column handed to the grid: the fixed shuffle tree and one partial per
// workgroup, or (exact) the wave's merged expansion deposited into the column's sub-accumulator
__device__ __forceinline__ void wave_hand(double v, double *slot) {
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) st_agent(slot, v);
}
__device__ __forceinline__ void wave_hand(XAcc &v, double *) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        double o[kXK];
#pragma unroll
        for (int k = 0; k < kXK; k++) o[k] = __shfl_down(v.t[k], off, kWave);
        if (lane < off)
#pragma unroll
            for (int k = 0; k < kXK; k++) v.add(o[k]);
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < kXK; k++) xdeposit(v.ovf, v.t[k]);
}

// pols.f[j]: column j's policy (select / fin); st: the panel's kMK states; Y: the products,
// column j at Y + j * ldy; Ys (optional): the products with the rows >= n negated, [u; -t] (the
// input of cpminres's M * [u; -t], cpminres.m:190); part: [grid][kMK][2] partials; any: the
// panel's "any column running" word, written here for the kernels that follow
template <class Pol, class A>
__global__ __launch_bounds__(kBlock) void spmm_krylov_kernel(const uint32_t *__restrict__ ptr,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const int32_t *__restrict__ blk, int64_t nblk, DState *st,
                                                              int kc, Panel<Pol> pols, double *Y, int64_t ldy, double *Ys,
                                                              int64_t n, double *part, RedBufM rbm, int *any) {
    __shared__ double sv[kSpmvCap];
    __shared__ int32_t sc[kSpmvCap];
    __shared__ double pr[kSpmmWaves][kSpmmSub];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int wj = __builtin_amdgcn_readfirstlane(wid);  // the wave's first column, in an SGPR
    // PolStart::start per column: `running` from `stop` (nothing in this kernel writes stop)
    unsigned mask = 0;
    for (int j = 0; j < kc; j++)
        if (st[j].stop == 0) mask |= 1u << j;
    if (blockIdx.x == 0 && tid == 0) {
        for (int j = 0; j < kc; j++) st[j].running = (mask >> j) & 1;
        *any = mask != 0;
    }
    if (!mask) return;
    const double *xj[kSpmmCols];
    double *yj[kSpmmCols], *ysj[kSpmmCols];
    bool on[kSpmmCols];
    A dn[kSpmmCols], dm[kSpmmCols];
#pragma unroll
    for (int c = 0; c < kSpmmCols; c++) {
        const int j = wj + c * kSpmmWaves;
        on[c] = (mask >> j) & 1;
        Pol pj = pols.f[j];  // a copy out of the kernel arguments (wave-uniform index)
        xj[c] = on[c] ? pj.select(st + j, nullptr) : nullptr;
        yj[c] = Y + (int64_t)j * ldy;
        ysj[c] = Ys ? Ys + (int64_t)j * ldy : nullptr;
        int64_t *xs = rbm.xsub ? rbm.xsub + (size_t)j * kMultiXStride : nullptr;
        acc_init(dn[c], xs, 0, 2), acc_init(dm[c], xs, 1, 2);
    }
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        if (b != blockIdx.x) __syncthreads();  // the previous block's staged entries fully consumed
        const int64_t r0 = blk[b], r1 = blk[b + 1];
        const uint32_t e0 = ptr[r0], e1 = ptr[r1];
        if (e1 - e0 <= (uint32_t)kSpmvCap) {
            for (uint32_t e = tid; e < e1 - e0; e += kBlock) {
                sc[e] = __builtin_nontemporal_load(col + e0 + e);  // streamed once per panel
                sv[e] = __builtin_nontemporal_load(val + e0 + e);
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < kSpmmCols; c++) {
                if (!on[c]) continue;
                const double *x = xj[c];
                for (int64_t r = r0 + lane; r < r1; r += kWave) {
                    const uint32_t q1 = ptr[r + 1] - e0;
                    double acc = 0.0;
                    for (uint32_t e = ptr[r] - e0; e < q1; e++) acc += sv[e] * x[sc[e]];
                    const double xr = x[r];
                    yj[c][r] = acc;
                    if (r < n) {
                        if (ysj[c]) ysj[c][r] = acc;
                        dadd(dn[c], acc, xr);
                    } else {
                        if (ysj[c]) ysj[c][r] = -acc;
                        dadd(dm[c], acc, xr);
                    }
                }
            }
        } else {
            // one long row (r1 == r0 + 1): chunks of kSpmvCap entries staged by the workgroup; each
            // wave forms its columns' products kSpmmSub at a time and its lane 0 sums them in order
            double racc[kSpmmCols];
#pragma unroll
            for (int c = 0; c < kSpmmCols; c++) racc[c] = 0.0;
            for (uint32_t c0 = e0; c0 < e1; c0 += kSpmvCap) {
                const uint32_t len = min(e1 - c0, (uint32_t)kSpmvCap);
                if (c0 != e0) __syncthreads();
                for (uint32_t e = tid; e < len; e += kBlock) sc[e] = col[c0 + e], sv[e] = val[c0 + e];
                __syncthreads();
#pragma unroll
                for (int c = 0; c < kSpmmCols; c++) {
                    for (uint32_t s0 = 0; s0 < len; s0 += kSpmmSub) {  // uniform over the workgroup
                        const uint32_t sl = min(len - s0, (uint32_t)kSpmmSub);
                        if (on[c])
                            for (uint32_t i = lane; i < sl; i += kWave) pr[wid][i] = sv[s0 + i] * xj[c][sc[s0 + i]];
                        __syncthreads();
                        if (on[c] && lane == 0)
                            for (uint32_t i = 0; i < sl; i++) racc[c] += pr[wid][i];
                        __syncthreads();
                    }
                }
            }
            if (lane == 0)
#pragma unroll
                for (int c = 0; c < kSpmmCols; c++) {
                    if (!on[c]) continue;
                    const double acc = racc[c], xr = xj[c][r0];
                    yj[c][r0] = acc;
                    if (r0 < n) {
                        if (ysj[c]) ysj[c][r0] = acc;
                        dadd(dn[c], acc, xr);
                    } else {
                        if (ysj[c]) ysj[c][r0] = -acc;
                        dadd(dm[c], acc, xr);
                    }
                }
        }
    }
    // a column's two sums: inside its wave, then one partial (or deposit) per workgroup
#pragma unroll
    for (int c = 0; c < kSpmmCols; c++) {
        if (!on[c]) continue;
        const int j = wj + c * kSpmmWaves;
        double *slot = part + ((size_t)blockIdx.x * kMK + j) * 2;
        wave_hand(dn[c], slot);
        wave_hand(dm[c], slot + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing / depositing wave drains
    __syncthreads();
    if (tid == 0) s_last = arrive_last(rbm.counter + (size_t)kMK * kTicketWords);
    __syncthreads();
    if (!s_last) return;
    if constexpr (std::is_same<A, XAcc>::value) {
        __shared__ int64_t dig[2][kXW];
        __shared__ double rt[2];
        for (int j = 0; j < kc; j++) {  // uniform: every thread holds the same mask
            if (!((mask >> j) & 1)) continue;
            gather_digits(rbm.xsub + (size_t)j * kMultiXStride, 2, 0, 2, dig, nullptr);
            if (tid < 2) rt[tid] = xround(dig[tid]);
            __syncthreads();
            if (tid == 0) {
                const double tot[2] = {rt[0], rt[1]};
                Pol pj = pols.f[j];
                pj.fin(st + j, tot);
            }
            __syncthreads();
        }
    } else {
#pragma unroll
        for (int c = 0; c < kSpmmCols; c++) {
            if (!on[c]) continue;
            const int j = wj + c * kSpmmWaves;
            double a0 = 0.0, a1 = 0.0;
            for (unsigned g = lane; g < gridDim.x; g += kWave) {
                a0 += ld_agent(part + ((size_t)g * kMK + j) * 2);
                a1 += ld_agent(part + ((size_t)g * kMK + j) * 2 + 1);
            }
            a0 = wave_sum(a0), a1 = wave_sum(a1);
            if (lane == 0) {
                const double tot[2] = {a0, a1};
                Pol pj = pols.f[j];
                pj.fin(st + j, tot);
            }
        }
    }
}

}  // namespace cpk
