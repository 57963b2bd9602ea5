// multiapply.hip -- the refined apply Y = M*X for a panel of kMultiKP right-hand sides
// (cpk_pc_apply_multi; opLDL2.multiply, ops/opLDL2.m:161-188, column by column): the kernels
// around the panel sweeps of multisweep.hip.
//
// Natural-order panels: Yp[i * KP + j] (the solution) and Rp[i * KP + j] (the residual), row i
// in the original order, so the KP values of a row are one 64-byte segment.
//
//   multi_resid_kernel   R = X - Kp*Y for the panel, one workgroup per row block of Kp (DMat::blk).
//                        Kp's (col, val) are streamed once per panel and staged in LDS; the work
//                        items are (row, j) pairs with j fastest across lanes, so each nonzero
//                        gathers one segment of Yp for all KP columns.  Each row sums its
//                        separately rounded products in column order from 0.0, then r = x - acc:
//                        spmv_stream's order, bit for bit.  A row longer than kSpmvCap sits alone
//                        in its block and is summed chunk by chunk.  With norms it also leaves
//                        the block's partial sums of r^2 (and of x^2 on the first use) per column.
//   multi_pred_kernel    per column: sum the row blocks' partials in block order (64 contiguous
//                        chunks, then the chunks in order: a fixed order that depends on Kp's
//                        row blocks only, not on a launch grid), then the loop's predicate
//                        ||r|| >= tol * ||x|| (opLDL2.m:183), the step count and the panel's
//                        "any column active" word.  A column that went inactive stays inactive.
//   multi_state_kernel   the panel's initial state; multi_store_kernel the user's Y and counts.
//
// Columns never mix: every value of column j is computed by lanes of column j from values of
// column j, so a non-finite value stays in its column.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev.hpp"

namespace cpk {

namespace {

constexpr int KP = kMultiKP;
constexpr int kResidThreads = 256;
constexpr int kLongChunk = kSpmvCap / KP;  // entries of a long row whose products are staged at once
constexpr int kPredThreads = 1024;
constexpr int kPredChunks = kPredThreads / (2 * KP);  // 64 chunks of row blocks x 16 sums

// part[b * 2 * KP + q]: q < KP the block's sum of r^2 of column q, q >= KP of x^2 of column q - KP
template <bool NORMS>
__global__ __launch_bounds__(kResidThreads) void multi_resid_kernel(
    const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
    const int32_t *__restrict__ blk, const double *__restrict__ X, int64_t ldx, int kc, const double *__restrict__ Yp,
    double *__restrict__ Rp, const int32_t *__restrict__ act, double *__restrict__ part, int first) {
    __shared__ double sv[kSpmvCap];   // staged values; a long row: its chunk's products [kLongChunk][KP]
    __shared__ int32_t sc[kSpmvCap];  // staged columns
    __shared__ double red[2 * kResidThreads];
    constexpr int TPB = kResidThreads;
    static_assert(TPB % KP == 0 && kLongChunk * KP <= kSpmvCap, "panel work items");
    if (act[KP] == 0) return;
    const int tid = threadIdx.x, j = tid % KP;
    const int64_t b = blockIdx.x;
    const int64_t r0 = blk[b], r1 = blk[b + 1];
    const uint32_t e0 = ptr[r0], e1 = ptr[r1];
    double rr = 0.0, xx = 0.0;
    if (e1 - e0 <= (uint32_t)kSpmvCap) {
        for (uint32_t e = tid; e < e1 - e0; e += TPB) {
            sc[e] = __builtin_nontemporal_load(col + e0 + e);  // streamed once per panel
            sv[e] = __builtin_nontemporal_load(val + e0 + e);
        }
        __syncthreads();
        for (int64_t i = tid; i < (r1 - r0) * KP; i += TPB) {
            const int64_t row = r0 + i / KP;
            const uint32_t q1 = ptr[row + 1] - e0;
            double acc = 0.0;
            for (uint32_t e = ptr[row] - e0; e < q1; e++) acc += sv[e] * Yp[(size_t)sc[e] * KP + j];
            const double xi = j < kc ? X[row + (int64_t)j * ldx] : 0.0;
            const double ri = xi - acc;
            Rp[(size_t)row * KP + j] = ri;
            if (NORMS) {
                rr += ri * ri;
                if (first) xx += xi * xi;
            }
        }
    } else {
        double acc = 0.0;  // one long row (r1 == r0 + 1); the threads tid < KP sum column tid
        for (uint32_t c0 = e0; c0 < e1; c0 += kLongChunk) {
            const uint32_t n = min(e1 - c0, (uint32_t)kLongChunk);
            for (uint32_t i = tid; i < n * KP; i += TPB) sv[i] = val[c0 + i / KP] * Yp[(size_t)col[c0 + i / KP] * KP + j];
            __syncthreads();
            if (tid < KP)
                for (uint32_t e = 0; e < n; e++) acc += sv[e * KP + tid];
            __syncthreads();
        }
        if (tid < KP) {
            const double xi = j < kc ? X[r0 + (int64_t)j * ldx] : 0.0;
            const double ri = xi - acc;
            Rp[(size_t)r0 * KP + j] = ri;
            if (NORMS) {
                rr += ri * ri;
                if (first) xx += xi * xi;
            }
        }
    }
    if (!NORMS) return;
    // the block's sums in a fixed order: each thread's rows ascending (above), then the TPB / KP
    // threads of a column ascending
    red[tid] = rr, red[TPB + tid] = xx;
    __syncthreads();
    if (tid < 2 * KP && (tid < KP || first)) {
        const double *p = red + (tid / KP) * TPB + tid % KP;
        double s = 0.0;
        for (int t = 0; t < TPB / KP; t++) s += p[t * KP];
        part[b * 2 * KP + tid] = s;
    }
}

// state: act[KP], any, nit[KP] (MultiState); xn2[KP]: the columns' sums of x^2, kept from the
// first use.  step: refinement solves taken so far; a column that stays active takes one more.
__global__ __launch_bounds__(kPredThreads) void multi_pred_kernel(const double *__restrict__ part, int64_t nblk,
                                                                   double tol, int step, int first, int32_t *state,
                                                                   double *xn2) {
    __shared__ double red[kPredThreads];
    const int tid = threadIdx.x, c = tid / (2 * KP), q = tid % (2 * KP);
    if (state[KP] == 0) return;
    const int64_t per = (nblk + kPredChunks - 1) / kPredChunks;
    const int64_t b1 = (c + 1) * per < nblk ? (c + 1) * per : nblk;
    double s = 0.0;
    if (q < KP || first) {
#pragma unroll 4  // 1024 threads: 128 registers each
        for (int64_t b = c * per; b < b1; b++) s += part[b * 2 * KP + q];
    }
    red[tid] = s;
    __syncthreads();
    if (tid < KP) {
        double rr = 0.0, xx = 0.0;
#pragma unroll 8
        for (int t = 0; t < kPredChunks; t++) rr += red[t * 2 * KP + tid];
        if (first) {
#pragma unroll 8
            for (int t = 0; t < kPredChunks; t++) xx += red[t * 2 * KP + KP + tid];
            xn2[tid] = xx;
        } else {
            xx = xn2[tid];
        }
        // while nit < nitref & (rNorm >= itref_tol * xNorm | force_itref)   (opLDL2.m:183)
        const int a = state[tid] != 0 && sqrt(rr) >= tol * sqrt(xx);
        state[tid] = a;
        if (a) state[KP + 1 + tid] = step + 1;
    }
    __syncthreads();
    if (tid == 0) {
        int any = 0;
        for (int t = 0; t < KP; t++) any |= state[t];
        state[KP] = any;
    }
}

// the panel's initial state: its kc columns active, no step taken (forced: `steps` for each)
__global__ void multi_state_kernel(int32_t *state, int kc, int steps, const int *gate) {
    const int t = threadIdx.x;
    if (t < KP) state[t] = t < kc, state[KP + 1 + t] = t < kc ? steps : 0;
    if (t == 0) state[KP] = kc > 0 && (!gate || *gate != 0);
}

// Y(:, j) = Yp(:, j) for the panel's kc columns (the padding columns and rows are never stored)
// and their step counts
__global__ void multi_store_kernel(int64_t N, int kc, const double *__restrict__ Yp, double *__restrict__ Y, int64_t ldy,
                                   const int32_t *__restrict__ state, int32_t *__restrict__ nit, const int *gate) {
    if (gate && *gate == 0) return;
    if (nit && blockIdx.x == 0 && threadIdx.x < (unsigned)kc) nit[threadIdx.x] = state[KP + 1 + threadIdx.x];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N * KP; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % KP);
        if (j < kc) Y[i / KP + (int64_t)j * ldy] = Yp[i];
    }
}

// the single-column apply's step count (Precond::apply's nit): set, or one more where the
// predicate held
__global__ void nit_kernel(int32_t *nit, int v, const int *active) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *nit = active ? *nit + (*active != 0) : v;
}

}  // namespace

void launch_nit_set(Ctx &c, int32_t *nit, int v) {
    hipLaunchKernelGGL(nit_kernel, dim3(1), dim3(64), 0, c.stream, nit, v, (const int *)nullptr);
    CPK_HIP(hipGetLastError());
}

void launch_nit_count(Ctx &c, int32_t *nit, const int *active) {
    hipLaunchKernelGGL(nit_kernel, dim3(1), dim3(64), 0, c.stream, nit, 0, active);
    CPK_HIP(hipGetLastError());
}

void launch_multi_state(Ctx &c, int32_t *state, int kc, int steps, const int *gate) {
    hipLaunchKernelGGL(multi_state_kernel, dim3(1), dim3(64), 0, c.stream, state, kc, steps, gate);
    CPK_HIP(hipGetLastError());
}

void launch_multi_resid(Ctx &c, const DMat &A, int kc, const double *X, int64_t ldx, const double *Yp, double *Rp,
                        const int32_t *state, double *part, bool norms, bool first) {
    if (!A.nblk || !A.nrows) return;
    if (norms)
        hipLaunchKernelGGL((multi_resid_kernel<true>), dim3((unsigned)A.nblk), dim3(kResidThreads), 0, c.stream, A.ptr.p,
                           A.col.p, A.val.p, A.blk.p, X, ldx, kc, Yp, Rp, state, part, first ? 1 : 0);
    else
        hipLaunchKernelGGL((multi_resid_kernel<false>), dim3((unsigned)A.nblk), dim3(kResidThreads), 0, c.stream, A.ptr.p,
                           A.col.p, A.val.p, A.blk.p, X, ldx, kc, Yp, Rp, state, part, 0);
    CPK_HIP(hipGetLastError());
}

void launch_multi_pred(Ctx &c, const double *part, int64_t nblk, double tol, int step, bool first, int32_t *state,
                       double *xn2) {
    hipLaunchKernelGGL(multi_pred_kernel, dim3(1), dim3(kPredThreads), 0, c.stream, part, nblk, tol, step, first ? 1 : 0,
                       state, xn2);
    CPK_HIP(hipGetLastError());
}

void launch_multi_store(Ctx &c, int64_t N, int kc, const double *Yp, double *Y, int64_t ldy, const int32_t *state,
                        int32_t *nit, const int *gate) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((N * KP + 255) / 256, 2048));
    hipLaunchKernelGGL(multi_store_kernel, dim3(grid), dim3(256), 0, c.stream, N, kc, Yp, Y, ldy, state, nit, gate);
    CPK_HIP(hipGetLastError());
}

}  // namespace cpk
