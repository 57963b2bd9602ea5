// adjoint.hip -- a sum of outer products sampled on a matrix handle's sparsity and handed back in
// the creating call's value order (cpk_mat_sample_outer[_device]): the value gradients of the
// adjoint solve (cpk_kkt_adjoint, DESIGN.md "The adjoint solve").  For every stored entry
// q = (i, j) of the canonical CSR
//     g_q = alpha * (u_0[i]*v_0[j] + u_1[i]*v_1[j] + ... + u_{k-1}[i]*v_{k-1}[j]),
// the sum from 0.0 over the separately rounded products in column order c = 0 ... k-1 (no FMA),
// alpha applied last with one rounding.  g_q then goes back through the handle's value map
// (host.hpp, ValueMap), the transpose of what set_values does with it: out[q] (identity),
// out[perm[q]] (perm), or every source src[t], t in [sptr[q], sptr[q + 1]) (the summands of a
// summed duplicate each have derivative 1).  Every caller entry is written exactly once: no
// atomics, and the values of the matrix are never read.
//
// The walk is spmv_stream's (spmv.hpp): a workgroup owns row blocks of DMat::blk, whose entries
// (<= kSpmvCap) are contiguous.  Its threads read their rows' pointers and write each row's local
// index over the row's span of an LDS table, one 16-bit word per entry; then consecutive lanes take
// consecutive entries, find the row in the table, gather u by row (neighbouring lanes share it) and
// v by column, and store.  A row longer than kSpmvCap sits alone in its block and needs no table.
// The index streams (columns, map) are read once per launch: non-temporal, so they leave the
// caches to the gathered vectors.
//
// The second half is the same pass for the blocks of the block adjoint (cpk_kkt_sample_multi,
// DESIGN.md "The block adjoint"): a transposing pass and sample_panel_kernel, the same sums bit for
// bit from interleaved operands.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev.hpp"
#include "devutil.hpp"

namespace cpk {

namespace {

enum { kMapIdentity = 0, kMapPerm = 1, kMapSum = 2 };

// KC > 0: that many columns, unrolled (the adjoint's k = 1 and k = 2); KC == 0: k at run time
template <int KC>
__device__ __forceinline__ double outer_sum(int k, const double *__restrict__ U, int64_t ldu,
                                            const double *__restrict__ V, int64_t ldv, int64_t row, int32_t c) {
    double s = 0.0;
    if constexpr (KC > 0) {
        double u[KC], v[KC];
#pragma unroll
        for (int j = 0; j < KC; j++) u[j] = U[row + j * ldu], v[j] = V[c + j * ldv];
#pragma unroll
        for (int j = 0; j < KC; j++) s = s + u[j] * v[j];
    } else {
        for (int j = 0; j < k; j++) s = s + U[row + j * ldu] * V[c + j * ldv];
    }
    return s;
}

// m0: perm (kMapPerm) or sptr (kMapSum); m1: src (kMapSum)
template <int MODE>
__device__ __forceinline__ void map_store(const uint32_t *__restrict__ m0, const uint32_t *__restrict__ m1, uint32_t e,
                                          double g, double *__restrict__ out) {
    if constexpr (MODE == kMapIdentity) {
        // a stream written once and read by nobody in this launch: non-temporal, as the index streams
        // are read (k = 2 on A at S10: 88 -> 77 us; a scattered store gains nothing from it)
        __builtin_nontemporal_store(g, out + e);
    } else if constexpr (MODE == kMapPerm) {
        out[__builtin_nontemporal_load(m0 + e)] = g;
    } else {
        const uint32_t t1 = __builtin_nontemporal_load(m0 + e + 1);
        for (uint32_t t = __builtin_nontemporal_load(m0 + e); t < t1; t++) out[__builtin_nontemporal_load(m1 + t)] = g;
    }
}

template <int KC, int MODE>
__global__ __launch_bounds__(kBlock) void sample_outer_kernel(const uint32_t *__restrict__ ptr,
                                                               const int32_t *__restrict__ col,
                                                               const int32_t *__restrict__ blk, int64_t nblk, int k,
                                                               const double *__restrict__ U, int64_t ldu,
                                                               const double *__restrict__ V, int64_t ldv, double alpha,
                                                               const uint32_t *__restrict__ m0,
                                                               const uint32_t *__restrict__ m1,
                                                               double *__restrict__ out) {
    __shared__ uint16_t srow[kSpmvCap];  // entry of the block -> its row, local to the block
    constexpr int EPT = kSpmvCap / kBlock, RPT = kSpmvMaxRows / kBlock;
    const int tid = threadIdx.x;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        if (b != blockIdx.x) __syncthreads();  // srow[] of the previous block fully consumed
        const int64_t r0 = blk[b], r1 = blk[b + 1];
        const uint32_t e0 = ptr[r0], e1 = ptr[r1];
        if (e1 == e0) continue;  // no entry (uniform over the workgroup); below, e1 - 1 and r1 - 1 exist
        if (e1 - e0 <= (uint32_t)kSpmvCap) {
            // every load is unconditional, on an index clamped into the block (a lane past the end
            // repeats the block's last entry or row and stores nothing), so a thread's loads of one
            // kind are all in flight at once: under `e < e1 ? load : 0` the compiler branched around
            // each load and waited for it before the next
            int32_t cc[EPT];
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const uint32_t e = e0 + tid + j * kBlock;
                cc[j] = __builtin_nontemporal_load(col + (e < e1 ? e : e1 - 1));
            }
            uint32_t pa[RPT], pb[RPT];
#pragma unroll
            for (int j = 0; j < RPT; j++) {
                const int64_t r = r0 + tid + j * kBlock < r1 ? r0 + tid + j * kBlock : r1 - 1;
                pa[j] = __builtin_nontemporal_load(ptr + r), pb[j] = __builtin_nontemporal_load(ptr + r + 1);
            }
#pragma unroll
            for (int j = 0; j < RPT; j++)
                if (r0 + tid + j * kBlock < r1)
                    for (uint32_t q = pa[j] - e0; q < pb[j] - e0; q++) srow[q] = (uint16_t)(tid + j * kBlock);
            __syncthreads();
            double s[EPT];
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const uint32_t q = tid + j * kBlock;
                s[j] = outer_sum<KC>(k, U, ldu, V, ldv, r0 + srow[q < e1 - e0 ? q : e1 - e0 - 1], cc[j]);
            }
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const uint32_t e = e0 + tid + j * kBlock;
                if (e < e1) map_store<MODE>(m0, m1, e, alpha * s[j], out);
            }
        } else {  // one long row (r1 == r0 + 1)
            for (uint32_t e = e0 + tid; e < e1; e += kBlock) {
                const double s = outer_sum<KC>(k, U, ldu, V, ldv, r0, __builtin_nontemporal_load(col + e));
                map_store<MODE>(m0, m1, e, alpha * s, out);
            }
        }
    }
}

// the workgroups resident at once (as spmv_grid sizes the SpMV's launch): each walks every
// grid-th row block
template <int KC, int MODE>
unsigned sample_grid(int64_t nblk) {
    static const int64_t resident = [] {
        int occ = 0, dev = 0, cus = 256;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)sample_outer_kernel<KC, MODE>, kBlock, 0) !=
                hipSuccess ||
            occ < 1)
            occ = 1;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return (int64_t)occ * cus;
    }();
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(nblk, resident));
}

template <int KC, int MODE>
void sample_launch(Ctx &c, const DMat &A, int k, const double *U, int64_t ldu, const double *V, int64_t ldv, double alpha,
                   const uint32_t *m0, const uint32_t *m1, double *out) {
    hipLaunchKernelGGL((sample_outer_kernel<KC, MODE>), dim3(sample_grid<KC, MODE>(A.nblk)), dim3(kBlock), 0, c.stream,
                       A.ptr.p, A.col.p, A.blk.p, A.nblk, k, U, ldu, V, ldv, alpha, m0, m1, out);
    CPK_HIP(hipGetLastError());
}

template <int MODE>
void sample_launch_k(Ctx &c, const DMat &A, int k, const double *U, int64_t ldu, const double *V, int64_t ldv, double alpha,
                     const uint32_t *m0, const uint32_t *m1, double *out) {
    if (k == 1) sample_launch<1, MODE>(c, A, k, U, ldu, V, ldv, alpha, m0, m1, out);
    else if (k == 2) sample_launch<2, MODE>(c, A, k, U, ldu, V, ldv, alpha, m0, m1, out);
    else sample_launch<0, MODE>(c, A, k, U, ldu, V, ldv, alpha, m0, m1, out);
}

// ---- the panel sampler: the gradients of a block of k columns (cpk_kkt_sample_multi) ----------------
// The operands are interleaved panels [panel][row][kMultiKP]: a row's 8 columns are 64 contiguous
// bytes, so an entry's row group and column group are four 16-byte loads each, where the run-time-k
// path above issues 2k 8-byte gathers, and gB's two pairs of operands need no 2k-column block.  The
// price is the transposing pass below, once per call; which path a call takes is measured
// (dev.hpp, sample_panel_rule).  The last panel is padded with +0.0: a padded product is +0.0, and
// a sum that starts at +0.0 is never -0.0 (x + -x and 0.0 + -0.0 round to +0.0), so adding it
// changes no bit.
typedef double d2 __attribute__((ext_vector_type(2)));
constexpr int kPackBlock = 256;

// PX[(p * N + i) * 8 + c] = X[i + (8 p + c) * ldx] (c beyond k: +0.0), PL the same from Lam; a thread
// takes one (panel, row): neighbouring lanes read neighbouring rows of each column and store their
// own 64 bytes as four vector stores
__global__ __launch_bounds__(kPackBlock) void pack_panels_kernel(int64_t N, int k, int64_t np,
                                                                  const double *__restrict__ X, int64_t ldx,
                                                                  const double *__restrict__ L, int64_t ldl,
                                                                  double *__restrict__ PX, double *__restrict__ PL) {
    constexpr int KP = kMultiKP;
    const int64_t stride = (int64_t)gridDim.x * kPackBlock;
    for (int64_t t = blockIdx.x * (int64_t)kPackBlock + threadIdx.x; t < np * N; t += stride) {
        const int64_t p = t / N, i = t - p * N;
        const int kc = (int)min((int64_t)KP, k - p * KP);
        double x[KP], l[KP];
#pragma unroll
        for (int c = 0; c < KP; c++) {
            const int64_t cc = p * KP + (c < kc ? c : kc - 1);  // clamped: every load in bounds and in flight
            const double xv = X[i + cc * ldx], lv = L[i + cc * ldl];
            x[c] = c < kc ? xv : 0.0, l[c] = c < kc ? lv : 0.0;
        }
        d2 *dx = reinterpret_cast<d2 *>(PX + t * KP), *dl = reinterpret_cast<d2 *>(PL + t * KP);
#pragma unroll
        for (int c = 0; c < KP / 2; c++) dx[c] = d2{x[2 * c], x[2 * c + 1]}, dl[c] = d2{l[2 * c], l[2 * c + 1]};
    }
}

struct Group8 {
    d2 v[kMultiKP / 2];
    __device__ __forceinline__ void load(const double *__restrict__ p) {
        const d2 *q = reinterpret_cast<const d2 *>(p);
#pragma unroll
        for (int c = 0; c < kMultiKP / 2; c++) v[c] = q[c];
    }
    __device__ __forceinline__ double operator[](int c) const { return c & 1 ? v[c >> 1].y : v[c >> 1].x; }
};

// NT == 1: g = alpha * sum_c U1_c[i] * V1_c[j]  (A and C);  NT == 2: each column adds U1_c[i] * V1_c[j]
// and then U2_c[i] * V2_c[j]  (B: the sum over the 2k columns [ly_0, xy_0, ...] x [xx_0, lx_0, ...]).
// G entries of a thread are in flight at once: G * NT * 2 groups of 8 doubles, 64 VGPRs of operands
// for either NT.  The running sums stay in registers across the panels, so any k is one launch.
template <int NT>
struct PanelOps {
    const double *U1, *V1, *U2, *V2;  // panel p of an array starts at p * pstride doubles
    int64_t pstride, np;
    __device__ __forceinline__ double sum(int64_t row, int32_t c) const {
        double s = 0.0;
        for (int64_t p = 0; p < np; p++) {
            const int64_t ro = p * pstride + row * kMultiKP, co = p * pstride + (int64_t)c * kMultiKP;
            Group8 u1, v1, u2, v2;
            u1.load(U1 + ro), v1.load(V1 + co);
            if constexpr (NT == 2) u2.load(U2 + ro), v2.load(V2 + co);
#pragma unroll
            for (int j = 0; j < kMultiKP; j++) {
                s = s + u1[j] * v1[j];
                if constexpr (NT == 2) s = s + u2[j] * v2[j];
            }
        }
        return s;
    }
    template <int G>
    __device__ __forceinline__ void sums(const int64_t (&row)[G], const int32_t (&c)[G], double (&s)[G]) const {
#pragma unroll
        for (int g = 0; g < G; g++) s[g] = 0.0;
        for (int64_t p = 0; p < np; p++) {
            Group8 u1[G], v1[G], u2[G], v2[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                const int64_t ro = p * pstride + row[g] * kMultiKP, co = p * pstride + (int64_t)c[g] * kMultiKP;
                u1[g].load(U1 + ro), v1[g].load(V1 + co);
                if constexpr (NT == 2) u2[g].load(U2 + ro), v2[g].load(V2 + co);
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
#pragma unroll
                for (int j = 0; j < kMultiKP; j++) {
                    s[g] = s[g] + u1[g][j] * v1[g][j];
                    if constexpr (NT == 2) s[g] = s[g] + u2[g][j] * v2[g][j];
                }
            }
        }
    }
};

// sample_outer_kernel's walk (row blocks of DMat::blk, the 16-bit LDS row table, clamped
// unconditional loads, non-temporal index streams and identity store, a long row alone in its block)
template <int NT, int MODE>
__global__ __launch_bounds__(kBlock) void sample_panel_kernel(const uint32_t *__restrict__ ptr,
                                                               const int32_t *__restrict__ col,
                                                               const int32_t *__restrict__ blk, int64_t nblk,
                                                               PanelOps<NT> ops, double alpha,
                                                               const uint32_t *__restrict__ m0,
                                                               const uint32_t *__restrict__ m1,
                                                               double *__restrict__ out) {
    __shared__ uint16_t srow[kSpmvCap];
    constexpr int EPT = kSpmvCap / kBlock, RPT = kSpmvMaxRows / kBlock, G = 2 / NT;
    const int tid = threadIdx.x;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        if (b != blockIdx.x) __syncthreads();  // srow[] of the previous block fully consumed
        const int64_t r0 = blk[b], r1 = blk[b + 1];
        const uint32_t e0 = ptr[r0], e1 = ptr[r1];
        if (e1 == e0) continue;  // uniform over the workgroup; below, e1 - 1 and r1 - 1 exist
        if (e1 - e0 <= (uint32_t)kSpmvCap) {
            int32_t cc[EPT];
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const uint32_t e = e0 + tid + j * kBlock;
                cc[j] = __builtin_nontemporal_load(col + (e < e1 ? e : e1 - 1));
            }
            uint32_t pa[RPT], pb[RPT];
#pragma unroll
            for (int j = 0; j < RPT; j++) {
                const int64_t r = r0 + tid + j * kBlock < r1 ? r0 + tid + j * kBlock : r1 - 1;
                pa[j] = __builtin_nontemporal_load(ptr + r), pb[j] = __builtin_nontemporal_load(ptr + r + 1);
            }
#pragma unroll
            for (int j = 0; j < RPT; j++)
                if (r0 + tid + j * kBlock < r1)
                    for (uint32_t q = pa[j] - e0; q < pb[j] - e0; q++) srow[q] = (uint16_t)(tid + j * kBlock);
            __syncthreads();
#pragma unroll
            for (int j0 = 0; j0 < EPT; j0 += G) {
                if ((uint32_t)(j0 * kBlock) >= e1 - e0) break;  // no thread has an entry from here on (uniform)
                int64_t row[G];
                int32_t cg[G];
                double s[G];
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const uint32_t q = tid + (j0 + g) * kBlock;
                    row[g] = r0 + srow[q < e1 - e0 ? q : e1 - e0 - 1], cg[g] = cc[j0 + g];
                }
                ops.template sums<G>(row, cg, s);
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const uint32_t e = e0 + tid + (j0 + g) * kBlock;
                    if (e < e1) map_store<MODE>(m0, m1, e, alpha * s[g], out);
                }
            }
        } else {  // one long row (r1 == r0 + 1)
            for (uint32_t e = e0 + tid; e < e1; e += kBlock)
                map_store<MODE>(m0, m1, e, alpha * ops.sum(r0, __builtin_nontemporal_load(col + e)), out);
        }
    }
}

template <int NT, int MODE>
void panel_launch(Ctx &c, const DMat &A, const PanelOps<NT> &ops, double alpha, const uint32_t *m0, const uint32_t *m1,
                  double *out) {
    static const int64_t resident = [] {
        int occ = 0, dev = 0, cus = 256;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)sample_panel_kernel<NT, MODE>, kBlock, 0) !=
                hipSuccess ||
            occ < 1)
            occ = 1;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return (int64_t)occ * cus;
    }();
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(A.nblk, resident));
    hipLaunchKernelGGL((sample_panel_kernel<NT, MODE>), dim3(grid), dim3(kBlock), 0, c.stream, A.ptr.p, A.col.p, A.blk.p,
                       A.nblk, ops, alpha, m0, m1, out);
    CPK_HIP(hipGetLastError());
}

template <int NT>
void panel_launch_mode(Ctx &c, const DMat &A, const ValueMap &vm, const DValueMap &dm, const PanelOps<NT> &ops,
                       double alpha, double *out) {
    const bool sum = !vm.identity && !vm.sptr.empty();
    if (vm.identity) panel_launch<NT, kMapIdentity>(c, A, ops, alpha, nullptr, nullptr, out);
    else if (sum) panel_launch<NT, kMapSum>(c, A, ops, alpha, dm.sptr.p, dm.src.p, out);
    else panel_launch<NT, kMapPerm>(c, A, ops, alpha, dm.perm.p, nullptr, out);
}

void check_device_map(const DMat &A, const ValueMap &vm, const DValueMap &dm) {
    // the maps hold one entry per stored entry (perm: nnz, sptr: nnz + 1); every destination index
    // is below vm.count, the length the caller's array was checked against
    const bool sum = !vm.identity && !vm.sptr.empty();
    if (!vm.identity &&
        (!dm.ready || (sum ? dm.sptr.n != (size_t)A.nnz + 1 || dm.src.n != (size_t)vm.count : dm.perm.n != (size_t)A.nnz)))
        throw Error(CPK_ERR_ARGS, "sample_outer: the device value map does not match the matrix");
}

}  // namespace

void launch_pack_panels(Ctx &c, int64_t N, int64_t k, const double *X, int64_t ldx, const double *L, int64_t ldl,
                        double *PX, double *PL) {
    const int64_t np = panel_count(k);
    if (N <= 0 || np <= 0) return;
    const int grid = (int)std::min<int64_t>((np * N + kPackBlock - 1) / kPackBlock, 8192);
    hipLaunchKernelGGL(pack_panels_kernel, dim3(grid), dim3(kPackBlock), 0, c.stream, N, (int)k, np, X, ldx, L, ldl, PX, PL);
    CPK_HIP(hipGetLastError());
}

void launch_sample_panel(Ctx &c, const DMat &A, const ValueMap &vm, const DValueMap &dm, int64_t k, int64_t pstride,
                         const double *U1, const double *V1, const double *U2, const double *V2, double alpha,
                         double *out) {
    if (A.nnz <= 0) return;  // no stored entry, so no entry of the creating call either
    if (k > INT32_MAX) throw Error(CPK_ERR_DIM, "sample_panel: k out of range");
    check_device_map(A, vm, dm);
    if (U2) panel_launch_mode<2>(c, A, vm, dm, PanelOps<2>{U1, V1, U2, V2, pstride, panel_count(k)}, alpha, out);
    else panel_launch_mode<1>(c, A, vm, dm, PanelOps<1>{U1, V1, nullptr, nullptr, pstride, panel_count(k)}, alpha, out);
}

void launch_sample_outer(Ctx &c, const DMat &A, const ValueMap &vm, const DValueMap &dm, int64_t k, const double *U,
                         int64_t ldu, const double *V, int64_t ldv, double alpha, double *out) {
    if (A.nnz <= 0) return;  // no stored entry, so no entry of the creating call either
    if (k > INT32_MAX) throw Error(CPK_ERR_DIM, "sample_outer: k out of range");
    check_device_map(A, vm, dm);
    const bool sum = !vm.identity && !vm.sptr.empty();
    if (vm.identity) sample_launch_k<kMapIdentity>(c, A, (int)k, U, ldu, V, ldv, alpha, nullptr, nullptr, out);
    else if (sum) sample_launch_k<kMapSum>(c, A, (int)k, U, ldu, V, ldv, alpha, dm.sptr.p, dm.src.p, out);
    else sample_launch_k<kMapPerm>(c, A, (int)k, U, ldu, V, ldv, alpha, dm.perm.p, nullptr, out);
}

}  // namespace cpk
