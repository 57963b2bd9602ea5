// ldl.hip -- numeric phase of the LDL' factorization on the device.
//
// Replaces the numeric half of [L,D,P] = ldl(op.A) (ops/opLDL2.m:82) and its refactorization
// when G, B or C change with the same sparsity (the IPM outer loop that rebuilds opLDL2 per
// iteration).  The host keeps the symbolic analysis (ordering, elimination tree, the pattern of
// every row of L, the sweep schedule; factor.cpp: ldl_factor(..., sym, numeric = false)).
//
// Up-looking by rows: row k of L solves L(0:k,0:k) y = Kp(perm, perm)(0:k, k) over its pattern
// (the reach of its Kp entries in the elimination tree) and D(k) = Kp(k,k) - sum l_ki y_i.  A
// row depends only on its descendants in the tree, so rows of one tree height run
// concurrently, one thread per row, one launch per height.  Each thread walks its row pattern in
// ascending column order and, for each column i, column i's entries above row k in ascending
// row order -- exactly the operations and order of the host's ldl_factor -- so L and D equal
// the host factorization bit for bit (-ffp-contract=off: no FMA is formed).
//
// The values land in CSC order (the exported factor's layout); ldl_fill_kernel then gathers
// them into the forward / backward sweep layouts of DFactor (schedule order, summation order of
// the exported factor) and D into schedule order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "dev.hpp"
#include "devutil.hpp"

namespace cpk {

// Static pivot perturbation (engine option pivot_min = delta > 0, the REG instantiations of the
// two row kernels): sgn[k] = +1 where perm[k] is a dof of the (1,1) block, -1 otherwise.  A
// pivot d with sgn[k] * d < delta is stored as d' = sgn[k] * delta and E[k] = d' - d (one
// subtraction; E is zero elsewhere); a NaN pivot fails every comparison and stays.  The host's
// ldl_factor applies the same rule with the same operations.
__device__ __forceinline__ double ldl_perturb(double d, int32_t k, double delta, const int8_t *__restrict__ sgn,
                                              double *__restrict__ E) {
    const bool neg = sgn[k] < 0;
    if ((neg ? -d : d) < delta) {
        const double dn = neg ? -delta : delta;
        E[k] = dn - d;
        d = dn;
    }
    return d;
}

template <bool REG>
__global__ __launch_bounds__(256) void ldl_rows_kernel(
    const int32_t *__restrict__ rows, int nrows, const int32_t *__restrict__ Rp, const int32_t *__restrict__ Rc,
    const int32_t *__restrict__ Rcsc, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
    double *__restrict__ Lx, double *__restrict__ D, double *__restrict__ Y, const int32_t *__restrict__ kp_ptr,
    const int32_t *__restrict__ kp_tgt, const uint32_t *__restrict__ kp_src, const double *__restrict__ kpv,
    int *__restrict__ bad, double delta, const int8_t *__restrict__ sgn, double *__restrict__ E) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows) return;
    const int32_t k = rows[idx];
    const int32_t t0 = Rp[k], t1 = Rp[k + 1];
    for (int32_t t = t0; t < t1; t++) Y[t] = 0.0;
    // seeds: y(i) += Kp(perm(k), perm(i)) for the row's entries left of and on the diagonal
    double d = 0.0;
    for (int32_t q = kp_ptr[k]; q < kp_ptr[k + 1]; q++) {
        const int32_t tg = kp_tgt[q];
        const double v = kpv[kp_src[q]];
        if (tg < 0) d += v;
        else Y[tg] += v;
    }
    for (int32_t t = t0; t < t1; t++) {
        const int32_t i = Rc[t];
        const double yi = Y[t];
        // y(j) -= L(j,i) * y(i) for column i's rows j < k; every such j is in row k's pattern
        // (right of i), found by merging the two ascending lists
        int32_t s = t + 1;
        const int32_t p1 = Lp[i + 1];
        for (int32_t p = Lp[i]; p < p1; p++) {
            const int32_t j = Li[p];
            if (j >= k) break;
            while (s < t1 && Rc[s] < j) s++;
            if (s >= t1 || Rc[s] != j) {  // impossible for a consistent symbolic analysis
                atomicOr(bad, 2);
                return;
            }
            Y[s] -= Lx[p] * yi;
        }
        const double lki = yi / D[i];
        d -= lki * yi;
        Lx[Rcsc[t]] = lki;
    }
    if constexpr (REG) d = ldl_perturb(d, k, delta, sgn, E);
    D[k] = d;
    if (d == 0.0 || !(d == d)) {
        atomicOr(bad, 1);
        atomicMin(bad + 1, k);
    }
}

// Long rows (a pattern of kLdlWaveMin or more columns): one wave per row.  The dense top of a
// factor (cvxqp1_m: the last ~470 rows form one chain of tree levels, each row's pattern the
// whole separator) made the one-thread-per-row kernel walk ~10 M dependent steps on one lane
// per level (seconds).  Here the row's y lives in LDS, and for each column i of the pattern (in
// the same ascending order) the lanes take column i's entries j < k together: each finds j's
// slot in the row's sorted pattern by binary search and subtracts L(j,i) y(i) -- distinct slots,
// so the updates of one column are independent, and every slot still receives its updates in
// ascending column order.  The seeds and the pivot run on lane 0 in the thread kernel's order.
// Same operations in the same order per value: bit-identical to the host factorization.
constexpr int kLdlWaveMin = 48;
template <bool REG>
__global__ __launch_bounds__(64) void ldl_rows_wave_kernel(
    const int32_t *__restrict__ rows, const int32_t *__restrict__ Rp, const int32_t *__restrict__ Rc,
    const int32_t *__restrict__ Rcsc, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
    double *__restrict__ Lx, double *__restrict__ D, const int32_t *__restrict__ kp_ptr,
    const int32_t *__restrict__ kp_tgt, const uint32_t *__restrict__ kp_src, const double *__restrict__ kpv,
    int *__restrict__ bad, double delta, const int8_t *__restrict__ sgn, double *__restrict__ E) {
    extern __shared__ __attribute__((aligned(16))) double ly[];  // y[n] | pattern columns[n]
    const int lane = threadIdx.x;
    const int32_t k = rows[blockIdx.x];
    const int32_t t0 = Rp[k], n = Rp[k + 1] - t0;
    int32_t *rc = reinterpret_cast<int32_t *>(ly + n);
    for (int32_t t = lane; t < n; t += 64) ly[t] = 0.0, rc[t] = Rc[t0 + t];
    __syncthreads();
    double d = 0.0;
    if (lane == 0)  // seeds in Kp's entry order (a slot may receive several)
        for (int32_t q = kp_ptr[k]; q < kp_ptr[k + 1]; q++) {
            const int32_t tg = kp_tgt[q];
            const double v = kpv[kp_src[q]];
            if (tg < 0) d += v;
            else ly[tg - t0] += v;
        }
    __syncthreads();
    for (int32_t t = 0; t < n; t++) {
        const int32_t i = rc[t];
        const double yi = ly[t];
        const int32_t p0 = Lp[i], p1 = Lp[i + 1];
        for (int32_t p = p0 + lane; p < p1; p += 64) {
            const int32_t j = Li[p];
            if (j < k) {  // column i's rows are ascending: those below k follow, and are skipped
                int32_t lo = t + 1, hi = n;  // first slot with rc >= j
                while (lo < hi) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (rc[mid] < j) lo = mid + 1;
                    else hi = mid;
                }
                if (lo >= n || rc[lo] != j) atomicOr(bad, 2);  // impossible for a consistent analysis
                else ly[lo] -= Lx[p] * yi;
            }
        }
        if (lane == 0) {
            const double lki = yi / D[i];
            d -= lki * yi;
            Lx[Rcsc[t0 + t]] = lki;
        }
        __syncthreads();
    }
    if (lane == 0) {
        if constexpr (REG) d = ldl_perturb(d, k, delta, sgn, E);
        D[k] = d;
        if (d == 0.0 || !(d == d)) {
            atomicOr(bad, 1);
            atomicMin(bad + 1, k);
        }
    }
}

// The factor report (host.hpp: FactorReport) in one pass over D, the signs and -- with HAS_E, a
// factorization under pivot_min > 0 -- E.  Every field is a count, an extreme or a lowest
// position, so the result does not depend on the order in which it is combined; it is combined in
// a fixed one all the same, devutil.hpp's grid reduction: each workgroup reduces in a fixed tree
// and publishes its partial, the last to arrive (the ticket) combines the partials in workgroup
// order.  No floating-point atomics; ties of min |d| go to the lowest position.
struct LdlPart {
    int64_t n_pos, n_neg, n_wrong, first_wrong, n_pert, argmin;  // first_wrong / argmin: INT64_MAX = none
    double min_abs, max_abs, max_shift;
};
constexpr int kLdlPartWords = 9;
constexpr int kLdlStatWords = 11;  // DLdl::stat: bad[2] in word 0, then the FactorReport
constexpr int64_t kLdlNone = INT64_MAX;
__device__ __forceinline__ LdlPart ldl_part_empty() {
    return LdlPart{0, 0, 0, kLdlNone, 0, kLdlNone, __builtin_inf(), 0.0, 0.0};
}
__device__ __forceinline__ void ldl_part_join(LdlPart &a, const LdlPart &b) {
    a.n_pos += b.n_pos, a.n_neg += b.n_neg, a.n_wrong += b.n_wrong, a.n_pert += b.n_pert;
    a.first_wrong = b.first_wrong < a.first_wrong ? b.first_wrong : a.first_wrong;
    if (b.min_abs < a.min_abs || (b.min_abs == a.min_abs && b.argmin < a.argmin)) a.min_abs = b.min_abs, a.argmin = b.argmin;
    a.max_abs = b.max_abs > a.max_abs ? b.max_abs : a.max_abs;
    a.max_shift = b.max_shift > a.max_shift ? b.max_shift : a.max_shift;
}
__device__ __forceinline__ LdlPart ldl_part_shfl(const LdlPart &a, int off) {
    LdlPart b;
    b.n_pos = __shfl_down((long long)a.n_pos, off, kWave), b.n_neg = __shfl_down((long long)a.n_neg, off, kWave);
    b.n_wrong = __shfl_down((long long)a.n_wrong, off, kWave);
    b.first_wrong = __shfl_down((long long)a.first_wrong, off, kWave);
    b.n_pert = __shfl_down((long long)a.n_pert, off, kWave), b.argmin = __shfl_down((long long)a.argmin, off, kWave);
    b.min_abs = __shfl_down(a.min_abs, off, kWave), b.max_abs = __shfl_down(a.max_abs, off, kWave);
    b.max_shift = __shfl_down(a.max_shift, off, kWave);
    return b;
}
// block-wide join in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ void ldl_part_block(LdlPart &v) {
    __shared__ LdlPart red[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) ldl_part_join(v, ldl_part_shfl(v, off));
    if (lane == 0) red[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / kWave; w++) ldl_part_join(v, red[w]);
    __syncthreads();
}
__device__ __forceinline__ void st_agent_i64(int64_t *p, int64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int64_t ld_agent_i64(const int64_t *p) {
    return __hip_atomic_load(const_cast<int64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// part: [gridDim.x][kLdlPartWords] 8-byte words; out: the FactorReport's first nine fields (the
// host fills pivot_min)
template <bool HAS_E>
__global__ __launch_bounds__(kBlock) void ldl_report_kernel(int64_t N, const double *__restrict__ D,
                                                            const int8_t *__restrict__ sgn, const double *__restrict__ E,
                                                            int64_t *__restrict__ part, unsigned *__restrict__ ticket,
                                                            int64_t *__restrict__ out) {
    __shared__ int s_last;
    LdlPart v = ldl_part_empty();
    for (int64_t k = blockIdx.x * (int64_t)kBlock + threadIdx.x; k < N; k += (int64_t)gridDim.x * kBlock) {
        const double d = D[k], a = fabs(d);  // positions ascend per thread: "<" keeps the lowest
        v.n_pos += d > 0, v.n_neg += d < 0;
        if ((sgn[k] < 0 ? -d : d) < 0) {
            v.n_wrong++;
            if (v.first_wrong == kLdlNone) v.first_wrong = k;
        }
        if (a < v.min_abs || v.argmin == kLdlNone) v.min_abs = a, v.argmin = k;
        if (a > v.max_abs) v.max_abs = a;
        if constexpr (HAS_E) {
            const double e = E[k];
            if (e != 0.0) {
                v.n_pert++;
                const double ae = fabs(e);
                if (ae > v.max_shift) v.max_shift = ae;
            }
        }
    }
    ldl_part_block(v);
    if (threadIdx.x == 0) {
        int64_t *p = part + (size_t)blockIdx.x * kLdlPartWords;
        st_agent_i64(p + 0, v.n_pos), st_agent_i64(p + 1, v.n_neg), st_agent_i64(p + 2, v.n_wrong);
        st_agent_i64(p + 3, v.first_wrong), st_agent_i64(p + 4, v.n_pert), st_agent_i64(p + 5, v.argmin);
        st_agent(reinterpret_cast<double *>(p + 6), v.min_abs), st_agent(reinterpret_cast<double *>(p + 7), v.max_abs);
        st_agent(reinterpret_cast<double *>(p + 8), v.max_shift);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = arrive_last(ticket);
    }
    __syncthreads();
    if (!s_last) return;
    LdlPart t = ldl_part_empty();
    for (unsigned b = threadIdx.x; b < gridDim.x; b += kBlock) {  // workgroup order per thread, then the tree
        const int64_t *p = part + (size_t)b * kLdlPartWords;
        LdlPart q;
        q.n_pos = ld_agent_i64(p + 0), q.n_neg = ld_agent_i64(p + 1), q.n_wrong = ld_agent_i64(p + 2);
        q.first_wrong = ld_agent_i64(p + 3), q.n_pert = ld_agent_i64(p + 4), q.argmin = ld_agent_i64(p + 5);
        q.min_abs = ld_agent(reinterpret_cast<const double *>(p + 6));
        q.max_abs = ld_agent(reinterpret_cast<const double *>(p + 7));
        q.max_shift = ld_agent(reinterpret_cast<const double *>(p + 8));
        ldl_part_join(t, q);
    }
    ldl_part_block(t);
    if (threadIdx.x == 0) {
        const bool none = t.argmin == kLdlNone;  // N == 0
        out[0] = t.n_pos, out[1] = t.n_neg, out[2] = t.n_wrong;
        out[3] = t.first_wrong == kLdlNone ? -1 : t.first_wrong;
        out[4] = t.n_pert, out[5] = none ? -1 : t.argmin;
        double *od = reinterpret_cast<double *>(out + 6);
        od[0] = none ? 0.0 : t.min_abs, od[1] = t.max_abs, od[2] = t.max_shift;
    }
}

// sweep layouts of DFactor from the CSC values, D into schedule order
__global__ void ldl_fill_kernel(int64_t nf, int64_t nb, int64_t N, const int32_t *__restrict__ fsrc,
                                const int32_t *__restrict__ bsrc, const int32_t *__restrict__ dsrc,
                                const double *__restrict__ Lx, const double *__restrict__ Dp, double *__restrict__ fval,
                                double *__restrict__ bval, double *__restrict__ Ds) {
    const int64_t n = nf > nb ? (nf > N ? nf : N) : (nb > N ? nb : N);
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        if (q < nf) fval[q] = Lx[fsrc[q]];
        if (q < nb) bval[q] = Lx[bsrc[q]];
        if (q < N) Ds[q] = Dp[dsrc[q]];
    }
}

// Kp's values from the user's blocks: src = (block << 40) | entry, block 0 = A11 (G),
// 1 = B (B or B' entries), 2 = C22
__global__ void kp_assemble_kernel(int64_t nnz, const int64_t *__restrict__ src, const double *__restrict__ a,
                                   const double *__restrict__ b, const double *__restrict__ c, double *__restrict__ kpv) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = src[q];
        const int64_t blk = s >> 40, e = s & ((int64_t(1) << 40) - 1);
        kpv[q] = blk == 0 ? a[e] : (blk == 1 ? b[e] : c[e]);
    }
}

void dldl_setup_sym(DLdl &d, const LdlSymbolic &sym, const Factor &f, int64_t n) {
    d.N = f.N;
    d.nnz = (int64_t)f.Li.size();
    d.lev_ptr = sym.lev_ptr;
    // within each height: the short rows first, then the long ones (ldl_rows_wave_kernel)
    std::vector<int32_t> rows = sym.lev_rows;
    const int64_t nlev = (int64_t)d.lev_ptr.size() - 1;
    d.lev_long.assign((size_t)std::max<int64_t>(nlev, 0), 0);
    d.max_long = 0;
    for (int64_t l = 0; l < nlev; l++) {
        auto b = rows.begin() + d.lev_ptr[l], e = rows.begin() + d.lev_ptr[l + 1];
        auto mid = std::stable_partition(b, e, [&](int32_t k) { return sym.Rp[k + 1] - sym.Rp[k] < kLdlWaveMin; });
        d.lev_long[l] = (int32_t)(mid - rows.begin());
        for (auto it = mid; it != e; ++it) d.max_long = std::max<int64_t>(d.max_long, sym.Rp[*it + 1] - sym.Rp[*it]);
    }
    SubClock clk;
    d.lev_rows.upload(rows);
    d.Rp.upload(sym.Rp);
    d.Rc.upload(sym.Rc);
    d.Rcsc.upload(sym.Rcsc);
    std::vector<int32_t> lp(f.Lp.begin(), f.Lp.end());
    d.Lp.upload(lp);
    d.Li.upload(f.Li);
    d.kp_ptr.upload(sym.kp_ptr);
    d.kp_tgt.upload(sym.kp_tgt);
    d.kp_src.upload(sym.kp_src);
    {
        std::vector<int8_t> sg((size_t)std::max<int64_t>(d.N, 1), 1);
        for (int64_t k = 0; k < d.N; k++) sg[k] = f.perm[k] < n ? 1 : -1;
        d.sgn.upload(sg);
    }
    d.rep_grid = (int)std::min<int64_t>(std::max<int64_t>((d.N + kBlock * 8 - 1) / (kBlock * 8), 1), 1024);
    d.rep_part.alloc((size_t)d.rep_grid * kLdlPartWords);
    d.rep_ticket.alloc(kTicketWords);
    CPK_HIP(hipMemset(d.rep_ticket.p, 0, d.rep_ticket.bytes()));
    d.Lx.alloc((size_t)std::max<int64_t>(d.nnz, 1));
    d.D.alloc((size_t)std::max<int64_t>(d.N, 1));
    d.Y.alloc((size_t)std::max<int64_t>(d.nnz, 1));
    d.stat.alloc(kLdlStatWords);
    d.sym_ready = true;
    clk.lap("ldl setup: symbolic uploads");
}

void dldl_setup_src(DLdl &d, const std::vector<int32_t> &fsrc, const std::vector<int32_t> &bsrc,
                    const std::vector<int32_t> &order) {
    if (!d.sym_ready) throw Error(CPK_ERR_ARGS, "internal: value sources before the symbolic data");
    d.nf = (int64_t)fsrc.size(), d.nb = (int64_t)bsrc.size();
    d.fsrc.upload(fsrc);
    d.bsrc.upload(bsrc);
    d.dsrc.upload(order);
    d.ready = true;
}

void dldl_setup(DLdl &d, const LdlSymbolic &sym, const Factor &f, int64_t n, const std::vector<int32_t> &fsrc,
                const std::vector<int32_t> &bsrc, const std::vector<int32_t> &order) {
    dldl_setup_sym(d, sym, f, n);
    dldl_setup_src(d, fsrc, bsrc, order);
}

void dldl_assemble_kp(Ctx &c, const DLdl &d, const double *a, const double *b, const double *cc, double *kpv) {
    const int64_t nnz = (int64_t)d.kp_from.n;
    if (!nnz) return;
    const int grid = (int)std::min<int64_t>((nnz + 255) / 256, 4096);
    hipLaunchKernelGGL(kp_assemble_kernel, dim3(grid), dim3(256), 0, c.stream, nnz, d.kp_from.p, a, b, cc, kpv);
    CPK_HIP(hipGetLastError());
}

// the two instantiations of a row kernel as one launch
template <class... A>
static void launch_rows(bool reg, dim3 grid, hipStream_t s, A... a) {
    if (reg) hipLaunchKernelGGL(ldl_rows_kernel<true>, grid, dim3(256), 0, s, a...);
    else hipLaunchKernelGGL(ldl_rows_kernel<false>, grid, dim3(256), 0, s, a...);
}
template <class... A>
static void launch_rows_wave(bool reg, dim3 grid, size_t lds, hipStream_t s, A... a) {
    if (reg) hipLaunchKernelGGL(ldl_rows_wave_kernel<true>, grid, dim3(64), lds, s, a...);
    else hipLaunchKernelGGL(ldl_rows_wave_kernel<false>, grid, dim3(64), lds, s, a...);
}

void dldl_numeric(Ctx &c, DLdl &d, const double *kpv, double *Lx, double *D, double *E, FactorReport &rep) {
    if (!d.ready) throw Error(CPK_ERR_ARGS, "internal: device factorization without its symbolic data");
    const double delta = c.opts.pivot_min;
    const bool reg = delta > 0;
    if (reg && !E) throw Error(CPK_ERR_ARGS, "internal: pivot perturbation without its shift buffer");
    // word 0: the kernels' bad[2] = {flags, lowest bad position}; then the report
    int64_t stat[kLdlStatWords] = {0};
    const int init[2] = {0, 0x7fffffff};
    std::memcpy(stat, init, sizeof init);
    CPK_HIP(hipMemcpyAsync(d.stat.p, stat, sizeof stat, hipMemcpyHostToDevice, c.stream));
    int *bad = reinterpret_cast<int *>(d.stat.p);
    if (reg && d.N) CPK_HIP(hipMemsetAsync(E, 0, (size_t)d.N * sizeof(double), c.stream));
    const int64_t nlev = (int64_t)d.lev_ptr.size() - 1;
    // long rows whose y does not fit in LDS stay on the thread kernel (global scratch)
    const size_t lds = 12 * (size_t)d.max_long;
    static const bool big_lds = hipFuncSetAttribute((const void *)ldl_rows_wave_kernel<false>,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
                                hipFuncSetAttribute((const void *)ldl_rows_wave_kernel<true>,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    const bool wave = d.max_long > 0 && (lds <= 64 * 1024 || (big_lds && lds <= 160 * 1024));
    for (int64_t l = 0; l < nlev; l++) {
        const int32_t a = d.lev_ptr[l], z = d.lev_ptr[l + 1], w = wave ? d.lev_long[l] : z;
        if (w > a)
            launch_rows(reg, dim3((unsigned)((w - a + 255) / 256)), c.stream, d.lev_rows.p + a, w - a, d.Rp.p, d.Rc.p,
                        d.Rcsc.p, d.Lp.p, d.Li.p, Lx, D, d.Y.p, d.kp_ptr.p, d.kp_tgt.p, d.kp_src.p, kpv, bad, delta,
                        d.sgn.p, E);
        if (z > w)
            launch_rows_wave(reg, dim3((unsigned)(z - w)), lds, c.stream, d.lev_rows.p + w, d.Rp.p, d.Rc.p, d.Rcsc.p,
                             d.Lp.p, d.Li.p, Lx, D, d.kp_ptr.p, d.kp_tgt.p, d.kp_src.p, kpv, bad, delta, d.sgn.p, E);
    }
    // the report: one pass over D (and E), read back with the pivot check below
    if (reg)
        hipLaunchKernelGGL(ldl_report_kernel<true>, dim3((unsigned)d.rep_grid), dim3(kBlock), 0, c.stream, d.N, D,
                           d.sgn.p, E, d.rep_part.p, d.rep_ticket.p, d.stat.p + 1);
    else
        hipLaunchKernelGGL(ldl_report_kernel<false>, dim3((unsigned)d.rep_grid), dim3(kBlock), 0, c.stream, d.N, D,
                           d.sgn.p, (const double *)nullptr, d.rep_part.p, d.rep_ticket.p, d.stat.p + 1);
    CPK_HIP(hipGetLastError());
    CPK_HIP(hipMemcpyAsync(stat, d.stat.p, sizeof stat, hipMemcpyDeviceToHost, c.stream));
    CPK_HIP(hipStreamSynchronize(c.stream));
    int hbad[2];
    std::memcpy(hbad, stat, sizeof hbad);
    if (hbad[0] & 2) throw Error(CPK_ERR_FACTOR, "ldl (device): inconsistent symbolic structure");
    if (hbad[0] & 1)
        throw Error(CPK_ERR_FACTOR, "ldl: zero or NaN pivot at position " + std::to_string(hbad[1]) +
                                        " (static 1x1 pivoting needs G > 0 on the nullspace and C > 0)");
    static_assert(sizeof(FactorReport) == (kLdlStatWords - 1) * sizeof(int64_t), "the report follows the bad word");
    std::memcpy(&rep, stat + 1, sizeof rep);  // the kernel wrote the first nine fields
    rep.pivot_min = delta;
}

void dldl_fill(Ctx &c, const DLdl &d, DFactor &dF) {
    const int64_t n = std::max(std::max(d.nf, d.nb), d.N);
    if (!n) return;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(ldl_fill_kernel, dim3(grid), dim3(256), 0, c.stream, d.nf, d.nb, d.N, d.fsrc.p, d.bsrc.p,
                       d.dsrc.p, d.Lx.p, d.D.p, dF.fval.p, dF.bval.p, dF.D.p);
    CPK_HIP(hipGetLastError());
}

__global__ void vmap_capture_kernel(const double *__restrict__ x, int64_t n, int32_t *__restrict__ map) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x)
        map[q] = (int32_t)x[q] - 1;  // exact: indices < 2^31
}

__global__ void vmap_fill_kernel(const int32_t *__restrict__ map, int64_t n, const double *__restrict__ src,
                                 double *__restrict__ x) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = map[q];
        x[q] = s >= 0 ? src[s] : 0.0;
    }
}

void vmap_capture(Ctx &c, const double *x, size_t n, DBuf<int32_t> &map) {
    map.alloc(n);
    if (!n) return;
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(vmap_capture_kernel, dim3(grid), dim3(256), 0, c.stream, x, (int64_t)n, map.p);
    CPK_HIP(hipGetLastError());
}

void vmap_fill(Ctx &c, const int32_t *map, size_t n, const double *src, double *x) {
    if (!n) return;
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(vmap_fill_kernel, dim3(grid), dim3(256), 0, c.stream, map, (int64_t)n, src, x);
    CPK_HIP(hipGetLastError());
}

void dldl_numeric_own(Ctx &c, DLdl &d, const double *kpv) {
    if (c.opts.pivot_min > 0 && !d.E.n) d.E.alloc((size_t)std::max<int64_t>(d.N, 1));
    else if (!(c.opts.pivot_min > 0) && d.E.n) d.E.zero(c.stream);
    dldl_numeric(c, d, kpv, d.Lx.p, d.D.p, c.opts.pivot_min > 0 ? d.E.p : nullptr, d.rep);
}

void dldl_commit_report(Ctx &c, DLdl &d, const double *E, const FactorReport &rep) {
    if (E) {
        if (!d.E.n) d.E.alloc((size_t)std::max<int64_t>(d.N, 1));
        if (d.N) CPK_HIP(hipMemcpyAsync(d.E.p, E, (size_t)d.N * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    } else if (d.E.n) {
        d.E.zero(c.stream);
    }
    d.rep = rep;
}

void dldl_factor(Ctx &c, DLdl &d, const double *kpv, DFactor &dF) {
    dldl_numeric_own(c, d, kpv);
    dldl_fill(c, d, dF);
}

}  // namespace cpk
