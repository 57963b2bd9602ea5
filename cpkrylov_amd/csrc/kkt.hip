// kkt.hip -- the saddle-point operator K = [A B'; B -C] itself (cpk_kkt_*): its value refresh from
// the three handles' device values, the product y = K*z and the true residual r = b - K*z with its
// four sums of squares, split at row n.
//
// K is a DMat in assemble_kp's entry order, so the product and the residual are spmv_stream
// (spmv.hpp) with an epilogue: row i sums its separately rounded products in entry order from 0.0
// (no FMA), y_i = s_i, r_i = b_i - s_i.  The reducing epilogue keeps the sums of r(1:n)^2,
// r(n+1:N)^2, b(1:n)^2 and b(n+1:N)^2 per thread and finishes them in the last workgroup
// (devutil.hpp grid_sum; xacc.hpp under exact_dots), as EpiResidNorm does for the refinement
// residual.  A row reads b_i (Epi::pre) before it writes r_i, so r may overwrite b.
// A block of columns can take the panel path instead: kkt_panel_kernel forms R for up to 8 columns
// with K streamed once, and kkt_sums_kernel takes each column's sums from its r and b in the
// single-column pass's order, so a column has the same bits on either path (kkt_driver.cpp routes).
// kkt_resid_exact_kernel forms the exactly rounded residual (cpk_kkt_residual_exact): the exact row
// sum rounded once, whose sums of squares kkt_sums_kernel then takes from the stored r.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "dev.hpp"
#include "devutil.hpp"
#include "spmv.hpp"
#include "xacc.hpp"

namespace cpk {

namespace {

constexpr int kGatherBlock = 256;

// K's stored entry q <- entry src[q] of the concatenation [A's values; B's values; C's values]
// (the stored orders of the handles), the C block negated.  The map is read once per refresh:
// non-temporal, as set_values_perm_kernel reads its own.
__global__ __launch_bounds__(kGatherBlock) void kkt_gather_kernel(const uint32_t *__restrict__ src, int64_t nnz,
                                                                   const double *__restrict__ va, uint32_t na,
                                                                   const double *__restrict__ vb, uint32_t nb,
                                                                   const double *__restrict__ vc,
                                                                   double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kGatherBlock;
    for (int64_t q = blockIdx.x * (int64_t)kGatherBlock + threadIdx.x; q < nnz; q += stride) {
        const uint32_t s = __builtin_nontemporal_load(src + q);
        double v;
        if (s < na) v = va[s];
        else if (s - na < nb) v = vb[s - na];
        else v = -vc[s - na - nb];
        out[q] = v;
    }
}

struct EpiKktStore {
    double *y;
    __device__ bool skip() const { return false; }
    __device__ const double *xvec(const double *x) const { return x; }
    __device__ double pre(int64_t) const { return 0.0; }
    __device__ void row(int64_t r, double acc, double) { y[r] = acc; }
    __device__ void finish() {}
};

struct EpiKktResid {  // r = b - K*z
    const double *b;
    double *r;
    __device__ bool skip() const { return false; }
    __device__ const double *xvec(const double *x) const { return x; }
    __device__ double pre(int64_t i) const { return b[i]; }
    __device__ void row(int64_t i, double acc, double bi) { r[i] = bi - acc; }
    __device__ void finish() {}
};

// r = b - K*z (r null: not stored) and norms[0..3] = sum r(1:n)^2, sum r(n+1:N)^2, sum b(1:n)^2,
// sum b(n+1:N)^2: fixed-order sums (double) or the exact ones (XAcc)
template <class A = double>
struct EpiKktNorm {
    const double *b;
    double *r;
    int64_t n;
    double *norms;
    RedBuf rb;
    // A thread meets its rows in ascending order (spmv_stream: its row blocks ascend, and its rows
    // within one), so it keeps one live pair of sums: once it crosses row n the pair of the x rows
    // is set aside and the pair of the y rows starts.  Two accumulation sites, as EpiResidNorm has.
    A cr{}, cb{}, xr{}, xb{};
    bool low = true;
    static constexpr int kWaves = std::is_same<A, XAcc>::value ? 4 : 5;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ const double *xvec(const double *x) {
        acc_init(cr, rb.xsub, 0, 4), acc_init(cb, rb.xsub, 2, 4);
        return x;
    }
    __device__ __forceinline__ void cross() {
        xr = cr, xb = cb;
        acc_init(cr, rb.xsub, 1, 4), acc_init(cb, rb.xsub, 3, 4);
        low = false;
    }
    __device__ __forceinline__ double pre(int64_t i) const { return b[i]; }
    __device__ __forceinline__ void sums(int64_t i, double ri, double bi) {
        if (low && i >= n) cross();
        dadd(cr, ri, ri);
        dadd(cb, bi, bi);
    }
    __device__ __forceinline__ void row(int64_t i, double acc, double bi) {
        const double ri = bi - acc;
        if (r) r[i] = ri;
        sums(i, ri, bi);
    }
    __device__ __forceinline__ void finish() {
        if (low) cross();  // no y row met: empty sums there
        A v[4] = {xr, cr, xb, cb};
        double tot[4];
        if (grid_sum<4>(v, rb, tot) && threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) norms[j] = tot[j];
        }
    }
};

// The four sums of a column whose r is already in memory (the panel path), in the single-column
// pass's order exactly: the same grid, the same walk over K's row blocks, thread t of a block's
// workgroup taking rows r0 + t, r0 + t + kBlock, ... (the thread that spmv_stream hands those
// rows; a long row sits alone in its block: thread 0), the same accumulation sites and finish.
template <class A>
__global__ __launch_bounds__(kBlock) void kkt_sums_kernel(const int32_t *__restrict__ blk, int64_t nblk,
                                                           const double *__restrict__ rv, EpiKktNorm<A> epi) {
    constexpr int RPT = kSpmvMaxRows / kBlock;
    epi.xvec(nullptr);
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t r0 = blk[b], r1 = blk[b + 1];
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const int64_t i = r0 + threadIdx.x + j * kBlock;
            if (i < r1) epi.sums(i, rv[i], epi.b[i]);
        }
    }
    epi.finish();
}

// R(:, j) = B(:, j) - K * Z(:, j) for the kc <= kMultiKP columns of a panel, K streamed once: one
// workgroup per row block of K (DMat::blk), its (col, val) staged in LDS as multi_resid_kernel
// stages them; a thread owns a row for all columns (the rows spmv_stream hands it) and adds the
// separately rounded products in entry order from 0.0, so every column is spmv_stream's row sum
// bit for bit.  The operands are column-major with the caller's leading dimensions, gathered
// strided: neighbouring lanes hold neighbouring rows, whose columns are neighbours in each of the
// kc vectors.  A row longer than kSpmvCap sits alone in its block: its products are staged chunk
// by chunk, [entry][column], and thread j sums column j in entry order.  Columns never mix.
constexpr int kPanelLongChunk = kSpmvCap / kMultiKP;
__global__ __launch_bounds__(kBlock) void kkt_panel_kernel(const uint32_t *__restrict__ ptr,
                                                            const int32_t *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            const int32_t *__restrict__ blk, int kc, const double *Z,
                                                            int64_t ldz, const double *B, int64_t ldb, double *R,
                                                            int64_t ldr) {
    constexpr int KP = kMultiKP;
    __shared__ double sv[kSpmvCap];
    __shared__ int32_t sc[kSpmvCap];
    const int tid = threadIdx.x;
    const int64_t r0 = blk[blockIdx.x], r1 = blk[blockIdx.x + 1];
    const uint32_t e0 = ptr[r0], e1 = ptr[r1];
    if (e1 - e0 <= (uint32_t)kSpmvCap) {
        for (uint32_t e = tid; e < e1 - e0; e += kBlock) {
            sc[e] = __builtin_nontemporal_load(col + e0 + e);  // streamed once per panel
            sv[e] = __builtin_nontemporal_load(val + e0 + e);
        }
        __syncthreads();
        for (int64_t row = r0 + tid; row < r1; row += kBlock) {
            double acc[KP];
#pragma unroll
            for (int j = 0; j < KP; j++) acc[j] = 0.0;
            const uint32_t q1 = ptr[row + 1] - e0;
            for (uint32_t e = ptr[row] - e0; e < q1; e++) {
                const double v = sv[e];
                const double *z = Z + sc[e];
#pragma unroll
                for (int j = 0; j < KP; j++)
                    if (j < kc) acc[j] += v * z[(int64_t)j * ldz];
            }
#pragma unroll
            for (int j = 0; j < KP; j++)
                if (j < kc) R[row + (int64_t)j * ldr] = B[row + (int64_t)j * ldb] - acc[j];
        }
    } else {
        double acc = 0.0;  // one long row (r1 == r0 + 1); thread j < kc sums column j
        for (uint32_t c0 = e0; c0 < e1; c0 += kPanelLongChunk) {
            const uint32_t n = min(e1 - c0, (uint32_t)kPanelLongChunk);
            for (uint32_t i = tid; i < n * KP; i += kBlock) {
                const int j = (int)(i % KP);
                sv[i] = j < kc ? val[c0 + i / KP] * Z[col[c0 + i / KP] + (int64_t)j * ldz] : 0.0;
            }
            __syncthreads();
            if (tid < kc)
                for (uint32_t e = 0; e < n; e++) acc += sv[e * KP + tid];
            __syncthreads();
        }
        if (tid < kc) R[r0 + (int64_t)tid * ldr] = B[r0 + (int64_t)tid * ldb] - acc;
    }
}

// ---- the exactly rounded residual: r_i = RN(b_i - sum_e K_ie z_col(e)), the sum exact ----------
//
// The terms of row i are b_i and the TwoProd pairs p = -v*z, q = fma(-v, z, -p) of its entries (p + q
// = -v*z unless the product under- or overflows: xacc.hpp's caveat).  A thread sums a row's terms
// into an expansion of kXK doubles by XAcc's TwoSum cascade, level 0 kept at or below 2^1023 as
// XAcc::add keeps it.  While no term is refused for that bound (or as non-finite) and no cascade
// leaves a residue, t0 + t1 + t2 IS the exact sum, and xround3 rounds it once.  Any other row is
// summed again as fixed-point digits in LDS (xacc.hpp's layout, which holds any sum of finite
// doubles and counts non-finite terms) and rounded by xround: the same value where both apply, so
// the route cannot change a bit.  An exact zero is +0.0 on either route (xround's).

// the digits of x added into d[0..kXW) in LDS (xdeposit's words, 8-byte LDS atomics)
__device__ inline void xdeposit_lds(int64_t *d, double x) {
    if (x == 0) return;
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
    const int E = (int)((bits >> 52) & 0x7ff);
    unsigned long long *u = reinterpret_cast<unsigned long long *>(d);
    if (E == 0x7ff) {  // inf / nan: the sum is NaN
        atomicAdd(u + kXW - 1, 1ull);
        return;
    }
    uint64_t mant = bits & ((1ull << 52) - 1);
    int off = 0;
    if (E) mant |= 1ull << 52, off = E - 1;
    const int i = off >> 5, sh = off & 31;  // off <= 2045: words i .. i + 2 <= 65
    const uint64_t lo = mant << sh, hi = sh ? mant >> (64 - sh) : 0;
    int64_t c0 = (int64_t)(lo & 0xffffffffu), c1 = (int64_t)(lo >> 32), c2 = (int64_t)hi;
    if (bits >> 63) c0 = -c0, c1 = -c1, c2 = -c2;
    if (c0) atomicAdd(u + i, (unsigned long long)c0);
    if (c1) atomicAdd(u + i + 1, (unsigned long long)c1);
    if (c2) atomicAdd(u + i + 2, (unsigned long long)c2);
}

// x + y rounded to odd: the TwoSum's error decides; an inexact sum with an even significand moves
// one place toward the exact value, which makes it odd (a zero sum is exact)
__device__ __forceinline__ double add_round_odd(double x, double y) {
    const double s = x + y, bb = s - x, err = (x - (s - bb)) + (y - bb);
    long long sb = __double_as_longlong(s);
    if (err != 0 && !(sb & 1)) sb += ((err > 0) == (s > 0)) ? 1 : -1;
    return __longlong_as_double(sb);
}

// RN(t0 + t1 + t2) for any three doubles whose sums stay finite (Boldo & Melquiond 2008, the
// correctly rounded sum of three numbers): two error-free additions, one addition rounded to odd,
// one rounded to nearest
__device__ __forceinline__ double xround3(double t0, double t1, double t2) {
    const double uh = t1 + t2, ub = uh - t1, ul = (t1 - (uh - ub)) + (t2 - ub);
    const double th = t0 + uh, tb = th - t0, tl = (t0 - (th - tb)) + (uh - tb);
    const double res = th + add_round_odd(tl, ul);
    return res == 0 ? 0.0 : res;
}

// one term into a row's expansion; false once the expansion no longer holds the exact sum
__device__ __forceinline__ bool xrow_add(XAcc &a, double x) {
    const bool fin = fabs(a.t[0] + x) <= XAcc::kXTop;
    return (a.cascade(fin ? x : 0.0) == 0) & fin;
}
// a TwoProd pair with one range test (XAcc::add_prod's argument)
__device__ __forceinline__ bool xrow_add_pair(XAcc &a, double p, double q) {
    const bool fin = fabs(a.t[0] + p) <= XAcc::kXTop;
    const double rp = a.cascade(fin ? p : 0.0), rq = a.cascade(fin ? q : 0.0);
    return (rp == 0) & (rq == 0) & fin;
}

// The walk over K's row blocks is spmv_stream's: phase 1 streams (col, val) coalesced, gathers z and
// stages every entry's TwoProd pair in LDS; phase 2 gives each thread whole rows.  Rows whose
// expansion gave up are then summed one at a time by the whole workgroup in the digits (the lowest
// such row elected through s_next); a row longer than kSpmvCap sits alone in its block and goes to
// the digits directly, each thread's share through an expansion of its own.  A row reads b_i before
// its r_i is written and no other row reads it, so r may be b.
__global__ __launch_bounds__(kBlock) void kkt_resid_exact_kernel(const uint32_t *__restrict__ ptr,
                                                                  const int32_t *__restrict__ col,
                                                                  const double *__restrict__ val,
                                                                  const int32_t *__restrict__ blk, int64_t nblk,
                                                                  const double *__restrict__ z, const double *b,
                                                                  double *r) {
    __shared__ double sp[kSpmvCap], sq[kSpmvCap];
    __shared__ int64_t dig[kXW];
    __shared__ int s_next;
    const int tid = threadIdx.x;
    for (int64_t bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        if (bi != blockIdx.x) __syncthreads();  // sp[], sq[], dig[] of the previous block consumed
        const int64_t r0 = blk[bi], r1 = blk[bi + 1];
        const uint32_t e0 = ptr[r0], e1 = ptr[r1];
        if (e1 - e0 <= (uint32_t)kSpmvCap) {
            constexpr int EPT = kSpmvCap / kBlock, RPT = kSpmvMaxRows / kBlock;
            int32_t cc[EPT];
            double vv[EPT], xv[EPT];
            uint32_t pa[RPT], pb[RPT];
            double pr[RPT];
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const uint32_t e = e0 + tid + j * kBlock;
                cc[j] = e < e1 ? __builtin_nontemporal_load(col + e) : 0;
                vv[j] = e < e1 ? __builtin_nontemporal_load(val + e) : 0.0;
            }
#pragma unroll
            for (int j = 0; j < RPT; j++) {
                const int64_t row = r0 + tid + j * kBlock;
                if (row < r1) pa[j] = ptr[row], pb[j] = ptr[row + 1], pr[j] = b[row];
            }
#pragma unroll
            for (int j = 0; j < EPT; j++) xv[j] = z[cc[j]];
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const uint32_t e = e0 + tid + j * kBlock;
                if (e < e1) {
                    const double p = -vv[j] * xv[j];
                    sp[e - e0] = p;
                    sq[e - e0] = fma(-vv[j], xv[j], -p);
                }
            }
            __syncthreads();
            unsigned slow = 0;  // bit j: this thread's row j goes to the digits
#pragma unroll
            for (int j = 0; j < RPT; j++) {
                const int64_t row = r0 + tid + j * kBlock;
                if (row < r1) {
                    XAcc a;
                    a.init(nullptr);
                    bool ok = xrow_add(a, pr[j]);
                    for (uint32_t e = pa[j] - e0; e < pb[j] - e0; e++) ok &= xrow_add_pair(a, sp[e], sq[e]);
                    if (ok) r[row] = xround3(a.t[0], a.t[1], a.t[2]);
                    else slow |= 1u << j;
                }
            }
            if (__syncthreads_or((int)slow)) {
                for (;;) {
                    if (tid == 0) s_next = INT_MAX;
                    __syncthreads();
                    if (slow) atomicMin(&s_next, tid + (__ffs((int)slow) - 1) * kBlock);
                    __syncthreads();
                    const int cur = s_next;
                    if (cur == INT_MAX) break;
                    for (int w = tid; w < kXW; w += kBlock) dig[w] = 0;
                    __syncthreads();
                    const int64_t row = r0 + cur;
                    const uint32_t qb = ptr[row + 1] - e0;
                    for (uint32_t e = ptr[row] - e0 + tid; e < qb; e += kBlock) {
                        xdeposit_lds(dig, sp[e]);
                        xdeposit_lds(dig, sq[e]);
                    }
                    if (tid == 0) xdeposit_lds(dig, b[row]);
                    __syncthreads();
                    if (tid == 0) r[row] = xround(dig);
                    if (cur % kBlock == tid) slow &= ~(1u << (cur / kBlock));
                }
            }
        } else {  // one long row (r1 == r0 + 1)
            for (int w = tid; w < kXW; w += kBlock) dig[w] = 0;
            __syncthreads();
            XAcc a;
            a.init(nullptr);
            for (uint32_t e = e0 + tid; e < e1; e += kBlock) {
                const double v = val[e], x = z[col[e]];
                const double p = -v * x, q = fma(-v, x, -p);
                const bool fin = fabs(a.t[0] + p) <= XAcc::kXTop;
                const double rp = a.cascade(fin ? p : 0.0), rq = a.cascade(fin ? q : 0.0);
                if (rp != 0 || !fin) xdeposit_lds(dig, fin ? rp : p);
                if (rq != 0 || !fin) xdeposit_lds(dig, fin ? rq : q);
            }
#pragma unroll
            for (int k = 0; k < kXK; k++) xdeposit_lds(dig, a.t[k]);
            if (tid == 0) xdeposit_lds(dig, b[r0]);
            __syncthreads();
            if (tid == 0) r[r0] = xround(dig);
        }
    }
}

template <class Epi>
void kkt_launch(Ctx &c, const DMat &K, const double *z, const Epi &e, unsigned grid) {
    hipLaunchKernelGGL((spmv_stream<Epi, false>), dim3(grid), dim3(kBlock), 0, c.stream, K.ptr.p, K.col.p, K.val.p,
                       K.blk.p, K.nblk, z, (int64_t)0, e, (const double *)nullptr, (int64_t)0);
    CPK_HIP(hipGetLastError());
}

template <class A>
void kkt_launch_norm(Ctx &c, const DMat &K, int64_t n, const double *z, const double *b, double *r, double *norms) {
    const unsigned grid = spmv_grid<EpiKktNorm<A>, false>(K.nblk);
    c.ensure_partials(std::max<size_t>((size_t)grid * 4, 4096));
    kkt_launch(c, K, z, EpiKktNorm<A>{b, r, n, norms, red_buf(c)}, grid);
}

}  // namespace

void launch_kkt_gather(Ctx &c, const uint32_t *src, int64_t nnz, const double *va, int64_t na, const double *vb,
                       int64_t nb, const double *vc, double *out) {
    if (nnz <= 0) return;
    const int grid = (int)std::min<int64_t>((nnz + kGatherBlock - 1) / kGatherBlock, 8192);
    hipLaunchKernelGGL(kkt_gather_kernel, dim3(grid), dim3(kGatherBlock), 0, c.stream, src, nnz, va, (uint32_t)na, vb,
                       (uint32_t)nb, vc, out);
    CPK_HIP(hipGetLastError());
}

void launch_kkt_apply(Ctx &c, const DMat &K, const double *z, double *y) {
    if (!K.nrows) return;
    kkt_launch(c, K, z, EpiKktStore{y}, spmv_grid<EpiKktStore, false>(K.nblk));
}

void launch_kkt_resid(Ctx &c, const DMat &K, int64_t n, const double *z, const double *b, double *r, double *norms) {
    if (!K.nrows) {  // no rows: empty sums
        if (norms) CPK_HIP(hipMemsetAsync(norms, 0, 4 * sizeof(double), c.stream));
        return;
    }
    if (!norms) {
        if (r) kkt_launch(c, K, z, EpiKktResid{b, r}, spmv_grid<EpiKktResid, false>(K.nblk));
    } else if (c.exact()) {
        kkt_launch_norm<XAcc>(c, K, n, z, b, r, norms);
    } else {
        kkt_launch_norm<double>(c, K, n, z, b, r, norms);
    }
}

template <class A>
static void kkt_launch_sums(Ctx &c, const DMat &K, int64_t n, const double *r, const double *b, double *norms) {
    const unsigned grid = spmv_grid<EpiKktNorm<A>, false>(K.nblk);  // the single-column pass's grid
    c.ensure_partials(std::max<size_t>((size_t)grid * 4, 4096));
    hipLaunchKernelGGL((kkt_sums_kernel<A>), dim3(grid), dim3(kBlock), 0, c.stream, K.blk.p, K.nblk, r,
                       EpiKktNorm<A>{b, nullptr, n, norms, red_buf(c)});
    CPK_HIP(hipGetLastError());
}

void launch_kkt_sums(Ctx &c, const DMat &K, int64_t n, const double *r, const double *b, double *norms) {
    if (!K.nrows) {
        CPK_HIP(hipMemsetAsync(norms, 0, 4 * sizeof(double), c.stream));
        return;
    }
    if (c.exact()) kkt_launch_sums<XAcc>(c, K, n, r, b, norms);
    else kkt_launch_sums<double>(c, K, n, r, b, norms);
}

void launch_kkt_resid_exact(Ctx &c, const DMat &K, const double *z, const double *b, double *r) {
    if (!K.nrows || !K.nblk) return;
    // the resident workgroups, each walking every grid-th row block (spmv_grid's rule)
    static const int64_t resident = [] {
        int occ = 0, dev = 0, cus = 256;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)kkt_resid_exact_kernel, kBlock, 0) !=
                hipSuccess ||
            occ < 1)
            occ = 1;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return (int64_t)occ * cus;
    }();
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(K.nblk, resident));
    hipLaunchKernelGGL(kkt_resid_exact_kernel, dim3(grid), dim3(kBlock), 0, c.stream, K.ptr.p, K.col.p, K.val.p, K.blk.p,
                       K.nblk, z, b, r);
    CPK_HIP(hipGetLastError());
}

void launch_kkt_panel(Ctx &c, const DMat &K, int kc, const double *Z, int64_t ldz, const double *B, int64_t ldb, double *R,
                      int64_t ldr) {
    if (!K.nrows || !K.nblk || kc <= 0) return;
    hipLaunchKernelGGL(kkt_panel_kernel, dim3((unsigned)K.nblk), dim3(kBlock), 0, c.stream, K.ptr.p, K.col.p, K.val.p,
                       K.blk.p, kc, Z, ldz, B, ldb, R, ldr);
    CPK_HIP(hipGetLastError());
}

}  // namespace cpk
