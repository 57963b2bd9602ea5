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
// single-column pass's order, so a column has the same bits on either path (capi.cpp routes).
#include <hip/hip_runtime.h>

#include <algorithm>

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

void launch_kkt_panel(Ctx &c, const DMat &K, int kc, const double *Z, int64_t ldz, const double *B, int64_t ldb, double *R,
                      int64_t ldr) {
    if (!K.nrows || !K.nblk || kc <= 0) return;
    hipLaunchKernelGGL(kkt_panel_kernel, dim3((unsigned)K.nblk), dim3(kBlock), 0, c.stream, K.ptr.p, K.col.p, K.val.p,
                       K.blk.p, kc, Z, ldz, B, ldb, R, ldr);
    CPK_HIP(hipGetLastError());
}

}  // namespace cpk
