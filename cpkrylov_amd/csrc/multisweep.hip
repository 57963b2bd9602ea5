// multisweep.hip -- the bare factor composite Y = P * L' \ (D \ (L \ P' * X)) for a block of
// right-hand sides (cpk_pc_apply_ldl_multi; opLDL2's M' and conj(M), ops/opLDL2.m:127-136).
//
// Columns are solved in panels of kMultiKP.  A panel lives in the work array W[row * KP + j], rows in
// schedule order, so the KP values of a row are one contiguous 64-byte segment.  One forward and
// one backward kernel, each launched once per round with one workgroup per block (the rounds are
// ordered by the stream, as for sptrsv_fwd_kernel / sptrsv_bwd_kernel).  A block stages its
// entries, columns and row pointers in LDS once for all KP columns and keeps its own W rows
// there; references outside the block read the global panel, one segment per entry.  Within a
// level the work items are (row, j) pairs with j fastest across lanes: the 8 lanes of a row read
// the same staged entry (an LDS broadcast) and one 64-byte segment of W.
//
// Arithmetic: every (row, j) starts from its input (forward: X; backward: W / D) and subtracts
// val[e] * W[col[e]][j] for e ascending in stored order, each product and each subtraction
// rounded on its own (-ffp-contract=off) -- the order cpk_analysis_schedule documents and the
// single-column sweeps keep, so every column equals cpk_pc_apply_ldl on it bit for bit.  No
// reassociation: no reduction over a row, no split rows.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev.hpp"

namespace cpk {

namespace {

constexpr int KP = kMultiKP;
constexpr int kMultiThreads = 256;
constexpr int kMultiPre = 4;  // panel reads in flight per lane in the outside-prefix pass
constexpr size_t kMultiMaxLds = 160 * 1024;  // gfx950: 160 KB of LDS per workgroup

// LDS image of a block of nr rows and ne entries: its W rows, the entries' values and columns,
// the row pointers and each row's start behind its leading outside terms; every part a multiple
// of 16 bytes
__host__ __device__ inline size_t multi_img_bytes(int nr, int ne) {
    const size_t w = (size_t)nr * KP * 8, v = ((size_t)ne * 8 + 15) & ~(size_t)15, c = ((size_t)ne * 4 + 15) & ~(size_t)15,
                 p = ((size_t)(2 * nr + 2) * 4 + 15) & ~(size_t)15;  // row pointers [nr + 1], row starts [nr], a flag
    return w + v + c + p;
}

// a block is staged when it keeps the round's configured block shape (rows, entries of either
// direction: what the schedule built it for) and its image fits the LDS the launch may ask for;
// one predicate for the kernels and for the host's launch sizes
__host__ __device__ inline bool multi_staged(int nr, int nef, int neb, int R, int CAP, int lds_limit) {
    const int ne = nef > neb ? nef : neb;
    return nr <= R && ne <= CAP && multi_img_bytes(nr, ne) <= (size_t)lds_limit;
}

// X, Y: column-major, kc <= KP columns of this panel (the missing ones are computed as zeros and
// never stored).  ptr / col / val: the sweep's rows (forward: fptr..., backward: bptr...), optr:
// the other direction's row pointers (the staging predicate).  BWD: store_w = 0 skips the panel
// write-back of staged blocks (round 0: nothing reads it afterwards).
// MODE 1: act[j] != 0 marks column j active, act[KP] any of them (null: all active)
struct MultiRef {
    const double *Rp = nullptr;    // forward input, natural order
    double *Yp = nullptr;          // backward output, natural order
    const int32_t *act = nullptr;  // [KP + 1] on the device
    int acc = 0;                   // backward: Yp += w for the active columns (0: Yp = w, every column)
    const int *gate = nullptr;     // a zero word: the launch does nothing (a block solve's frozen panel)
};

template <bool BWD, int MODE>
__global__ __launch_bounds__(kMultiThreads) void multisweep_kernel(
    int64_t blk0, int R, int CAP, int lds_limit, const int32_t *__restrict__ blk_lvl, const int32_t *__restrict__ lvl_row,
    const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ optr, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ D, const int32_t *__restrict__ perm,
    const double *__restrict__ X, int64_t ldx, double *__restrict__ Y, int64_t ldy, int kc, double *W, int store_w,
    MultiRef ref) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TPB = kMultiThreads;
    static_assert(TPB % KP == 0, "a thread keeps its column across strided passes");
    if (ref.gate && *ref.gate == 0) return;
    bool on = true;  // MODE 1: this thread's column (threadIdx.x % KP) is active
    if (MODE == 1 && ref.act) {
        if (ref.act[KP] == 0) return;
        on = ref.act[threadIdx.x % KP] != 0;
    }
    const int64_t b = blk0 + blockIdx.x;
    const int l0 = blk_lvl[b], l1 = blk_lvl[b + 1];
    const int r0 = lvl_row[l0], r1 = lvl_row[l1];
    const uint32_t e0 = ptr[r0];
    const int nr = r1 - r0, ne = (int)(ptr[r1] - e0), neo = (int)(optr[r1] - optr[r0]);
    const int tid = threadIdx.x;
    if (multi_staged(nr, BWD ? neo : ne, BWD ? ne : neo, R, CAP, lds_limit)) {
        double *Wl = reinterpret_cast<double *>(smem);
        double *Vl = Wl + (size_t)nr * KP;
        int32_t *Cl = reinterpret_cast<int32_t *>(smem + (size_t)nr * KP * 8 + (((size_t)ne * 8 + 15) & ~(size_t)15));
        int32_t *Pl = Cl + (((size_t)ne + 3) & ~(size_t)3);
        int32_t *Ps = Pl + nr + 1;
        int32_t *flag = Ps + nr;  // any entry outside the block (all LDS in the dynamic region: no static)
        int any_out = 0;
        if (tid == 0) *flag = 0;
        __syncthreads();
        if (BWD) {
            for (int i = tid; i < nr * KP; i += TPB) Wl[i] = W[(size_t)r0 * KP + i] / D[r0 + i / KP];
        } else if (MODE == 1) {
            for (int i = tid; i < nr * KP; i += TPB)  // one 64-byte segment per row; i % KP == tid % KP
                Wl[i] = on ? ref.Rp[(size_t)perm[r0 + i / KP] * KP + i % KP] : 0.0;
        } else {
            // gather with the row fastest across lanes, as the single-column sweep reads x(perm)
            for (int i = tid; i < nr * KP; i += TPB) {
                const int j = i / nr, row = i - j * nr;
                Wl[row * KP + j] = j < kc ? X[(int64_t)perm[r0 + row] + (int64_t)j * ldx] : 0.0;
            }
        }
        for (int i = tid; i <= nr; i += TPB) Pl[i] = (int32_t)(ptr[r0 + i] - e0);
        for (int e = tid; e < ne; e += TPB) {
            const int32_t c = __builtin_nontemporal_load(col + e0 + e);  // streamed once per panel
            Vl[e] = __builtin_nontemporal_load(val + e0 + e);
            const bool local = c >= r0 && c < r1;
            Cl[e] = local ? c - r0 : ~c;  // outside the block: ~(schedule row) < 0
            any_out |= !local;
        }
        if (any_out) *flag = 1;
        __syncthreads();
        const bool outside = *flag != 0;
        // A row's leading outside terms (rows solved in other rounds: final in the global panel)
        // wait for nothing in this block, so all rows take them at once, before the levels, kMultiPre
        // panel reads in flight per lane -- the same subtractions in the same stored order as the
        // level loop would make.  The stored order puts them first: forward columns ascend
        // (earlier rounds are lower schedule rows), backward rows descend.
        const int32_t *St = Pl;
        if (outside) {
            for (int i = tid; i < nr * KP; i += TPB) {
                const int row = i / KP, j = i % KP;
                const int q1 = Pl[row + 1];
                int e = Pl[row];
                double acc = Wl[i];
                while (e < q1) {
                    int32_t c[kMultiPre];
                    double v[kMultiPre], x[kMultiPre];
#pragma unroll
                    for (int u = 0; u < kMultiPre; u++) {
                        const int eu = e + u < q1 ? e + u : q1 - 1;
                        c[u] = Cl[eu], v[u] = Vl[eu];
                    }
#pragma unroll
                    for (int u = 0; u < kMultiPre; u++) x[u] = W[(size_t)(c[u] < 0 ? ~c[u] : 0) * KP + j];
                    int t = 0;  // the leading outside terms of this chunk
#pragma unroll
                    for (int u = 0; u < kMultiPre; u++) {
                        if (t == u && e + u < q1 && c[u] < 0) {
                            acc -= v[u] * x[u];
                            t = u + 1;
                        }
                    }
                    e += t;
                    if (t < kMultiPre) break;
                }
                Wl[i] = acc;
                if (j == 0) Ps[row] = e;
            }
            St = Ps;
            __syncthreads();
        }
        for (int s = 0; s < l1 - l0; s++) {
            const int l = BWD ? l1 - 1 - s : l0 + s;
            const int a = lvl_row[l] - r0, z = lvl_row[l + 1] - r0;
            for (int i = tid; i < (z - a) * KP; i += TPB) {
                const int row = a + i / KP, j = i % KP;
                double acc = Wl[row * KP + j];
                const int q1 = Pl[row + 1];
                for (int e = St[row]; e < q1; e++) {
                    const int32_t c = Cl[e];
                    const double x = c >= 0 ? Wl[c * KP + j] : W[(size_t)(~c) * KP + j];
                    acc -= Vl[e] * x;
                }
                Wl[row * KP + j] = acc;
            }
            __syncthreads();
        }
        if (!BWD || store_w)
            for (int i = tid; i < nr * KP; i += TPB) W[(size_t)r0 * KP + i] = Wl[i];
        if (BWD && MODE == 1) {
            for (int i = tid; i < nr * KP; i += TPB) {
                double *y = ref.Yp + (size_t)perm[r0 + i / KP] * KP + i % KP;
                if (!ref.acc) *y = Wl[i];
                else if (on) *y = *y + Wl[i];
            }
        } else if (BWD) {
            for (int i = tid; i < nr * kc; i += TPB) {
                const int j = i / nr, row = i - j * nr;
                Y[(int64_t)perm[r0 + row] + (int64_t)j * ldy] = Wl[row * KP + j];
            }
        }
        return;
    }
    // direct path through global memory: a block above the configured shape (a factor row longer
    // than every cap) or whose image does not fit
    for (int s = 0; s < l1 - l0; s++) {
        const int l = BWD ? l1 - 1 - s : l0 + s;
        const int a = lvl_row[l], z = lvl_row[l + 1];
        for (int64_t i = tid; i < (int64_t)(z - a) * KP; i += TPB) {
            const int k = a + (int)(i / KP), j = (int)(i % KP);
            double acc;
            if (BWD) acc = W[(size_t)k * KP + j] / D[k];
            else if (MODE == 1) acc = on ? ref.Rp[(size_t)perm[k] * KP + j] : 0.0;
            else acc = j < kc ? X[(int64_t)perm[k] + (int64_t)j * ldx] : 0.0;
            const uint32_t q1 = ptr[k + 1];
            for (uint32_t e = ptr[k]; e < q1; e++) acc -= val[e] * W[(size_t)col[e] * KP + j];
            W[(size_t)k * KP + j] = acc;
            if (BWD && MODE == 1) {
                double *y = ref.Yp + (size_t)perm[k] * KP + j;
                if (!ref.acc) *y = acc;
                else if (on) *y = *y + acc;
            } else if (BWD && j < kc) {
                Y[(int64_t)perm[k] + (int64_t)j * ldy] = acc;
            }
        }
        __syncthreads();
    }
}

// the dynamic LDS a launch may ask for: 64 KB always, kMultiMaxLds when the device grants the
// kernels the opt-in (asked once)
int multi_lds_limit() {
    static const int limit = [] {
        bool ok = true;
        for (const void *f : {(const void *)multisweep_kernel<false, 0>, (const void *)multisweep_kernel<true, 0>,
                              (const void *)multisweep_kernel<false, 1>, (const void *)multisweep_kernel<true, 1>})
            ok = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMultiMaxLds) == hipSuccess && ok;
        if (!ok) (void)hipGetLastError();  // not granted: no error left behind for the launches' check
        return ok ? (int)kMultiMaxLds : 64 * 1024;
    }();
    return limit;
}

}  // namespace

// the launch plan of a factor: per round the LDS of its largest staged block in each direction,
// and the path counts (cpk_pc_multi_info)
const MultiPlan &multisweep_plan(const DFactor &F) {
    MultiPlan &p = F.multi;
    if (p.ready) return p;
    const int64_t nr = (int64_t)F.round_ptr.size() - 1;
    const int limit = multi_lds_limit();
    p.lds.assign((size_t)std::max<int64_t>(nr, 0) * 2, 0);
    p.staged = p.direct = 0;
    if (F.hmeta.size() < (size_t)F.nblk * 8) throw Error(CPK_ERR_UNSUPPORTED, "internal: factor without block records");
    for (int64_t r = 0; r < nr; r++) {
        for (int64_t b = F.round_ptr[r]; b < F.round_ptr[r + 1]; b++) {
            const int32_t *m = &F.hmeta[(size_t)b * 8];
            const int rows = m[1] - m[0], nef = m[5] - m[4], neb = m[7] - m[6];
            if (!multi_staged(rows, nef, neb, F.rows_of(r), F.cap_of(r), limit)) {
                p.direct++;
                continue;
            }
            p.staged++;
            p.lds[(size_t)r * 2] = std::max(p.lds[(size_t)r * 2], multi_img_bytes(rows, nef));
            p.lds[(size_t)r * 2 + 1] = std::max(p.lds[(size_t)r * 2 + 1], multi_img_bytes(rows, neb));
        }
    }
    p.launches = 2 * nr;
    p.ready = true;
    return p;
}

namespace {

// one panel's forward rounds (ascending) / backward rounds (descending), one launch per round
template <int MODE>
void multi_fwd_rounds(Ctx &c, const DFactor &F, const double *Xp, int64_t ldx, int kc, double *panel, const MultiRef &ref) {
    const MultiPlan &p = multisweep_plan(F);
    const int64_t R = (int64_t)F.round_ptr.size() - 1;
    const int limit = multi_lds_limit();
    for (int64_t r = 0; r < R; r++) {
        const int64_t b0 = F.round_ptr[r], nb = F.round_ptr[r + 1] - b0;
        if (!nb) continue;
        hipLaunchKernelGGL((multisweep_kernel<false, MODE>), dim3((unsigned)nb), dim3(kMultiThreads), p.lds[(size_t)r * 2],
                           c.stream, b0, F.rows_of(r), F.cap_of(r), limit, F.blk_lvl.p, F.lvl_row.p, F.fptr.p,
                           F.bptr.p, F.fcol.p, F.fval.p, F.D.p, F.perm.p, Xp, ldx, (double *)nullptr, (int64_t)0, kc, panel,
                           1, ref);
    }
}

template <int MODE>
void multi_bwd_rounds(Ctx &c, const DFactor &F, double *Yp, int64_t ldy, int kc, double *panel, const MultiRef &ref) {
    const MultiPlan &p = multisweep_plan(F);
    const int64_t R = (int64_t)F.round_ptr.size() - 1;
    const int limit = multi_lds_limit();
    for (int64_t r = R - 1; r >= 0; r--) {
        const int64_t b0 = F.round_ptr[r], nb = F.round_ptr[r + 1] - b0;
        if (!nb) continue;
        // the backward sweep's last round: nothing reads its staged blocks' panel rows again
        hipLaunchKernelGGL((multisweep_kernel<true, MODE>), dim3((unsigned)nb), dim3(kMultiThreads),
                           p.lds[(size_t)r * 2 + 1], c.stream, b0, F.rows_of(r), F.cap_of(r), limit, F.blk_lvl.p,
                           F.lvl_row.p, F.bptr.p, F.fptr.p, F.bcol.p, F.bval.p, F.D.p, F.perm.p, (const double *)nullptr,
                           (int64_t)0, Yp, ldy, kc, panel, r == 0 ? 0 : 1, ref);
    }
}

}  // namespace

void launch_multisweep(Ctx &c, const DFactor &F, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                       double *panel) {
    for (int64_t j0 = 0; j0 < k; j0 += KP) {
        const int kc = (int)std::min<int64_t>(KP, k - j0);
        multi_fwd_rounds<0>(c, F, X + j0 * ldx, ldx, kc, panel, MultiRef{});
        multi_bwd_rounds<0>(c, F, Y + j0 * ldy, ldy, kc, panel, MultiRef{});
    }
    CPK_HIP(hipGetLastError());
}

void launch_multisweep_first(Ctx &c, const DFactor &F, int kc, const double *X, int64_t ldx, double *Yp, double *panel,
                             const int *gate) {
    MultiRef ref, fwd;
    ref.Yp = Yp, ref.gate = gate, fwd.gate = gate;
    multi_fwd_rounds<0>(c, F, X, ldx, kc, panel, fwd);
    multi_bwd_rounds<1>(c, F, nullptr, 0, kc, panel, ref);
    CPK_HIP(hipGetLastError());
}

void launch_multisweep_refine(Ctx &c, const DFactor &F, const double *Rp, double *Yp, const int32_t *act, double *panel) {
    MultiRef ref;
    ref.Rp = Rp, ref.Yp = Yp, ref.act = act, ref.acc = 1;
    multi_fwd_rounds<1>(c, F, nullptr, 0, KP, panel, ref);
    multi_bwd_rounds<1>(c, F, nullptr, 0, KP, panel, ref);
    CPK_HIP(hipGetLastError());
}

}  // namespace cpk
