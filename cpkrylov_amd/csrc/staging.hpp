// staging.hpp -- host arrays of capi.cpp's host-array entries <-> device memory; launches no kernel
#pragma once
#include <algorithm>
#include <exception>

#include "dev.hpp"

namespace cpk {

template <class T>
void h2d(DBuf<T> &d, const T *h, size_t n) {
    d.alloc(n);
    if (n) CPK_HIP(hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice));
}

// rows x k of a host block with leading dimension ld, packed on the device (leading dimension
// ld(): rows, at least 1; at least one element, so k = 0 is a block like any other whose up and
// down copy nothing); the caller's padding rows are never touched
struct HostBlock {
    DBuf<double> d;
    int64_t rows, k;
    HostBlock(int64_t rows_, int64_t k_) : rows(rows_), k(k_) { d.alloc(std::max<size_t>((size_t)ld() * (size_t)k, 1)); }
    int64_t ld() const { return std::max<int64_t>(rows, 1); }
    void up(const double *H, int64_t ldh) {
        if (rows && k) CPK_HIP(hipMemcpy2D(d.p, ld() * sizeof(double), H, (size_t)ldh * sizeof(double), rows * sizeof(double),
                                           (size_t)k, hipMemcpyHostToDevice));
    }
    // rows [row0, row0 + nrows) of every column (default: all rows)
    void down(double *H, int64_t ldh, int64_t row0 = 0, int64_t nrows = -1) const {
        if (nrows < 0) nrows = rows;
        if (nrows && k) CPK_HIP(hipMemcpy2D(H, (size_t)ldh * sizeof(double), d.p + row0, ld() * sizeof(double),
                                            nrows * sizeof(double), (size_t)k, hipMemcpyDeviceToHost));
    }
};

// the gradient arrays of a host entry on the device, and back
struct HostGrads {
    DBuf<double> d[3];
    double *h[3];
    int64_t cnt[3];
    HostGrads(double *gA, int64_t cA, double *gB, int64_t cB, double *gC, int64_t cC) : h{gA, gB, gC}, cnt{cA, cB, cC} {
        for (int i = 0; i < 3; i++)
            if (h[i]) d[i].alloc((size_t)std::max<int64_t>(cnt[i], 1));
    }
    double *dev(int i) { return h[i] ? d[i].p : nullptr; }
    void down(hipStream_t s) {
        for (int i = 0; i < 3; i++)
            if (h[i] && cnt[i]) CPK_HIP(hipMemcpyAsync(h[i], d[i].p, (size_t)cnt[i] * sizeof(double), hipMemcpyDeviceToHost, s));
        CPK_HIP(hipStreamSynchronize(s));
    }
};

// The host form of a solve of one column of N values: b up, x up (warm) or allocated, run(d_b, d_x),
// then x back to the host -- also when run threw, unless run left *wrote_x false (null: always
// back) -- the gradients g (if any) back only when nothing threw, the wait, and run's exception again.
template <class Run>
void host_column_solve(hipStream_t s, int64_t N, const double *b, double *x, int warm, const bool *wrote_x, HostGrads *g,
                       Run run) {
    DBuf<double> db, dx;
    h2d(db, b, (size_t)N);
    if (warm) h2d(dx, x, (size_t)N);
    else dx.alloc((size_t)std::max<int64_t>(N, 1));
    std::exception_ptr err;
    try {
        run((const double *)db.p, dx.p);
    } catch (...) {
        err = std::current_exception();
    }
    if (N && (!wrote_x || *wrote_x)) CPK_HIP(hipMemcpyAsync(x, dx.p, N * sizeof(double), hipMemcpyDeviceToHost, s));
    if (g && !err) g->down(s);  // ends with the wait
    else CPK_HIP(hipStreamSynchronize(s));
    if (err) std::rethrow_exception(err);
}

}  // namespace cpk
