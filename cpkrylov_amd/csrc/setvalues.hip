// setvalues.hip -- new values of a matrix handle from device memory (cpk_mat_set_values_device):
// the stored entries gathered from the creating call's value order through the handle's value
// map (host.hpp, ValueMap).  Streaming kernels, one thread per stored entry: 12 bytes read and 8
// written per entry for a permutation ("Value refresh").  Sums of duplicates
// run in map order from the first source, additions only, as the host conversion sums them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev.hpp"

namespace cpk {

constexpr int kSetBlock = 256;

// the map is read once per update: non-temporal, it leaves the caches to the gathered values
__global__ __launch_bounds__(kSetBlock) void set_values_perm_kernel(const uint32_t *__restrict__ perm,
                                                                     const double *__restrict__ in, int64_t nnz,
                                                                     double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kSetBlock;
    for (int64_t q = blockIdx.x * (int64_t)kSetBlock + threadIdx.x; q < nnz; q += stride)
        out[q] = in[__builtin_nontemporal_load(perm + q)];
}

__global__ __launch_bounds__(kSetBlock) void set_values_sum_kernel(const uint32_t *__restrict__ sptr,
                                                                    const uint32_t *__restrict__ src,
                                                                    const double *__restrict__ in, int64_t nnz,
                                                                    double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kSetBlock;
    for (int64_t q = blockIdx.x * (int64_t)kSetBlock + threadIdx.x; q < nnz; q += stride) {
        const uint32_t t0 = sptr[q], t1 = sptr[q + 1];
        double s = in[src[t0]];
        for (uint32_t t = t0 + 1; t < t1; t++) s = s + in[src[t]];
        out[q] = s;
    }
}

void upload_value_map(const ValueMap &vm, DValueMap &dm) {
    if (dm.ready) return;
    if (!vm.identity) {
        if (vm.sptr.empty()) dm.perm.upload(vm.perm);
        else dm.sptr.upload(vm.sptr), dm.src.upload(vm.src);
    }
    dm.ready = true;
}

void launch_set_values(Ctx &c, const ValueMap &vm, const DValueMap &dm, int64_t nnz, const double *in, double *out) {
    if (nnz <= 0) return;
    if (vm.identity) {
        CPK_HIP(hipMemcpyAsync(out, in, (size_t)nnz * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
        return;
    }
    // the maps hold one entry per stored entry (perm: nnz, sptr: nnz + 1); every source index is
    // below vm.count, the length the caller's array was checked against
    const bool sum = !vm.sptr.empty();
    if (!dm.ready || (sum ? dm.sptr.n != (size_t)nnz + 1 || dm.src.n != (size_t)vm.count : dm.perm.n != (size_t)nnz))
        throw Error(CPK_ERR_ARGS, "set_values: the device value map does not match the matrix");
    const int grid = (int)std::min<int64_t>((nnz + kSetBlock - 1) / kSetBlock, 8192);
    if (sum)
        hipLaunchKernelGGL(set_values_sum_kernel, dim3(grid), dim3(kSetBlock), 0, c.stream, dm.sptr.p, dm.src.p, in, nnz, out);
    else
        hipLaunchKernelGGL(set_values_perm_kernel, dim3(grid), dim3(kSetBlock), 0, c.stream, dm.perm.p, in, nnz, out);
    CPK_HIP(hipGetLastError());
}

}  // namespace cpk
