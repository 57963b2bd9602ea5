// Checks the value map of the matrix conversions (hostsparse.cpp: csr_from_csc / csr_from_csr with a
// ValueMap, apply_value_map) on seeded random input: column-compressed input, row-compressed input
// with unsorted columns, and row-compressed input with duplicates.  New values pushed through the
// map must equal, bit for bit, the conversion of the same index arrays with those values.  Host
// only; meant to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -I include -I cpkrylov_amd/csrc tools/micro/value_map_check.cpp cpkrylov_amd/csrc/hostsparse.cpp \
//       cpkrylov_amd/csrc/ordering.cpp -lpthread -o value_map_check && ./value_map_check
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cpk.h"
#include "host.hpp"

using namespace cpk;

static int bad = 0;

static void compare(const char *what, const HCsr &fresh, const ValueMap &vm, const HCsr &made, const std::vector<double> &v2) {
    std::vector<double> out((size_t)made.nnz() + 1, -7.0);  // one guard entry behind
    apply_value_map(vm, made.nnz(), v2.data(), out.data());
    const bool same = fresh.ptr == made.ptr && fresh.ind == made.ind && (int64_t)v2.size() == vm.count &&
                      (made.nnz() == 0 || std::memcmp(out.data(), fresh.val.data(), (size_t)made.nnz() * sizeof(double)) == 0) &&
                      out.back() == -7.0;
    if (!same) bad++, printf("MISMATCH %s\n", what);
}

// values whose sums depend on the order: huge terms that cancel beside small ones
static std::vector<double> values(std::mt19937_64 &rng, size_t n) {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<double> v(n);
    for (auto &x : v) {
        x = u(rng);
        const auto k = rng() % 8;
        if (k == 0) x = 1e16;
        if (k == 1) x = -1e16;
        if (k == 2) x = 0.0;
    }
    return v;
}

int main() {
    std::mt19937_64 rng(20260101);
    const char *kinds[3] = {"csc", "csr unsorted", "csr duplicates"};
    int maps[3] = {0, 0, 0};  // identity / permutation / sums seen
    for (int trial = 0; trial < 300; trial++) {
        const int kind = trial % 3;
        const int64_t nr = (int64_t)(rng() % 40), nc = (int64_t)(rng() % 40);
        const int64_t major = kind == 0 ? nc : nr, minor = kind == 0 ? nr : nc;
        const int maxper = trial % 7 == 0 ? 0 : (int)(rng() % 12);
        std::vector<int64_t> ptr(major + 1, 0);
        std::vector<int64_t> idx;
        for (int64_t i = 0; i < major; i++) {
            const int cnt = minor > 0 ? (int)(rng() % (maxper + 1)) : 0;
            std::vector<int64_t> r;
            for (int t = 0; t < cnt; t++) r.push_back((int64_t)(rng() % minor));
            if (kind != 2 || trial % 2) {  // distinct indices (shuffled order stays)
                std::vector<int64_t> u;
                for (auto x : r)
                    if (std::find(u.begin(), u.end(), x) == u.end()) u.push_back(x);
                r = u;
            }
            if (trial % 5 == 0) std::sort(r.begin(), r.end());  // sorted input: the identity map for CSR
            idx.insert(idx.end(), r.begin(), r.end());
            ptr[i + 1] = (int64_t)idx.size();
        }
        const std::vector<double> v1 = values(rng, idx.size()), v2 = values(rng, idx.size());
        ValueMap vm;
        HCsr made, fresh;
        if (kind == 0) {
            std::vector<size_t> jc(ptr.begin(), ptr.end()), ir(idx.begin(), idx.end());
            made = csr_from_csc(nr, nc, jc.data(), ir.data(), v1.data(), &vm);
            fresh = csr_from_csc(nr, nc, jc.data(), ir.data(), v2.data());
        } else {
            std::vector<int32_t> ci(idx.begin(), idx.end());
            made = csr_from_csr(nr, nc, ptr.data(), ci.data(), v1.data(), &vm);
            fresh = csr_from_csr(nr, nc, ptr.data(), ci.data(), v2.data());
        }
        maps[vm.identity ? 0 : vm.sptr.empty() ? 1 : 2]++;
        compare(kinds[kind], fresh, vm, made, v2);
    }
    printf("value maps: %d identity, %d permutations, %d with sums; %d mismatches\n", maps[0], maps[1], maps[2], bad);
    return bad || !maps[0] || !maps[1] || !maps[2] ? 1 : 0;
}
