// Stand-alone probe of the K-best list code of the kNN kernels (aux_kernels.hpp k_knn_t, knn_index_kernels.hpp k_knn_ix) on candidate
// streams with many EQUAL distances, against std::sort on the host. Per list it checks the unsorted K best (the accept / replace-the-worst
// statements of k_knn_ix) and the ordered output written two ways: by the compare-and-swap network that ends k_knn_t, and by the counting
// order that ends k_knn_ix. Built with the library's flags:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -fno-slp-vectorize tools/knn_tie_probe.hip -o /tmp/knn_tie_probe
// Output of one run on an MI355X: profiles/knn_tie_probe.txt.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

template <int K, int MODE>
__global__ void k_probe(const double* __restrict__ cd, const int* __restrict__ ci, int n, int k, double* __restrict__ ud, int* __restrict__ ui,
                        int* __restrict__ si) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    const double* d_ = cd + (long long)q * n;
    const int* c_ = ci + (long long)q * n;
    double bd[K]; int bi[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { bd[t] = __builtin_inf(); bi[t] = 0x7fffffff - t; }
    double wd = __builtin_inf(); int wi = 0x7fffffff;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const double d = d_[i]; const int c = c_[i];
        if (!(d < wd || (d == wd && c < wi))) continue;
        double nd = -1.0; int ni = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if (bi[t] == wi) { bd[t] = d; bi[t] = c; }
            if (bd[t] > nd || (bd[t] == nd && bi[t] > ni)) { nd = bd[t]; ni = bi[t]; }
        }
        wd = nd; wi = ni;
    }
#pragma unroll
    for (int t = 0; t < K; ++t) { ud[(long long)q * K + t] = bd[t]; ui[(long long)q * K + t] = bi[t]; }
    if (MODE == 0) {         // the network of k_knn_t
#pragma unroll
        for (int a = 0; a < K - 1; ++a) {
#pragma unroll
            for (int t = 0; t < K - 1 - a; ++t) {
                if (bd[t + 1] < bd[t] || (bd[t + 1] == bd[t] && bi[t + 1] < bi[t])) {
                    const double td = bd[t]; const int ti = bi[t];
                    bd[t] = bd[t + 1]; bi[t] = bi[t + 1]; bd[t + 1] = td; bi[t + 1] = ti;
                }
            }
        }
        for (int r = 0; r < k; ++r) si[(long long)q * k + r] = bi[r] >= 0x7fffffff - K ? -1 : bi[r];
    } else {                 // the counting order of k_knn_ix
#pragma unroll
        for (int t = 0; t < K; ++t) {
            int place = 0;
#pragma unroll
            for (int s = 0; s < K; ++s) place += (bd[s] < bd[t] || (bd[s] == bd[t] && bi[s] < bi[t])) ? 1 : 0;
            if (place < k) si[(long long)q * k + place] = bi[t] >= 0x7fffffff - K ? -1 : bi[t];
        }
    }
}

template <int K, int MODE>
int run(int k) {
    const int Q = 256, n = 60;
    std::mt19937 g(K);
    std::vector<double> cd(Q * n); std::vector<int> ci(Q * n);
    for (int q = 0; q < Q; ++q) {
        std::vector<int> idx(n);
        for (int i = 0; i < n; ++i) idx[i] = i * 7 + q;
        std::shuffle(idx.begin(), idx.end(), g);
        for (int i = 0; i < n; ++i) { ci[q * n + i] = idx[i]; cd[q * n + i] = q % 4 == 0 ? 5.0 : (double)(g() % 3); }
    }
    double *dcd, *dud; int *dci, *dui, *dsi;
    CK(hipMalloc(&dcd, cd.size() * 8)); CK(hipMalloc(&dci, ci.size() * 4)); CK(hipMalloc(&dud, Q * K * 8)); CK(hipMalloc(&dui, Q * K * 4));
    CK(hipMalloc(&dsi, Q * k * 4));
    CK(hipMemcpy(dcd, cd.data(), cd.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dci, ci.data(), ci.size() * 4, hipMemcpyHostToDevice));
    k_probe<K, MODE><<<Q / 64, 64>>>(dcd, dci, n, k, dud, dui, dsi);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    std::vector<double> ud(Q * K); std::vector<int> ui(Q * K), si(Q * k);
    CK(hipMemcpy(ud.data(), dud, ud.size() * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(ui.data(), dui, ui.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(si.data(), dsi, si.size() * 4, hipMemcpyDeviceToHost));
    int bad_set = 0, bad_pair = 0, bad_sort = 0, shown = 0;
    for (int q = 0; q < Q; ++q) {
        std::vector<std::pair<double, int>> all(n), got(K);
        for (int i = 0; i < n; ++i) all[i] = {cd[q * n + i], ci[q * n + i]};
        std::sort(all.begin(), all.end());
        for (int t = 0; t < K; ++t) got[t] = {ud[q * K + t], ui[q * K + t]};
        bool pair_ok = true;                      // every unsorted entry is a real (d, idx) pair of the stream
        for (auto& e : got) pair_ok &= std::find(all.begin(), all.end(), e) != all.end();
        std::sort(got.begin(), got.end());
        bool set_ok = std::equal(got.begin(), got.end(), all.begin());
        bool sort_ok = true;
        for (int r = 0; r < k; ++r) sort_ok &= si[q * k + r] == all[r].second;
        bad_pair += !pair_ok; bad_set += !set_ok; bad_sort += !sort_ok;
        if ((!set_ok || !sort_ok) && shown++ < 2) {
            printf("  q %d unsorted:", q); for (int t = 0; t < K; ++t) printf(" (%g,%d)", ud[q * K + t], ui[q * K + t]);
            printf("\n  sorted out:"); for (int r = 0; r < k; ++r) printf(" %d", si[q * k + r]);
            printf("\n  want:"); for (int r = 0; r < k; ++r) printf(" (%g,%d)", all[r].first, all[r].second); printf("\n");
        }
    }
    printf("%s K=%d k=%d: lists with a foreign pair %d, wrong set %d, wrong sorted output %d of %d\n", MODE == 0 ? "network " : "counting", K, k, bad_pair, bad_set, bad_sort, Q);
    return 0;
}

int main() {
    return run<8, 0>(8) | run<8, 0>(3) | run<10, 0>(10) | run<16, 0>(16) | run<8, 1>(8) | run<8, 1>(3) | run<10, 1>(10) | run<16, 1>(16);
}
