// ------------------------------------------------------------------------------------------------
// Exact k-nearest-neighbour search on the device: the `knn(x_context / 1000, x_query / 1000, k)` calls of the
// reference -- SpatialAttention's query edges (module.py:282; a NEW 112 000-point query set per candidate in the refine pass,
// process_continuous_days.py:926-980) and the base graphs of the product graph (`knn(x/1000, x/1000, k + 1)` +
// `remove_self_loops`, process_utils.py:718-719). Brute force (3-D, n_context is 10^4..10^5: 10^9 pair distances = a millisecond) with
// a wave (k_knn), a workgroup (k_knn_b) or a lane (k_knn_t) per query, and through a cell index (k_knn_ix, knn_index_kernels.hpp). All
// four write ONE table, bit for bit (tests/test_knn_ties_gpu.py holds each to a float64 stable argsort on the host): neighbours by the
// distance and in the order below, -1 where the context has fewer than k points. exclude_self: skip candidate == query id (query set =
// context set). The rules stand here once; a kernel keeps how it visits candidates.
// ------------------------------------------------------------------------------------------------

// The distance: fp64 on the fp32 coordinates themselves (the common 1 / 1000 scale does not change the order; coordinate differences
// of fp32 values are exact in fp64), squared, summed in the order (a + b) + c. One statement for every kernel, so that every kernel
// gets the same instructions for it: the HIP _rn intrinsics are plain * and +, which the compiler does fuse (profiles/EXPERIMENTS.md).
__device__ __forceinline__ double knn_sum3(double a, double b, double c) { return __dadd_rn(__dadd_rn(a, b), c); }
__device__ __forceinline__ double knn_dist2(double q0, double q1, double q2, float cx, float cy, float cz) {
    const double d0 = q0 - (double)cx, d1 = q1 - (double)cy, d2 = q2 - (double)cz;
    return knn_sum3(__dmul_rn(d0, d0), __dmul_rn(d1, d1), __dmul_rn(d2, d2));
}

// The order: lexicographic (distance, index) -- of two points at exactly the same distance the one with the smaller index comes first.
__device__ __forceinline__ bool knn_before(double d, int i, double od, int oi) { return d < od || (d == od && i < oi); }

// An empty slot of a list is (inf, KNN_NONE), or (inf, KNN_NONE - t) where the slots must differ: after every point in the order, and
// -1 in the table (a context's indices stay far below: 3 * index is an int).
constexpr int KNN_NONE = 0x7fffffff;
__device__ __forceinline__ int knn_index_or_none(int i, int K) { return i >= KNN_NONE - K ? -1 : i; }

// The K best of ALL candidates of a query in one lane, UNSORTED, with the worst one (largest (distance, index)) tracked (k_knn_t,
// k_knn_ix): an accepted candidate overwrites the worst and the worst is found again (K compares) -- about half the instructions of
// a K-step bubble, and with a lane per query the accept path is what a wave mostly pays for (some lane accepts in ~a quarter of the
// steps). The empty slots have distinct indices, so all entries are distinct; they are the largest entries, so while one is left it
// is the worst, any point replaces it, and a list whose worst is a point holds K points.
template <int K>
struct KnnWorst {
    double d[K];
    int i[K];
    double wd;          // the worst entry
    int wi;
    float thr;          // fp32 guard of wd
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int t = 0; t < K; ++t) { d[t] = __builtin_inf(); i[t] = KNN_NONE - t; }
        wd = __builtin_inf(); wi = KNN_NONE; thr = __builtin_inff();
    }
    // The fp32 pre-filter most candidates end on: dropped only if the fp32 distance exceeds the worst by more than 1e-5 relative (fp32
    // rounding is < 1e-6); what passes is decided by offer() on the exact distance.
    __device__ __forceinline__ bool passes(float d32) const { return d32 <= thr; }
    // ASCENDING: candidates arrive in increasing index order, so a tie with the worst has the larger index and the gate is the distance
    // alone; otherwise the full test.
    template <bool ASCENDING>
    __device__ __forceinline__ void offer(double nd, int ni) {
        if (!(ASCENDING ? nd < wd : knn_before(nd, ni, wd, wi))) return;
        double xd = -1.0;                            // replace the worst, find the new worst
        int xi = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if (i[t] == wi) { d[t] = nd; i[t] = ni; }
            if (knn_before(xd, xi, d[t], i[t])) { xd = d[t]; xi = i[t]; }
        }
        wd = xd; wi = xi;
        thr = (float)wd;
        thr = thr + thr * 1e-5f;                    // inf stays inf
    }
    __device__ __forceinline__ bool full() const { return wi < KNN_NONE - K; }      // K points, no empty slot
    __device__ __forceinline__ double worst_d() const { return wd; }
    // The table row, in order BY COUNTING: an entry's place is the number of entries before it (distinct entries: places 0 .. K - 1 once
    // each). Not by exchanges: the compare-and-swap network k_knn_t used to end with wrote an index twice and dropped another on the
    // device when three or more of the K best tied (profiles/EXPERIMENTS.md, tools/knn_tie_probe.hip).
    __device__ __forceinline__ void write_ranked(int32_t* __restrict__ out_row, int k) const {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            int place = 0;
#pragma unroll
            for (int s = 0; s < K; ++s) place += knn_before(d[s], i[s], d[t], i[t]) ? 1 : 0;
            if (place < k) out_row[place] = knn_index_or_none(i[t], K);
        }
    }
};

// One wave per query: lane l scans candidates l, l + 64, ... keeping its K best SORTED in registers (a K-step bubble per accept), then
// k rounds of a wave-wide minimum pop the K best of the 64 lists in order. k_knn_b keeps the same list. On purpose the two do NOT share
// a list type, and the bubble's test here is spelled out: either change makes the compiler predicate the bubble instead of branching
// over it -- k_knn<16> 80 -> 107 VGPRs (6 -> 4 waves per SIMD), k_knn_b<10> 62 -> 66 (8 -> 7): profiles/EXPERIMENTS.md.
template <int K>
__global__ __launch_bounds__(256) void k_knn(const float* __restrict__ xc, int nc, const float* __restrict__ xq, int nq, int k,
                                             int exclude_self, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const double q0 = (double)xq[qi * 3 + 0], q1 = (double)xq[qi * 3 + 1], q2 = (double)xq[qi * 3 + 2];
    double bd[K];
    int bi[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { bd[t] = __builtin_inf(); bi[t] = KNN_NONE; }
    // candidates four at a time: their twelve coordinate loads are in flight together (112 000 queries x 10 000 points 4.3 -> 3.7 ms,
    // 50 000 x 50 000 at k = 15 14.7 -> 10.4 ms, the 8 source queries of forward_fixed 210 -> 173 us)
    constexpr int UB = 4;
    for (int c0 = lane; c0 < nc; c0 += 64 * UB) {
        float cx[UB][3];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = min(c0 + 64 * u, nc - 1);
            cx[u][0] = xc[c * 3 + 0]; cx[u][1] = xc[c * 3 + 1]; cx[u][2] = xc[c * 3 + 2];
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = c0 + 64 * u;
            if (c >= nc || (exclude_self && c == qi)) continue;
            double d = knn_dist2(q0, q1, q2, cx[u][0], cx[u][1], cx[u][2]);
            int id = c;
            if (d < bd[K - 1]) {          // candidates arrive in increasing index order: a tie never displaces an earlier entry
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    if (d < bd[t] || (d == bd[t] && id < bi[t])) {       // knn_before, spelled out (above): a displaced entry that ties
                                                                          // with the next slot goes in front of it (it has the smaller index)
                        const double td = bd[t]; const int ti = bi[t];
                        bd[t] = d; bi[t] = id; d = td; id = ti;
                    }
                }
            }
        }
    }
    for (int r = 0; r < k; ++r) {
        double md = bd[0];
        int mi = bi[0];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const double od = __shfl_xor(md, s);
            const int oi = __shfl_xor(mi, s);
            if (knn_before(od, oi, md, mi)) { md = od; mi = oi; }
        }
        if (bi[0] == mi && bd[0] == md) {        // the owner pops its head (indices are unique across lanes; when the wave has run out
                                                 // of points every lane "owns" the empty slot, and shifting an all-empty list changes nothing)
#pragma unroll
            for (int t = 0; t + 1 < K; ++t) { bd[t] = bd[t + 1]; bi[t] = bi[t + 1]; }
            bd[K - 1] = __builtin_inf(); bi[K - 1] = KNN_NONE;
        }
        if (lane == 0) out[(long long)qi * k + r] = knn_index_or_none(mi, K);
    }
}

// A handful of queries (the one spatial query and the one candidate source of the association pass, process_continuous_days.py:1052;
// the 4-8 source queries of a training sample): with a wave per query ONE wave walked the whole context -- 134-170 us per call at 10 000
// grid nodes, twice per forward_fixed -- so a query gets a workgroup of 16 waves instead: every lane scans a 1024-th of the context
// (same exact arithmetic and per-lane lists as k_knn), every wave pops its K best into LDS, wave 0 merges the 16 lists. Same table.
template <int K>
__global__ __launch_bounds__(1024) void k_knn_b(const float* __restrict__ xc, int nc, const float* __restrict__ xq, int nq, int k,
                                                int exclude_self, int32_t* __restrict__ out) {
    __shared__ double sd[16 * K];
    __shared__ int si[16 * K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const double q0 = (double)xq[qi * 3 + 0], q1 = (double)xq[qi * 3 + 1], q2 = (double)xq[qi * 3 + 2];
    double bd[K];
    int bi[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { bd[t] = __builtin_inf(); bi[t] = KNN_NONE; }
    auto insert = [&](double d, int id) {
        if (knn_before(d, id, bd[K - 1], bi[K - 1])) {      // the full test: the merge below offers indices in no order
#pragma unroll
            for (int t = 0; t < K; ++t) {
                if (knn_before(d, id, bd[t], bi[t])) {
                    const double td = bd[t]; const int ti = bi[t];
                    bd[t] = d; bi[t] = id; d = td; id = ti;
                }
            }
        }
    };
    auto pop = [&](double& md, int& mi) {          // the wave's smallest (distance, index); its owner drops it
        md = bd[0]; mi = bi[0];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const double od = __shfl_xor(md, s);
            const int oi = __shfl_xor(mi, s);
            if (knn_before(od, oi, md, mi)) { md = od; mi = oi; }
        }
        if (bi[0] == mi && bd[0] == md && mi != KNN_NONE) {      // (the last test is idle: no wave here runs out of points)
#pragma unroll
            for (int t = 0; t + 1 < K; ++t) { bd[t] = bd[t + 1]; bi[t] = bi[t + 1]; }
            bd[K - 1] = __builtin_inf(); bi[K - 1] = KNN_NONE;
        }
    };
    for (int c = threadIdx.x; c < nc; c += 1024) {
        if (exclude_self && c == qi) continue;
        insert(knn_dist2(q0, q1, q2, xc[c * 3 + 0], xc[c * 3 + 1], xc[c * 3 + 2]), c);
    }
    for (int r = 0; r < K; ++r) {
        double md; int mi;
        pop(md, mi);
        if (lane == 0) { sd[wave * K + r] = md; si[wave * K + r] = mi; }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int t = 0; t < K; ++t) { bd[t] = __builtin_inf(); bi[t] = KNN_NONE; }
    for (int e = lane; e < 16 * K; e += 64)
        if (si[e] != KNN_NONE) insert(sd[e], si[e]);
    for (int r = 0; r < k; ++r) {
        double md; int mi;
        pop(md, mi);
        if (lane == 0) out[(long long)qi * k + r] = knn_index_or_none(mi, K);
    }
}

// ONE LANE per query, for large query sets (the refine pass's 112 000-point clouds, process_continuous_days.py:929: with a wave per
// query every candidate step paid a lane's insertion and the 64 partial lists were merged afterwards: 4.3 ms of the pass's 4.9 ms per
// source). Here a lane scans every candidate, in index order, against a KnnWorst list: after the first few hundred candidates a wave
// rarely leaves the fp32 distance-and-compare path.
constexpr int KNN_TILE = 2048;
template <int K>
__global__ __launch_bounds__(256) void k_knn_t(const float* __restrict__ xc, int nc, const float* __restrict__ xq, int nq, int k,
                                               int exclude_self, int32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[KNN_TILE * 4];
    const int qi = blockIdx.x * 256 + threadIdx.x;
    const int qc = qi < nq ? qi : nq - 1;
    const float f0 = xq[qc * 3 + 0], f1 = xq[qc * 3 + 1], f2 = xq[qc * 3 + 2];
    const double q0 = (double)f0, q1 = (double)f1, q2 = (double)f2;
    KnnWorst<K> best;
    best.clear();
    // tiles of the context staged in LDS, read by all lanes at the same address (a broadcast). (Reading the wave-uniform candidate
    // through the scalar cache instead -- three 16-byte scalar loads per four candidates, no staging, no barrier -- measured the same:
    // 2.44 against 2.38 ms at 112 000 x 10 000.)
    for (int c0 = 0; c0 < nc; c0 += KNN_TILE) {
        const int n = min(KNN_TILE, nc - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const float* p = xc + (long long)(c0 + i) * 3;
            *(f32x4*)(tile + i * 4) = f32x4{p[0], p[1], p[2], 0.f};
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const f32x4 cv = *(const f32x4*)(tile + i * 4);
            const float e0 = f0 - cv.x, e1 = f1 - cv.y, e2 = f2 - cv.z;
            if (!best.passes(e0 * e0 + e1 * e1 + e2 * e2)) continue;
            const int c = c0 + i;
            if (exclude_self && c == qi) continue;
            best.template offer<true>(knn_dist2(q0, q1, q2, cv.x, cv.y, cv.z), c);
        }
    }
    if (qi < nq) best.write_ranked(out + (long long)qi * k, k);
}
