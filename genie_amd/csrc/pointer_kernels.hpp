// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the time-pointer tables of the association
// heads (`assemble_time_pointers_for_stations`, utils.py:602-622; genie_amd/graph.py::time_pointers is the host statement), built on
// the device by genie_time_pointers.

// ------------------------------------------------------------------------------------------------
// Wanted, per phase, station i and time step t_j: the k candidates of station i smallest under the key (|double(trv) - t_j|, product-node
// id), nearest first. The key is a total order, so the answer does not depend on how it is found:
//
//   1. k_tp_bins<false>   every (product node, phase) entry finds its BIN among the time steps, b = #{j : t_j <= trv} (bin b holds
//                         t_{b-1} <= trv < t_b; n_t + 1 bins), and counts itself in cnt[phase][station][b].
//   2. k_tp_scan          exclusive prefix sum of a (phase, station)'s bin counts -> start[.][0 .. n_t + 1] (start[n_t + 1] = the
//                         station's candidates); cnt becomes the fill cursors. k_tp_segments: exclusive prefix of the stations'
//                         candidate counts = where a station's candidates begin (used by the irregular form; the Cartesian one has
//                         i * G), and the number of stations with none.
//   3. k_tp_bins<true>    the entries again, each written to its bin's next free slot as (trv bits << 32 | id): a counting sort by bin.
//                         The order INSIDE a bin depends on scheduling; nothing below depends on it.
//   4. k_tp_select        one wave per (phase, station, time step j). Bins <= j lie left of t_j (trv < t_j), bins > j right of it. Whole
//                         bins are taken leftwards until they hold k candidates (or none are left), and rightwards likewise -- two binary
//                         searches in `start`. A candidate of a bin further out on one side is STRICTLY further from t_j than the >= k
//                         taken on that side, so it is not among the k nearest whatever its id: the k smallest keys of the taken range
//                         are the k smallest of the station. The wave keeps the best 64 keys sorted, one per lane, streams the range in
//                         chunks of 64 and inserts what beats the key at rank k - 1; lanes 0 .. k-1 store rank r mod n (a station with
//                         n < k candidates cycles through them).
//
// All-equal travel times put a whole station in one bin: the range is then every candidate, i.e. the full ranking the reference does. No
// size limit inside: segments live in global memory. Entries whose travel time is not finite (an integer test on the bits: the library
// is built without NaN semantics) are skipped by both passes alike and raise status[1]; an out-of-range station index likewise is skipped.
// Stores are ordinary vector stores; the atomics are vector atomics on the counters.
//
// Source-node-sharded model (genie_time_pointers_candidates + genie_time_pointers_merge, genie_amd/dist.py): a rank holds the travel
// times of its OWNED source nodes only, rows in its local node order. The same four steps run over those rows with the GLOBAL
// product-node id in every key (`node_global`: local source node -> global one), and k_tp_select<true> emits, per (phase, station,
// time step), its min(k, n_own) best as (bits of the float64 distance, global id) pairs -- padded to k with the key (max double, max
// int), which sorts after every candidate and is never listed; no cycling. The k smallest of the union of the ranks' lists are the k
// smallest of the station (each rank's list holds every one of ITS candidates that can be among them), so after one all-gather
// k_tp_merge ranks world x k keys per entry with the same wave-wide insertion and writes the replicated tables.
// ------------------------------------------------------------------------------------------------
constexpr int TP_MAX_K = 32;                    // ranks kept per (station, time step): at most one per lane of half a wave
constexpr int TP_BLOCK = 256;
constexpr int TP_WAVES = TP_BLOCK / 64;         // time steps per workgroup of k_tp_select
constexpr int TP_MAX_WG = 1 << 16;              // k_tp_bins walks the entries with a grid stride beyond this many workgroups

struct TpLayout {                               // byte offsets into the caller's scratch
    size_t sorted, cnt, start, seg, ncand, total;
};

inline size_t tp_pad(size_t b) { return (b + 255) & ~(size_t)255; }

inline TpLayout tp_layout(int64_t n_prod, int n_sta, int n_t) {
    TpLayout L;
    size_t o = 0;
    L.sorted = o; o += tp_pad(sizeof(unsigned long long) * 2 * (size_t)n_prod);
    L.cnt = o;    o += tp_pad(sizeof(int32_t) * 2 * (size_t)n_sta * (size_t)(n_t + 1));
    L.start = o;  o += tp_pad(sizeof(int32_t) * 2 * (size_t)n_sta * (size_t)(n_t + 2));
    L.seg = o;    o += tp_pad(sizeof(int32_t) * ((size_t)n_sta + 1));
    L.ncand = o;  o += tp_pad(sizeof(int32_t) * (size_t)n_sta);
    L.total = o;
    return L;
}

// #{j : t[j] <= x} for t ascending
__device__ __forceinline__ int tp_bin(const double* __restrict__ t, int n_t, double x) {
    int lo = 0, hi = n_t;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// trv [P, 2]; sta_of [P] or null (Cartesian: station = p mod S, segment of station i = [i * G, (i + 1) * G)); cnt [2][S][n_t + 1]
template <bool FILL>
__global__ __launch_bounds__(TP_BLOCK) void k_tp_bins(const float* __restrict__ trv, const int32_t* __restrict__ sta_of, long long P, int S,
                                                      long long G, const double* __restrict__ t, int n_t, int32_t* __restrict__ cnt,
                                                      const int32_t* __restrict__ seg, unsigned long long* __restrict__ sorted,
                                                      int32_t* __restrict__ status, const int32_t* __restrict__ node_global = nullptr) {
    const long long n = 2 * P, stride = (long long)gridDim.x * TP_BLOCK;
    for (long long e = (long long)blockIdx.x * TP_BLOCK + threadIdx.x; e < n; e += stride) {
        const long long p = e >> 1;
        const int ph = (int)(e & 1);
        const unsigned bits = __float_as_uint(trv[e]);
        if ((bits & 0x7f800000u) == 0x7f800000u) {           // inf / NaN: never a candidate
            if (!FILL) atomicOr(status + 1, 1);
            continue;
        }
        const int i = sta_of ? sta_of[p] : (int)(p % S);
        if ((unsigned)i >= (unsigned)S) continue;
        const int b = tp_bin(t, n_t, (double)__uint_as_float(bits));
        int32_t* c = cnt + ((size_t)ph * S + i) * (size_t)(n_t + 1) + b;
        if (!FILL) {
            atomicAdd(c, 1);
        } else {
            const long long pos = (seg ? (long long)seg[i] : (long long)i * G) + atomicAdd(c, 1);
            // a shard's rows (Cartesian form only): the key carries the GLOBAL product-node id of local row p = l * S + i
            const long long id = node_global ? (long long)node_global[p / S] * S + i : p;
            sorted[(size_t)ph * (size_t)P + (size_t)pos] = ((unsigned long long)bits << 32) | (unsigned long long)(unsigned)id;
        }
    }
}

// exclusive prefix sum of src[0 .. n) by one workgroup: dst[0 .. n) (and dst2, when given) get the prefix, the return value is the total
// (valid in every thread). s_buf: TP_BLOCK ints.
__device__ __forceinline__ int tp_block_scan(const int32_t* src, int n, int32_t* dst, int32_t* dst2, int* s_buf) {
    int running = 0;
    for (int base = 0; base < n; base += TP_BLOCK) {
        const int idx = base + (int)threadIdx.x;
        const int v = idx < n ? src[idx] : 0;
        s_buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < TP_BLOCK; o <<= 1) {
            const int add = (int)threadIdx.x >= o ? s_buf[threadIdx.x - o] : 0;
            __syncthreads();
            s_buf[threadIdx.x] += add;
            __syncthreads();
        }
        const int incl = s_buf[threadIdx.x], total = s_buf[TP_BLOCK - 1];
        __syncthreads();
        if (idx < n) {
            dst[idx] = running + incl - v;
            if (dst2) dst2[idx] = running + incl - v;
        }
        running += total;
    }
    return running;
}

// one workgroup per (phase, station): cnt [n_t + 1] counts -> start [n_t + 2] offsets; cnt becomes the cursors of the fill pass
__global__ __launch_bounds__(TP_BLOCK) void k_tp_scan(int32_t* __restrict__ cnt, int32_t* __restrict__ start, int S, int n_t,
                                                      int32_t* __restrict__ ncand) {
    __shared__ int s_buf[TP_BLOCK];
    const size_t sg = blockIdx.x;
    int32_t* c = cnt + sg * (size_t)(n_t + 1);
    int32_t* s = start + sg * (size_t)(n_t + 2);
    const int total = tp_block_scan(c, n_t + 1, s, c, s_buf);
    if (threadIdx.x == 0) {
        s[n_t + 1] = total;
        atomicMax(ncand + sg % (size_t)S, total);            // (the phases differ only where a travel time is not finite)
    }
}

// one workgroup: seg [S + 1] = exclusive prefix of the stations' candidate counts, status[0] = stations without a candidate
__global__ __launch_bounds__(TP_BLOCK) void k_tp_segments(const int32_t* __restrict__ ncand, int S, int32_t* __restrict__ seg,
                                                          int32_t* __restrict__ status) {
    __shared__ int s_buf[TP_BLOCK];
    __shared__ int s_empty;
    if (threadIdx.x == 0) s_empty = 0;
    __syncthreads();
    int empty = 0;
    for (int i = threadIdx.x; i < S; i += TP_BLOCK) empty += ncand[i] == 0 ? 1 : 0;
    if (empty) atomicAdd(&s_empty, empty);
    const int total = tp_block_scan(ncand, S, seg, nullptr, s_buf);   // (its barriers order s_empty as well)
    if (threadIdx.x == 0) {
        seg[S] = total;
        status[0] = s_empty;
    }
}

constexpr double TP_EMPTY_D = 1.7976931348623157e308;     // (max double, max int): an empty rank; after every candidate in knn_before's order
constexpr int TP_EMPTY_ID = 0x7fffffff;

// One chunk of up to 64 keys (one per lane, `have`: this lane holds one) into the wave's sorted list (lane r: the key of rank r): what
// beats the key at rank k - 1 is inserted, one key at a time. Every lane takes part in the shuffles.
__device__ __forceinline__ void tp_wave_insert(double& kd, int& kid, double d, int id, bool have, int k, int lane) {
    const double td = __shfl(kd, k - 1);
    const int tid = __shfl(kid, k - 1);
    unsigned long long m = __ballot(have && knn_before(d, id, td, tid));
    while (m) {                                               // wave-uniform
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const double cd = __shfl(d, src);
        const int cid = __shfl(id, src);
        if (!knn_before(cd, cid, __shfl(kd, k - 1), __shfl(kid, k - 1))) continue;   // rank k - 1 has moved past it meanwhile
        const double pd = __shfl_up(kd, 1);
        const int pid = __shfl_up(kid, 1);
        if (knn_before(cd, cid, kd, kid)) {                      // it ranks before mine: I take my left neighbour's key, or the new one
            const bool shift = lane > 0 && knn_before(cd, cid, pd, pid);
            kd = shift ? pd : cd;
            kid = shift ? pid : cid;
        }
    }
}

typedef long long tp_ll2 __attribute__((ext_vector_type(2)));     // one emitted key: (bits of the float64 distance, product-node id)

// CAND: the keys go to cand [2][S][n_t][k] instead of the ids to the tables (a rank of a source-node-sharded model)
template <bool CAND>
__global__ __launch_bounds__(TP_BLOCK) void k_tp_select(const unsigned long long* __restrict__ sorted, const int32_t* __restrict__ start,
                                                        const int32_t* __restrict__ seg, long long P, long long G, int S,
                                                        const double* __restrict__ t, int n_t, int k, int32_t* __restrict__ out_p,
                                                        int32_t* __restrict__ out_s, tp_ll2* __restrict__ cand_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (n_t + TP_WAVES - 1) / TP_WAVES;
    const int i = (int)(blockIdx.x / (unsigned)groups);
    const int j = (int)(blockIdx.x % (unsigned)groups) * TP_WAVES + wave;
    const int ph = blockIdx.y;
    if (j >= n_t) return;                                     // (a whole wave; the kernel has no barrier)
    const int32_t* B = start + ((size_t)ph * S + i) * (size_t)(n_t + 2);
    int32_t* out = CAND ? nullptr : (ph ? out_s : out_p) + ((size_t)i * n_t + j) * (size_t)k;
    tp_ll2* ck = CAND ? cand_out + (((size_t)ph * S + i) * (size_t)n_t + j) * (size_t)k : nullptr;
    const int n = B[n_t + 1];
    if (n <= 0) {                                             // no candidate: the caller reads status[0] and raises
        if (lane < k) {
            if (CAND) ck[lane] = tp_ll2{__double_as_longlong(TP_EMPTY_D), (long long)TP_EMPTY_ID};
            else out[lane] = 0;
        }
        return;
    }
    const int mid = B[j + 1];                                 // candidates left of t_j
    int a = 0, b = n;
    if (mid > k) {                                            // the largest bin lo <= j with k candidates in bins lo .. j
        int lo = 0, hi = j;
        while (lo < hi) {
            const int m = (lo + hi + 1) >> 1;
            if (mid - B[m] >= k) lo = m; else hi = m - 1;
        }
        a = B[lo];
    }
    if (n - mid > k) {                                        // the smallest e > j + 1 with k candidates in bins j + 1 .. e - 1
        int lo = j + 1, hi = n_t + 1;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (B[m] - mid >= k) hi = m; else lo = m + 1;
        }
        b = B[lo];
    }
    const unsigned long long* cand = sorted + (size_t)ph * (size_t)P + (size_t)(seg ? (long long)seg[i] : (long long)i * G);
    const double tj = t[j];
    double kd = TP_EMPTY_D;                                   // lane r: the key of rank r so far
    int kid = TP_EMPTY_ID;
    for (int c0 = a; c0 < b; c0 += 64) {
        const int c = c0 + lane;
        const bool have = c < b;
        double d = TP_EMPTY_D;
        int id = TP_EMPTY_ID;
        if (have) {
            const unsigned long long e = cand[c];
            id = (int)(unsigned)e;
            d = fabs((double)__uint_as_float((unsigned)(e >> 32)) - tj);
        }
        tp_wave_insert(kd, kid, d, id, have, k, lane);
    }
    if (CAND) {                                               // ranks >= n stay empty: a rank that owns fewer than k nodes does not cycle
        if (lane < k) ck[lane] = tp_ll2{__double_as_longlong(kd), (long long)kid};
        return;
    }
    const int id_out = __shfl(kid, lane % (n < 64 ? n : 64));
    if (lane < k) out[lane] = id_out;
}

// The ranks' lists merged: cand [world][2][S][n_t][k] keys, every rank's k ascending (empty ones last) -> the k_out <= k smallest of the
// world * k per (phase, station, time step), nearest first, as int32 ids in the tables [S][n_t][k_out]. One wave per entry, as
// k_tp_select: lane c of a chunk reads key c % k of rank c / k (k consecutive 16-byte keys per rank). An entry with fewer than k_out
// real keys (the ranks' lists do not cover the station: an inconsistent call) sets status[0].
__global__ __launch_bounds__(TP_BLOCK) void k_tp_merge(const tp_ll2* __restrict__ cand, int world, int S, int n_t, int k, int k_out,
                                                       int32_t* __restrict__ out_p, int32_t* __restrict__ out_s, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (n_t + TP_WAVES - 1) / TP_WAVES;
    const int i = (int)(blockIdx.x / (unsigned)groups);
    const int j = (int)(blockIdx.x % (unsigned)groups) * TP_WAVES + wave;
    const int ph = blockIdx.y;
    if (j >= n_t) return;                                     // (a whole wave; the kernel has no barrier)
    const size_t entry = (((size_t)ph * S + i) * (size_t)n_t + j) * (size_t)k, rank_stride = 2 * (size_t)S * (size_t)n_t * (size_t)k;
    const int total = world * k;
    double kd = TP_EMPTY_D;
    int kid = TP_EMPTY_ID;
    for (int c0 = 0; c0 < total; c0 += 64) {
        const int c = c0 + lane;
        const bool have = c < total;
        double d = TP_EMPTY_D;
        int id = TP_EMPTY_ID;
        if (have) {
            const int r = c / k;
            const tp_ll2 e = cand[(size_t)r * rank_stride + entry + (size_t)(c - r * k)];
            d = __longlong_as_double(e.x);
            id = (int)e.y;
        }
        tp_wave_insert(kd, kid, d, id, have, k_out, lane);    // (an empty key never beats the list's own empty ranks)
    }
    if (lane < k_out) {
        const bool empty = kid == TP_EMPTY_ID;
        if (empty) atomicOr(status, 1);
        ((ph ? out_s : out_p) + ((size_t)i * n_t + j) * (size_t)k_out)[lane] = empty ? 0 : kid;
    }
}
