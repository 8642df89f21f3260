// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the growable pick store of the online day loop
// (apply.PickStore), whose picks stay time-sorted on the device while chunks of a live feed arrive.

// ------------------------------------------------------------------------------------------------
// Merge by rank of two time-sorted runs of picks, the resident one (a, n_a elements) and a chunk (b, n_b), into a second buffer (o):
//   resident element i lands at i + #{chunk elements with t < t_a[i]}      (lower bound of t_a[i] in the chunk)
//   chunk element j    lands at j + #{resident elements with t <= t_b[j]}  (upper bound of t_b[j] in the resident run)
// i.e. the stable merge in which a resident pick precedes a chunk pick of the same time: the order of a stable sort by time of the
// resident picks followed by the chunk's (feed order). The two rank rules are each other's complement, so every output position is
// written by exactly one thread: no atomics. One thread per element of either run, a binary search in the other run, and the
// element's four fields (time f64, station i32, phase i32, row index i64) stored at its rank. The runs are small next to a window's
// work (a day's resident picks fit the L2), so the searches are not worth staging in LDS.
// ------------------------------------------------------------------------------------------------
struct PickRun {
    const double* t;
    const int32_t* sta;
    const int32_t* phase;
    const long long* index;
    long long n;
};

__global__ __launch_bounds__(256) void k_picks_merge(PickRun a, PickRun b, double* __restrict__ o_t, int32_t* __restrict__ o_sta,
                                                     int32_t* __restrict__ o_phase, long long* __restrict__ o_index) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n + b.n) return;
    const bool chunk = i >= a.n;
    const long long k = chunk ? i - a.n : i;
    const double t = (chunk ? b.t : a.t)[k];
    const double* other = chunk ? a.t : b.t;
    long long lo = 0, hi = chunk ? a.n : b.n;        // the first element of the other run that does not precede this one
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        const double u = other[mid];
        if (chunk ? u <= t : u < t) lo = mid + 1; else hi = mid;
    }
    const long long r = k + lo;
    o_t[r] = t;
    o_sta[r] = (chunk ? b.sta : a.sta)[k];
    o_phase[r] = (chunk ? b.phase : a.phase)[k];
    o_index[r] = (chunk ? b.index : a.index)[k];
}

// ------------------------------------------------------------------------------------------------
// The pick lists of one window (apply.ResidentPicks.pick_inputs = extract_pick_inputs_from_data, process_utils.py:644-699) in one
// launch: a contiguous range of the time-sorted store, cut by the ball query, stable-sorted by station -- a counting sort, since
// the key is a station index below n_sta. One workgroup of 256 threads:
//   1. histogram of the kept picks' stations in LDS (integer LDS adds: the counts do not depend on the order of the adds);
//   2. exclusive scan of the histogram: every thread sums its own contiguous segment of the table, a 256-wide scan of the segment
//      sums, and the segment is rewritten as running offsets; the grand total is the count;
//   3. placement, the range in chunks of 256 in order: a pick lands at (its station's running offset) + (the kept picks of the same
//      station on earlier threads of the chunk), then the running offsets are bumped -- so within a station the picks keep the
//      order of the range, which is what a stable sort gives.
// Every output slot is written by exactly one thread, with vector stores; nothing is atomic in global memory and the result does not
// depend on scheduling. A range of a few hundred picks is latency, not bandwidth: one workgroup, no second launch for the scan.
// A station outside [0, n_sta) cannot come out of a PickStore; such a pick is left out (the count shows it), never used as an index.
// ------------------------------------------------------------------------------------------------
constexpr int PL_BLOCK = 256;
constexpr int PL_MAX_STA = 8192;                      // the LDS station table: 32 KB of int32

__global__ __launch_bounds__(PL_BLOCK) void k_pick_lists(const double* __restrict__ t, const int32_t* __restrict__ sta,
                                                         const int32_t* __restrict__ phase, const long long* __restrict__ index, int n,
                                                         int n_sta, double t0, int ball, double centre, double radius,
                                                         double* __restrict__ o_tp, long long* __restrict__ o_ip,
                                                         double* __restrict__ o_ph, long long* __restrict__ o_idx,
                                                         long long* __restrict__ o_count) {
    __shared__ int table[PL_MAX_STA];                 // counts, then running offsets, per station
    __shared__ int part[2][PL_BLOCK];                 // the scan of the segment sums (two buffers, swapped per step)
    __shared__ __attribute__((aligned(16))) int chunk[PL_BLOCK];      // the stations of the chunk being placed (-1: not kept)
    const int tid = threadIdx.x;
    for (int s = tid; s < n_sta; s += PL_BLOCK) table[s] = 0;
    __syncthreads();
    // 1. histogram
    for (int i = tid; i < n; i += PL_BLOCK) {
        const int s = sta[i];
        const bool keep = (unsigned)s < (unsigned)n_sta && (!ball || fabs(t[i] - centre) <= radius);
        if (keep) atomicAdd(&table[s], 1);
    }
    __syncthreads();
    // 2. exclusive scan
    const int seg = (n_sta + PL_BLOCK - 1) / PL_BLOCK;
    const int s_lo = min(tid * seg, n_sta), s_hi = min(s_lo + seg, n_sta);
    int sum = 0;
    for (int s = s_lo; s < s_hi; ++s) sum += table[s];
    part[0][tid] = sum;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < PL_BLOCK; d <<= 1) {
        part[cur ^ 1][tid] = part[cur][tid] + (tid >= d ? part[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int run = part[cur][tid] - sum;                   // the kept picks of every station below this thread's segment
    for (int s = s_lo; s < s_hi; ++s) {
        const int c = table[s];
        table[s] = run;
        run += c;
    }
    if (tid == PL_BLOCK - 1) o_count[0] = (long long)part[cur][PL_BLOCK - 1];
    __syncthreads();
    // 3. placement
    for (int base = 0; base < n; base += PL_BLOCK) {
        const int i = base + tid;
        int s = -1;
        double ti = 0.0;
        if (i < n) {
            s = sta[i];
            ti = t[i];
            if (!((unsigned)s < (unsigned)n_sta && (!ball || fabs(ti - centre) <= radius))) s = -1;
        }
        chunk[tid] = s;
        __syncthreads();
        int pos = 0;
        if (s >= 0) pos = table[s];
        const int4* c4 = reinterpret_cast<const int4*>(chunk);
        for (int j = 0; j < PL_BLOCK / 4; ++j) {      // the same address on every lane: LDS broadcasts
            const int4 v = c4[j];
            const int j0 = 4 * j;
            pos += (v.x == s && j0 < tid) + (v.y == s && j0 + 1 < tid) + (v.z == s && j0 + 2 < tid) + (v.w == s && j0 + 3 < tid);
        }
        __syncthreads();                              // every thread has read the offsets and the chunk
        if (s >= 0) {
            atomicAdd(&table[s], 1);                  // (seen by the next chunk, after its barrier)
            o_tp[pos] = ti - t0;
            o_ip[pos] = (long long)s;
            o_ph[pos] = (double)phase[i];
            o_idx[pos] = index[i];
        }
    }
}
