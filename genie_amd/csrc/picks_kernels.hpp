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
