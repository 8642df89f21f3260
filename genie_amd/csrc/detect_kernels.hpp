// Source detection after the apply loop, on the device (process_continuous_days.py:843-891, LocalMarching of process_utils.py:40-100):
// the distance rule of scipy.signal.find_peaks per query row, the time groups separated by gaps >= break_win, and LocalMarching
// (max propagation over a space-time radius graph) on time-sorted nodes. Included by genie_hip.hip (inside its anonymous namespace).
// Everything here is integer / compare work and exact fp64 distances: the host functions of genie_amd/postproc.py are the oracle,
// and the results are equal to theirs flag for flag.
#pragma once

// ------------------------------------------------------------------------------------------------
// (a) Distance rule of find_peaks (scipy `_select_by_peak_distance`): walking from the highest peak of a row down, a kept peak
// removes every other peak of the row closer than d columns. The walk has a unique result for a strict priority order, and that
// result is the fixed point of a local rule: a peak is KEPT once every higher-priority peak within d is removed, and REMOVED once
// any peak within d is kept. One wave per row repeats that rule over the row's undecided peaks until none is left (the highest
// undecided peak is always decided, so the loop ends; a day's rows settle in two or three rounds).
// Priority order: height, then column -- of two equal heights within d the LATER column wins (what a stable ascending sort walked
// from the end gives; scipy's own order for exact ties is an unstable sort's and therefore unspecified).
// `col` ascends within a row (genie_row_select_fill order). State lives in `keep` itself: 0 undecided, 1 kept, 2 removed; 2 becomes 0
// at the end. Only this wave touches its row's flags; the workgroup-scope fence orders its lanes' stores and loads between rounds.
// ------------------------------------------------------------------------------------------------
constexpr int PD_ROWS_PER_BLOCK = 4;
__global__ __launch_bounds__(256) void k_peak_distance(const long long* __restrict__ offsets, int rows, long long n,
                                                       const int32_t* __restrict__ col, const float* __restrict__ val, int d,
                                                       unsigned char* keep) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * PD_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    long long a = offsets[row], b = row + 1 < rows ? offsets[row + 1] : n;
    a = a < 0 ? 0 : (a > n ? n : a);                     // offsets are the caller's: never index outside [0, n)
    b = b < a ? a : (b > n ? n : b);
    if (b - a <= 1) {
        if (lane == 0 && b > a) keep[a] = 1;
        return;
    }
    volatile unsigned char* st = keep;
    for (long long k = a + lane; k < b; k += 64) st[k] = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    bool open = true;
    while (open) {
        open = false;
        for (long long k0 = a; k0 < b; k0 += 64) {
            const long long k = k0 + lane;
            if (k < b && st[k] == 0) {
                const int ck = col[k];
                const float vk = val[k];
                bool kept_near = false, higher_open = false;
                for (long long j = k - 1; j >= a && ck - col[j] < d; --j) {
                    const unsigned char s = st[j];
                    kept_near |= s == 1;
                    higher_open |= s == 0 && val[j] > vk;                     // an earlier column wins only when strictly higher
                }
                for (long long j = k + 1; j < b && col[j] - ck < d; ++j) {
                    const unsigned char s = st[j];
                    kept_near |= s == 1;
                    higher_open |= s == 0 && val[j] >= vk;                    // a later column wins ties
                }
                if (kept_near) st[k] = 2;
                else if (!higher_open) st[k] = 1;
                else open = true;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        open = __any(open);
    }
    for (long long k = a + lane; k < b; k += 64)
        if (st[k] == 2) st[k] = 0;
}

// ------------------------------------------------------------------------------------------------
// (b) Time groups of time-sorted nodes (`group_sources`, process_continuous_days.py:856-870): node i starts a new group when
// t[i] - t[i - 1] >= break_win; group[i] = number of starts in 1..i. Two passes over blocks of TG_BLOCK nodes: the starts of every
// block are counted, then a block adds the counts of the blocks before it (a few hundred words for a day) to its own running count.
// ------------------------------------------------------------------------------------------------
constexpr int TG_BLOCK = 4096;                           // nodes per workgroup: 256 threads x 16 consecutive nodes
__device__ __forceinline__ int tg_block_scan(int mine, int* total) {      // exclusive sum of `mine` over the 256 threads
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(inc, s);
        if (lane >= s) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (k < wave) before += wsum[k]; all += wsum[k]; }
    *total = all;
    return before + inc - mine;
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_time_groups(const double* __restrict__ t, long long n, double break_win,
                                                     int32_t* __restrict__ block_counts, int32_t* __restrict__ group) {
    __shared__ int s_base;
    const long long i0 = (long long)blockIdx.x * TG_BLOCK + (long long)threadIdx.x * 16;
    unsigned starts = 0;                                  // bit u: node i0 + u starts a group
    int mine = 0;
    if (i0 < n) {
        double prev = i0 > 0 ? t[i0 - 1] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const long long i = i0 + u;
            if (i >= n) break;
            const double ti = t[i];
            if (i > 0 && ti - prev >= break_win) { starts |= 1u << u; ++mine; }
            prev = ti;
        }
    }
    int all;
    const int before = tg_block_scan(mine, &all);
    if (!FILL) {
        if (threadIdx.x == 0) block_counts[blockIdx.x] = all;
        return;
    }
    if (threadIdx.x < 64) {                               // starts of the blocks before this one
        int s = 0;
        for (int k = threadIdx.x; k < (int)blockIdx.x; k += 64) s += block_counts[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (threadIdx.x == 0) s_base = s;
    }
    __syncthreads();
    int g = s_base + before;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const long long i = i0 + u;
        if (i >= n) break;
        g += (starts >> u) & 1u;
        group[i] = g;
    }
}

// ------------------------------------------------------------------------------------------------
// (c) LocalMarching on nodes sorted by time (`postproc.local_marching`, process_utils.py:46-100).
//   j is an in-neighbour of i  <=>  same group, (t_i - t_j)^2 <= tc_win^2 and ((dx0^2 + dx1^2) + dx2^2) <= sp_win^2
// in fp64, every product and sum rounded on its own (cKDTree.query_ball_point is inclusive and the host does not fuse: with times on a
// 0.75 s grid and tc_win = 9 x 0.75 the pairs exactly on the time radius are the common case). i is its own neighbour.
//   active_i = i has a neighbour other than itself (the host's connected component of size > 1);
//   use_directed keeps the edges with val0[i] <= val0[j];
//   a step: new_i = max(0, max over the kept in-neighbours j of vals_j) for active nodes, inactive nodes keep their value;
//   the march ends after the step whose max |new - vals| <= tol;   keep_i = !active_i || |val0_i - vals_i| <= 1e-8 + tol |vals_i| (fp32).
// Because t ascends, the candidates of the 256 consecutive nodes of a workgroup are ONE contiguous index range (two binary searches
// with a margin that covers the rounding of the bounds: the range only has to contain every neighbour, each pair is decided by the
// exact test). The range goes through LDS in chunks; all lanes read the same candidate (a broadcast), each thread owns the maximum of
// its node: no atomics on values. The pair tests are recomputed in every step (production runs two) instead of storing an edge list.
// Steps are launched back to back without a host round trip: `diff` holds three rotating words, step s writes the bit pattern of its
// max |new - vals| into word s % 3 (non-negative floats order like unsigned integers), reads word (s - 1) % 3 and clears word
// (s + 1) % 3; once a step met `tol`, the later ones only copy the values through.
// ------------------------------------------------------------------------------------------------
constexpr int LM_CHUNK = 512;
struct __attribute__((aligned(16))) LmPos { double x0, x1, x2, t; };
struct __attribute__((aligned(16))) LmAux { float v, v0; int32_t g, pad; };

// the pair rule; contraction is off so that hipcc emits v_mul_f64 / v_add_f64 and no v_fma_f64 here
__device__ __forceinline__ bool lm_linked(double xi0, double xi1, double xi2, double ti, const LmPos& c, double tc2, double sp2) {
#pragma clang fp contract(off)
    const double dt = ti - c.t;
    const double d0 = xi0 - c.x0, d1 = xi1 - c.x1, d2 = xi2 - c.x2;
    const double dt2 = dt * dt;
    const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
    return dt2 <= tc2 && r2 <= sp2;
}

template <bool DIRECTED>
__global__ __launch_bounds__(256) void k_local_marching_step(const double* __restrict__ xs, const double* __restrict__ t,
                                                             const float* __restrict__ val0, const int32_t* __restrict__ group,
                                                             const float* __restrict__ vals_in, float* __restrict__ vals_out,
                                                             unsigned char* __restrict__ active, long long n, double tc_win,
                                                             double tc2, double sp2, double tol, int step, unsigned* diff) {
    __shared__ LmPos s_pos[LM_CHUNK];
    __shared__ LmAux s_aux[LM_CHUNK];
    __shared__ long long s_range[2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const long long ic = live ? i : n - 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) diff[(step + 1) % 3] = 0u;
    if (step > 0 && (double)__uint_as_float(diff[(step - 1) % 3]) <= tol) {           // the march has ended: pass the values on
        if (live) vals_out[i] = vals_in[i];
        return;
    }
    if (threadIdx.x < 2) {
        const long long first = (long long)blockIdx.x * 256, last = min(first + 255, n - 1);
        const double tf = t[first], tl = t[last];
        const double w = tc_win + (tc_win * 1e-9 + (fabs(tf) + fabs(tl) + tc_win) * 1e-14);
        long long lo = 0, hi = n;
        if (threadIdx.x == 0) {                           // first j with t[j] >= tf - w
            const double b = tf - w;
            hi = first;
            while (lo < hi) { const long long m = (lo + hi) >> 1; if (t[m] < b) lo = m + 1; else hi = m; }
        } else {                                          // first j with t[j] > tl + w
            const double b = tl + w;
            lo = last + 1;
            while (lo < hi) { const long long m = (lo + hi) >> 1; if (t[m] <= b) lo = m + 1; else hi = m; }
        }
        s_range[threadIdx.x] = lo;
    }
    const double xi0 = xs[ic * 3 + 0], xi1 = xs[ic * 3 + 1], xi2 = xs[ic * 3 + 2], ti = t[ic];
    const float v0i = val0[ic], vi = vals_in[ic];
    const int gi = group ? group[ic] : 0;
    float best = 0.f;                                     // the host scatters into zeros: `max` of an empty set is 0
    bool act = false;
    __syncthreads();
    const long long lo = s_range[0], hi = s_range[1];
    for (long long c0 = lo; c0 < hi; c0 += LM_CHUNK) {
        const int m = (int)min((long long)LM_CHUNK, hi - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < m; e += 256) {
            const long long j = c0 + e;
            s_pos[e] = LmPos{xs[j * 3 + 0], xs[j * 3 + 1], xs[j * 3 + 2], t[j]};
            s_aux[e] = LmAux{vals_in[j], val0[j], group ? group[j] : 0, 0};
        }
        __syncthreads();
        for (int e = 0; e < m; ++e) {
            const LmAux a = s_aux[e];
            if (lm_linked(xi0, xi1, xi2, ti, s_pos[e], tc2, sp2) && a.g == gi) {
                act |= c0 + e != i;
                if (!DIRECTED || v0i <= a.v0) best = fmaxf(best, a.v);
            }
        }
    }
    const float nv = act ? best : vi;
    float dv = live ? fabsf(nv - vi) : 0.f;
    if (live) { vals_out[i] = nv; active[i] = act ? 1 : 0; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) dv = fmaxf(dv, __shfl_xor(dv, o));
    if ((threadIdx.x & 63) == 0 && dv > 0.f) atomicMax(&diff[step % 3], __float_as_uint(dv));
}

// keep_i = !active_i || |val0_i - vals_i| <= 1e-8 + tol |vals_i|, in fp32 with every operation rounded on its own: numpy evaluates the
// host line on float32 arrays, the Python floats 1e-8 and tol enter as float32
__global__ __launch_bounds__(256) void k_local_marching_keep(const float* __restrict__ val0, const float* __restrict__ vals,
                                                             const unsigned char* __restrict__ active, long long n, float tol,
                                                             unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v0 = val0[i], v = vals[i];
    const bool same = fabsf(__fsub_rn(v0, v)) <= __fadd_rn(1e-8f, __fmul_rn(tol, fabsf(v)));
    keep[i] = (!active[i] || same) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// (d) Peak candidates of a column BAND of Out_2 (`postproc.detect_sources_banded`): what k_row_select MODE 1 finds on the full matrix,
// restricted to the peaks whose reported column lies in the caller's OWN range [o_lo, o_hi). band [rows, width] (row stride `stride`)
// holds the global columns [b_lo, b_lo + width) of an axis of n_cols columns. A peak is a maximal run of equal values >= thr whose two
// outer neighbours are lower, reported at the run's midpoint (start + end) / 2; a run that contains global column 0 or n_cols - 1 has
// no outer neighbour there and is no peak (scipy `_local_maxima_1d`). The ranks' own ranges partition the axis, so of all the bands
// that see a run exactly one reports it.
// A run that touches an end of the band which is not an end of the axis may go on outside: its start (its end) is then only bounded,
// start in [1, b_lo] (end in [b_hi - 1, n_cols - 2]). If the neighbour on the known side is lower and some admissible midpoint falls
// into the own range, the band cannot decide the peak: *flag is set and nothing is reported for that run (the caller falls back to the
// dense merge). If no admissible midpoint is the caller's, the run is another rank's in every case and is passed over in silence (so a rank
// whose own range is empty reports nothing and never sets the flag).
// One wave per row walks it in chunks of 64 columns, one coalesced load per chunk; the neighbours come from the adjacent lanes
// (lane 0's from the chunk before, lane 63's by one load of the next column), a run's start from a ballot of the lanes where the
// value changes, or from the wave-uniform carry when the run began in an earlier chunk. Peaks are decided at the run's END lane, so
// they come out in ascending column order. bp_chunk is the one decision both passes make: COUNT adds up its ballots, FILL ranks them.
// ------------------------------------------------------------------------------------------------
constexpr int BP_ROWS_PER_BLOCK = 4;
struct BpGeom { long long width, b_lo, o_lo, o_hi, n_cols; float thr; };
struct BpCarry { float last; long long start; bool rise; };       // wave-uniform: the previous column's value, the open run's start

__device__ __forceinline__ bool bp_chunk(const float* __restrict__ xr, long long c0, int lane, const BpGeom& g, BpCarry& carry,
                                         long long* col, float* val, bool* undecided) {
    const long long j = c0 + lane;
    const bool valid = j < g.width;
    const float v = valid ? xr[j] : 0.f;
    float left = __shfl_up(v, 1);
    if (lane == 0) left = carry.last;
    float right = __shfl_down(v, 1);
    if (lane == 63 && j + 1 < g.width) right = xr[j + 1];
    const bool brk = valid && (j == 0 || left != v);                         // a run starts here
    const bool rise = valid && j > 0 && left < v;
    const unsigned long long bm = __ballot(brk), rm = __ballot(rise);
    bool sel = false, und = false;
    if (valid && v >= g.thr && (j == g.width - 1 || right != v)) {            // the end of a run that reaches the threshold
        const unsigned long long below = bm & ((2ull << lane) - 1ull);
        long long s = carry.start;
        bool rising = carry.rise;
        if (below) {
            const int ls = 63 - __clzll(below);
            s = c0 + ls;
            rising = (rm >> ls) & 1ull;
        }
        const bool left_known = s > 0, right_known = j < g.width - 1;
        const bool left_ok = left_known ? rising : g.b_lo > 0;                // lower on the left, or possibly so
        const bool right_ok = right_known ? right < v : g.b_lo + g.width < g.n_cols;
        if (left_ok && right_ok) {
            const long long gs = g.b_lo + s, ge = g.b_lo + j;
            const long long m_lo = ((left_known ? gs : 1) + ge) / 2;          // the admissible midpoints, inclusive
            const long long m_hi = (gs + (right_known ? ge : g.n_cols - 2)) / 2;
            const bool mine = g.o_lo < g.o_hi && m_hi >= g.o_lo && m_lo < g.o_hi;    // (an empty own range has no midpoint)
            sel = mine && left_known && right_known;                           // (then m_lo == m_hi)
            und = mine && !(left_known && right_known);
            *col = m_lo;
        }
    }
    *val = v;
    *undecided = und;
    carry.last = __shfl(v, 63);
    if (bm) {
        const int ls = 63 - __clzll(bm);
        carry.start = c0 + ls;
        carry.rise = (rm >> ls) & 1ull;
    }
    return sel;
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_band_peaks(const float* __restrict__ band, int rows, long long stride, BpGeom g,
                                                    int32_t* __restrict__ counts, const long long* __restrict__ offsets,
                                                    int32_t* __restrict__ out_row, int32_t* __restrict__ out_col,
                                                    float* __restrict__ out_val, int32_t* flag) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * BP_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = band + row * stride;
    const long long base = COUNT ? 0 : offsets[row];
    BpCarry carry{0.f, 0, false};
    long long total = 0;
    bool any_und = false;
    for (long long c0 = 0; c0 < g.width; c0 += 64) {
        long long col = 0;
        float val;
        bool und;
        const bool sel = bp_chunk(xr, c0, lane, g, carry, &col, &val, &und);
        const unsigned long long b = __ballot(sel);
        if (!COUNT && sel) {
            const long long o = base + total + __popcll(b & ((1ull << lane) - 1ull));
            out_row[o] = (int32_t)row; out_col[o] = (int32_t)col; out_val[o] = val;
        }
        total += __popcll(b);
        any_und |= und;
    }
    if (COUNT && lane == 0) counts[row] = (int32_t)total;
    if (__any(any_und) && lane == 0) atomicOr(flag, 1);
}

// ------------------------------------------------------------------------------------------------
// (e) Peak candidates of a STREAM of column blocks (`postproc.StreamPeaks`, the online day loop's closed columns): the peaks of
// k_row_select MODE 1 on the full matrix, found block by block. block [rows, width] (row stride `stride`) holds the global columns
// [c0, c0 + width) of an axis of n_cols columns; blocks arrive in order and without gaps. The definition is (d)'s: a maximal run of
// equal values >= thr whose two outer neighbours are lower, reported at (start + end) / 2; a run that holds column 0 or n_cols - 1
// is no peak. Where (d) has to flag a run that touches an end of its band, the stream carries it: per row, SpCarry is what BpCarry
// holds wave-uniformly inside one call, kept in device memory from call to call -- `last` the value of column c0 - 1, `start` the
// GLOBAL column where the run that holds it began, `rise` whether the value before that run was lower (0 if the run holds column
// 0). Before the first block (c0 == 0) there is no previous column and carry_in is not read.
// A call decides every run whose end it knows: the runs that end inside the block with their successor in the block (at the END
// lane, sp_chunk) and the carried run when the block's first value differs from `last` (sp_carried). The carried run's end lane is
// gone, so lane 0 emits it at rank 0, ahead of everything the block itself yields: a row's columns ascend within a call and
// from call to call. A run that reaches the block's last column is deferred through the carry -- if that column is n_cols - 1 no
// later call comes and it is no peak. No flag, no fallback.
// COUNT reads carry_in, writes carry_out, counts and lowers *bound; FILL reads the same carry_in and writes the triplets at
// offsets[row] + rank: neither pass reads what the other writes, and both take every decision from sp_carried / sp_chunk.
// *bound (set to c0 + width by k_stream_bound_init in front of the COUNT launch): no peak a LATER call emits has a column below
// it. The only peaks of later calls that can lie below c0 + width are those of runs still open at the block's end; such a run
// [start, e] with e >= c0 + width - 1 is reported at (start + e) / 2 >= (start + c0 + width - 1) / 2, and only if it reaches thr, rose
// and does not hold column 0: one atomicMin per such row, by lane 0.
// ------------------------------------------------------------------------------------------------
constexpr int SP_ROWS_PER_BLOCK = 4;
struct __attribute__((aligned(16))) SpCarry { float last; int32_t rise; long long start; };
struct SpGeom { long long width, c0, n_cols; float thr; };

// the run carried into the block, decided by the block's first value
__device__ __forceinline__ bool sp_carried(const SpGeom& g, const SpCarry& carry, float first, long long* col) {
    if (g.c0 == 0 || first == carry.last) return false;                        // no previous column / the run goes on
    *col = (carry.start + g.c0 - 1) / 2;
    return carry.last >= g.thr && carry.rise != 0 && first < carry.last;
}

// the runs that end inside the chunk [cc, cc + 64) of the block with their successor in the block; advances the carry
__device__ __forceinline__ bool sp_chunk(const float* __restrict__ xr, long long cc, int lane, const SpGeom& g, SpCarry& carry,
                                         long long* col, float* val) {
    const long long j = cc + lane, gj = g.c0 + j;
    const bool valid = j < g.width;
    const float v = valid ? xr[j] : 0.f;
    float left = __shfl_up(v, 1);
    if (lane == 0) left = carry.last;
    float right = __shfl_down(v, 1);
    if (lane == 63 && j + 1 < g.width) right = xr[j + 1];
    const bool brk = valid && (gj == 0 || left != v);                          // a run starts here
    const bool rise = valid && gj > 0 && left < v;
    const unsigned long long bm = __ballot(brk), rm = __ballot(rise);
    bool sel = false;
    if (valid && j < g.width - 1 && right != v && v >= g.thr) {                // the known end of a run that reaches the threshold
        const unsigned long long below = bm & ((2ull << lane) - 1ull);
        long long s = carry.start;
        bool rising = carry.rise != 0;
        if (below) {
            const int ls = 63 - __clzll(below);
            s = g.c0 + cc + ls;
            rising = (rm >> ls) & 1ull;
        }
        sel = rising && right < v;                                             // (`rising` implies s > 0)
        *col = (s + gj) / 2;
    }
    *val = v;
    const long long rest = g.width - 1 - cc;                                   // the chunk's last valid lane holds the carry's value
    carry.last = __shfl(v, rest < 63 ? (int)rest : 63);
    if (bm) {
        const int ls = 63 - __clzll(bm);
        carry.start = g.c0 + cc + ls;
        carry.rise = (int32_t)((rm >> ls) & 1ull);
    }
    return sel;
}

__global__ void k_stream_bound_init(long long* bound, long long value) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *bound = value;
}

// launched with width >= 1 only
template <bool COUNT>
__global__ __launch_bounds__(256) void k_stream_peaks(const float* __restrict__ block, int rows, long long stride, SpGeom g,
                                                      const SpCarry* __restrict__ carry_in, SpCarry* __restrict__ carry_out,
                                                      int32_t* __restrict__ counts, long long* bound,
                                                      const long long* __restrict__ offsets, int32_t* __restrict__ out_row,
                                                      int32_t* __restrict__ out_col, float* __restrict__ out_val) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * SP_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = block + row * stride;
    const long long base = COUNT ? 0 : offsets[row];
    SpCarry carry{0.f, 0, 0};
    if (g.c0 > 0) carry = carry_in[row];
    long long total = 0;
    {
        long long col = 0;
        if (sp_carried(g, carry, xr[0], &col)) {
            if (!COUNT && lane == 0) { out_row[base] = (int32_t)row; out_col[base] = (int32_t)col; out_val[base] = carry.last; }
            total = 1;
        }
    }
    for (long long cc = 0; cc < g.width; cc += 64) {
        long long col = 0;
        float val;
        const bool sel = sp_chunk(xr, cc, lane, g, carry, &col, &val);
        const unsigned long long b = __ballot(sel);
        if (!COUNT && sel) {
            const long long o = base + total + __popcll(b & ((1ull << lane) - 1ull));
            out_row[o] = (int32_t)row; out_col[o] = (int32_t)col; out_val[o] = val;
        }
        total += __popcll(b);
    }
    if (COUNT && lane == 0) {
        counts[row] = (int32_t)total;
        carry_out[row] = carry;
        if (g.c0 + g.width < g.n_cols && carry.last >= g.thr && carry.rise != 0 && carry.start > 0)
            atomicMin((unsigned long long*)bound, (unsigned long long)((carry.start + g.c0 + g.width - 1) / 2));
    }
}
