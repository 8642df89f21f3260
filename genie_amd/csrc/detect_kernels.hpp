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
// (d) Peak candidates of a SEGMENT of Out_2's columns: what k_row_select MODE 1 finds on the full matrix, found on a piece of it.
// THE DEFINITION, stated here for all three paths (k_row_select in aux_kernels.hpp follows it on the dense matrix): a peak is a
// maximal run of equal values >= thr whose two outer neighbours are lower, reported at the run's midpoint (start + end) / 2; a
// run that holds global column 0 or n_cols - 1 has no outer neighbour there and is no peak (scipy `_local_maxima_1d`). pk_is_peak is
// that sentence; pk_scan (with pk_load and pk_run_start) is the only code that loads a chunk and that knows how a run's start is found.
// seg [rows, width] (row stride `stride`) holds the global columns [lo, lo + width) of an axis of n_cols columns. One wave per row
// walks it in chunks of 64 columns, one coalesced load per chunk, issued one chunk ahead; the neighbours come from the adjacent lanes
// (lane 0's from the carry, lane 63's by one load of the next column), a run's start from a ballot of the lanes where the value
// changes, or from the carry when the run began in an earlier chunk. PkCarry is wave-uniform: `last` the value of the column before
// the chunk, `start` the GLOBAL column where the run that holds it began, `rise` whether the value before that run was lower (0 when
// unknown: the run holds column 0 or began at a cut left end). Peaks are decided at the run's END lane, in ascending column order.
// Each kernel loops over chunks: scanner, end policy, emitter; COUNT and FILL differ in pk_emit's stores alone. The end policies:
// * BAND (`postproc.detect_sources_banded`, k_band_peaks): the segment is a column band [b_lo, b_lo + width) of the finished axis, and
//   only the peaks whose column lies in the caller's OWN range [o_lo, o_hi) are reported; own ranges partition the axis, so exactly
//   one band reports a run. The carry lives in registers. A run that touches an end of the band which is not an end of the axis may
//   go on outside: its start (end) is only bounded, start in [1, b_lo] (end in [b_hi - 1, n_cols - 2]). If the known side is lower
//   and some admissible midpoint falls into the own range, the band cannot decide: *flag is set and the run not reported (the caller
//   falls back to the dense merge). If no admissible midpoint is the caller's, the run is another rank's in every case and is passed
//   over (so a rank whose own range is empty reports nothing and never sets the flag).
// * STREAM (`postproc.StreamPeaks`, k_stream_peaks): the segment is the next block [c0, c0 + width) of closed columns of the online
//   day loop; blocks arrive in order and without gaps. Where the band flags, the stream carries: the carry is kept per row in
//   device memory from call to call (with c0 == 0 carry_in is not read). A call decides every run whose end it knows: those that
//   end inside the block with their successor in the block (sp_decide) and the carried run when the block's first value differs
//   from `last` (sp_carried). The carried run's end lane is gone, so lane 0 emits it at rank 0, ahead of everything the block
//   yields: a row's columns ascend within a call and from call to call. A run that reaches the block's last column is deferred
//   through the carry -- if that column is n_cols - 1 no later call comes and it is no peak. No flag, no fallback. COUNT reads
//   carry_in, writes carry_out, counts and lowers *bound; FILL reads the same carry_in: neither pass reads what the other writes.
//   *bound (set to c0 + width by k_stream_bound_init in front of the COUNT launch): no peak a LATER call emits has a column below
//   it. Only runs still open at the block's end can yield one below c0 + width; such a run [start, e], e >= c0 + width - 1, is
//   reported at (start + e) / 2 >= (start + c0 + width - 1) / 2, and only if it reaches thr, rose and does not hold column 0:
//   one atomicMin per such row, by lane 0.
// ------------------------------------------------------------------------------------------------
constexpr int PK_ROWS_PER_BLOCK = 4;
struct __attribute__((aligned(16))) PkCarry { float last; int32_t rise; long long start; };
static_assert(sizeof(PkCarry) == 16, "genie_stream_peaks_carry_bytes hands this size to the caller");
struct PkRun {                                            // per lane, of the run that ends at this lane (if one does)
    bool ends, last_col;                                  // `last_col`: the lane is the segment's last column, `right` is then unknown
    float v, right;
    unsigned long long brk, rise; long long lane0; PkCarry open;      // where the run began, read through pk_run_start: the chunk's
};                                                        // ballots, lane 0's global column, the carry in front of the chunk

// a run [start, end] of value v with the neighbours' verdicts `rose` (the left one is lower) and `right`
__device__ __forceinline__ bool pk_is_peak(float v, float thr, bool rose, float right, long long start, long long end, long long n_cols) {
    return v >= thr && rose && right < v && start > 0 && end < n_cols - 1;
}

// a lane's column of the chunk [c0, c0 + 64) of a row of `width` >= 1 columns and the column behind the chunk (lane 63's right neighbour).
// Unconditional (past the row's end the row's last column is read, and not used) so that the NEXT chunk's loads can stay in flight
struct PkLoad { float v, next; };
__device__ __forceinline__ PkLoad pk_load(const float* __restrict__ xr, long long c0, int lane, long long width) {
    const long long j = c0 + lane, n = c0 + 64;
    return PkLoad{xr[j < width ? j : width - 1], xr[n < width ? n : width - 1]};
}

// the chunk [c0, c0 + 64) of the segment [lo, lo + width) in the row xr; advances the carry. `cut_left`: the segment's first column
// starts a run whatever came before it, and whether that run rose is unknown (it is in any case when the column is global column 0).
// `ahead` holds this chunk's values (pk_load of chunk 0 first) and leaves with the next chunk's, loading while this one is decided
__device__ __forceinline__ PkRun pk_scan(const float* __restrict__ xr, long long c0, int lane, long long width, long long lo,
                                         bool cut_left, PkCarry& carry, PkLoad& ahead) {
    const long long j = c0 + lane;
    const bool valid = j < width;
    const float v = valid ? ahead.v : 0.f, next = ahead.next;
    ahead = pk_load(xr, c0 + 64, lane, width);
    float left = __shfl_up(v, 1);
    if (lane == 0) left = carry.last;
    float right = __shfl_down(v, 1);
    if (lane == 63 && j + 1 < width) right = next;
    const bool first = j == 0 && (cut_left || lo == 0);                       // no left neighbour
    const bool brk = valid && (first || left != v);                           // a run starts here
    const bool rise = valid && !first && left < v;
    const unsigned long long bm = __ballot(brk), rm = __ballot(rise);
    const bool last_col = j == width - 1;
    const PkRun r{valid && (last_col || right != v), last_col, v, right, bm, rm, lo + c0, carry};
    const long long rest = width - 1 - c0;                                    // the chunk's last valid lane holds the carry's value
    carry.last = __shfl(v, rest < 63 ? (int)rest : 63);
    if (bm) {
        const int ls = 63 - __clzll(bm);
        carry.start = lo + c0 + ls;
        carry.rise = (int32_t)((rm >> ls) & 1ull);
    }
    return r;
}

// the global start of the run that ends at this lane and whether it rose. The policies ask only at the end of a run that reaches thr:
// most chunks of a day hold none, and what every chunk executes is what the walk's time is made of
__device__ __forceinline__ bool pk_run_start(const PkRun& r, int lane, long long* start) {
    const unsigned long long below = r.brk & ((2ull << lane) - 1ull);         // none: the run began in an earlier chunk
    const int ls = below ? 63 - __clzll(below) : 0;
    *start = below ? r.lane0 + ls : r.open.start;
    return below ? (r.rise >> ls) & 1ull : r.open.rise != 0;
}

// ranks the wave's selected lanes behind the `total` triplets the row has so far; FILL writes (row, col, val) at base + total + rank
template <bool COUNT>
__device__ __forceinline__ void pk_emit(bool sel, int lane, long long row, long long col, float val, long long base, long long& total,
                                        int32_t* __restrict__ out_row, int32_t* __restrict__ out_col, float* __restrict__ out_val) {
    const unsigned long long b = __ballot(sel);
    if (!COUNT && sel) {
        const long long o = base + total + __popcll(b & ((1ull << lane) - 1ull));
        out_row[o] = (int32_t)row; out_col[o] = (int32_t)col; out_val[o] = val;
    }
    total += __popcll(b);
}

struct BpGeom { long long width, b_lo, o_lo, o_hi, n_cols; float thr; };
struct SpGeom { long long width, c0, n_cols; float thr; };

// the band's end policy on the run that ends at global column `end`: a peak of the own range, undecidable, or neither
__device__ __forceinline__ bool bp_decide(const PkRun& r, int lane, const BpGeom& g, long long* col, bool* undecided) {
    bool sel = false, und = false;
    if (r.ends && r.v >= g.thr) {
        long long start;
        const bool rose = pk_run_start(r, lane, &start);
        const long long end = r.lane0 + lane;
        const bool left_known = start > g.b_lo, right_known = !r.last_col;
        const long long m_lo = ((left_known ? start : 1) + end) / 2;         // the admissible midpoints, inclusive
        const long long m_hi = (start + (right_known ? end : g.n_cols - 2)) / 2;
        const bool mine = g.o_lo < g.o_hi && m_hi >= g.o_lo && m_lo < g.o_hi;        // (an empty own range has no midpoint)
        if (left_known && right_known) {                                      // (then m_lo == m_hi)
            sel = mine && pk_is_peak(r.v, g.thr, rose, r.right, start, end, g.n_cols);
        } else {                                                              // lower on the known side, possibly so on the other
            const bool left_ok = left_known ? rose : g.b_lo > 0;
            const bool right_ok = right_known ? r.right < r.v : g.b_lo + g.width < g.n_cols;
            und = mine && left_ok && right_ok;
        }
        *col = m_lo;
    }
    *undecided = und;
    return sel;
}

// the stream's end policy: a run whose successor is in the block is decided, one that reaches the block's end is left to the carry
__device__ __forceinline__ bool sp_decide(const PkRun& r, int lane, const SpGeom& g, long long* col) {
    if (!(r.ends && !r.last_col && r.v >= g.thr)) return false;
    long long start;
    const bool rose = pk_run_start(r, lane, &start);
    const long long end = r.lane0 + lane;
    *col = (start + end) / 2;
    return pk_is_peak(r.v, g.thr, rose, r.right, start, end, g.n_cols);
}

// the run carried into the block, decided by the block's first value
__device__ __forceinline__ bool sp_carried(const SpGeom& g, const PkCarry& carry, float first, long long* col) {
    if (g.c0 == 0 || first == carry.last) return false;                        // no previous column / the run goes on
    *col = (carry.start + g.c0 - 1) / 2;
    return pk_is_peak(carry.last, g.thr, carry.rise != 0, first, carry.start, g.c0 - 1, g.n_cols);
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_band_peaks(const float* __restrict__ band, int rows, long long stride, BpGeom g,
                                                    int32_t* __restrict__ counts, const long long* __restrict__ offsets,
                                                    int32_t* __restrict__ out_row, int32_t* __restrict__ out_col,
                                                    float* __restrict__ out_val, int32_t* flag) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * PK_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = band + row * stride;
    const long long base = COUNT ? 0 : offsets[row];
    PkCarry carry{0.f, 0, g.b_lo};
    long long total = 0;
    bool any_und = false;
    if (g.width == 0) { if (COUNT && lane == 0) counts[row] = 0; return; }    // (nothing to load)
    PkLoad ahead = pk_load(xr, 0, lane, g.width);
    for (long long c0 = 0; c0 < g.width; c0 += 64) {
        const PkRun r = pk_scan(xr, c0, lane, g.width, g.b_lo, true, carry, ahead);
        long long col = 0;
        bool und;
        const bool sel = bp_decide(r, lane, g, &col, &und);
        pk_emit<COUNT>(sel, lane, row, col, r.v, base, total, out_row, out_col, out_val);
        any_und |= und;
    }
    if (COUNT && lane == 0) counts[row] = (int32_t)total;
    if (__any(any_und) && lane == 0) atomicOr(flag, 1);
}

// Column occupancy of the held candidates (`postproc.OnlineDetector`): one thread per new candidate, ring[col mod W] += 1. Integer
// atomics commute, so the counts do not depend on the schedule. The slot is taken on the unsigned column: always inside [0, W).
__global__ __launch_bounds__(256) void k_col_counts(const int32_t* __restrict__ cols, long long n, int32_t* ring, unsigned W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    atomicAdd(&ring[(unsigned)cols[i] % W], 1);
}

__global__ void k_stream_bound_init(long long* bound, long long value) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *bound = value;
}

// launched with width >= 1 only
template <bool COUNT>
__global__ __launch_bounds__(256) void k_stream_peaks(const float* __restrict__ block, int rows, long long stride, SpGeom g,
                                                      const PkCarry* __restrict__ carry_in, PkCarry* __restrict__ carry_out,
                                                      int32_t* __restrict__ counts, long long* bound,
                                                      const long long* __restrict__ offsets, int32_t* __restrict__ out_row,
                                                      int32_t* __restrict__ out_col, float* __restrict__ out_val) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * PK_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = block + row * stride;
    const long long base = COUNT ? 0 : offsets[row];
    PkCarry carry{0.f, 0, 0};
    if (g.c0 > 0) carry = carry_in[row];
    long long total = 0;
    {
        long long col = 0;
        const bool sel = sp_carried(g, carry, xr[0], &col) && lane == 0;
        pk_emit<COUNT>(sel, lane, row, col, carry.last, base, total, out_row, out_col, out_val);
    }
    PkLoad ahead = pk_load(xr, 0, lane, g.width);
    for (long long c0 = 0; c0 < g.width; c0 += 64) {
        const PkRun r = pk_scan(xr, c0, lane, g.width, g.c0, false, carry, ahead);
        long long col = 0;
        const bool sel = sp_decide(r, lane, g, &col);
        pk_emit<COUNT>(sel, lane, row, col, r.v, base, total, out_row, out_col, out_val);
    }
    if (COUNT && lane == 0) {
        counts[row] = (int32_t)total;
        carry_out[row] = carry;
        if (g.c0 + g.width < g.n_cols && carry.last >= g.thr && carry.rise != 0 && carry.start > 0)
            atomicMin((unsigned long long*)bound, (unsigned long long)((carry.start + g.c0 + g.width - 1) / 2));
    }
}
