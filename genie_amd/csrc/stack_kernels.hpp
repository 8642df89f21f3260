// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the apply loop's stacking of window read-outs
// into Out_2 (process_continuous_days.py:797-805), one launch per flush.

// ------------------------------------------------------------------------------------------------
// Out_2[q, cols[k][j]] += x_l[k, q, j] * scale, for k = 0..B-1, then j = 0..T-1, then l = 0..L-1 INNERMOST, entries cols[k][j] < 0
// skipped. x_l: the read-outs of the L source grids ("legs") of a day (process_continuous_days.py:761-810: `for n in times_need: for
// x_grid_ind in x_grid_ind_list:`, every leg adding into the one Out_2); a single-grid loop is L = 1.
// Windows of a flush overlap in columns (at 1 s stride a column is fed by 6-8 of them), so the work is split by OUTPUT element:
// one thread owns one (q, c) of the flush's column range [c_min, c_min + width) and walks the B x T table (in LDS; every lane reads
// the same entry: a broadcast) in (k, j) order. No atomics: the owner adds its contributions in window order. A table row that lists no
// column twice (window_cols_table makes such rows) gives every output element at most one j per window, so the owner's order (k, l) is
// the order of the torch loop this replaces, `for window: for leg: Out_2.index_add_(...)`, and the sums carry the same bits. Lanes are
// consecutive in c: the read-modify-write of Out_2 and the reads of x_l[k, q, :] are contiguous runs. An entry outside the range matches
// no thread, so no table content can make a thread write outside its own element, and an element no entry lists is not written at all.
// Contraction is off: the product is rounded before the add (v_mul_f32 + v_add_f32, no v_fma_f32), as the two torch kernels round it.
// The leg pointers travel by value in the kernel arguments, as k_refine_select_partial takes them: the loop over l indexes the
// kernel-argument segment (scalar loads), no private copy of the table exists and nothing is copied to the device before the launch.
// RING (the online day loop): out is a ring [Q, n_cols] of the day's open columns and the element of column c lives in slot c % n_cols;
// everything else is the dense kernel, statement for statement, so a column's running sum carries the same bits in either form. The
// launcher admits a range narrower than the ring only: two columns of one launch never share a slot.
// ------------------------------------------------------------------------------------------------
constexpr int SW_MAX_B = 16;
constexpr int SW_MAX_T = 64;
constexpr int SW_MAX_LEGS = 32;

struct SwLegs {
    const float* x[SW_MAX_LEGS];
};

template <bool RING>
__global__ __launch_bounds__(256) void k_stack_windows(SwLegs legs, int L, const int32_t* __restrict__ cols, int B, long long Q, int T,
                                                       float scale, float* __restrict__ out, long long n_cols, int c_min, int width) {
#pragma clang fp contract(off)
    __shared__ int32_t s_cols[SW_MAX_B * SW_MAX_T];
    for (int i = threadIdx.x; i < B * T; i += 256) s_cols[i] = cols[i];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q * width) return;
    const long long q = i / width;
    const int c = c_min + (int)(i - q * width);
    float* o = out + q * n_cols + (RING ? (long long)c % n_cols : (long long)c);   // 64-bit element offset: a day is 10 000 x 115 200 > 2^31 elements
    float acc = *o;
    bool hit = false;
    for (int k = 0; k < B; ++k) {
        const long long row = ((long long)k * Q + q) * T;      // 64-bit element offset into every leg's x
        for (int j = 0; j < T; ++j) {
            if (s_cols[k * T + j] == c) {
                for (int l = 0; l < L; ++l) {
                    const float v = legs.x[l][row + j] * scale;
                    acc = acc + v;
                }
                hit = true;
            }
        }
    }
    if (hit) *o = acc;
}

// ------------------------------------------------------------------------------------------------
// out[q, j] = ring[q, (c_lo + j) % W]; ring[q, (c_lo + j) % W] = 0, for j = 0..n-1 (n <= W: every slot is read and zeroed by exactly one
// thread): the columns [c_lo, c_lo + n) of the online day loop leave the ring as a dense block and their slots are free for the columns
// W further on. One pass, one thread per element, lanes consecutive in j (the block's rows are contiguous runs, the ring's wrap at most
// once per row).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ring_close(float* __restrict__ ring, long long Q, long long W, long long c_lo, long long n,
                                                    float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q * n) return;
    const long long q = i / n;
    float* r = ring + q * W + (c_lo + (i - q * n)) % W;
    out[i] = *r;
    *r = 0.f;
}

// ------------------------------------------------------------------------------------------------
// The ring's open columns as a checkpoint (apply.OnlineDay.state_dict / load_state_dict), k_ring_close's indexing without its zeroing:
// k_ring_save reads, out[q, j] = ring[q, (c_lo + j) % W], and writes nothing of the ring; k_ring_load is the inverse store,
// ring[q, (c_lo + j) % W] = block[q, j], into a ring whose W may differ from the saving ring's (n <= W: every slot written by exactly one
// thread, every other slot untouched). The dense block is what travels, so neither side knows the other's W.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ring_save(const float* __restrict__ ring, long long Q, long long W, long long c_lo, long long n,
                                                   float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q * n) return;
    const long long q = i / n;
    out[i] = ring[q * W + (c_lo + (i - q * n)) % W];
}

__global__ __launch_bounds__(256) void k_ring_load(float* __restrict__ ring, long long Q, long long W, long long c_lo, long long n,
                                                   const float* __restrict__ block) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q * n) return;
    const long long q = i / n;
    ring[q * W + (c_lo + (i - q * n)) % W] = block[i];
}
