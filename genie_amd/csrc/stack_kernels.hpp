// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the apply loop's stacking of window read-outs
// into Out_2 (process_continuous_days.py:797-805), one launch per flush.

// ------------------------------------------------------------------------------------------------
// Out_2[q, cols[k][j]] += x[k, q, j] * scale, for k = 0..B-1 and j = 0..T-1 IN THAT ORDER, entries cols[k][j] < 0 skipped.
// Windows of a flush overlap in columns (at 1 s stride a column is fed by 6-8 of them), so the work is split by OUTPUT element:
// one thread owns one (q, c) of the flush's column range [c_min, c_min + width) and walks the B x T table (in LDS; every lane reads
// the same entry: a broadcast) in (k, j) order. No atomics: the owner adds its contributions in window order, which is the order
// of the torch loop this replaces (`Out_2.index_add_` per window), so the sums carry the same bits. Lanes are consecutive in c: the
// read-modify-write of Out_2 and the reads of x[k, q, :] are contiguous runs. An entry outside the range matches no thread, so no
// table content can make a thread write outside its own element. Contraction is off: the product is rounded before the add (v_mul_f32 +
// v_add_f32, no v_fma_f32), as the two torch kernels round it.
// ------------------------------------------------------------------------------------------------
constexpr int SW_MAX_B = 16;
constexpr int SW_MAX_T = 64;

__global__ __launch_bounds__(256) void k_stack_windows(const float* __restrict__ x, const int32_t* __restrict__ cols, int B, long long Q,
                                                       int T, float scale, float* __restrict__ out, long long n_cols, int c_min,
                                                       int width) {
#pragma clang fp contract(off)
    __shared__ int32_t s_cols[SW_MAX_B * SW_MAX_T];
    for (int i = threadIdx.x; i < B * T; i += 256) s_cols[i] = cols[i];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q * width) return;
    const long long q = i / width;
    const int c = c_min + (int)(i - q * width);
    float* o = out + q * n_cols + c;                 // 64-bit element offset: a day is 10 000 x 115 200 > 2^31 elements
    float acc = *o;
    bool hit = false;
    for (int k = 0; k < B; ++k) {
        const float* xk = x + ((long long)k * Q + q) * T;
        for (int j = 0; j < T; ++j) {
            if (s_cols[k * T + j] == c) {
                const float v = xk[j] * scale;
                acc = acc + v;
                hit = true;
            }
        }
    }
    if (hit) *o = acc;
}
