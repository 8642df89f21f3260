// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the refine pass's selection of the refined
// source out of the legs' query read-outs (process_continuous_days.py:972-978), one launch pair per source.

// ------------------------------------------------------------------------------------------------
// acc[q, t] = ((0 + x_0[q, t] * inv) + x_1[q, t] * inv) + ...   in leg order, fp32, every product rounded before its add (contraction
// off: v_mul_f32 + v_add_f32) -- the bits of `acc = zeros; acc += x_l[:, :, 0] / n_scale` per leg, where torch divides a tensor by a
// host scalar as a multiplication by its fp32 reciprocal `inv`. Rows with keep[q] == 0 do not take part. Wanted: the FIRST row whose
// row maximum equals the global maximum and the first column of that row holding it (`argmax(acc.max(1)[0])`, then `argmax(acc[ip])`,
// both "first maximum"). That element is the one of smallest LINEAR index q * n_t + t among the elements equal to the global maximum:
// every earlier row has a smaller row maximum, hence no such element, and within the row the first column wins. So the reduction
// carries (value, linear index) pairs and prefers the greater value, then the smaller index: associative and commutative, hence
// independent of how threads, waves and workgroups split the elements -- no atomics, nothing depends on scheduling. An index of
// RS_NONE marks "no kept element yet" (no infinity is needed as a neutral value). NaN is out of scope: the inputs are finite
// sigmoid-range read-outs, and the library is built without NaN semantics.
// A thread walks i = first + k * stride (stride = all threads of the grid: consecutive lanes read consecutive floats of every leg);
// (q, t) of its first element cost one 64-bit division, every later one an add and a carry. Each x_l is read once, with 64-bit offsets.
// Pass 1 leaves one pair per workgroup in the caller's scratch, pass 2 (one workgroup) reduces those and writes the fp64 row
// (ip, it, value, any_kept) with ordinary vector stores; nothing kept (or Q = 0) gives (0, 0, -inf, 0), as torch's argmax over an
// all -inf `where(keep, acc, -inf)` does.
// ------------------------------------------------------------------------------------------------
constexpr int RS_MAX_LEGS = 32;                 // leg pointers travel by value in the kernel arguments: no device copy of a pointer table
constexpr int RS_BLOCK = 256;
constexpr int RS_PER_THREAD = 8;                // elements per thread at which the grid stops growing with the problem
constexpr int RS_SPAN = RS_BLOCK * RS_PER_THREAD;   // elements per workgroup up to RS_MAX_WG workgroups
constexpr int RS_MAX_WG = 1024;                 // pass 2 reduces at most this many partials: 4 per thread
constexpr long long RS_NONE = 0x7fffffffffffffffLL;

struct RsLegs {
    const float* x[RS_MAX_LEGS];
};

struct RsPartial {                              // 16 bytes per workgroup in the scratch
    long long i;
    float v;
    float pad;
};

__device__ __forceinline__ void rs_take(float& v, long long& i, float ov, long long oi) {
    if (oi != RS_NONE && (i == RS_NONE || ov > v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}

// the best pair of the workgroup, valid in thread 0; s_v / s_i: one slot per wave
__device__ __forceinline__ void rs_block_reduce(float& v, long long& i, float* s_v, long long* s_i) {
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(i, o);
        rs_take(v, i, ov, oi);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_v[wave] = v;
        s_i[wave] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < RS_BLOCK / 64; ++w) rs_take(v, i, s_v[w], s_i[w]);
}

// pass 1 of one source: workgroup blockIdx.x of gridDim.x over the n_elem elements of the read-outs legs.x[0 .. n_used), its pair to `part`
template <class Legs>
__device__ __forceinline__ void rs_partial(const Legs& legs, int n_used, long long n_elem, int n_t, const uint8_t* __restrict__ keep,
                                           float inv, RsPartial* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float s_v[RS_BLOCK / 64];
    __shared__ long long s_i[RS_BLOCK / 64];
    const long long stride = (long long)gridDim.x * RS_BLOCK;
    const long long dq = stride / n_t;
    const int dt = (int)(stride - dq * n_t);
    long long i = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    long long q = i / n_t;
    int t = (int)(i - q * n_t);
    float bv = 0.f;
    long long bi = RS_NONE;
    for (; i < n_elem; i += stride) {
        if (!keep || keep[q]) {
            float a = 0.f;
            for (int l = 0; l < n_used; ++l) {
                const float p = legs.x[l][i] * inv;
                a = a + p;
            }
            if (bi == RS_NONE || a > bv) {      // i ascends within a thread: an equal value never replaces an earlier one
                bv = a;
                bi = i;
            }
        }
        q += dq;
        t += dt;
        if (t >= n_t) {
            t -= n_t;
            ++q;
        }
    }
    rs_block_reduce(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) {
        RsPartial p;
        p.i = bi;
        p.v = bv;
        p.pad = 0.f;
        part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(RS_BLOCK) void k_refine_select_partial(RsLegs legs, int n_used, long long n_elem, int n_t,
                                                                     const uint8_t* __restrict__ keep, float inv,
                                                                     RsPartial* __restrict__ part) {
    rs_partial(legs, n_used, n_elem, n_t, keep, inv, part);
}

// pass 2: workgroup b (the single form launches one) reduces the n_part partials of source b into row b of out
__global__ __launch_bounds__(RS_BLOCK) void k_refine_select_final(const RsPartial* __restrict__ part, int n_part, int n_t,
                                                                   double* __restrict__ out) {
    __shared__ float s_v[RS_BLOCK / 64];
    __shared__ long long s_i[RS_BLOCK / 64];
    part += (long long)blockIdx.x * n_part;
    out += 4 * (long long)blockIdx.x;
    float bv = 0.f;
    long long bi = RS_NONE;
    for (int k = threadIdx.x; k < n_part; k += RS_BLOCK) rs_take(bv, bi, part[k].v, part[k].i);
    rs_block_reduce(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) {
        if (bi == RS_NONE) {
            out[0] = 0.0;
            out[1] = 0.0;
            ((unsigned long long*)out)[2] = 0xfff0000000000000ULL;      // -inf, as a bit pattern
            out[3] = 0.0;
        } else {
            const long long q = bi / n_t;
            out[0] = (double)q;
            out[1] = (double)(bi - q * n_t);
            out[2] = (double)bv;
            out[3] = 1.0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same selection for a batch of sources in one launch pair (the refine pass with `source_batch` > 1): blockIdx.y = source b, whose
// read-outs are row b of a DEVICE table [n_batch, n_legs] of pointers (a batch has up to 16 x 32 of them: too many to travel by value),
// a null entry = that leg produced no window for the source and is skipped, so the sum runs over the source's legs in leg order exactly as
// the single form's `n_used` pointers do. keep [n_batch, n_query], partials [n_batch, gridDim.x], out [n_batch, 4]. Per source the grid
// (gridDim.x = the single form's workgroup count), the element walk and the block reduction are the single form's (rs_partial), and
// pass 2 is k_refine_select_final with one workgroup per source, so row b carries its bits; the reduction is order-independent anyway.
// A workgroup compacts its source's non-null pointers into LDS once.
// ------------------------------------------------------------------------------------------------
struct RsLegsLds {
    const float* const* x;
};

__global__ __launch_bounds__(RS_BLOCK) void k_refine_select_partial_b(const float* const* __restrict__ table, int n_legs, long long n_query,
                                                                       int n_t, const uint8_t* __restrict__ keep, float inv,
                                                                       RsPartial* __restrict__ part) {
    __shared__ const float* s_x[RS_MAX_LEGS];
    __shared__ int s_used;
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        int u = 0;
        for (int l = 0; l < n_legs; ++l) {
            const float* p = table[(long long)b * n_legs + l];
            if (p) s_x[u++] = p;
        }
        s_used = u;
    }
    __syncthreads();
    RsLegsLds legs;
    legs.x = s_x;
    rs_partial(legs, s_used, n_query * n_t, n_t, keep ? keep + (long long)b * n_query : nullptr, inv, part + (long long)b * gridDim.x);
}
