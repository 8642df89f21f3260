// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the refine pass's query cloud of one candidate
// source (process_continuous_days.py:929, :934), drawn where it is consumed -- one launch per source, nothing crosses from the host.

// ------------------------------------------------------------------------------------------------
// The draw is a pure function of (key, source, element): Philox4x64-10 as numpy's `np.random.Philox` runs it, so that
//   r = np.random.Generator(np.random.Philox(key=[key0, key1], counter=[0, source, 0, 0])).random((n, 3))
// holds as bits. Flat element j of the row-major [n, 3] array is word j % 4 of Philox block j / 4; the counter of block b is
// (b + 1, source, 0, 0): numpy's `philox_next` increments counter word 0 BEFORE it generates, and hands the four words of a block out in
// order. One round maps (c0, c1, c2, c3) to (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0) with hi0:lo0 = M0 * c0 and hi1:lo1 = M1 * c2 (64 x
// 64 -> 128 bit), and the key is bumped by the two Weyl constants after every round; `Generator.random` makes a double of a word u as
// (u >> 11) * 2^-53 (exact: a 53-bit integer times a power of two).
// The cloud: Xc[j] = src[j % 3] + (r[j] * off_range[j % 3] + off_min[j % 3]) in fp64, every operation rounded on its own (contraction
// off: v_mul_f64, v_add_f64, v_add_f64) -- the bits of torch's `src + (r * off_range + off_min)`, three element-wise kernels; xq[j] =
// (float)Xc[j], round to nearest = `Xc.float()`.
// One thread owns one Philox block = four consecutive flat elements (blocks straddle the rows of [n, 3]: harmless on flat arrays); the
// axis of element 4 b + k is (b + k) % 3 because 4 = 1 mod 3, so a thread pays one 64-bit remainder and then counts. The three small
// vectors travel by value in the kernel arguments and are picked with selects (no indexed kernel-argument array: that would go through
// scratch memory). A full block is written as 2 x 16 B (fp64) and 1 x 16 B (fp32) per array, the last, partial block element by element
// below 3 n; 64-bit offsets throughout. 256 threads span 1 024 elements per workgroup up to RC_MAX_WG workgroups, beyond which threads
// stride. No LDS, no atomics, no scratch memory, no verdict word: nothing here can fail on the device.
// ------------------------------------------------------------------------------------------------
constexpr int RC_BLOCK = 256;
constexpr int RC_MAX_WG = 1024;                 // 4 workgroups per CU of a 256-CU device; 2^20 elements per sweep of the grid
constexpr unsigned long long RC_M0 = 0xD2E7470EE14C6C93ULL, RC_M1 = 0xCA5A826395121157ULL;      // Philox4x64 multipliers
constexpr unsigned long long RC_W0 = 0x9E3779B97F4A7C15ULL, RC_W1 = 0xBB67AE8584CAA73BULL;      // Weyl constants of the key schedule

struct RcAxes {                                 // per axis: the source's Cartesian position, X_offset_range, X_offset_min
    double sx, sy, sz;
    double rx, ry, rz;
    double mx, my, mz;
};

// One source's cloud around (sx, sy, sz) (a's own position is not read), by the workgroups of grid axis x. `vec`: r, xc and xq are 16-byte aligned, full blocks go out as 16-byte stores
// (else element by element: the same values).
__device__ __forceinline__ void rc_cloud(unsigned long long key0, unsigned long long key1, unsigned long long source, long long n_elem,
                                         const double sx, const double sy, const double sz, const RcAxes& a, double* __restrict__ r, double* __restrict__ xc, float* __restrict__ xq,
                                         const bool vec) {
#pragma clang fp contract(off)
    const long long n_blk = (n_elem + 3) >> 2;
    const long long stride = (long long)gridDim.x * RC_BLOCK;
    for (long long b = (long long)blockIdx.x * RC_BLOCK + threadIdx.x; b < n_blk; b += stride) {
        unsigned long long c0 = (unsigned long long)b + 1ull, c1 = source, c2 = 0ull, c3 = 0ull, k0 = key0, k1 = key1;
#pragma unroll
        for (int round = 0; round < 10; ++round) {
            const unsigned long long hi0 = __umul64hi(RC_M0, c0), lo0 = RC_M0 * c0;
            const unsigned long long hi1 = __umul64hi(RC_M1, c2), lo1 = RC_M1 * c2;
            c0 = hi1 ^ c1 ^ k0;
            c1 = lo1;
            c2 = hi0 ^ c3 ^ k1;
            c3 = lo0;
            k0 += RC_W0;
            k1 += RC_W1;
        }
        const unsigned long long u[4] = {c0, c1, c2, c3};
        double d[4], x[4];
        float f[4];
        int ax = (int)(b % 3);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = (double)(u[k] >> 11) * (1.0 / 9007199254740992.0);
            const double rg = ax == 0 ? a.rx : (ax == 1 ? a.ry : a.rz);
            const double mn = ax == 0 ? a.mx : (ax == 1 ? a.my : a.mz);
            const double s = ax == 0 ? sx : (ax == 1 ? sy : sz);
            const double p = d[k] * rg;
            const double o = p + mn;
            x[k] = s + o;
            f[k] = (float)x[k];
            ax = ax == 2 ? 0 : ax + 1;
        }
        const long long j = b << 2;
        if (vec && j + 4 <= n_elem) {
            if (r) {
                *(double2*)(r + j) = make_double2(d[0], d[1]);
                *(double2*)(r + j + 2) = make_double2(d[2], d[3]);
            }
            *(double2*)(xc + j) = make_double2(x[0], x[1]);
            *(double2*)(xc + j + 2) = make_double2(x[2], x[3]);
            *(float4*)(xq + j) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j + k < n_elem) {
                    if (r) r[j + k] = d[k];
                    xc[j + k] = x[k];
                    xq[j + k] = f[k];
                }
        }
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_refine_cloud(unsigned long long key0, unsigned long long key1, unsigned long long source,
                                                            long long n_elem, RcAxes a, double* __restrict__ r, double* __restrict__ xc,
                                                            float* __restrict__ xq) {
    rc_cloud(key0, key1, source, n_elem, a.sx, a.sy, a.sz, a, r, xc, xq, true);
}

// The clouds of the sources source0 .. source0 + gridDim.y - 1 in one launch (the refine pass with `source_batch` > 1): blockIdx.y = b draws
// source0 + b around src[b] (a DEVICE array [n_batch, 3]: the ranges and minima are the batch's and stay in the arguments) into row block b
// of xc / xq [n_batch, n_elem]. A row block starts n_elem elements after the one before, which is 16-byte aligned for every b only when
// n_elem is a multiple of 4 (`vec`, said by the host); the values do not depend on it. Row block b = k_refine_cloud of source0 + b.
__global__ __launch_bounds__(RC_BLOCK) void k_refine_cloud_b(unsigned long long key0, unsigned long long key1, unsigned long long source0,
                                                              long long n_elem, const double* __restrict__ src, RcAxes a,
                                                              double* __restrict__ xc, float* __restrict__ xq, int vec) {
    const long long b = blockIdx.y;
    rc_cloud(key0, key1, source0 + (unsigned long long)b, n_elem, src[3 * b + 0], src[3 * b + 1], src[3 * b + 2], a, nullptr, xc + b * n_elem,
             xq + b * n_elem, vec != 0);
}
