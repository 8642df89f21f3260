// ------------------------------------------------------------------------------------------------
// Exact kNN of large query sets through a cell index of the context points (genie_knn_index_plan /
// genie_knn_index_build / genie_knn_indexed). The refine pass draws a NEW cloud of 112 000 queries per candidate source
// (process_continuous_days.py:929) inside a box of X_offset_range around it, and every cloud paid a brute-force sweep of the whole
// grid (k_knn_t: 112 000 x 10 000 pair distances). The grid is fixed at set_adjacencies: a uniform cell grid over its bounding box,
// built once per grid, leaves a query a few hundred candidates. The search is EXACT: the table of genie_knn, bit for bit, ties
// included (neighbours in (distance, index) order), because every accept is decided as k_knn_t decides it and a search stops only
// when no point it has not seen can enter the list (the argument stands above k_knn_ix).
//
// The index: cell (c0, c1, c2) of a point = kix_cell of each coordinate, cell id = (c2 * n1 + c1) * n0 + c0 (axis 0 runs fastest: a
// row of cells along axis 0 is one contiguous run of records); cell_start[n_cells + 1] int32 and the points reordered by cell as
// 16-byte records (x, y, z, bits of the original index): a candidate costs one load.
// ------------------------------------------------------------------------------------------------
struct KixGrid {
    float o[3];        // the bounding box's lower corner = the cell grid's origin
    float hi[3];       // its upper corner (every context point p has o[a] <= p[a] <= hi[a], exactly: they are the min / max of the floats)
    float inv;         // 1 / cell edge, fp32: what kix_cell multiplies by
    int n[3];          // cells per axis (1 on an axis of zero extent)
    int nc;            // records of the index (= context points): no run read from cell_start reaches past it
    double h;          // 1 / (double)inv: the cell edge the face bounds are made from
};

// The cell function, fp32: floor(fl(fl(x - o) * inv)) clamped to [0, n - 1]. Two explicitly rounded operations (nothing for the compiler
// to contract or reorder), each monotone non-decreasing in x, as are floor and the clamps: a larger coordinate never gets a smaller
// cell. Clamped in fp32 first, so that a query far outside the box cannot overflow the conversion.
__device__ __forceinline__ int kix_cell(float x, float o, float inv, int n) {
    float t = floorf(__fmul_rn(__fsub_rn(x, o), inv));
    t = fminf(fmaxf(t, 0.f), (float)(n - 1));
    return min(max((int)t, 0), n - 1);
}

__device__ __forceinline__ int kix_cell_id(const KixGrid& g, float x, float y, float z) {
    return (kix_cell(z, g.o[2], g.inv, g.n[2]) * g.n[1] + kix_cell(y, g.o[1], g.inv, g.n[1])) * g.n[0] + kix_cell(x, g.o[0], g.inv, g.n[0]);
}

// Bounding box of the context points: bbox[0..2] = min, bbox[3..5] = max. One workgroup (a build happens once per grid). A coordinate
// with an all-ones exponent (NaN or infinity) makes the box infinite, which the host refuses. The library is built with
// -fno-honor-nans: the test is made on words LOADED as integers, which the compiler cannot fold into a float compare.
__global__ __launch_bounds__(1024) void k_kix_bbox(const float* __restrict__ x, int n, float* __restrict__ bbox) {
    __shared__ float red[6][16];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool bad = false;
    const uint32_t* xw = (const uint32_t*)x;
    for (int i = threadIdx.x; i < n; i += 1024) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t w = xw[(long long)i * 3 + a];
            const float v = __uint_as_float(w);
            bad |= (w & 0x7f800000u) == 0x7f800000u;
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    }
    if (bad) { lo[0] = -__builtin_inff(); hi[0] = __builtin_inff(); }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], s)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], s)); }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[threadIdx.x][0];
        for (int w = 1; w < 16; ++w) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
        bbox[threadIdx.x] = v;
    }
}

// Histogram of the cell ids (count[] zeroed by the caller).
__global__ __launch_bounds__(256) void k_kix_count(const float* __restrict__ x, int n, KixGrid g, int32_t* __restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = x + (long long)i * 3;
    atomicAdd(&count[kix_cell_id(g, p[0], p[1], p[2])], 1);
}

// Exclusive scan of count[n_cells] into cell_start[n_cells + 1], one workgroup: a thread sums a contiguous chunk, the chunk sums are
// scanned through LDS, the thread writes its chunk. count[] is left zeroed: the scatter uses it as the cells' cursors.
__global__ __launch_bounds__(1024) void k_kix_scan(int32_t* __restrict__ count, int n_cells, int32_t* __restrict__ cell_start) {
    __shared__ int part[1024];
    const int chunk = (n_cells + 1023) / 1024;
    const int b = min(threadIdx.x * chunk, n_cells), e = min(b + chunk, n_cells);
    int s = 0;
    for (int i = b; i < e; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                 // inclusive scan of the 1024 chunk sums
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = b; i < e; ++i) { const int c = count[i]; cell_start[i] = run; run += c; count[i] = 0; }
    if (threadIdx.x == 1023) cell_start[n_cells] = part[1023];
}

// The points into their cells' runs. The order inside a cell is the order of the atomics, which the search does not depend on: every
// accept is the full (distance, index) test.
__global__ __launch_bounds__(256) void k_kix_scatter(const float* __restrict__ x, int n, KixGrid g, const int32_t* __restrict__ cell_start,
                                                     int32_t* __restrict__ cursor, f32x4* __restrict__ rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = x + (long long)i * 3;
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    const int c = kix_cell_id(g, p0, p1, p2);
    const int at = cell_start[c] + atomicAdd(&cursor[c], 1);
    if (at < n) rec[at] = f32x4{p0, p1, p2, __int_as_float(i)};
}

// The search, ONE LANE per query with a KnnWorst list as in k_knn_t (the query sets this serves are large; knn_kernels.hpp has the
// distance, the order, the list and its fp32 pre-filter). A query starts in its own cell -- its cell coordinate clamped, clouds do reach
// outside the grid's box -- and visits shells of growing Chebyshev radius r in cell coordinates: after shell r it has seen every point
// whose cell lies in the box [cq - r, cq + r] (cut to the grid) on all three axes. Two things are this kernel's own.
//
// (1) Candidates do not arrive in increasing index order, so every accept is the full test: offer<false>.
//
// (2) Termination. After shell r the search stops when the list is full() and its worst exact squared distance wd is
//     STRICTLY smaller than B, a lower bound of the kernel's own squared distance to every point outside the visited box (strictly: a
//     point at exactly wd with a smaller index would belong in the table) -- or when the visited box is the whole grid.
//     A point p outside the box lies beyond one of its faces on some axis a: cell(p_a) >= j = hi_a + 1, or cell(p_a) <= lo_a - 1.
//     A face of the box that is a face of the grid has no point beyond it and gives no bound. For the others, with u = 2^-24 (fp32
//     rounding, t(x) = fl(fl(x - o) * inv) = (x - o) * inv * (1 + e1)(1 + e2), |e| <= u; p - o >= 0 for every context point):
//       upper face: j <= n - 1, so the clamp does not matter and t(p_a) >= j >= 1, hence p_a - o >= (j / inv) / (1 + u)^2
//                   > j * h * (1 - 2^-22)                                                 [ (1 + u)^-2 > 1 - 2^-23 ]
//       lower face: floor(t(p_a)) <= lo_a - 1, t(p_a) < lo_a, hence p_a - o < (lo_a / inv) / (1 - u)^2 < lo_a * h * (1 + 2^-22)
//     (the plan keeps the cell edge within [1e-30, 2^126], so inv is a normal fp32 number, and the box's edges below 1e38, so x - o
//     is finite: neither product leaves the range where the relative error holds). The slack 2^-22 is twice the rounding of the cell function; the fp64 roundings of h = 1 / (double)inv, of the
//     products, of q - o and of the difference (2^-53 each, relative to a term no larger than face + |q - o|) are covered by
//     subtracting (face + |q - o|) * 2^-40 once more. So g_a <= |p_a - q_a| in real numbers, and because rounding is monotone also
//     g_a <= |fl(q_a - p_a)|, the kernel's d_a. On the other axes b the point is at least E_b = the distance of q_b to the grid's
//     box [o_b, hi_b] away (exact min / max of the floats, again monotone under fl). B is then knn_dist2's own statement on these
//     lower bounds, knn_sum3 of their rounded squares in axis order: every operation is monotone in non-negative
//     arguments, so B <= d(p), and wd < B <= d(p) keeps p out whatever its index. B is the minimum over the (at most six) faces.
//     A loose bound costs one more shell now and then; nothing here is tight.
template <int K>
__global__ __launch_bounds__(256) void k_knn_ix(const int32_t* __restrict__ cell_start, const f32x4* __restrict__ rec, KixGrid g,
                                                const float* __restrict__ xq, int nq, int k, int exclude_self, int32_t* __restrict__ out) {
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    const float f[3] = {xq[(long long)qi * 3 + 0], xq[(long long)qi * 3 + 1], xq[(long long)qi * 3 + 2]};
    const double q0 = (double)f[0], q1 = (double)f[1], q2 = (double)f[2];
    KnnWorst<K> best;
    best.clear();
    int cq[3];
    double qo[3], E2[3];                             // q - o per axis; squared distance of q to the grid's box per axis
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cq[a] = kix_cell(f[a], g.o[a], g.inv, g.n[a]);
        qo[a] = (double)f[a] - (double)g.o[a];
        const double below = (double)g.o[a] - (double)f[a], above = (double)f[a] - (double)g.hi[a];
        const double e = fmax(fmax(below, above), 0.0);
        E2[a] = __dmul_rn(e, e);
    }
    const int rmax = max(g.n[0], max(g.n[1], g.n[2]));
    for (int r = 0; r < rmax; ++r) {
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = max(cq[a] - r, 0); hi[a] = min(cq[a] + r, g.n[a] - 1); }
        // shell r: the cells of the box at Chebyshev distance exactly r from cq. A row (c1, c2) that lies on the shell in axis 1 or 2
        // is taken whole -- one contiguous run of records --, any other row contributes its two end cells cq[0] - r and cq[0] + r.
        // One scan site for every run, so that lanes in different rows stay together in it.
        for (int c2 = lo[2]; c2 <= hi[2]; ++c2) {
            const bool s2 = c2 == cq[2] - r || c2 == cq[2] + r;
            for (int c1 = lo[1]; c1 <= hi[1]; ++c1) {
                const int row = (c2 * g.n[1] + c1) * g.n[0];
                const bool full = s2 || c1 == cq[1] - r || c1 == cq[1] + r;
                for (int seg = 0; seg < (full ? 1 : 2); ++seg) {
                    const int a0 = full ? lo[0] : seg == 0 ? cq[0] - r : cq[0] + r, a1 = full ? hi[0] : a0;
                    if (a0 < 0 || a1 >= g.n[0]) continue;              // (an end cell outside the grid)
                    const int e = min(cell_start[row + a1 + 1], g.nc);
#pragma unroll 1
                    for (int i = max(cell_start[row + a0], 0); i < e; ++i) {
                        const f32x4 cv = rec[i];
                        const float e0 = f[0] - cv.x, e1 = f[1] - cv.y, e2 = f[2] - cv.z;
                        if (!best.passes(e0 * e0 + e1 * e1 + e2 * e2)) continue;
                        const int c = __float_as_int(cv.w);
                        if (exclude_self && c == qi) continue;
                        best.template offer<false>(knn_dist2(q0, q1, q2, cv.x, cv.y, cv.z), c);
                    }
                }
            }
        }
        // (2): stop?
        bool whole = true;
        double B = __builtin_inf();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            auto face = [&](double gap) {                // the distance statement on the lower bounds: gap on axis a, E on the others
                gap = fmax(gap, 0.0);
                const double gg = __dmul_rn(gap, gap);
                B = fmin(B, knn_sum3(a == 0 ? gg : E2[0], a == 1 ? gg : E2[1], a == 2 ? gg : E2[2]));
            };
            if (hi[a] < g.n[a] - 1) {
                whole = false;
                const double fc = (double)(hi[a] + 1) * g.h;
                face(fc * (1.0 - 0x1p-22) - qo[a] - (fc + fabs(qo[a])) * 0x1p-40);
            }
            if (lo[a] > 0) {
                whole = false;
                const double fc = (double)lo[a] * g.h;
                face(qo[a] - fc * (1.0 + 0x1p-22) - (fc + fabs(qo[a])) * 0x1p-40);
            }
        }
        if (whole) break;
        if (best.full() && best.worst_d() < B) break;
    }
    best.write_ranked(out + (long long)qi * k, k);
}
