// Item table of k_stage1_h2 with PACKED station tail tiles: plain C++ (genie_hip.hip includes it for the device;
// tests/tile_items_check.cpp builds it alone on the host).
//
// A chunk [gbeg, gend) of the processing order (one XCD's share of a launched range, as in ItemIter) holds n source nodes with
// T = ceil(S / 16) station tiles each. When r = S mod 16 is in 1 .. 8 the last tile of a node has r live rows in a 16-lane row. Two
// such tail tiles share one MIXED item: node g keeps lanes 0 .. r-1, its partner g + 1 (the next position of the same chunk) takes
// lanes 8 .. 8+r-1. Items of a chunk, in sweep order:
//  * seg == 1 (node-major sweeps): node PAIRS, 2 T - 1 items each: tiles 0 .. T-2 of g, the mixed tile, tiles 0 .. T-2 of g + 1.
//    An odd n leaves the last node of the chunk alone with its T items, the last one padded as before.
//  * seg >= 2 (station-tile-major sweeps over segments of seg nodes): tiles 0 .. T-2 of the segment's nodes tile by tile, then one
//    mixed item per pair (2 j, 2 j + 1) of the segment; an odd segment's last node keeps its padded tail tile.
// A pair never leaves its chunk, so it never straddles a range cut of the sharded path either (chunks are cut inside a range).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TILE_ITEMS_HD __host__ __device__ __forceinline__
#else
#define TILE_ITEMS_HD inline
#endif

namespace tile_items {

// tail tiles are packed for this station count (r > 8: two tails do not fit one row; r == 0: there is no tail)
TILE_ITEMS_HD bool packs(int S) { return (S & 15) >= 1 && (S & 15) <= 8; }

// chunk x of nx of the range [gi0, gi0 + G): the cut of ItemIter and of s2u_plan
TILE_ITEMS_HD void chunk(int gi0, int G, int x, int nx, int& gbeg, int& gend) {
    gbeg = gi0 + (int)((long long)G * x / nx);
    gend = gi0 + (int)((long long)G * (x + 1) / nx);
}

// items of a chunk of n nodes
TILE_ITEMS_HD long long count(int n, int T, int seg) {
    if (seg <= 1) return (long long)(n / 2) * (2 * T - 1) + (long long)(n & 1) * T;
    const int full = n / seg, rest = n - full * seg;
    return (long long)full * ((long long)seg * (T - 1) + (seg + 1) / 2) + (long long)rest * (T - 1) + (rest + 1) / 2;
}

struct Packed {
    int gbeg, T;
    unsigned seg, per, m_per, n_full, m_full, n_last, m_last, last_seg;     // divisors and their 2^32 reciprocals
    long long nitems;
    // floor(x / d) for x < 2^31 with m = floor(2^32 / d) (ItemIter::fdiv)
    static TILE_ITEMS_HD unsigned fdiv(unsigned x, unsigned d, unsigned m, unsigned& r) {
        unsigned q = (unsigned)(((unsigned long long)x * m) >> 32);
        r = x - q * d;
        if (r >= d) { r -= d; ++q; }
        if (r >= d) { r -= d; ++q; }
        return q;
    }
    static TILE_ITEMS_HD unsigned recip(unsigned d) { return d <= 1u ? 0xffffffffu : (unsigned)(0x100000000ull / d); }
    TILE_ITEMS_HD void init(int gbeg_, int gend_, int T_, int seg_) {
        gbeg = gbeg_; T = T_;
        const int n = gend_ - gbeg_;
        seg = (unsigned)(seg_ <= 1 ? 1 : seg_);
        const unsigned span = seg == 1u ? 2u : seg;                           // nodes that one `per` block of items covers
        per = seg == 1u ? (unsigned)(2 * T - 1) : seg * (unsigned)(T - 1) + (seg + 1u) / 2u;
        m_per = recip(per);
        n_full = span; m_full = recip(n_full);
        last_seg = (unsigned)n / span;                                        // index of the (short or empty) last block
        n_last = (unsigned)n - last_seg * span;
        if (n_last == 0u) n_last = 1u;
        m_last = recip(n_last);
        nitems = count(n, T, (int)seg);
    }
    // item -> positions gi, gj of the processing order and the station tile. gj == gi: a plain item (16 stations of one node);
    // gj == gi + 1: a mixed item (tile T - 1: lanes 0 .. 7 belong to gi, lanes 8 .. 15 to gj)
    TILE_ITEMS_HD void decode(long long item, int& gi, int& gj, int& tb) const {
        unsigned rem, r2;
        const unsigned sidx = per <= 1u ? (rem = 0u, (unsigned)item) : fdiv((unsigned)item, per, m_per, rem);
        const bool last = sidx >= last_seg;
        const unsigned tm1 = (unsigned)(T - 1);
        if (seg == 1u) {
            const int base = gbeg + 2 * (int)sidx;
            const bool second = !last && rem > tm1;
            gi = base + (second ? 1 : 0);
            gj = gi + ((!last && rem == tm1) ? 1 : 0);
            tb = (int)(second ? rem - tm1 - 1u : rem);
            return;
        }
        const unsigned n = last ? n_last : n_full;
        const unsigned nt = n * tm1;
        const int base = gbeg + (int)(sidx * seg);
        if (rem < nt) {
            const unsigned q = n <= 1u ? (r2 = 0u, rem) : fdiv(rem, n, last ? m_last : m_full, r2);
            tb = (int)q;
            gi = gj = base + (int)r2;
        } else {
            const unsigned j = rem - nt;
            tb = (int)tm1;
            gi = base + 2 * (int)j;
            gj = gi + (2u * j + 1u < n ? 1 : 0);
        }
    }
};

}  // namespace tile_items
