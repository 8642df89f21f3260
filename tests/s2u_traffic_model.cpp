// Host model of the L2 fills of k_stage2_h2u (tools/s2u_traffic.py drives it; tests/test_s2u_traffic.py builds it with the address
// and undefined-behaviour sanitizers). Plain C++, no HIP.
//
// The real plan of genie_amd/csrc/s2u_plan.hpp is swept in the kernel's item order (item = (group of L blocks, station tile),
// group-major, tile-minor, backwards; workgroup lb of an XCD takes items lb, lb + nbx, ...). All nbx workgroups of an XCD are
// resident and advance in lockstep, one block-tile per round (--jitter P: a workgroup skips a round with probability P). Every
// block-tile issues the 128-byte-line requests of the kernel's loads:
//   wv    staged rows ids[e], e < nst: 4 planes x 256 B of the tile's 16 stations (node-planar [g][4][S] x 16 B)
//   c     8 slots (empty slots of a short block read node 0, as the kernel does): 8 planes x 256 B ([g][8][S] x 16 B)
//   frag  8 slots: 2 planes x 256 B ([g][2][S] x 16 B)
//   mask  8 slots: 64 B ([g][S] x 4 B)
//   wu    8 slots x 16 stations x 8 station neighbours: 64-B rows ([g][S] x 64 B)
// through one LRU cache per XCD (--l2-mib, 4 by default). A miss is a fill of one line, counted per buffer and per cause:
//   first    no XCD has fetched the line before
//   refetch  this XCD has fetched it before and lost it
//   cross    another XCD has fetched it, this one has not
//
//   s2u_traffic_model TAB N_POS N_NODES STA S [--L n] [--bpc n] [--cus n] [--l2-mib x] [--order group|tile] [--jitter p] [--stream-kib k]
// --stream-kib k: c, frag and mask pass through a cache of k KiB of their own and leave the L2 to the rows (the most that streaming
// loads could do).
// TAB: int32 [N_POS][16] neighbour table of the processing order; STA: int32 [S][8] station neighbours in processing order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <unordered_map>
#include <vector>

#include "../genie_amd/csrc/s2u_plan.hpp"

using s2u_plan::Block;
using s2u_plan::NB;
using s2u_plan::NXCD;
using s2u_plan::Plan;

enum Buf { B_C = 0, B_WU, B_WV, B_FRAG, B_MASK, N_BUF };
static const char* const BUF_NAME[N_BUF] = {"c", "wu", "wv", "frag", "mask"};
enum Cause { FIRST = 0, REFETCH, CROSS, N_CAUSE };

// LRU set of 128-byte lines: last use per resident line, and the uses in time order (stale entries are skipped when evicting)
struct Lru {
    size_t cap = 0;
    uint64_t clock = 0;
    std::unordered_map<uint64_t, uint64_t> last;
    std::deque<std::pair<uint64_t, uint64_t>> uses;      // (clock, line)
    bool touch(uint64_t line) {                          // true: hit
        ++clock;
        auto it = last.find(line);
        const bool hit = it != last.end();
        if (hit) it->second = clock;
        else last.emplace(line, clock);
        uses.emplace_back(clock, line);
        while (last.size() > cap) {
            const auto u = uses.front();
            uses.pop_front();
            auto v = last.find(u.second);
            if (v != last.end() && v->second == u.first) last.erase(v);
        }
        while (uses.size() > 4 * cap + 64) {             // keep the queue bounded: drop stale heads
            const auto u = uses.front();
            auto v = last.find(u.second);
            if (v != last.end() && v->second == u.first) break;
            uses.pop_front();
        }
        return hit;
    }
};

struct Model {
    int S = 0, T = 0, L = 1;
    std::vector<int32_t> sta;                            // [S][8]
    Lru l2[NXCD], side[NXCD];                            // side: where the read-once streams go with --stream-kib (0: into l2)
    bool bypass = false;
    std::unordered_map<uint64_t, uint32_t> seen;         // line -> bit x set: XCD x has fetched it
    long long fills[N_BUF][N_CAUSE] = {}, requests[N_BUF] = {};

    void line(int x, Buf b, uint64_t ln) {
        ++requests[b];
        const uint64_t key = ((uint64_t)b << 56) | ln;
        const bool stream = b == B_C || b == B_FRAG || b == B_MASK;
        if ((bypass && stream ? side[x] : l2[x]).touch(key)) return;
        uint32_t& m = seen[key];
        const Cause c = m == 0 ? FIRST : (m >> x & 1u) ? REFETCH : CROSS;
        m |= 1u << x;
        ++fills[b][c];
    }
    void bytes(int x, Buf b, uint64_t addr, uint64_t n) {      // one request per 128-byte line the range touches
        for (uint64_t ln = addr / 128; ln <= (addr + n - 1) / 128; ++ln) line(x, b, ln);
    }
    void block_tile(int x, const Block& b, int tb) {
        const uint64_t uS = (uint64_t)S;
        const int s0 = tb * 16, ns = S - s0 < 16 ? S - s0 : 16;      // lanes past the last station re-read station S - 1
        for (int e = 0; e < b.nst; ++e)
            for (int q = 0; q < 4; ++q) bytes(x, B_WV, ((uint64_t)b.ids[e] * 4 + q) * uS * 16 + (uint64_t)s0 * 16, (uint64_t)ns * 16);
        for (int i = 0; i < NB; ++i) {
            const uint64_t g = b.idx[i][0] < 0 ? 0 : (uint64_t)b.idx[i][0];
            for (int q = 0; q < 8; ++q) bytes(x, B_C, (g * 8 + q) * uS * 16 + (uint64_t)s0 * 16, (uint64_t)ns * 16);
            bytes(x, B_MASK, g * uS * 4 + (uint64_t)s0 * 4, (uint64_t)ns * 4);
            for (int q = 0; q < 2; ++q) bytes(x, B_FRAG, (g * 2 + q) * uS * 16 + (uint64_t)s0 * 16, (uint64_t)ns * 16);
            for (int j = 0; j < ns; ++j)
                for (int k = 0; k < 8; ++k) bytes(x, B_WU, (g * uS + (uint64_t)sta[(size_t)(s0 + j) * 8 + k]) * 64, 64);
        }
    }
};

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: s2u_traffic_model TAB N_POS N_NODES STA S [--L n] [--bpc n] [--cus n] [--l2-mib x] [--order group|tile] [--jitter p] [--stream-kib k]\n"); return 2; }
    const int n_pos = atoi(argv[2]), n_nodes = atoi(argv[3]), S = atoi(argv[5]);
    int L = 4, bpc = 2, cus = 256;
    double l2_mib = 4.0, jitter = 0.0, stream_kib = 0.0;
    bool tile_major = false;
    for (int i = 6; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--L") L = atoi(argv[i + 1]);
        else if (k == "--bpc") bpc = atoi(argv[i + 1]);
        else if (k == "--cus") cus = atoi(argv[i + 1]);
        else if (k == "--l2-mib") l2_mib = atof(argv[i + 1]);
        else if (k == "--jitter") jitter = atof(argv[i + 1]);
        else if (k == "--stream-kib") stream_kib = atof(argv[i + 1]);
        else if (k == "--order") tile_major = std::string(argv[i + 1]) == "tile";
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (n_pos < 1 || n_nodes < 1 || S < 1 || L < 1 || bpc < 1 || cus < 8 || l2_mib <= 0 || jitter < 0 || jitter >= 1) { fprintf(stderr, "bad argument\n"); return 2; }
    std::vector<int32_t> tab((size_t)n_pos * 16);
    Model m;
    m.S = S; m.T = (S + 15) / 16; m.L = L;
    m.sta.resize((size_t)S * 8);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(tab.data(), sizeof(int32_t), tab.size(), f) != tab.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    f = fopen(argv[4], "rb");
    if (!f || fread(m.sta.data(), sizeof(int32_t), m.sta.size(), f) != m.sta.size()) { fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    fclose(f);
    for (int32_t v : m.sta)
        if (v < 0 || v >= S) { fprintf(stderr, "station neighbour %d out of range\n", v); return 2; }
    Plan pl;
    if (!s2u_plan::build(tab.data(), n_pos, n_nodes, 0, n_pos, L, pl)) { fprintf(stderr, "plan build failed\n"); return 2; }
    const int T = m.T;
    long long groups = 0;
    for (int x = 0; x < NXCD; ++x) groups += (pl.xcd0[x + 1] - pl.xcd0[x] + L - 1) / L;
    const long long items = groups * T;
    long long grid = (long long)cus * bpc;                       // launch_stage2_h2u
    if ((items + 7) / 8 * 8 < grid) grid = (items + 7) / 8 * 8;
    grid = grid / 8 * 8;
    if (grid < 8) grid = 8;
    const int nbx = (int)(grid / NXCD);
    for (int x = 0; x < NXCD; ++x) m.l2[x].cap = (size_t)(l2_mib * 1024.0 * 1024.0 / 128.0);
    m.bypass = stream_kib > 0;
    for (int x = 0; x < NXCD; ++x) m.side[x].cap = (size_t)(stream_kib * 1024.0 / 128.0) + 1;

    // cursors of the workgroups: the kernel's item_at / step
    struct Cur { long long it; int blk, end, tb; bool live; };
    std::vector<Cur> cur((size_t)NXCD * nbx);
    auto item_at = [&](int x, long long it, Cur& c) {
        const int blk0 = pl.xcd0[x], blk1 = pl.xcd0[x + 1];
        const long long ng = (blk1 - blk0 + L - 1) / L, n_items = ng * T;
        const long long itr = n_items - 1 - it;
        const long long kb = tile_major ? itr % ng : itr / T, rem = tile_major ? itr / ng : itr % T;
        c.it = it;
        c.blk = blk0 + (int)kb * L;
        c.end = c.blk + L < blk1 ? c.blk + L : blk1;
        c.tb = (int)rem;
    };
    for (int x = 0; x < NXCD; ++x) {
        const long long n_items = (long long)((pl.xcd0[x + 1] - pl.xcd0[x] + L - 1) / L) * T;
        for (int lb = 0; lb < nbx; ++lb) {
            Cur& c = cur[(size_t)x * nbx + lb];
            c.live = lb < n_items;
            if (c.live) item_at(x, lb, c);
        }
    }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (double)(rng >> 11) / 9007199254740992.0; };
    long long block_tiles = 0, rounds = 0;
    for (bool any = true; any; ++rounds) {
        any = false;
        for (int lb = 0; lb < nbx; ++lb)
            for (int x = 0; x < NXCD; ++x) {
                Cur& c = cur[(size_t)x * nbx + lb];
                if (!c.live) continue;
                any = true;
                if (jitter > 0 && rnd() < jitter) continue;
                m.block_tile(x, pl.blocks[(size_t)c.blk], c.tb);
                ++block_tiles;
                const long long n_items = (long long)((pl.xcd0[x + 1] - pl.xcd0[x] + L - 1) / L) * T;
                if (c.blk + 1 < c.end) ++c.blk;
                else if (c.it + nbx >= n_items) c.live = false;
                else item_at(x, c.it + nbx, c);
            }
    }
    // rows of every chunk's boundary groups (first and last group of a chunk): the surface that several XCDs can share
    long long boundary_rows = 0;
    for (int x = 0; x < NXCD; ++x) {
        const int b0 = pl.xcd0[x], b1 = pl.xcd0[x + 1];
        for (int k = b0; k < b1; ++k)
            if (k < b0 + L || k >= b1 - ((b1 - b0 - 1) % L + 1)) boundary_rows += pl.blocks[(size_t)k].U;
    }
    printf("plan L %d S %d tiles %d blocks %zu groups %lld items %lld grid %lld nbx %d block_tiles %lld rounds %lld carried %.4f\n", L, S, T,
           pl.blocks.size(), groups, items, grid, nbx, block_tiles, rounds, pl.carried_fraction());
    printf("boundary_union_rows %lld of %lld\n", boundary_rows, pl.rows_union);
    long long tot[N_CAUSE] = {}, treq = 0;
    for (int b = 0; b < N_BUF; ++b) {
        printf("fills %-4s first %lld refetch %lld cross %lld requests %lld\n", BUF_NAME[b], m.fills[b][FIRST], m.fills[b][REFETCH],
               m.fills[b][CROSS], m.requests[b]);
        for (int c = 0; c < N_CAUSE; ++c) tot[c] += m.fills[b][c];
        treq += m.requests[b];
    }
    printf("fills all  first %lld refetch %lld cross %lld requests %lld\n", tot[FIRST], tot[REFETCH], tot[CROSS], treq);
    printf("fill_bytes %lld\n", (tot[FIRST] + tot[REFETCH] + tot[CROSS]) * 128);
    return 0;
}
