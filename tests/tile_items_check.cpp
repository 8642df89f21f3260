// Stand-alone check of genie_amd/csrc/tile_items.hpp (host only; tests/test_tile_items.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the item table of k_stage1_h2 with packed station tail tiles.
//
// For station counts with r = S mod 16 in {0, 1 .. 8, 9 .. 15}, node-major (seg 1) and tile-major (seg 2, 3, 16) sweeps, whole grids
// and ranges cut in two at every kind of position (next to a pair, inside one, at a chunk of one node, empty ranges):
//  * every (position, station) of the range is covered exactly once, by the lanes the kernel gives it;
//  * a mixed item pairs positions g, g + 1 of the same chunk, on the last tile, and only when packs(S);
//  * the item count is count(), which is the padded count minus one item per pair.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../genie_amd/csrc/tile_items.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                                                                             \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (++g_fail <= 20) { fprintf(stderr, "FAIL S %d G %d gi0 %d seg %d: ", S, G, gi0, seg); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
            return;                                                                                                  \
        }                                                                                                            \
    } while (0)

static long long g_items = 0, g_mixed = 0;

// one launched range [gi0, gi0 + G) of a grid of n_pos positions
static void check_range(int S, int n_pos, int gi0, int G, int seg) {
    const int T = (S + 15) / 16, r = S & 15, NX = 8;
    std::vector<uint8_t> cover((size_t)n_pos * S, 0);
    long long total = 0, padded = 0, pairs = 0;
    for (int x = 0; x < NX; ++x) {
        int gb, ge;
        tile_items::chunk(gi0, G, x, NX, gb, ge);
        CHECK(gb >= gi0 && ge <= gi0 + G && gb <= ge, "chunk %d = [%d, %d)", x, gb, ge);
        tile_items::Packed w;
        w.init(gb, ge, T, seg);
        CHECK(w.nitems == tile_items::count(ge - gb, T, seg), "chunk %d: nitems", x);
        padded += (long long)(ge - gb) * T;
        total += w.nitems;
        for (long long it = 0; it < w.nitems; ++it) {
            int gi, gj, tb;
            w.decode(it, gi, gj, tb);
            CHECK(gi >= gb && gi < ge && gj >= gb && gj < ge, "item %lld of chunk %d [%d, %d): positions %d, %d", it, x, gb, ge, gi, gj);
            CHECK(tb >= 0 && tb < T, "item %lld: tile %d", it, tb);
            CHECK(gj == gi || gj == gi + 1, "item %lld: partner %d of %d", it, gj, gi);
            const bool mixed = gj != gi;
            if (mixed) {
                CHECK(tb == T - 1, "item %lld: mixed on tile %d", it, tb);
                CHECK(r >= 1 && r <= 8, "item %lld: mixed with r = %d", it, r);
                ++pairs;
            }
            for (int lane = 0; lane < 16; ++lane) {      // the kernel's lanes: station tb * 16 + (mixed ? lane & 7 : lane) of gi / gj
                const int s = tb * 16 + (mixed ? (lane & 7) : lane);
                if (s >= S) continue;
                const int g = lane >= 8 ? gj : gi;
                uint8_t& c = cover[(size_t)g * S + s];
                CHECK(c == 0, "item %lld: (%d, station %d) covered twice", it, g, s);
                c = 1;
            }
        }
    }
    for (int g = 0; g < n_pos; ++g)
        for (int s = 0; s < S; ++s)
            CHECK(cover[(size_t)g * S + s] == ((g >= gi0 && g < gi0 + G) ? 1 : 0), "(%d, station %d) covered %d times", g, s, cover[(size_t)g * S + s]);
    CHECK(total == padded - pairs, "items %lld, padded %lld, pairs %lld", total, padded, pairs);
    g_items += total; g_mixed += pairs;
}

int main() {
    const int stations[] = {1, 3, 8, 9, 13, 16, 17, 19, 24, 29, 32, 40, 200};
    const int grids[] = {1, 2, 7, 8, 9, 33, 40, 250};
    const int segs[] = {1, 2, 3, 16};
    for (int S : stations)
        for (int G : grids)
            for (int seg : segs) {
                if (tile_items::packs(S) != ((S & 15) >= 1 && (S & 15) <= 8)) { fprintf(stderr, "packs(%d) is wrong\n", S); return 1; }
                if (!tile_items::packs(S)) continue;      // the kernel keeps ItemIter's padded table for these S
                check_range(S, G, 0, G, seg);
                // the sharded path's range launches: every cut of the grid in two (next to a pair, inside one, empty ranges)
                for (int cut = 0; cut <= G; cut += (G > 40 ? 37 : 1)) {
                    check_range(S, G, 0, cut, seg);
                    check_range(S, G, cut, G - cut, seg);
                }
            }
    for (int S : {16, 32, 29, 13, 2000})
        if (tile_items::packs(S)) { fprintf(stderr, "packs(%d) is true\n", S); return 1; }
    // one-node chunks: G <= 8 gives chunks of 0 or 1 nodes, nothing to pair
    {
        long long before = g_mixed;
        check_range(19, 8, 0, 8, 1);
        if (g_mixed != before) { fprintf(stderr, "one-node chunks were paired\n"); return 1; }
    }
    // config 2 (200 stations, 10 000 nodes, node-major): 13 -> 12.5 items per node
    {
        long long n = 0;
        for (int x = 0; x < 8; ++x) { int gb, ge; tile_items::chunk(0, 10000, x, 8, gb, ge); n += tile_items::count(ge - gb, 13, 1); }
        printf("S = 200, G = 10000: %lld items (padded %d)\n", n, 130000);
        if (n != 125000) { fprintf(stderr, "config 2: %lld items\n", n); return 1; }
    }
    printf("checked %lld items, %lld mixed\n", g_items, g_mixed);
    if (g_fail) { fprintf(stderr, "tile_items_check: %d failures\n", g_fail); return 1; }
    printf("tile_items_check: ok\n");
    return 0;
}
