// Stand-alone check of genie_amd/csrc/s2u_plan.hpp (host only; tests/test_s2u_plan.py builds it with the address and
// undefined-behaviour sanitizers and runs it).
//
//   s2u_plan_check                 random 3-D grids with 15-nearest-neighbour graphs: every plan is replayed with an array standing in
//                                  for the LDS slots
//   s2u_plan_check TAB G L...      carried fraction of the plans of a neighbour table dumped as int32 [G][16] (whole range)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../genie_amd/csrc/s2u_plan.hpp"

using s2u_plan::Block;
using s2u_plan::KP;
using s2u_plan::NB;
using s2u_plan::NXCD;
using s2u_plan::Plan;
using s2u_plan::UCAP;

static int g_fail = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++g_fail <= 20) { fprintf(stderr, "FAIL %s: ", what); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
            return;                                                        \
        }                                                                  \
    } while (0)

// the block table as it was built before the plan header existed (union row u in LDS row u, everything staged per block)
struct OldBlock { int32_t gi0, n, U, pad; int32_t ids[64]; int32_t idx[NB][16]; };
static void build_old(const std::vector<int32_t>& tab, int n_nodes, int gb0, int ge0, std::vector<OldBlock>& blks, int32_t* x0) {
    std::vector<int32_t> seen_blk((size_t)n_nodes, -1), seen_at((size_t)n_nodes, 0);
    int32_t serial = 0;
    const int nxc = 8, n = ge0 - gb0;
    for (int x = 0; x < nxc; ++x) {
        x0[x] = (int32_t)blks.size();
        const int gb = gb0 + (int)((long long)n * x / nxc), ge = gb0 + (int)((long long)n * (x + 1) / nxc);
        int pos = gb;
        while (pos < ge) {
            OldBlock b;
            memset(&b, 0, sizeof(b));
            b.gi0 = pos;
            ++serial;
            int32_t uni[64 + 15];
            int nuni = 0;
            while (pos < ge && b.n < 8) {
                int32_t where[15];
                const int before = nuni;
                for (int k = 0; k < 15; ++k) {
                    const int32_t nb = tab[(size_t)pos * 16 + 1 + k];
                    if (seen_blk[(size_t)nb] != serial) { seen_blk[(size_t)nb] = serial; seen_at[(size_t)nb] = nuni; uni[nuni++] = nb; }
                    where[k] = seen_at[(size_t)nb];
                }
                if (b.n > 0 && nuni > 64) {
                    for (int u = before; u < nuni; ++u) seen_blk[(size_t)uni[u]] = -1;
                    nuni = before;
                    break;
                }
                b.idx[b.n][0] = tab[(size_t)pos * 16];
                for (int k = 0; k < 15; ++k) b.idx[b.n][1 + k] = where[k];
                ++b.n; ++pos;
            }
            for (int e = b.n; e < 8; ++e) b.idx[e][0] = -1;
            b.U = (int32_t)nuni;
            for (int u = 0; u < 64; ++u) b.ids[u] = uni[u < nuni ? u : 0];
            blks.push_back(b);
        }
    }
    x0[nxc] = (int32_t)blks.size();
}

// [G][16] neighbour table of G random points of a box (the third axis `flat` times shorter), in Z-curve order or, `shuffled`, in a
// random order (adjacent positions then share no neighbours and the 64-row cap cuts the blocks short)
static std::vector<int32_t> random_table(int G, unsigned seed, bool shuffled, double flat) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> un(0.0, 1.0);
    std::vector<double> p((size_t)G * 3);
    for (int i = 0; i < G; ++i) { p[3 * i] = un(rng); p[3 * i + 1] = un(rng); p[3 * i + 2] = un(rng) / flat; }
    std::vector<int32_t> order(G);
    for (int i = 0; i < G; ++i) order[i] = i;
    if (shuffled) std::shuffle(order.begin(), order.end(), rng);
    else {
        std::vector<uint32_t> code(G);
        for (int i = 0; i < G; ++i) {
            uint32_t c = 0;
            for (int ax = 0; ax < 3; ++ax) {
                const uint32_t q = (uint32_t)std::min(1023.0, p[3 * i + ax] * 1023.0);
                for (int bit = 0; bit < 10; ++bit) c |= ((q >> bit) & 1u) << (3 * bit + ax);
            }
            code[i] = c;
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return code[a] < code[b]; });
    }
    std::vector<int32_t> tab((size_t)G * 16);
    std::vector<std::pair<double, int>> d(G);
    for (int gi = 0; gi < G; ++gi) {
        const int g = order[gi];
        for (int j = 0; j < G; ++j) {
            double s = 0;
            for (int ax = 0; ax < 3; ++ax) { const double t = p[3 * g + ax] - p[3 * j + ax]; s += t * t; }
            d[j] = {j == g ? 1e30 : s, j};
        }
        const int k = std::min(KP, G - 1);
        std::partial_sort(d.begin(), d.begin() + k, d.end());
        tab[(size_t)gi * 16] = g;
        for (int q = 0; q < KP; ++q) tab[(size_t)gi * 16 + 1 + q] = d[q % k].second;
    }
    return tab;
}

// every block of the plan against the table and against a model of the LDS slots
static void replay(const char* what, const std::vector<int32_t>& tab, int G, int gb0, int ge0, int L, const Plan& pl) {
    CHECK(pl.L == L, "L %d", pl.L);
    CHECK(pl.xcd0[0] == 0 && pl.xcd0[NXCD] == (int32_t)pl.blocks.size(), "xcd0 ends");
    const int n = ge0 - gb0;
    long long uni_rows = 0, carried = 0;
    for (int x = 0; x < NXCD; ++x) {
        const int gb = gb0 + (int)((long long)n * x / NXCD), ge = gb0 + (int)((long long)n * (x + 1) / NXCD);
        CHECK(pl.xcd0[x] <= pl.xcd0[x + 1], "xcd0 order");
        int pos = gb;
        int32_t lds[UCAP];
        for (int k = pl.xcd0[x]; k < pl.xcd0[x + 1]; ++k) {
            const Block& b = pl.blocks[(size_t)k];
            const bool first = (k - pl.xcd0[x]) % L == 0;
            if (first)
                for (int s = 0; s < UCAP; ++s) lds[s] = -1;           // another workgroup's LDS: nothing is known about it
            CHECK(b.gi0 == pos, "block %d starts at %d, expected %d", k, b.gi0, pos);
            CHECK(b.n >= 1 && b.n <= NB && pos + b.n <= ge, "block %d: n %d", k, b.n);
            CHECK(b.U >= 1 && b.U <= UCAP && b.nst >= 0 && b.nst <= b.U && b.nst <= 64, "block %d: U %d nst %d", k, b.U, b.nst);
            if (first) CHECK(b.nst == b.U, "block %d opens a group and stages %d of %d", k, b.nst, b.U);
            // the rows this block reads
            std::vector<int32_t> need;
            for (int i = 0; i < b.n; ++i)
                for (int q = 0; q < KP; ++q) need.push_back(tab[(size_t)(pos + i) * 16 + 1 + q]);
            std::sort(need.begin(), need.end());
            need.erase(std::unique(need.begin(), need.end()), need.end());
            CHECK((int)need.size() == b.U, "block %d: U %d, distinct rows %d", k, b.U, (int)need.size());
            bool written[UCAP] = {};
            for (int e = 0; e < b.nst; ++e) {
                const int s = b.slot[e];
                CHECK(s < UCAP && !written[s], "block %d: slot %d staged twice", k, s);
                CHECK(b.ids[e] >= 0 && b.ids[e] < G, "block %d: staged node %d", k, b.ids[e]);
                CHECK(!std::binary_search(need.begin(), need.end(), lds[s]), "block %d: slot %d held row %d, which the block reads", k, s, lds[s]);
                CHECK(std::binary_search(need.begin(), need.end(), b.ids[e]), "block %d: stages row %d, which it does not read", k, b.ids[e]);
                written[s] = true;
            }
            for (int e = 0; e < b.nst; ++e) lds[b.slot[e]] = b.ids[e];
            for (int e = b.nst; e < 64; ++e) CHECK(b.ids[e] >= 0 && b.ids[e] < G, "block %d: padding id %d", k, b.ids[e]);
            for (int i = 0; i < NB; ++i) {
                if (i >= b.n) { CHECK(b.idx[i][0] == -1, "block %d: empty node slot %d", k, i); continue; }
                CHECK(b.idx[i][0] == tab[(size_t)(pos + i) * 16], "block %d node %d: id", k, i);
                for (int q = 0; q < KP; ++q) {
                    const int s = b.idx[i][1 + q];
                    CHECK(s >= 0 && s < UCAP, "block %d node %d: slot %d", k, i, s);
                    CHECK(lds[s] == tab[(size_t)(pos + i) * 16 + 1 + q], "block %d node %d neighbour %d: slot %d holds %d, not %d", k, i, q, s,
                          lds[s], tab[(size_t)(pos + i) * 16 + 1 + q]);
                }
            }
            uni_rows += b.U; carried += b.U - b.nst;
            pos += b.n;
        }
        CHECK(pos == ge, "chunk %d ends at %d, expected %d", x, pos, ge);
    }
    CHECK(uni_rows == pl.rows_union && carried == pl.rows_carried, "row counts");
}

static void same_as_old(const char* what, const std::vector<int32_t>& tab, int G, int gb0, int ge0, const Plan& pl) {
    std::vector<OldBlock> old;
    int32_t x0[9];
    build_old(tab, G, gb0, ge0, old, x0);
    CHECK(old.size() == pl.blocks.size(), "L = 1: %zu blocks, %zu before", pl.blocks.size(), old.size());
    for (int x = 0; x <= NXCD; ++x) CHECK(x0[x] == pl.xcd0[x], "L = 1: xcd0[%d]", x);
    for (size_t k = 0; k < old.size(); ++k) {
        const OldBlock& o = old[k];
        const Block& b = pl.blocks[k];
        CHECK(o.gi0 == b.gi0 && o.n == b.n && o.U == b.U && b.nst == b.U, "L = 1: header of block %zu", k);
        CHECK(!memcmp(o.ids, b.ids, sizeof(o.ids)) && !memcmp(o.idx, b.idx, sizeof(o.idx)), "L = 1: lists of block %zu", k);
        for (int e = 0; e < b.nst; ++e) CHECK(b.slot[e] == e, "L = 1: block %zu stages row %d into slot %d", k, e, b.slot[e]);
    }
    CHECK(pl.rows_carried == 0, "L = 1 carries rows");
}

static void one_case(const char* what, int G, unsigned seed, bool shuffled, int gb0, int ge0, bool expect_cut) {
    const std::vector<int32_t> tab = random_table(G, seed, shuffled, 4.0);
    if (ge0 < 0) ge0 = G;
    const int Ls[4] = {1, 2, 4, 8};
    double fprev = -1.0;
    for (int L : Ls) {
        Plan pl;
        if (!s2u_plan::build(tab.data(), G, G, gb0, ge0, L, pl)) { fprintf(stderr, "FAIL %s: build L = %d\n", what, L); ++g_fail; continue; }
        replay(what, tab, G, gb0, ge0, L, pl);
        if (L == 1) same_as_old(what, tab, G, gb0, ge0, pl);
        bool cut = false;
        for (int x = 0; x < NXCD; ++x)
            for (int k = pl.xcd0[x]; k + 1 < pl.xcd0[x + 1]; ++k) cut |= pl.blocks[(size_t)k].n < NB;
        if (expect_cut && !cut) { fprintf(stderr, "FAIL %s: no block was cut short\n", what); ++g_fail; }
        printf("%-28s G %4d [%d, %d) L %d: %4zu blocks, carried fraction %.3f%s\n", what, G, gb0, ge0, L, pl.blocks.size(),
               pl.carried_fraction(), cut ? ", blocks cut short" : "");
        if (pl.carried_fraction() + 1e-12 < fprev) { fprintf(stderr, "FAIL %s: a longer group carries less\n", what); ++g_fail; }
        fprev = pl.carried_fraction();
    }
}

int main(int argc, char** argv) {
    if (argc >= 4) {
        const int G = atoi(argv[2]);
        std::vector<int32_t> tab((size_t)G * 16);
        FILE* f = fopen(argv[1], "rb");
        if (!f || fread(tab.data(), sizeof(int32_t), tab.size(), f) != tab.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        fclose(f);
        for (int i = 3; i < argc; ++i) {
            const int L = atoi(argv[i]);
            Plan pl;
            if (!s2u_plan::build(tab.data(), G, G, 0, G, L, pl)) { fprintf(stderr, "build failed\n"); return 2; }
            replay("table", tab, G, 0, G, L, pl);
            size_t groups = 0;
            for (int x = 0; x < NXCD; ++x) groups += (size_t)(pl.xcd0[x + 1] - pl.xcd0[x] + L - 1) / L;
            printf("L %d: %zu blocks, %zu groups, union rows %lld (%.1f per block), carried %lld, f = %.4f\n", L, pl.blocks.size(), groups,
                   pl.rows_union, (double)pl.rows_union / pl.blocks.size(), pl.rows_carried, pl.carried_fraction());
        }
        return g_fail ? 1 : 0;
    }
    one_case("single short block", 16, 1, false, 3, 12, false);          // range of 9 positions: one node per chunk, then two
    one_case("G = 9", 9, 2, false, 0, -1, false);
    one_case("G = 64", 64, 3, false, 0, -1, false);
    one_case("G = 500", 500, 4, false, 0, -1, false);
    one_case("G = 500 shuffled", 500, 5, true, 0, -1, true);
    one_case("G = 500 range mid-grid", 500, 6, false, 137, 401, false);
    one_case("G = 300 range of one chunk", 300, 7, false, 100, 107, false);
    {   // bad arguments are refused
        const std::vector<int32_t> tab = random_table(32, 8, false, 1.0);
        Plan pl;
        std::vector<int32_t> bad = tab;
        bad[16 * 5 + 3] = 32;
        if (s2u_plan::build(tab.data(), 32, 32, 0, 33, 2, pl) || s2u_plan::build(tab.data(), 32, 32, 0, 32, 0, pl) ||
            s2u_plan::build(bad.data(), 32, 32, 0, 32, 2, pl) || !s2u_plan::build(tab.data(), 32, 32, 7, 7, 2, pl) || !pl.blocks.empty()) {
            fprintf(stderr, "FAIL bad arguments\n"); ++g_fail;
        }
    }
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("s2u_plan_check: ok\n");
    return 0;
}
