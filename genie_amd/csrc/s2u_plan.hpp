// Plan of k_stage2_h2u's block table: plain C++, no HIP calls (genie_hip.hip includes it; tests/s2u_plan_check.cpp builds it alone).
//
// A range [gb0, ge0) of the processing order is cut into NXCD chunks (the chunks of ItemIter), every chunk into blocks of up to NB
// consecutive source nodes whose neighbour rows (their union, in first-use order) fit UCAP rows; a block is cut short where the
// union would grow past that. The kernel stages a block's union rows in LDS slots and every node sums its 15 rows from there.
//
// Groups: L consecutive blocks of a chunk form a group (the last group of a chunk may be shorter). A workgroup runs the blocks of
// a group in order for one station tile, so the rows of LDS that the next block needs again stay where they are:
//  * the first block of a group stages its whole union, union row u into slot u;
//  * in every later block a union row whose source node is still resident (left by ANY earlier block of the group) keeps its slot,
//    a new row takes a slot whose occupant the block does not use (empty slots first, then the least recently used occupant);
//  * idx[b][1 + k] names the SLOT of node b's k-th neighbour; ids[e] / slot[e], e < nst, list the rows to stage and where to.
// With L = 1 every block is a group's first: slot[e] = e, nst = U, and the table is the one the kernel has always read.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace s2u_plan {

constexpr int NB = 8;        // source nodes per block
constexpr int UCAP = 64;     // LDS slots = distinct neighbour rows of a block
constexpr int KP = 15;       // neighbours per source node
constexpr int NXCD = 8;      // chunks of a range

struct Block {
    int32_t gi0, n, U, nst;  // first position, source nodes (1 .. NB), union size, rows to stage (= U in a group's first block)
    int32_t ids[64];         // source node of staged row e (padded with the first one); one per lane of the wave that stages them
    int32_t idx[NB][16];     // node b: [0] = its source node id (-1: the block has no node b), [1 + k] = slot of its k-th neighbour
    uint8_t slot[64];        // LDS slot of staged row e (padding: 0)
};

struct Plan {
    std::vector<Block> blocks;
    int32_t xcd0[NXCD + 1];  // first block of every chunk, then the block count
    int L;                   // blocks per group
    long long rows_union, rows_carried;      // summed over all blocks: union rows, and those of them that were not staged again
    double carried_fraction() const { return rows_union ? (double)rows_carried / (double)rows_union : 0.0; }
};

// tab: [n_pos][16] of the processing order, [0] = source node id, [1 + k] = its k-th neighbour (node ids in [0, n_nodes)).
// Returns false (plan untouched in its meaning) on a bad argument: range outside [0, n_pos], L < 1, a neighbour id out of range.
inline bool build(const int32_t* tab, int n_pos, int n_nodes, int gb0, int ge0, int L, Plan& out) {
    out.blocks.clear();
    out.L = L;
    out.rows_union = out.rows_carried = 0;
    for (int x = 0; x <= NXCD; ++x) out.xcd0[x] = 0;
    if (!tab || gb0 < 0 || ge0 > n_pos || gb0 > ge0 || L < 1 || n_nodes < 1) return false;
    for (size_t i = (size_t)gb0 * 16; i < (size_t)ge0 * 16; ++i)
        if ((i & 15) && (tab[i] < 0 || tab[i] >= n_nodes)) return false;
    // membership of a neighbour row in the block's union by a stamp per source node (`seen_blk[nb]` = serial of the block that
    // listed it, `seen_at[nb]` = its position there): the table of 10 000 source nodes builds in ~0.2 ms, where a linear search
    // of the union per neighbour took 2.5 ms of every context (re)build of a training sample
    std::vector<int32_t> seen_blk((size_t)n_nodes, -1), seen_at((size_t)n_nodes, 0);
    std::vector<int32_t> slot_of((size_t)n_nodes, -1);      // LDS slot that holds the node's row in the running group, -1: none
    int32_t serial = 0;
    const int n = ge0 - gb0;
    for (int x = 0; x < NXCD; ++x) {
        out.xcd0[x] = (int32_t)out.blocks.size();
        const int gb = gb0 + (int)((long long)n * x / NXCD), ge = gb0 + (int)((long long)n * (x + 1) / NXCD);
        int pos = gb;
        int32_t occ[UCAP], last_use[UCAP];       // slot -> source node (-1: empty), serial of the last block that used it
        int in_group = 0;
        for (int s = 0; s < UCAP; ++s) { occ[s] = -1; last_use[s] = -1; }
        while (pos < ge) {
            Block b;
            memset(&b, 0, sizeof(b));
            b.gi0 = pos;
            ++serial;
            int32_t uni[UCAP + KP];
            int nuni = 0;
            while (pos < ge && b.n < NB) {
                int32_t where[KP];
                const int before = nuni;
                for (int k = 0; k < KP; ++k) {
                    const int32_t nb = tab[(size_t)pos * 16 + 1 + k];
                    if (seen_blk[(size_t)nb] != serial) { seen_blk[(size_t)nb] = serial; seen_at[(size_t)nb] = nuni; uni[nuni++] = nb; }
                    where[k] = seen_at[(size_t)nb];
                }
                if (b.n > 0 && nuni > UCAP) {       // the node does not fit: take its additions back, it opens the next block
                    for (int u = before; u < nuni; ++u) seen_blk[(size_t)uni[u]] = -1;
                    nuni = before;
                    break;
                }
                b.idx[b.n][0] = tab[(size_t)pos * 16];
                for (int k = 0; k < KP; ++k) b.idx[b.n][1 + k] = where[k];
                ++b.n; ++pos;
            }
            if (nuni > UCAP) return false;          // (a single node lists 15 rows: cannot happen)
            for (int e = b.n; e < NB; ++e) b.idx[e][0] = -1;       // empty slots of a short block
            b.U = (int32_t)nuni;
            // ---- union row u -> LDS slot
            int32_t slot_u[UCAP];
            int nst = 0;
            if (in_group == 0) {                    // a group's first block stages everything, row u into slot u
                for (int s = 0; s < UCAP; ++s) {
                    if (occ[s] >= 0) slot_of[(size_t)occ[s]] = -1;
                    occ[s] = -1; last_use[s] = -1;
                }
                for (int u = 0; u < nuni; ++u) {
                    slot_u[u] = u;
                    b.ids[nst] = uni[u]; b.slot[nst] = (uint8_t)u; ++nst;
                }
            } else {
                for (int u = 0; u < nuni; ++u) {    // resident rows keep their slots
                    slot_u[u] = slot_of[(size_t)uni[u]];
                    if (slot_u[u] >= 0) last_use[slot_u[u]] = serial;
                }
                for (int u = 0; u < nuni; ++u) {    // new rows: the empty or least recently used slot that this block does not read
                    if (slot_u[u] >= 0) continue;
                    int best = -1;
                    for (int s = 0; s < UCAP; ++s)
                        if (last_use[s] != serial && (best < 0 || last_use[s] < last_use[best])) best = s;
                    if (best < 0) return false;     // (nuni <= UCAP slots: cannot happen)
                    slot_u[u] = best; last_use[best] = serial;
                    b.ids[nst] = uni[u]; b.slot[nst] = (uint8_t)best; ++nst;
                }
            }
            for (int e = 0; e < nst; ++e) {
                const int s = b.slot[e];
                if (occ[s] >= 0) slot_of[(size_t)occ[s]] = -1;
                occ[s] = b.ids[e]; slot_of[(size_t)b.ids[e]] = s; last_use[s] = serial;
            }
            b.nst = nst;
            for (int e = nst; e < 64; ++e) b.ids[e] = nst ? b.ids[0] : uni[0];
            for (int i = 0; i < b.n; ++i)
                for (int k = 0; k < KP; ++k) b.idx[i][1 + k] = slot_u[b.idx[i][1 + k]];
            out.rows_union += nuni;
            out.rows_carried += nuni - nst;
            out.blocks.push_back(b);
            if (++in_group == L) in_group = 0;
        }
        for (int s = 0; s < UCAP; ++s)
            if (occ[s] >= 0) slot_of[(size_t)occ[s]] = -1;
    }
    out.xcd0[NXCD] = (int32_t)out.blocks.size();
    return true;
}

}  // namespace s2u_plan
