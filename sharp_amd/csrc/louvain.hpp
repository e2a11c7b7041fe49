// louvain.hpp -- Louvain community detection on a symmetric weighted graph: the project's own synchronous form of the
// method, built so that a call is a pure function of its arguments.  Weights are quantised to integers once (rule 1), so every sum of
// weights is an exact int64 sum whatever the order of the atomics; a round of local moving works from the round's start state and lets
// a community either lose or gain members (one hashed bit per community and round, rule 2); a round is kept when the modularity, summed
// in a fixed order, rises by more than tol (rule 3); the communities become the next level's vertices (rule 4).  The graph is what
// umap_graph or snn_graph leave on the device (graph.hpp's Graph), or any symmetric CSR.  The C ABI entries (sharp_louvain_*, include/sharp_hip.h) wrap these.
#pragma once
#include <vector>

#include "graph.hpp"

namespace sharp {

// one level's graph on the device: integer weights, rows sorted by column, a self-loop entry holds a coarse vertex's internal weight
struct LouvainGraph : Csr<u64> {             // val: the integer weights q
    long long m2 = 0;                        // 2m = sum of k
    DevBuf<int> row;                         // nnz: the row of every entry
    DevBuf<u64> k;                           // n strengths
};

struct LouvainArgs {
    double resolution = 1.0, tol = 1e-7;
    int max_levels = 20, max_rounds = 200, max_fails = 4;
    unsigned long long seed = 10;
};

struct LouvainLevel {
    long long n = 0, communities = 0;
    int rounds = 0;
    double q = 0.0;
};

constexpr long long kLvMaxN = 1ll << 24;
constexpr long long kLvMaxNnz = 1ll << 38;
constexpr int kLvWaveCap = 128;              // rows up to this many entries: one wave, a 256-slot LDS table
constexpr int kLvBlockCap = 3072;            // up to this many: one workgroup, a 4096-slot LDS table; longer rows: a dense row in HBM

// rule 1 on a float-weighted graph; q = 0 entries are dropped from L
void louvain_quantise(const Graph &G, LouvainGraph &L);
// rules 2 - 5; membership: 1 .. G by decreasing size (host, n values); level_membership (when wanted): levels x n, the 0-based coarse
// vertex of every input vertex after each level
void louvain_run(LouvainGraph &L, const LouvainArgs &a, std::vector<int> &membership, std::vector<LouvainLevel> &levels,
                 std::vector<int> *level_membership);

}  // namespace sharp
