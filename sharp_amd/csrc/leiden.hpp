// leiden.hpp -- Leiden community detection on a symmetric weighted graph: Louvain's levels (louvain.hpp, §18's rules
// 1 - 4 unchanged) with a refinement between a level's move phase and its aggregation.  The move phase starts from a given partition
// (L1); its result P is re-partitioned from the singletons into well-connected sub-communities that never leave their community of P
// (L2); the sub-communities become the next level's vertices and the connected parts of P its start (L3); the returned partition is
// the last level's P split into its connected components (L4).  The project's own deterministic form: a call is a pure function of
// its arguments; no parity with leidenalg, igraph or scanpy is claimed.  The C ABI entries (sharp_leiden_*, include/sharp_hip.h) wrap
// these.
#pragma once
#include <vector>

#include "louvain.hpp"

namespace sharp {

constexpr int kLdMaxRefineRounds = 100000;
constexpr int kLdRefineRound0 = 1 << 30;     // the refinement's bits are §18's h at the round number 2^30 + r

// rules L1 - L4 on a quantised graph; membership: 1 .. G by decreasing size (host, n values); Q: of that membership on L;
// levels: louvain.hpp's record, with the sub-communities and the refinement's rounds filled in, q that of the level's P;
// level_membership (when wanted): levels x n, the 0-based rank of the community P of every input vertex at each level
void leiden_run(LouvainGraph &L, const LouvainArgs &a, int max_refine_rounds, std::vector<int> &membership, double *Q,
                std::vector<LouvainLevel> &levels, std::vector<int> *level_membership);

}  // namespace sharp
