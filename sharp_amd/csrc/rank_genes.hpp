// rank_genes.hpp -- per-cluster differential expression on the gene-major copy of expr_load: the limits and the options
// of rank_genes.hip.  The C ABI entries (sharp_rank_genes_csc, sharp_rank_sums_csc; include/sharp_hip.h) are thin wrappers over it.
#pragma once
#include "expr_pca.hpp"

namespace sharp {

constexpr int kRankMaxGroups = 1024;             // a group id takes the low 10 bits of the (run, group) key
constexpr int kRankGroupBits = 10;
constexpr long long kRankMaxCells = 2097151;     // 2^21 - 1: the sum of t^3 - t stays below 2^63, a run's start fits 21 bits
constexpr int kRankChunk = kExprChunk;           // entries of a gene that one wave of the statistics kernels takes: expr_load's chunks

struct RankOptions {
    int G = 0;
    int method = 0;                              // 0 Wilcoxon, 1 Welch
    int reference = -1;                          // -1: the rest
    bool log1p = true, tie_correct = true, continuity = false;
};

}  // namespace sharp
