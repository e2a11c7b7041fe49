// snn.hpp -- the shared-nearest-neighbour graph with Jaccard weights (Seurat's ComputeSNN): from k-NN lists, the sparse
// product A A^T of the 0/1 matrix with k = K + 1 ones per row (the row itself and its K neighbours), the diagonal left out:
// s(i, j) = |S(i) n S(j)|, w = s / (2k - s), an entry kept iff w >= prune.  Everything the device computes is an integer, so a call is a
// pure function of its arguments.  The result is a Graph (graph.hpp) on the device: what louvain_quantise takes.  The C ABI entries
// (sharp_snn_graph, sharp_louvain_snn, include/sharp_hip.h) wrap these.
#pragma once
#include <string>

#include "graph.hpp"

namespace sharp {

constexpr long long kSnnMaxN = 1ll << 24;
constexpr long long kSnnMaxNnz = 1ll << 38;
// Row classes by the row work t(i) = sum over m in S(i) of |R(m)| (the candidate increments of row i, an upper bound on its distinct
// candidates); a table is at most three quarters full at its cap
constexpr int kSnnWaveSlots = 2048, kSnnWaveCap = 1536;      // one wave per row, a 16 KB LDS table
constexpr int kSnnBlockSlots = 8192, kSnnBlockCap = 6144;    // one workgroup per row, a 64 KB LDS table; beyond: a dense counter row in HBM

// the smallest s in 1 .. k with (double)s / (double)(2k - s) >= prune (w rises with s and w(k) = 1, so there is one for prune in [0, 1])
int snn_min_shared(int k, double prune);
// the lists as the entries take them: refused by name (who) before any device work
void snn_check_args(const std::string &who, long long n, int K, double prune);
// idx: n x K on the device, not yet validated (range, self, an index twice in a row are refused here, before an index is dereferenced).
// count_only: G.row_ptr, G.n and G.nnz only.  Otherwise G in full (col ascending within a row, val, wmax) and, when wanted, the s of
// every entry.  cap >= 0: a graph of more entries is refused after the count, with the count in the message and in G.nnz.
void snn_graph(const std::string &who, const DevBuf<int> &idx, long long n, int K, double prune, bool count_only, Graph &G,
               DevBuf<int> *shared, long long cap = -1);

}  // namespace sharp
