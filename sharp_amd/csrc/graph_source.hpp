// graph_source.hpp -- the one way in for each source of a neighbour graph: a caller's neighbour lists made Euclidean on
// the device, the same lists turned into UMAP's fuzzy union (umap.hpp), or into the SNN / Jaccard graph (snn.hpp).  The third source, a
// caller's own CSR, goes through graph.hpp's csr_to_device behind the consumer's own checks.  umap, Louvain, Leiden and the diffusion
// map come through here; a new consumer of a graph does too, instead of calling upload_neighbours, umap_graph or snn_graph itself.
// Host code only, on ctx().stream; the entry has checked the arguments (pointers, n, K, prune), the lists' contents are validated
// here, and refusals begin with the entry's name `who`.
#pragma once
#include <string>

#include "graph.hpp"

namespace sharp {

// the lists (host, n x K; index 0-based) on the device, validated as upload_neighbours validates them; dist: Euclidean distances
// (squared: the caller's are their squares)
SHARP_LOCAL void lists_to_device(const std::string &who, const int *index, const double *distance, long long n, int K, bool squared,
                                 DevBuf<int> &idx, DevBuf<double> &dist);
// G = umap_graph of those lists (n_neighbors = K + 1); the lists are released before it returns
SHARP_LOCAL void fuzzy_graph_from_lists(const std::string &who, const int *index, const double *distance, long long n, int K, bool squared,
                                        Graph &G);
// G = snn_graph(index, prune) in full; a prune that leaves no positive weight is refused
SHARP_LOCAL void snn_graph_from_lists(const std::string &who, const int *index, long long n, int K, double prune, Graph &G);

}  // namespace sharp
