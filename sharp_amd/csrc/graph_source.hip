// graph_source.hip -- see graph_source.hpp.  No kernel lives here: every launch is behind upload_neighbours (knn.hip), umap_sqrt_lists
// and umap_graph (umap.hip) or snn_graph (snn.hip), in the code objects that have held them from the start.
#include "graph_source.hpp"

#include "knn.hpp"
#include "snn.hpp"
#include "umap.hpp"

namespace sharp {

void lists_to_device(const std::string &who, const int *index, const double *distance, long long n, int K, bool squared, DevBuf<int> &idx,
                     DevBuf<double> &dist) {
    upload_neighbours(who.c_str(), index, distance, n, K, true, idx, dist);   // (true: nothing is squared there)
    if (squared) umap_sqrt_lists(dist, n, K);
}

void fuzzy_graph_from_lists(const std::string &who, const int *index, const double *distance, long long n, int K, bool squared, Graph &G) {
    DevBuf<int> idx;
    DevBuf<double> dist;
    lists_to_device(who, index, distance, n, K, squared, idx, dist);
    umap_graph(idx, dist, n, K, G);
    idx.release();
    dist.release();
}

void snn_graph_from_lists(const std::string &who, const int *index, long long n, int K, double prune, Graph &G) {
    {
        DevBuf<int> idx(static_cast<size_t>(n) * K);
        idx.upload(index, static_cast<size_t>(n) * K);
        snn_graph(who, idx, n, K, prune, false, G, nullptr);   // (synchronises: idx leaves scope)
    }
    SHARP_REQUIRE(G.nnz >= 1 && G.wmax > 0.0, who + ": the pruned graph holds no positive weight");
}

}  // namespace sharp
