// umap.hpp -- the UMAP embedding beside t-SNE: the a / b curve fitted on the host, the fuzzy graph from k-NN lists (one
// wave per row: rho, the bisection on sigma; the union A + A^T - A o A^T as a CSR), and the epoch optimiser (stateless schedule,
// hashed negative samples, all rows updated at once from the old positions).  Input preparation, the exact k-NN and the validation of
// given lists are t-SNE's (tsne.hpp).  The C ABI entries (sharp_umap*, include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include "common.hpp"

namespace sharp {

// W = A + A^T - A o A^T, CSR on the device (rows sorted by column), wmax = max W
struct UmapGraph {
    long long n = 0, nnz = 0;
    DevBuf<long long> row_ptr;   // n + 1
    DevBuf<int> col;             // nnz
    DevBuf<double> val;          // nnz
    double wmax = 0.0;
};

// a, b minimising sum_k (1 / (1 + a x_k^(2b)) - y(x_k))^2 over the 300 points x = linspace(0, 3 spread); host only, no device
void umap_ab(double spread, double min_dist, double *a, double *b);
// the graph from the lists (device, n x K, Euclidean distances, self excluded; n_neighbors = K + 1); rho / sigma (n each) when wanted
void umap_graph(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, UmapGraph &G, DevBuf<double> *rho = nullptr,
                DevBuf<double> *sigma = nullptr);
// epochs [ep0, ep1) of n_epochs on dY (device, n x dims, in and out)
void umap_epochs(const UmapGraph &G, double *dY, int dims, int n_epochs, int ep0, int ep1, double learning_rate, double a, double b,
                 int negative_sample_rate, double repulsion_strength, unsigned long long seed);

}  // namespace sharp
