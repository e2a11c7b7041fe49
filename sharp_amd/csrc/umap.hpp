// umap.hpp -- the UMAP embedding beside t-SNE: the a / b curve fitted on the host, the fuzzy graph from k-NN lists (one
// wave per row: rho, the bisection on sigma; the union A + A^T - A o A^T as a CSR), and the epoch optimiser (stateless schedule,
// hashed negative samples, all rows updated at once from the old positions).  Input preparation is prepare.hpp's, the exact k-NN and the
// validation of given lists are knn.hpp's.  The C ABI entries (sharp_umap*, include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include "graph.hpp"

namespace sharp {

// the clip of every gradient term of the epochs, umap's and the transform's
__device__ __forceinline__ double clip4(double v) { return fmin(4.0, fmax(-4.0, v)); }

// W = A + A^T - A o A^T, CSR on the device (rows sorted by column), wmax = max W
using UmapGraph = Graph;

// a, b minimising sum_k (1 / (1 + a x_k^(2b)) - y(x_k))^2 over the 300 points x = linspace(0, 3 spread); host only, no device
void umap_ab(double spread, double min_dist, double *a, double *b);
// the graph from the lists (device, n x K, Euclidean distances, self excluded; n_neighbors = K + 1); rho / sigma (n each) when wanted
void umap_graph(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, UmapGraph &G, DevBuf<double> *rho = nullptr,
                DevBuf<double> *sigma = nullptr);
// squared distances of lists (device, n x K) made Euclidean in place
void umap_sqrt_lists(DevBuf<double> &dist, long long n, int K);
// epochs [ep0, ep1) of n_epochs on dY (device, n x dims, in and out)
void umap_epochs(const UmapGraph &G, double *dY, int dims, int n_epochs, int ep0, int ep1, double learning_rate, double a, double b,
                 int negative_sample_rate, double repulsion_strength, unsigned long long seed);

// ---- the spectral start, init = "normlaplacian" (umap_spectral.hip) ----
struct UmapSpectral {
    int outcome = 0;             // 0 converged, 1 not connected (nothing solved), 2 not converged
    int steps = 0;               // Lanczos steps taken
    long long components = 0;
    double theta[3] = {0.0, 0.0, 0.0};      // outcome 0: the dims largest eigenvalues of M = D^-1/2 W D^-1/2 below the trivial 1
    double residual[3] = {0.0, 0.0, 0.0};   // outcome 0: the true ||M v - theta v||; outcome 2: the last estimates
    std::vector<double> V;       // outcome 0: the unit eigenvectors, n x dims row-major (host), the largest |component| positive
};
// the number of connected components of G's pattern; label (n, device) = the smallest vertex of each vertex's component when wanted
long long umap_components(const UmapGraph &G, DevBuf<int> *label = nullptr);
// the same sweeps on any CSR pattern on the device (1 <= n < 2^31): label[i] = the smallest vertex of i's component; within (n, device,
// or null): only the entries whose two ends carry the same value count -- the components inside a labelling (Leiden).
// Self-loops never count.  timer: the name the sweeps are timed under.  Returns the number of components.
long long csr_components(const long long *row_ptr, const int *col, long long n, const int *within, DevBuf<int> &label, const char *timer);
// tol <= 0 / max_steps <= 0: the library's defaults (1e-6, 400); max_steps is capped at n - 2
void umap_spectral(const UmapGraph &G, int dims, double tol, int max_steps, UmapSpectral &R);
// what the calling context's last sharp_umap / sharp_umap_neighbors call started from (init codes: 0 pca, 1 random, 2 Y_init,
// 3 normlaplacian); components, steps and residual are the spectral stage's, 0 when it did not run
struct UmapInitInfo {
    int requested = -1, used = -1;
    long long components = 0;
    int steps = 0;
    double residual = 0.0;
};
UmapInitInfo &umap_init_info();

}  // namespace sharp
