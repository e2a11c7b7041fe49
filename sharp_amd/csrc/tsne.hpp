// tsne.hpp -- the exact t-SNE embedding behind visualization_SHARP (R/visualization_SHARP.R:94 calls Rtsne there): input preparation
// (PCA, normalisation), exact k-NN on the f64 MFMA, per-row perplexity calibration, the symmetric P in CSR, and the optimiser loop with
// an exact O(n^2) repulsion or bhtsne's Barnes-Hut one.  The C ABI entries (sharp_tsne*, include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include "graph.hpp"

namespace sharp {

// P = (P_cond + P_cond^T) / sum, CSR on the device (rows sorted by column)
using TsneP = Csr<double>;

// X (n rows of d values, row i at X + i * ld, host) -> the prepared matrix on the device (n x d_out, row-major, ld d_out):
// PCA to min(initial_dims, d) components if pca, then centring and division by the largest |entry| if normalize
void tsne_prepare(const double *X, long long n, int d, long long ld, bool pca, int initial_dims, bool pca_center, bool pca_scale,
                  bool normalize, DevBuf<double> &out, int *d_out);
// exact K nearest neighbours of every row of dX (n x d, device), self excluded, ties by the lower index; sorted by (distance, index),
// distances re-ranked as sum (x_i - x_j)^2
void tsne_knn(const double *dX, long long n, int d, int K, DevBuf<int> &idx, DevBuf<double> &dist);
// calibration + symmetrisation: P from the k-NN lists
void tsne_affinities(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, double perplexity, TsneP &P);
// the K nearest neighbours of every object from R's dist vector d (host, n (n - 1) / 2 entries, finite and >= 0; n <= SHARP_DIST_MAX_N):
// selected on the distances as given (exact comparisons, ties by the lower index, self excluded), sorted by (distance, index);
// dist2 = d * d.  The vector and the full matrix are released before it returns.
void tsne_knn_dist(const double *d, int n, int K, DevBuf<int> &idx, DevBuf<double> &dist2);
// a caller's neighbour lists (host, n x K; index 0-based) on the device, validated by a kernel before anything dereferences an index
// (range, self, an index twice in a row, distances finite and >= 0: an Error naming the first offending row); squared == 0: the
// distances are squared on the device.  The lists keep the caller's order.
void tsne_upload_neighbours(const int *index, const double *distance, long long n, int K, bool squared, DevBuf<int> &idx,
                            DevBuf<double> &dist2);
// dY = sum_j P_ij q_ij (y_i - y_j) - (1/Z) sum_j q_ij^2 (y_i - y_j) at Y (device, n x dims); theta > 0: the repulsion and Z by
// Barnes-Hut at that theta; Z (host, may be null) receives Z
void tsne_gradient(const TsneP &P, const double *dY_in, int dims, double *dGrad, double theta = 0.0, double *Z = nullptr);
// the host eigensolver behind tsne_prepare's PCA (Householder + implicit QL), for a caller with a small symmetric matrix of its own:
// V (d x d, row-major) holds the matrix on entry and the eigenvectors as columns on exit, w their eigenvalues (the caller orders them)
void symmetric_eigen(int d, std::vector<double> &V, std::vector<double> &w);

}  // namespace sharp
