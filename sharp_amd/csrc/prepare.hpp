// prepare.hpp -- input preparation for the maps: column statistics in a fixed order, the affine map of rows, PCA by
// X^T X on the f64 MFMA and a host symmetric eigensolver, normalisation.  Rtsne and umap prepare their input with it, the exact k-NN
// (knn.hip) centres with it, expression_pca (expr_pca.hip) uses the eigensolver.  Refusals begin with the caller's name `who`.
#pragma once
#include <vector>

#include "graph.hpp"

namespace sharp {

// column means (mu == nullptr) or sums of squared deviations, / div: out[0 .. d), device; part: the slabs' partial sums
SHARP_LOCAL void column_stat(const double *X, long long n, int d, long long ld, const double *mu, double div, DevBuf<double> &part, double *out);
// out[i * d + c] = (X[i * ld + c] - mu[c]) / (sd ? sd[c] : scal); mu may be null; in place when out == X and ld == d
SHARP_LOCAL void affine_rows(const double *X, long long n, int d, long long ld, const double *mu, const double *sd, double scal, double *out);
// X (n rows of d values, row i at X + i * ld, host) -> the prepared matrix on the device (n x d_out, row-major, ld d_out):
// PCA to min(initial_dims, d) components if pca, then centring and division by the largest |entry| if normalize
SHARP_LOCAL void prepare_input(const char *who, const double *X, long long n, int d, long long ld, bool pca, int initial_dims, bool pca_center,
                               bool pca_scale, bool normalize, DevBuf<double> &out, int *d_out);
// the host eigensolver behind the PCA (Householder + implicit QL), for a caller with a small symmetric matrix of its own:
// V (d x d, row-major) holds the matrix on entry and the eigenvectors as columns on exit, w their eigenvalues (the caller orders them)
SHARP_LOCAL void symmetric_eigen(const char *who, int d, std::vector<double> &V, std::vector<double> &w);

}  // namespace sharp
