// tsne.hpp -- the exact t-SNE embedding behind visualization_SHARP (R/visualization_SHARP.R:94 calls Rtsne there): per-row perplexity
// calibration, the symmetric P in CSR, and the optimiser loop with an exact O(n^2) repulsion or bhtsne's Barnes-Hut one.  Input
// preparation is prepare.hpp's, the neighbour lists are knn.hpp's.  The C ABI entries (sharp_tsne*, include/sharp_hip.h) are thin
// wrappers over these.
#pragma once
#include "graph.hpp"

namespace sharp {

// P = (P_cond + P_cond^T) / sum, CSR on the device (rows sorted by column)
using TsneP = Csr<double>;

// calibration + symmetrisation: P from the k-NN lists
void tsne_affinities(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, double perplexity, TsneP &P);
// dY = sum_j P_ij q_ij (y_i - y_j) - (1/Z) sum_j q_ij^2 (y_i - y_j) at Y (device, n x dims); theta > 0: the repulsion and Z by
// Barnes-Hut at that theta; Z (host, may be null) receives Z
void tsne_gradient(const TsneP &P, const double *dY_in, int dims, double *dGrad, double theta = 0.0, double *Z = nullptr);

}  // namespace sharp
