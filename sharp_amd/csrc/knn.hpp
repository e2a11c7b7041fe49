// knn.hpp -- the exact k-NN on the f64 MFMA, of a matrix against itself and of query rows against a reference,
// the selection from given distances, and the lists a caller brings: one check, one set of fault kinds, one decoder.  Rtsne, umap,
// umap_transform, louvain_neighbors, knn_descent, the neighbour ranks and the SNN graph all come through here.  Refusals begin with the
// caller's name `who`.
#pragma once
#include <string>

#include "graph.hpp"

namespace sharp {

// ---- the launch plan ------------------------------------------------------------------------------------------------------------------
// Launches of about 8e9 candidate pairs at d = 50 (measured 1e11 pairs / s at d = 50: under 0.1 s each at any n)
SHARP_LOCAL double knn_pair_budget(int d);
// nq query rows against nref candidate rows of d columns: rows per launch from that budget (a multiple of 16; at most max_rows when
// max_rows > 0), and the candidate columns cut into chunks (of cols columns, a multiple of 64) so that a launch has >= ~1024 workgroups
// however few its rows are.  The plan changes no list: a pair's value depends on d and its two rows, and every comparison is exact.
struct KnnPlan {
    long long rows, cols;
    int chunks;
};
SHARP_LOCAL KnnPlan knn_plan(long long nq, long long nref, int d, int max_rows);

// ---- the searches ---------------------------------------------------------------------------------------------------------------------
// exact K nearest neighbours of every row of dX (n x d, device), self excluded, ties by the lower index; sorted by (distance, index),
// distances re-ranked as sum (x_i - x_j)^2
SHARP_LOCAL void knn_self(const char *who, const double *dX, long long n, int d, int K, DevBuf<int> &idx, DevBuf<double> &dist);
// the K nearest neighbours of every object from R's dist vector d (host, n (n - 1) / 2 entries, finite and >= 0; n <= SHARP_DIST_MAX_N):
// selected on the distances as given (exact comparisons, ties by the lower index, self excluded), sorted by (distance, index);
// dist2 = d * d.  The vector and the full matrix are released before it returns.
SHARP_LOCAL void knn_from_dist(const char *who, const double *d, int n, int K, DevBuf<int> &idx, DevBuf<double> &dist2);
// out = X - mu (n x d, device) and its squared row norms; refuses, with msg, norms that are not finite or would overflow a squared distance
SHARP_LOCAL void center_and_norm(const double *dX, long long n, int d, const double *mu, DevBuf<double> &out, DevBuf<double> &nrm,
                                 const std::string &msg);
// the K nearest rows of the reference X (n x d, device; W = X - mu and wn its squared row norms, as center_and_norm leaves them) of
// every row of dXq (device, nq x d packed): idx / dist (device, nq x K, Euclidean), ties by the lower index
SHARP_LOCAL void knn_cross(const char *who, const double *W, const double *wn, const double *X, const double *mu, long long n, int d,
                           const double *dXq, long long nq, int K, int max_rows, DevBuf<int> &idx, DevBuf<double> &dist);

// ---- the lists a caller brings --------------------------------------------------------------------------------------------------------
// What a check kernel finds wrong with a row of lists, before anything dereferences an index.  A kernel lowers a word that starts as
// NN_OK to (row << 3 | kind) by atomicMin: the first offending row and its lowest kind, whatever the scheduling.
enum NnKind { NN_RANGE = 1, NN_SELF = 2, NN_TWICE = 3, NN_DIST = 4 };
constexpr unsigned long long NN_OK = ~0ull;
// the Error that such a word stands for, in who's name (word != NN_OK)
[[noreturn]] SHARP_LOCAL void throw_list_fault(const std::string &who, unsigned long long word);
// a caller's neighbour lists (host, n x K; index 0-based) on the device, validated (range, self, an index twice in a row, distances
// finite and >= 0); squared == 0: the distances are squared on the device.  The lists keep the caller's order.
SHARP_LOCAL void upload_neighbours(const char *who, const int *index, const double *distance, long long n, int K, bool squared, DevBuf<int> &idx,
                                   DevBuf<double> &dist2);

}  // namespace sharp
