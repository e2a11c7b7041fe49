// knn_descent.hpp -- the approximate k-NN beside tsne_knn: a start from sorted random projections, then NN-descent joins
// in a bulk-synchronous gather form.  Every pair a list keeps carries the direct sum (x_i - x_j)^2 in column order, the bits tsne_knn's
// re-rank gives the same pair; the lists are a pure function of (X, K, the parameters, seed).  The C ABI entries (sharp_knn_descent*,
// include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include "common.hpp"

namespace sharp {

struct KnnDescentInfo {
    long long joins = 0;     // joins run
    long long updates = 0;   // entries the last join changed (0 when none ran)
    long long reason = 0;    // 0: n_iters reached, 1: updates <= delta n K
    long long gathered = 0;  // candidate rows the joins gathered and measured (what the filters let through)
};

// S = max_candidates, 0: min(K, 30)
int knn_descent_candidates(int K, int max_candidates);
// the start alone: dX (n x d, device, finite) -> each row's K best of its T windows, sorted by (distance, index).
// max_rows_per_launch 0: the library's choice; it only cuts the work into launches.
void knn_descent_start(const double *dX, long long n, int d, int K, int n_projections, unsigned long long seed, int max_rows_per_launch,
                       DevBuf<int> &idx, DevBuf<double> &dist2);
// sorted lists with their distances from indices alone (n x K, device, validated by the caller)
void knn_descent_lists(const double *dX, long long n, int d, int K, const int *index, int max_rows_per_launch, DevBuf<int> &idx,
                       DevBuf<double> &dist2);
// join number `iteration` (1-based) from sorted lists: idx / dist2 are replaced by the joined lists; returns the entries that changed
// and adds the candidate rows it gathered to *gathered
long long knn_descent_join(const double *dX, long long n, int d, int K, int S, int iteration, unsigned long long seed, int max_rows_per_launch,
                           DevBuf<int> &idx, DevBuf<double> &dist2, long long *gathered = nullptr);
// start, then joins until updates <= delta n K or n_iters
void knn_descent(const double *dX, long long n, int d, int K, int n_projections, int max_candidates, int n_iters, double delta,
                 unsigned long long seed, DevBuf<int> &idx, DevBuf<double> &dist2, KnnDescentInfo &info);

}  // namespace sharp
