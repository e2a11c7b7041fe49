// doublets.hpp -- Scrublet-style doublet detection from sparse count blocks: the pairs, the simulated doublets made on the
// device from the resident cell-major copy (a merge of two sorted sparse columns per doublet, in slabs), their PCA scores through the
// transform route of expr_pca.hip, the count of simulated neighbours, the score table and the threshold.  The C ABI entries
// (sharp_doublet_*, sharp_scrublet_csc, include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "expr_pca.hpp"

namespace sharp {

constexpr int kDoubletMaxK = 255;                // the k-NN stages' limit on K = k_adj
constexpr int kDoubletBins = 256;                // bins of the simulated scores' histogram
constexpr int kDoubletMaxSmooth = 10000;         // three-bin means at the most
constexpr double kDoubletSlabBytes = 1073741824.0;   // the budget of a slab's two copies (the merged one and the gene subset)

// what a call works with, from (n, ratio, n_neighbors); n_neighbors 0: the default min(round(0.5 sqrt(n)), the largest whose k_adj fits)
struct DoubletPlan {
    long long n_sim = 0;
    int n_neighbors = 0, k_adj = 0;
};
// round(x) = floor(x + 0.5) everywhere.  Refuses by name, in who's name; needs no device.
DoubletPlan doublet_plan(const std::string &who, long long n, double sim_doublet_ratio, int n_neighbors);
// parents[2 s], parents[2 s + 1] = floor((double)(h(s, j) >> 11) 2^-53 (double)n), j = 0, 1; h(s, j) = mix64(mix64(seed G + s) + j)
void doublet_pairs(long long n, long long n_sim, u64 seed, long long *parents);
u64 doublet_seed(const std::string &who, long long seed);
void doublet_check_parents(const std::string &who, const long long *parents, long long n_sim, long long n);

// One slab of simulated doublets on the device, as an ExprData whose values are the summed counts and whose lsum is L_a + L_b.
// Calls fn(first doublet, the slab) slab after slab; the slab's buffers are the callee's until it returns (it may transform, subset
// and multiply them).  D: the observed cells' raw counts (expr_load without a transform).  len: the stored entries of every observed
// cell (host), from which the slabs are cut so that no slab holds more than the budget; max_per_slab > 0 cuts further.
void doublet_slabs(const ExprData &D, const std::vector<long long> &len, const long long *parents, long long n_sim, int max_per_slab,
                   const std::function<void(long long, ExprData &)> &fn);
// the doublets' PCA scores (device, n_sim x k at Y): per slab the transform, the subset and the cell-side product of any new cell
void doublet_project(const ExprData &D, const std::vector<long long> &len, const long long *parents, long long n_sim, int max_per_slab,
                     double normalize_total, bool lg, const int *genes, int n_genes, const double *mu, const double *w, const double *V, int k,
                     double *Y);
// counts[i] = the entries of row i of idx (rows x K, device) that are >= n_obs
void doublet_neighbor_counts(const int *idx, long long rows, int K, long long n_obs, int *counts);
// table[c] = q rho / r / (1 - rho - q (1 - rho - rho / r)), q = (c + 1) / (k_adj + 2), c = 0 .. k_adj; host
void doublet_score_table(int k_adj, double r, double rho, double *table);

struct DoubletCall {
    double threshold = 0.0;
    bool found = false, have = false;            // found: by the histogram; have: found or given
    double detected = 0.0, detectable = 0.0, overall = 0.0;
    int passes = 0, maxima = 0;                  // smoothing passes run, local maxima left
};
// threshold_in NaN: the minimum between the two modes of the simulated scores' histogram; host
void doublet_threshold(const double *obs, long long n, const double *sim, long long n_sim, double threshold_in, DoubletCall &out,
                       int *predicted);

}  // namespace sharp
