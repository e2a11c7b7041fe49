// diffmap.hpp -- diffusion maps and diffusion pseudotime on the neighbour graph (diffmap.hip): the transition operator
// T = Z^-1/2 K Z^-1/2 applied through its scaling a (never stored), the extraction of one connected component as a CSR of its own,
// the thick-restart Lanczos for the n_comps - 1 largest non-trivial eigenpairs, and the pseudotime of every cell from given roots.
// The C ABI entries (sharp_diffmap*, sharp_dpt; include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include "umap.hpp"

namespace sharp {

constexpr int kDiffmapMaxComps = 64;
constexpr double kDiffmapTol = 1e-6;          // §15's kSpectralTol
constexpr int kDiffmapMaxMatvecs = 4000;      // the default cap on operator applications
constexpr int kDiffmapCheckEvery = 8;         // operator applications between two solves of H on the host
// the columns kept at a restart and the basis' capacity for k = n_comps - 1 wanted pairs
constexpr int diffmap_keep(int k) { return 8 * ((k + k / 2 + 1 + 7) / 8); }
constexpr int diffmap_basis(int k) { return 2 * diffmap_keep(k) + 16; }

// q_i = sum_j W_ij (CSR order); density: z_i = (1 / q_i) sum_j W_ij / q_j, a_i = 1 / (q_i sqrt(z_i)); otherwise z = q, a = 1 / sqrt(q).
// sq (when wanted) = sqrt(z).  An empty row gets z = a = 0.  All n each, on the device.
void diffmap_transitions(const Graph &G, bool density, DevBuf<double> &a, DevBuf<double> &z, DevBuf<double> *sq = nullptr);

struct DiffmapComponent {
    int label = 0;                  // the chosen component, in csr_components' labels (its smallest vertex)
    long long components = 0;
    Graph sub;                      // the component's rows and columns renumbered in ascending order of the old ids
    DevBuf<int> new_id;             // n: the new id of every row, -1 outside the component
};
// root >= 0: root's component; root = -1: the largest, ties to the smallest label
void diffmap_component(const Graph &G, long long root, DiffmapComponent &C);

struct DiffmapSolve {
    int outcome = 0;                // 0 converged, 2 the cap on operator applications was reached
    int steps = 0, restarts = 0;    // operator applications of the recurrence; restarts of the basis
    std::vector<double> theta;      // n_comps: 1, then the Ritz values in descending order
    std::vector<double> residual;   // n_comps: the true ||T v - theta v|| of the returned unit vectors
};
// V: n x n_comps column by column on the device: q0, then the unit Ritz vectors (no sign rule yet)
void diffmap_solve(const Graph &G, int n_comps, bool density, double tol, int max_matvecs, DevBuf<double> &V, DiffmapSolve &R);

}  // namespace sharp
