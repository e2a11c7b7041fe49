// doublets.hip -- Scrublet-style doublet detection from sparse count blocks: DESIGN.md §24 (the specification is the project's own,
// modelled on Wolock, Lopez and Klein 2019; no parity with the scrublet or scanpy packages is claimed).
//   pairs      doublet s has the parents floor(u(s, j) n), j = 0, 1, u from the 64-bit mix that keys Omega: a pure function of (n, n_sim, seed)
//   synthesis  the counts of doublet s are column a_s + column b_s, made from the resident cell-major copy of the observed cells, one
//              wave per doublet, in two passes.  Both parents' gene lists are sorted, so a lane takes an entry of one list (64 at a
//              time) and finds its lower bound in the other by binary search; the entry's place in the union is its own index plus
//              that lower bound minus the matches before it (a ballot and popcount prefix per 64-entry step, carried from step to
//              step).  The count pass counts the union, the scan turns the counts into offsets, the fill pass writes: an entry of a
//              writes the gene and, for a shared gene, the sum; a matched entry of b writes nothing.  No atomic: every entry's place
//              is a function of the two lists.
//   slabs      the doublets are made slab after slab, cut on the host from the parents' stored entries so that a slab's two copies
//              stay within a budget; the whole simulated matrix never exists
//   scores     per slab expr_pca.hip's transform, subset and cell-side product, as for any new cell: the bits of
//              expression_pca_transform on the host-built block A[:, a] + A[:, b]
//   counts     per row of the k-NN lists of (observed, simulated) the neighbours that are simulated: an integer
//   host       the score as a table over that count, the threshold between the two modes of the simulated scores' histogram
#include "doublets.hpp"
#include "graph_prim.hpp"
#include "knn.hpp"
#include "knn_descent.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>

namespace sharp {
namespace {

constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;

// the first position in [b, e) whose gene is >= x (e when none is)
__device__ __forceinline__ long long gene_lower_bound(const int *__restrict__ ridx, long long b, long long e, int x) {
    while (b < e) {
        const long long mid = (b + e) >> 1;
        if (ridx[mid] < x) b = mid + 1; else e = mid;
    }
    return b;
}

// cnt[s] = the genes that parent a or parent b of doublet s stores: |a| + |b| - the entries of a whose gene b stores too
__global__ __launch_bounds__(256) void doublet_count_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx,
                                                            const long long *__restrict__ parents, long long ns, long long *__restrict__ cnt) {
    const long long s = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (s >= ns) return;
    const int lane = threadIdx.x & 63;
    const long long a = parents[2 * s], b = parents[2 * s + 1];
    const long long ab = cptr[a], ae = cptr[a + 1], bb = cptr[b], be = cptr[b + 1];
    int match = 0;
    for (long long p = ab + lane; p < ae; p += 64) {
        const int x = ridx[p];
        const long long q = gene_lower_bound(ridx, bb, be, x);
        match += q < be && ridx[q] == x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) match += __shfl_xor(match, off);
    if (lane == 0) cnt[s] = (ae - ab) + (be - bb) - match;
}

// The entries [sb, se) of one parent into the union that starts at o: entry i goes to o + i + (its lower bound in the other list [ob, oe))
// - (the matched entries before it).  SUM: a matched entry writes the sum of the two values; otherwise a matched entry writes nothing.
template <bool SUM>
__device__ __forceinline__ void doublet_place(const int *__restrict__ ridx, const double *__restrict__ val, long long sb, long long se,
                                              long long ob, long long oe, long long o, int lane, int *__restrict__ ridx_out,
                                              double *__restrict__ val_out) {
    long long before = 0;                                    // the matched entries of the steps behind
    for (long long p0 = sb; p0 < se; p0 += 64) {
        const long long p = p0 + lane;
        const bool act = p < se;
        int x = 0;
        long long q = ob;
        bool hit = false;
        if (act) {
            x = ridx[p];
            q = gene_lower_bound(ridx, ob, oe, x);
            hit = q < oe && ridx[q] == x;
        }
        const u64 hits = __ballot(hit);
        if (act && (SUM || !hit)) {
            const long long at = o + (p - sb) + (q - ob) - (before + __popcll(hits & ((1ull << lane) - 1ull)));
            const double v = val[p];
            ridx_out[at] = x;
            val_out[at] = (SUM && hit) ? v + val[q] : v;
        }
        before += __popcll(hits);
    }
}

// doublet s = column a + column b into [nptr[s], nptr[s + 1]), genes ascending, a shared gene once; lsum_out[s] = L_a + L_b
__global__ __launch_bounds__(256) void doublet_fill_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx,
                                                           const double *__restrict__ val, const double *__restrict__ lsum,
                                                           const long long *__restrict__ parents, long long ns,
                                                           const long long *__restrict__ nptr, int *__restrict__ ridx_out,
                                                           double *__restrict__ val_out, double *__restrict__ lsum_out) {
    const long long s = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (s >= ns) return;
    const int lane = threadIdx.x & 63;
    const long long a = parents[2 * s], b = parents[2 * s + 1];
    const long long ab = cptr[a], ae = cptr[a + 1], bb = cptr[b], be = cptr[b + 1];
    const long long o = nptr[s];
    doublet_place<true>(ridx, val, ab, ae, bb, be, o, lane, ridx_out, val_out);
    doublet_place<false>(ridx, val, bb, be, ab, ae, o, lane, ridx_out, val_out);
    if (lane == 0) lsum_out[s] = lsum[a] + lsum[b];
}

// counts[i] = the entries of row i that are >= n_obs: one wave per row
__global__ __launch_bounds__(256) void doublet_neighbor_count_kernel(const int *__restrict__ idx, long long rows, int K, int n_obs,
                                                                     int *__restrict__ counts) {
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    int c = 0;
    for (int k = lane; k < K; k += 64) c += idx[i * K + k] >= n_obs;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) counts[i] = c;
}

long long round_half_up(double x) { return static_cast<long long>(std::floor(x + 0.5)); }

int k_adj_of(long long nn, long long n, long long n_sim) {
    const double k = std::floor(static_cast<double>(nn) * (1.0 + static_cast<double>(n_sim) / static_cast<double>(n)) + 0.5);
    return k > 2.0e9 ? INT_MAX : static_cast<int>(k);
}

// the local maxima of h: a run of equal values that is higher than the value on either side of it (a missing side counts as lower);
// at[]: the first bin of each run
int local_maxima(const std::vector<double> &h, std::vector<int> &at) {
    at.clear();
    const int nb = static_cast<int>(h.size());
    int i = 0;
    while (i < nb) {
        int j = i;
        while (j + 1 < nb && h[j + 1] == h[i]) ++j;
        const bool up = i == 0 || h[i - 1] < h[i];
        const bool down = j == nb - 1 || h[j + 1] < h[i];
        if (up && down) at.push_back(i);
        i = j + 1;
    }
    return static_cast<int>(at.size());
}

}  // namespace

u64 doublet_seed(const std::string &who, long long seed) {
    SHARP_REQUIRE(seed >= 0 && seed < (1ll << 53), who + ": seed must be a whole number in [0, 2^53)");
    return static_cast<u64>(seed);
}

DoubletPlan doublet_plan(const std::string &who, long long n, double ratio, int n_neighbors) {
    SHARP_REQUIRE(n >= 2, who + ": need at least 2 cells in all");
    SHARP_REQUIRE(n <= kExprMaxN, who + ": need at most 2^31 - 2 cells in all");
    SHARP_REQUIRE(std::isfinite(ratio) && ratio > 0.0, who + ": sim_doublet_ratio must be finite and > 0");
    const double want = std::floor(ratio * static_cast<double>(n) + 0.5);
    SHARP_REQUIRE(want >= 1.0, who + ": sim_doublet_ratio gives fewer than 1 simulated doublet");
    SHARP_REQUIRE(want + static_cast<double>(n) <= static_cast<double>(kExprMaxN),
                  who + ": the observed cells and the simulated doublets must be at most 2^31 - 2 rows in all");
    DoubletPlan P;
    P.n_sim = static_cast<long long>(want);
    const long long cap = std::min<long long>(kDoubletMaxK, n + P.n_sim - 1);
    SHARP_REQUIRE(n_neighbors >= 0, who + ": n_neighbors must be >= 1 (None: the default)");
    if (n_neighbors == 0) {
        long long nn = std::max<long long>(1, round_half_up(0.5 * std::sqrt(static_cast<double>(n))));
        while (nn > 1 && k_adj_of(nn, n, P.n_sim) > cap) --nn;
        P.n_neighbors = static_cast<int>(nn);
    } else {
        P.n_neighbors = n_neighbors;
    }
    P.k_adj = k_adj_of(P.n_neighbors, n, P.n_sim);
    SHARP_REQUIRE(P.k_adj >= 1, who + ": n_neighbors gives k_adj = 0 neighbours per row");
    SHARP_REQUIRE(P.k_adj <= kDoubletMaxK, who + ": n_neighbors = " + std::to_string(P.n_neighbors) + " gives k_adj = round(n_neighbors (1 + n_sim / n)) = " +
                                               std::to_string(P.k_adj) + " neighbours per row; the k-NN stages take at most 255");
    SHARP_REQUIRE(P.k_adj <= n + P.n_sim - 1, who + ": n_neighbors = " + std::to_string(P.n_neighbors) + " gives k_adj = " + std::to_string(P.k_adj) +
                                                  " neighbours per row; there are only n + n_sim - 1 = " + std::to_string(n + P.n_sim - 1) + " other rows");
    return P;
}

void doublet_pairs(long long n, long long n_sim, u64 seed, long long *parents) {
    const double dn = static_cast<double>(n);
    for (long long s = 0; s < n_sim; ++s) {
        const u64 h0 = mix64(seed * kGolden + static_cast<u64>(s));
        for (int j = 0; j < 2; ++j) {
            const double u = static_cast<double>(mix64(h0 + static_cast<u64>(j)) >> 11) * 0x1.0p-53;
            long long p = static_cast<long long>(std::floor(u * dn));
            parents[2 * s + j] = p < n ? p : n - 1;          // (u < 1 and n < 2^31: the product cannot round up to n; a guard all the same)
        }
    }
}

void doublet_check_parents(const std::string &who, const long long *parents, long long n_sim, long long n) {
    for (long long e = 0; e < 2 * n_sim; ++e)
        SHARP_REQUIRE(parents[e] >= 0 && parents[e] < n,
                      who + ": a parent outside [0, n) (doublet " + std::to_string(e / 2) + ", counted from 0)");
}

void doublet_slabs(const ExprData &D, const std::vector<long long> &len, const long long *parents, long long n_sim, int max_per_slab,
                   const std::function<void(long long, ExprData &)> &fn) {
    Ctx &c = ctx();
    size_t free_b = 0, total_b = 0;
    SHARP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    // a slab's entry costs 12 bytes in the merged copy and up to 12 more in the gene subset; a quarter of what is free at the most
    const double budget = std::min(kDoubletSlabBytes, static_cast<double>(free_b) / 4.0);
    const long long max_entries = std::max<long long>(1, static_cast<long long>(budget / 24.0));
    std::vector<long long> cut(1, 0);
    long long acc = 0, held = 0, cap_cells = 0;
    for (long long s = 0; s < n_sim; ++s) {
        const long long ub = len[parents[2 * s]] + len[parents[2 * s + 1]];
        if (held > 0 && (acc + ub > max_entries || (max_per_slab > 0 && held >= max_per_slab) || held >= (1ll << 24))) {
            cut.push_back(s);
            acc = held = 0;
        }
        acc += ub;
        ++held;
        cap_cells = std::max(cap_cells, held);
    }
    cut.push_back(n_sim);
    DevBuf<long long> dpar(2 * cap_cells), cnt(cap_cells + 1);
    Scratch tmp;
    for (size_t q = 0; q + 1 < cut.size(); ++q) {
        const long long s0 = cut[q], ns = cut[q + 1] - s0;
        if (ns == 0) continue;
        ExprData S;
        S.n = ns;
        S.m = S.m_in = D.m;
        S.cptr.alloc(ns + 1);
        S.lsum.alloc(ns);
        dpar.upload(parents + 2 * s0, 2 * ns);
        {
            KernelTimer timer("doublet_count");
            SHARP_HIP_CHECK(hipMemsetAsync(cnt.p + ns, 0, sizeof(long long), c.stream));     // (the scan's extra slot)
            hipLaunchKernelGGL(doublet_count_kernel, dim3(wave_grid(ns)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, dpar.p, ns, cnt.p);
            launch_check("doublet_count_kernel");
        }
        long long total = 0;
        {
            KernelTimer timer("doublet_scan");
            exclusive_scan(cnt.p, S.cptr.p, static_cast<size_t>(ns + 1), tmp);
            SHARP_HIP_CHECK(hipMemcpyAsync(&total, S.cptr.p + ns, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
        }
        stream_sync();
        S.nnz = total;
        S.ridx.alloc(std::max<long long>(total, 1));
        S.t.alloc(std::max<long long>(total, 1));
        {
            KernelTimer timer("doublet_fill");
            hipLaunchKernelGGL(doublet_fill_kernel, dim3(wave_grid(ns)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, D.t.p, D.lsum.p, dpar.p, ns,
                               S.cptr.p, S.ridx.p, S.t.p, S.lsum.p);
            launch_check("doublet_fill_kernel");
        }
        fn(s0, S);
        stream_sync();                                       // (the slab's buffers go; the parents are written again)
    }
}

void doublet_project(const ExprData &D, const std::vector<long long> &len, const long long *parents, long long n_sim, int max_per_slab,
                     double normalize_total, bool lg, const int *genes, int n_genes, const double *mu, const double *w, const double *V, int k,
                     double *Y) {
    doublet_slabs(D, len, parents, n_sim, max_per_slab, [&](long long s0, ExprData &S) {
        {
            KernelTimer timer("doublet_transform");
            expr_transform(S, normalize_total, lg);
            if (genes) expr_subset(S, genes, n_genes);
        }
        KernelTimer timer("doublet_product");
        expr_spmm_cells(S, mu, w, V, k, Y + s0 * k);
    });
}

void doublet_neighbor_counts(const int *idx, long long rows, int K, long long n_obs, int *counts) {
    KernelTimer timer("doublet_neighbor_counts");
    hipLaunchKernelGGL(doublet_neighbor_count_kernel, dim3(wave_grid(rows)), dim3(256), 0, ctx().stream, idx, rows, K, static_cast<int>(n_obs),
                       counts);
    launch_check("doublet_neighbor_count_kernel");
}

void doublet_score_table(int k_adj, double r, double rho, double *table) {
    const double u = rho / r;
    const double one = 1.0 - rho;
    const double v = one - u;
    for (int c = 0; c <= k_adj; ++c) {
        const double q = (static_cast<double>(c) + 1.0) / (static_cast<double>(k_adj) + 2.0);
        const double num = (q * rho) / r;
        const double den = one - q * v;
        table[c] = num / den;
    }
}

void doublet_threshold(const double *obs, long long n, const double *sim, long long n_sim, double threshold_in, DoubletCall &out, int *predicted) {
    out = DoubletCall();
    if (!std::isnan(threshold_in)) {
        out.threshold = threshold_in;
        out.have = true;
    } else {
        double mn = sim[0], mx = sim[0];
        for (long long s = 1; s < n_sim; ++s) { mn = std::min(mn, sim[s]); mx = std::max(mx, sim[s]); }
        const double width = mx - mn;
        if (width > 0.0) {
            std::vector<double> h(kDoubletBins, 0.0), g(kDoubletBins);
            for (long long s = 0; s < n_sim; ++s) {
                int b = static_cast<int>(std::floor((sim[s] - mn) / width * static_cast<double>(kDoubletBins)));
                b = b < 0 ? 0 : (b >= kDoubletBins ? kDoubletBins - 1 : b);
                h[b] += 1.0;
            }
            std::vector<int> at;
            int nmax = local_maxima(h, at);
            while (nmax > 2 && out.passes < kDoubletMaxSmooth) {
                for (int i = 0; i < kDoubletBins; ++i) {
                    const double lo = h[i == 0 ? 1 : i - 1], hi = h[i == kDoubletBins - 1 ? kDoubletBins - 2 : i + 1];
                    g[i] = ((lo + h[i]) + hi) / 3.0;
                }
                h.swap(g);
                ++out.passes;
                nmax = local_maxima(h, at);
            }
            out.maxima = nmax;
            if (nmax == 2) {
                int best = at[0];
                for (int i = at[0]; i <= at[1]; ++i)
                    if (h[i] < h[best]) best = i;
                out.threshold = mn + ((static_cast<double>(best) + 0.5) * width) / static_cast<double>(kDoubletBins);
                out.found = out.have = true;
            }
        } else {
            out.maxima = 1;
        }
    }
    if (!out.have) return;
    long long above = 0, above_sim = 0;
    for (long long i = 0; i < n; ++i) {
        const int p = obs[i] > out.threshold;
        if (predicted) predicted[i] = p;
        above += p;
    }
    for (long long s = 0; s < n_sim; ++s) above_sim += sim[s] > out.threshold;
    out.detected = static_cast<double>(above) / static_cast<double>(n);
    out.detectable = static_cast<double>(above_sim) / static_cast<double>(n_sim);
    out.overall = above_sim > 0 ? out.detected / out.detectable : 0.0;
}

namespace {

// the refusals of the block list that need no device, before anything is allocated: the cells in all, and every stored value finite
// and not negative; len[c] = the stored entries of cell c
long long check_counts(const std::string &who, const ExprBlocks &B, std::vector<long long> &len) {
    expr_check_options(who, 0.0, B.m);
    const long long n = expr_total_cells(who, B);
    len.assign(static_cast<size_t>(n), 0);
    long long c0 = 0;
    for (int b = 0; b < B.nblocks; ++b) {
        const int *p = B.colptr[b];
        SHARP_REQUIRE(p && p[0] == 0, who + ": block " + std::to_string(b + 1) + ": colptr must start at 0");
        for (long long c = 0; c < B.ncb[b]; ++c) {
            SHARP_REQUIRE(p[c + 1] >= p[c], who + ": colptr decreases (cell " + std::to_string(c0 + c) + ", counted from 0)");
            len[c0 + c] = p[c + 1] - p[c];
        }
        const long long cnt = p[B.ncb[b]];
        SHARP_REQUIRE(cnt == 0 || (B.rowidx[b] && B.val[b]), who + ": block " + std::to_string(b + 1) + ": null rowidx / val");
        long long c = 0;
        for (long long e = 0; e < cnt; ++e) {
            const double v = B.val[b][e];
            if (std::isfinite(v) && v >= 0.0) continue;
            while (p[c + 1] <= e) ++c;
            throw Error(SHARP_ERR_ARG, who + (std::isfinite(v) ? ": a negative value where counts are expected" : ": a value that is NaN or infinite") +
                                           " (cell " + std::to_string(c0 + c) + ", counted from 0)");
        }
        c0 += B.ncb[b];
    }
    return n;
}

// the observed cells' raw counts on the device
void load_counts(const std::string &who, const ExprBlocks &B, int l_work, ExprData &D) {
    ExprExtra extra;
    extra.refuse_negative = true;
    expr_load(who, B, 0.0, false, false, false, l_work, 2, D, extra);
}

// a fit's centre and scale as the cell-side product takes them (expression_pca_transform's check and weights)
void fit_weights(const std::string &who, const double *center, const double *scale, int mk, std::vector<double> &wt) {
    wt.resize(mk);
    for (int g = 0; g < mk; ++g) {
        SHARP_REQUIRE(std::isfinite(scale[g]) && scale[g] > 0.0 && std::isfinite(center[g]),
                      who + ": the fit's scale must be positive and its center finite (gene " + std::to_string(g) + ", counted from 0)");
        wt[g] = 1.0 / scale[g];
    }
}

void pass(int rc) {
    if (rc != SHARP_OK) throw Error(rc, sharp_last_error());
}

}  // namespace
}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_doublet_plan(long long n, double sim_doublet_ratio, int n_neighbors, long long *n_sim, int *n_neighbors_out, int *k_adj) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(n_sim && n_neighbors_out && k_adj, "scrublet: null output");
    const DoubletPlan P = doublet_plan("scrublet", n, sim_doublet_ratio, n_neighbors);
    *n_sim = P.n_sim;
    *n_neighbors_out = P.n_neighbors;
    *k_adj = P.k_adj;
    SHARP_API_END
}

int sharp_doublet_pairs(long long n, long long n_sim, long long seed, long long *parents) {
    SHARP_API_BEGIN
    const std::string w("doublet_pairs");
    SHARP_REQUIRE(parents, w + ": null output");
    SHARP_REQUIRE(n >= 1 && n <= kExprMaxN, w + ": need 1 <= n <= 2^31 - 2 cells");
    SHARP_REQUIRE(n_sim >= 1 && n_sim <= kExprMaxN, w + ": need 1 <= n_sim <= 2^31 - 2 doublets");
    doublet_pairs(n, n_sim, doublet_seed(w, seed), parents);
    SHARP_API_END
}

int sharp_doublet_synth_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                            int m, const long long *parents, long long n_sim, int max_doublets_per_slab, long long capacity,
                            long long *colptr_out, int *rowidx_out, double *val_out, double *cell_sum_out) {
    SHARP_API_BEGIN
    const std::string w("simulate_doublets");
    SHARP_REQUIRE(parents && colptr_out && rowidx_out && val_out, w + ": null parents / output");
    SHARP_REQUIRE(n_sim >= 1 && n_sim <= kExprMaxN, w + ": need 1 <= n_sim <= 2^31 - 2 doublets");
    SHARP_REQUIRE(max_doublets_per_slab >= 0, w + ": max_doublets_per_slab must be >= 0");
    SHARP_REQUIRE(capacity >= 0, w + ": capacity must be >= 0");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    std::vector<long long> len;
    const long long n = check_counts(w, B, len);
    SHARP_REQUIRE(n >= 1, w + ": need at least 1 cell in all");
    doublet_check_parents(w, parents, n_sim, n);
    ctx();
    ExprData D;
    ExprExtra extra;
    extra.refuse_negative = true;
    expr_load(w, B, 0.0, false, false, false, 0, 1, D, extra);
    long long at = 0;
    colptr_out[0] = 0;
    doublet_slabs(D, len, parents, n_sim, max_doublets_per_slab, [&](long long s0, ExprData &S) {
        SHARP_REQUIRE(at + S.nnz <= capacity, w + ": the doublets hold more stored entries than the capacity of rowidx / val (" +
                                                  std::to_string(capacity) + "); the parents' entries added up always suffice");
        std::vector<long long> cp(static_cast<size_t>(S.n) + 1);
        S.cptr.download(cp.data(), cp.size());
        for (long long s = 0; s < S.n; ++s) colptr_out[s0 + s + 1] = at + cp[s + 1];
        if (S.nnz) {
            S.ridx.download(rowidx_out + at, static_cast<size_t>(S.nnz));
            S.t.download(val_out + at, static_cast<size_t>(S.nnz));
        }
        if (cell_sum_out) S.lsum.download(cell_sum_out + s0, static_cast<size_t>(S.n));
        at += S.nnz;
    });
    SHARP_API_END
}

int sharp_doublet_project_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                              int m, const long long *parents, long long n_sim, double normalize_total, int log1p, const double *loadings,
                              const double *center, const double *scale, int n_components, const int *genes, int n_genes,
                              int max_doublets_per_slab, double *scores) {
    SHARP_API_BEGIN
    const std::string w("doublet_project");
    SHARP_REQUIRE(parents && loadings && center && scale && scores, w + ": null parents / loadings / center / scale / scores");
    SHARP_REQUIRE(n_sim >= 1 && n_sim <= kExprMaxN, w + ": need 1 <= n_sim <= 2^31 - 2 doublets");
    SHARP_REQUIRE(max_doublets_per_slab >= 0, w + ": max_doublets_per_slab must be >= 0");
    SHARP_REQUIRE(n_components >= 1 && n_components <= kExprMaxL, w + ": need 1 <= n_components <= 128");
    expr_check_options(w, normalize_total, m);
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    std::vector<long long> len;
    const long long n = check_counts(w, B, len);
    SHARP_REQUIRE(n >= 1, w + ": need at least 1 cell in all");
    doublet_check_parents(w, parents, n_sim, n);
    const int mk = expr_check_genes(w, genes, n_genes, m);
    std::vector<double> wt;
    fit_weights(w, center, scale, mk, wt);
    ctx();
    ExprData D;
    ExprExtra extra;
    extra.refuse_negative = true;
    expr_load(w, B, 0.0, false, false, false, n_components, 1, D, extra);
    const int k = n_components;
    DevBuf<double> V(static_cast<size_t>(mk) * k), mu(mk), dw(mk), Y(static_cast<size_t>(n_sim) * k);
    V.upload(loadings, V.n);
    mu.upload(center, mk);
    dw.upload(wt.data(), mk);
    doublet_project(D, len, parents, n_sim, max_doublets_per_slab, normalize_total, log1p != 0, genes, n_genes, mu.p, dw.p, V.p, k, Y.p);
    Y.download(scores, Y.n);
    SHARP_API_END
}

int sharp_doublet_neighbor_counts(const int *index, long long rows, int K, long long n_obs, int *counts) {
    SHARP_API_BEGIN
    const std::string w("doublet_neighbor_counts");
    SHARP_REQUIRE(index && counts, w + ": null index / counts");
    SHARP_REQUIRE(rows >= 1 && rows <= kExprMaxN, w + ": need 1 <= rows <= 2^31 - 2");
    SHARP_REQUIRE(K >= 1 && K <= kDoubletMaxK, w + ": K must be in 1 .. 255");
    SHARP_REQUIRE(n_obs >= 0 && n_obs <= rows, w + ": need 0 <= n_obs <= rows");
    ctx();
    DevBuf<int> di(static_cast<size_t>(rows) * K), dc(rows);
    di.upload(index, di.n);
    doublet_neighbor_counts(di.p, rows, K, n_obs, dc.p);
    dc.download(counts, dc.n);
    SHARP_API_END
}

int sharp_doublet_score_table(int k_adj, double r, double expected_doublet_rate, double *table) {
    SHARP_API_BEGIN
    const std::string w("doublet_score_table");
    SHARP_REQUIRE(table, w + ": null output");
    SHARP_REQUIRE(k_adj >= 1 && k_adj <= kDoubletMaxK, w + ": k_adj must be in 1 .. 255");
    SHARP_REQUIRE(std::isfinite(r) && r > 0.0, w + ": r = n_sim / n must be finite and > 0");
    SHARP_REQUIRE(expected_doublet_rate > 0.0 && expected_doublet_rate < 1.0, w + ": expected_doublet_rate must lie in (0, 1)");
    doublet_score_table(k_adj, r, expected_doublet_rate, table);
    SHARP_API_END
}

int sharp_doublet_threshold(const double *scores_obs, long long n, const double *scores_sim, long long n_sim, double threshold_in,
                            double *threshold, int *found, int *predicted, double *rates, int *passes) {
    SHARP_API_BEGIN
    const std::string w("doublet_threshold");
    SHARP_REQUIRE(scores_obs && scores_sim && threshold && found && predicted && rates, w + ": null input / output");
    SHARP_REQUIRE(n >= 1 && n_sim >= 1, w + ": need at least one observed and one simulated score");
    for (long long i = 0; i < n; ++i) SHARP_REQUIRE(std::isfinite(scores_obs[i]), w + ": a score that is NaN or infinite");
    for (long long s = 0; s < n_sim; ++s) SHARP_REQUIRE(std::isfinite(scores_sim[s]), w + ": a score that is NaN or infinite");
    SHARP_REQUIRE(!std::isinf(threshold_in), w + ": threshold must be finite (NaN: find it)");
    DoubletCall R;
    doublet_threshold(scores_obs, n, scores_sim, n_sim, threshold_in, R, predicted);
    *threshold = R.have ? R.threshold : std::numeric_limits<double>::quiet_NaN();
    *found = R.found ? 1 : 0;
    rates[0] = R.detected; rates[1] = R.detectable; rates[2] = R.overall;
    if (passes) *passes = R.passes;
    SHARP_API_END
}

int sharp_scrublet_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                       double sim_doublet_ratio, double expected_doublet_rate, int n_neighbors, int n_prin_comps, int n_top_genes,
                       const int *genes, int n_genes, const double *fit_scores, const double *fit_loadings, const double *fit_center,
                       const double *fit_scale, double normalize_total, int log1p, int scale, double threshold, int nn_method,
                       const double *nn_args, long long seed, int max_doublets_per_slab, double *doublet_scores, double *doublet_scores_sim,
                       int *predicted, double *threshold_out, int *threshold_found, double *rates, int *n_neighbors_out, int *k_adj_out,
                       long long *parents, int *genes_out, int *n_genes_out, int *neighbor_counts, double *sim_pca) {
    SHARP_API_BEGIN
    const std::string w("scrublet");
    SHARP_REQUIRE(doublet_scores && doublet_scores_sim && predicted && threshold_out && threshold_found && rates && n_neighbors_out && k_adj_out &&
                      parents && genes_out && n_genes_out && neighbor_counts,
                  w + ": null output");
    const bool have_fit = fit_scores || fit_loadings || fit_center || fit_scale;
    SHARP_REQUIRE(!have_fit || (fit_scores && fit_loadings && fit_center && fit_scale), w + ": a fit needs scores, loadings, center and scale");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    std::vector<long long> len;
    expr_check_options(w, normalize_total, m);
    const long long n = check_counts(w, B, len);
    const DoubletPlan P = doublet_plan(w, n, sim_doublet_ratio, n_neighbors);
    SHARP_REQUIRE(expected_doublet_rate > 0.0 && expected_doublet_rate < 1.0, w + ": expected_doublet_rate must lie in (0, 1)");
    const u64 sd = doublet_seed(w, seed);
    SHARP_REQUIRE(!std::isinf(threshold), w + ": threshold must be finite");
    SHARP_REQUIRE(nn_method == 0 || nn_method == 1, w + ": nn_method must be 0 (exact) or 1 (descent)");
    SHARP_REQUIRE(max_doublets_per_slab >= 0, w + ": max_doublets_per_slab must be >= 0");
    SHARP_REQUIRE(n_prin_comps >= 1 && n_prin_comps <= kExprMaxL, w + ": need 1 <= n_prin_comps <= 128");
    SHARP_REQUIRE(have_fit || genes || n_top_genes >= 1, w + ": n_top_genes must be >= 1");
    int mk = expr_check_genes(w, genes, n_genes, m);
    const long long n_sim = P.n_sim, N = n + n_sim;
    const int k = n_prin_comps, K = P.k_adj;
    ctx();
    doublet_pairs(n, n_sim, sd, parents);
    // the fit: the caller's, or variable genes and the sparse PCA of the observed cells through the entries a caller would use
    std::vector<int> gsel;
    std::vector<double> f_scores, f_load, f_mu, f_sd;
    if (!have_fit) {
        if (!genes) {
            std::vector<double> a(m), b(m), cc(m), d(m);
            std::vector<int> rank(m), hv(m);
            gsel.resize(std::min(n_top_genes, m));
            int ns = 0, q = 0, dc[3];
            pass(sharp_expr_hvg_csc(colptr, rowidx, val, ncb, nblocks, m, n_top_genes, 0.3, a.data(), b.data(), cc.data(), d.data(), rank.data(),
                                    hv.data(), gsel.data(), &ns, &q, dc));
            gsel.resize(ns);
            genes = gsel.data();
            n_genes = ns;
            mk = expr_check_genes(w, genes, n_genes, m);
        }
        f_scores.resize(static_cast<size_t>(n) * k);
        f_load.resize(static_cast<size_t>(mk) * k);
        f_mu.resize(mk);
        f_sd.resize(mk);
        std::vector<double> sv(k), sdev(k), gv(mk);
        double tv = 0.0;
        pass(sharp_expr_pca_sub_csc(colptr, rowidx, val, ncb, nblocks, m, k, 10, 4, normalize_total, log1p, scale, 0, f_scores.data(), f_load.data(),
                                    sv.data(), sdev.data(), f_mu.data(), f_sd.data(), gv.data(), &tv, genes, n_genes));
        fit_scores = f_scores.data();
        fit_loadings = f_load.data();
        fit_center = f_mu.data();
        fit_scale = f_sd.data();
    }
    *n_genes_out = genes ? n_genes : 0;
    for (int g = 0; genes && g < n_genes; ++g) genes_out[g] = genes[g];
    std::vector<double> wt;
    fit_weights(w, fit_center, fit_scale, mk, wt);
    DevBuf<double> Y(static_cast<size_t>(N) * k);
    Y.upload(fit_scores, static_cast<size_t>(n) * k);
    {
        ExprData D;
        load_counts(w, B, k, D);
        DevBuf<double> V(static_cast<size_t>(mk) * k), mu(mk), dw(mk);
        V.upload(fit_loadings, V.n);
        mu.upload(fit_center, mk);
        dw.upload(wt.data(), mk);
        doublet_project(D, len, parents, n_sim, max_doublets_per_slab, normalize_total, log1p != 0, genes, n_genes, mu.p, dw.p, V.p, k,
                        Y.p + n * k);
        stream_sync();                                       // (the counts and the fit leave the device before the k-NN)
    }
    if (sim_pca) {
        SHARP_HIP_CHECK(hipMemcpyAsync(sim_pca, Y.p + n * k, static_cast<size_t>(n_sim) * k * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        stream_sync();
    }
    DevBuf<int> idx, counts(N);
    {
        DevBuf<double> dist;
        if (nn_method == 0) {
            KernelTimer timer("doublet_knn");
            knn_self("scrublet", Y.p, N, k, K, idx, dist);
        } else {
            const double *a = nn_args;
            const int n_proj = a ? static_cast<int>(a[0]) : 8, cand = a ? static_cast<int>(a[1]) : 0, iters = a ? static_cast<int>(a[2]) : 12;
            const double delta = a ? a[3] : 0.001, dseed = a ? a[4] : 10.0;
            SHARP_REQUIRE(n_proj >= 1 && n_proj <= 32, w + ": nn_args: n_projections must be in 1 .. 32");
            SHARP_REQUIRE(cand >= 0 && cand <= 255, w + ": nn_args: max_candidates must be in 1 .. 255 (0: min(K, 30))");
            SHARP_REQUIRE(iters >= 0, w + ": nn_args: n_iters must be >= 0");
            SHARP_REQUIRE(std::isfinite(delta) && delta >= 0.0 && delta <= 1.0, w + ": nn_args: delta must be in [0, 1]");
            SHARP_REQUIRE(dseed >= 0.0 && dseed < 0x1.0p53 && dseed == std::floor(dseed), w + ": nn_args: seed must be a whole number in [0, 2^53)");
            KernelTimer timer("doublet_knn");
            KnnDescentInfo info;
            knn_descent(Y.p, N, k, K, n_proj, cand, iters, delta, static_cast<u64>(dseed), idx, dist, info);
        }
        doublet_neighbor_counts(idx.p, N, K, n, counts.p);
        counts.download(neighbor_counts, static_cast<size_t>(N));
    }
    std::vector<double> table(K + 1);
    doublet_score_table(K, static_cast<double>(n_sim) / static_cast<double>(n), expected_doublet_rate, table.data());
    for (long long i = 0; i < n; ++i) doublet_scores[i] = table[neighbor_counts[i]];
    for (long long s = 0; s < n_sim; ++s) doublet_scores_sim[s] = table[neighbor_counts[n + s]];
    DoubletCall R;
    doublet_threshold(doublet_scores, n, doublet_scores_sim, n_sim, threshold, R, predicted);
    *threshold_out = R.have ? R.threshold : std::numeric_limits<double>::quiet_NaN();
    *threshold_found = R.found ? 1 : 0;
    rates[0] = R.detected; rates[1] = R.detectable; rates[2] = R.overall;
    *n_neighbors_out = P.n_neighbors;
    *k_adj_out = K;
    SHARP_API_END
}

}  // extern "C"
