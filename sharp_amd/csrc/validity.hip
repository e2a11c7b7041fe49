// validity.hip -- what a user does with a tree and with a labelling: stats::cutree on sharp_hclust's merge matrix, cluster::silhouette
// (sildist()) and the Calinski-Harabasz index (R/get_opt_hclust.R:101-105,132-144, there fused into get_opt_hclust's statistics kernels
// on one task of at most 16384 rows; here as entry points of their own, on any labelling of any number of cells).
//   sharp_cutree           host only, no device context: the first n - k merges applied in O(n), ids by first appearance (R_cutree)
//   sil_tile_kernel        the matrix-free silhouette: dist_kernel's pair loop (dist_pairs.hpp: the same functors, the same order of
//                          the features, so a distance here is bitwise sharp_dist's) with an epilogue that reduces every row's distances
//                          per cluster instead of storing them.  The cells are uploaded SORTED by cluster code, so a column tile covers a
//                          contiguous run of clusters; a workgroup owns 64 rows, walks its column tiles in ascending order, keeps the
//                          running sum of the current cluster per row in registers and finishes a cluster's mean at its boundary: a(i), or
//                          a candidate for b(i) taken with a strict <, so the first smallest in cluster-code order wins an exact tie as in
//                          sildist().  No n x n and no n x k array, no atomics: two calls give the same bits.
//                          For small n the clusters (never a part of one) are dealt to several workgroups per row tile; every mean is
//                          still one workgroup's sum in one order, and sil_finish_kernel takes the minimum over the parts in ascending
//                          order, so the result does not depend on the number of parts either.
//   sil_dist_kernel        the same from R's dist vector: one wave per cell, the clusters in ascending order, lanes strided over a
//                          cluster's members (gathered through the sort permutation), a butterfly sum
//   ch_within_kernel       Calinski-Harabasz: the within-cluster sum over all cells (squared Euclidean, or (1 - Pearson r)^2 for
//                          clues::get_CH's "1-corr"), one wave per cell, per-workgroup partial sums added on the host in index order;
//                          the centroids come from cluster_means_kernel (meta.hip)
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "dist_pairs.hpp"
#include "meta.hpp"

namespace sharp {

namespace {

constexpr long long kSilMaxN = 1ll << 24;   // cells of the matrix-free silhouette / the CH index: row indices and cluster offsets are ints, the
                                            // per-part minima take 12 bytes per cell and part
constexpr int kSilMaxParts = 32;            // workgroups per row tile (parts of the cluster range) when the row tiles alone leave CUs idle

// the pair functors of the tile kernel: the four difference metrics as dist_kernel applies them, and 1 - u.v on unit rows
template <class F>
struct PairDiff {
    static __device__ __forceinline__ void acc(double &a, double x, double y, double mp) { F::acc(a, x - y, mp); }
    static __device__ __forceinline__ double fin(double a, double mp) { return F::fin(a, mp); }
};
struct PairCorr {
    static __device__ __forceinline__ void acc(double &a, double x, double y, double) { a = fma(x, y, a); }
    static __device__ __forceinline__ double fin(double a, double) { return 1.0 - fmin(fmax(a, -1.0), 1.0); }   // the GEMM's epilogue 1
};

// sildist(): (b - a) / max(a, b), 0 when a == b or when the cell is alone in its cluster
__device__ __forceinline__ double sil_width(double a, double b, int own_count) {
    return (own_count > 1 && b != a) ? (b - a) / fmax(a, b) : 0.0;
}

// sum over the 16 lanes that share a row of the tile (tx = lane & 15): a butterfly, so every lane ends with the same bits
__device__ __forceinline__ double sum16(double v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 16);
    return v;
}
__device__ __forceinline__ double sum64(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// x: the n cells sorted by cluster, p features each (row-major, ld p).  start[c] .. start[c + 1]: the rows of cluster c (0-based, k + 1
// entries), scl[i]: the cluster of sorted row i.  part_c[s] .. part_c[s + 1]: the clusters of part s = blockIdx.y.
// Outputs per sorted row: A[i] = a(i), written by the part that holds the row's own cluster; PB / PNB[s * n + i]: the smallest mean
// distance to another cluster of part s and that cluster (+inf / -1 when the part holds no other cluster).
template <class P>
__global__ __launch_bounds__(256) void sil_tile_kernel(const double *__restrict__ x, int n, int p, double mp,
                                                       const int *__restrict__ start, const int *__restrict__ scl,
                                                       const int *__restrict__ part_c, double *__restrict__ A, double *__restrict__ PB,
                                                       int *__restrict__ PNB) {
    __shared__ __attribute__((aligned(16))) double sA[DK][DLD];
    __shared__ __attribute__((aligned(16))) double sB[DK][DLD];
    const int i0 = blockIdx.x * DT;
    const int c_first = part_c[blockIdx.y], c_last = part_c[blockIdx.y + 1];
    const int jbeg = start[c_first], jend = start[c_last];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int skk = tid & 31, sr = tid >> 5;
    int row[4], rc[4], nb[4];
    double a_i[4], b_i[4], run[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        row[u] = i0 + ty * 4 + u;
        rc[u] = row[u] < n ? scl[row[u]] : -1;
        nb[u] = -1;
        a_i[u] = 0.0;
        b_i[u] = std::numeric_limits<double>::infinity();
        run[u] = 0.0;
    }
    int cur = c_first, ce = start[c_first + 1], lo = jbeg;
    for (int j0 = jbeg; j0 < jend; j0 += DT) {
        double acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
        for (int k0 = 0; k0 < p; k0 += DK) {
            const int k = k0 + skk;
#pragma unroll
            for (int u = 0; u < DT / 8; ++u) {
                const int r = sr + 8 * u;
                const int gi = i0 + r, gj = j0 + r;
                sA[skk][r] = (gi < n && k < p) ? x[static_cast<long long>(gi) * p + k] : 0.0;
                sB[skk][r] = (gj < n && k < p) ? x[static_cast<long long>(gj) * p + k] : 0.0;
            }
            __syncthreads();
            const int kend = min(DK, p - k0);        // (a feature beyond p would add |0 - 0| or 0 * 0: leaving it out changes no bit)
#pragma unroll 8
            for (int kk = 0; kk < kend; ++kk) {
                const double2 a01 = *reinterpret_cast<const double2 *>(&sA[kk][ty * 4]);
                const double2 a23 = *reinterpret_cast<const double2 *>(&sA[kk][ty * 4 + 2]);
                const double2 b01 = *reinterpret_cast<const double2 *>(&sB[kk][tx * 2]);
                const double2 b23 = *reinterpret_cast<const double2 *>(&sB[kk][32 + tx * 2]);
                const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) P::acc(acc[u][v], a[u], b[v], mp);
            }
            __syncthreads();
        }
        const int col[4] = {j0 + tx * 2, j0 + tx * 2 + 1, j0 + 32 + tx * 2, j0 + 33 + tx * 2};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = P::fin(acc[u][v], mp);
        // the tile's columns belong to the clusters cur, cur + 1, ...: every condition below is uniform over the workgroup
        const int jt_end = min(j0 + DT, jend);
        for (;;) {
            const int hi = min(ce, jt_end);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)         // the diagonal pair (i, i) never contributes
                    run[u] += (col[v] >= lo && col[v] < hi && col[v] != row[u]) ? acc[u][v] : 0.0;
            lo = hi;
            if (ce > jt_end) break;                 // the cluster goes on in the next tile
            const int cnt = ce - start[cur];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double t = sum16(run[u]);
                run[u] = 0.0;
                if (cur == rc[u]) {
                    a_i[u] = cnt > 1 ? t / static_cast<double>(cnt - 1) : 0.0;
                } else {
                    const double m = t / static_cast<double>(cnt);
                    if (m < b_i[u]) { b_i[u] = m; nb[u] = cur; }
                }
            }
            ++cur;
            if (cur >= c_last) break;
            const bool tile_done = ce >= jt_end;
            ce = start[cur + 1];
            if (tile_done) break;
        }
    }
    if (tx == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (row[u] >= n) continue;
            const long long o = static_cast<long long>(blockIdx.y) * n + row[u];
            PB[o] = b_i[u];
            PNB[o] = nb[u];
            if (rc[u] >= c_first && rc[u] < c_last) A[row[u]] = a_i[u];
        }
    }
}

// b(i) = the smallest of the parts' minima, the parts in ascending order of their clusters and a strict <: the first smallest cluster
__global__ __launch_bounds__(256) void sil_finish_kernel(int n, int parts, const int *__restrict__ start, const int *__restrict__ scl,
                                                         const double *__restrict__ A, const double *__restrict__ PB,
                                                         const int *__restrict__ PNB, int *__restrict__ neighbor, double *__restrict__ width) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double b = std::numeric_limits<double>::infinity();
    int nb = -1;
    for (int s = 0; s < parts; ++s) {
        const double m = PB[static_cast<long long>(s) * n + i];
        if (m < b) { b = m; nb = PNB[static_cast<long long>(s) * n + i]; }
    }
    const int c = scl[i];
    neighbor[i] = nb + 1;
    width[i] = sil_width(A[i], b, start[c + 1] - start[c]);
}

// centre a cell's features and scale them to unit norm (cor() of two cells = the dot product of their unit rows); nrm: the norm before
// scaling, 0 for a constant cell.  One thread per cell: O(n p) beside the O(n^2 p) pair loop.
__global__ __launch_bounds__(256) void sil_unit_rows_kernel(double *__restrict__ x, int n, int p, double *__restrict__ nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double *r = x + static_cast<long long>(i) * p;
    double s = 0.0;
    for (int k = 0; k < p; ++k) s += r[k];
    double mean = s / p;
    s = 0.0;
    for (int k = 0; k < p; ++k) s += r[k] - mean;       // cov.c's second pass over the mean
    mean += s / p;
    double ss = 0.0;
    for (int k = 0; k < p; ++k) { const double c = r[k] - mean; ss = fma(c, c, ss); }
    const double nr = sqrt(ss);
    nrm[i] = nr;
    for (int k = 0; k < p; ++k) r[k] = (r[k] - mean) / nr;
}

// sildist() on R's dist vector.  perm[i]: the observation at sorted position i.  One wave per sorted position.
__global__ __launch_bounds__(256) void sil_dist_kernel(const double *__restrict__ cond, int n, int k, const int *__restrict__ start,
                                                       const int *__restrict__ scl, const int *__restrict__ perm,
                                                       int *__restrict__ neighbor, double *__restrict__ width) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;                                  // (whole waves leave; no barrier below)
    const int oi = perm[i], ci = scl[i];
    double a = 0.0, b = std::numeric_limits<double>::infinity();
    int nb = -1;
    for (int c = 0; c < k; ++c) {
        const int s0 = start[c], s1 = start[c + 1];
        double run = 0.0;
        for (int j = s0 + lane; j < s1; j += 64) {
            if (j == i) continue;
            const int oj = perm[j];
            run += cond[cond_index(n, min(oi, oj), max(oi, oj))];
        }
        const double t = sum64(run);
        if (c == ci) {
            a = s1 - s0 > 1 ? t / static_cast<double>(s1 - s0 - 1) : 0.0;
        } else {
            const double m = t / static_cast<double>(s1 - s0);
            if (m < b) { b = m; nb = c; }
        }
    }
    if (lane == 0) {
        neighbor[i] = nb + 1;
        width[i] = sil_width(a, b, start[ci + 1] - start[ci]);
    }
}

// kind 0: sum_k (x_ik - m_k)^2 ; kind 1: (1 - cor(x_i, m))^2, m = the centroid of the cell's cluster.  A wave per cell (lanes strided
// over the features), 64 cells per workgroup; part[blockIdx.x] = the workgroup's sum, its four waves added in order.
template <int KIND>
__global__ __launch_bounds__(256) void ch_within_kernel(const double *__restrict__ x, int n, int p, const int *__restrict__ cl0,
                                                        const double *__restrict__ means, double *__restrict__ part) {
    __shared__ double sw[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double tot = 0.0;
    for (int q = 0; q < 16; ++q) {
        const int i = blockIdx.x * 64 + q * 4 + w;
        if (i >= n) break;
        const double *r = x + static_cast<long long>(i) * p;
        const double *m = means + static_cast<long long>(cl0[i]) * p;
        if (KIND == 0) {
            double s = 0.0;
            for (int k = lane; k < p; k += 64) { const double d = r[k] - m[k]; s = fma(d, d, s); }
            tot += sum64(s);
        } else {
            double sx = 0.0, sm = 0.0;
            for (int k = lane; k < p; k += 64) { sx += r[k]; sm += m[k]; }
            const double mx = sum64(sx) / p, mm = sum64(sm) / p;
            double sxx = 0.0, smm = 0.0, sxm = 0.0;
            for (int k = lane; k < p; k += 64) {
                const double a = r[k] - mx, b = m[k] - mm;
                sxx = fma(a, a, sxx); smm = fma(b, b, smm); sxm = fma(a, b, sxm);
            }
            sxx = sum64(sxx); smm = sum64(smm); sxm = sum64(sxm);
            double rr = sxm / (sqrt(sxx) * sqrt(smm));   // (NaN for a constant cell or centroid, as cor() gives NA)
            rr = rr > 1.0 ? 1.0 : rr < -1.0 ? -1.0 : rr;
            const double d = 1.0 - rr;
            tot += d * d;
        }
    }
    if (lane == 0) sw[w] = tot;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// the cells in cluster order: a stable counting sort of the codes 1 .. k
struct ClusterOrder {
    std::vector<int> start, perm, scl;   // k + 1 offsets; perm[sorted position] = observation; scl[sorted position] = cluster (0-based)
};
void cluster_order(const int *cl, long long n, int k, const char *who, ClusterOrder &o) {
    const std::string w(who);
    SHARP_REQUIRE(cl, w + ": null cluster codes");
    SHARP_REQUIRE(k >= 2 && k <= n - 1, w + ": the number of clusters must be between 2 and n - 1");
    o.start.assign(static_cast<size_t>(k) + 1, 0);
    for (long long i = 0; i < n; ++i) {
        SHARP_REQUIRE(cl[i] >= 1 && cl[i] <= k, w + ": cluster codes must be between 1 and k");
        ++o.start[cl[i]];
    }
    for (int c = 0; c < k; ++c) {
        SHARP_REQUIRE(o.start[c + 1] > 0, w + ": every cluster code 1 .. k must occur");
        o.start[c + 1] += o.start[c];
    }
    o.perm.resize(static_cast<size_t>(n));
    o.scl.resize(static_cast<size_t>(n));
    std::vector<int> fill(o.start.begin(), o.start.end() - 1);
    for (long long i = 0; i < n; ++i) {
        const int q = fill[cl[i] - 1]++;
        o.perm[q] = static_cast<int>(i);
        o.scl[q] = cl[i] - 1;
    }
}

void check_obs(const double *x, long long n, int p, long long ld, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(x, w + ": null x");
    SHARP_REQUIRE(n >= 3 && p >= 1 && ld >= p, w + ": need n >= 3 observations of p >= 1 features (ld >= p)");
    SHARP_REQUIRE(n <= kSilMaxN, w + ": more than 16777216 observations is not supported");
    for (long long i = 0; i < n; ++i)
        for (int k = 0; k < p; ++k) SHARP_REQUIRE(std::isfinite(x[i * ld + k]), w + ": x holds NA / NaN / Inf");
}

// the clusters dealt to at most `want` parts of about equal numbers of cells (never a part of a cluster)
std::vector<int> split_clusters(const std::vector<int> &start, int want) {
    const int k = static_cast<int>(start.size()) - 1, n = start[k];
    std::vector<int> pc{0};
    for (int s = 1; s < want; ++s) {
        const long long target = static_cast<long long>(n) * s / want;
        int c = static_cast<int>(std::lower_bound(start.begin(), start.end(), static_cast<int>(target)) - start.begin());
        if (c > pc.back() && c < k) pc.push_back(c);
    }
    pc.push_back(k);
    return pc;
}

template <class P>
void launch_sil_tile(dim3 grid, const double *x, int n, int p, double mp, const int *start, const int *scl, const int *pc, double *A,
                     double *PB, int *PNB) {
    hipLaunchKernelGGL(sil_tile_kernel<P>, grid, dim3(256), 0, ctx().stream, x, n, p, mp, start, scl, pc, A, PB, PNB);
}

}  // namespace

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_cutree(const int *merge, int n, const int *k, int nk, int *out) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(merge && k && out, "sharp_cutree: null argument");
    SHARP_REQUIRE(n >= 2, "sharp_cutree: invalid 'tree' (merge component)");
    SHARP_REQUIRE(nk >= 1, "sharp_cutree: no k given");
    const int *ma = merge, *mb = merge + (n - 1);
    for (int s = 0; s < n - 1; ++s)
        for (const int v : {ma[s], mb[s]})
            SHARP_REQUIRE(v != 0 && v >= -n && v <= s, "sharp_cutree: invalid 'tree' (merge component)");
    std::vector<int> root(static_cast<size_t>(n)), obs(static_cast<size_t>(n)), id(static_cast<size_t>(n));
    for (int q = 0; q < nk; ++q) {
        SHARP_REQUIRE(k[q] >= 1 && k[q] <= n, "elements of 'k' must be between 1 and " + std::to_string(n));
        const int nm = n - k[q];                     // the first nm merges are applied
        // top down: a step nobody claimed is the root of a cluster; its members inherit it
        std::fill(root.begin(), root.begin() + nm, -1);
        std::fill(obs.begin(), obs.end(), -1);
        for (int s = nm - 1; s >= 0; --s) {
            const int r = root[s] < 0 ? s : root[s];
            for (const int v : {ma[s], mb[s]}) {
                if (v < 0) obs[-v - 1] = r; else root[v - 1] = r;
            }
        }
        std::fill(id.begin(), id.end(), 0);
        int ncl = 0;
        int *lab = out + static_cast<size_t>(q) * n;
        for (int i = 0; i < n; ++i) {                // ids by first appearance in observation order (R_cutree)
            if (obs[i] < 0) { lab[i] = ++ncl; continue; }
            if (!id[obs[i]]) id[obs[i]] = ++ncl;
            lab[i] = id[obs[i]];
        }
    }
    SHARP_API_END
}

int sharp_silhouette_dist(const double *d, int n, const int *cl, int k, int *neighbor, double *width) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    SHARP_REQUIRE(d && neighbor && width, "sharp_silhouette_dist: null argument");
    SHARP_REQUIRE(n >= 3, "sharp_silhouette_dist: need n >= 3 observations");
    SHARP_REQUIRE(n <= SHARP_DIST_MAX_N, "sharp_silhouette_dist: a dist vector of more than 46340 observations is not supported: "
                                         "give the observations themselves (sharp_silhouette)");
    ClusterOrder o;
    cluster_order(cl, n, k, "sharp_silhouette_dist", o);
    const size_t len = static_cast<size_t>(n) * (n - 1) / 2;
    for (size_t e = 0; e < len; ++e) SHARP_REQUIRE(std::isfinite(d[e]), "sharp_silhouette_dist: d holds NA / NaN / Inf");
    DevBuf<double> cond(len), dw(n);
    DevBuf<int> dstart(k + 1), dscl(n), dperm(n), dnb(n);
    cond.upload(d, len);
    dstart.upload(o.start.data(), k + 1);
    dscl.upload(o.scl.data(), n);
    dperm.upload(o.perm.data(), n);
    {
        KernelTimer tm("silhouette_dist");
        hipLaunchKernelGGL(sil_dist_kernel, dim3((n + 3) / 4), dim3(256), 0, c.stream, cond.p, n, k, dstart.p, dscl.p, dperm.p, dnb.p, dw.p);
        launch_check("sil_dist_kernel");
    }
    std::vector<int> hnb(n);
    std::vector<double> hw(n);
    dnb.download(hnb.data(), n);
    dw.download(hw.data(), n);
    for (int q = 0; q < n; ++q) { neighbor[o.perm[q]] = hnb[q]; width[o.perm[q]] = hw[q]; }
    SHARP_API_END
}

int sharp_silhouette(const double *x, long long n, int p, long long ld, int dist_method, double minkowski_p, const int *cl, int k,
                     int *neighbor, double *width) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    SHARP_REQUIRE(neighbor && width, "sharp_silhouette: null output");
    SHARP_REQUIRE(dist_method != 4 && dist_method != 5,
                  "sharp_silhouette: the \"canberra\" and \"binary\" distances are not supported (their NA rules are out of scope)");
    SHARP_REQUIRE(dist_method == 1 || dist_method == 2 || dist_method == 3 || dist_method == 6 || dist_method == 7, "invalid distance method");
    if (dist_method == 6) SHARP_REQUIRE(std::isfinite(minkowski_p) && minkowski_p > 0, "sharp_silhouette: minkowski needs a finite p > 0");
    if (dist_method == 7) SHARP_REQUIRE(p >= 2, "sharp_silhouette: the correlation distance needs at least 2 features");
    check_obs(x, n, p, ld, "sharp_silhouette");
    ClusterOrder o;
    cluster_order(cl, n, k, "sharp_silhouette", o);
    const int ni = static_cast<int>(n);
    // the cells in cluster order, packed
    std::vector<double> xs(static_cast<size_t>(n) * p);
    host_parallel_for(ni, 16, [&](int q) { std::copy(x + o.perm[q] * ld, x + o.perm[q] * ld + p, xs.begin() + static_cast<size_t>(q) * p); });
    const int row_tiles = (ni + DT - 1) / DT;
    const int want = std::max(1, std::min(kSilMaxParts, (4 * c.num_cu + row_tiles - 1) / row_tiles));
    const std::vector<int> pc = split_clusters(o.start, want);
    const int parts = static_cast<int>(pc.size()) - 1;
    DevBuf<double> dx(xs.size()), dA(n), dPB(static_cast<size_t>(parts) * n), dw(n);
    DevBuf<int> dstart(k + 1), dscl(n), dpc(pc.size()), dPNB(static_cast<size_t>(parts) * n), dnb(n);
    dx.upload(xs.data(), xs.size());
    dstart.upload(o.start.data(), k + 1);
    dscl.upload(o.scl.data(), n);
    dpc.upload(pc.data(), pc.size());
    if (dist_method == 7) {
        DevBuf<double> nrm(n);
        {
            KernelTimer tm("silhouette_unit_rows");
            hipLaunchKernelGGL(sil_unit_rows_kernel, dim3((ni + 255) / 256), dim3(256), 0, c.stream, dx.p, ni, p, nrm.p);
            launch_check("sil_unit_rows_kernel");
        }
        std::vector<double> hn(n);
        nrm.download(hn.data(), n);
        for (long long q = 0; q < n; ++q)
            SHARP_REQUIRE(hn[q] > 0 && std::isfinite(hn[q]), "sharp_silhouette: a constant observation has no correlation distance");
    }
    {
        KernelTimer tm("silhouette_tiles");
        const dim3 grid(row_tiles, parts);
        switch (dist_method) {
            case 1: launch_sil_tile<PairDiff<DistEuclid>>(grid, dx.p, ni, p, minkowski_p, dstart.p, dscl.p, dpc.p, dA.p, dPB.p, dPNB.p); break;
            case 2: launch_sil_tile<PairDiff<DistMaximum>>(grid, dx.p, ni, p, minkowski_p, dstart.p, dscl.p, dpc.p, dA.p, dPB.p, dPNB.p); break;
            case 3: launch_sil_tile<PairDiff<DistManhattan>>(grid, dx.p, ni, p, minkowski_p, dstart.p, dscl.p, dpc.p, dA.p, dPB.p, dPNB.p); break;
            case 6: launch_sil_tile<PairDiff<DistMinkowski>>(grid, dx.p, ni, p, minkowski_p, dstart.p, dscl.p, dpc.p, dA.p, dPB.p, dPNB.p); break;
            default: launch_sil_tile<PairCorr>(grid, dx.p, ni, p, minkowski_p, dstart.p, dscl.p, dpc.p, dA.p, dPB.p, dPNB.p); break;
        }
        launch_check("sil_tile_kernel");
    }
    {
        KernelTimer tm("silhouette_finish");
        hipLaunchKernelGGL(sil_finish_kernel, dim3((ni + 255) / 256), dim3(256), 0, c.stream, ni, parts, dstart.p, dscl.p, dA.p, dPB.p, dPNB.p,
                           dnb.p, dw.p);
        launch_check("sil_finish_kernel");
    }
    std::vector<int> hnb(n);
    std::vector<double> hw(n);
    dnb.download(hnb.data(), n);
    dw.download(hw.data(), n);
    for (long long q = 0; q < n; ++q) { neighbor[o.perm[q]] = hnb[q]; width[o.perm[q]] = hw[q]; }
    SHARP_API_END
}

int sharp_calinski_harabasz(const double *x, long long n, int p, long long ld, const int *cl, int k, int kind, double *out) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    SHARP_REQUIRE(out, "sharp_calinski_harabasz: null output");
    SHARP_REQUIRE(kind == 0 || kind == 1, "sharp_calinski_harabasz: kind must be 0 (euclidean) or 1 (1-corr)");
    if (kind == 1) SHARP_REQUIRE(p >= 2, "sharp_calinski_harabasz: the 1-corr form needs at least 2 features");
    check_obs(x, n, p, ld, "sharp_calinski_harabasz");
    ClusterOrder o;                                  // (validates the codes; the counts are start's differences)
    cluster_order(cl, n, k, "sharp_calinski_harabasz", o);
    const int ni = static_cast<int>(n);
    DevBuf<double> dx(static_cast<size_t>(n) * p), dm(static_cast<size_t>(k) * p);
    if (ld == p) dx.upload(x, static_cast<size_t>(n) * p);
    else SHARP_HIP_CHECK(hipMemcpy2DAsync(dx.p, static_cast<size_t>(p) * 8, x, static_cast<size_t>(ld) * 8, static_cast<size_t>(p) * 8,
                                          static_cast<size_t>(n), hipMemcpyHostToDevice, c.stream));
    std::vector<int> cl0(cl, cl + n);
    for (int &v : cl0) --v;
    cluster_means_dev(dx.p, p, ni, p, cl0, k, dm.p);
    DevBuf<int> dcl(n);
    dcl.upload(cl0.data(), n);
    const int blocks = (ni + 63) / 64;
    DevBuf<double> dpart(blocks);
    {
        KernelTimer tm("ch_within");
        if (kind == 0) hipLaunchKernelGGL(ch_within_kernel<0>, dim3(blocks), dim3(256), 0, c.stream, dx.p, ni, p, dcl.p, dm.p, dpart.p);
        else hipLaunchKernelGGL(ch_within_kernel<1>, dim3(blocks), dim3(256), 0, c.stream, dx.p, ni, p, dcl.p, dm.p, dpart.p);
        launch_check("ch_within_kernel");
    }
    std::vector<double> part(blocks), cen(static_cast<size_t>(k) * p);
    dpart.download(part.data(), blocks);
    dm.download(cen.data(), cen.size());
    double W = 0.0;
    for (int b = 0; b < blocks; ++b) W += part[b];
    // the k centroids against the overall mean: O(k p) on the host
    std::vector<double> all(p, 0.0);
    for (int q = 0; q < k; ++q)
        for (int f = 0; f < p; ++f) all[f] += cen[static_cast<size_t>(q) * p + f] * (o.start[q + 1] - o.start[q]);
    for (int f = 0; f < p; ++f) all[f] /= static_cast<double>(n);
    double B = 0.0;
    for (int q = 0; q < k; ++q) {
        const double *m = cen.data() + static_cast<size_t>(q) * p;
        const double cnt = o.start[q + 1] - o.start[q];
        if (kind == 0) {
            double s = 0.0;
            for (int f = 0; f < p; ++f) s += (m[f] - all[f]) * (m[f] - all[f]);
            B += cnt * s;
        } else {
            double mx = 0.0, ma = 0.0;
            for (int f = 0; f < p; ++f) { mx += m[f]; ma += all[f]; }
            mx /= p; ma /= p;
            double sxx = 0.0, saa = 0.0, sxa = 0.0;
            for (int f = 0; f < p; ++f) { const double a = m[f] - mx, b = all[f] - ma; sxx += a * a; saa += b * b; sxa += a * b; }
            double r = sxa / (std::sqrt(sxx) * std::sqrt(saa));
            r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
            B += cnt * (1.0 - r) * (1.0 - r);
        }
    }
    *out = (B / (k - 1)) / (W / static_cast<double>(n - k));
    SHARP_API_END
}

}  // extern "C"
