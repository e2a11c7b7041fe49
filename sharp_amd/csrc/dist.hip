// dist.hip -- stats::dist on the GPU and stats::hclust as a tree (merge / height / order): what pheatmap computes inside the reference's
// plot_markers (R/plot_markers.R:214-237: cluster_rows = T, cluster_cols = T, clustering_method = "ward.D") over up to ~10 000 cells.
//   dist_kernel        the four difference metrics of R's dist() (euclidean, maximum, manhattan, minkowski): every pair is computed from
//                      the differences x_ik - x_jk, accumulated in fp64 in the fixed order k = 0 .. p - 1, so that duplicate rows are at
//                      distance exactly 0 and copies of a row have bitwise equal distances to every third row (R's dist has both
//                      properties; the agglomeration's tie order depends on them; ||x||^2 + ||y||^2 - 2 x.y has neither)
//   "correlation"      as.dist(1 - cor(t(x))) (pheatmap's clustering_distance = "correlation"): the row preparation and fp64-MFMA GEMM of
//                      get_opt_hclust (linalg.hip)
//   condense / expand  R's dist vector (column-wise lower triangle) <-> the full symmetric nld x nld matrix the agglomeration reads
//                      (hclust_tree, hclust.hip: one distance task through the chunk pipeline, the kernels of hclust_agglo.hip)
//   HCASS2             hclust.f's conversion of the (ia, ib) merge list into R's merge matrix and leaf order, on the host (n <= 16384)
#include <algorithm>
#include <cmath>
#include <vector>

#include "dist_pairs.hpp"
#include "hclust.hpp"
#include "linalg.hpp"

namespace sharp {

namespace {

// One workgroup per DT x DT tile of the full matrix (both triangles: |a - b| and (a - b)^2 are exactly symmetric, so the two copies of
// a pair agree bitwise without a mirrored store).  The k-major LDS panels sA[k][row] / sB[k][col] are read as 16-byte vectors: a lane's
// four rows are contiguous (four distinct addresses per wave, broadcast), its columns are two pairs 32 apart so that the sixteen lanes
// of a row group read, and later store, 256 contiguous bytes.  Every element of the nld x nld matrix is written (padding: 0).
template <class F>
__global__ __launch_bounds__(256) void dist_kernel(const double *__restrict__ x, int n, int p, long long ld, double mp,
                                                   double *__restrict__ D, int nld) {
    __shared__ __attribute__((aligned(16))) double sA[DK][DLD];
    __shared__ __attribute__((aligned(16))) double sB[DK][DLD];
    const int i0 = blockIdx.y * DT, j0 = blockIdx.x * DT;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    const int skk = tid & 31, sr = tid >> 5;
    for (int k0 = 0; k0 < p; k0 += DK) {
        const int k = k0 + skk;
#pragma unroll
        for (int u = 0; u < DT / 8; ++u) {
            const int r = sr + 8 * u;
            const int gi = i0 + r, gj = j0 + r;
            sA[skk][r] = (gi < n && k < p) ? x[static_cast<long long>(gi) * ld + k] : 0.0;
            sB[skk][r] = (gj < n && k < p) ? x[static_cast<long long>(gj) * ld + k] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < DK; ++kk) {            // (features beyond p are 0 in both panels: they add |0 - 0|)
            const double2 a01 = *reinterpret_cast<const double2 *>(&sA[kk][ty * 4]);
            const double2 a23 = *reinterpret_cast<const double2 *>(&sA[kk][ty * 4 + 2]);
            const double2 b01 = *reinterpret_cast<const double2 *>(&sB[kk][tx * 2]);
            const double2 b23 = *reinterpret_cast<const double2 *>(&sB[kk][32 + tx * 2]);
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) F::acc(acc[u][v], a[u] - b[v], mp);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int row = i0 + ty * 4 + u;             // < nld: the grid is nld / DT tiles each way
        double *drow = D + static_cast<long long>(row) * nld;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = j0 + 32 * h + tx * 2;
            double2 o;
            o.x = (row < n && col < n && row != col) ? F::fin(acc[u][2 * h], mp) : 0.0;
            o.y = (row < n && col + 1 < n && row != col + 1) ? F::fin(acc[u][2 * h + 1], mp) : 0.0;
            *reinterpret_cast<double2 *>(drow + col) = o;
        }
    }
}

// cond <- the upper-triangle entries of row blockIdx.y (contiguous in the matrix and in the vector)
__global__ __launch_bounds__(256) void dist_condense_kernel(const double *__restrict__ D, int n, int nld, double *__restrict__ cond) {
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c > r && c < n) cond[cond_index(n, r, c)] = D[static_cast<long long>(r) * nld + c];
}
__global__ __launch_bounds__(256) void dist_expand_kernel(const double *__restrict__ cond, int n, int nld, double *__restrict__ D) {
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nld) return;
    double v = 0.0;
    if (r < n && c < n && r != c) v = cond[r < c ? cond_index(n, r, c) : cond_index(n, c, r)];
    D[static_cast<long long>(r) * nld + c] = v;
}

inline int rup128(int n) { return (n + 127) / 128 * 128; }

// R's dist(): method codes of its C code (1 euclidean, 2 maximum, 3 manhattan, 4 canberra, 5 binary, 6 minkowski) + 7 correlation
void check_dist_args(const double *x, int n, int p, long long ld, int method, double mp, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(x, w + ": null x");
    SHARP_REQUIRE(n >= 2 && p >= 1 && ld >= p, w + ": need n >= 2 observations of p >= 1 features (ld >= p)");
    SHARP_REQUIRE(method != 4 && method != 5, w + ": the \"canberra\" and \"binary\" distances are not supported (their NA rules are out of scope)");
    SHARP_REQUIRE(method == 1 || method == 2 || method == 3 || method == 6 || method == 7, "invalid distance method");
    if (method == 6) SHARP_REQUIRE(std::isfinite(mp) && mp > 0, "dist: minkowski needs a finite p > 0");
    if (method == 7) SHARP_REQUIRE(p >= 2, w + ": the correlation distance needs at least 2 features");
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < p; ++k)
            SHARP_REQUIRE(std::isfinite(x[static_cast<long long>(i) * ld + k]), w + ": x holds NA / NaN / Inf");
}

// the full symmetric nld x nld distance matrix of the host observations x, in device memory
void dist_full(const double *x, int n, int p, long long ld, int method, double mp, DevBuf<double> &D) {
    Ctx &c = ctx();
    const int nld = rup128(n);
    DevBuf<double> dx(static_cast<size_t>(n) * p);
    if (ld == p) dx.upload(x, static_cast<size_t>(n) * p);
    else SHARP_HIP_CHECK(hipMemcpy2DAsync(dx.p, static_cast<size_t>(p) * 8, x, static_cast<size_t>(ld) * 8, static_cast<size_t>(p) * 8, n,
                                          hipMemcpyHostToDevice, c.stream));
    D.alloc(static_cast<size_t>(nld) * nld);
    if (method == 7) {
        const int p_pad = (p + 15) / 16 * 16;
        DevBuf<double> Cr(static_cast<size_t>(n) * p), Ct(static_cast<size_t>(p_pad) * nld), nrm(n);
        DevBuf<RowPrepTask> dprep(1);
        DevBuf<GemmTask> dg(1);
        const RowPrepTask prep{dx.p, p, n, p, nld, p_pad, 0, Cr.p, Ct.p, nrm.p, D.p};
        const GemmTask g{Ct.p, Ct.p, D.p, n, n, p, nld, nld, nld, 1, 1, 1};
        dprep.upload(&prep, 1);
        dg.upload(&g, 1);
        D.zero();
        row_prep_batched(dprep.p, 1, n, p, false);
        gemm_tn_f64_batched(dg.p, 1, n, n, "corr_dist_gemm", true, true);
        stream_sync();
        return;
    }
    KernelTimer tm("dist");
    const dim3 grid(nld / DT, nld / DT), block(256);
    switch (method) {
        case 1: hipLaunchKernelGGL(dist_kernel<DistEuclid>, grid, block, 0, c.stream, dx.p, n, p, static_cast<long long>(p), mp, D.p, nld); break;
        case 2: hipLaunchKernelGGL(dist_kernel<DistMaximum>, grid, block, 0, c.stream, dx.p, n, p, static_cast<long long>(p), mp, D.p, nld); break;
        case 3: hipLaunchKernelGGL(dist_kernel<DistManhattan>, grid, block, 0, c.stream, dx.p, n, p, static_cast<long long>(p), mp, D.p, nld); break;
        default: hipLaunchKernelGGL(dist_kernel<DistMinkowski>, grid, block, 0, c.stream, dx.p, n, p, static_cast<long long>(p), mp, D.p, nld); break;
    }
    launch_check("dist_kernel");
    stream_sync();      // (dx goes out of scope)
}

// hclust.f's HCASS2: (ia, ib) in observation representatives -> R's merge (singletons negative, earlier steps positive; a singleton
// before a cluster, two clusters in ascending order) and the leaf order (left-to-right expansion of the last step).
// merge: (n - 1) x 2 column-major as R holds it.
void hcass2(int n, const int *ia, const int *ib, int *merge, int *order) {
    int *iia = merge, *iib = merge + (n - 1);
    std::vector<int> last(n + 1, 0);                  // the step (1-based) that last produced the cluster a representative stands for
    for (int i = 0; i < n - 1; ++i) {
        const int a = ia[i], b = ib[i];
        int va = last[a] ? last[a] : -a, vb = last[b] ? last[b] : -b;
        last[std::min(a, b)] = i + 1;
        if (va > 0 && vb < 0) std::swap(va, vb);
        if (va > 0 && vb > 0 && va > vb) std::swap(va, vb);
        iia[i] = va; iib[i] = vb;
    }
    std::vector<int> stack;
    stack.reserve(64);
    stack.push_back(n - 1);
    int loc = 0;
    while (!stack.empty()) {
        const int v = stack.back();
        stack.pop_back();
        if (v < 0) { order[loc++] = -v; continue; }
        stack.push_back(iib[v - 1]);
        stack.push_back(iia[v - 1]);
    }
}

void tree_from_full(const DevBuf<double> &D, int n, int hmethod, int *merge, double *height, int *order) {
    SHARP_REQUIRE(merge && height && order, "hclust: null output");
    if (n == 2) {                                     // one merge: nothing to agglomerate
        double d = 0;                                 // (on the library's stream, behind whatever filled D)
        SHARP_HIP_CHECK(hipMemcpyAsync(&d, D.p + 1, sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        stream_sync();
        merge[0] = -1; merge[1] = -2; height[0] = d; order[0] = 1; order[1] = 2;
        return;
    }
    HcTree T;
    hclust_tree(D.p, rup128(n), n, hmethod, T);
    for (int i = 0; i < n - 1; ++i)
        SHARP_REQUIRE(std::isfinite(T.crit[i]) && T.ia[i] >= 1 && T.ia[i] <= n && T.ib[i] >= 1 && T.ib[i] <= n && T.ia[i] != T.ib[i],
                      "hclust: NA/NaN/Inf in the distances (a constant row under the correlation distance?)");
    HostTimer ht("hcass2");
    hcass2(n, T.ia.data(), T.ib.data(), merge, order);
    std::copy(T.crit.begin(), T.crit.end(), height);
}

}  // namespace

int dist_nld(int n) { return rup128(n); }

void dist_expand(const double *cond, int n, double *D) {
    const int nld = rup128(n);
    KernelTimer tm("dist_expand");
    hipLaunchKernelGGL(dist_expand_kernel, dim3((nld + 255) / 256, nld), dim3(256), 0, ctx().stream, cond, n, nld, D);
    launch_check("dist_expand_kernel");
}

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_dist(const double *x, int n, int p, long long ld, int method, double minkowski_p, double *d_out) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    SHARP_REQUIRE(d_out, "sharp_dist: null output");
    SHARP_REQUIRE(n <= SHARP_DIST_MAX_N, "sharp_dist: more than 46340 observations (the dist vector would pass 2^30 entries) is not supported");
    check_dist_args(x, n, p, ld, method, minkowski_p, "sharp_dist");
    DevBuf<double> D;
    dist_full(x, n, p, ld, method, minkowski_p, D);
    const size_t len = static_cast<size_t>(n) * (n - 1) / 2;
    DevBuf<double> cond(len);
    {
        KernelTimer tm("dist_condense");
        hipLaunchKernelGGL(dist_condense_kernel, dim3((n + 255) / 256, n - 1), dim3(256), 0, c.stream, D.p, n, rup128(n), cond.p);
        launch_check("dist_condense_kernel");
    }
    cond.download(d_out, len);
    SHARP_API_END
}

int sharp_hclust_dist(const double *d, int n, int hmethod, int *merge, double *height, int *order) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(d, "sharp_hclust_dist: null d");
    SHARP_REQUIRE(n >= 2, "sharp_hclust_dist: must have n >= 2 objects to cluster");
    SHARP_REQUIRE(n <= kHcMaxN, "sharp_hclust_dist: more than 16384 observations is not supported");
    SHARP_REQUIRE(hmethod >= 1 && hmethod <= 8, "sharp_hclust_dist: invalid clustering method");
    const size_t len = static_cast<size_t>(n) * (n - 1) / 2;
    for (size_t e = 0; e < len; ++e) SHARP_REQUIRE(std::isfinite(d[e]), "sharp_hclust_dist: d holds NA / NaN / Inf");
    const int nld = rup128(n);
    DevBuf<double> cond(len), D(static_cast<size_t>(nld) * nld);
    cond.upload(d, len);
    dist_expand(cond.p, n, D.p);
    tree_from_full(D, n, hmethod, merge, height, order);
    SHARP_API_END
}

int sharp_hclust(const double *x, int n, int p, long long ld, int dist_method, double minkowski_p, int hmethod, int *merge, double *height,
                 int *order) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(n <= kHcMaxN, "sharp_hclust: more than 16384 observations is not supported");
    SHARP_REQUIRE(hmethod >= 1 && hmethod <= 8, "sharp_hclust: invalid clustering method");
    check_dist_args(x, n, p, ld, dist_method, minkowski_p, "sharp_hclust");
    DevBuf<double> D;
    dist_full(x, n, p, ld, dist_method, minkowski_p, D);
    tree_from_full(D, n, hmethod, merge, height, order);
    SHARP_API_END
}

}  // extern "C"
