// hvg.hip -- variable-gene selection on raw counts (the specification is the project's own: a variance-stabilising
// selection in the manner of Seurat's "vst" / scanpy's "seurat_v3", with the local fit evaluated directly at every gene instead of
// through R's interpolated loess surface, so no parity with either is claimed).
//   stats     mu and var per gene of the untransformed counts: expr_load's statistics (§21), bit for bit gene_stats(blocks, None, False)
//   loess     over the genes with var > 0, x = log10 mu, y = log10 var (host).  The points are sorted by x (one stable sort_pairs on an
//             order-preserving 64-bit image of x).  One wave per point: the bandwidth h = the q-th smallest |x_j - x_i| by a binary search
//             over the contiguous windows of q sorted points that contain i; the points with |x_j - x_i| < h, a contiguous run found
//             by two more binary searches, are strided by the lanes in sorted order, eight tricube-weighted moments go through the
//             butterfly, and every lane solves the 3 x 3 normal equations by LDL^T (degree 2, falling to 1 and 0 on a small pivot)
//   clipvar   sigma^2 = 10^fit, clip = mu + sigma sqrt(n) (host); the sum of (min(x, clip) - mu)^2 per chunk of the gene-major copy, one
//             wave per chunk, a gene's chunks folded in chunk order by one thread: the standardised variance
//   select    on the host: by the standardised variance descending, ties by the lower gene
// No floating-point atomic: every sum's order is fixed by the input, so two calls give the same bits.
#include "expr_pca.hpp"
#include "graph_prim.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace sharp {
namespace {

constexpr int kHvgMaxFit = 1 << 20;              // fit genes: the direct fit costs about span N^2 weights
constexpr double kHvgPivot = 0x1.0p-30;          // a pivot at or below this share of S0 lowers the degree

// keys[i] = an image of x[i] (+ 0.0, so that -0 and 0 are one value) whose unsigned order is x's; src[i] = i
__global__ __launch_bounds__(256) void hvg_keys_kernel(const double *__restrict__ x, int N, u64 *__restrict__ keys, int *__restrict__ src) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 b = static_cast<u64>(__double_as_longlong(x[i] + 0.0));
    keys[i] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    src[i] = i;
}

// xs[i] = x[src[i]], ys[i] = y[src[i]]
__global__ __launch_bounds__(256) void hvg_gather_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                         const int *__restrict__ src, int N, double *__restrict__ xs,
                                                         double *__restrict__ ys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int s = src[i];
    xs[i] = x[s];
    ys[i] = y[s];
}

// One wave per sorted point i, four points a workgroup (xs ascending, 1 <= q <= N).  fit / bw / deg are written at the point's place in
// the caller's order, src[i], by lane 0.
__global__ __launch_bounds__(256) void hvg_loess_kernel(const double *__restrict__ xs, const double *__restrict__ ys,
                                                        const int *__restrict__ src, int N, int q, double *__restrict__ fit,
                                                        double *__restrict__ bw, int *__restrict__ deg) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int lane = threadIdx.x & 63;
    const double xi = xs[i];
    // h = the smallest, over the windows [a, a + q) that contain i, of the window's largest distance: the left distance falls and the
    // right one grows with a, so the best window is the first whose right distance reaches its left one, or the one before it
    const int alo = i - q + 1 > 0 ? i - q + 1 : 0, ahi = i < N - q ? i : N - q;
    int a0 = alo, a1 = ahi + 1;
    while (a0 < a1) {
        const int mid = (a0 + a1) >> 1;
        if (xs[mid + q - 1] - xi >= xi - xs[mid]) a1 = mid; else a0 = mid + 1;
    }
    double h = 0.0;
    if (a0 <= ahi) h = xs[a0 + q - 1] - xi;
    if (a0 > alo) {
        const double hl = xi - xs[a0 - 1];
        h = a0 <= ahi ? fmin(h, hl) : hl;
    }
    // the run [lo, hi) that takes part: |x_j - x_i| < h, or x_j = x_i when h = 0
    int lo, hi;
    {
        int b0 = 0, b1 = i;                                  // the first j <= i with x_i - x_j < h (<= 0 when h = 0); i itself qualifies
        while (b0 < b1) {
            const int mid = (b0 + b1) >> 1;
            const double d = xi - xs[mid];
            if (h > 0.0 ? d < h : d <= 0.0) b1 = mid; else b0 = mid + 1;
        }
        lo = b0;
        b0 = i + 1;
        b1 = N;                                              // the first j > i with x_j - x_i >= h (> 0 when h = 0), or N
        while (b0 < b1) {
            const int mid = (b0 + b1) >> 1;
            const double d = xs[mid] - xi;
            if (h > 0.0 ? d >= h : d > 0.0) b1 = mid; else b0 = mid + 1;
        }
        hi = b0;
    }
    double out;
    int degree = 0;
    if (!(h > 0.0)) {
        double a = 0.0;
        for (int j = lo + lane; j < hi; j += 64) a += ys[j];
        out = wave_sum(a) / static_cast<double>(hi - lo);
    } else {
        double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
        for (int j = lo + lane; j < hi; j += 64) {
            const double u = (xs[j] - xi) / h;
            const double a = fabs(u);
            const double c = 1.0 - a * a * a;
            const double w = c * c * c;
            const double u2 = u * u;
            const double wy = w * ys[j];
            S0 += w;
            S1 += w * u;
            S2 += w * u2;
            S3 += w * (u2 * u);
            S4 += w * (u2 * u2);
            T0 += wy;
            T1 += wy * u;
            T2 += wy * u2;
        }
        S0 = wave_sum(S0); S1 = wave_sum(S1); S2 = wave_sum(S2); S3 = wave_sum(S3); S4 = wave_sum(S4);
        T0 = wave_sum(T0); T1 = wave_sum(T1); T2 = wave_sum(T2);
        // LDL^T of [[S0, S1, S2], [S1, S2, S3], [S2, S3, S4]] without pivoting; the intercept is the fit at u = 0
        const double l10 = S1 / S0, l20 = S2 / S0;
        const double p1 = S2 - S1 * l10;
        const double tiny = kHvgPivot * S0;
        if (!(p1 > tiny)) {
            out = T0 / S0;
        } else {
            const double l21 = (S3 - l20 * S1) / p1;
            const double p2 = S4 - l20 * S2 - l21 * l21 * p1;
            const double z1 = T1 - l10 * T0;
            if (!(p2 > tiny)) {
                degree = 1;
                out = T0 / S0 - l10 * (z1 / p1);
            } else {
                degree = 2;
                const double z2 = T2 - l20 * T0 - l21 * z1;
                const double b2 = z2 / p2;
                const double b1 = z1 / p1 - l21 * b2;
                out = T0 / S0 - l10 * b1 - l20 * b2;
            }
        }
    }
    if (lane == 0) {
        const int s = src[i];
        fit[s] = out;
        bw[s] = h;
        deg[s] = degree;
    }
}

// One wave per chunk of the gene-major copy: psum[ch] = the chunk's sum of (min(x, clip_g) - mu_g)^2
__global__ __launch_bounds__(256) void hvg_clipvar_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr,
                                                          const int *__restrict__ chgene, long long nch, const double *__restrict__ gval,
                                                          const double *__restrict__ mu, const double *__restrict__ clip,
                                                          double *__restrict__ psum) {
    const long long ch = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (ch >= nch) return;
    const int lane = threadIdx.x & 63;
    const int g = chgene[ch];
    long long b, e;
    chunk_range(gptr, chptr, g, ch, b, e);
    const double m0 = mu[g], cg = clip[g];
    double a = 0.0;
    for (long long p = b + lane; p < e; p += 64) { const double d = fmin(gval[p], cg) - m0; a += d * d; }
    a = wave_sum(a);
    if (lane == 0) psum[ch] = a;
}

// One thread per gene folds its chunks in chunk order: vs = (SS + (n - stored) mu^2) / ((n - 1) sigma^2), 0 for a constant gene
__global__ __launch_bounds__(256) void hvg_clipfold_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr, int m,
                                                           long long n, const double *__restrict__ psum, const double *__restrict__ mu,
                                                           const double *__restrict__ var, const double *__restrict__ sig2,
                                                           double *__restrict__ vs) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= m) return;
    const long long stored = gptr[g + 1] - gptr[g];
    const long long c1 = chptr[g + 1];
    double S = 0.0;
    for (long long ch = chptr[g]; ch < c1; ++ch) S += psum[ch];
    const double m0 = mu[g];
    vs[g] = var[g] > 0.0 ? (S + static_cast<double>(n - stored) * (m0 * m0)) / (static_cast<double>(n - 1) * sig2[g]) : 0.0;
}

int loess_q(int N, double span) { return std::min(N, std::max(3, static_cast<int>(std::ceil(span * static_cast<double>(N))))); }

void check_span(const std::string &who, double span) {
    SHARP_REQUIRE(std::isfinite(span) && span > 0.0 && span <= 1.0, who + ": span must lie in (0, 1]");
}

// the loess of N points (host arrays, any order) -> fit, bandwidth, degree in the caller's order
void hvg_loess(const double *x, const double *y, int N, double span, double *fit, double *bw, int *deg) {
    Ctx &c = ctx();
    KernelTimer timer("hvg_loess");
    const int q = loess_q(N, span);
    DevBuf<double> dx(N), dy(N), xs(N), ys(N), dfit(N), dbw(N);
    DevBuf<u64> keys(N), keys_s(N);
    DevBuf<int> src(N), src_s(N), ddeg(N);
    Scratch tmp;
    dx.upload(x, N);
    dy.upload(y, N);
    hipLaunchKernelGGL(hvg_keys_kernel, dim3(grid_for(N, 256)), dim3(256), 0, c.stream, dx.p, N, keys.p, src.p);
    launch_check("hvg_keys_kernel");
    sort_pairs(keys.p, keys_s.p, src.p, src_s.p, static_cast<size_t>(N), 0, 64, tmp);      // stable: equal x stay in the caller's order
    hipLaunchKernelGGL(hvg_gather_kernel, dim3(grid_for(N, 256)), dim3(256), 0, c.stream, dx.p, dy.p, src_s.p, N, xs.p, ys.p);
    hipLaunchKernelGGL(hvg_loess_kernel, dim3(wave_grid(N)), dim3(256), 0, c.stream, xs.p, ys.p, src_s.p, N, q, dfit.p, dbw.p, ddeg.p);
    launch_check("hvg_loess_kernel");
    dfit.download(fit, N);
    dbw.download(bw, N);
    ddeg.download(deg, N);                                   // (synchronises: the temporaries leave scope)
}

}  // namespace
}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_hvg_loess(const double *x, const double *y, int npts, double span, double *fit, double *bandwidth, int *degree) {
    SHARP_API_BEGIN
    const std::string w("hvg_loess");
    SHARP_REQUIRE(x && y && fit && bandwidth && degree, w + ": null x / y / fit / bandwidth / degree");
    SHARP_REQUIRE(npts >= 1 && npts <= kHvgMaxFit, w + ": need 1 <= npts <= 1048576 points");
    check_span(w, span);
    for (int i = 0; i < npts; ++i)
        SHARP_REQUIRE(std::isfinite(x[i]) && std::isfinite(y[i]), w + ": x and y must be finite (point " + std::to_string(i) + ", counted from 0)");
    ctx();
    hvg_loess(x, y, npts, span, fit, bandwidth, degree);
    SHARP_API_END
}

int sharp_expr_hvg_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                       int n_top_genes, double span, double *means, double *variances, double *variances_expected, double *variances_norm,
                       int *rank, int *highly_variable, int *genes, int *n_selected, int *q, int *degree_counts) {
    SHARP_API_BEGIN
    const std::string w("highly_variable_genes");
    SHARP_REQUIRE(means && variances && variances_expected && variances_norm && rank && highly_variable && genes && n_selected && q &&
                      degree_counts, w + ": null output");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    expr_check_options(w, 0.0, m);
    const long long n = expr_total_cells(w, B);
    SHARP_REQUIRE(n >= 2, w + ": need at least 2 cells in all");
    SHARP_REQUIRE(n_top_genes >= 1, w + ": n_top_genes must be >= 1");
    check_span(w, span);
    Ctx &c = ctx();
    ExprData D;
    ExprExtra extra;
    extra.refuse_negative = true;
    expr_load(w, B, 0.0, false, true, false, 0, 2, D, extra);
    D.mu.download(means, m);
    D.var.download(variances, m);
    // the fit genes: those that vary
    std::vector<int> fg;
    for (int g = 0; g < m; ++g)
        if (variances[g] > 0.0) fg.push_back(g);
    const int N = static_cast<int>(fg.size());
    SHARP_REQUIRE(N >= 1, w + ": every gene is constant");
    SHARP_REQUIRE(N <= kHvgMaxFit, w + ": " + std::to_string(N) + " genes vary; the direct loess fit takes at most 1048576");
    std::vector<double> x(N), y(N), f(N), h(N);
    std::vector<int> dg(N);
    for (int i = 0; i < N; ++i) {
        x[i] = std::log10(means[fg[i]]);
        y[i] = std::log10(variances[fg[i]]);
        SHARP_REQUIRE(std::isfinite(x[i]) && std::isfinite(y[i]), w + ": a gene that varies has a mean that is not positive (gene " +
                                                                      std::to_string(fg[i]) + ", counted from 0)");
    }
    hvg_loess(x.data(), y.data(), N, span, f.data(), h.data(), dg.data());
    *q = loess_q(N, span);
    degree_counts[0] = degree_counts[1] = degree_counts[2] = 0;
    for (int i = 0; i < N; ++i) ++degree_counts[dg[i]];
    std::vector<double> sig2(m, 0.0), clip(m, 0.0);
    const double rn = std::sqrt(static_cast<double>(n));
    for (int i = 0; i < N; ++i) {
        const int g = fg[i];
        sig2[g] = std::pow(10.0, f[i]);
        clip[g] = means[g] + std::sqrt(sig2[g]) * rn;
        SHARP_REQUIRE(sig2[g] > 0.0 && std::isfinite(sig2[g]), w + ": the fitted variance of gene " + std::to_string(g) + " is not a positive number");
    }
    {
        KernelTimer timer("hvg_clipvar");
        const long long nch = D.nch;
        DevBuf<double> dsig(m), dclip(m), psum(std::max<long long>(nch, 1)), vs(m);
        dsig.upload(sig2.data(), m);
        dclip.upload(clip.data(), m);
        if (nch) hipLaunchKernelGGL(hvg_clipvar_kernel, dim3(wave_grid(nch)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, D.chgene.p, nch,
                                    D.gval.p, D.mu.p, dclip.p, psum.p);
        hipLaunchKernelGGL(hvg_clipfold_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, m, n, psum.p, D.mu.p, D.var.p,
                           dsig.p, vs.p);
        launch_check("hvg_clipfold_kernel");
        vs.download(variances_norm, m);                      // (synchronises: the temporaries leave scope)
    }
    for (int g = 0; g < m; ++g) {
        variances_expected[g] = sig2[g];
        rank[g] = -1;
        highly_variable[g] = 0;
    }
    // by the standardised variance descending, ties by the lower gene (fg ascends and the sort is stable)
    std::stable_sort(fg.begin(), fg.end(), [&](int a, int b) { return variances_norm[a] > variances_norm[b]; });
    const int ns = std::min(n_top_genes, N);
    for (int r = 0; r < ns; ++r) {
        rank[fg[r]] = r;
        highly_variable[fg[r]] = 1;
    }
    int at = 0;
    for (int g = 0; g < m; ++g)
        if (highly_variable[g]) genes[at++] = g;
    *n_selected = ns;
    SHARP_API_END
}

}  // extern "C"
