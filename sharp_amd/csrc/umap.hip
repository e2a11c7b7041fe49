// umap.hip -- UMAP beside t-SNE: DESIGN.md §13 (the project's specification, modelled on umap-learn's algorithm and uwot's batch mode;
// no bit parity with either is claimed).
//   curve      a, b by a small Levenberg-Marquardt on the host (fp64), no device needed
//   graph      one wave per row of the k-NN lists: rho (the smallest positive distance), sigma by bisection on
//              sum_j exp(-(d_ij - rho_i) / sigma) = log2(n_neighbors), a floor on sigma, the weights; then COO (i, j, w) + (j, i, w),
//              radix sort by (row, col), the at most two entries of a key merged by x + y - x y (commutative), CSR; wmax = max W
//   epochs     one wave per row, its lanes over the row's (edge, term) slots: term 0 of a firing edge is the attraction (twice: the
//              mirrored entry fires in the same epoch), terms 1 .. negative_sample_rate its hashed negative samples; a butterfly sum
//              per row, all rows from the old positions into a second buffer.  Which edges fire and what they draw depends on
//              (seed, epoch, edge, term) alone, so any range of epochs can be run from a given Y.
// fp64 throughout, no floating-point atomics, every sum in an order fixed by the shape alone: a call is bitwise reproducible.
#include "umap.hpp"
#include "graph_prim.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "graph_source.hpp"
#include "knn.hpp"
#include "prepare.hpp"
#include "rrng.hpp"

namespace sharp {
namespace {

__global__ __launch_bounds__(256) void sqrt_kernel(double *__restrict__ v, long long n) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < n) v[e] = sqrt(v[e]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// graph
// ---------------------------------------------------------------------------------------------------------------------------
// One wave per row (four 64-wide strides of registers, K <= 255): rho[i] = the smallest positive distance of the row (0: none),
// rowsum[i] = sum_j d_ij (per lane over its strides, then the butterfly)
__global__ __launch_bounds__(256) void row_stat_kernel(const double *__restrict__ dist, long long n, int K, double *__restrict__ rho,
                                                       double *__restrict__ rowsum) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double mn = DBL_MAX, s = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = lane + 64 * t;
        const double d = p < K ? dist[i * K + p] : 0.0;
        s += d;
        if (d > 0.0) mn = fmin(mn, d);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = fmin(mn, __shfl_xor(mn, off));
    s = wave_sum(s);
    if (lane == 0) { rho[i] = mn == DBL_MAX ? 0.0 : mn; rowsum[i] = s; }
}

// One wave per row: the bisection on sigma (lo = 0, hi = inf, mid = 1, at most 64 steps, tolerance 1e-5 on the sum), the floor
// 1e-3 * (the row's mean distance, or the global one when rho = 0), the weights, and the row's COO entries (i, j, w) and (j, i, w).
__global__ __launch_bounds__(256) void sigma_kernel(const int *__restrict__ idx, const double *__restrict__ dist, long long n, int K,
                                                    double target, const double *__restrict__ rho, const double *__restrict__ rowsum,
                                                    const double *__restrict__ total, double *__restrict__ sigma,
                                                    unsigned long long *__restrict__ keys, double *__restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double r = rho[i];
    double dv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int p = lane + 64 * t; dv[t] = p < K ? dist[i * K + p] - r : 0.0; }
    double lo = 0.0, hi = HUGE_VAL, mid = 1.0;
    for (int it = 0; it < 64; ++it) {
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (lane + 64 * t < K) s += dv[t] > 0.0 ? exp(-dv[t] / mid) : 1.0;
        s = wave_sum(s);
        if (fabs(s - target) < 1e-5) break;
        if (s > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == HUGE_VAL ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double nn = static_cast<double>(K + 1);
    const double m = r > 0.0 ? rowsum[i] / nn : total[0] / (static_cast<double>(n) * nn);
    const double sg = fmax(mid, 1e-3 * m);
    if (lane == 0) sigma[i] = sg;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = lane + 64 * t;
        if (p >= K) continue;
        const long long e = i * K + p;
        const unsigned long long j = static_cast<unsigned long long>(idx[e]), ui = static_cast<unsigned long long>(i);
        const double w = dv[t] > 0.0 ? exp(-dv[t] / sg) : 1.0;
        keys[2 * e] = ui * static_cast<unsigned long long>(n) + j;
        vals[2 * e] = w;
        keys[2 * e + 1] = j * static_cast<unsigned long long>(n) + ui;
        vals[2 * e + 1] = w;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// epochs
// ---------------------------------------------------------------------------------------------------------------------------
// One wave per row i, lanes over the slots s = edge * T + term of the row (T = 1 + negative_sample_rate), pass after pass of 64 in
// slot order; a slot whose edge fires adds its term to the lane's sum, the lanes' sums are folded by a butterfly, and
// Yout_i = Yin_i + alpha * sum.  x0 = mix(seed * 0x9E3779B97F4A7C15 + ep).
template <int DIMS>
__global__ __launch_bounds__(256) void epoch_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                    const double *__restrict__ Yin, double *__restrict__ Yout, long long n, int ep, double alpha,
                                                    double a, double b, double gamma, int T, double wmax, unsigned long long x0) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double yi[DIMS], acc[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { yi[k] = Yin[i * DIMS + k]; acc[k] = 0.0; }
    const long long e0 = rp[i];
    const unsigned slots = static_cast<unsigned>(rp[i + 1] - e0) * static_cast<unsigned>(T);   // (< 2^31: checked on the host)
    const double epd = static_cast<double>(ep), epm = static_cast<double>(ep - 1);
    if (ep >= 1)
        for (unsigned s = lane; s < slots; s += 64) {
            const unsigned el = s / static_cast<unsigned>(T), t = s - el * static_cast<unsigned>(T);
            const long long e = e0 + el;
            const double r = val[e] / wmax;
            if (!(floor(epd * r) > floor(epm * r))) continue;
            long long v;
            if (t == 0) {
                v = col[e];
            } else {
                const unsigned long long x = mix64(mix64(x0 + static_cast<unsigned long long>(e)) + static_cast<unsigned long long>(t - 1));
                v = static_cast<long long>(floor(static_cast<double>(x >> 11) * 0x1.0p-53 * static_cast<double>(n)));
                if (v > n - 1) v = n - 1;   // (never taken: (1 - 2^-53) n rounds below n)
                if (v == i) continue;
            }
            double diff[DIMS], D = 0.0;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) { diff[k] = yi[k] - Yin[v * DIMS + k]; D += diff[k] * diff[k]; }
            if (!(D > 0.0)) continue;
            const double den = a * pow(D, b) + 1.0;
            if (t == 0) {
                const double c = (-2.0 * a * b * pow(D, b - 1.0)) / den;
#pragma unroll
                for (int k = 0; k < DIMS; ++k) acc[k] += 2.0 * clip4(c * diff[k]);
            } else {
                const double c = (2.0 * gamma * b) / ((0.001 + D) * den);
#pragma unroll
                for (int k = 0; k < DIMS; ++k) acc[k] += clip4(c * diff[k]);
            }
        }
#pragma unroll
    for (int k = 0; k < DIMS; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DIMS; ++k) Yout[i * DIMS + k] = yi[k] + alpha * acc[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host pieces
// ---------------------------------------------------------------------------------------------------------------------------
// residuals and Jacobian of the curve at (a, b): r_k = 1 / (1 + a x_k^(2b)) - y_k; cost = sum r^2, g = J^T r, H = J^T J
struct CurveEval { double cost, g[2], H[3], jn2; };
CurveEval curve_eval(const std::vector<double> &x, const std::vector<double> &y, double a, double b) {
    CurveEval c{0.0, {0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0};
    for (size_t k = 0; k < x.size(); ++k) {
        double f = 1.0, ja = 0.0, jb = 0.0;
        if (x[k] > 0.0) {
            const double p = std::pow(x[k], 2.0 * b), q = 1.0 + a * p;
            f = 1.0 / q;
            ja = -p / (q * q);
            jb = -(a * p * 2.0 * std::log(x[k])) / (q * q);
        }
        const double r = f - y[k];
        c.cost += r * r;
        c.g[0] += ja * r;
        c.g[1] += jb * r;
        c.H[0] += ja * ja;
        c.H[1] += ja * jb;
        c.H[2] += jb * jb;
    }
    c.jn2 = c.H[0] + c.H[2];
    return c;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
void umap_ab(double spread, double min_dist, double *a_out, double *b_out) {
    SHARP_REQUIRE(std::isfinite(spread) && std::isfinite(min_dist), "umap: spread and min_dist must be finite");
    SHARP_REQUIRE(spread > 0.0, "umap: spread must be positive");
    SHARP_REQUIRE(min_dist >= 0.0, "umap: min_dist must be >= 0");
    SHARP_REQUIRE(min_dist < 3.0 * spread, "umap: min_dist must be below 3 spread (the curve is fitted on [0, 3 spread])");
    const int np = 300;
    std::vector<double> x(np), y(np);
    const double stop = 3.0 * spread, step = stop / (np - 1);
    for (int k = 0; k < np; ++k) {
        x[k] = k == np - 1 ? stop : k * step;   // numpy's linspace
        y[k] = x[k] < min_dist ? 1.0 : std::exp(-(x[k] - min_dist) / spread);
    }
    double a = 1.0, b = 1.0, lambda = 1e-3;
    CurveEval c = curve_eval(x, y, a, b);
    for (int it = 0; it < 1000; ++it) {
        const double gn = std::sqrt(c.g[0] * c.g[0] + c.g[1] * c.g[1]);
        if (gn <= 1e-14 * std::sqrt(c.jn2) * std::sqrt(c.cost)) break;
        // (H + lambda diag H) delta = -g
        const double h00 = c.H[0] * (1.0 + lambda), h11 = c.H[2] * (1.0 + lambda), h01 = c.H[1];
        const double det = h00 * h11 - h01 * h01;
        bool ok = det > 0.0 && std::isfinite(det);
        double na = a, nb = b;
        if (ok) {
            na = a - (h11 * c.g[0] - h01 * c.g[1]) / det;
            nb = b - (h00 * c.g[1] - h01 * c.g[0]) / det;
            ok = std::isfinite(na) && std::isfinite(nb) && na > 0.0 && nb > 0.0;
        }
        if (ok) {
            const CurveEval t = curve_eval(x, y, na, nb);
            // (at the end the cost is flat to rounding: there a step counts when it shrinks the gradient)
            const double tgn = std::sqrt(t.g[0] * t.g[0] + t.g[1] * t.g[1]);
            if (std::isfinite(t.cost) && (t.cost < c.cost || (t.cost <= c.cost * (1.0 + 1e-15) && tgn < gn))) {
                const bool still = na == a && nb == b;
                a = na;
                b = nb;
                c = t;
                lambda = std::max(lambda * 0.1, 1e-12);
                if (still) break;
                continue;
            }
        }
        lambda *= 10.0;
        if (lambda > 1e12) break;
    }
    SHARP_REQUIRE(std::isfinite(a) && std::isfinite(b) && a > 0.0 && b > 0.0, "umap: the a / b curve fit failed");
    *a_out = a;
    *b_out = b;
}

void umap_graph(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, UmapGraph &G, DevBuf<double> *rho_out,
                DevBuf<double> *sigma_out) {
    Ctx &c = ctx();
    SHARP_REQUIRE(K >= 1 && K <= 255 && K <= n - 1, "umap_graph: need 1 <= K <= 255 and K < n");
    const size_t ne = static_cast<size_t>(n) * K * 2;
    DevBuf<double> rho_l, sigma_l;
    DevBuf<double> &rho = rho_out ? *rho_out : rho_l, &sigma = sigma_out ? *sigma_out : sigma_l;
    rho.alloc(n);
    sigma.alloc(n);
    DevBuf<unsigned long long> keys(ne), keys2(ne);
    DevBuf<double> vals(ne), vals2(ne), red(kRedBlocks), scal(2);
    {
        KernelTimer t("umap_graph");
        DevBuf<double> rowsum(n);
        hipLaunchKernelGGL(row_stat_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, dist.p, n, K, rho.p, rowsum.p);
        launch_check("row_stat_kernel");
        fixed_reduce(Fold::Sum, rowsum.p, n, red.p, scal.p);
        hipLaunchKernelGGL(sigma_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, idx.p, dist.p, n, K, std::log2(static_cast<double>(K + 1)),
                           rho.p, rowsum.p, scal.p, sigma.p, keys.p, vals.p);
        launch_check("sigma_kernel");
        stream_sync();   // (rowsum goes out of scope)
    }
    KernelTimer t("umap_sym");
    // the fuzzy union of the at most two entries of a key
    const u64 un = static_cast<u64>(n);
    MergeScratch tmp;
    const size_t nnz = merge_by_key<double, FuzzyUnion>(keys.p, vals.p, ne, un * un, keys2.p, vals2.p, keys.p, vals.p, tmp);
    SHARP_REQUIRE(nnz >= static_cast<size_t>(n) * K && nnz <= ne, "umap_graph: the union holds an impossible number of entries");
    fixed_reduce(Fold::Max, vals.p, static_cast<long long>(nnz), red.p, scal.p + 1);
    G.n = n;
    G.nnz = static_cast<long long>(nnz);
    G.row_ptr.alloc(n + 1);
    G.col.alloc(nnz);
    G.val.alloc(nnz);
    merged_to_csr<double>(keys.p, G.nnz, n, false, G.row_ptr.p, G.col.p, nullptr, vals.p, nullptr, G.val.p);   // (no row is empty: K entries each)
    SHARP_HIP_CHECK(hipMemcpyAsync(&G.wmax, scal.p + 1, sizeof(double), hipMemcpyDeviceToHost, c.stream));
    stream_sync();
}

void umap_epochs(const UmapGraph &G, double *dY, int dims, int n_epochs, int ep0, int ep1, double learning_rate, double a, double b,
                 int negative_sample_rate, double repulsion_strength, unsigned long long seed) {
    Ctx &c = ctx();
    SHARP_REQUIRE(dims >= 1 && dims <= 3, "umap: n_components must be 1, 2 or 3");
    SHARP_REQUIRE(n_epochs >= 0 && ep0 >= 0 && ep0 <= ep1 && ep1 <= n_epochs, "umap: need 0 <= ep0 <= ep1 <= n_epochs");
    SHARP_REQUIRE(negative_sample_rate >= 0 && negative_sample_rate <= 64, "umap: negative_sample_rate must be in 0 .. 64");
    SHARP_REQUIRE(std::isfinite(learning_rate) && std::isfinite(repulsion_strength), "umap: learning_rate and repulsion_strength must be finite");
    SHARP_REQUIRE(std::isfinite(a) && std::isfinite(b) && a > 0.0 && b > 0.0, "umap: a and b must be positive");
    const int T = 1 + negative_sample_rate;
    SHARP_REQUIRE(G.n >= 2 && G.n * T < INT_MAX, "umap: n (1 + negative_sample_rate) must stay below 2^31");
    SHARP_REQUIRE(G.wmax > 0.0 && std::isfinite(G.wmax), "umap: the graph holds no positive weight");
    if (ep0 == ep1) return;
    const size_t ne = static_cast<size_t>(G.n) * dims;
    DevBuf<double> other(ne);
    double *cur = dY, *nxt = other.p;
    KernelTimer t("umap_epochs");
    for (int ep = ep0; ep < ep1; ++ep) {
        const double alpha = learning_rate * (1.0 - static_cast<double>(ep) / static_cast<double>(n_epochs));
        const unsigned long long x0 = mix64(seed * 0x9E3779B97F4A7C15ull + static_cast<unsigned long long>(ep));
        const dim3 grid(grid_for(G.n, 4)), block(256);
        if (dims == 1)
            hipLaunchKernelGGL(epoch_kernel<1>, grid, block, 0, c.stream, G.row_ptr.p, G.col.p, G.val.p, cur, nxt, G.n, ep, alpha, a, b,
                               repulsion_strength, T, G.wmax, x0);
        else if (dims == 2)
            hipLaunchKernelGGL(epoch_kernel<2>, grid, block, 0, c.stream, G.row_ptr.p, G.col.p, G.val.p, cur, nxt, G.n, ep, alpha, a, b,
                               repulsion_strength, T, G.wmax, x0);
        else
            hipLaunchKernelGGL(epoch_kernel<3>, grid, block, 0, c.stream, G.row_ptr.p, G.col.p, G.val.p, cur, nxt, G.n, ep, alpha, a, b,
                               repulsion_strength, T, G.wmax, x0);
        launch_check("epoch_kernel");
        std::swap(cur, nxt);
    }
    if (cur != dY) SHARP_HIP_CHECK(hipMemcpyAsync(dY, cur, ne * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    stream_sync();   // (the second buffer goes out of scope)
}

void umap_sqrt_lists(DevBuf<double> &dist, long long n, int K) {
    KernelTimer t("umap_sqrt");
    hipLaunchKernelGGL(sqrt_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, ctx().stream, dist.p, n * K);
    launch_check("sqrt_kernel");
}

}  // namespace sharp

using namespace sharp;

namespace {

struct UmapArgs {
    int dims, n_epochs;
    double learning_rate, min_dist, spread;
    double *ab;
    int negative_sample_rate;
    double repulsion_strength;
    int init;                  // 0 "pca", 1 "random", 2 Y_init, 3 "normlaplacian" 
    const double *Y_init;
    double seed;
};

void check_umap_args(long long n, const UmapArgs &u, const double *Y) {
    SHARP_REQUIRE(u.dims >= 1 && u.dims <= 3, "umap: n_components must be 1, 2 or 3");
    SHARP_REQUIRE(Y && u.ab, "umap: null Y / ab");
    SHARP_REQUIRE(u.init >= 0 && u.init <= 3, "umap: init must be 0 (pca), 1 (random), 2 (Y_init) or 3 (normlaplacian)");
    SHARP_REQUIRE(u.init != 3 || n >= u.dims + 2, "umap: init = \"normlaplacian\" needs at least n_components + 2 rows");
    SHARP_REQUIRE(u.init != 2 || u.Y_init, "umap: init = 2 needs Y_init");
    SHARP_REQUIRE(u.negative_sample_rate >= 0 && u.negative_sample_rate <= 64, "umap: negative_sample_rate must be in 0 .. 64");
    SHARP_REQUIRE(std::isfinite(u.learning_rate) && std::isfinite(u.repulsion_strength), "umap: learning_rate and repulsion_strength must be finite");
    SHARP_REQUIRE(std::isfinite(u.seed) && std::fabs(u.seed) < 9.0e18, "umap: seed must be a finite integer");
    SHARP_REQUIRE(n * (1 + u.negative_sample_rate) < INT_MAX, "umap: n (1 + negative_sample_rate) must stay below 2^31");
    if (u.init == 2)
        for (size_t e = 0; e < static_cast<size_t>(n) * u.dims; ++e) SHARP_REQUIRE(std::isfinite(u.Y_init[e]), "umap: init holds NA / NaN / Inf");
}

// a, b: as given when both are positive, else fitted from (spread, min_dist) and written back
void resolve_ab(const UmapArgs &u) {
    if (u.ab[0] > 0.0 && u.ab[1] > 0.0 && std::isfinite(u.ab[0]) && std::isfinite(u.ab[1])) return;
    HostTimer ht("umap_ab");
    umap_ab(u.spread, u.min_dist, &u.ab[0], &u.ab[1]);
}

int resolve_epochs(long long n, int n_epochs) { return n_epochs >= 0 ? n_epochs : (n <= 10000 ? 500 : 200); }

// every coordinate mapped affinely onto [0, 10]; a constant coordinate becomes 0
void scale_start(std::vector<double> &y, long long n, int dims) {
    for (int k = 0; k < dims; ++k) {
        double mn = DBL_MAX, mx = -DBL_MAX;
        for (long long i = 0; i < n; ++i) { mn = std::min(mn, y[i * dims + k]); mx = std::max(mx, y[i * dims + k]); }
        const double w = mx - mn;
        for (long long i = 0; i < n; ++i) y[i * dims + k] = w > 0.0 ? (y[i * dims + k] - mn) / w * 10.0 : 0.0;
    }
}

// Everything behind the neighbour lists (idx, dist: device, n x K, Euclidean; released once the graph exists).  Xp: the prepared input
// on the device (n x dp) for init = 0 and for init = 3 (whose fallback is the PCA start), else null.
void run_from_lists(DevBuf<int> &idx, DevBuf<double> &dist, long long n, int K, const DevBuf<double> *Xp, int dp, const UmapArgs &u, double *Y) {
    resolve_ab(u);
    const int n_epochs = resolve_epochs(n, u.n_epochs);
    const size_t ne = static_cast<size_t>(n) * u.dims;
    std::vector<double> y0(ne);
    // the start of code 0, 1 or 2, mapped onto [0, 10]
    auto start_from = [&](int code) {
        HostTimer ht("umap_init");
        if (code == 2) {
            std::copy(u.Y_init, u.Y_init + ne, y0.begin());
        } else if (code == 1) {
            RRng rng(static_cast<uint32_t>(static_cast<long long>(u.seed)));   // runif(-10, 10) from set.seed(seed), row by row
            for (size_t e = 0; e < ne; ++e) y0[e] = -10.0 + 20.0 * rng.unif();
        } else {
            SHARP_REQUIRE(Xp, "umap: init = \"pca\" needs the data (give init = \"random\" or a matrix with neighbour lists)");
            SHARP_REQUIRE(dp >= u.dims, "umap: init = \"pca\" needs at least n_components columns");
            std::vector<double> hx(static_cast<size_t>(n) * dp);
            Xp->download(hx.data(), hx.size());
            DevBuf<double> pc;
            int k = 0;
            prepare_input("umap", hx.data(), n, dp, dp, true, u.dims, true, false, false, pc, &k);
            SHARP_REQUIRE(k == u.dims, "umap: the PCA start has the wrong number of components");
            pc.download(y0.data(), ne);
        }
        scale_start(y0, n, u.dims);
    };
    UmapInitInfo &info = umap_init_info();
    info = UmapInitInfo();
    info.requested = info.used = u.init;
    if (u.init != 3) start_from(u.init);
    UmapGraph G;
    umap_graph(idx, dist, n, K, G);
    idx.release();
    dist.release();
    if (u.init == 3) {
        // the bottom eigenvectors of the graph's normalised Laplacian; a graph in pieces or a solve that does not converge falls back
        // as uwot does: to the PCA start where the data are at hand, else to the random one
        UmapSpectral S;
        umap_spectral(G, u.dims, 0.0, 0, S);
        info.components = S.components;
        info.steps = S.steps;
        info.residual = S.outcome == 1 ? 0.0 : *std::max_element(S.residual, S.residual + u.dims);
        if (S.outcome == 0) {
            HostTimer ht("umap_init");
            y0 = S.V;
            scale_start(y0, n, u.dims);
        } else {
            info.used = Xp ? 0 : 1;
            start_from(info.used);
        }
    }
    DevBuf<double> dY(ne);
    dY.upload(y0.data(), ne);
    umap_epochs(G, dY.p, u.dims, n_epochs, 0, n_epochs, u.learning_rate, u.ab[0], u.ab[1], u.negative_sample_rate, u.repulsion_strength,
                static_cast<unsigned long long>(static_cast<long long>(u.seed)));
    dY.download(Y, ne);
}

void check_lists(const int *index, const double *distance, long long n, int K, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(index && distance, w + ": null index / distance");
    SHARP_REQUIRE(n >= 2 && n < INT_MAX, w + ": need 2 <= n < 2^31 rows");
    SHARP_REQUIRE(K >= 1, w + ": need at least one neighbour per row (K >= 1)");
    SHARP_REQUIRE(K <= 255, w + ": at most 255 neighbours per row");
    SHARP_REQUIRE(K <= n - 1, w + ": K neighbours per row need K <= n - 1");
}

}  // namespace

extern "C" {

int sharp_umap_ab(double spread, double min_dist, double *a, double *b) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(a && b, "sharp_umap_ab: null output");
    umap_ab(spread, min_dist, a, b);
    SHARP_API_END
}

int sharp_umap(const double *X, long long n, int d, long long ld, int n_neighbors, int dims, int n_epochs, double learning_rate, double min_dist,
               double spread, double *ab, int negative_sample_rate, double repulsion_strength, int init, const double *Y_init, int pca,
               int pca_center, double seed, double *Y, int *nn_index, double *nn_distance) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(X && n >= 2 && d >= 1 && ld >= d, "umap: bad input matrix (need n >= 2 rows of d >= 1 values, ld >= d)");
    SHARP_REQUIRE(n < INT_MAX, "umap: at most 2^31 - 1 rows");
    SHARP_REQUIRE(n_neighbors >= 2 && n_neighbors <= 256, "umap: n_neighbors must be in 2 .. 256");
    SHARP_REQUIRE(n_neighbors <= n - 1, "umap: n_neighbors must be smaller than the number of rows");
    SHARP_REQUIRE(pca >= 0, "umap: pca must be 0 (none) or a number of components");
    SHARP_REQUIRE((nn_index == nullptr) == (nn_distance == nullptr), "umap: nn_index and nn_distance go together");
    const UmapArgs u{dims, n_epochs, learning_rate, min_dist, spread, ab, negative_sample_rate, repulsion_strength, init, Y_init, seed};
    check_umap_args(n, u, Y);
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < d; ++c)
            if (!std::isfinite(X[i * ld + c]))
                throw sharp::Error(SHARP_ERR_ARG, "umap: the input holds NA / NaN / Inf (row " + std::to_string(i + 1) + ", column " +
                                                      std::to_string(c + 1) + ")");
    const int K = n_neighbors - 1;
    DevBuf<double> Xp;
    int dp = 0;
    prepare_input("umap", X, n, d, ld, pca > 0, pca, pca_center != 0, false, false, Xp, &dp);
    DevBuf<int> idx;
    DevBuf<double> dist;
    knn_self("umap", Xp.p, n, dp, K, idx, dist);
    umap_sqrt_lists(dist, n, K);
    if (nn_index) {
        idx.download(nn_index, static_cast<size_t>(n) * K);
        dist.download(nn_distance, static_cast<size_t>(n) * K);
    }
    const bool keep_x = init == 0 || init == 3;   // (the spectral start falls back to the PCA one)
    if (!keep_x) Xp.release();
    run_from_lists(idx, dist, n, K, keep_x ? &Xp : nullptr, dp, u, Y);
    SHARP_API_END
}

int sharp_umap_neighbors(const int *index, const double *distance, long long n, int K, int squared, int dims, int n_epochs, double learning_rate,
                         double min_dist, double spread, double *ab, int negative_sample_rate, double repulsion_strength, int init,
                         const double *Y_init, double seed, double *Y) {
    SHARP_API_BEGIN
    ctx();
    check_lists(index, distance, n, K, "sharp_umap_neighbors");
    const UmapArgs u{dims, n_epochs, learning_rate, min_dist, spread, ab, negative_sample_rate, repulsion_strength, init, Y_init, seed};
    check_umap_args(n, u, Y);
    SHARP_REQUIRE(init != 0, "umap_neighbors: init = \"pca\" needs the data; give \"random\" or a matrix");
    DevBuf<int> idx;
    DevBuf<double> dist;
    lists_to_device("umap_neighbors", index, distance, n, K, squared != 0, idx, dist);
    run_from_lists(idx, dist, n, K, nullptr, 0, u, Y);
    SHARP_API_END
}

int sharp_umap_graph(const int *index, const double *distance, long long n, int K, int squared, long long cap, long long *row_ptr, int *col,
                     double *val, long long *nnz, double *rho, double *sigma) {
    SHARP_API_BEGIN
    ctx();
    check_lists(index, distance, n, K, "sharp_umap_graph");
    SHARP_REQUIRE(row_ptr && col && val && nnz && rho && sigma, "sharp_umap_graph: null output");
    DevBuf<int> idx;
    DevBuf<double> dist, drho, dsigma;
    lists_to_device("sharp_umap_graph", index, distance, n, K, squared != 0, idx, dist);
    UmapGraph G;
    umap_graph(idx, dist, n, K, G, &drho, &dsigma);
    *nnz = G.nnz;
    SHARP_REQUIRE(cap >= G.nnz, "sharp_umap_graph: col / val hold fewer than nnz entries (2 n K always suffice)");
    G.row_ptr.download(row_ptr, static_cast<size_t>(n) + 1);
    G.col.download(col, static_cast<size_t>(G.nnz));
    G.val.download(val, static_cast<size_t>(G.nnz));
    drho.download(rho, static_cast<size_t>(n));
    dsigma.download(sigma, static_cast<size_t>(n));
    SHARP_API_END
}

int sharp_umap_epochs(const long long *row_ptr, const int *col, const double *val, long long n, int dims, double *Y, int n_epochs, int ep0,
                      int ep1, double learning_rate, double a, double b, int negative_sample_rate, double repulsion_strength, double seed) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(row_ptr && col && val && Y && n >= 2 && n < INT_MAX, "sharp_umap_epochs: null argument, or n outside 2 .. 2^31 - 1");
    SHARP_REQUIRE(dims >= 1 && dims <= 3, "umap: n_components must be 1, 2 or 3");
    SHARP_REQUIRE(std::isfinite(seed) && std::fabs(seed) < 9.0e18, "umap: seed must be a finite integer");
    SHARP_REQUIRE(row_ptr[0] == 0 && row_ptr[n] >= 1, "sharp_umap_epochs: row_ptr must run from 0 to nnz >= 1");
    for (long long i = 0; i < n; ++i)
        SHARP_REQUIRE(row_ptr[i] <= row_ptr[i + 1] && row_ptr[i + 1] - row_ptr[i] <= n, "sharp_umap_epochs: row_ptr is not monotone, or a row holds more than n entries");
    double wmax = 0.0;
    for (long long e = 0; e < row_ptr[n]; ++e) {
        SHARP_REQUIRE(col[e] >= 0 && col[e] < n, "sharp_umap_epochs: a column index out of range");
        SHARP_REQUIRE(val[e] >= 0.0 && val[e] <= DBL_MAX, "sharp_umap_epochs: a weight that is NA / NaN / Inf or negative");
        wmax = std::max(wmax, val[e]);
    }
    const size_t ne = static_cast<size_t>(n) * dims;
    for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(std::isfinite(Y[e]), "sharp_umap_epochs: Y holds NA / NaN / Inf");
    UmapGraph G;
    csr_to_device(row_ptr, col, val, n, wmax, G);
    DevBuf<double> dY(ne);
    dY.upload(Y, ne);
    umap_epochs(G, dY.p, dims, n_epochs, ep0, ep1, learning_rate, a, b, negative_sample_rate, repulsion_strength,
                static_cast<unsigned long long>(static_cast<long long>(seed)));
    dY.download(Y, ne);
    SHARP_API_END
}

}  // extern "C"
