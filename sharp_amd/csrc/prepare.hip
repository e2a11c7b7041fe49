// prepare.hip -- input preparation (prepare.hpp): column means / sd (slab partials), X^T X on the f64 MFMA as slab
// partials summed in a fixed order, a host symmetric eigensolver (Householder tridiagonalisation + implicit QL), the projection X V;
// centring and division by the largest |entry|.  Every reduction runs in an order fixed by n alone.
#include "prepare.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#include "linalg.hpp"

namespace sharp {
namespace {

// ---- column statistics in a fixed order (the sum of a whole vector is graph.hpp's fixed_reduce) ------------------------------------
// column sums of X (n x d, row i at X + i * ld) over slabs of rows: part[s * d + c]; with mu, sums of (x - mu)^2
__global__ __launch_bounds__(256) void colsum_kernel(const double *__restrict__ X, long long n, int d, long long ld, long long rps,
                                                     const double *__restrict__ mu, double *__restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const long long r0 = static_cast<long long>(blockIdx.y) * rps, r1 = r0 + rps < n ? r0 + rps : n;
    double a = 0.0;
    if (mu) {
        const double m = mu[c];
        for (long long r = r0; r < r1; ++r) { const double t = X[r * ld + c] - m; a += t * t; }
    } else {
        for (long long r = r0; r < r1; ++r) a += X[r * ld + c];
    }
    part[static_cast<long long>(blockIdx.y) * d + c] = a;
}

__global__ void slab_sum_kernel(const double *__restrict__ part, int nslab, long long len, double div, double *__restrict__ out) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= len) return;
    double a = 0.0;
    for (int s = 0; s < nslab; ++s) a += part[s * len + e];
    out[e] = a / div;
}

// out[i * d + c] = (X[i * ld + c] - mu[c]) / (sd ? sd[c] : scal)
__global__ __launch_bounds__(256) void affine_kernel(const double *X, long long n, int d, long long ld, const double *__restrict__ mu,
                                                     const double *__restrict__ sd, double scal, double *out) {   // (in place when out == X, ld == d)
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * d) return;
    const long long r = e / d;
    const int c = static_cast<int>(e - r * d);
    double v = X[r * ld + c];
    if (mu) v = v - mu[c];
    out[e] = v / (sd ? sd[c] : scal);
}

// out (n x k) = Xc (n x d) . V (d x k), one thread per output, sequential over d
__global__ __launch_bounds__(256) void project_kernel(const double *__restrict__ Xc, const double *__restrict__ V, long long n, int d, int k,
                                                      double *__restrict__ out) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * k) return;
    const long long r = e / k;
    const int j = static_cast<int>(e - r * k);
    double a = 0.0;
    for (int c = 0; c < d; ++c) a += Xc[r * d + c] * V[static_cast<long long>(c) * k + j];
    out[e] = a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host symmetric eigensolver: Householder tridiagonalisation + implicit QL (the EISPACK tred2 / tql2 pair); V (n x n, row-major) holds
// the matrix on entry and the eigenvectors (columns) on exit, w their eigenvalues in the order QL leaves them (callers sort)
// ---------------------------------------------------------------------------------------------------------------------------
void tred2(int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e) {
    auto A = [&](int i, int j) -> double & { return V[static_cast<size_t>(i) * n + j]; };
    for (int j = 0; j < n; ++j) d[j] = A(n - 1, j);
    for (int i = n - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) { d[j] = A(i - 1, j); A(i, j) = 0.0; A(j, i) = 0.0; }
        } else {
            for (int k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
            double f = d[i - 1], g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h = h - f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j];
                A(j, i) = f;
                g = e[j] + A(j, j) * f;
                for (int k = j + 1; k <= i - 1; ++k) { g += A(k, j) * d[k]; e[k] += A(k, j) * f; }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; ++k) A(k, j) -= (f * e[k] + g * d[k]);
                d[j] = A(i - 1, j);
                A(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; ++i) {
        A(n - 1, i) = A(i, i);
        A(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; ++k) d[k] = A(k, i + 1) / h;
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
                for (int k = 0; k <= i; ++k) g += A(k, i + 1) * A(k, j);
                for (int k = 0; k <= i; ++k) A(k, j) -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) A(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; ++j) { d[j] = A(n - 1, j); A(n - 1, j) = 0.0; }
    A(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
}

void tql2(const char *who, int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e) {
    auto A = [&](int i, int j) -> double & { return V[static_cast<size_t>(i) * n + j]; };
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1 && !(std::fabs(e[m]) <= eps * tst1)) ++m;
        if (m > l) {
            int guard = 0;
            do {
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    for (int k = 0; k < n; ++k) {
                        h = A(k, i + 1);
                        A(k, i + 1) = s * A(k, i) + c * h;
                        A(k, i) = c * A(k, i) - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (!(std::fabs(e[l]) <= eps * tst1) && ++guard < 60);   // (a NaN keeps iterating and is refused below)
            SHARP_REQUIRE(guard < 60, std::string(who) + ": the PCA eigensolver did not converge (non-finite input?)");
        }
        d[l] += f;
        e[l] = 0.0;
    }
}

// the k leading eigenvectors of the symmetric G (d x d) as the columns of Vk (d x k, row-major); sign: the largest |component| positive
void leading_eigenvectors(const char *who, std::vector<double> G, int d, int k, std::vector<double> &Vk) {
    std::vector<double> w(d), e(d);
    tred2(d, G, w, e);
    tql2(who, d, G, w, e);
    std::vector<int> ord(d);
    for (int i = 0; i < d; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return w[a] > w[b]; });
    Vk.assign(static_cast<size_t>(d) * k, 0.0);
    for (int j = 0; j < k; ++j) {
        const int src = ord[j];
        int arg = 0;
        for (int i = 1; i < d; ++i)
            if (std::fabs(G[static_cast<size_t>(i) * d + src]) > std::fabs(G[static_cast<size_t>(arg) * d + src])) arg = i;
        const double sg = G[static_cast<size_t>(arg) * d + src] < 0 ? -1.0 : 1.0;
        for (int i = 0; i < d; ++i) Vk[static_cast<size_t>(i) * k + j] = sg * G[static_cast<size_t>(i) * d + src];
    }
}

}  // namespace

void column_stat(const double *X, long long n, int d, long long ld, const double *mu, double div, DevBuf<double> &part, double *out) {
    const int nslab = static_cast<int>(std::min<long long>(256, std::max<long long>(1, n / 256)));
    const long long rps = (n + nslab - 1) / nslab;
    part.ensure(static_cast<size_t>(nslab) * d);
    hipLaunchKernelGGL(colsum_kernel, dim3(grid_for(d, 256), nslab), dim3(256), 0, ctx().stream, X, n, d, ld, rps, mu, part.p);
    hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(d, 256)), dim3(256), 0, ctx().stream, part.p, nslab, static_cast<long long>(d), div, out);
    launch_check("colsum_kernel");
}

void affine_rows(const double *X, long long n, int d, long long ld, const double *mu, const double *sd, double scal, double *out) {
    hipLaunchKernelGGL(affine_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, ctx().stream, X, n, d, ld, mu, sd, scal, out);
    launch_check("affine_kernel");
}

void symmetric_eigen(const char *who, int d, std::vector<double> &V, std::vector<double> &w) {
    std::vector<double> e(d);
    w.assign(d, 0.0);
    tred2(d, V, w, e);
    tql2(who, d, V, w, e);
}

void prepare_input(const char *who, const double *X, long long n, int d, long long ld, bool pca, int initial_dims, bool pca_center, bool pca_scale,
                   bool normalize, DevBuf<double> &out, int *d_out) {
    Ctx &c = ctx();
    const std::string w(who);
    DevBuf<double> raw, part, stat(static_cast<size_t>(2) * d + 2);
    upload_rows(X, n, d, ld, raw);
    int dd = d;
    if (pca) {
        KernelTimer t("tsne_pca");
        const int k = std::min(initial_dims, d);
        SHARP_REQUIRE(k >= 1, w + ": initial_dims must be >= 1");
        const double *mu = nullptr, *sd = nullptr;
        if (pca_center) { column_stat(raw.p, n, d, d, nullptr, static_cast<double>(n), part, stat.p); mu = stat.p; }
        if (pca_scale) {
            // prcomp(scale. = TRUE): the sd (n - 1) around the centre used (the column mean, or 0 without centring: the root mean square)
            DevBuf<double> zero;
            if (!mu) { zero.alloc(d); zero.zero(); }
            column_stat(raw.p, n, d, d, mu ? mu : zero.p, static_cast<double>(std::max<long long>(n - 1, 1)), part, stat.p + d);
            std::vector<double> v(d);
            SHARP_HIP_CHECK(hipMemcpyAsync(v.data(), stat.p + d, d * sizeof(double), hipMemcpyDeviceToHost, c.stream));
            stream_sync();
            for (int j = 0; j < d; ++j) {
                SHARP_REQUIRE(v[j] > 0 && std::isfinite(v[j]), w + ": cannot rescale a constant/zero column to unit variance (column " + std::to_string(j + 1) + ")");
                v[j] = std::sqrt(v[j]);
            }
            SHARP_HIP_CHECK(hipMemcpyAsync(stat.p + d, v.data(), d * sizeof(double), hipMemcpyHostToDevice, c.stream));
            stream_sync();
            sd = stat.p + d;
        }
        DevBuf<double> xc(static_cast<size_t>(n) * d);
        affine_rows(raw.p, n, d, d, mu, sd, 1.0, xc.p);
        raw.release();
        // X^T X: slab partials on the f64 MFMA (linalg.hip's TN GEMM, symmetric tiles), summed in slab order
        const size_t dd2 = static_cast<size_t>(d) * d;
        int nslab = static_cast<int>(std::min<long long>({64, std::max<long long>(1, n / 512),
                                                          std::max<long long>(1, static_cast<long long>((512ull << 20) / (dd2 * sizeof(double))))}));
        const long long rps = (n + nslab - 1) / nslab;
        nslab = static_cast<int>((n + rps - 1) / rps);
        DevBuf<double> gpart(dd2 * nslab), gram(dd2);
        std::vector<GemmTask> tasks(nslab);
        for (int s = 0; s < nslab; ++s) {
            const long long r0 = s * rps, rows = std::min(rps, n - r0);
            GemmTask &g = tasks[s];
            g.At = xc.p + r0 * d;
            g.Bt = g.At;
            g.C = gpart.p + s * dd2;
            g.M = g.N = d;
            g.K = static_cast<int>(rows);
            g.lda = g.ldb = g.ldc = d;
            g.epilogue = 0;
            g.symmetric = 1;
            g.fast = 0;
        }
        DevBuf<GemmTask> dtasks(tasks.size());
        dtasks.upload(tasks.data(), tasks.size());
        gemm_tn_f64_batched(dtasks.p, nslab, d, d, "tsne_pca_gram", false, true);
        hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(static_cast<long long>(dd2), 256)), dim3(256), 0, c.stream, gpart.p, nslab,
                           static_cast<long long>(dd2), 1.0, gram.p);
        launch_check("slab_sum_kernel");
        std::vector<double> G(dd2), Vk;
        gram.download(G.data(), dd2);
        {
            HostTimer ht("tsne_pca_eigen");
            leading_eigenvectors(who, std::move(G), d, k, Vk);
        }
        DevBuf<double> dV(Vk.size());
        dV.upload(Vk.data(), Vk.size());
        out.alloc(static_cast<size_t>(n) * k);
        hipLaunchKernelGGL(project_kernel, dim3(grid_for(n * k, 256)), dim3(256), 0, c.stream, xc.p, dV.p, n, d, k, out.p);
        launch_check("project_kernel");
        stream_sync();
        dd = k;
    } else {
        out = std::move(raw);
    }
    if (normalize) {
        KernelTimer t("tsne_normalize");
        column_stat(out.p, n, dd, dd, nullptr, static_cast<double>(n), part, stat.p);
        affine_rows(out.p, n, dd, dd, stat.p, nullptr, 1.0, out.p);
        const unsigned nb = fixed_reduce_blocks(n * dd);
        DevBuf<double> mx(nb);
        fixed_reduce_parts(Fold::AbsMax, out.p, n * dd, mx.p);
        std::vector<double> hm(nb);
        mx.download(hm.data(), nb);
        double m = 0.0;
        for (double v : hm) m = std::max(m, v);
        SHARP_REQUIRE(m > 0 && std::isfinite(m), w + ": the normalised input is all zero or not finite");
        affine_rows(out.p, n, dd, dd, nullptr, nullptr, m, out.p);
    }
    *d_out = dd;
}

}  // namespace sharp

using namespace sharp;

extern "C" {

/* Test entry: symmetric_eigen on a host matrix (include/sharp_hip.h); no device is touched. */
int sharp_symmetric_eigen(int d, const double *A, double *w, double *V) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(d >= 1 && A && w && V, "sharp_symmetric_eigen: need d >= 1 and A, w, V");
    const size_t dd = static_cast<size_t>(d) * d;
    std::vector<double> M(A, A + dd), lam;
    symmetric_eigen("sharp_symmetric_eigen", d, M, lam);
    // symmetric_eigen leaves the pairs in the solver's order: ascending here, ties in that order
    std::vector<int> ord(d);
    for (int i = 0; i < d; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return lam[a] < lam[b]; });
    for (int j = 0; j < d; ++j) {
        w[j] = lam[ord[j]];
        for (int i = 0; i < d; ++i) V[static_cast<size_t>(i) * d + j] = M[static_cast<size_t>(i) * d + ord[j]];
    }
    SHARP_API_END
}

}  // extern "C"
