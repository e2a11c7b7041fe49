// umap_spectral.hip -- UMAP's spectral start, init = "normlaplacian": DESIGN.md §15 (the project's specification, modelled on uwot's
// "normlaplacian" and umap-learn's spectral layout; no bit parity with either is claimed).
//   components  min-label propagation over the CSR pattern with pointer jumping: every sweep hooks each tree's root onto the smallest
//               root an edge reaches (integer atomicMin: the fixed point does not depend on the order) and then flattens every tree,
//               until a device flag says that nothing moved.  label[i] = the smallest vertex of i's component.
//   operator    deg_i = sum_j W_ij (one wave per row, CSR order), s = 1 / sqrt(deg), M = D^-1/2 W D^-1/2 applied as
//               y_i = s_i sum_j W_ij s_j x_j (one wave per row, lanes stride the row in passes of 64, a butterfly folds them);
//               q0 = sqrt(deg) / ||sqrt(deg)|| is M's eigenvector for the eigenvalue 1
//   solver      Lanczos on the complement of q0 with full reorthogonalisation (two classical Gram-Schmidt passes against q0 and every
//               earlier vector), the basis column by column in HBM; the host solves T = tridiag(alpha, beta) by implicit QL every
//               kCheckEvery steps; when the Ritz estimates |beta_m S_mj| of the top dims pairs are <= tol the Ritz vectors V = Q S are
//               formed, normalised, and their true residuals ||M v - theta v|| decide.
// Defaults (tol <= 0, max_steps <= 0): kSpectralTol = 1e-6, kSpectralMaxSteps = 400.
// fp64 throughout, no floating-point atomics, every sum in an order fixed by the shape alone: two calls give the same bits.
#include "spectral_dev.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

namespace sharp {
namespace {

constexpr double kSpectralTol = 1e-6;
constexpr int kSpectralMaxSteps = 400;
constexpr int kCheckEvery = 8;      // steps between two solves of T on the host (and once more at max_steps)

// ---------------------------------------------------------------------------------------------------------------------------
// connected components
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_init_kernel(int *__restrict__ label, int *__restrict__ prev, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) { label[i] = static_cast<int>(i); prev[i] = static_cast<int>(i); }
}

// One wave per row.  prev holds the sweep's starting labels (every tree is flat: prev[i] is i's root) and is only read; the roots'
// entries of label are lowered.  An edge is taken in both directions, so a pattern that is not symmetric is treated as undirected.
// WITHIN: only the entries whose two ends carry the same value of `within` count (the components inside a labelling).
template <bool WITHIN>
__global__ __launch_bounds__(256) void cc_hook_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const int *__restrict__ prev,
                                                      int *__restrict__ label, long long n, int *__restrict__ changed,
                                                      const int *__restrict__ within) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int li = prev[i];
    const long long e1 = rp[i + 1];
    const int wi = WITHIN ? within[i] : 0;
    for (long long e = rp[i] + lane; e < e1; e += 64) {
        if (WITHIN && within[col[e]] != wi) continue;
        const int lj = prev[col[e]];
        if (lj < li) {
            atomicMin(&label[li], lj);
            *changed = 1;
        } else if (lj > li) {
            atomicMin(&label[lj], li);
            *changed = 1;
        }
    }
}

// Every vertex follows its pointers to the root (pointers lead to smaller numbers, the roots do not move during this kernel, and a
// pointer another thread has already shortened still leads to the same root) and takes it; prev = label afterwards.
__global__ __launch_bounds__(256) void cc_jump_kernel(int *label, int *__restrict__ prev, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    int l = label[i];
    for (int p = label[l]; p != l; p = label[l]) l = p;
    label[i] = l;
    prev[i] = l;
}

__global__ __launch_bounds__(256) void cc_count_kernel(const int *__restrict__ label, long long n, unsigned long long *__restrict__ count) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const bool root = i < n && label[i] == static_cast<int>(i);
    const unsigned long long b = __ballot(root);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, static_cast<unsigned long long>(__popcll(b)));
}

// ---------------------------------------------------------------------------------------------------------------------------
// the operator
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void degree_kernel(const long long *__restrict__ rp, const double *__restrict__ val, long long n,
                                                     double *__restrict__ s, double *__restrict__ sq) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long e1 = rp[i + 1];
    double a = 0.0;
    for (long long e = rp[i] + lane; e < e1; e += 64) a += val[e];
    a = wave_sum(a);
    if (lane == 0) { const double r = sqrt(a); sq[i] = r; s[i] = 1.0 / r; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the basis: Q holds its vectors column by column (n contiguous doubles each)
// ---------------------------------------------------------------------------------------------------------------------------
// V_j[i] = sum_k Q_k[i] S[k][j], k ascending (S: m x DIMS row-major; V: DIMS columns of n)
template <int DIMS>
__global__ __launch_bounds__(256) void ritz_kernel(const double *__restrict__ Q, int m, const double *__restrict__ S, double *__restrict__ V,
                                                   long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double a[DIMS];
#pragma unroll
    for (int j = 0; j < DIMS; ++j) a[j] = 0.0;
    for (int k = 0; k < m; ++k) {
        const double q = Q[static_cast<long long>(k) * n + i];
#pragma unroll
        for (int j = 0; j < DIMS; ++j) a[j] += q * S[k * DIMS + j];
    }
#pragma unroll
    for (int j = 0; j < DIMS; ++j) V[static_cast<long long>(j) * n + i] = a[j];
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the symmetric tridiagonal eigenproblem by implicit QL (EISPACK's tql2).  d (m): the diagonal in, the eigenvalues out (not
// sorted); e (m): e[i] couples i and i + 1, e[m - 1] = 0; Z (rows x m, row-major): any rows of an orthogonal matrix in (rows of the
// identity), the same rows of (that matrix times the eigenvectors) out -- the bottom row alone gives the residual estimates in O(m^2).
// ---------------------------------------------------------------------------------------------------------------------------
void tridiag_ql(int m, std::vector<double> &d, std::vector<double> &e, std::vector<double> &Z, int rows) {
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < m; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int mm = l;
        while (mm < m - 1 && !(std::fabs(e[mm]) <= eps * tst1)) ++mm;
        if (mm > l) {
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
                for (int i = l + 2; i < m; ++i) d[i] -= h;
                f += h;
                p = d[mm];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = mm - 1; i >= l; --i) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    for (int k = 0; k < rows; ++k) {
                        double *z = &Z[static_cast<size_t>(k) * m];
                        h = z[i + 1];
                        z[i + 1] = s * z[i] + c * h;
                        z[i] = c * z[i] - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1 && ++guard < 60);
            if (guard >= 60) throw Error(SHARP_ERR, "umap_spectral: the tridiagonal eigensolver did not converge");
        }
        d[l] += f;
        e[l] = 0.0;
    }
}

}  // namespace

UmapInitInfo &umap_init_info() { return per_slot<UmapInitInfo>(); }

// ---------------------------------------------------------------------------------------------------------------------------
long long umap_components(const UmapGraph &G, DevBuf<int> *label_out) {
    SHARP_REQUIRE(G.n >= 1 && G.n < INT_MAX, "umap_components: need 1 <= n < 2^31 rows");
    DevBuf<int> label_l;
    return csr_components(G.row_ptr.p, G.col.p, G.n, nullptr, label_out ? *label_out : label_l, "umap_components");
}

long long csr_components(const long long *row_ptr, const int *col, long long n, const int *within, DevBuf<int> &label, const char *timer) {
    Ctx &c = ctx();
    DevBuf<int> prev(n), flag(1);
    label.alloc(n);
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, label.p, prev.p, n);
    launch_check("cc_init_kernel");
    // a sweep at least halves the trees of a path, and a flat tree per component is the fixed point; n sweeps are never needed
    for (long long sweep = 0;; ++sweep) {
        SHARP_REQUIRE(sweep <= n, std::string(timer) + ": the sweeps did not end");
        KernelTimer t(timer);
        int changed = 0;
        flag.zero();
        if (within)
            hipLaunchKernelGGL(cc_hook_kernel<true>, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, row_ptr, col, prev.p, label.p, n, flag.p, within);
        else
            hipLaunchKernelGGL(cc_hook_kernel<false>, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, row_ptr, col, prev.p, label.p, n, flag.p, within);
        launch_check("cc_hook_kernel");
        flag.download(&changed, 1);
        if (!changed) break;
        hipLaunchKernelGGL(cc_jump_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, label.p, prev.p, n);
        launch_check("cc_jump_kernel");
    }
    DevBuf<unsigned long long> count(1);
    count.zero();
    hipLaunchKernelGGL(cc_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, label.p, n, count.p);
    launch_check("cc_count_kernel");
    unsigned long long k = 0;
    count.download(&k, 1);
    return static_cast<long long>(k);
}

void umap_spectral(const UmapGraph &G, int dims, double tol, int max_steps, UmapSpectral &R) {
    Ctx &c = ctx();
    const long long n = G.n;
    SHARP_REQUIRE(dims >= 1 && dims <= 3, "umap_spectral: n_components must be 1, 2 or 3");
    SHARP_REQUIRE(n >= dims + 2 && n < INT_MAX, "umap_spectral: need n_components + 2 <= n < 2^31 rows");
    SHARP_REQUIRE(!std::isnan(tol) && tol < HUGE_VAL, "umap_spectral: tol must be finite (<= 0: the default)");
    if (!(tol > 0.0)) tol = kSpectralTol;
    if (max_steps <= 0) max_steps = kSpectralMaxSteps;
    max_steps = static_cast<int>(std::min<long long>(max_steps, n - 2));
    R = UmapSpectral();
    R.components = umap_components(G);
    if (R.components != 1) { R.outcome = 1; return; }

    KernelTimer timer("umap_spectral");
    const int cols = max_steps + 2;   // q0, q_1 .. q_{max_steps + 1}
    DevBuf<double> s(n), sq(n), u(n), Q(static_cast<size_t>(n) * cols), coef(cols), alpha(max_steps), beta(max_steps + 1);
    DevBuf<double> Vd(static_cast<size_t>(n) * dims), Sd(static_cast<size_t>(max_steps) * dims), scal(4);
    Reducer red(n, cols);
    auto col = [&](int j) { return Q.p + static_cast<long long>(j) * n; };
    // u orthogonalised against the first ncols columns (two classical Gram-Schmidt passes; the first pass's coefficient of the last
    // column to *a when wanted), its norm to *nrm, u / norm to column ncols
    auto extend = [&](int ncols, double *a, double *nrm) {
        red.dots(Q.p, ncols, u.p, coef.p, false, a);
        apply(Q.p, ncols, coef.p, u.p, n);
        red.dots(Q.p, ncols, u.p, coef.p);
        apply(Q.p, ncols, coef.p, u.p, n);
        red.dots(u.p, 1, u.p, nrm, true);
        scale(u.p, nrm, col(ncols), n);
    };
    hipLaunchKernelGGL(degree_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, G.row_ptr.p, G.val.p, n, s.p, sq.p);
    launch_check("degree_kernel");
    red.dots(sq.p, 1, sq.p, scal.p, true);
    scale(sq.p, scal.p, col(0), n);
    hipLaunchKernelGGL(start_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, u.p, n);
    launch_check("start_kernel");
    extend(1, nullptr, beta.p + max_steps);   // (the start's norm goes to the spare slot)

    std::vector<double> ha(max_steps), hb(max_steps + 1), d, e, Z, hS(static_cast<size_t>(max_steps) * dims);
    std::vector<int> ord;
    // the Ritz pairs of T_m: theta (the top dims, descending), their places in d, and the estimates |beta_m S_mj|
    auto solve_T = [&](int m, double bm, int rows) {
        d.assign(ha.begin(), ha.begin() + m);
        e.assign(m, 0.0);
        for (int i = 0; i + 1 < m; ++i) e[i] = hb[i];
        Z.assign(static_cast<size_t>(rows) * m, 0.0);
        for (int r = 0; r < rows; ++r) Z[static_cast<size_t>(r) * m + (m - rows + r)] = 1.0;
        tridiag_ql(m, d, e, Z, rows);
        ord.resize(m);
        for (int i = 0; i < m; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return d[a] > d[b]; });
        for (int j = 0; j < dims; ++j) R.residual[j] = std::fabs(bm * Z[static_cast<size_t>(rows - 1) * m + ord[j]]);
    };
    bool exhausted = false;
    for (int k = 1; k <= max_steps && !exhausted; ++k) {
        spmv(G, s.p, col(k), u.p);
        extend(k + 1, alpha.p + (k - 1), beta.p + (k - 1));
        if (k % kCheckEvery != 0 && k != max_steps) continue;
        alpha.download(ha.data(), k);
        beta.download(hb.data(), k);
        int m = k;
        // beta_j at rounding level: q_1 .. q_j span an invariant subspace, T_j's pairs are exact and nothing lies beyond
        for (int j = 0; j < k; ++j)
            if (!(hb[j] > 64.0 * DBL_EPSILON)) { m = j + 1; exhausted = true; break; }
        R.steps = m;
        if (m < dims) { std::fill(R.residual, R.residual + dims, HUGE_VAL); break; }
        solve_T(m, hb[m - 1], 1);
        bool ok = true;
        for (int j = 0; j < dims; ++j) ok = ok && R.residual[j] <= tol;
        if (!ok) continue;
        solve_T(m, hb[m - 1], m);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < dims; ++j) hS[static_cast<size_t>(i) * dims + j] = Z[static_cast<size_t>(i) * m + ord[j]];
        Sd.upload(hS.data(), static_cast<size_t>(m) * dims);
        const dim3 grid(grid_for(n, 256)), block(256);
        if (dims == 1) hipLaunchKernelGGL(ritz_kernel<1>, grid, block, 0, c.stream, col(1), m, Sd.p, Vd.p, n);
        else if (dims == 2) hipLaunchKernelGGL(ritz_kernel<2>, grid, block, 0, c.stream, col(1), m, Sd.p, Vd.p, n);
        else hipLaunchKernelGGL(ritz_kernel<3>, grid, block, 0, c.stream, col(1), m, Sd.p, Vd.p, n);
        launch_check("ritz_kernel");
        double theta[3], res[3];
        for (int j = 0; j < dims; ++j) {
            double *v = Vd.p + static_cast<long long>(j) * n;
            theta[j] = d[ord[j]];
            red.dots(v, 1, v, scal.p, true);
            scale(v, scal.p, v, n);
            spmv(G, s.p, v, u.p);
            SHARP_HIP_CHECK(hipMemcpyAsync(scal.p + 1, &theta[j], sizeof(double), hipMemcpyHostToDevice, c.stream));
            apply(v, 1, scal.p + 1, u.p, n);
            red.dots(u.p, 1, u.p, scal.p + 2, true);
            SHARP_HIP_CHECK(hipMemcpyAsync(&res[j], scal.p + 2, sizeof(double), hipMemcpyDeviceToHost, c.stream));
            stream_sync();   // (theta[j] and res[j] are pageable host memory in flight)
        }
        ok = true;
        for (int j = 0; j < dims; ++j) { R.residual[j] = res[j]; ok = ok && res[j] <= tol; }
        if (!ok) continue;
        // converged: download, the sign rule (the largest |component| positive, ties by the lowest index), n x dims row-major
        std::vector<double> hv(static_cast<size_t>(n) * dims);
        Vd.download(hv.data(), hv.size());
        R.V.assign(static_cast<size_t>(n) * dims, 0.0);
        for (int j = 0; j < dims; ++j) {
            const double *v = hv.data() + static_cast<size_t>(j) * n;
            long long arg = 0;
            for (long long i = 1; i < n; ++i)
                if (std::fabs(v[i]) > std::fabs(v[arg])) arg = i;
            const double sg = v[arg] < 0 ? -1.0 : 1.0;
            for (long long i = 0; i < n; ++i) R.V[static_cast<size_t>(i) * dims + j] = sg * v[i];
            R.theta[j] = theta[j];
        }
        R.outcome = 0;
        stream_sync();
        return;
    }
    R.outcome = 2;
    stream_sync();   // (the buffers go out of scope)
}

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_umap_components(const long long *row_ptr, const int *col, long long n, int *label, long long *count) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(n >= 1 && n < INT_MAX, "sharp_umap_components: need 1 <= n < 2^31 rows");
    SHARP_REQUIRE(label && count, "sharp_umap_components: null output");
    UmapGraph G;
    upload_csr("sharp_umap_components", row_ptr, col, nullptr, n, G);
    DevBuf<int> dl;
    *count = umap_components(G, &dl);
    dl.download(label, static_cast<size_t>(n));
    SHARP_API_END
}

int sharp_umap_spectral(const long long *row_ptr, const int *col, const double *val, long long n, int dims, double tol, int max_steps, double *V,
                        double *theta, double *residual, int *steps, long long *components, int *outcome) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(dims >= 1 && dims <= 3, "umap_spectral: n_components must be 1, 2 or 3");
    SHARP_REQUIRE(n >= dims + 2 && n < INT_MAX, "umap_spectral: need n_components + 2 <= n < 2^31 rows");
    SHARP_REQUIRE(val && V && theta && residual && steps && components && outcome, "sharp_umap_spectral: null argument");
    UmapGraph G;
    upload_csr("sharp_umap_spectral", row_ptr, col, val, n, G);
    UmapSpectral R;
    umap_spectral(G, dims, tol, max_steps, R);
    *steps = R.steps;
    *components = R.components;
    *outcome = R.outcome;
    if (R.outcome != 1) std::copy(R.residual, R.residual + dims, residual);
    if (R.outcome == 0) {
        std::copy(R.theta, R.theta + dims, theta);
        std::copy(R.V.begin(), R.V.end(), V);
    }
    SHARP_API_END
}

int sharp_umap_init_info(int *requested, int *used, long long *components, int *steps, double *residual) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(requested && used && components && steps && residual, "sharp_umap_init_info: null output");
    const UmapInitInfo &I = umap_init_info();
    *requested = I.requested;
    *used = I.used;
    *components = I.components;
    *steps = I.steps;
    *residual = I.residual;
    SHARP_API_END
}

}  // extern "C"
