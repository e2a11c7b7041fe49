// tsne.hip -- exact t-SNE for visualization_SHARP (R/visualization_SHARP.R:94 hands x1 to Rtsne): DESIGN.md §10.
//   input preparation   column means / sd (slab partials), X^T X on the f64 MFMA as slab partials summed in a fixed order, a host
//                       symmetric eigensolver (Householder tridiagonalisation + implicit QL), the projection X V; centring and division
//                       by the largest |entry|
//   exact k-NN          distances ||w_i||^2 + ||w_j||^2 - 2 w_i.w_j of the centred rows w = x - mean on v_mfma_f64_16x16x4_f64 over streamed
//                       column tiles, a per-row top-K in LDS behind a threshold filter, the chosen K re-ranked by a direct sum (x_i - x_j)^2
//   given distances     Rtsne(is_distance = TRUE): R's dist vector expanded to the full matrix (dist.hip), one wave per row selecting its K
//                       smallest entries through the same LDS list; given neighbours (Rtsne_neighbors): a validation kernel, then
//                       the caller's lists as they are
//   calibration         one wave per row, fp64 bisection on beta (bhtsne's rule)
//   symmetrisation      COO (i, j, p) + (j, i, p), radix sort by (row, col), duplicates merged, normalised by a fixed-order sum -> CSR
//   optimiser loop      attraction over the CSR rows (fp64); exact repulsion, a workgroup owning 256 rows and streaming every y_j through
//                       LDS (fp32 pair terms, fp64 per-tile folds, launches cut so that none exceeds ~1e11 pairs); one update kernel
//                       (gains, velocity, position), mean subtraction, KL every 50 iterations
// No floating-point atomics anywhere; every reduction runs in an order fixed by n alone, so a call is bitwise reproducible.
#include "tsne.hpp"
#include "graph_prim.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

#include "dist_pairs.hpp"
#include "linalg.hpp"
#include "rrng.hpp"

namespace sharp {
namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// column statistics in a fixed order (the sum of a whole vector is graph.hpp's fixed_reduce)
// ---------------------------------------------------------------------------------------------------------------------------
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

// column means (mu == nullptr) or sums of squared deviations / div: out[0..d), device
void column_stat(const double *X, long long n, int d, long long ld, const double *mu, double div, DevBuf<double> &part, double *out) {
    const int nslab = static_cast<int>(std::min<long long>(256, std::max<long long>(1, n / 256)));
    const long long rps = (n + nslab - 1) / nslab;
    part.ensure(static_cast<size_t>(nslab) * d);
    hipLaunchKernelGGL(colsum_kernel, dim3(grid_for(d, 256), nslab), dim3(256), 0, ctx().stream, X, n, d, ld, rps, mu, part.p);
    hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(d, 256)), dim3(256), 0, ctx().stream, part.p, nslab, static_cast<long long>(d), div, out);
    launch_check("colsum_kernel");
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
// the matrix on entry and the eigenvectors (columns) on exit, w the eigenvalues in ascending order
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

void tql2(int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e) {
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
            } while (std::fabs(e[l]) > eps * tst1 && ++guard < 60);
            SHARP_REQUIRE(guard < 60, "Rtsne: the PCA eigensolver did not converge (non-finite input?)");
        }
        d[l] += f;
        e[l] = 0.0;
    }
}

// the k leading eigenvectors of the symmetric G (d x d) as the columns of Vk (d x k, row-major); sign: the largest |component| positive
void leading_eigenvectors(std::vector<double> G, int d, int k, std::vector<double> &Vk) {
    std::vector<double> w(d), e(d);
    tred2(d, G, w, e);
    tql2(d, G, w, e);
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

// ---------------------------------------------------------------------------------------------------------------------------
// exact k-NN
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int KQ = 16;       // query rows per workgroup (one MFMA row block)
constexpr int KCT = 64;      // candidates per column tile (4 waves x 16 MFMA columns)
constexpr int KDT = KCT + 1; // LDS row of the distance tile
constexpr double KNN_INF = 1.0e300;

__device__ __forceinline__ bool lex_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

__global__ __launch_bounds__(256) void rownorm_kernel(const double *__restrict__ X, long long n, int d, double *__restrict__ nrm) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int c = 0; c < d; ++c) { const double t = X[i * d + c]; a += t * t; }
    nrm[i] = a;
}

// Offers a tile of 64 candidates (lane l: distance v, index ci, valid) to one row's top-K list in LDS (Ld / Li, K entries, unsorted; the
// row's current worst (thr, widx) at wpos).  A ballot of (dist, index) < worst leaves the few that enter; each replaces the worst and the
// new worst is found by a wave-wide argmax.  Comparisons are lexicographic on (distance, index): ties go to the lower index.
__device__ __forceinline__ void knn_offer(double v, int ci, bool valid, double *Ld, int *Li, int K, int lane, double &thr, int &widx, int &wpos) {
    unsigned long long m = __ballot(valid && lex_less(v, ci, thr, widx));
    while (m) {
        const int bsel = __ffsll(static_cast<long long>(m)) - 1;
        m &= m - 1;
        const double vb = __shfl(v, bsel);
        const int ib = __shfl(ci, bsel);
        if (!lex_less(vb, ib, thr, widx)) continue;
        if (lane == 0) { Ld[wpos] = vb; Li[wpos] = ib; }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double bd = -1.0;
        int bi = -1, bp = 0;
        for (int p = lane; p < K; p += 64) {
            const double dv = Ld[p];
            const int iv = Li[p];
            if (lex_less(bd, bi, dv, iv)) { bd = dv; bi = iv; bp = p; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(bd, off);
            const int oi = __shfl_xor(bi, off), op = __shfl_xor(bp, off);
            if (lex_less(bd, bi, od, oi)) { bd = od; bi = oi; bp = op; }
        }
        thr = bd;
        widx = bi;
        wpos = bp;   // (lane 0's copy is the one used: a position holding the worst)
    }
}

// Workgroup (blockIdx.x, blockIdx.y): KQ query rows [q0, q0 + 16) against the candidate columns of chunk blockIdx.y, tile by tile of KCT.
// Wave w computes the 16 x 16 block of columns c0 + 16 w .. + 16 on the f64 MFMA (C/D: row (lane >> 4) + 4 r, column lane & 15) into the
// LDS tile; then wave w offers them to rows 4w .. 4w + 3.  The chunk's top-K of every row (GEMM distances, unsorted; sentinels
// (KNN_INF, INT_MAX) where the chunk holds fewer than K candidates) goes to part[(chunk * rows + r) * K ..].
__global__ __launch_bounds__(256) void knn_kernel(const double *__restrict__ X, const double *__restrict__ nrm, long long n, int d, int K,
                                                  long long row0, long long row_end, long long cj, int *__restrict__ part_idx,
                                                  double *__restrict__ part_dist) {
    extern __shared__ double smem[];
    double *dt = smem;                              // [KQ][KDT]
    double *Ld = dt + KQ * KDT;                     // [KQ][K]
    int *Li = reinterpret_cast<int *>(Ld + KQ * K);   // [KQ][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long q0 = row0 + static_cast<long long>(blockIdx.x) * KQ, rows = row_end - row0;
    const long long cbeg = static_cast<long long>(blockIdx.y) * cj, cend = cbeg + cj < n ? cbeg + cj : n;
    for (int e = tid; e < KQ * K; e += 256) { Ld[e] = KNN_INF; Li[e] = INT_MAX; }
    double thr[4];
    int widx[4], wpos[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { thr[r] = KNN_INF; widx[r] = INT_MAX; wpos[r] = 0; }
    const long long qa = q0 + (lane & 15);
    const bool qa_ok = qa < row_end;
    double nq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long qq = q0 + (lane >> 4) + 4 * r;
        nq[r] = qq < row_end ? nrm[qq] : 0.0;
    }
    __syncthreads();
    for (long long c0 = cbeg; c0 < cend; c0 += KCT) {
        const long long cb = c0 + wave * 16 + (lane & 15);
        const bool cb_ok = cb < cend;
        v4f64 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < d; k0 += 4) {
            const int k = k0 + (lane >> 4);
            const double a = (qa_ok && k < d) ? X[qa * d + k] : 0.0;
            const double b = (cb_ok && k < d) ? X[cb * d + k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        const double nc = cb_ok ? nrm[cb] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (lane >> 4) + 4 * r;
            dt[row * KDT + wave * 16 + (lane & 15)] = nq[r] + nc - 2.0 * acc[r];
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = wave * 4 + rr;
            const long long qq = q0 + row;
            if (qq >= row_end) continue;
            const long long ci = c0 + lane;
            knn_offer(dt[row * KDT + lane], static_cast<int>(ci), ci < cend && ci != qq, Ld + row * K, Li + row * K, K, lane, thr[rr], widx[rr],
                      wpos[rr]);
        }
        __syncthreads();
    }
    for (int e = tid; e < KQ * K; e += 256) {
        const long long r = q0 - row0 + e / K;
        if (r < rows) {
            part_idx[(static_cast<long long>(blockIdx.y) * rows + r) * K + e % K] = Li[e];
            part_dist[(static_cast<long long>(blockIdx.y) * rows + r) * K + e % K] = Ld[e];
        }
    }
}

// One wave per row of the launch: the K best of the chunks' lists (nc x K candidates, chunk after chunk), re-ranked by the direct sum
// (x_i - x_j)^2 and sorted by (distance, index).  A row left with a sentinel (no finite distance to enough rows) sets *bad and writes
// nothing it would have to read X for.
__global__ __launch_bounds__(256) void knn_merge_kernel(const double *__restrict__ X, long long n, int d, int K, long long row0, long long rows,
                                                        int nc, const int *__restrict__ part_idx, const double *__restrict__ part_dist,
                                                        int *__restrict__ out_idx, double *__restrict__ out_dist, int *__restrict__ bad) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *Ld = smem + wave * K;                                  // [4][K] doubles, then [4][K] ints
    int *Li = reinterpret_cast<int *>(smem + 4 * K) + wave * K;
    const long long r = static_cast<long long>(blockIdx.x) * 4 + wave, qq = row0 + r;
    if (r >= rows || qq >= n) return;
    for (int p = lane; p < K; p += 64) { Ld[p] = KNN_INF; Li[p] = INT_MAX; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double thr = KNN_INF;
    int widx = INT_MAX, wpos = 0;
    for (int c = 0; c < nc; ++c) {
        const long long base = (static_cast<long long>(c) * rows + r) * K;
        for (int t = 0; t < K; t += 64) {
            const bool in = t + lane < K;
            const int ci = in ? part_idx[base + t + lane] : INT_MAX;
            const double v = in ? part_dist[base + t + lane] : KNN_INF;
            knn_offer(v, ci, in && ci >= 0 && ci < n, Ld, Li, K, lane, thr, widx, wpos);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int p = lane; p < K; p += 64) {
        const int j = Li[p];
        double s = KNN_INF;
        if (j >= 0 && j < n) {
            s = 0.0;
            for (int c = 0; c < d; ++c) { const double t = X[qq * d + c] - X[static_cast<long long>(j) * d + c]; s += t * t; }
        } else {
            *bad = 1;   // every writer stores the same value
        }
        Ld[p] = s;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p];
        int rank = 0;
        for (int q = 0; q < K; ++q) rank += lex_less(Ld[q], Li[q], dp, ip) ? 1 : 0;
        out_idx[qq * K + rank] = ip < n ? ip : -1;
        out_dist[qq * K + rank] = dp;
    }
}

// *bad = 1 when a row norm is not finite or so large that a squared distance could overflow (NaN / Inf / huge input)
__global__ __launch_bounds__(256) void norm_check_kernel(const double *__restrict__ nrm, long long n, int *__restrict__ bad) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && !(nrm[i] <= 0.125 * DBL_MAX)) *bad = 1;   // (false for NaN too)
}

__global__ __launch_bounds__(256) void dup_flag_kernel(const double *__restrict__ dist, long long n, int K, int *__restrict__ flag) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && dist[i * K] == 0.0) *flag = 1;   // every writer stores the same value
}

// ---------------------------------------------------------------------------------------------------------------------------
// neighbours that are given, or selected from given distances (DESIGN.md §10 "Given neighbours, given distances")
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int NN_RS = 8;     // 64-wide loads in flight per lane before their offers (hclust_agglo.hip's HC_RS idea)
constexpr unsigned long long NN_OK = ~0ull;
enum NnKind { NN_RANGE = 1, NN_SELF = 2, NN_TWICE = 3, NN_DIST = 4 };

// One wave per row r of the full symmetric matrix D (nld x nld, as dist_expand_kernel writes it): the K smallest (D[r][c], c) over
// c < n, c != r, lexicographic (ties to the lower index), through knn_offer on an LDS list; then ranked by (distance, index) and written
// as idx and dist2 = d * d.  Selection is on the distances as given.  A row left with a sentinel or a square that overflows sets *bad.
__global__ __launch_bounds__(256) void knn_rows_kernel(const double *__restrict__ D, int n, int nld, int K, int *__restrict__ out_idx,
                                                       double *__restrict__ out_dist2, int *__restrict__ bad) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *Ld = smem + wave * K;                                  // [4][K] doubles, then [4][K] ints
    int *Li = reinterpret_cast<int *>(smem + 4 * K) + wave * K;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n) return;
    for (int p = lane; p < K; p += 64) { Ld[p] = KNN_INF; Li[p] = INT_MAX; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double thr = KNN_INF;
    int widx = INT_MAX, wpos = 0;
    const double *row = D + static_cast<long long>(r) * nld;
    for (int c0 = 0; c0 < n; c0 += 64 * NN_RS) {
        double v[NN_RS];
#pragma unroll
        for (int u = 0; u < NN_RS; ++u) { const int c = c0 + 64 * u + lane; v[u] = c < n ? row[c] : KNN_INF; }
#pragma unroll
        for (int u = 0; u < NN_RS; ++u) {
            const int c = c0 + 64 * u + lane;
            if (c0 + 64 * u < n) knn_offer(v[u], c, c < n && c != r, Ld, Li, K, lane, thr, widx, wpos);   // (wave-uniform condition)
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p];
        int rank = 0;
        for (int q = 0; q < K; ++q) rank += lex_less(Ld[q], Li[q], dp, ip) ? 1 : 0;
        const double d2 = dp * dp;
        if (ip >= n || !(d2 <= DBL_MAX)) { *bad = 1; continue; }   // every writer stores the same value
        out_idx[static_cast<long long>(r) * K + rank] = ip;
        out_dist2[static_cast<long long>(r) * K + rank] = d2;
    }
}

// One wave per row of a caller's neighbour lists, before anything dereferences an index: every index in [0, n), none its own row, none
// twice in a row, every distance finite and >= 0.  *word = min over the offending rows of (row << 3 | kind): the first offending row
// and its lowest kind, whatever the scheduling.
__global__ __launch_bounds__(256) void nn_check_kernel(const int *__restrict__ idx, const double *__restrict__ dist, long long n, int K,
                                                       unsigned long long *__restrict__ word) {
    extern __shared__ int sidx[];                                  // [4][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int *Li = sidx + wave * K;
    const long long r = static_cast<long long>(blockIdx.x) * 4 + wave;
    if (r >= n) return;
    int kind = 8;
    for (int p = lane; p < K; p += 64) {
        const int j = idx[r * K + p];
        const double d = dist[r * K + p];
        Li[p] = j;
        if (j < 0 || j >= n) kind = min(kind, static_cast<int>(NN_RANGE));
        else if (j == r) kind = min(kind, static_cast<int>(NN_SELF));
        if (!(d >= 0.0 && d <= DBL_MAX)) kind = min(kind, static_cast<int>(NN_DIST));   // (false for NaN too)
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int p = lane; p < K; p += 64) {
        const int j = Li[p];
        for (int q = 0; q < p; ++q)
            if (Li[q] == j) { kind = min(kind, static_cast<int>(NN_TWICE)); break; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kind = min(kind, __shfl_xor(kind, off));
    if (lane == 0 && kind < 8) atomicMin(word, (static_cast<unsigned long long>(r) << 3) | static_cast<unsigned long long>(kind));
}

__global__ __launch_bounds__(256) void square_kernel(double *__restrict__ v, long long n, int *__restrict__ bad) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n) return;
    const double s = v[e] * v[e];
    if (!(s <= DBL_MAX)) *bad = 1;   // every writer stores the same value
    v[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// perplexity calibration: one wave per row, fp64 (bhtsne's bisection: beta from 1, doubling / halving while a bound is open, tol 1e-5
// on the entropy in nats, at most 200 steps)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void calib_kernel(const double *__restrict__ dist, long long n, int K, double logU, double *__restrict__ P) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double dv[4], pv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int p = lane + 64 * t; dv[t] = p < K ? dist[i * K + p] : 0.0; pv[t] = 0.0; }
    double beta = 1.0, minb = -DBL_MAX, maxb = DBL_MAX, sumP = DBL_MIN;
    for (int it = 0; it < 200; ++it) {
        double s = 0.0, h = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pv[t] = lane + 64 * t < K ? exp(-beta * dv[t]) : 0.0;
            s += pv[t];
            h += beta * (dv[t] * pv[t]);
        }
        s = wave_sum(s);
        h = wave_sum(h);
        sumP = DBL_MIN + s;
        const double Hdiff = (h / sumP + log(sumP)) - logU;
        if (Hdiff < 1e-5 && -Hdiff < 1e-5) break;
        if (Hdiff > 0) {
            minb = beta;
            beta = (maxb == DBL_MAX || maxb == -DBL_MAX) ? beta * 2.0 : (beta + maxb) / 2.0;
        } else {
            maxb = beta;
            beta = (minb == -DBL_MAX || minb == DBL_MAX) ? beta / 2.0 : (beta + minb) / 2.0;
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = lane + 64 * t;
        if (p < K) P[i * K + p] = pv[t] / sumP;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// symmetrisation
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coo_kernel(const int *__restrict__ idx, const double *__restrict__ Pc, long long n, int K,
                                                  unsigned long long *__restrict__ keys, double *__restrict__ vals) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * K) return;
    const unsigned long long i = static_cast<unsigned long long>(e / K), j = static_cast<unsigned long long>(idx[e]);
    const double p = Pc[e];
    keys[2 * e] = i * static_cast<unsigned long long>(n) + j;
    vals[2 * e] = p;
    keys[2 * e + 1] = j * static_cast<unsigned long long>(n) + i;
    vals[2 * e + 1] = p;
}

__global__ __launch_bounds__(256) void scale_kernel(double *__restrict__ v, long long n, double f, int divide) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < n) v[e] = divide ? v[e] / f : v[e] * f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// gradient: attraction (CSR rows, fp64), exact repulsion (fp32 pair terms, fp64 folds), Z
// ---------------------------------------------------------------------------------------------------------------------------
template <int DIMS>
__global__ __launch_bounds__(256) void attr_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                   const double *__restrict__ Y, long long n, double *__restrict__ attr) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double yi[DIMS], acc[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { yi[k] = Y[i * DIMS + k]; acc[k] = 0.0; }
    for (long long e = rp[i]; e < rp[i + 1]; ++e) {
        const long long j = col[e];
        double diff[DIMS], D = 1.0;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) { diff[k] = yi[k] - Y[j * DIMS + k]; D += diff[k] * diff[k]; }
        D = val[e] / D;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) acc[k] += D * diff[k];
    }
#pragma unroll
    for (int k = 0; k < DIMS; ++k) attr[i * DIMS + k] = acc[k];
}

constexpr int RT = 256;                 // rows per workgroup and points per LDS tile of the repulsion
constexpr double kPairsPerLaunch = 1e11;  // ~25 ms at the arithmetic rate: no repulsion launch near 0.1 s at any n

// Workgroup (blockIdx.x, blockIdx.y): rows row0 + 256 blockIdx.x + tid against the columns of chunk blockIdx.y, 256 points per LDS tile.
// Per pair (fp32, explicit fmaf): d = y_i - y_j, q = 1 / (1 + |d|^2), z += q, f += q^2 d.  Each tile's fp32 partials are folded into
// fp64; the self pair (q = 1, d = 0) is taken out of z in fp64.  part[(chunk * rows + r) * 4 + k]: f_k (k < DIMS), z (k = DIMS).
template <int DIMS>
__global__ __launch_bounds__(256) void rep_kernel(const float *__restrict__ Yf, long long n, long long row0, long long rows, long long cj,
                                                  double *__restrict__ part) {
    __shared__ float ys[RT * DIMS];
    const int tid = threadIdx.x;
    const long long r = static_cast<long long>(blockIdx.x) * RT + tid, i = row0 + r;
    const bool active = r < rows && i < n;
    float yi[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) yi[k] = active ? Yf[i * DIMS + k] : 0.0f;
    double F[DIMS + 1];
#pragma unroll
    for (int k = 0; k <= DIMS; ++k) F[k] = 0.0;
    const long long jb = static_cast<long long>(blockIdx.y) * cj, je = jb + cj < n ? jb + cj : n;
    for (long long t0 = jb; t0 < je; t0 += RT) {
        const int cnt = static_cast<int>(je - t0 < RT ? je - t0 : RT);
        __syncthreads();
        for (int e = tid; e < cnt * DIMS; e += RT) ys[e] = Yf[t0 * DIMS + e];
        __syncthreads();
        float f[DIMS], z = 0.0f;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) f[k] = 0.0f;
#pragma unroll 8
        for (int jj = 0; jj < cnt; ++jj) {
            float dv[DIMS], d2 = 0.0f;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) { dv[k] = yi[k] - ys[jj * DIMS + k]; d2 = fmaf(dv[k], dv[k], d2); }
            const float q = __builtin_amdgcn_rcpf(1.0f + d2);
            z += q;
            const float q2 = q * q;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) f[k] = fmaf(q2, dv[k], f[k]);
        }
#pragma unroll
        for (int k = 0; k < DIMS; ++k) F[k] += static_cast<double>(f[k]);
        F[DIMS] += static_cast<double>(z);
        if (i >= t0 && i < t0 + cnt) F[DIMS] -= 1.0;
    }
    if (r < rows) {
#pragma unroll
        for (int k = 0; k <= DIMS; ++k) part[(static_cast<long long>(blockIdx.y) * rows + r) * 4 + k] = F[k];
    }
}

template <int DIMS>
__global__ __launch_bounds__(256) void fold_kernel(const double *__restrict__ part, int nc, long long row0, long long rows, long long n,
                                                   double *__restrict__ rep, double *__restrict__ zrow) {
    const long long r = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x, i = row0 + r;
    if (r >= rows || i >= n) return;
    double F[DIMS + 1];
#pragma unroll
    for (int k = 0; k <= DIMS; ++k) F[k] = 0.0;
    for (int c = 0; c < nc; ++c)
#pragma unroll
        for (int k = 0; k <= DIMS; ++k) F[k] += part[(static_cast<long long>(c) * rows + r) * 4 + k];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) rep[i * DIMS + k] = F[k];
    zrow[i] = F[DIMS];
}

template <int DIMS>
__global__ __launch_bounds__(256) void grad_kernel(const double *__restrict__ attr, const double *__restrict__ rep, const double *__restrict__ Z,
                                                   long long ne, double *__restrict__ dY) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < ne) dY[e] = attr[e] - rep[e] / Z[0];
}

__device__ __forceinline__ double sgn(double x) { return x == 0.0 ? 0.0 : (x < 0.0 ? -1.0 : 1.0); }

// gains, velocity and position of one coordinate
__global__ __launch_bounds__(256) void update_kernel(const double *__restrict__ attr, const double *__restrict__ rep, const double *__restrict__ Z,
                                                     long long ne, double momentum, double eta, double *__restrict__ gains,
                                                     double *__restrict__ uY, double *__restrict__ Y) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= ne) return;
    const double dY = attr[e] - rep[e] / Z[0];
    double g = gains[e];
    const double u = uY[e];
    g = sgn(dY) != sgn(u) ? g + 0.2 : g * 0.8;
    if (g < 0.01) g = 0.01;
    gains[e] = g;
    const double un = momentum * u - eta * g * dY;
    uY[e] = un;
    Y[e] = Y[e] + un;
}

// Y -= mean (when mean), and the fp32 copy the repulsion reads
template <int DIMS>
__global__ __launch_bounds__(256) void center_kernel(double *__restrict__ Y, long long n, const double *__restrict__ mean, float *__restrict__ Yf) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * DIMS) return;
    double v = Y[e];
    if (mean) { v = v - mean[e % DIMS]; Y[e] = v; }
    Yf[e] = static_cast<float>(v);
}

// per-row KL: sum_j P_ij log((P_ij + FLT_MIN) / (q_ij / Z + FLT_MIN))
template <int DIMS>
__global__ __launch_bounds__(256) void kl_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                 const double *__restrict__ Y, long long n, const double *__restrict__ Z, double *__restrict__ kl) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double yi[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) yi[k] = Y[i * DIMS + k];
    const double z = Z[0];
    double c = 0.0;
    for (long long e = rp[i]; e < rp[i + 1]; ++e) {
        const long long j = col[e];
        double D = 1.0;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) { const double t = yi[k] - Y[j * DIMS + k]; D += t * t; }
        const double Q = (1.0 / D) / z;
        c += val[e] * log((val[e] + FLT_MIN) / (Q + FLT_MIN));
    }
    kl[i] = c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Barnes-Hut repulsion (DESIGN.md §10 "Barnes-Hut"): bhtsne's SPTree as a compressed 2^DIMS-ary tree over quantised Morton keys,
// rebuilt from the fp64 Y at every gradient evaluation and laid out in preorder with a skip index per node, so that one lane per point
// walks it without a stack.  fp64 throughout; every sum in an order fixed by n and the keys; no atomics, no inter-workgroup flags.
// ---------------------------------------------------------------------------------------------------------------------------
template <int DIMS> struct BhBits { static constexpr int value = DIMS == 1 ? 63 : (DIMS == 2 ? 32 : 21); };   // levels below the root
constexpr int kBhSlabs = 256;        // slabs of the bounding-box reduction
constexpr int kBhRadix = 32;         // chunk length of the layered sums behind the centres of mass
constexpr int kBhMaxLayers = 8;      // 32^7 > 2^31 rows
constexpr unsigned kBhInternal = 0xFFFFFFFFu;   // meta.z of an internal node (a leaf holds its lowest point index there)

// layer 0: the sorted Y (n x DIMS); layer l + 1: sums of kBhRadix consecutive entries of layer l, in order
struct BhLayers {
    const double *p[kBhMaxLayers];
    long long len[kBhMaxLayers];
    int nl;
};

// slab b: per-dimension sum, min and max of Y's rows [b rps, (b + 1) rps) -> part[b * 3 DIMS + {k, DIMS + k, 2 DIMS + k}]
template <int DIMS>
__global__ __launch_bounds__(256) void bh_bounds_kernel(const double *__restrict__ Y, long long n, long long rps, double *__restrict__ part) {
    __shared__ double s[3 * DIMS][256];
    const int tid = threadIdx.x;
    const long long r0 = static_cast<long long>(blockIdx.x) * rps, r1 = r0 + rps < n ? r0 + rps : n;
    double a[3 * DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { a[k] = 0.0; a[DIMS + k] = DBL_MAX; a[2 * DIMS + k] = -DBL_MAX; }
    for (long long r = r0 + tid; r < r1; r += 256)
#pragma unroll
        for (int k = 0; k < DIMS; ++k) {
            const double v = Y[r * DIMS + k];
            a[k] += v;
            a[DIMS + k] = fmin(a[DIMS + k], v);
            a[2 * DIMS + k] = fmax(a[2 * DIMS + k], v);
        }
#pragma unroll
    for (int k = 0; k < 3 * DIMS; ++k) s[k][tid] = a[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int k = 0; k < DIMS; ++k) {
                s[k][tid] += s[k][tid + w];
                s[DIMS + k][tid] = fmin(s[DIMS + k][tid], s[DIMS + k][tid + w]);
                s[2 * DIMS + k][tid] = fmax(s[2 * DIMS + k][tid], s[2 * DIMS + k][tid + w]);
            }
        __syncthreads();
    }
    if (tid < 3 * DIMS) part[static_cast<long long>(blockIdx.x) * 3 * DIMS + tid] = s[tid][0];
}

// the root cell (bhtsne's SPTree constructor): centre = mean, half-width w_d = max(max - mean, mean - min) + 1e-5.
// root[3 + k] = mean - w (the lower corner), root[6 + k] = 2^bits / (2 w) (finest cells per unit), root[9] = max_d w_d
template <int DIMS>
__global__ void bh_root_kernel(const double *__restrict__ part, int nslab, long long n, double *__restrict__ root) {
    if (threadIdx.x != 0) return;
    double wmax = 0.0;
    for (int k = 0; k < DIMS; ++k) {
        double sum = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
        for (int b = 0; b < nslab; ++b) {
            sum += part[b * 3 * DIMS + k];
            mn = fmin(mn, part[b * 3 * DIMS + DIMS + k]);
            mx = fmax(mx, part[b * 3 * DIMS + 2 * DIMS + k]);
        }
        const double mean = sum / static_cast<double>(n);
        const double w = fmax(mx - mean, mean - mn) + 1e-5;
        root[k] = mean;
        root[3 + k] = mean - w;
        root[6 + k] = ldexp(1.0, BhBits<DIMS>::value) / (2.0 * w);
        wmax = fmax(wmax, w);
    }
    root[9] = wmax;
}

// key[i]: the finest cell of y_i as a Morton key.  Per dimension c = floor((y - lower corner) * cells per unit), clamped to the grid
// (a point on a midline goes to the upper half), then inverted so that the upper half sorts first: digit L (from the top) holds bit
// (bits - L) of every dimension, dimension k at bit k -- bhtsne's child number, so ascending keys visit children in bhtsne's order.
template <int DIMS>
__global__ __launch_bounds__(256) void bh_key_kernel(const double *__restrict__ Y, long long n, const double *__restrict__ root,
                                                     unsigned long long *__restrict__ key) {
    constexpr int bits = BhBits<DIMS>::value;
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double lim = ldexp(1.0, bits);
    const unsigned long long top = (1ull << bits) - 1ull;
    unsigned long long c[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) {
        const double t = (Y[i * DIMS + k] - root[3 + k]) * root[6 + k];
        const unsigned long long u = t >= lim ? top : (t >= 0.0 ? static_cast<unsigned long long>(t) : 0ull);   // (NaN: 0)
        c[k] = top - u;
    }
    unsigned long long K = 0;
    for (int b = bits - 1; b >= 0; --b)
#pragma unroll
        for (int k = 0; k < DIMS; ++k) K |= ((c[k] >> b) & 1ull) << (b * DIMS + k);
    key[i] = K;
}

template <int DIMS>
__global__ __launch_bounds__(256) void bh_gather_kernel(const double *__restrict__ Y, const int *__restrict__ perm, long long n, double *__restrict__ Ys) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * DIMS) return;
    const long long s = e / DIMS;
    Ys[e] = Y[static_cast<long long>(perm[s]) * DIMS + (e - s * DIMS)];
}

template <int DIMS>
__global__ __launch_bounds__(256) void bh_layer_kernel(const double *__restrict__ in, long long len_in, double *__restrict__ out, long long len_out) {
    const long long c = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (c >= len_out) return;
    const long long t0 = c * kBhRadix, t1 = t0 + kBhRadix < len_in ? t0 + kBhRadix : len_in;
    double a[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) a[k] = 0.0;
    for (long long t = t0; t < t1; ++t)
#pragma unroll
        for (int k = 0; k < DIMS; ++k) a[k] += in[t * DIMS + k];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) out[c * DIMS + k] = a[k];
}

// sum of sorted rows [a, b) from the layers: the partial chunks at each end of a layer, then the whole chunks one layer up
template <int DIMS>
__device__ void bh_range_sum(const BhLayers &Ls, long long a, long long b, double *acc) {
    for (int l = 0;; ++l) {
        const double *p = Ls.p[l];
        const long long au = (a + kBhRadix - 1) / kBhRadix * kBhRadix, bd = b / kBhRadix * kBhRadix;
        if (l + 1 >= Ls.nl || au >= bd) {
            for (long long t = a; t < b; ++t)
#pragma unroll
                for (int k = 0; k < DIMS; ++k) acc[k] += p[t * DIMS + k];
            return;
        }
        for (long long t = a; t < au; ++t)
#pragma unroll
            for (int k = 0; k < DIMS; ++k) acc[k] += p[t * DIMS + k];
        for (long long t = bd; t < b; ++t)
#pragma unroll
            for (int k = 0; k < DIMS; ++k) acc[k] += p[t * DIMS + k];
        a = au / kBhRadix;
        b = bd / kBhRadix;
    }
}

// leading digits two keys share (bits when they are equal)
template <int DIMS>
__device__ __forceinline__ int bh_lcp(unsigned long long a, unsigned long long b) {
    if (a == b) return BhBits<DIMS>::value;
    return BhBits<DIMS>::value - 1 - (63 - __builtin_clzll(a ^ b)) / DIMS;
}

// the first sorted position after s outside the level-L cell of key[s]: galloping, then bisection
template <int DIMS>
__device__ long long bh_cell_end(const unsigned long long *__restrict__ key, long long n, long long s, int L) {
    if (L == 0) return n;
    const unsigned long long v = key[s] | ((1ull << ((BhBits<DIMS>::value - L) * DIMS)) - 1ull);
    long long a = s, b, step = 1;   // key[a] <= v; key[b] > v or b == n
    for (;;) {
        b = a + step;
        if (b >= n) { b = n; break; }
        if (key[b] > v) break;
        a = b;
        step *= 2;
    }
    while (b - a > 1) {
        const long long m = a + (b - a) / 2;
        if (key[m] <= v) a = m; else b = m;
    }
    return b;
}

// The nodes of the compressed tree that start at the sorted position s of a run of equal keys: f(level, end) for each internal node,
// outermost first (a chain of cells with one non-empty child is one node, at the level of its deepest cell), then f(bits, end) for the
// leaf, the run itself.  Cells at levels <= lcp(key[s - 1], key[s]) start before s.
template <int DIMS, class F>
__device__ void bh_chain(const unsigned long long *__restrict__ key, long long n, long long s, F f) {
    constexpr int bits = BhBits<DIMS>::value;
    int L = s == 0 ? 0 : bh_lcp<DIMS>(key[s - 1], key[s]) + 1;
    while (L < bits) {
        const long long e = bh_cell_end<DIMS>(key, n, s, L);
        const int g = bh_lcp<DIMS>(key[s], key[e - 1]);   // the deepest level of the chain: its cells all hold [s, e)
        if (g >= bits) break;
        f(g, e);
        L = g + 1;
    }
    f(bits, bh_cell_end<DIMS>(key, n, s, bits));
}

__device__ __forceinline__ bool bh_run_start(const unsigned long long *__restrict__ key, long long s) { return s == 0 || key[s] != key[s - 1]; }

// cnt[s]: nodes that start at sorted position s (0 unless s starts a run; cnt[n] = 0)
template <int DIMS>
__global__ __launch_bounds__(256) void bh_count_kernel(const unsigned long long *__restrict__ key, long long n, unsigned *__restrict__ cnt) {
    const long long s = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s > n) return;
    unsigned c = 0;
    if (s < n && bh_run_start(key, s)) bh_chain<DIMS>(key, n, s, [&](int, long long) { ++c; });
    cnt[s] = c;
}

// The nodes in preorder: those starting at s go to off[s], off[s] + 1, ... (off: exclusive scan of cnt, off[n] = node count).  A node
// holding sorted rows [s, e) skips to off[e], the first node that starts at or after e.  meta = (points, skip, lowest point index of a
// leaf or kBhInternal, level); com: the centre of mass (fp64 sum from the layers / count).
template <int DIMS>
__global__ __launch_bounds__(256) void bh_node_kernel(const unsigned long long *__restrict__ key, const int *__restrict__ perm, long long n,
                                                      const unsigned *__restrict__ off, BhLayers Ls, uint4 *__restrict__ meta,
                                                      double *__restrict__ com) {
    const long long s = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= n || !bh_run_start(key, s)) return;
    unsigned o = off[s];
    bh_chain<DIMS>(key, n, s, [&](int level, long long e) {
        const bool leaf = level == BhBits<DIMS>::value;
        meta[o] = make_uint4(static_cast<unsigned>(e - s), off[e], leaf ? static_cast<unsigned>(perm[s]) : kBhInternal, static_cast<unsigned>(level));
        double acc[DIMS];
#pragma unroll
        for (int k = 0; k < DIMS; ++k) acc[k] = 0.0;
        bh_range_sum<DIMS>(Ls, s, e, acc);
#pragma unroll
        for (int k = 0; k < DIMS; ++k) com[static_cast<size_t>(o) * DIMS + k] = acc[k] / static_cast<double>(e - s);
        ++o;
    });
}

// One lane per point, lanes in sorted-key order: bhtsne's computeNonEdgeForces over the preorder layout.  A leaf whose lowest index is
// i is skipped; a leaf, or an internal node with max_d(half-width) / sqrt(D) < theta, is a summary (cnt q to z, cnt q^2 (y_i - com) to
// the repulsion; k = skip); otherwise the walk enters its first child (k + 1).  rep / zrow as rep_kernel + fold_kernel leave them.
template <int DIMS>
__global__ __launch_bounds__(256) void bh_walk_kernel(const double *__restrict__ Ys, const int *__restrict__ perm, long long n,
                                                      const uint4 *__restrict__ meta, const double *__restrict__ com,
                                                      const double *__restrict__ root, double theta, double *__restrict__ rep,
                                                      double *__restrict__ zrow) {
    const long long s = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= n) return;
    const unsigned i = static_cast<unsigned>(perm[s]);
    double yi[DIMS], f[DIMS], z = 0.0;
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { yi[k] = Ys[s * DIMS + k]; f[k] = 0.0; }
    const double wmax = root[9];
    const unsigned M = meta[0].y;   // the root's skip: the node count
    unsigned k = 0;
    while (k < M) {
        const uint4 m = meta[k];
        if (m.z == i) { k = m.y; continue; }
        double d[DIMS], D = 0.0;
#pragma unroll
        for (int c = 0; c < DIMS; ++c) { d[c] = yi[c] - com[static_cast<size_t>(k) * DIMS + c]; D += d[c] * d[c]; }
        if (m.z != kBhInternal || ldexp(wmax, -static_cast<int>(m.w)) / sqrt(D) < theta) {
            const double q = 1.0 / (1.0 + D);
            double mult = static_cast<double>(m.x) * q;
            z += mult;
            mult *= q;
#pragma unroll
            for (int c = 0; c < DIMS; ++c) f[c] += mult * d[c];
            k = m.y;
        } else {
            ++k;
        }
    }
#pragma unroll
    for (int c = 0; c < DIMS; ++c) rep[static_cast<long long>(i) * DIMS + c] = f[c];
    zrow[i] = z;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------------------------------------
struct RepPlan {
    long long rows = 0, cj = 0;   // rows per launch, columns per chunk
    int nc = 1;                   // chunks
};

RepPlan rep_plan(long long n) {
    RepPlan p;
    const long long n_up = (n + RT - 1) / RT * RT;
    long long rows = static_cast<long long>(kPairsPerLaunch / static_cast<double>(std::max<long long>(n, 1))) / RT * RT;
    p.rows = std::min(n_up, std::max<long long>(RT, rows));
    const long long rb = (p.rows + RT - 1) / RT;
    long long nc = std::max<long long>(1, std::min<long long>((n + RT - 1) / RT, (2048 + rb - 1) / rb));   // >= ~2048 workgroups per launch
    p.cj = ((n + nc - 1) / nc + RT - 1) / RT * RT;
    p.nc = static_cast<int>((n + p.cj - 1) / p.cj);
    return p;
}

// the Barnes-Hut tree's buffers, allocated once per call (at most 2n - 1 nodes)
struct BhTree {
    DevBuf<unsigned long long> key, key_s;
    DevBuf<int> iota, perm;
    DevBuf<double> Ys, lay, part, root, com;
    DevBuf<unsigned> cnt, off;
    DevBuf<uint4> meta;
    Scratch sort_tmp, scan_tmp;   // (sized by the first build, reused by every later one: the counts do not change)
    BhLayers L{};
    int nslab = 1, end_bit = 64;
    long long rps = 1;
    void init(long long n, int dims) {
        const size_t nn = static_cast<size_t>(n);
        key.alloc(nn); key_s.alloc(nn); iota.alloc(nn); perm.alloc(nn);
        Ys.alloc(nn * dims);
        cnt.alloc(nn + 1); off.alloc(nn + 1);
        meta.alloc(2 * nn); com.alloc(2 * nn * dims);
        root.alloc(16);
        nslab = static_cast<int>(std::min<long long>(kBhSlabs, std::max<long long>(1, n / 256)));
        rps = (n + nslab - 1) / nslab;
        nslab = static_cast<int>((n + rps - 1) / rps);
        part.alloc(static_cast<size_t>(nslab) * 3 * dims);
        std::vector<long long> len{n}, at{0};
        long long total = 0;
        while (len.back() > kBhRadix) {
            at.push_back(total);
            len.push_back((len.back() + kBhRadix - 1) / kBhRadix);
            total += len.back();
        }
        SHARP_REQUIRE(len.size() <= static_cast<size_t>(kBhMaxLayers), "tsne_bh: too many rows");
        lay.alloc(std::max<size_t>(1, static_cast<size_t>(total) * dims));
        L.nl = static_cast<int>(len.size());
        for (int l = 0; l < L.nl; ++l) {
            L.len[l] = len[l];
            L.p[l] = l == 0 ? Ys.p : lay.p + at[l] * dims;
        }
        end_bit = dims == 1 ? 63 : (dims == 2 ? 64 : 63);
        sharp::iota(iota.p, n);
    }
};

struct Work {
    long long n = 0;
    int dims = 2;
    RepPlan plan;
    DevBuf<double> Y, uY, gains, attr, rep, zrow, kl, part, red, scal, colpart;   // scal: [0] Z, [1] KL sum, [2..] mean
    DevBuf<float> Yf;
    double theta = 0.0;   // > 0: the Barnes-Hut repulsion with this theta instead of the exact one
    BhTree bh;
    void init(long long n_, int dims_, double theta_ = 0.0) {
        n = n_;
        dims = dims_;
        theta = theta_;
        plan = rep_plan(n);
        const size_t ne = static_cast<size_t>(n) * dims;
        Y.alloc(ne); uY.alloc(ne); gains.alloc(ne); attr.alloc(ne); rep.alloc(ne); Yf.alloc(ne);
        zrow.alloc(n); kl.alloc(n);
        if (theta > 0.0) bh.init(n, dims);
        else part.alloc(static_cast<size_t>(plan.nc) * plan.rows * 4);
        red.alloc(kRedBlocks);
        scal.alloc(8);
    }
};

// the tree at the current Y (DESIGN.md §10 "Barnes-Hut"): bounding box and mean, keys, stable sort, sorted Y and its layered sums,
// node counts per run start, their scan, the nodes
template <int DIMS>
void bh_build(Work &w) {
    Ctx &c = ctx();
    BhTree &t = w.bh;
    const long long n = w.n;
    KernelTimer tm("tsne_bh_tree");
    hipLaunchKernelGGL(bh_bounds_kernel<DIMS>, dim3(t.nslab), dim3(256), 0, c.stream, w.Y.p, n, t.rps, t.part.p);
    hipLaunchKernelGGL(bh_root_kernel<DIMS>, dim3(1), dim3(64), 0, c.stream, t.part.p, t.nslab, n, t.root.p);
    hipLaunchKernelGGL(bh_key_kernel<DIMS>, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, w.Y.p, n, t.root.p, t.key.p);
    launch_check("bh_key_kernel");
    sort_pairs(t.key.p, t.key_s.p, t.iota.p, t.perm.p, static_cast<size_t>(n), 0, t.end_bit, t.sort_tmp, t.sort_tmp.n > 0);
    hipLaunchKernelGGL(bh_gather_kernel<DIMS>, dim3(grid_for(n * DIMS, 256)), dim3(256), 0, c.stream, w.Y.p, t.perm.p, n, t.Ys.p);
    for (int l = 1; l < t.L.nl; ++l)
        hipLaunchKernelGGL(bh_layer_kernel<DIMS>, dim3(grid_for(t.L.len[l], 256)), dim3(256), 0, c.stream, t.L.p[l - 1], t.L.len[l - 1],
                           const_cast<double *>(t.L.p[l]), t.L.len[l]);
    hipLaunchKernelGGL(bh_count_kernel<DIMS>, dim3(grid_for(n + 1, 256)), dim3(256), 0, c.stream, t.key_s.p, n, t.cnt.p);
    launch_check("bh_count_kernel");
    exclusive_scan(t.cnt.p, t.off.p, static_cast<size_t>(n) + 1, t.scan_tmp, t.scan_tmp.n > 0);
    hipLaunchKernelGGL(bh_node_kernel<DIMS>, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, t.key_s.p, t.perm.p, n, t.off.p, t.L, t.meta.p,
                       t.com.p);
    launch_check("bh_node_kernel");
}

template <int DIMS>
void to_f32(Work &w, bool center) {
    if (center) column_stat(w.Y.p, w.n, DIMS, DIMS, nullptr, static_cast<double>(w.n), w.colpart, w.scal.p + 2);
    hipLaunchKernelGGL(center_kernel<DIMS>, dim3(grid_for(w.n * DIMS, 256)), dim3(256), 0, ctx().stream, w.Y.p, w.n, center ? w.scal.p + 2 : nullptr, w.Yf.p);
    launch_check("center_kernel");
}

// attr, rep, zrow and Z (scal[0]) at the current Y / Yf
template <int DIMS>
void gradient_terms(const TsneP &P, Work &w) {
    Ctx &c = ctx();
    {
        KernelTimer t("tsne_attr");
        hipLaunchKernelGGL(attr_kernel<DIMS>, dim3(grid_for(w.n, 256)), dim3(256), 0, c.stream, P.row_ptr.p, P.col.p, P.val.p, w.Y.p, w.n, w.attr.p);
        launch_check("attr_kernel");
    }
    if (w.theta > 0.0) {
        bh_build<DIMS>(w);
        KernelTimer t("tsne_bh_walk");
        hipLaunchKernelGGL(bh_walk_kernel<DIMS>, dim3(grid_for(w.n, 256)), dim3(256), 0, c.stream, w.bh.Ys.p, w.bh.perm.p, w.n, w.bh.meta.p,
                           w.bh.com.p, w.bh.root.p, w.theta, w.rep.p, w.zrow.p);
        launch_check("bh_walk_kernel");
        fixed_reduce(Fold::Sum, w.zrow.p, w.n, w.red.p, w.scal.p);
        return;
    }
    KernelTimer t("tsne_rep");
    for (long long r0 = 0; r0 < w.n; r0 += w.plan.rows) {
        hipLaunchKernelGGL(rep_kernel<DIMS>, dim3(grid_for(w.plan.rows, RT), w.plan.nc), dim3(RT), 0, c.stream, w.Yf.p, w.n, r0, w.plan.rows, w.plan.cj,
                           w.part.p);
        hipLaunchKernelGGL(fold_kernel<DIMS>, dim3(grid_for(w.plan.rows, 256)), dim3(256), 0, c.stream, w.part.p, w.plan.nc, r0, w.plan.rows, w.n,
                           w.rep.p, w.zrow.p);
        launch_check("rep_kernel");
    }
    fixed_reduce(Fold::Sum, w.zrow.p, w.n, w.red.p, w.scal.p);
}

template <int DIMS>
void kl_eval(const TsneP &P, Work &w, double *dst) {
    KernelTimer t("tsne_kl");
    hipLaunchKernelGGL(kl_kernel<DIMS>, dim3(grid_for(w.n, 256)), dim3(256), 0, ctx().stream, P.row_ptr.p, P.col.p, P.val.p, w.Y.p, w.n, w.scal.p, w.kl.p);
    launch_check("kl_kernel");
    fixed_reduce(Fold::Sum, w.kl.p, w.n, w.red.p, dst);
}

struct LoopArgs {
    int max_iter, stop_lying_iter, mom_switch_iter;
    double momentum, final_momentum, eta, exaggeration;
};

template <int DIMS>
void optimise(TsneP &P, Work &w, const LoopArgs &a, std::vector<double> &itercosts, double *costs) {
    Ctx &c = ctx();
    const long long ne = w.n * DIMS;
    const bool lying = a.stop_lying_iter > 0;
    if (lying) hipLaunchKernelGGL(scale_kernel, dim3(grid_for(P.nnz, 256)), dim3(256), 0, c.stream, P.val.p, P.nnz, a.exaggeration, 0);
    SHARP_HIP_CHECK(hipMemsetAsync(w.uY.p, 0, ne * sizeof(double), c.stream));
    std::vector<double> ones(static_cast<size_t>(ne), 1.0);
    w.gains.upload(ones.data(), ones.size());
    to_f32<DIMS>(w, false);
    std::vector<int> record;   // iterations whose KL is recorded
    for (int it = 0; it < a.max_iter; ++it)
        if ((it > 0 && it % 50 == 0) || it == a.max_iter - 1) record.push_back(it);
    DevBuf<double> dcost(std::max<size_t>(1, record.size()));
    size_t next_cost = 0;
    bool pending = false;     // the KL of the previous iteration's positions is due: it is evaluated with this iteration's Z
    double momentum = a.momentum;
    for (int it = 0; it < a.max_iter; ++it) {
        gradient_terms<DIMS>(P, w);
        if (pending) { kl_eval<DIMS>(P, w, dcost.p + next_cost++); pending = false; }
        {
            KernelTimer t("tsne_update");
            hipLaunchKernelGGL(update_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c.stream, w.attr.p, w.rep.p, w.scal.p, ne, momentum, a.eta,
                               w.gains.p, w.uY.p, w.Y.p);
            launch_check("update_kernel");
            to_f32<DIMS>(w, true);
        }
        if (it == a.stop_lying_iter && lying)
            hipLaunchKernelGGL(scale_kernel, dim3(grid_for(P.nnz, 256)), dim3(256), 0, c.stream, P.val.p, P.nnz, a.exaggeration, 1);
        if (it == a.mom_switch_iter) momentum = a.final_momentum;
        if (next_cost < record.size() && record[next_cost] == it) pending = true;
    }
    // the last recorded KL (the last iteration's), or the cost at the start when there are no iterations
    if (pending || costs) {
        gradient_terms<DIMS>(P, w);
        kl_eval<DIMS>(P, w, pending ? dcost.p + next_cost++ : w.scal.p + 1);
    }
    itercosts.assign(record.size(), 0.0);
    if (!record.empty()) dcost.download(itercosts.data(), record.size());
    if (costs) w.kl.download(costs, static_cast<size_t>(w.n));
}

// ---- stage helpers used by the entries -----------------------------------------------------------------------------------
void upload_rows(const double *X, long long n, int d, long long ld, DevBuf<double> &dst) {
    dst.alloc(static_cast<size_t>(n) * d);
    if (ld == d) {
        dst.upload(X, static_cast<size_t>(n) * d);
    } else {
        SHARP_HIP_CHECK(hipMemcpy2DAsync(dst.p, d * sizeof(double), X, ld * sizeof(double), d * sizeof(double), n, hipMemcpyHostToDevice, ctx().stream));
    }
}

int perplexity_K(double perplexity) {
    SHARP_REQUIRE(std::isfinite(perplexity) && perplexity > 0, "Rtsne: perplexity must be positive");
    SHARP_REQUIRE(perplexity <= 85.0, "Rtsne: perplexity above 85 is not supported (at most 255 neighbours per row)");
    return static_cast<int>(std::floor(3.0 * perplexity));
}

}  // namespace

void symmetric_eigen(int d, std::vector<double> &V, std::vector<double> &w) {
    std::vector<double> e(d);
    w.assign(d, 0.0);
    tred2(d, V, w, e);
    tql2(d, V, w, e);
}

// ---------------------------------------------------------------------------------------------------------------------------
void tsne_prepare(const double *X, long long n, int d, long long ld, bool pca, int initial_dims, bool pca_center, bool pca_scale, bool normalize,
                  DevBuf<double> &out, int *d_out) {
    Ctx &c = ctx();
    DevBuf<double> raw, part, stat(static_cast<size_t>(2) * d + 2);
    upload_rows(X, n, d, ld, raw);
    int dd = d;
    if (pca) {
        KernelTimer t("tsne_pca");
        const int k = std::min(initial_dims, d);
        SHARP_REQUIRE(k >= 1, "Rtsne: initial_dims must be >= 1");
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
                SHARP_REQUIRE(v[j] > 0 && std::isfinite(v[j]), "Rtsne: cannot rescale a constant/zero column to unit variance (column " + std::to_string(j + 1) + ")");
                v[j] = std::sqrt(v[j]);
            }
            SHARP_HIP_CHECK(hipMemcpyAsync(stat.p + d, v.data(), d * sizeof(double), hipMemcpyHostToDevice, c.stream));
            stream_sync();
            sd = stat.p + d;
        }
        DevBuf<double> xc(static_cast<size_t>(n) * d);
        hipLaunchKernelGGL(affine_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, c.stream, raw.p, n, d, static_cast<long long>(d), mu, sd, 1.0, xc.p);
        launch_check("affine_kernel");
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
            leading_eigenvectors(std::move(G), d, k, Vk);
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
        hipLaunchKernelGGL(affine_kernel, dim3(grid_for(n * dd, 256)), dim3(256), 0, c.stream, out.p, n, dd, static_cast<long long>(dd), stat.p,
                           nullptr, 1.0, out.p);
        const unsigned nb = fixed_reduce_blocks(n * dd);
        DevBuf<double> mx(nb);
        fixed_reduce_parts(Fold::AbsMax, out.p, n * dd, mx.p);
        std::vector<double> hm(nb);
        mx.download(hm.data(), nb);
        double m = 0.0;
        for (double v : hm) m = std::max(m, v);
        SHARP_REQUIRE(m > 0 && std::isfinite(m), "Rtsne: the normalised input is all zero or not finite");
        hipLaunchKernelGGL(affine_kernel, dim3(grid_for(n * dd, 256)), dim3(256), 0, c.stream, out.p, n, dd, static_cast<long long>(dd), nullptr,
                           nullptr, m, out.p);
        launch_check("affine_kernel");
    }
    *d_out = dd;
}

void tsne_knn(const double *dX, long long n, int d, int K, DevBuf<int> &idx, DevBuf<double> &dist) {
    Ctx &c = ctx();
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, "tsne_knn: need 1 <= K <= 255 and K < n");
    KernelTimer t("tsne_knn");
    // The candidates are selected on w = x - column mean (fp64): distances do not change under a translation, but the error of
    // ||x_i||^2 + ||x_j||^2 - 2 x_i.x_j scales with ||x||^2, and input far from the origin (Rtsne(pca = FALSE, normalize = FALSE),
    // sharp_tsne_knn) would otherwise lose true neighbours to it.  The merge re-ranks the chosen K on the caller's values.
    DevBuf<double> Xc(static_cast<size_t>(n) * d), mu(d), mupart;
    column_stat(dX, n, d, d, nullptr, static_cast<double>(n), mupart, mu.p);
    hipLaunchKernelGGL(affine_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, c.stream, dX, n, d, static_cast<long long>(d), mu.p, nullptr, 1.0,
                       Xc.p);
    launch_check("affine_kernel");
    DevBuf<double> nrm(n);
    DevBuf<int> bad(1);
    bad.zero();
    hipLaunchKernelGGL(rownorm_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, Xc.p, n, d, nrm.p);
    hipLaunchKernelGGL(norm_check_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, nrm.p, n, bad.p);
    launch_check("norm_check_kernel");
    int hb = 0;
    bad.download(&hb, 1);
    SHARP_REQUIRE(hb == 0, "Rtsne: the (prepared) input holds NA / NaN / Inf, or values so large that squared distances overflow");
    idx.alloc(static_cast<size_t>(n) * K);
    dist.alloc(static_cast<size_t>(n) * K);
    // Launches of about 8e9 candidate pairs at d = 50 (measured 1e11 pairs / s at d = 50: under 0.1 s each at any n): rows per launch
    // from that budget, and the candidate columns cut into chunks so that a launch has >= ~1024 workgroups however few its rows are.
    const double budget = 8e9 / (std::max(d, 4) / 50.0 + 0.25);
    const long long rows = std::min((n + KQ - 1) / KQ * KQ, std::max<long long>(KQ, static_cast<long long>(budget / static_cast<double>(n)) / KQ * KQ));
    const long long rb = (rows + KQ - 1) / KQ;
    const long long nc0 = std::max<long long>(1, std::min<long long>((n + KCT - 1) / KCT, (1024 + rb - 1) / rb));
    const long long cj = ((n + nc0 - 1) / nc0 + KCT - 1) / KCT * KCT;
    const int nc = static_cast<int>((n + cj - 1) / cj);
    DevBuf<int> pidx(static_cast<size_t>(nc) * rows * K);
    DevBuf<double> pdist(static_cast<size_t>(nc) * rows * K);
    const size_t lds = sizeof(double) * KQ * KDT + (sizeof(double) + sizeof(int)) * KQ * K;
    const size_t lds_merge = (sizeof(double) + sizeof(int)) * 4 * K;
    for (long long r0 = 0; r0 < n; r0 += rows) {
        const long long r1 = std::min(n, r0 + rows);
        hipLaunchKernelGGL(knn_kernel, dim3(grid_for(r1 - r0, KQ), nc), dim3(256), lds, c.stream, Xc.p, nrm.p, n, d, K, r0, r1, cj, pidx.p, pdist.p);
        launch_check("knn_kernel");
        hipLaunchKernelGGL(knn_merge_kernel, dim3(grid_for(r1 - r0, 4)), dim3(256), lds_merge, c.stream, dX, n, d, K, r0, r1 - r0, nc, pidx.p,
                           pdist.p, idx.p, dist.p, bad.p);
        launch_check("knn_merge_kernel");
    }
    bad.download(&hb, 1);
    SHARP_REQUIRE(hb == 0, "Rtsne: fewer than K rows at a finite distance from some row (non-finite input?)");
}

void tsne_affinities(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, double perplexity, TsneP &P) {
    Ctx &c = ctx();
    DevBuf<double> Pc(static_cast<size_t>(n) * K);
    {
        KernelTimer t("tsne_calib");
        hipLaunchKernelGGL(calib_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, dist.p, n, K, std::log(perplexity), Pc.p);
        launch_check("calib_kernel");
    }
    KernelTimer t("tsne_sym");
    const size_t ne = static_cast<size_t>(n) * K * 2;
    DevBuf<unsigned long long> keys(ne), keys2(ne);
    DevBuf<double> vals(ne), vals2(ne);
    hipLaunchKernelGGL(coo_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, c.stream, idx.p, Pc.p, n, K, keys.p, vals.p);
    launch_check("coo_kernel");
    Pc.release();
    // merge the (at most two) entries of a key: p_ij + p_ji
    const u64 un = static_cast<u64>(n);
    MergeScratch tmp;
    const size_t nnz = merge_by_key<double, Plus>(keys.p, vals.p, ne, un * un, keys2.p, vals2.p, keys.p, vals.p, tmp);
    DevBuf<double> red(kRedBlocks), total(1);
    fixed_reduce(Fold::Sum, vals.p, static_cast<long long>(nnz), red.p, total.p);
    P.n = n;
    P.nnz = static_cast<long long>(nnz);
    P.row_ptr.alloc(n + 1);
    P.col.alloc(nnz);
    P.val.alloc(nnz);
    merged_to_csr<double>(keys.p, P.nnz, n, false, P.row_ptr.p, P.col.p, nullptr, vals.p, total.p, P.val.p);   // (no row is empty: K entries each)
    stream_sync();
}

void tsne_knn_dist(const double *d, int n, int K, DevBuf<int> &idx, DevBuf<double> &dist2) {
    Ctx &c = ctx();
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, "tsne_knn_dist: need 1 <= K <= 255 and K < n");
    const size_t len = static_cast<size_t>(n) * (n - 1) / 2;
    const int nld = dist_nld(n);
    DevBuf<double> D(static_cast<size_t>(nld) * nld);
    {
        DevBuf<double> cond(len);
        {
            KernelTimer t("tsne_dist_upload");
            cond.upload(d, len);
        }
        dist_expand(cond.p, n, D.p);
        stream_sync();   // (the vector goes out of scope)
    }
    idx.alloc(static_cast<size_t>(n) * K);
    dist2.alloc(static_cast<size_t>(n) * K);
    DevBuf<int> bad(1);
    bad.zero();
    {
        KernelTimer t("tsne_knn_dist");
        hipLaunchKernelGGL(knn_rows_kernel, dim3(grid_for(n, 4)), dim3(256), (sizeof(double) + sizeof(int)) * 4 * K, c.stream, D.p, n, nld, K, idx.p,
                           dist2.p, bad.p);
        launch_check("knn_rows_kernel");
    }
    int hb = 0;
    bad.download(&hb, 1);
    SHARP_REQUIRE(hb == 0, "Rtsne: the distances are so large that their squares overflow");
}

void tsne_upload_neighbours(const int *index, const double *distance, long long n, int K, bool squared, DevBuf<int> &idx,
                            DevBuf<double> &dist2) {
    Ctx &c = ctx();
    const size_t ne = static_cast<size_t>(n) * K;
    idx.alloc(ne);
    dist2.alloc(ne);
    idx.upload(index, ne);
    dist2.upload(distance, ne);
    DevBuf<unsigned long long> word(1);
    SHARP_HIP_CHECK(hipMemsetAsync(word.p, 0xFF, sizeof(unsigned long long), c.stream));
    {
        KernelTimer t("tsne_nn_check");
        hipLaunchKernelGGL(nn_check_kernel, dim3(grid_for(n, 4)), dim3(256), sizeof(int) * 4 * K, c.stream, idx.p, dist2.p, n, K, word.p);
        launch_check("nn_check_kernel");
    }
    unsigned long long w = NN_OK;
    word.download(&w, 1);
    if (w != NN_OK) {
        const std::string row = " (row " + std::to_string(w >> 3) + ", counted from 0)";
        switch (static_cast<int>(w & 7)) {
            case NN_RANGE: throw Error(SHARP_ERR_ARG, "Rtsne_neighbors: a neighbour index outside [0, n)" + row);
            case NN_SELF: throw Error(SHARP_ERR_ARG, "Rtsne_neighbors: a row names itself as a neighbour" + row);
            case NN_TWICE: throw Error(SHARP_ERR_ARG, "Rtsne_neighbors: the same neighbour index twice in a row" + row);
            default: throw Error(SHARP_ERR_ARG, "Rtsne_neighbors: a distance that is NA / NaN / Inf or negative" + row);
        }
    }
    if (!squared) {
        DevBuf<int> bad(1);
        bad.zero();
        hipLaunchKernelGGL(square_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, c.stream, dist2.p, n * K, bad.p);
        launch_check("square_kernel");
        int hb = 0;
        bad.download(&hb, 1);
        SHARP_REQUIRE(hb == 0, "Rtsne_neighbors: the distances are so large that their squares overflow");
    }
}

void tsne_gradient(const TsneP &P, const double *dY_in, int dims, double *dGrad, double theta, double *Z) {
    Work w;
    w.init(P.n, dims, theta);
    SHARP_HIP_CHECK(hipMemcpyAsync(w.Y.p, dY_in, static_cast<size_t>(P.n) * dims * sizeof(double), hipMemcpyDeviceToDevice, ctx().stream));
    const long long ne = P.n * dims;
    auto run = [&](auto tag) {
        constexpr int D = decltype(tag)::value;
        to_f32<D>(w, false);
        gradient_terms<D>(P, w);
        hipLaunchKernelGGL(grad_kernel<D>, dim3(grid_for(ne, 256)), dim3(256), 0, ctx().stream, w.attr.p, w.rep.p, w.scal.p, ne, dGrad);
        launch_check("grad_kernel");
    };
    if (dims == 1) run(std::integral_constant<int, 1>());
    else if (dims == 2) run(std::integral_constant<int, 2>());
    else run(std::integral_constant<int, 3>());
    if (Z) SHARP_HIP_CHECK(hipMemcpyAsync(Z, w.scal.p, sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    stream_sync();
}

}  // namespace sharp

using namespace sharp;

namespace {
void check_dims(int dims) { SHARP_REQUIRE(dims >= 1 && dims <= 3, "Rtsne: dims must be 1, 2 or 3"); }
void check_X(const double *X, long long n, int d, long long ld) {
    SHARP_REQUIRE(X && n >= 2 && d >= 1 && ld >= d, "Rtsne: bad input matrix (need n >= 2 rows of d >= 1 values, ld >= d)");
    SHARP_REQUIRE(n < INT_MAX, "Rtsne: at most 2^31 - 1 rows");
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < d; ++c)
            if (!std::isfinite(X[i * ld + c]))
                throw sharp::Error(SHARP_ERR_ARG, "Rtsne: the input holds NA / NaN / Inf (row " + std::to_string(i + 1) + ", column " +
                                                      std::to_string(c + 1) + ")");
}

void check_loop_args(int dims, int max_iter, double momentum, double final_momentum, double eta, double exaggeration, const double *Y) {
    check_dims(dims);
    SHARP_REQUIRE(Y, "sharp_tsne: null Y");
    SHARP_REQUIRE(max_iter >= 0 && std::isfinite(eta) && std::isfinite(momentum) && std::isfinite(final_momentum), "Rtsne: bad optimiser arguments");
    SHARP_REQUIRE(std::isfinite(exaggeration) && exaggeration > 0, "Rtsne: exaggeration_factor must be positive");
}

// Everything behind the k-NN: P from the lists (idx, dist2: device, n x K, squared distances; released once P exists), the start, the
// optimiser loop.  bh_theta > 0 takes the Barnes-Hut repulsion with that theta, 0 the exact one.
void run_from_neighbours(DevBuf<int> &idx, DevBuf<double> &dist, long long n, int K, int dims, double perplexity, double bh_theta,
                         const LoopArgs &la, const double *Y_init, double seed, double *Y, double *itercosts, double *costs) {
    TsneP P;
    tsne_affinities(idx, dist, n, K, perplexity, P);
    idx.release();
    dist.release();
    Work w;
    w.init(n, dims, bh_theta);
    const size_t ne = static_cast<size_t>(n) * dims;
    std::vector<double> y0(ne);
    if (Y_init) {
        for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(std::isfinite(Y_init[e]), "Rtsne: Y_init holds NA / NaN / Inf");
        std::copy(Y_init, Y_init + ne, y0.begin());
    } else {
        // Y = 1e-4 N(0, 1): R's set.seed(seed) stream, one normal per pair of unif_rand() (polar method, the second draw discarded)
        RRng rng(static_cast<uint32_t>(static_cast<int>(seed)));
        for (size_t e = 0; e < ne; ++e) {
            double x, y, rad;
            do {
                x = 2.0 * rng.unif() - 1.0;
                y = 2.0 * rng.unif() - 1.0;
                rad = x * x + y * y;
            } while (rad >= 1.0 || rad == 0.0);
            y0[e] = x * std::sqrt(-2.0 * std::log(rad) / rad) * 1e-4;
        }
    }
    w.Y.upload(y0.data(), ne);
    std::vector<double> ic;
    if (dims == 1) optimise<1>(P, w, la, ic, costs);
    else if (dims == 2) optimise<2>(P, w, la, ic, costs);
    else optimise<3>(P, w, la, ic, costs);
    w.Y.download(Y, ne);
    if (itercosts) std::copy(ic.begin(), ic.end(), itercosts);
}

// Rtsne's body: prepare, exact k-NN, the duplicate check, then run_from_neighbours
void run_tsne(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale,
              int normalize, int check_duplicates, double perplexity, double bh_theta, int max_iter, int stop_lying_iter, int mom_switch_iter,
              double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y,
              double *itercosts, double *costs) {
    check_X(X, n, d, ld);
    check_loop_args(dims, max_iter, momentum, final_momentum, eta, exaggeration, Y);
    const int K = perplexity_K(perplexity);
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
    DevBuf<double> Xp;
    int dp = 0;
    tsne_prepare(X, n, d, ld, pca != 0, initial_dims, pca_center != 0, pca_scale != 0, normalize != 0, Xp, &dp);
    DevBuf<int> idx;
    DevBuf<double> dist;
    tsne_knn(Xp.p, n, dp, K, idx, dist);
    if (check_duplicates) {
        DevBuf<int> flag(1);
        flag.zero();
        hipLaunchKernelGGL(dup_flag_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, dist.p, n, K, flag.p);
        int f = 0;
        flag.download(&f, 1);
        SHARP_REQUIRE(f == 0, "Remove duplicates before running TSNE.");
    }
    Xp.release();
    run_from_neighbours(idx, dist, n, K, dims, perplexity, bh_theta,
                        LoopArgs{max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration}, Y_init, seed, Y,
                        itercosts, costs);
}

// Rtsne's own check on theta, as far as it is known here
void check_bh_theta(double theta) { SHARP_REQUIRE(std::isfinite(theta) && theta >= 0.0 && theta <= 1.0, "Incorrect theta."); }
}  // namespace

extern "C" {

// R/visualization_SHARP.R:94: Rtsne(x1, check_duplicates = FALSE, pca = flag, ...), with an exact repulsion (theta accepted, unused)
int sharp_tsne(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale, int normalize,
               int check_duplicates, double perplexity, double theta, int max_iter, int stop_lying_iter, int mom_switch_iter, double momentum,
               double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y, double *itercosts,
               double *costs) {
    SHARP_API_BEGIN
    (void)theta;
    ctx();
    run_tsne(X, n, d, ld, dims, initial_dims, pca, pca_center, pca_scale, normalize, check_duplicates, perplexity, 0.0, max_iter, stop_lying_iter,
             mom_switch_iter, momentum, final_momentum, eta, exaggeration, Y_init, seed, Y, itercosts, costs);
    SHARP_API_END
}

// the same with bhtsne's Barnes-Hut repulsion at theta (0 <= theta <= 1; theta == 0: the exact path above, bit for bit)
int sharp_tsne_bh(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale,
                  int normalize, int check_duplicates, double perplexity, double theta, int max_iter, int stop_lying_iter, int mom_switch_iter,
                  double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y,
                  double *itercosts, double *costs) {
    SHARP_API_BEGIN
    ctx();
    check_bh_theta(theta);
    run_tsne(X, n, d, ld, dims, initial_dims, pca, pca_center, pca_scale, normalize, check_duplicates, perplexity, theta, max_iter, stop_lying_iter,
             mom_switch_iter, momentum, final_momentum, eta, exaggeration, Y_init, seed, Y, itercosts, costs);
    SHARP_API_END
}

int sharp_tsne_prepare(const double *X, long long n, int d, long long ld, int pca, int initial_dims, int pca_center, int pca_scale, int normalize,
                       double *out, int *d_out) {
    SHARP_API_BEGIN
    ctx();
    check_X(X, n, d, ld);
    SHARP_REQUIRE(out && d_out, "sharp_tsne_prepare: null output");
    DevBuf<double> Xp;
    tsne_prepare(X, n, d, ld, pca != 0, initial_dims, pca_center != 0, pca_scale != 0, normalize != 0, Xp, d_out);
    Xp.download(out, static_cast<size_t>(n) * *d_out);
    SHARP_API_END
}

int sharp_tsne_knn(const double *X, long long n, int d, long long ld, int K, int *idx, double *dist) {
    SHARP_API_BEGIN
    ctx();
    check_X(X, n, d, ld);
    SHARP_REQUIRE(idx && dist, "sharp_tsne_knn: null output");
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_knn(dX.p, n, d, K, di, dd);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist, static_cast<size_t>(n) * K);
    SHARP_API_END
}

int sharp_tsne_affinities(const double *X, long long n, int d, long long ld, double perplexity, long long cap, long long *row_ptr, int *col,
                          double *val, long long *nnz) {
    SHARP_API_BEGIN
    ctx();
    check_X(X, n, d, ld);
    SHARP_REQUIRE(row_ptr && col && val && nnz, "sharp_tsne_affinities: null output");
    const int K = perplexity_K(perplexity);
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_knn(dX.p, n, d, K, di, dd);
    TsneP P;
    tsne_affinities(di, dd, n, K, perplexity, P);
    *nnz = P.nnz;
    SHARP_REQUIRE(cap >= P.nnz, "sharp_tsne_affinities: col / val hold fewer than nnz entries (2 n floor(3 perplexity) always suffice)");
    P.row_ptr.download(row_ptr, static_cast<size_t>(n) + 1);
    P.col.download(col, static_cast<size_t>(P.nnz));
    P.val.download(val, static_cast<size_t>(P.nnz));
    SHARP_API_END
}

}  // extern "C"

namespace {
// the arguments every entry on given neighbours checks before it touches the lists
void check_neighbour_args(const int *index, const double *distance, long long n, int K, double perplexity, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(index && distance, w + ": null index / distance");
    SHARP_REQUIRE(n >= 2 && n < INT_MAX, w + ": need 2 <= n < 2^31 rows");
    SHARP_REQUIRE(K >= 1, w + ": need at least one neighbour per row (K >= 1)");
    SHARP_REQUIRE(K <= 255, w + ": at most 255 neighbours per row");
    SHARP_REQUIRE(K <= n - 1, w + ": K neighbours per row need K <= n - 1");
    SHARP_REQUIRE(std::isfinite(perplexity) && perplexity > 0, "Rtsne: perplexity must be positive");
    SHARP_REQUIRE(perplexity <= static_cast<double>(K), w + ": perplexity above K, the entropy of K neighbours cannot reach it");
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
}

// d: R's dist vector, every entry finite and >= 0, checked on the host before the upload
void check_dist_vector(const double *d, int n, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(n <= SHARP_DIST_MAX_N, w + ": more than 46340 objects (the dist vector would pass 2^30 entries) is not supported");
    SHARP_REQUIRE(n >= 2, w + ": need n >= 2 objects");
    SHARP_REQUIRE(d, w + ": null d");
    const size_t len = static_cast<size_t>(n) * (n - 1) / 2;
    for (size_t e = 0; e < len; ++e)
        SHARP_REQUIRE(d[e] >= 0.0 && d[e] <= DBL_MAX, w + ": d holds NA / NaN / Inf or a negative distance");   // (false for NaN too)
}
}  // namespace

extern "C" {

int sharp_tsne_neighbors(const int *index, const double *distance, long long n, int K, int squared, int repulsion, int dims, double perplexity,
                         double theta, int max_iter, int stop_lying_iter, int mom_switch_iter, double momentum, double final_momentum, double eta,
                         double exaggeration, const double *Y_init, double seed, double *Y, double *itercosts, double *costs) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(repulsion == 0 || repulsion == 1, "sharp_tsne_neighbors: repulsion must be 0 (exact) or 1 (Barnes-Hut)");
    if (repulsion) check_bh_theta(theta);
    check_neighbour_args(index, distance, n, K, perplexity, "sharp_tsne_neighbors");
    check_loop_args(dims, max_iter, momentum, final_momentum, eta, exaggeration, Y);
    DevBuf<int> idx;
    DevBuf<double> dist;
    tsne_upload_neighbours(index, distance, n, K, squared != 0, idx, dist);
    run_from_neighbours(idx, dist, n, K, dims, perplexity, repulsion ? theta : 0.0,
                        LoopArgs{max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration}, Y_init, seed, Y,
                        itercosts, costs);
    SHARP_API_END
}

int sharp_tsne_dist(const double *d, int n, int repulsion, int dims, double perplexity, double theta, int max_iter, int stop_lying_iter,
                    int mom_switch_iter, double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init,
                    double seed, double *Y, double *itercosts, double *costs) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(n <= SHARP_DIST_MAX_N, "sharp_tsne_dist: more than 46340 objects (the dist vector would pass 2^30 entries) is not supported");
    SHARP_REQUIRE(repulsion == 0 || repulsion == 1, "sharp_tsne_dist: repulsion must be 0 (exact) or 1 (Barnes-Hut)");
    if (repulsion) check_bh_theta(theta);
    check_loop_args(dims, max_iter, momentum, final_momentum, eta, exaggeration, Y);
    const int K = perplexity_K(perplexity);
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
    check_dist_vector(d, n, "sharp_tsne_dist");
    DevBuf<int> idx;
    DevBuf<double> dist;
    tsne_knn_dist(d, n, K, idx, dist);
    run_from_neighbours(idx, dist, n, K, dims, perplexity, repulsion ? theta : 0.0,
                        LoopArgs{max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration}, Y_init, seed, Y,
                        itercosts, costs);
    SHARP_API_END
}

int sharp_tsne_knn_dist(const double *d, int n, int K, int *idx, double *dist2) {
    SHARP_API_BEGIN
    ctx();
    check_dist_vector(d, n, "sharp_tsne_knn_dist");
    SHARP_REQUIRE(idx && dist2, "sharp_tsne_knn_dist: null output");
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_knn_dist(d, n, K, di, dd);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist2, static_cast<size_t>(n) * K);
    SHARP_API_END
}

int sharp_tsne_affinities_nn(const int *index, const double *distance, long long n, int K, int squared, double perplexity, long long cap,
                             long long *row_ptr, int *col, double *val, long long *nnz) {
    SHARP_API_BEGIN
    ctx();
    check_neighbour_args(index, distance, n, K, perplexity, "sharp_tsne_affinities_nn");
    SHARP_REQUIRE(row_ptr && col && val && nnz, "sharp_tsne_affinities_nn: null output");
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_upload_neighbours(index, distance, n, K, squared != 0, di, dd);
    TsneP P;
    tsne_affinities(di, dd, n, K, perplexity, P);
    *nnz = P.nnz;
    SHARP_REQUIRE(cap >= P.nnz, "sharp_tsne_affinities_nn: col / val hold fewer than nnz entries (2 n K always suffice)");
    P.row_ptr.download(row_ptr, static_cast<size_t>(n) + 1);
    P.col.download(col, static_cast<size_t>(P.nnz));
    P.val.download(val, static_cast<size_t>(P.nnz));
    SHARP_API_END
}

}  // extern "C"

namespace {
void gradient_entry(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double theta, double *dY,
                    double *Z) {
    check_dims(dims);
    SHARP_REQUIRE(row_ptr && col && val && Y && dY && n >= 2, "sharp_tsne_gradient: null argument");
    TsneP P;
    P.n = n;
    SHARP_REQUIRE(row_ptr[0] == 0 && row_ptr[n] >= 0, "sharp_tsne_gradient: row_ptr must run from 0 to nnz");
    P.nnz = row_ptr[n];
    P.row_ptr.alloc(n + 1);
    P.row_ptr.upload(row_ptr, n + 1);
    P.col.alloc(std::max<long long>(P.nnz, 1));
    P.val.alloc(std::max<long long>(P.nnz, 1));
    if (P.nnz) { P.col.upload(col, P.nnz); P.val.upload(val, P.nnz); }
    const size_t ne = static_cast<size_t>(n) * dims;
    for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(std::isfinite(Y[e]), "sharp_tsne_gradient: Y holds NA / NaN / Inf");
    for (long long i = 0; i < n; ++i) SHARP_REQUIRE(row_ptr[i] <= row_ptr[i + 1], "sharp_tsne_gradient: row_ptr is not monotone");
    for (long long e = 0; e < P.nnz; ++e) SHARP_REQUIRE(col[e] >= 0 && col[e] < n, "sharp_tsne_gradient: a column index out of range");
    DevBuf<double> dYin(ne), dG(ne);
    dYin.upload(Y, ne);
    tsne_gradient(P, dYin.p, dims, dG.p, theta, Z);
    dG.download(dY, ne);
}
}  // namespace

extern "C" {

int sharp_tsne_gradient(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double *dY) {
    SHARP_API_BEGIN
    ctx();
    gradient_entry(row_ptr, col, val, n, dims, Y, 0.0, dY, nullptr);
    SHARP_API_END
}

int sharp_tsne_gradient_bh(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double theta,
                           double *dY, double *Z) {
    SHARP_API_BEGIN
    ctx();
    check_bh_theta(theta);
    gradient_entry(row_ptr, col, val, n, dims, Y, theta, dY, Z);
    SHARP_API_END
}

}  // extern "C"
