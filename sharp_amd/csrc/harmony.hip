// harmony.hip -- a Harmony-style batch integration of PCA scores (the specification is the project's own, modelled on
// Korsunsky et al. 2019 for one categorical covariate: no parity with the Harmony packages is claimed).
//   order      block(i) = h(0, i) mod n_blocks; the working order is the cells sorted by (block, batch, i) with one stable sort_pairs, so
//              every (block, batch) segment is contiguous.  A segment is cut into slabs of kHarmonySlab cells.
//   assign     the hot pass: per cell the K dots against Y (Y in LDS, tiled over clusters beyond kHarmonyLdsTile doubles), the minimum,
//              the exponentials, the factor of the cell's batch, the normalisation over K and R's row; in argmax mode a_i instead
//   sums       cells-major TN products C[K x d] = sum over a slab's cells of R[cell, :]^T X[cell, :] through gemm_tn_f64_batched, one task
//              per slab; one thread per entry and batch folds a segment's slabs in slab order and the batch's segments in block order,
//              then one thread per entry the batches in batch order.  The column sums O^j (K x 1 per slab) have a kernel of their own, and the table kernel folds the other
//              blocks' tables in block order into O, E and P = ((E + 1) / (O + 1))^theta
//   objective  the assign pass's dots again, R read: a wave carries four cells, a butterfly over K per cell; the cells' terms go through
//              fixed_reduce
//   correct    the K B d numbers W on the host from the downloaded sums (the ridge system is an arrowhead matrix: a closed form), then one
//              wave per cell, lanes over the d columns
// No floating-point atomic: every sum's order is fixed by the input's shape, so two calls give the same bits.
#include "harmony.hpp"
#include "graph_prim.hpp"
#include "linalg.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace sharp {
namespace {

constexpr double kInf = __builtin_huge_val();

// keys[i] = block(i) * B + batch[i]; src[i] = i
__global__ __launch_bounds__(256) void harmony_keys_kernel(const int *__restrict__ batch, long long n, int B, int n_blocks, u64 seed,
                                                           u64 *__restrict__ keys, int *__restrict__ src) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 blk = harmony_hash(seed, 0, static_cast<u64>(i)) % static_cast<u64>(n_blocks);
    keys[i] = blk * static_cast<u64>(B) + static_cast<u64>(batch[i]);
    src[i] = static_cast<int>(i);
}

// dst[r, :] = src[idx[r], :] (rows x d); bdst[r] = bsrc[idx[r]] when wanted
__global__ __launch_bounds__(256) void harmony_gather_kernel(const double *__restrict__ src, const int *__restrict__ idx, long long rows, int d,
                                                             double *__restrict__ dst, const int *__restrict__ bsrc, int *__restrict__ bdst) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= rows * d) return;
    const long long r = e / d;
    const int c = static_cast<int>(e - r * d);
    const long long s = idx[r];
    dst[e] = src[s * d + c];
    if (bdst && c == 0) bdst[r] = bsrc[s];
}

// One wave per row: dst[r, :] = src[s, :] / its 2-norm, s = idx[r] (or r).  A zero row: dst[r, :] stays as it is when keep, else it is zero.
__global__ __launch_bounds__(256) void harmony_normalize_kernel(const double *__restrict__ src, const int *__restrict__ idx, long long rows, int d,
                                                                int keep, double *__restrict__ dst) {
    const long long r = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const long long s = idx ? idx[r] : r;
    const double v0 = lane < d ? src[s * d + lane] : 0.0;
    const double v1 = lane + 64 < d ? src[s * d + lane + 64] : 0.0;
    const double nrm = sqrt(wave_sum(v0 * v0 + v1 * v1));
    if (!(nrm > 0.0) && keep) return;
    const double f = nrm > 0.0 ? nrm : 1.0;
    if (lane < d) dst[r * d + lane] = v0 / f;
    if (lane + 64 < d) dst[r * d + lane + 64] = v1 / f;
}

// The hot pass over the cells [c0, c1) of the order the arrays are stored in.  A workgroup of four waves takes groups of 16 cells in a
// grid-stride loop, a wave kHarmonyWaveCells of them; lane l owns the clusters l, l + 64, .. (NU of them).  Y is staged in LDS with an odd
// row stride dp (no bank conflict between the lanes' rows), KT clusters at a time: once per workgroup when it fits, else once per group
// and tile.  Per cell: dot_k = sum over c of Y[k, c] Zh[cell, c] (fma, c ascending), D_k = 2 (1 - dot_k);
//   argmax = 0: R[cell, k] = exp(-(D_k - min D) / sigma) * P[batch[cell], k] (P null: 1), divided by the sum over k (per lane over its
//               clusters ascending, then the butterfly)
//   argmax = 1: a[cell] = the k of the largest dot, ties to the lower k
//   mode 2 (harmony_objective_kernel): obj[cell] = sum over k of R (D + sigma log R + sigma theta L[batch[cell], k]), the middle term 0
//               where R = 0, with R read and L in P's place: per lane over its clusters ascending, then the butterfly
template <int NU>
__device__ __forceinline__ void harmony_cells(const double *__restrict__ Zh, const double *__restrict__ Y, const int *__restrict__ batch,
                                              const double *__restrict__ P, long long c0, long long c1, int d, int K, int dp, int KT, double sigma,
                                              double theta, int mode, double *__restrict__ R, int *__restrict__ a, double *__restrict__ obj) {
    __shared__ double Ys[kHarmonyLdsTile];
    const int argmax = mode == 1;
    constexpr int C = kHarmonyWaveCells;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long groups = (c1 - c0 + 4 * C - 1) / (4 * C);
    const bool tiled = K > KT;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long base = c0 + g * (4 * C) + static_cast<long long>(wave) * C;
        const bool live = base < c1;
        const double *z[C];
#pragma unroll
        for (int q = 0; q < C; ++q) z[q] = Zh + (base + q < c1 ? base + q : c1 - 1) * d;      // (a cell beyond the range reads the last one's row)
        double dot[NU][C];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int q = 0; q < C; ++q) dot[u][q] = 0.0;
        for (int t0 = 0; t0 < K; t0 += KT) {
            const int t1 = t0 + KT < K ? t0 + KT : K;
            if (tiled || g == static_cast<long long>(blockIdx.x)) {
                __syncthreads();
                for (int e = tid; e < (t1 - t0) * d; e += 256) {
                    const int k = e / d, c = e - k * d;
                    Ys[k * dp + c] = Y[static_cast<long long>(t0 + k) * d + c];
                }
                __syncthreads();
            }
            if (!live) continue;
            bool act[NU];
            const double *row[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int k = lane + 64 * u;
                act[u] = k >= t0 && k < t1;
                row[u] = Ys + (act[u] ? k - t0 : 0) * dp;
            }
#pragma unroll 4
            for (int c = 0; c < d; ++c) {
                double zc[C];
#pragma unroll
                for (int q = 0; q < C; ++q) zc[q] = z[q][c];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const double y = act[u] ? row[u][c] : 0.0;
#pragma unroll
                    for (int q = 0; q < C; ++q) dot[u][q] = fma(y, zc[q], dot[u][q]);
                }
            }
        }
        if (!live) continue;
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const long long cell = base + q;
            if (cell >= c1) break;
            if (argmax) {
                double bv = -kInf;
                int bk = 0x7fffffff;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int k = lane + 64 * u;
                    if (k < K && dot[u][q] > bv) { bv = dot[u][q]; bk = k; }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double ov = __shfl_xor(bv, off);
                    const int ok = __shfl_xor(bk, off);
                    if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
                }
                if (lane == 0) a[cell] = bk;
                continue;
            }
            double D[NU], mn = kInf;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                D[u] = 2.0 * (1.0 - dot[u][q]);
                if (lane + 64 * u < K) mn = fmin(mn, D[u]);
            }
            if (mode == 2) {
                const double *Lb = P + static_cast<long long>(batch[cell]) * K;
                double acc = 0.0;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int k = lane + 64 * u;
                    if (k < K) {
                        const double r = R[cell * K + k];
                        const double mid = r > 0.0 ? sigma * log(r) : 0.0;
                        acc += r * (D[u] + mid + sigma * theta * Lb[k]);
                    }
                }
                acc = wave_sum(acc);
                if (lane == 0) obj[cell] = acc;
                continue;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mn = fmin(mn, __shfl_xor(mn, off));
            const double *Pb = P ? P + static_cast<long long>(batch[cell]) * K : nullptr;
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int k = lane + 64 * u;
                double e = 0.0;
                if (k < K) {
                    e = exp(-(D[u] - mn) / sigma);
                    if (Pb) e *= Pb[k];
                }
                D[u] = e;
                s += e;
            }
            s = wave_sum(s);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int k = lane + 64 * u;
                if (k < K) R[cell * K + k] = D[u] / s;
            }
        }
    }
}

template <int NU>
__global__ __launch_bounds__(256) void harmony_assign_kernel(const double *__restrict__ Zh, const double *__restrict__ Y, const int *__restrict__ batch,
                                                             const double *__restrict__ P, long long c0, long long c1, int d, int K, int dp, int KT,
                                                             double sigma, int argmax, double *__restrict__ R, int *__restrict__ a) {
    harmony_cells<NU>(Zh, Y, batch, P, c0, c1, d, K, dp, KT, sigma, 0.0, argmax ? 1 : 0, R, a, nullptr);
}

// The cells' objective terms (mode 2 above): the assign kernel's dots and D, R only read
template <int NU>
__global__ __launch_bounds__(256) void harmony_objective_kernel(const double *__restrict__ Zh, const double *__restrict__ Y, const int *__restrict__ batch,
                                                                const double *__restrict__ R, const double *__restrict__ L, long long n, int d,
                                                                int K, int dp, int KT, double sigma, double theta, double *__restrict__ obj) {
    harmony_cells<NU>(Zh, Y, batch, L, 0, n, d, K, dp, KT, sigma, theta, 2, const_cast<double *>(R), nullptr, obj);
}

// R[pos, k] = 1 where a[pos] = k, else 0: the Lloyd rounds' sums go through the same slabs as every other sum
__global__ __launch_bounds__(256) void harmony_onehot_kernel(const int *__restrict__ a, long long n, int K, double *__restrict__ R) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * K) return;
    const long long pos = e / K;
    R[e] = a[pos] == static_cast<int>(e - pos * K) ? 1.0 : 0.0;
}

// One workgroup per slab (slab0 + blockIdx.x), thread k: part[slab, k] = the sum of R[cell, k] over the slab's cells, ascending
__global__ __launch_bounds__(256) void harmony_colsum_kernel(const double *__restrict__ R, const long long *__restrict__ slab_cell, long long slab0,
                                                             int K, double *__restrict__ part) {
    const long long sl = slab0 + blockIdx.x;
    const int k = threadIdx.x;
    if (k >= K) return;
    const long long b = slab_cell[sl], e = slab_cell[sl + 1];
    double s = 0.0;
    for (long long cell = b; cell < e; ++cell) s += R[cell * K + k];
    part[sl * K + k] = s;
}

// One workgroup per cluster k, the threads strided over the batches.  Oseg[j, b, k] = the fold of segment (j, b)'s slabs in slab order,
// taken anew for j = refresh (-2: every block, -1: none).  O[b, k] = the fold over the blocks j != skip in block order; tot = the sum of
// O[., k] (256 strided running folds, then a tree); E = Pr[b] tot; P[b, k] = ((E + 1) / (O + 1))^theta; L[b, k] = log((O + 1) / (E + 1)).
__global__ __launch_bounds__(256) void harmony_table_kernel(const double *__restrict__ part, const long long *__restrict__ seg_slab, int n_blocks,
                                                            int B, int K, int skip, int refresh, const double *__restrict__ Pr, double theta,
                                                            double *__restrict__ Oseg, double *__restrict__ O, double *__restrict__ P,
                                                            double *__restrict__ L) {
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double run = 0.0;
    for (int b = tid; b < B; b += 256) {
        double o = 0.0;
        for (int j = 0; j < n_blocks; ++j) {
            const long long sg = static_cast<long long>(j) * B + b;
            if (refresh == -2 || refresh == j) {
                double s = 0.0;
                for (long long sl = seg_slab[sg]; sl < seg_slab[sg + 1]; ++sl) s += part[sl * K + k];
                Oseg[sg * K + k] = s;
            }
            if (j != skip) o += Oseg[sg * K + k];
        }
        O[static_cast<long long>(b) * K + k] = o;
        run += o;
    }
    red[tid] = run;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double tot = red[0];
    for (int b = tid; b < B; b += 256) {
        const long long at = static_cast<long long>(b) * K + k;
        const double o = O[at], e = Pr[b] * tot;
        P[at] = pow((e + 1.0) / (o + 1.0), theta);
        L[at] = log((o + 1.0) / (e + 1.0));
    }
}

// One thread per entry e of K x d and batch b (blockIdx.y): S[b, e] = the fold of the slabs' products gp[slab, e] -- a segment's slabs in
// slab order, the batch's segments in block order
__global__ __launch_bounds__(256) void harmony_fold_kernel(const double *__restrict__ gp, const long long *__restrict__ seg_slab, int n_blocks, int B,
                                                           long long kd, double *__restrict__ S) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= kd) return;
    const int b = blockIdx.y;
    double sb = 0.0;
    for (int j = 0; j < n_blocks; ++j) {
        const long long sg = static_cast<long long>(j) * B + b;
        const long long s0 = seg_slab[sg], s1 = seg_slab[sg + 1];
        if (s0 == s1) continue;
        double s = 0.0;
        for (long long sl = s0; sl < s1; ++sl) s += gp[sl * kd + e];
        sb += s;
    }
    S[static_cast<long long>(b) * kd + e] = sb;
}

// T[e] = the fold of S[b, e] over the batches in batch order
__global__ __launch_bounds__(256) void harmony_total_kernel(const double *__restrict__ S, int B, long long kd, double *__restrict__ T) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= kd) return;
    double tot = 0.0;
    for (int b = 0; b < B; ++b) tot += S[static_cast<long long>(b) * kd + e];
    T[e] = tot;
}

// One wave per cell, lanes over the d columns (two per lane above 64): out[dst, :] = Z[cell, :] - sum over k (ascending) of R[cell, k]
// W[batch, k, :]; dst = order[cell], or the cell itself
__global__ __launch_bounds__(256) void harmony_correct_kernel(const double *__restrict__ Z, const double *__restrict__ R, const int *__restrict__ batch,
                                                              const double *__restrict__ W, const int *__restrict__ order, long long n, int d, int K,
                                                              double *__restrict__ out) {
    const long long cell = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (cell >= n) return;
    const int lane = threadIdx.x & 63;
    const double *Wb = W + static_cast<long long>(batch[cell]) * K * d;
    const double *r = R + cell * K;
    const bool h0 = lane < d, h1 = lane + 64 < d;
    double a0 = 0.0, a1 = 0.0;
    for (int k = 0; k < K; ++k) {
        const double rk = r[k];
        if (h0) a0 += rk * Wb[static_cast<long long>(k) * d + lane];
        if (h1) a1 += rk * Wb[static_cast<long long>(k) * d + lane + 64];
    }
    const long long dst = order ? order[cell] : cell;
    if (h0) out[dst * d + lane] = Z[cell * d + lane] - a0;
    if (h1) out[dst * d + lane + 64] = Z[cell * d + lane + 64] - a1;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------

struct Shape {
    long long n;
    int d, K, B, n_blocks;
};

void check_shape(const std::string &w, long long n, int d, int K, int B) {
    SHARP_REQUIRE(n >= 1 && n <= kHarmonyMaxN, w + ": need 1 <= n <= 2^31 - 2 cells");
    SHARP_REQUIRE(d >= 2 && d <= kHarmonyMaxD, w + ": need 2 <= d <= 128 columns");
    SHARP_REQUIRE(B != 1, w + ": one batch: nothing to integrate");
    SHARP_REQUIRE(B >= 2 && B <= kHarmonyMaxB, w + ": need 2 <= batches <= 4096");
    SHARP_REQUIRE(K <= n, w + ": n_clusters exceeds the number of cells");
    SHARP_REQUIRE(K >= 2 && K <= kHarmonyMaxK, w + ": need 2 <= n_clusters <= min(n, 256)");
}

void check_blocks(const std::string &w, int n_blocks) {
    SHARP_REQUIRE(n_blocks >= 1 && n_blocks <= kHarmonyMaxBlocks, w + ": need 1 <= n_blocks <= 1024");
}

// the batch codes lie in [0, B) and every code occurs; returns the cells per batch
std::vector<long long> check_batch(const std::string &w, const int *batch, long long n, int B) {
    std::vector<long long> nb(B, 0);
    for (long long i = 0; i < n; ++i) {
        SHARP_REQUIRE(batch[i] >= 0 && batch[i] < B, w + ": a batch code outside [0, batches) (cell " + std::to_string(i) + ", counted from 0)");
        ++nb[batch[i]];
    }
    for (int b = 0; b < B; ++b) SHARP_REQUIRE(nb[b] > 0, w + ": an empty batch code (" + std::to_string(b) + ")");
    return nb;
}

void check_finite(const std::string &w, const char *what, const double *v, long long count, int per) {
    for (long long e = 0; e < count; ++e)
        SHARP_REQUIRE(std::isfinite(v[e]), w + ": a non-finite value in " + what + " (row " + std::to_string(e / per) + ", counted from 0)");
}

void check_rows(const std::string &w, const double *Z, long long n, int d) {
    for (long long i = 0; i < n; ++i) {
        bool any = false;
        for (int c = 0; c < d; ++c) {
            const double v = Z[i * d + c];
            SHARP_REQUIRE(std::isfinite(v), w + ": a non-finite value in Z (cell " + std::to_string(i) + ", counted from 0)");
            any = any || v != 0.0;
        }
        SHARP_REQUIRE(any, w + ": a zero row in Z (cell " + std::to_string(i) + ", counted from 0)");
    }
}

// the working order's tables, from the batches in working order (host)
struct Layout {
    std::vector<long long> seg_cell;             // n_blocks B + 1: a segment's cells
    std::vector<long long> seg_slab;             // n_blocks B + 1: a segment's slabs
    std::vector<long long> slab_cell;            // nslab + 1: a slab's cells (a segment's last slab ends where the segment ends)
    long long nslab = 0;
};

Layout make_layout(const int *batch, long long n, int B, int n_blocks, u64 seed) {
    Layout Lo;
    const long long nseg = static_cast<long long>(n_blocks) * B;
    Lo.seg_cell.assign(nseg + 1, 0);
    for (long long i = 0; i < n; ++i) {
        const long long blk = static_cast<long long>(harmony_hash(seed, 0, static_cast<u64>(i)) % static_cast<u64>(n_blocks));
        ++Lo.seg_cell[blk * B + batch[i] + 1];
    }
    for (long long s = 0; s < nseg; ++s) Lo.seg_cell[s + 1] += Lo.seg_cell[s];
    Lo.seg_slab.assign(nseg + 1, 0);
    for (long long s = 0; s < nseg; ++s)
        Lo.seg_slab[s + 1] = Lo.seg_slab[s] + (Lo.seg_cell[s + 1] - Lo.seg_cell[s] + kHarmonySlab - 1) / kHarmonySlab;
    Lo.nslab = Lo.seg_slab[nseg];
    Lo.slab_cell.assign(Lo.nslab + 1, n);
    for (long long s = 0; s < nseg; ++s)
        for (long long sl = Lo.seg_slab[s]; sl < Lo.seg_slab[s + 1]; ++sl) Lo.slab_cell[sl] = Lo.seg_cell[s] + (sl - Lo.seg_slab[s]) * kHarmonySlab;
    // (slab_cell[sl + 1] of a segment's last slab is the next segment's first cell, or n: where the segment ends)
    return Lo;
}

double bytes_needed(const Shape &s, long long nslab_max) {
    const double n = static_cast<double>(s.n), kd = static_cast<double>(s.K) * s.d, bk = static_cast<double>(s.B) * s.K;
    double b = n * s.d * 32.0 + n * s.K * 8.0 + n * 8.0;                       // Z, Zw, Zhat, Z_corr; R; the objective's terms
    b += n * 44.0 + n * 16.0;                                                   // keys, order, batches, a; the sort's storage
    b += static_cast<double>(nslab_max) * (kd + s.K + 1.0) * 8.0 + static_cast<double>(nslab_max) * 2.0 * sizeof(GemmTask);
    b += static_cast<double>(s.n_blocks) * bk * 8.0 + static_cast<double>(s.n_blocks) * s.B * 16.0;
    b += 2.0 * bk * s.d * 8.0 + 3.0 * bk * 8.0 + 2.0 * kd * 8.0;
    return b + 67108864.0;
}

void check_memory(const std::string &w, const Shape &s) {
    // (every segment that holds a cell ends in one slab that may be short)
    const long long nslab_max = s.n / kHarmonySlab + std::min<long long>(s.n, static_cast<long long>(s.n_blocks) * s.B);
    size_t free_b = 0, total_b = 0;
    SHARP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const double need = bytes_needed(s, nslab_max);
    SHARP_REQUIRE(need <= static_cast<double>(free_b), w + ": the workspaces need about " + std::to_string(static_cast<long long>(need / 1048576.0)) +
                                                          " MB; the device has " + std::to_string(free_b >> 20) + " MB free");
}

// everything a call holds on the device, in working order unless said otherwise
struct Work {
    Shape s;
    Layout lo;
    DevBuf<int> order, batch;                    // n: the cell at a position; its batch
    DevBuf<double> Zw, Zh, R, Y;                 // n x d, n x d, n x K, K x d
    DevBuf<long long> seg_slab, slab_cell;
    DevBuf<double> gpart, cpart, Oseg, O, P, L, Pr, T, S;
    DevBuf<GemmTask> tasks_h, tasks_w;           // R^T Zh, R^T Zw
};

void launch_assign(const Work &W, const double *Zh, const double *Y, const int *batch, const double *P, long long c0, long long c1, double sigma,
                   int argmax, double *R, int *a, const char *tname) {
    if (c1 <= c0) return;
    Ctx &c = ctx();
    KernelTimer timer(tname);
    const int d = W.s.d, K = W.s.K;
    const int dp = d | 1;
    const int KT = std::min(K, kHarmonyLdsTile / dp);
    const long long groups = (c1 - c0 + 4 * kHarmonyWaveCells - 1) / (4 * kHarmonyWaveCells);
    const unsigned grid = static_cast<unsigned>(std::min<long long>(groups, static_cast<long long>(c.num_cu) * 3));   // (48 KB of LDS: three a CU)
    const int nu = (K + 63) / 64;
#define SHARP_HARMONY_ASSIGN(NU)                                                                                                              \
    hipLaunchKernelGGL(harmony_assign_kernel<NU>, dim3(grid), dim3(256), 0, c.stream, Zh, Y, batch, P, c0, c1, d, K, dp, KT, sigma, argmax, R, a)
    if (nu == 1) SHARP_HARMONY_ASSIGN(1);
    else if (nu == 2) SHARP_HARMONY_ASSIGN(2);
    else if (nu == 3) SHARP_HARMONY_ASSIGN(3);
    else SHARP_HARMONY_ASSIGN(4);
#undef SHARP_HARMONY_ASSIGN
    launch_check("harmony_assign_kernel");
}

// obj[pos] = the objective's term of every cell (working order), from L = log((O + 1) / (E + 1)) of all blocks
void launch_objective(const Work &W, const double *L, double sigma, double theta, double *obj) {
    Ctx &c = ctx();
    const int d = W.s.d, K = W.s.K;
    const int dp = d | 1;
    const int KT = std::min(K, kHarmonyLdsTile / dp);
    const long long groups = (W.s.n + 4 * kHarmonyWaveCells - 1) / (4 * kHarmonyWaveCells);
    const unsigned grid = static_cast<unsigned>(std::min<long long>(groups, static_cast<long long>(c.num_cu) * 3));
    const int nu = (K + 63) / 64;
#define SHARP_HARMONY_OBJECTIVE(NU)                                                                                                           \
    hipLaunchKernelGGL(harmony_objective_kernel<NU>, dim3(grid), dim3(256), 0, c.stream, W.Zh.p, W.Y.p, W.batch.p, W.R.p, L, W.s.n, d, K, dp, KT, \
                       sigma, theta, obj)
    if (nu == 1) SHARP_HARMONY_OBJECTIVE(1);
    else if (nu == 2) SHARP_HARMONY_OBJECTIVE(2);
    else if (nu == 3) SHARP_HARMONY_OBJECTIVE(3);
    else SHARP_HARMONY_OBJECTIVE(4);
#undef SHARP_HARMONY_OBJECTIVE
    launch_check("harmony_objective_kernel");
}

// the layout's tables on the device, the slabs' workspaces and the GEMM tasks of R^T Zh and R^T Zw (Zw may be null)
void setup_sums(Work &W, bool tables) {
    const Shape &s = W.s;
    const Layout &lo = W.lo;
    const long long kd = static_cast<long long>(s.K) * s.d, bk = static_cast<long long>(s.B) * s.K;
    W.seg_slab.alloc(lo.seg_slab.size());
    W.seg_slab.upload(lo.seg_slab.data(), lo.seg_slab.size());
    W.slab_cell.alloc(lo.slab_cell.size());
    W.slab_cell.upload(lo.slab_cell.data(), lo.slab_cell.size());
    W.gpart.alloc(static_cast<size_t>(lo.nslab) * kd);
    W.cpart.alloc(static_cast<size_t>(lo.nslab) * s.K);
    W.Oseg.alloc(static_cast<size_t>(s.n_blocks) * bk);
    W.T.alloc(kd);
    if (tables) {
        W.O.alloc(bk);
        W.P.alloc(bk);
        W.L.alloc(bk);
    }
    std::vector<GemmTask> th(lo.nslab), tw(lo.nslab);
    for (long long sl = 0; sl < lo.nslab; ++sl) {
        GemmTask t{};
        const long long b = lo.slab_cell[sl];
        t.At = W.R.p + b * s.K;
        t.Bt = W.Zh.p ? W.Zh.p + b * s.d : nullptr;
        t.C = W.gpart.p + sl * kd;
        t.M = s.K;
        t.N = s.d;
        t.K = static_cast<int>(std::min<long long>(lo.slab_cell[sl + 1] - b, kHarmonySlab));
        t.lda = s.K;
        t.ldb = t.ldc = s.d;
        th[sl] = t;
        t.Bt = W.Zw.p ? W.Zw.p + b * s.d : nullptr;
        tw[sl] = t;
    }
    W.tasks_h.alloc(lo.nslab);
    W.tasks_h.upload(th.data(), lo.nslab);
    W.tasks_w.alloc(lo.nslab);
    W.tasks_w.upload(tw.data(), lo.nslab);
    stream_sync();                                           // (the host tables go)
}

// S[b] = R^T X over the batch's cells and T = their fold over the batches; X's tasks
void sums(Work &W, const GemmTask *tasks, double *S, const char *tname) {
    Ctx &c = ctx();
    const long long kd = static_cast<long long>(W.s.K) * W.s.d;
    gemm_tn_f64_batched(tasks, static_cast<int>(W.lo.nslab), W.s.K, W.s.d, tname);
    KernelTimer timer(tname);
    hipLaunchKernelGGL(harmony_fold_kernel, dim3(grid_for(kd, 256), W.s.B), dim3(256), 0, c.stream, W.gpart.p, W.seg_slab.p, W.s.n_blocks, W.s.B, kd,
                       S);
    hipLaunchKernelGGL(harmony_total_kernel, dim3(grid_for(kd, 256)), dim3(256), 0, c.stream, S, W.s.B, kd, W.T.p);
    launch_check("harmony_fold_kernel");
}

// the column sums of the slabs [s0, s1)
void colsums(Work &W, long long s0, long long s1, const char *tname) {
    if (s1 <= s0) return;
    Ctx &c = ctx();
    KernelTimer timer(tname);
    for (long long b = s0; b < s1; b += 1 << 30) {
        const unsigned grid = static_cast<unsigned>(std::min<long long>(s1 - b, 1 << 30));
        hipLaunchKernelGGL(harmony_colsum_kernel, dim3(grid), dim3(256), 0, c.stream, W.R.p, W.slab_cell.p, b, W.s.K, W.cpart.p);
    }
    launch_check("harmony_colsum_kernel");
}

void table(Work &W, int skip, int refresh, double theta, const char *tname) {
    Ctx &c = ctx();
    KernelTimer timer(tname);
    hipLaunchKernelGGL(harmony_table_kernel, dim3(W.s.K), dim3(256), 0, c.stream, W.cpart.p, W.seg_slab.p, W.s.n_blocks, W.s.B, W.s.K, skip, refresh,
                       W.Pr.p, theta, W.Oseg.p, W.O.p, W.P.p, W.L.p);
    launch_check("harmony_table_kernel");
}

void normalize(const double *src, const int *idx, long long rows, int d, bool keep, double *dst) {
    hipLaunchKernelGGL(harmony_normalize_kernel, dim3(grid_for(rows, 4)), dim3(256), 0, ctx().stream, src, idx, rows, d, keep ? 1 : 0, dst);
    launch_check("harmony_normalize_kernel");
}

// order (n ints on the device) = the cells sorted by (block, batch, i)
void working_order(const int *d_batch, long long n, int B, int n_blocks, u64 seed, DevBuf<int> &order) {
    Ctx &c = ctx();
    DevBuf<u64> keys(n), keys_s(n);
    DevBuf<int> src(n);
    Scratch tmp;
    order.alloc(n);
    hipLaunchKernelGGL(harmony_keys_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, d_batch, n, B, n_blocks, seed, keys.p, src.p);
    launch_check("harmony_keys_kernel");
    sort_pairs(keys.p, keys_s.p, src.p, order.p, static_cast<size_t>(n), 0, key_bits(static_cast<u64>(n_blocks) * B), tmp);
    stream_sync();                                           // (the temporaries leave scope)
}

struct Params {
    double sigma, theta, lam, eps_cluster, eps_harmony;
    int max_iter, max_iter_cluster, init_iter;
    u64 seed;
};

void check_params(const std::string &w, const Params &p) {
    SHARP_REQUIRE(std::isfinite(p.sigma) && p.sigma > 0.0, w + ": sigma must be > 0");
    SHARP_REQUIRE(std::isfinite(p.theta) && p.theta >= 0.0, w + ": theta must be >= 0");
    SHARP_REQUIRE(std::isfinite(p.lam) && p.lam > 0.0, w + ": lam must be > 0");
    SHARP_REQUIRE(p.max_iter >= 1 && p.max_iter_cluster >= 1 && p.init_iter >= 0, w + ": need max_iter >= 1, max_iter_cluster >= 1, init_iter >= 0");
    SHARP_REQUIRE(std::isfinite(p.eps_cluster) && p.eps_cluster >= 0.0 && std::isfinite(p.eps_harmony) && p.eps_harmony >= 0.0,
                  w + ": epsilon_cluster and epsilon_harmony must be finite and >= 0");
}

// W[b, k, :] (host) from N[b, k] and S[b, k, :]: the closed form of the ridge system with an unpenalised intercept
void ridge(const std::vector<double> &N, const std::vector<double> &S, int B, int K, int d, double lam, std::vector<double> &Wt) {
    Wt.assign(static_cast<size_t>(B) * K * d, 0.0);
    std::vector<double> num(d);
    for (int k = 0; k < K; ++k) {
        double sq = 0.0;
        std::fill(num.begin(), num.end(), 0.0);
        for (int b = 0; b < B; ++b) {
            const double nb = N[static_cast<size_t>(b) * K + k];
            const double q = nb / (nb + lam);
            sq += q;
            const double *sv = &S[(static_cast<size_t>(b) * K + k) * d];
            for (int c = 0; c < d; ++c) num[c] += sv[c] - q * sv[c];
        }
        const double s = lam * sq;
        if (!(s > 0.0)) continue;
        for (int b = 0; b < B; ++b) {
            const double nb = N[static_cast<size_t>(b) * K + k];
            const double *sv = &S[(static_cast<size_t>(b) * K + k) * d];
            double *wv = &Wt[(static_cast<size_t>(b) * K + k) * d];
            for (int c = 0; c < d; ++c) wv[c] = (sv[c] - nb * (num[c] / s)) / (nb + lam);
        }
    }
}

void harmony_run(const std::string &w, const double *Z, const int *batch, const Shape &s, const std::vector<long long> &nb, const Params &p,
                 double *Z_corr, double *Yout, double *objective, int *rounds, int *n_iter, int *converged, double *Rout) {
    Ctx &c = ctx();
    check_memory(w, s);
    const long long n = s.n;
    const int d = s.d, K = s.K, B = s.B;
    const long long kd = static_cast<long long>(K) * d, bk = static_cast<long long>(B) * K;
    Work W;
    W.s = s;
    DevBuf<double> Zin(static_cast<size_t>(n) * d), Zc(static_cast<size_t>(n) * d), obj(n), red(kRedBlocks), objv(1), Wd(bk * d);
    DevBuf<int> bin(n), a(n), start(K);
    {
        KernelTimer timer("harmony_init");
        Zin.upload(Z, static_cast<size_t>(n) * d);
        bin.upload(batch, n);
        working_order(bin.p, n, B, s.n_blocks, p.seed, W.order);
        W.lo = make_layout(batch, n, B, s.n_blocks, p.seed);
        W.Zw.alloc(static_cast<size_t>(n) * d);
        W.Zh.alloc(static_cast<size_t>(n) * d);
        W.R.alloc(static_cast<size_t>(n) * K);
        W.Y.alloc(kd);
        W.batch.alloc(n);
        W.S.alloc(bk * d);
        W.Pr.alloc(B);
        std::vector<double> pr(B);
        for (int b = 0; b < B; ++b) pr[b] = static_cast<double>(nb[b]) / static_cast<double>(n);
        W.Pr.upload(pr.data(), B);
        setup_sums(W, true);
        hipLaunchKernelGGL(harmony_gather_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, c.stream, Zin.p, W.order.p, n, d, W.Zw.p, bin.p,
                           W.batch.p);
        launch_check("harmony_gather_kernel");
        normalize(Zin.p, W.order.p, n, d, false, W.Zh.p);
        // the start cells: the K smallest h(1, i), ties to the lower i
        std::vector<std::pair<u64, int>> hs(n);
        for (long long i = 0; i < n; ++i) hs[i] = {harmony_hash(p.seed, 1, static_cast<u64>(i)), static_cast<int>(i)};
        std::partial_sort(hs.begin(), hs.begin() + K, hs.end());
        std::vector<int> st(K);
        for (int k = 0; k < K; ++k) st[k] = hs[k].second;
        start.upload(st.data(), K);
        normalize(Zin.p, start.p, K, d, false, W.Y.p);
        stream_sync();                                       // (pr, st go)
    }
    for (int it = 0; it < p.init_iter; ++it) {
        launch_assign(W, W.Zh.p, W.Y.p, W.batch.p, nullptr, 0, n, p.sigma, 1, nullptr, a.p, "harmony_init");
        {
            KernelTimer timer("harmony_init");
            hipLaunchKernelGGL(harmony_onehot_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, c.stream, a.p, n, K, W.R.p);
            launch_check("harmony_onehot_kernel");
        }
        sums(W, W.tasks_h.p, W.S.p, "harmony_init");
        normalize(W.T.p, nullptr, K, d, true, W.Y.p);
    }
    launch_assign(W, W.Zh.p, W.Y.p, W.batch.p, nullptr, 0, n, p.sigma, 0, W.R.p, nullptr, "harmony_init");
    colsums(W, 0, W.lo.nslab, "harmony_init");
    int stale = -2;                                          // the block whose table the next table kernel takes anew (-2: all, -1: none)
    std::vector<double> Nh(bk), Sh(bk * d), Wh;
    double last_prev = 0.0;
    int t = 0;
    *converged = 0;
    for (t = 0; t < p.max_iter; ++t) {
        double prev = 0.0, cur = 0.0;
        int r = 0;
        for (r = 1; r <= p.max_iter_cluster; ++r) {
            sums(W, W.tasks_h.p, W.S.p, "harmony_sums");
            normalize(W.T.p, nullptr, K, d, true, W.Y.p);
            for (int j = 0; j < s.n_blocks; ++j) {
                const long long sg0 = static_cast<long long>(j) * B, sg1 = sg0 + B;
                const long long c0 = W.lo.seg_cell[sg0], c1 = W.lo.seg_cell[sg1];
                if (c1 == c0) continue;
                table(W, j, stale, p.theta, "harmony_sums");
                launch_assign(W, W.Zh.p, W.Y.p, W.batch.p, W.P.p, c0, c1, p.sigma, 0, W.R.p, nullptr, "harmony_assign");
                colsums(W, W.lo.seg_slab[sg0], W.lo.seg_slab[sg1], "harmony_sums");
                stale = j;
            }
            table(W, -1, stale, p.theta, "harmony_sums");
            stale = -1;
            {
                KernelTimer timer("harmony_objective");
                launch_objective(W, W.L.p, p.sigma, p.theta, obj.p);
                fixed_reduce(Fold::Sum, obj.p, n, red.p, objv.p);
            }
            prev = cur;
            objv.download(&cur, 1);                          // the round's one synchronisation
            SHARP_REQUIRE(std::isfinite(cur), w + ": the objective is not finite (round " + std::to_string(r) + " of iteration " + std::to_string(t + 1) + ")");
            if (p.eps_cluster > 0.0 && r >= 2 && prev - cur < p.eps_cluster * std::fabs(prev)) { ++r; break; }
        }
        rounds[t] = r - 1;
        objective[t] = cur;
        sums(W, W.tasks_w.p, W.S.p, "harmony_correct");
        W.O.download(Nh.data(), bk);
        W.S.download(Sh.data(), bk * d);
        ridge(Nh, Sh, B, K, d, p.lam, Wh);
        {
            KernelTimer timer("harmony_correct");
            Wd.upload(Wh.data(), bk * d);
            hipLaunchKernelGGL(harmony_correct_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, W.Zw.p, W.R.p, W.batch.p, Wd.p, W.order.p, n, d, K,
                               Zc.p);
            launch_check("harmony_correct_kernel");
            normalize(Zc.p, W.order.p, n, d, false, W.Zh.p);
            stream_sync();                                   // (Wh is written again)
        }
        if (p.eps_harmony > 0.0 && t >= 1 && last_prev - cur < p.eps_harmony * std::fabs(last_prev)) {
            *converged = 1;
            ++t;
            break;
        }
        last_prev = cur;
    }
    *n_iter = t;
    Zc.download(Z_corr, static_cast<size_t>(n) * d);
    W.Y.download(Yout, kd);
    if (Rout) {
        std::vector<double> Rw(static_cast<size_t>(n) * K);
        W.R.download(Rw.data(), Rw.size());
        std::vector<int> order(n);
        W.order.download(order.data(), n);
        for (long long pos = 0; pos < n; ++pos) std::copy(&Rw[pos * K], &Rw[pos * K] + K, Rout + static_cast<long long>(order[pos]) * K);
    }
    stream_sync();
}

}  // namespace
}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_harmony_caps(int *slab, int *lds_tile) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(slab && lds_tile, "harmony_caps: null output");
    *slab = kHarmonySlab;
    *lds_tile = kHarmonyLdsTile;
    SHARP_API_END
}

int sharp_harmony_assign(const double *Zhat, const double *Y, const int *batch, const double *P, long long n, int d, int K, int B, long long i0,
                         long long i1, double sigma, int argmax, double *R, int *a) {
    SHARP_API_BEGIN
    const std::string w("harmony_assign");
    SHARP_REQUIRE(Zhat && Y && batch && (argmax ? a != nullptr : R != nullptr), w + ": null Zhat / Y / batch / output");
    check_shape(w, n, d, K, B);
    SHARP_REQUIRE(i0 >= 0 && i0 <= i1 && i1 <= n, w + ": need 0 <= i0 <= i1 <= n");
    SHARP_REQUIRE(std::isfinite(sigma) && sigma > 0.0, w + ": sigma must be > 0");
    check_batch(w, batch, n, B);
    check_finite(w, "Zhat", Zhat, n * d, d);
    check_finite(w, "Y", Y, static_cast<long long>(K) * d, d);
    if (P) check_finite(w, "P", P, static_cast<long long>(B) * K, K);
    ctx();
    Work W;
    W.s = Shape{n, d, K, B, 1};
    check_memory(w, W.s);
    DevBuf<double> dz(static_cast<size_t>(n) * d), dy(static_cast<size_t>(K) * d), dp(P ? static_cast<size_t>(B) * K : 0), dr(argmax ? 0 : static_cast<size_t>(n) * K);
    DevBuf<int> db(n), da(argmax ? n : 0);
    dz.upload(Zhat, dz.n);
    dy.upload(Y, dy.n);
    db.upload(batch, n);
    if (P) dp.upload(P, dp.n);
    if (argmax) da.upload(a, n); else dr.upload(R, dr.n);    // (the rows outside [i0, i1) come back as they went)
    launch_assign(W, dz.p, dy.p, db.p, P ? dp.p : nullptr, i0, i1, sigma, argmax ? 1 : 0, dr.p, da.p, "harmony_assign");
    if (argmax) da.download(a, n); else dr.download(R, dr.n);
    stream_sync();
    SHARP_API_END
}

int sharp_harmony_sums(const double *R, const double *X, const int *batch, long long n, int d, int K, int B, long long seed, int n_blocks, double *O,
                       double *S) {
    SHARP_API_BEGIN
    const std::string w("harmony_sums");
    SHARP_REQUIRE(R && X && batch && O && S, w + ": null R / X / batch / O / S");
    check_shape(w, n, d, K, B);
    check_blocks(w, n_blocks);
    check_batch(w, batch, n, B);
    check_finite(w, "R", R, n * K, K);
    check_finite(w, "X", X, n * d, d);
    Ctx &c = ctx();
    Work W;
    W.s = Shape{n, d, K, B, n_blocks};
    check_memory(w, W.s);
    const long long bk = static_cast<long long>(B) * K;
    DevBuf<double> rin(static_cast<size_t>(n) * K), xin(static_cast<size_t>(n) * d);
    DevBuf<int> bin(n);
    rin.upload(R, rin.n);
    xin.upload(X, xin.n);
    bin.upload(batch, n);
    working_order(bin.p, n, B, n_blocks, static_cast<u64>(seed), W.order);
    W.lo = make_layout(batch, n, B, n_blocks, static_cast<u64>(seed));
    W.R.alloc(static_cast<size_t>(n) * K);
    W.Zw.alloc(static_cast<size_t>(n) * d);
    W.batch.alloc(n);
    W.S.alloc(bk * d);
    hipLaunchKernelGGL(harmony_gather_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, c.stream, rin.p, W.order.p, n, K, W.R.p, bin.p, W.batch.p);
    hipLaunchKernelGGL(harmony_gather_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, c.stream, xin.p, W.order.p, n, d, W.Zw.p,
                       static_cast<const int *>(nullptr), static_cast<int *>(nullptr));
    launch_check("harmony_gather_kernel");
    std::vector<double> pr(B, 0.0);
    W.Pr.alloc(B);
    W.Pr.upload(pr.data(), B);
    setup_sums(W, true);
    sums(W, W.tasks_w.p, W.S.p, "harmony_sums");
    colsums(W, 0, W.lo.nslab, "harmony_sums");
    table(W, -1, -2, 0.0, "harmony_sums");
    W.Oseg.download(O, static_cast<size_t>(n_blocks) * bk);
    W.S.download(S, bk * d);
    stream_sync();
    SHARP_API_END
}

int sharp_harmony_ridge(const double *N, const double *S, int B, int K, int d, double lam, double *W) {
    SHARP_API_BEGIN
    const std::string w("harmony_ridge");
    SHARP_REQUIRE(N && S && W, w + ": null N / S / W");
    SHARP_REQUIRE(d >= 2 && d <= kHarmonyMaxD, w + ": need 2 <= d <= 128 columns");
    SHARP_REQUIRE(B >= 2 && B <= kHarmonyMaxB, w + ": need 2 <= batches <= 4096");
    SHARP_REQUIRE(K >= 2 && K <= kHarmonyMaxK, w + ": need 2 <= n_clusters <= 256");
    SHARP_REQUIRE(std::isfinite(lam) && lam > 0.0, w + ": lam must be > 0");
    const size_t bk = static_cast<size_t>(B) * K;
    for (size_t e = 0; e < bk; ++e) SHARP_REQUIRE(std::isfinite(N[e]) && N[e] >= 0.0, w + ": N must be finite and >= 0");
    check_finite(w, "S", S, static_cast<long long>(bk) * d, K * d);
    const std::vector<double> Nv(N, N + bk), Sv(S, S + bk * d);
    std::vector<double> Wt;
    ridge(Nv, Sv, B, K, d, lam, Wt);                         // the function the whole call runs between its sums and its correction
    std::copy(Wt.begin(), Wt.end(), W);
    SHARP_API_END
}

int sharp_harmony_correct(const double *Z, const double *R, const int *batch, const double *W, long long n, int d, int K, int B, double *Z_corr) {
    SHARP_API_BEGIN
    const std::string w("harmony_correct");
    SHARP_REQUIRE(Z && R && batch && W && Z_corr, w + ": null Z / R / batch / W / Z_corr");
    check_shape(w, n, d, K, B);
    check_batch(w, batch, n, B);
    check_finite(w, "Z", Z, n * d, d);
    check_finite(w, "R", R, n * K, K);
    check_finite(w, "W", W, static_cast<long long>(B) * K * d, K * d);
    Ctx &c = ctx();
    check_memory(w, Shape{n, d, K, B, 1});
    DevBuf<double> dz(static_cast<size_t>(n) * d), dr(static_cast<size_t>(n) * K), dw(static_cast<size_t>(B) * K * d), out(static_cast<size_t>(n) * d);
    DevBuf<int> db(n);
    dz.upload(Z, dz.n);
    dr.upload(R, dr.n);
    dw.upload(W, dw.n);
    db.upload(batch, n);
    {
        KernelTimer timer("harmony_correct");
        hipLaunchKernelGGL(harmony_correct_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, dz.p, dr.p, db.p, dw.p, static_cast<const int *>(nullptr),
                           n, d, K, out.p);
        launch_check("harmony_correct_kernel");
    }
    out.download(Z_corr, out.n);
    SHARP_API_END
}

int sharp_harmony(const double *Z, long long n, int d, const int *batch, int n_batches, int n_clusters, double sigma, double theta, double lam,
                  int max_iter, int max_iter_cluster, int n_blocks, double epsilon_cluster, double epsilon_harmony, int init_iter, long long seed,
                  double *Z_corr, double *Y, double *objective, int *rounds, int *n_iter, int *converged, double *R) {
    SHARP_API_BEGIN
    const std::string w("harmony_integrate");
    SHARP_REQUIRE(Z && batch && Z_corr && Y && objective && rounds && n_iter && converged, w + ": null Z / batch / output");
    check_shape(w, n, d, n_clusters, n_batches);
    check_blocks(w, n_blocks);
    const Params p{sigma, theta, lam, epsilon_cluster, epsilon_harmony, max_iter, max_iter_cluster, init_iter, static_cast<u64>(seed)};
    check_params(w, p);
    const std::vector<long long> nb = check_batch(w, batch, n, n_batches);
    check_rows(w, Z, n, d);
    ctx();
    harmony_run(w, Z, batch, Shape{n, d, n_clusters, n_batches, n_blocks}, nb, p, Z_corr, Y, objective, rounds, n_iter, converged, R);
    SHARP_API_END
}

}  // extern "C"
