// knn.hip -- the exact k-NN (knn.hpp).
//   self search      distances ||w_i||^2 + ||w_j||^2 - 2 w_i.w_j of the centred rows w = x - mean on v_mfma_f64_16x16x4_f64 over streamed
//                    column tiles, a per-row top-K in LDS behind a threshold filter, the chosen K re-ranked by a direct sum (x_i - x_j)^2
//   cross search     the same between query rows and a reference, the query block's A fragments loaded once per workgroup
//   given distances  R's dist vector expanded to the full matrix (dist.hip), one wave per row selecting its K smallest entries
//   given lists      a validation kernel, then the caller's lists as they are
// No floating-point atomics; every comparison is exact, so a row's list depends on neither the launch split nor the chunking.
#include "knn.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>

#include "dist_pairs.hpp"
#include "knn_dev.hpp"
#include "prepare.hpp"

namespace sharp {
namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
constexpr int KREG = 16;      // k-steps of four columns whose A fragments stay in registers (the cross search)
constexpr size_t LDS_MAX = 160 * 1024;   // LDS of a gfx950 compute unit

// ---- the self search ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rownorm_kernel(const double *__restrict__ X, long long n, int d, double *__restrict__ nrm) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int c = 0; c < d; ++c) { const double t = X[i * d + c]; a += t * t; }
    nrm[i] = a;
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
    wave_sync();
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
    wave_sync();
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
    wave_sync();
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p], rank = knn_rank(Ld, Li, K, dp, ip);
        out_idx[qq * K + rank] = ip < n ? ip : -1;
        out_dist[qq * K + rank] = dp;
    }
}

// *bad = 1 when a row norm is not finite or so large that a squared distance could overflow (NaN / Inf / huge input)
__global__ __launch_bounds__(256) void norm_check_kernel(const double *__restrict__ nrm, long long n, int *__restrict__ bad) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && !(nrm[i] <= 0.125 * DBL_MAX)) *bad = 1;   // (false for NaN too)
}

// ---- the cross search: query rows against a reference -------------------------------------------------------------------------------
// out = X - mu, row-major n x d
__global__ __launch_bounds__(256) void center_rows_kernel(const double *__restrict__ X, long long n, int d, const double *__restrict__ mu,
                                                          double *__restrict__ out) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < n * d) out[e] = X[e] - mu[e % d];
}

// rownorm_kernel and norm_check_kernel in one.  *bad = 1 when a norm is not finite or so large that a squared distance could
// overflow (NaN / Inf / huge input)
__global__ __launch_bounds__(256) void rownorm_check_kernel(const double *__restrict__ X, long long n, int d, double *__restrict__ nrm,
                                                            int *__restrict__ bad) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int c = 0; c < d; ++c) { const double t = X[i * d + c]; a += t * t; }
    nrm[i] = a;
    if (!(a <= 0.125 * DBL_MAX)) *bad = 1;   // (false for NaN too; every writer stores the same value)
}

// Workgroup (blockIdx.x, blockIdx.y): the KQ query rows [q0, q0 + 16) of Q (nq x d, centred with the model's mean) against the reference
// rows of chunk blockIdx.y, tile by tile of KCT.  The A operand of the f64 MFMA (row lane & 15, column 4 s + (lane >> 4) in k-step s)
// is the same for every tile: a lane keeps its ceil(d / 4) values in registers, or, beyond KREG k-steps, the workgroup keeps them in an
// LDS panel laid out [k-step][lane], which every wave reads at consecutive addresses.  The k-steps run in order in both forms, so a
// pair's value depends on d and the two rows alone.  Wave w computes columns c0 + 16 w .. + 16 (C/D: row (lane >> 4) + 4 r, column
// lane & 15) into the LDS tile and then offers the tile to rows 4 w .. 4 w + 3.  The chunk's top-K of every row (GEMM values, unsorted;
// sentinels (KNN_INF, INT_MAX) where the chunk holds fewer than K candidates) goes to part[(chunk * rows + r) * K ..].
template <bool PANEL>
__global__ __launch_bounds__(256) void knn_cross_kernel(const double *__restrict__ Q, const double *__restrict__ qn, const double *__restrict__ W,
                                                        const double *__restrict__ wn, long long nref, int d, int K, long long row0,
                                                        long long row_end, long long cj, int *__restrict__ part_idx,
                                                        double *__restrict__ part_dist) {
    extern __shared__ double smem[];
    double *dt = smem;                                // [KQ][KDT]
    double *Ld = dt + KQ * KDT;                       // [KQ][K]
    int *Li = reinterpret_cast<int *>(Ld + KQ * K);   // [KQ][K]
    double *panel = reinterpret_cast<double *>(Li + KQ * K);   // [ksteps][64] (PANEL only; 16 K ints keep it 8-byte aligned)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long q0 = row0 + static_cast<long long>(blockIdx.x) * KQ, rows = row_end - row0;
    const long long cbeg = static_cast<long long>(blockIdx.y) * cj, cend = cbeg + cj < nref ? cbeg + cj : nref;
    const int ksteps = (d + 3) >> 2, kk = lane >> 4;
    for (int e = tid; e < KQ * K; e += 256) { Ld[e] = KNN_INF; Li[e] = INT_MAX; }
    double thr[4];
    int widx[4], wpos[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { thr[r] = KNN_INF; widx[r] = INT_MAX; wpos[r] = 0; }
    double a[KREG];
    if (PANEL) {
        for (int e = tid; e < ksteps * 64; e += 256) {
            const long long qr = q0 + (e & 15);
            const int k = 4 * (e >> 6) + ((e & 63) >> 4);
            panel[e] = (qr < row_end && k < d) ? Q[qr * d + k] : 0.0;
        }
    } else {
        const long long qa = q0 + (lane & 15);
#pragma unroll
        for (int s = 0; s < KREG; ++s) {
            const int k = 4 * s + kk;
            a[s] = (qa < row_end && k < d) ? Q[qa * d + k] : 0.0;
        }
    }
    double nq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long qq = q0 + kk + 4 * r;
        nq[r] = qq < row_end ? qn[qq] : 0.0;
    }
    __syncthreads();
    for (long long c0 = cbeg; c0 < cend; c0 += KCT) {
        const long long cb = c0 + wave * 16 + (lane & 15);
        const bool cb_ok = cb < cend;
        const double *wrow = W + (cb_ok ? cb : cbeg) * d;
        v4f64 acc = {0.0, 0.0, 0.0, 0.0};
        if (PANEL) {
            for (int s = 0; s < ksteps; ++s) {
                const int k = 4 * s + kk;
                const double b = (cb_ok && k < d) ? wrow[k] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(panel[s * 64 + lane], b, acc, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < KREG; ++s) {
                if (s < ksteps) {   // (wave-uniform)
                    const int k = 4 * s + kk;
                    const double b = (cb_ok && k < d) ? wrow[k] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b, acc, 0, 0, 0);
                }
            }
        }
        const double nc = cb_ok ? wn[cb] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) dt[(kk + 4 * r) * KDT + wave * 16 + (lane & 15)] = nq[r] + nc - 2.0 * acc[r];
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = wave * 4 + rr;
            if (q0 + row >= row_end) continue;
            const long long ci = c0 + lane;
            knn_offer(dt[row * KDT + lane], static_cast<int>(ci), ci < cend, Ld + row * K, Li + row * K, K, lane, thr[rr], widx[rr], wpos[rr]);
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

// knn_merge_kernel between two matrices.  One wave per query row of the launch: the K best of the chunks' lists (nc x K
// candidates, chunk after chunk), re-ranked by the direct sum (q_c - x_jc)^2 in column order on the caller's values, sorted by
// (distance, index) and written as Euclidean distances.  A row left with a sentinel sets *bad and reads nothing through it.
__global__ __launch_bounds__(256) void knn_cross_merge_kernel(const double *__restrict__ Xq, const double *__restrict__ Xr, long long nq,
                                                              long long nref, int d, int K, long long row0, long long rows, int nc,
                                                              const int *__restrict__ part_idx, const double *__restrict__ part_dist,
                                                              int *__restrict__ out_idx, double *__restrict__ out_dist, int *__restrict__ bad) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *Ld = smem + wave * K;                                  // [4][K] doubles, then [4][K] ints
    int *Li = reinterpret_cast<int *>(smem + 4 * K) + wave * K;
    const long long r = static_cast<long long>(blockIdx.x) * 4 + wave, qq = row0 + r;
    if (r >= rows || qq >= nq) return;
    for (int p = lane; p < K; p += 64) { Ld[p] = KNN_INF; Li[p] = INT_MAX; }
    wave_sync();
    double thr = KNN_INF;
    int widx = INT_MAX, wpos = 0;
    for (int c = 0; c < nc; ++c) {
        const long long base = (static_cast<long long>(c) * rows + r) * K;
        for (int t = 0; t < K; t += 64) {
            const bool in = t + lane < K;
            const int ci = in ? part_idx[base + t + lane] : INT_MAX;
            const double v = in ? part_dist[base + t + lane] : KNN_INF;
            knn_offer(v, ci, in && ci >= 0 && ci < nref, Ld, Li, K, lane, thr, widx, wpos);
        }
    }
    wave_sync();
    for (int p = lane; p < K; p += 64) {
        const int j = Li[p];
        double s = KNN_INF;
        if (j >= 0 && j < nref) {
            s = 0.0;
            for (int c = 0; c < d; ++c) { const double t = Xq[qq * d + c] - Xr[static_cast<long long>(j) * d + c]; s += t * t; }
        } else {
            *bad = 1;   // every writer stores the same value
        }
        Ld[p] = s;
    }
    wave_sync();
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p], rank = knn_rank(Ld, Li, K, dp, ip);
        out_idx[qq * K + rank] = ip < nref ? ip : -1;
        out_dist[qq * K + rank] = sqrt(dp);
    }
}

// ---- neighbours that are given, or selected from given distances (DESIGN.md §10 "Given neighbours, given distances") -----------------
constexpr int NN_RS = 8;     // 64-wide loads in flight per lane before their offers (hclust_agglo.hip's HC_RS idea)

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
    wave_sync();
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
    wave_sync();
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p], rank = knn_rank(Ld, Li, K, dp, ip);
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
    wave_sync();
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

}  // namespace

double knn_pair_budget(int d) { return 8e9 / (std::max(d, 4) / 50.0 + 0.25); }

KnnPlan knn_plan(long long nq, long long nref, int d, int max_rows) {
    KnnPlan p;
    p.rows = std::min((nq + KQ - 1) / KQ * KQ, std::max<long long>(KQ, static_cast<long long>(knn_pair_budget(d) / static_cast<double>(nref)) / KQ * KQ));
    if (max_rows > 0) p.rows = std::min(p.rows, std::max<long long>(KQ, max_rows / KQ * KQ));
    const long long rb = (p.rows + KQ - 1) / KQ;
    const long long nc0 = std::max<long long>(1, std::min<long long>((nref + KCT - 1) / KCT, (1024 + rb - 1) / rb));
    p.cols = ((nref + nc0 - 1) / nc0 + KCT - 1) / KCT * KCT;
    p.chunks = static_cast<int>((nref + p.cols - 1) / p.cols);
    return p;
}

void knn_self(const char *who, const double *dX, long long n, int d, int K, DevBuf<int> &idx, DevBuf<double> &dist) {
    Ctx &c = ctx();
    const std::string w(who);
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, w + ": need 1 <= K <= 255 and K < n");
    KernelTimer t("tsne_knn");
    // The candidates are selected on w = x - column mean (fp64): distances do not change under a translation, but the error of
    // ||x_i||^2 + ||x_j||^2 - 2 x_i.x_j scales with ||x||^2, and input far from the origin (Rtsne(pca = FALSE, normalize = FALSE),
    // sharp_tsne_knn) would otherwise lose true neighbours to it.  The merge re-ranks the chosen K on the caller's values.
    DevBuf<double> Xc(static_cast<size_t>(n) * d), mu(d), mupart;
    column_stat(dX, n, d, d, nullptr, static_cast<double>(n), mupart, mu.p);
    affine_rows(dX, n, d, d, mu.p, nullptr, 1.0, Xc.p);
    DevBuf<double> nrm(n);
    DevBuf<int> bad(1);
    bad.zero();
    hipLaunchKernelGGL(rownorm_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, Xc.p, n, d, nrm.p);
    hipLaunchKernelGGL(norm_check_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, nrm.p, n, bad.p);
    launch_check("norm_check_kernel");
    int hb = 0;
    bad.download(&hb, 1);
    SHARP_REQUIRE(hb == 0, w + ": the (prepared) input holds NA / NaN / Inf, or values so large that squared distances overflow");
    idx.alloc(static_cast<size_t>(n) * K);
    dist.alloc(static_cast<size_t>(n) * K);
    const auto [rows, cj, nc] = knn_plan(n, n, d, 0);
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
    SHARP_REQUIRE(hb == 0, w + ": fewer than K rows at a finite distance from some row (non-finite input?)");
}

void knn_from_dist(const char *who, const double *d, int n, int K, DevBuf<int> &idx, DevBuf<double> &dist2) {
    Ctx &c = ctx();
    const std::string w(who);
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, w + ": need 1 <= K <= 255 and K < n");
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
    SHARP_REQUIRE(hb == 0, w + ": the distances are so large that their squares overflow");
}

void throw_list_fault(const std::string &who, unsigned long long word) {
    const std::string row = " (row " + std::to_string(word >> 3) + ", counted from 0)";
    switch (static_cast<int>(word & 7)) {
        case NN_RANGE: throw Error(SHARP_ERR_ARG, who + ": a neighbour index outside [0, n)" + row);
        case NN_SELF: throw Error(SHARP_ERR_ARG, who + ": a row names itself as a neighbour" + row);
        case NN_TWICE: throw Error(SHARP_ERR_ARG, who + ": the same neighbour index twice in a row" + row);
        default: throw Error(SHARP_ERR_ARG, who + ": a distance that is NA / NaN / Inf or negative" + row);
    }
}

void upload_neighbours(const char *who, const int *index, const double *distance, long long n, int K, bool squared, DevBuf<int> &idx,
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
    if (w != NN_OK) throw_list_fault(who, w);
    if (!squared) {
        DevBuf<int> bad(1);
        bad.zero();
        hipLaunchKernelGGL(square_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, c.stream, dist2.p, n * K, bad.p);
        launch_check("square_kernel");
        int hb = 0;
        bad.download(&hb, 1);
        SHARP_REQUIRE(hb == 0, std::string(who) + ": the distances are so large that their squares overflow");
    }
}

void center_and_norm(const double *dX, long long n, int d, const double *mu, DevBuf<double> &out, DevBuf<double> &nrm, const std::string &msg) {
    Ctx &c = ctx();
    out.alloc(static_cast<size_t>(n) * d);
    nrm.alloc(n);
    DevBuf<int> bad(1);
    bad.zero();
    hipLaunchKernelGGL(center_rows_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, c.stream, dX, n, d, mu, out.p);
    hipLaunchKernelGGL(rownorm_check_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, out.p, n, d, nrm.p, bad.p);
    launch_check("rownorm_check_kernel");
    int hb = 0;
    bad.download(&hb, 1);
    SHARP_REQUIRE(hb == 0, msg);
}

void knn_cross(const char *who, const double *W, const double *wn, const double *X, const double *mu, long long n, int d, const double *dXq,
               long long nq, int K, int max_rows, DevBuf<int> &idx, DevBuf<double> &dist) {
    Ctx &c = ctx();
    const std::string w(who);
    SHARP_REQUIRE(K >= 1 && K <= 255, w + ": K must be in 1 .. 255");
    SHARP_REQUIRE(K <= n, w + ": K must not exceed the model's number of reference rows");
    SHARP_REQUIRE(nq >= 1 && nq < INT_MAX, w + ": nq must be in 1 .. 2^31 - 1");
    SHARP_REQUIRE(max_rows >= 0, w + ": max_rows_per_launch must be >= 0 (0: the library's choice)");
    const int ksteps = (d + 3) / 4;
    const bool panel = ksteps > KREG;
    const size_t lds = sizeof(double) * KQ * KDT + (sizeof(double) + sizeof(int)) * KQ * K + (panel ? sizeof(double) * 64 * ksteps : 0);
    SHARP_REQUIRE(lds <= LDS_MAX, w + ": d is too large for the query panel at this K (reduce the data first)");
    KernelTimer t("umap_knn_cross");
    DevBuf<double> Qc, qn;
    center_and_norm(dXq, nq, d, mu, Qc, qn, w + ": Xq holds NA / NaN / Inf, or values so large that squared distances overflow");
    idx.alloc(static_cast<size_t>(nq) * K);
    dist.alloc(static_cast<size_t>(nq) * K);
    const auto [rows, cj, nc] = knn_plan(nq, n, d, max_rows);
    DevBuf<int> pidx(static_cast<size_t>(nc) * rows * K), bad(1);
    DevBuf<double> pdist(static_cast<size_t>(nc) * rows * K);
    bad.zero();
    const size_t lds_merge = (sizeof(double) + sizeof(int)) * 4 * K;
    auto kern = panel ? knn_cross_kernel<true> : knn_cross_kernel<false>;
    if (lds > 65536) SHARP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    for (long long r0 = 0; r0 < nq; r0 += rows) {
        const long long r1 = std::min(nq, r0 + rows);
        hipLaunchKernelGGL(kern, dim3(grid_for(r1 - r0, KQ), nc), dim3(256), lds, c.stream, Qc.p, qn.p, W, wn, n, d, K, r0, r1, cj, pidx.p,
                           pdist.p);
        launch_check("knn_cross_kernel");
        hipLaunchKernelGGL(knn_cross_merge_kernel, dim3(grid_for(r1 - r0, 4)), dim3(256), lds_merge, c.stream, dXq, X, nq, n, d, K, r0, r1 - r0,
                           nc, pidx.p, pdist.p, idx.p, dist.p, bad.p);
        launch_check("knn_cross_merge_kernel");
    }
    int hb = 0;
    bad.download(&hb, 1);   // (synchronises: the temporaries go out of scope)
    SHARP_REQUIRE(hb == 0, w + ": fewer than K reference rows at a finite distance from some row");
}

}  // namespace sharp
