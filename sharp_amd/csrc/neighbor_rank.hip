// neighbor_rank.hip -- where the rows a list names stand among ALL rows: the counting step behind trustworthiness and continuity of a
// map.  For row i and each of its K given rows j:  rank(i, k) = 1 + #{ l != i : (d2(i, l), l) < (d2(i, j), j) },
// d2 the direct sum of (x_ic - x_lc)^2 in column order (DistEuclid::acc of dist_pairs.hpp without the root, knn_merge_kernel's re-rank:
// bitwise the squared distance sharp_tsne_knn returns), ties to the lower index.  Matrix-free: no n x n array.
//   nr_threshold_kernel   one wave per row: validates the row's K indices before one is dereferenced (range, self, twice: the word of
//                         nn_check_kernel in knn.hip), computes its K thresholds (d2(i, j), j), sorts them ascending and keeps the
//                         permutation back to the caller's order
//   nr_tile_kernel        sil_tile_kernel's pair loop (64 rows per workgroup, k-major panels of DK features through LDS, a 4 x 4 block of
//                         pairs per lane, the features in order) with a counting epilogue: a finished pair is compared with its row's
//                         LARGEST threshold first -- on a good map almost every pair leaves there --, a survivor that is not the diagonal
//                         pair binary-searches the row's sorted thresholds and adds 1, with an integer LDS atomic, to the bucket of the
//                         first threshold it is below.  After the last column tile a running sum over the buckets gives, per threshold,
//                         the number of rows below it.  The thresholds live in LDS, so a launch works on a SLICE of W of the K thresholds
//                         (W = 16 / 32 / 64: three / two / one workgroup per CU); K > 64 runs the pair loop once per slice (blockIdx.z).
//                         For small n the column tiles are dealt to parts (blockIdx.y), each writing its own partial counts.
//   nr_finish_kernel      adds the parts' counts, adds 1 and writes the rank at the caller's position
// Everything counted is an integer and integer adds commute: the result depends on neither the order of the atomics, the number of parts,
// the slices nor the rows per launch, and two calls give the same bits.  No floating-point atomic anywhere.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "dist_pairs.hpp"
#include "knn.hpp"
#include "knn_dev.hpp"

namespace sharp {

namespace {

constexpr long long kNrMaxN = 1ll << 24;     // rows: a count fits an int with room, row indices are ints
constexpr int kNrMaxK = 255;
constexpr int kNrMaxParts = 32;              // workgroups per row tile and slice when the row tiles alone leave CUs idle
constexpr double kNrXMax = 1.0e100;          // |x| above this is refused: a squared distance stays finite below it (knn_descent.hip's KD_XMAX)

// One wave per row i.  index: n x K as the caller gave it.  td / tj [i * K + s]: the row's thresholds in ascending (d2, j) order,
// pos[i * K + s]: the caller's column of the threshold at sorted place s.  An invalid row writes nothing and lowers *word to
// (row << 3 | kind): the first offending row and its lowest kind, whatever the scheduling.
__global__ __launch_bounds__(256) void nr_threshold_kernel(const double *__restrict__ X, long long n, int d, int K, const int *__restrict__ index,
                                                           double *__restrict__ td, int *__restrict__ tj, int *__restrict__ pos,
                                                           unsigned long long *__restrict__ word) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *Ld = smem + wave * K;                                  // [4][K] doubles, then [4][K] ints
    int *Li = reinterpret_cast<int *>(smem + 4 * K) + wave * K;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + wave;
    if (i >= n) return;                                            // (whole waves leave; no workgroup barrier below)
    int kind = 8;
    for (int p = lane; p < K; p += 64) {
        const int j = index[i * K + p];
        Li[p] = j;
        if (j < 0 || j >= n) kind = min(kind, static_cast<int>(NN_RANGE));
        else if (j == i) kind = min(kind, static_cast<int>(NN_SELF));
    }
    wave_sync();
    for (int p = lane; p < K; p += 64) {
        const int j = Li[p];
        for (int q = 0; q < p; ++q)
            if (Li[q] == j) { kind = min(kind, static_cast<int>(NN_TWICE)); break; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kind = min(kind, __shfl_xor(kind, off));
    if (kind < 8) {                                                // (the same in every lane of the wave)
        if (lane == 0) atomicMin(word, (static_cast<unsigned long long>(i) << 3) | static_cast<unsigned long long>(kind));
        return;
    }
    for (int p = lane; p < K; p += 64) {
        const long long j = Li[p];
        double s = 0.0;
        for (int c = 0; c < d; ++c) { const double t = X[i * d + c] - X[j * d + c]; s += t * t; }
        Ld[p] = s;
    }
    wave_sync();
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p], place = knn_rank(Ld, Li, K, dp, ip);
        td[i * K + place] = dp;
        tj[i * K + place] = ip;
        pos[i * K + place] = p;
    }
}

// The rows r0 .. r1 - 1 of the launch, 64 per blockIdx.x; the column tiles ct[blockIdx.y] .. ct[blockIdx.y + 1] - 1; the thresholds
// blockIdx.z * W .. of each row.  part[((blockIdx.y * (r1 - r0)) + row - r0) * K + s] = #{ columns l of the part, l != row :
// (d2(row, l), l) < threshold s of the row }.  Dynamic LDS: the slice, 64 rows of W + 1 slots (the odd stride spreads the four rows a
// wave searches at once over the banks), as doubles, then indices, then buckets.
template <int W>
__global__ __launch_bounds__(256) void nr_tile_kernel(const double *__restrict__ x, int n, int p, int K, int r0, int r1,
                                                      const int *__restrict__ ct, const double *__restrict__ td,
                                                      const int *__restrict__ tj, int *__restrict__ part) {
    constexpr int WS = W + 1;
    __shared__ __attribute__((aligned(16))) double sA[DK][DLD];
    __shared__ __attribute__((aligned(16))) double sB[DK][DLD];
    extern __shared__ __attribute__((aligned(16))) double nr_slice[];
    double *sTd = nr_slice;                                        // [DT][WS]
    int *sTj = reinterpret_cast<int *>(nr_slice + DT * WS);        // [DT][WS]
    int *sBk = sTj + DT * WS;                                      // [DT][WS]
    const int i0 = r0 + blockIdx.x * DT;
    const int k_first = blockIdx.z * W, kw = min(W, K - k_first);
    const int jbeg = ct[blockIdx.y] * DT, jend = min(n, ct[blockIdx.y + 1] * DT);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int skk = tid & 31, sr = tid >> 5;
    for (int e = tid; e < DT * kw; e += 256) {
        const int r = e / kw, s = e - r * kw;
        const long long g = static_cast<long long>(i0 + r) * K + k_first + s;
        const bool in = i0 + r < r1;
        sTd[r * WS + s] = in ? td[g] : -1.0;
        sTj[r * WS + s] = in ? tj[g] : 0;
        sBk[r * WS + s] = 0;
    }
    __syncthreads();
    // the row's largest threshold of the slice; a row beyond the launch has -1, which no squared distance is below
    int row[4], tmax_j[4];
    double tmax_d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = ty * 4 + u;
        row[u] = i0 + r;
        tmax_d[u] = sTd[r * WS + kw - 1];
        tmax_j[u] = sTj[r * WS + kw - 1];
    }
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
            const int kend = min(DK, p - k0);        // (a feature beyond p would add (0 - 0)^2: leaving it out changes no bit)
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
                    for (int v = 0; v < 4; ++v) DistEuclid::acc(acc[u][v], a[u] - b[v], 0.0);
            }
            __syncthreads();
        }
        const int col[4] = {j0 + tx * 2, j0 + tx * 2 + 1, j0 + 32 + tx * 2, j0 + 33 + tx * 2};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = ty * 4 + u;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const double val = acc[u][v];
                const int c = col[v];
                if (!lex_less(val, c, tmax_d[u], tmax_j[u])) continue;      // not below the largest: below none
                if (c == row[u] || c >= n) continue;                          // the diagonal pair; a column of the padding
                int lo = 0, hi = kw - 1;                                      // the first threshold the pair is below (kw - 1 is one)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (lex_less(val, c, sTd[r * WS + mid], sTj[r * WS + mid])) hi = mid; else lo = mid + 1;
                }
                atomicAdd(&sBk[r * WS + lo], 1);
            }
        }
    }
    __syncthreads();
    // bucket s holds the columns below threshold s and not below s - 1: the count of threshold s is the running sum
    if (tid < DT) {
        int run = 0;
        for (int s = 0; s < kw; ++s) { run += sBk[tid * WS + s]; sBk[tid * WS + s] = run; }
    }
    __syncthreads();
    const long long rows = r1 - r0;
    for (int e = tid; e < DT * kw; e += 256) {
        const int r = e / kw, s = e - r * kw;
        if (i0 + r < r1) part[(static_cast<long long>(blockIdx.y) * rows + (i0 + r - r0)) * K + k_first + s] = sBk[r * WS + s];
    }
}

// rank_out[i * K + pos[i * K + s]] = 1 + the sum over the parts of the count of row i's threshold s, for the rows of the launch
__global__ __launch_bounds__(256) void nr_finish_kernel(int r0, int r1, int K, int parts, const int *__restrict__ part,
                                                        const int *__restrict__ pos, int *__restrict__ rank_out) {
    const long long rows = r1 - r0, e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= rows * K) return;
    int cnt = 1;
    for (int s = 0; s < parts; ++s) cnt += part[static_cast<long long>(s) * rows * K + e];
    const long long g = static_cast<long long>(r0) * K + e;         // (row r0 + e / K, sorted place e % K)
    rank_out[g - e % K + pos[g]] = cnt;
}

template <int W>
void launch_nr_tile(dim3 grid, const double *x, int n, int p, int K, int r0, int r1, const int *ct, const double *td, const int *tj, int *part) {
    constexpr size_t static_lds = 2 * sizeof(double) * DK * DLD;
    const size_t lds = static_cast<size_t>(DT) * (W + 1) * (sizeof(double) + 2 * sizeof(int));
    const void *kern = reinterpret_cast<const void *>(nr_tile_kernel<W>);
    if (static_lds + lds > 65536) SHARP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    hipLaunchKernelGGL(nr_tile_kernel<W>, grid, dim3(256), lds, ctx().stream, x, n, p, K, r0, r1, ct, td, tj, part);
}

// the slice width for K thresholds: the narrowest that takes them in one pass, 64 and several passes above that
inline int nr_slice_width(int K) { return K <= 16 ? 16 : K <= 32 ? 32 : 64; }

}  // namespace

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_neighbor_ranks(const double *X, long long n, int d, long long ld, int K, const int *index, int max_rows_per_launch, int *rank_out) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    const std::string w("sharp_neighbor_ranks");
    SHARP_REQUIRE(X && index && rank_out, w + ": null argument");
    SHARP_REQUIRE(n >= 3 && d >= 1 && ld >= d, w + ": need n >= 3 rows of d >= 1 values (ld >= d)");
    SHARP_REQUIRE(n <= kNrMaxN, w + ": more than 16777216 rows is not supported");
    SHARP_REQUIRE(K >= 1 && K <= kNrMaxK, w + ": K must be in 1 .. 255");
    SHARP_REQUIRE(K <= n - 1, w + ": K neighbours per row need K <= n - 1");
    SHARP_REQUIRE(max_rows_per_launch >= 0, w + ": max_rows_per_launch must be >= 0");
    for (long long i = 0; i < n; ++i)
        for (int q = 0; q < d; ++q)
            if (!(std::fabs(X[i * ld + q]) <= kNrXMax))   // (false for NaN too)
                throw Error(SHARP_ERR_ARG, w + ": the input holds NA / NaN / Inf or a value beyond 1e100 (row " + std::to_string(i + 1) +
                                               ", column " + std::to_string(q + 1) + ")");
    const int ni = static_cast<int>(n);
    const size_t ne = static_cast<size_t>(n) * K;
    DevBuf<double> dx, dtd(ne);
    DevBuf<int> didx(ne), dtj(ne), dpos(ne), drank(ne);
    upload_rows(X, n, d, ld, dx);
    didx.upload(index, ne);
    DevBuf<unsigned long long> word(1);
    SHARP_HIP_CHECK(hipMemsetAsync(word.p, 0xFF, sizeof(unsigned long long), c.stream));
    {
        KernelTimer tm("nr_threshold_kernel");
        hipLaunchKernelGGL(nr_threshold_kernel, dim3(grid_for(n, 4)), dim3(256), (sizeof(double) + sizeof(int)) * 4 * K, c.stream, dx.p, n, d, K,
                           didx.p, dtd.p, dtj.p, dpos.p, word.p);
        launch_check("nr_threshold_kernel");
    }
    unsigned long long hw = NN_OK;
    word.download(&hw, 1);
    if (hw != NN_OK) throw_list_fault(w, hw);
    const int W = nr_slice_width(K), slices = (K + W - 1) / W;
    // rows per launch from the exact k-NN's pair budget, every slice being a pass of its own
    const double budget = knn_pair_budget(d);
    long long rows = std::min<long long>(n, std::max<long long>(DT, static_cast<long long>(budget / static_cast<double>(n) / slices) / DT * DT));
    if (max_rows_per_launch > 0) rows = std::min<long long>(rows, max_rows_per_launch);
    // the column tiles dealt to parts when the row tiles of a launch alone leave CUs idle
    const int col_tiles = (ni + DT - 1) / DT;
    const long long wgs = (rows + DT - 1) / DT * slices;
    const int parts = static_cast<int>(std::max<long long>(1, std::min<long long>(std::min(kNrMaxParts, col_tiles), (4ll * c.num_cu + wgs - 1) / wgs)));
    std::vector<int> ct(parts + 1);
    for (int s = 0; s <= parts; ++s) ct[s] = static_cast<int>(static_cast<long long>(col_tiles) * s / parts);
    DevBuf<int> dct(ct.size()), dpart(static_cast<size_t>(parts) * rows * K);
    dct.upload(ct.data(), ct.size());
    for (long long r0 = 0; r0 < n; r0 += rows) {
        const long long r1 = std::min(n, r0 + rows);
        {
            KernelTimer tm("nr_tile_kernel");
            const dim3 grid(grid_for(r1 - r0, DT), parts, slices);
            const int a = static_cast<int>(r0), b = static_cast<int>(r1);
            switch (W) {
                case 16: launch_nr_tile<16>(grid, dx.p, ni, d, K, a, b, dct.p, dtd.p, dtj.p, dpart.p); break;
                case 32: launch_nr_tile<32>(grid, dx.p, ni, d, K, a, b, dct.p, dtd.p, dtj.p, dpart.p); break;
                default: launch_nr_tile<64>(grid, dx.p, ni, d, K, a, b, dct.p, dtd.p, dtj.p, dpart.p); break;
            }
            launch_check("nr_tile_kernel");
        }
        KernelTimer tm("nr_finish_kernel");
        hipLaunchKernelGGL(nr_finish_kernel, dim3(grid_for((r1 - r0) * K, 256)), dim3(256), 0, c.stream, static_cast<int>(r0), static_cast<int>(r1),
                           K, parts, dpart.p, dpos.p, drank.p);
        launch_check("nr_finish_kernel");
    }
    drank.download(rank_out, ne);
    SHARP_API_END
}

}  // extern "C"
