// expr_pca.hip -- a truncated PCA of sparse expression blocks by randomised subspace iteration: DESIGN.md §21 (the specification is the
// project's own, modelled on Halko, Martinsson and Tropp and on what scanpy / Seurat compute; no parity with them is claimed).
//   upload     the blocks' stored entries side by side (cell-major: cptr, ridx, t), validated by expr_validate_kernel before anything
//              dereferences an index (range, strictly ascending within a cell, finite, >= 0 under a transform), the cells' sums
//              L_c, then t = log1p(x T / L_c) in place
//   subset     with a gene list: after the transform the entries of the other genes are dropped and the kept genes
//              renumbered (a count per cell, one wave each; the scan; a fill that keeps the stored order); everything below then works
//              on the kept genes
//   transpose  the gene-major copy (gptr, gcell, gval) by one stable radix sort of (gene << 32 | cell) keys on the gene bits: a gene's
//              entries stand in ascending cell order; a gene's entries are cut into chunks of kExprChunk
//   stats      mu and var per gene in two passes over the gene-major copy: one wave per chunk (64 strided sums, then the butterfly), a
//              gene's chunks folded in chunk order by one thread
//   products   A = (T^T - 1 mu^T) diag(w) is never formed.  Cell side: one wave per cell, lanes over the l columns (two per lane above
//              64), the cell's (gene, value) pairs loaded 64 at a time and broadcast, each a coalesced read of a row of diag(w) B,
//              summed in stored order; the shift mu^T diag(w) B from graph.hpp's fixed_reduce.  Gene side: the same loop per chunk over
//              rows of Q, in cell order, then a gene's partial sums added in chunk order; colsum(Q) from fixed_reduce.
//   orth       CholeskyQR2: the l x l Gram from gemm_tn_f64_batched over slabs of kExprSlabRows rows folded in slab order, the factor
//              on the host, the triangular solve one wave per row; twice
// No floating-point atomic anywhere: every sum's order is fixed by the input's shape, so two calls give the same bits.
#include "expr_pca.hpp"
#include "graph_prim.hpp"
#include "linalg.hpp"
#include "prepare.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace sharp {
namespace {

enum : int { EX_RANGE = 0, EX_ORDER = 1, EX_FINITE = 2, EX_NEGATIVE = 3 };
constexpr u64 EX_OK = ~0ull;
constexpr int kGramBatch = 1024;                 // slabs per launch of the Gram (their partial matrices are folded batch after batch)

__device__ __forceinline__ double lane_get(double x, int q) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), q), __builtin_amdgcn_readlane(__double2loint(x), q));
}

// One wave per cell: every stored entry's gene in [0, m) and above the one before it, every value finite and, under a transform, not
// negative.  *word = min over the offending cells of (cell << 3 | kind).
__global__ __launch_bounds__(256) void expr_validate_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx,
                                                            const double *__restrict__ val, long long n, int m, int check_neg,
                                                            u64 *__restrict__ word) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    const long long b = cptr[c], e = cptr[c + 1];
    int kind = 8;
    for (long long p = b + lane; p < e; p += 64) {
        const int r = ridx[p];
        const double v = val[p];
        int k = 8;
        if (r < 0 || r >= m) k = EX_RANGE;
        else if (p > b && ridx[p - 1] >= r) k = EX_ORDER;
        else if (!isfinite(v)) k = EX_FINITE;
        else if (check_neg && v < 0.0) k = EX_NEGATIVE;
        kind = k < kind ? k : kind;
    }
    if (kind < 8) atomicMin(word, (static_cast<u64>(c) << 3) | static_cast<u64>(kind));
}

// out[c] = the sum of the cell's stored values: 64 strided running sums, then the butterfly
__global__ __launch_bounds__(256) void expr_cell_sums_kernel(const long long *__restrict__ cptr, const double *__restrict__ val, long long n,
                                                             double *__restrict__ out) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    const long long e = cptr[c + 1];
    double a = 0.0;
    for (long long p = cptr[c] + lane; p < e; p += 64) a += val[p];
    a = wave_sum(a);
    if (lane == 0) out[c] = a;
}

// t = x (T / L_c) when T > 0 (a cell whose sum is 0 stays 0), then log1p when asked; in place
__global__ __launch_bounds__(256) void expr_transform_kernel(const long long *__restrict__ cptr, const double *__restrict__ lsum, long long n,
                                                             double total, int lg, double *__restrict__ val) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    const long long e = cptr[c + 1];
    const double L = lsum[c];
    const double f = L > 0.0 ? total / L : 0.0;
    for (long long p = cptr[c] + lane; p < e; p += 64) {
        double v = val[p];
        if (total > 0.0) v = v * f;
        if (lg) v = log1p(v);
        val[p] = v;
    }
}

// cnt[c] = the cell's entries whose gene is kept (remap[gene] >= 0): one wave per cell
__global__ __launch_bounds__(256) void expr_subset_count_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx, long long n,
                                                                const int *__restrict__ remap, long long *__restrict__ cnt) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    const long long e = cptr[c + 1];
    int k = 0;
    for (long long p = cptr[c] + lane; p < e; p += 64) k += remap[ridx[p]] >= 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k += __shfl_xor(k, off);
    if (lane == 0) cnt[c] = k;
}

// the kept entries of cell c, in stored order and renumbered, into [nptr[c], nptr[c + 1]): 64 entries at a time, each kept one placed
// behind the kept ones of the lower lanes
__global__ __launch_bounds__(256) void expr_subset_fill_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx,
                                                               const double *__restrict__ val, long long n, const int *__restrict__ remap,
                                                               const long long *__restrict__ nptr, int *__restrict__ ridx2,
                                                               double *__restrict__ val2) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    const long long e = cptr[c + 1];
    long long o = nptr[c];
    for (long long p0 = cptr[c]; p0 < e; p0 += 64) {
        const long long p = p0 + lane;
        int r = -1;
        double v = 0.0;
        if (p < e) { r = remap[ridx[p]]; v = val[p]; }
        const u64 keep = __ballot(r >= 0);
        if (r >= 0) {
            const long long at = o + __popcll(keep & ((1ull << lane) - 1ull));
            ridx2[at] = r;
            val2[at] = v;
        }
        o += __popcll(keep);
    }
}

// keys[p] = (gene << 32 | cell) of every stored entry
__global__ __launch_bounds__(256) void expr_keys_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx, long long n,
                                                        u64 *__restrict__ keys) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    const long long e = cptr[c + 1];
    for (long long p = cptr[c] + lane; p < e; p += 64) keys[p] = (static_cast<u64>(static_cast<unsigned>(ridx[p])) << 32) | static_cast<u64>(c);
}

__global__ __launch_bounds__(256) void expr_unkey_kernel(const u64 *__restrict__ keys, long long nnz, int *__restrict__ gcell) {
    const long long p = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (p < nnz) gcell[p] = static_cast<int>(keys[p] & 0xFFFFFFFFull);
}

// gptr[g] = the first sorted entry whose gene is >= g, g = 0 .. m; nchunk[g] = the gene's chunks (nchunk[m] = 0: the scan's extra slot)
__global__ __launch_bounds__(256) void expr_gptr_kernel(const u64 *__restrict__ keys, long long nnz, int m, long long *__restrict__ gptr) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g > m) return;
    const u64 want = static_cast<u64>(g) << 32;
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    gptr[g] = lo;
}

__global__ __launch_bounds__(256) void expr_nchunk_kernel(const long long *__restrict__ gptr, int m, long long *__restrict__ nchunk) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g > m) return;
    nchunk[g] = g < m ? (gptr[g + 1] - gptr[g] + kExprChunk - 1) / kExprChunk : 0;
}

__global__ __launch_bounds__(256) void expr_chgene_kernel(const long long *__restrict__ chptr, int m, int *__restrict__ chgene) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= m) return;
    const long long e = chptr[g + 1];
    for (long long ch = chptr[g]; ch < e; ++ch) chgene[ch] = g;
}

// One wave per chunk.  PASS 0: the chunk's sum, its non-zero values, its smallest and its largest value.  PASS 1: its sum of (t - mu_g)^2.
template <int PASS>
__global__ __launch_bounds__(256) void expr_gene_stats_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr,
                                                              const int *__restrict__ chgene, long long nch, const double *__restrict__ gval,
                                                              const double *__restrict__ mu, double *__restrict__ psum,
                                                              int *__restrict__ pcnt, double *__restrict__ pmin, double *__restrict__ pmax) {
    const long long ch = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (ch >= nch) return;
    const int lane = threadIdx.x & 63;
    const int g = chgene[ch];
    long long b, e;
    chunk_range(gptr, chptr, g, ch, b, e);
    double a = 0.0;
    if (PASS == 0) {
        int cnt = 0;
        double mn = gval[b], mx = mn;                        // (a chunk holds an entry)
        for (long long p = b + lane; p < e; p += 64) {
            const double v = gval[p];
            a += v;
            cnt += v != 0.0;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
        a = wave_sum(a);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off);
            mn = fmin(mn, __shfl_xor(mn, off));
            mx = fmax(mx, __shfl_xor(mx, off));
        }
        if (lane == 0) { psum[ch] = a; pcnt[ch] = cnt; pmin[ch] = mn; pmax[ch] = mx; }
    } else {
        const double m0 = mu[g];
        for (long long p = b + lane; p < e; p += 64) { const double d = gval[p] - m0; a += d * d; }
        a = wave_sum(a);
        if (lane == 0) psum[ch] = a;
    }
}

// One thread per gene folds its chunks in chunk order.  PASS 0: mu = S / n, or the one value of a gene whose n values are all equal
// (flag[g] = 1); gnnz.  PASS 1: var = (SS + (n - stored) mu^2) / (n - 1), 0 for a flagged gene.
template <int PASS>
__global__ __launch_bounds__(256) void expr_gene_fold_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr, int m,
                                                             long long n, const double *__restrict__ psum, const int *__restrict__ pcnt,
                                                             const double *__restrict__ pmin, const double *__restrict__ pmax,
                                                             double *__restrict__ mu, int *__restrict__ flag, long long *__restrict__ gnnz,
                                                             double *__restrict__ var) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= m) return;
    const long long stored = gptr[g + 1] - gptr[g];
    const long long c0 = chptr[g], c1 = chptr[g + 1];
    double S = 0.0;
    for (long long ch = c0; ch < c1; ++ch) S += psum[ch];
    if (PASS == 0) {
        long long cnt = 0;
        double mn = 0.0, mx = 0.0;
        if (stored > 0) { mn = pmin[c0]; mx = pmax[c0]; }
        for (long long ch = c0; ch < c1; ++ch) { cnt += pcnt[ch]; mn = fmin(mn, pmin[ch]); mx = fmax(mx, pmax[ch]); }
        if (stored > 0 && stored < n) { mn = fmin(mn, 0.0); mx = fmax(mx, 0.0); }
        const bool same = mn == mx;
        mu[g] = same ? mn : S / static_cast<double>(n);
        flag[g] = same;
        gnnz[g] = cnt;
    } else {
        const double m0 = mu[g];
        var[g] = flag[g] ? 0.0 : (S + static_cast<double>(n - stored) * (m0 * m0)) / static_cast<double>(n - 1);
    }
}

// sd = sqrt(var) and w = 1 / sd with scale (1 and 0 where var = 0), 1 and 1 without; wv = w^2 var
__global__ __launch_bounds__(256) void expr_weight_kernel(const double *__restrict__ var, int m, int scale, double *__restrict__ sd,
                                                          double *__restrict__ w, double *__restrict__ wv) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= m) return;
    const double v = var[g];
    double s = 1.0, x = 1.0;
    if (scale) {
        s = v > 0.0 ? sqrt(v) : 1.0;
        x = v > 0.0 ? 1.0 / s : 0.0;
    }
    sd[g] = s;
    w[g] = x;
    wv[g] = x * x * v;
}

// Bs[g, j] = w_g B[g, j]; col[j m + g] = mu_g Bs[g, j] (column-major, for the fixed-order sums of the shift)
__global__ __launch_bounds__(256) void expr_scale_rows_kernel(const double *__restrict__ B, const double *__restrict__ mu,
                                                              const double *__restrict__ w, long long m, int l, double *__restrict__ Bs,
                                                              double *__restrict__ col) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= m * l) return;
    const long long g = e / l;
    const int j = static_cast<int>(e - g * l);
    const double v = w[g] * B[e];
    Bs[e] = v;
    col[j * m + g] = mu[g] * v;
}

// col[j rows + r] = X[r, j]
__global__ __launch_bounds__(256) void expr_to_columns_kernel(const double *__restrict__ X, long long rows, int l, double *__restrict__ col) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= rows * l) return;
    const long long r = e / l;
    const int j = static_cast<int>(e - r * l);
    col[j * rows + r] = X[e];
}

// a0 (column lane) and a1 (column lane + 64) += sum over the entries [b, e), in stored order, of val[p] M[idx[p], column]: the pairs are
// loaded 64 at a time, one per lane, and broadcast; every entry is then one coalesced read of a row of M (l doubles)
template <int CPL>
__device__ __forceinline__ void gather_rows(const int *__restrict__ idx, const double *__restrict__ val, long long b, long long e,
                                            const double *__restrict__ M, int l, int lane, double &a0, double &a1) {
    const bool ok0 = lane < l, ok1 = CPL == 2 && lane + 64 < l;
    for (long long p0 = b; p0 < e; p0 += 64) {
        const int cnt = e - p0 < 64 ? static_cast<int>(e - p0) : 64;
        int r = 0;
        double v = 0.0;
        if (lane < cnt) { r = idx[p0 + lane]; v = val[p0 + lane]; }
        int q = 0;
        for (; q + 4 <= cnt; q += 4) {                       // four rows in flight; the sums keep the stored order
            const double *row[4];
            double vq[4], x0[4], x1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                row[u] = M + static_cast<long long>(__builtin_amdgcn_readlane(r, q + u)) * l;
                vq[u] = lane_get(v, q + u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                x0[u] = ok0 ? row[u][lane] : 0.0;
                x1[u] = ok1 ? row[u][lane + 64] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a0 += vq[u] * x0[u];
                if (CPL == 2) a1 += vq[u] * x1[u];
            }
        }
        for (; q < cnt; ++q) {
            const double *row = M + static_cast<long long>(__builtin_amdgcn_readlane(r, q)) * l;
            const double vq = lane_get(v, q);
            if (ok0) a0 += vq * row[lane];
            if (CPL == 2) { if (ok1) a1 += vq * row[lane + 64]; }
        }
    }
}

// Y[c, :] = sum over the cell's entries of t Bs[gene, :] - shift
template <int CPL>
__global__ __launch_bounds__(256) void expr_spmm_cells_kernel(const long long *__restrict__ cptr, const int *__restrict__ ridx,
                                                              const double *__restrict__ t, long long n, const double *__restrict__ Bs, int l,
                                                              const double *__restrict__ shift, double *__restrict__ Y) {
    const long long c = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const int lane = threadIdx.x & 63;
    double a0 = 0.0, a1 = 0.0;
    gather_rows<CPL>(ridx, t, cptr[c], cptr[c + 1], Bs, l, lane, a0, a1);
    if (lane < l) Y[c * l + lane] = a0 - shift[lane];
    if (CPL == 2 && lane + 64 < l) Y[c * l + lane + 64] = a1 - shift[lane + 64];
}

// part[ch, :] = sum over the chunk's entries, in cell order, of t Q[cell, :]
template <int CPL>
__global__ __launch_bounds__(256) void expr_spmm_genes_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr,
                                                              const int *__restrict__ chgene, long long nch, const int *__restrict__ gcell,
                                                              const double *__restrict__ gval, const double *__restrict__ Q, int l,
                                                              double *__restrict__ part) {
    const long long ch = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (ch >= nch) return;
    const int lane = threadIdx.x & 63;
    long long b, e;
    chunk_range(gptr, chptr, chgene[ch], ch, b, e);
    double a0 = 0.0, a1 = 0.0;
    gather_rows<CPL>(gcell, gval, b, e, Q, l, lane, a0, a1);
    if (lane < l) part[ch * l + lane] = a0;
    if (CPL == 2 && lane + 64 < l) part[ch * l + lane + 64] = a1;
}

// Z[g, j] = w_g (the gene's partial sums added in chunk order - mu_g cs[j])
__global__ __launch_bounds__(256) void expr_genes_fold_kernel(const long long *__restrict__ chptr, const double *__restrict__ part,
                                                              const double *__restrict__ mu, const double *__restrict__ w,
                                                              const double *__restrict__ cs, long long m, int l, double *__restrict__ Z) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= m * l) return;
    const long long g = e / l;
    const int j = static_cast<int>(e - g * l);
    double a = 0.0;
    const long long c1 = chptr[g + 1];
    for (long long ch = chptr[g]; ch < c1; ++ch) a += part[ch * l + j];
    Z[e] = w[g] * (a - mu[g] * cs[j]);
}

// out[e] (+)= the slabs' partial matrices in slab order
__global__ __launch_bounds__(256) void expr_slab_sum_kernel(const double *__restrict__ part, int nslab, int len, int first, double *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    double a = first ? 0.0 : out[e];
    for (int s = 0; s < nslab; ++s) a += part[static_cast<long long>(s) * len + e];
    out[e] = a;
}

// Y <- Y R^-1, R upper triangular (l x l, row-major): one wave per row, lane j holds y_j (and y_(j + 64)); step k fixes q_k = y_k / R_kk
// and takes q_k R_kj off every later column
template <int CPL>
__global__ __launch_bounds__(256) void expr_trsolve_kernel(double *__restrict__ Y, long long rows, int l, const double *__restrict__ R) {
    const int lane = threadIdx.x & 63;
    const int j0 = lane, j1 = lane + 64;
    for (long long r = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6); r < rows; r += static_cast<long long>(gridDim.x) * 4) {
        double y0 = j0 < l ? Y[r * l + j0] : 0.0;
        double y1 = (CPL == 2 && j1 < l) ? Y[r * l + j1] : 0.0;
        for (int k = 0; k < l; ++k) {
            const double yk = (CPL == 2 && k >= 64) ? lane_get(y1, k - 64) : lane_get(y0, k);
            const double qk = yk / R[k * l + k];
            if (j0 == k) y0 = qk;
            if (CPL == 2 && j1 == k) y1 = qk;
            if (j0 > k && j0 < l) y0 -= qk * R[k * l + j0];
            if (CPL == 2 && j1 > k && j1 < l) y1 -= qk * R[k * l + j1];
        }
        if (j0 < l) Y[r * l + j0] = y0;
        if (CPL == 2 && j1 < l) Y[r * l + j1] = y1;
    }
}

// Omega[g, j] = (mix(mix(seed * golden + g) + j) >> 11) 2^-53 - 0.5
__global__ __launch_bounds__(256) void expr_omega_kernel(u64 seed, long long m, int l, double *__restrict__ B) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= m * l) return;
    const long long g = e / l;
    const u64 j = static_cast<u64>(e - g * l);
    B[e] = static_cast<double>(mix64(mix64(seed * 0x9E3779B97F4A7C15ull + static_cast<u64>(g)) + j) >> 11) * 0x1.0p-53 - 0.5;
}

// out[r, j] = (sum over i of X[r, i] W[i, j]) f[j]: X rows x l, W l x k
__global__ __launch_bounds__(256) void expr_rotate_kernel(const double *__restrict__ X, const double *__restrict__ W, const double *__restrict__ f,
                                                          long long rows, int l, int k, double *__restrict__ out) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= rows * k) return;
    const long long r = e / k;
    const int j = static_cast<int>(e - r * k);
    double a = 0.0;
    for (int i = 0; i < l; ++i) a += X[r * l + i] * W[i * k + j];
    out[e] = a * f[j];
}

// sign[j] = -1 when component j's loading of largest magnitude (on ties the lowest gene) is negative, else 1; one workgroup per component
__global__ __launch_bounds__(256) void expr_sign_kernel(const double *__restrict__ L, long long m, int k, double *__restrict__ sign) {
    __shared__ double sa[256];
    __shared__ long long si[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    double best = -1.0;
    long long at = m;
    for (long long g = tid; g < m; g += 256) {
        const double a = fabs(L[g * k + j]);
        if (a > best) { best = a; at = g; }                  // (ascending g: the first of equal magnitudes stays)
    }
    sa[tid] = best;
    si[tid] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && (sa[tid + s] > sa[tid] || (sa[tid + s] == sa[tid] && si[tid + s] < si[tid]))) { sa[tid] = sa[tid + s]; si[tid] = si[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) sign[j] = (si[0] < m && L[si[0] * k + j] < 0.0) ? -1.0 : 1.0;
}

__global__ __launch_bounds__(256) void expr_flip_kernel(double *__restrict__ X, long long rows, int k, const double *__restrict__ sign) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < rows * k) X[e] *= sign[e % k];
}

// G (host, l x l) = Y^T Y
void gram(const double *Y, long long rows, int l, std::vector<double> &G) {
    Ctx &c = ctx();
    const int ll = l * l;
    const long long nslab = (rows + kExprSlabRows - 1) / kExprSlabRows;
    const int batch = static_cast<int>(std::min<long long>(nslab, kGramBatch));
    DevBuf<double> gpart(static_cast<size_t>(batch) * ll), g(ll);
    DevBuf<GemmTask> dtasks(batch);
    std::vector<GemmTask> tasks(batch);
    for (long long s0 = 0; s0 < nslab; s0 += batch) {
        const int ns = static_cast<int>(std::min<long long>(batch, nslab - s0));
        for (int s = 0; s < ns; ++s) {
            const long long r0 = (s0 + s) * kExprSlabRows;
            GemmTask &t = tasks[s];
            t = GemmTask{};
            t.At = Y + r0 * l;
            t.Bt = t.At;
            t.C = gpart.p + static_cast<long long>(s) * ll;
            t.M = t.N = l;
            t.K = static_cast<int>(std::min<long long>(kExprSlabRows, rows - r0));
            t.lda = t.ldb = t.ldc = l;
            t.epilogue = 0;
            t.symmetric = 1;
            t.fast = 0;
        }
        dtasks.upload(tasks.data(), ns);
        gemm_tn_f64_batched(dtasks.p, ns, l, l, "expr_gram", false, true);
        hipLaunchKernelGGL(expr_slab_sum_kernel, dim3(grid_for(ll, 256)), dim3(256), 0, c.stream, gpart.p, ns, ll, s0 == 0 ? 1 : 0, g.p);
        launch_check("expr_slab_sum_kernel");
        stream_sync();                                       // (the host tasks are written again)
    }
    G.resize(ll);
    g.download(G.data(), ll);
}

// R upper triangular (row-major) with G = R^T R.  A pivot that is not finite, <= 0 or within l 2^-52 of G's diagonal -- what rounding
// alone leaves of a zero -- refuses by name.
void cholesky_upper(const std::string &who, const std::vector<double> &G, int l, std::vector<double> &R) {
    R.assign(static_cast<size_t>(l) * l, 0.0);
    const double tiny = static_cast<double>(l) * 0x1.0p-52;
    for (int j = 0; j < l; ++j) {
        double d = G[static_cast<size_t>(j) * l + j];
        for (int k = 0; k < j; ++k) d -= R[static_cast<size_t>(k) * l + j] * R[static_cast<size_t>(k) * l + j];
        SHARP_REQUIRE(std::isfinite(d) && d > tiny * G[static_cast<size_t>(j) * l + j], who + ": numerical rank below n_components + oversample");
        const double rjj = std::sqrt(d);
        R[static_cast<size_t>(j) * l + j] = rjj;
        for (int i = j + 1; i < l; ++i) {
            double a = G[static_cast<size_t>(j) * l + i];
            for (int k = 0; k < j; ++k) a -= R[static_cast<size_t>(k) * l + j] * R[static_cast<size_t>(k) * l + i];
            R[static_cast<size_t>(j) * l + i] = a / rjj;
        }
    }
}

// out[j] = the sum of column j of col (column-major, rows values each), j = 0 .. l: graph.hpp's fixed order
void column_sums(const double *col, long long rows, int l, double *red, double *out) {
    for (int j = 0; j < l; ++j) fixed_reduce(Fold::Sum, col + static_cast<long long>(j) * rows, rows, red, out + j);
}

// m: the genes of the copies that the fit works on; m_in > 0: a subset of m_in genes, whose count, scan, fill and table stand beside the
// full cell-major copy
double bytes_needed(long long n, long long m, long long nnz, bool genes, int l, long long m_in) {
    double b = static_cast<double>(nnz) * 12.0 + static_cast<double>(n) * 16.0 + 67108864.0;
    if (m_in > 0) b += static_cast<double>(nnz) * 12.0 + static_cast<double>(n) * 24.0 + static_cast<double>(m_in) * 4.0;
    if (genes) b += static_cast<double>(nnz) * 28.0 + static_cast<double>(nnz / kExprChunk + m) * 32.0 + static_cast<double>(m) * 80.0;
    if (l > 0) {
        const double rows = static_cast<double>(std::max(n, m));
        b += (2.0 * static_cast<double>(n + m) + rows + static_cast<double>(nnz / kExprChunk + m)) * l * 8.0;
        b += std::min(rows / kExprSlabRows + 1.0, static_cast<double>(kGramBatch)) * l * l * 8.0;
    }
    return b;
}

void check_l(const std::string &who, int k, int oversample, long long n, int m) {
    SHARP_REQUIRE(k >= 1, who + ": n_components must be >= 1");
    SHARP_REQUIRE(oversample >= 0, who + ": oversample must be >= 0");
    SHARP_REQUIRE(static_cast<long long>(k) + oversample <= kExprMaxL, who + ": n_components + oversample must be <= 128");
    SHARP_REQUIRE(static_cast<long long>(k) + oversample <= std::min<long long>(n, m),
                  who + ": n_components + oversample must be <= min(cells, genes)");
}

// Drops the entries of the genes that `genes` does not keep and renumbers the kept ones by their position in it: a count
// per cell, the scan, a fill into fresh buffers.  genes was checked by expr_check_genes.
void subset_impl(ExprData &D, const int *genes, int mk) {
    Ctx &c = ctx();
    KernelTimer timer("expr_subset");
    const long long n = D.n;
    std::vector<int> map(D.m, -1);
    for (int i = 0; i < mk; ++i) map[genes[i]] = i;
    DevBuf<int> remap(D.m);
    remap.upload(map.data(), map.size());
    DevBuf<long long> cnt(n + 1), nptr(n + 1);
    Scratch tmp;
    SHARP_HIP_CHECK(hipMemsetAsync(cnt.p + n, 0, sizeof(long long), c.stream));      // (the scan's extra slot)
    hipLaunchKernelGGL(expr_subset_count_kernel, dim3(wave_grid(n)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, n, remap.p, cnt.p);
    launch_check("expr_subset_count_kernel");
    exclusive_scan(cnt.p, nptr.p, static_cast<size_t>(n + 1), tmp);
    long long kept = 0;
    SHARP_HIP_CHECK(hipMemcpyAsync(&kept, nptr.p + n, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
    stream_sync();
    DevBuf<int> ridx2(std::max<long long>(kept, 1));
    DevBuf<double> t2(std::max<long long>(kept, 1));
    hipLaunchKernelGGL(expr_subset_fill_kernel, dim3(wave_grid(n)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, D.t.p, n, remap.p, nptr.p,
                       ridx2.p, t2.p);
    launch_check("expr_subset_fill_kernel");
    stream_sync();                                           // (the old copy, map and the temporaries go)
    D.cptr = std::move(nptr);
    D.ridx = std::move(ridx2);
    D.t = std::move(t2);
    D.nnz = kept;
    D.m = mk;
}

}  // namespace

unsigned wave_grid(long long items) { return grid_for(items, 4); }

void expr_transform(ExprData &D, double normalize_total, bool lg) {
    if (normalize_total > 0.0 || lg)
        hipLaunchKernelGGL(expr_transform_kernel, dim3(wave_grid(D.n)), dim3(256), 0, ctx().stream, D.cptr.p, D.lsum.p, D.n, normalize_total,
                           lg ? 1 : 0, D.t.p);
    launch_check("expr_transform_kernel");
}

void expr_subset(ExprData &D, const int *genes, int n_genes) { subset_impl(D, genes, n_genes); }

void expr_check_options(const std::string &who, double normalize_total, int m) {
    SHARP_REQUIRE(m >= 1 && m <= kExprMaxM, who + ": need 1 <= m <= 16777216 genes");
    SHARP_REQUIRE(std::isfinite(normalize_total) && normalize_total >= 0.0, who + ": normalize_total must be finite and >= 0 (0: off)");
}

long long expr_total_cells(const std::string &who, const ExprBlocks &B) {
    SHARP_REQUIRE(B.nblocks >= 1 && B.colptr && B.rowidx && B.val && B.ncb, who + ": need a list of at least one block");
    long long n = 0;
    for (int b = 0; b < B.nblocks; ++b) {
        SHARP_REQUIRE(B.ncb[b] >= 0 && B.ncb[b] <= kExprMaxN, who + ": block " + std::to_string(b + 1) + " has an impossible number of cells");
        n += B.ncb[b];
        SHARP_REQUIRE(n <= kExprMaxN, who + ": need at most 2^31 - 2 cells in all");
    }
    return n;
}

int expr_check_genes(const std::string &who, const int *genes, int n_genes, int m) {
    if (!genes && n_genes == 0) return m;
    SHARP_REQUIRE(genes && n_genes >= 1, who + ": genes is empty (it must keep at least one gene)");
    for (int i = 0; i < n_genes; ++i) {
        SHARP_REQUIRE(genes[i] >= 0 && genes[i] < m, who + ": genes holds an index outside [0, m) (position " + std::to_string(i) + ", counted from 0)");
        if (i == 0) continue;
        SHARP_REQUIRE(genes[i] != genes[i - 1], who + ": genes holds a gene twice (position " + std::to_string(i) + ", counted from 0)");
        SHARP_REQUIRE(genes[i] > genes[i - 1], who + ": genes must be ascending (position " + std::to_string(i) + ", counted from 0)");
    }
    return n_genes;
}

void expr_load(const std::string &who, const ExprBlocks &B, double normalize_total, bool lg, bool genes, bool scale, int l_work,
               long long min_cells, ExprData &D, const ExprExtra &extra) {
    expr_check_options(who, normalize_total, B.m);
    const long long n = expr_total_cells(who, B);
    const int mk = expr_check_genes(who, extra.genes, extra.n_genes, B.m);
    SHARP_REQUIRE(n >= min_cells, who + ": need at least " + std::to_string(min_cells) + " cells in all");
    // the cells' offsets, from the blocks' own column pointers (checked here: the host reads the stored entries by them)
    std::vector<long long> cp(static_cast<size_t>(n) + 1);
    std::vector<long long> off(B.nblocks + 1, 0);
    long long c0 = 0;
    cp[0] = 0;
    for (int b = 0; b < B.nblocks; ++b) {
        const int *p = B.colptr[b];
        SHARP_REQUIRE(p && p[0] == 0, who + ": block " + std::to_string(b + 1) + ": colptr must start at 0");
        for (long long c = 0; c < B.ncb[b]; ++c) {
            SHARP_REQUIRE(p[c + 1] >= p[c], who + ": colptr decreases (cell " + std::to_string(c0 + c) + ", counted from 0)");
            cp[c0 + c + 1] = off[b] + p[c + 1];
        }
        off[b + 1] = off[b] + p[B.ncb[b]];
        SHARP_REQUIRE(p[B.ncb[b]] == 0 || (B.rowidx[b] && B.val[b]), who + ": block " + std::to_string(b + 1) + ": null rowidx / val");
        c0 += B.ncb[b];
    }
    const long long nnz = off[B.nblocks];
    SHARP_REQUIRE(nnz < kExprMaxNnz, who + ": the blocks hold " + std::to_string(nnz) + " stored entries; need fewer than 2^38");
    Ctx &c = ctx();
    size_t free_b = 0, total_b = 0;
    SHARP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const double need = bytes_needed(n, mk, nnz, genes, l_work, extra.genes ? B.m : 0);
    SHARP_REQUIRE(need <= static_cast<double>(free_b), who + ": the expression data (" + std::to_string(nnz) + " stored entries" +
                                                          (genes ? ", two copies" : "") + ") and the workspaces need about " +
                                                          std::to_string(static_cast<long long>(need / 1048576.0)) +
                                                          " MB; the device has " + std::to_string(free_b >> 20) + " MB free");
    D.n = n;
    D.m = D.m_in = B.m;
    D.nnz = nnz;
    const bool check_neg = normalize_total > 0.0 || lg || extra.refuse_negative;
    {
        KernelTimer timer("expr_upload");
        D.cptr.alloc(n + 1);
        D.cptr.upload(cp.data(), cp.size());
        D.ridx.alloc(std::max<long long>(nnz, 1));
        D.t.alloc(std::max<long long>(nnz, 1));
        D.lsum.alloc(std::max<long long>(n, 1));
        for (int b = 0; b < B.nblocks; ++b) {
            const long long cnt = off[b + 1] - off[b];
            if (!cnt) continue;
            SHARP_HIP_CHECK(hipMemcpyAsync(D.ridx.p + off[b], B.rowidx[b], cnt * sizeof(int), hipMemcpyHostToDevice, c.stream));
            SHARP_HIP_CHECK(hipMemcpyAsync(D.t.p + off[b], B.val[b], cnt * sizeof(double), hipMemcpyHostToDevice, c.stream));
        }
        DevBuf<u64> word(1);
        SHARP_HIP_CHECK(hipMemsetAsync(word.p, 0xFF, sizeof(u64), c.stream));
        hipLaunchKernelGGL(expr_validate_kernel, dim3(wave_grid(n)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, D.t.p, n, B.m, check_neg ? 1 : 0,
                           word.p);
        launch_check("expr_validate_kernel");
        u64 w = EX_OK;
        word.download(&w, 1);                                // (synchronises: cp may go)
        if (w != EX_OK) {
            const std::string cell = " (cell " + std::to_string(w >> 3) + ", counted from 0)";
            switch (static_cast<int>(w & 7)) {
                case EX_RANGE: throw Error(SHARP_ERR_ARG, who + ": a gene index outside [0, m)" + cell);
                case EX_ORDER: throw Error(SHARP_ERR_ARG, who + ": gene indices must be strictly ascending within a cell" + cell);
                case EX_FINITE: throw Error(SHARP_ERR_ARG, who + ": a value that is NaN or infinite" + cell);
                default:
                    throw Error(SHARP_ERR_ARG, who + (extra.refuse_negative ? ": a negative value where counts are expected" :
                                                                              ": a negative value under normalize_total / log1p") + cell);
            }
        }
        hipLaunchKernelGGL(expr_cell_sums_kernel, dim3(wave_grid(n)), dim3(256), 0, c.stream, D.cptr.p, D.t.p, n, D.lsum.p);
        expr_transform(D, normalize_total, lg);
        if (extra.want_tsum) {
            D.tsum.alloc(std::max<long long>(n, 1));
            hipLaunchKernelGGL(expr_cell_sums_kernel, dim3(wave_grid(n)), dim3(256), 0, c.stream, D.cptr.p, D.t.p, n, D.tsum.p);
            launch_check("expr_cell_sums_kernel");
        }
    }
    if (extra.genes) subset_impl(D, extra.genes, mk);
    if (!genes) return;
    const int m = D.m;
    {
        KernelTimer timer("expr_transpose");
        const long long nnz = D.nnz;                         // (the kept entries under a subset)
        D.gptr.alloc(m + 1);
        D.gcell.alloc(std::max<long long>(nnz, 1));
        D.gval.alloc(std::max<long long>(nnz, 1));
        DevBuf<u64> keys(std::max<long long>(nnz, 1)), keys_s(std::max<long long>(nnz, 1));
        Scratch tmp;
        if (nnz) {
            hipLaunchKernelGGL(expr_keys_kernel, dim3(wave_grid(n)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, n, keys.p);
            launch_check("expr_keys_kernel");
            // stable on the gene bits alone: the cells of a gene keep the ascending order they were written in
            sort_pairs(keys.p, keys_s.p, D.t.p, D.gval.p, static_cast<size_t>(nnz), 32, 32 + key_bits(static_cast<u64>(m - 1)), tmp);
            hipLaunchKernelGGL(expr_unkey_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, c.stream, keys_s.p, nnz, D.gcell.p);
        }
        hipLaunchKernelGGL(expr_gptr_kernel, dim3(grid_for(m + 1, 256)), dim3(256), 0, c.stream, keys_s.p, nnz, m, D.gptr.p);
        launch_check("expr_gptr_kernel");
        DevBuf<long long> nchunk(m + 1);
        D.chptr.alloc(m + 1);
        hipLaunchKernelGGL(expr_nchunk_kernel, dim3(grid_for(m + 1, 256)), dim3(256), 0, c.stream, D.gptr.p, m, nchunk.p);
        exclusive_scan(nchunk.p, D.chptr.p, static_cast<size_t>(m + 1), tmp);
        SHARP_HIP_CHECK(hipMemcpyAsync(&D.nch, D.chptr.p + m, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
        stream_sync();                                       // (keys, nchunk and tmp leave scope)
        D.chgene.alloc(std::max<long long>(D.nch, 1));
        hipLaunchKernelGGL(expr_chgene_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c.stream, D.chptr.p, m, D.chgene.p);
        launch_check("expr_chgene_kernel");
    }
    {
        KernelTimer timer("expr_stats");
        const long long nch = D.nch;
        D.mu.alloc(m); D.var.alloc(m); D.sd.alloc(m); D.w.alloc(m); D.gnnz.alloc(m);
        DevBuf<double> psum(std::max<long long>(nch, 1)), pmin(std::max<long long>(nch, 1)), pmax(std::max<long long>(nch, 1)), wv(m), red(kRedBlocks), tv(1);
        DevBuf<int> pcnt(std::max<long long>(nch, 1)), flag(m);
        if (nch) hipLaunchKernelGGL(expr_gene_stats_kernel<0>, dim3(wave_grid(nch)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, D.chgene.p, nch,
                                    D.gval.p, nullptr, psum.p, pcnt.p, pmin.p, pmax.p);
        hipLaunchKernelGGL(expr_gene_fold_kernel<0>, dim3(grid_for(m, 256)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, m, n, psum.p, pcnt.p,
                           pmin.p, pmax.p, D.mu.p, flag.p, D.gnnz.p, D.var.p);
        if (nch) hipLaunchKernelGGL(expr_gene_stats_kernel<1>, dim3(wave_grid(nch)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, D.chgene.p, nch,
                                    D.gval.p, D.mu.p, psum.p, nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(expr_gene_fold_kernel<1>, dim3(grid_for(m, 256)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, m, n, psum.p, pcnt.p,
                           pmin.p, pmax.p, D.mu.p, flag.p, D.gnnz.p, D.var.p);
        hipLaunchKernelGGL(expr_weight_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c.stream, D.var.p, m, scale ? 1 : 0, D.sd.p, D.w.p, wv.p);
        launch_check("expr_weight_kernel");
        fixed_reduce(Fold::Sum, wv.p, m, red.p, tv.p);
        tv.download(&D.total_var, 1);                        // (synchronises: the partial sums leave scope)
    }
}

void expr_spmm_cells(const ExprData &D, const double *mu, const double *w, const double *Bm, int l, double *Y) {
    Ctx &c = ctx();
    KernelTimer timer("expr_spmm_cells");
    const long long ml = static_cast<long long>(D.m) * l;
    DevBuf<double> Bs(ml), col(ml), shift(l), red(kRedBlocks);
    hipLaunchKernelGGL(expr_scale_rows_kernel, dim3(grid_for(ml, 256)), dim3(256), 0, c.stream, Bm, mu, w, static_cast<long long>(D.m), l, Bs.p,
                       col.p);
    launch_check("expr_scale_rows_kernel");
    column_sums(col.p, D.m, l, red.p, shift.p);
    KernelTimer kernel("expr_cells_kernel");
    if (l <= 64)
        hipLaunchKernelGGL(expr_spmm_cells_kernel<1>, dim3(wave_grid(D.n)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, D.t.p, D.n, Bs.p, l, shift.p, Y);
    else
        hipLaunchKernelGGL(expr_spmm_cells_kernel<2>, dim3(wave_grid(D.n)), dim3(256), 0, c.stream, D.cptr.p, D.ridx.p, D.t.p, D.n, Bs.p, l, shift.p, Y);
    launch_check("expr_spmm_cells_kernel");
    stream_sync();                                           // (the temporaries leave scope)
}

void expr_spmm_genes(const ExprData &D, const double *Q, int l, double *Z) {
    Ctx &c = ctx();
    KernelTimer timer("expr_spmm_genes");
    const long long nl = D.n * l, ml = static_cast<long long>(D.m) * l;
    DevBuf<double> col(nl), cs(l), red(kRedBlocks), part(std::max<long long>(D.nch, 1) * l);
    hipLaunchKernelGGL(expr_to_columns_kernel, dim3(grid_for(nl, 256)), dim3(256), 0, c.stream, Q, D.n, l, col.p);
    launch_check("expr_to_columns_kernel");
    column_sums(col.p, D.n, l, red.p, cs.p);
    if (D.nch) {
        KernelTimer kernel("expr_genes_kernel");
        if (l <= 64)
            hipLaunchKernelGGL(expr_spmm_genes_kernel<1>, dim3(wave_grid(D.nch)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, D.chgene.p, D.nch,
                               D.gcell.p, D.gval.p, Q, l, part.p);
        else
            hipLaunchKernelGGL(expr_spmm_genes_kernel<2>, dim3(wave_grid(D.nch)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, D.chgene.p, D.nch,
                               D.gcell.p, D.gval.p, Q, l, part.p);
    }
    hipLaunchKernelGGL(expr_genes_fold_kernel, dim3(grid_for(ml, 256)), dim3(256), 0, c.stream, D.chptr.p, part.p, D.mu.p, D.w.p, cs.p,
                       static_cast<long long>(D.m), l, Z);
    launch_check("expr_genes_fold_kernel");
    stream_sync();
}

void expr_orth(const std::string &who, double *Y, long long rows, int l) {
    Ctx &c = ctx();
    KernelTimer timer("expr_orth");
    DevBuf<double> dR(static_cast<size_t>(l) * l);
    std::vector<double> G, R;
    const unsigned grid = static_cast<unsigned>(std::min<long long>(wave_grid(rows), static_cast<long long>(c.num_cu) * 32));
    for (int pass = 0; pass < 2; ++pass) {
        gram(Y, rows, l, G);
        cholesky_upper(who, G, l, R);
        dR.upload(R.data(), R.size());
        if (l <= 64) hipLaunchKernelGGL(expr_trsolve_kernel<1>, dim3(grid), dim3(256), 0, c.stream, Y, rows, l, dR.p);
        else hipLaunchKernelGGL(expr_trsolve_kernel<2>, dim3(grid), dim3(256), 0, c.stream, Y, rows, l, dR.p);
        launch_check("expr_trsolve_kernel");
        stream_sync();                                       // (R is written again)
    }
}

namespace {

struct ExprFit {
    DevBuf<double> scores, loadings;
    std::vector<double> s;
};

void expr_fit(const std::string &who, ExprData &D, int k, int oversample, int n_iter, u64 seed, ExprFit &F) {
    Ctx &c = ctx();
    const int l = k + oversample, m = D.m;
    const long long n = D.n, ml = static_cast<long long>(m) * l, nl = n * l;
    SHARP_REQUIRE(D.total_var > 0.0 && std::isfinite(D.total_var),
                  who + ": numerical rank below n_components + oversample (no gene varies across the cells)");
    DevBuf<double> Y(nl), Z(ml);
    hipLaunchKernelGGL(expr_omega_kernel, dim3(grid_for(ml, 256)), dim3(256), 0, c.stream, seed, static_cast<long long>(m), l, Z.p);
    launch_check("expr_omega_kernel");
    expr_spmm_cells(D, D.mu.p, D.w.p, Z.p, l, Y.p);
    for (int it = 0; it < n_iter; ++it) {
        expr_orth(who, Y.p, n, l);
        expr_spmm_genes(D, Y.p, l, Z.p);
        expr_orth(who, Z.p, m, l);
        expr_spmm_cells(D, D.mu.p, D.w.p, Z.p, l, Y.p);
    }
    expr_orth(who, Y.p, n, l);
    expr_spmm_genes(D, Y.p, l, Z.p);
    // Z^T Z = W diag(lambda) W^T on the host, descending
    std::vector<double> G, lam;
    gram(Z.p, m, l, G);
    if (l == 1) lam.assign(1, G[0]), G[0] = 1.0;
    else {
        HostTimer ht("expr_eigen");
        symmetric_eigen("Rtsne", l, G, lam);   // (eigenvectors in G's columns; a refusal keeps the name it has always had)
    }
    std::vector<int> ord(l);
    for (int i = 0; i < l; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return lam[a] > lam[b]; });
    std::vector<double> W(static_cast<size_t>(l) * k), f(k);
    F.s.resize(k);
    for (int j = 0; j < k; ++j) {
        const int src = ord[j];
        SHARP_REQUIRE(lam[src] > 0.0 && std::isfinite(lam[src]), who + ": numerical rank below n_components + oversample");
        F.s[j] = std::sqrt(lam[src]);
        f[j] = 1.0 / F.s[j];
        for (int i = 0; i < l; ++i) W[static_cast<size_t>(i) * k + j] = G[static_cast<size_t>(i) * l + src];
    }
    DevBuf<double> dW(W.size()), df(f.size()), sign(k);
    dW.upload(W.data(), W.size());
    df.upload(f.data(), f.size());
    F.loadings.alloc(static_cast<long long>(m) * k);
    hipLaunchKernelGGL(expr_rotate_kernel, dim3(grid_for(static_cast<long long>(m) * k, 256)), dim3(256), 0, c.stream, Z.p, dW.p, df.p,
                       static_cast<long long>(m), l, k, F.loadings.p);
    hipLaunchKernelGGL(expr_sign_kernel, dim3(k), dim3(256), 0, c.stream, F.loadings.p, static_cast<long long>(m), k, sign.p);
    hipLaunchKernelGGL(expr_flip_kernel, dim3(grid_for(static_cast<long long>(m) * k, 256)), dim3(256), 0, c.stream, F.loadings.p,
                       static_cast<long long>(m), k, sign.p);
    launch_check("expr_flip_kernel");
    stream_sync();                                           // (the temporaries leave scope)
    // scores = A loadings: the cell-side product once more, which is what expression_pca_transform computes for any cell
    Y.release();
    F.scores.alloc(n * k);
    expr_spmm_cells(D, D.mu.p, D.w.p, F.loadings.p, k, F.scores.p);
}

}  // namespace
}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_expr_row_caps(int *chunk, int *slab_rows) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(chunk && slab_rows, "sharp_expr_row_caps: null output");
    *chunk = kExprChunk;
    *slab_rows = kExprSlabRows;
    SHARP_API_END
}

int sharp_expr_pca_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                       int n_components, int oversample, int n_iter, double normalize_total, int log1p, int scale, long long seed,
                       double *scores, double *loadings, double *singular_values, double *sdev, double *center, double *scale_out,
                       double *gene_var, double *total_var) {
    return sharp_expr_pca_sub_csc(colptr, rowidx, val, ncb, nblocks, m, n_components, oversample, n_iter, normalize_total, log1p, scale, seed,
                                  scores, loadings, singular_values, sdev, center, scale_out, gene_var, total_var, nullptr, 0);
}

int sharp_expr_pca_sub_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                           int m, int n_components, int oversample, int n_iter, double normalize_total, int log1p, int scale, long long seed,
                           double *scores, double *loadings, double *singular_values, double *sdev, double *center, double *scale_out,
                           double *gene_var, double *total_var, const int *genes, int n_genes) {
    SHARP_API_BEGIN
    const std::string w("expression_pca");
    SHARP_REQUIRE(scores && loadings && singular_values && sdev && center && scale_out && gene_var && total_var, w + ": null output");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    expr_check_options(w, normalize_total, m);
    const long long n = expr_total_cells(w, B);
    SHARP_REQUIRE(n >= 2, w + ": need at least 2 cells in all");
    const int mk = expr_check_genes(w, genes, n_genes, m);
    check_l(w, n_components, oversample, n, mk);
    SHARP_REQUIRE(n_iter >= 0 && n_iter <= 1000, w + ": n_iter must be in 0 .. 1000");
    ctx();
    ExprData D;
    ExprExtra extra;
    extra.genes = genes;
    extra.n_genes = n_genes;
    expr_load(w, B, normalize_total, log1p != 0, true, scale != 0, n_components + oversample, 2, D, extra);
    ExprFit F;
    expr_fit(w, D, n_components, oversample, n_iter, static_cast<u64>(seed), F);
    const int k = n_components;
    F.scores.download(scores, static_cast<size_t>(n) * k);
    F.loadings.download(loadings, static_cast<size_t>(mk) * k);
    for (int j = 0; j < k; ++j) {
        singular_values[j] = F.s[j];
        sdev[j] = F.s[j] / std::sqrt(static_cast<double>(n - 1));
    }
    D.mu.download(center, mk);
    D.sd.download(scale_out, mk);
    D.var.download(gene_var, mk);
    *total_var = D.total_var;
    SHARP_API_END
}

int sharp_expr_stats_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                         double normalize_total, int log1p, double *mean, double *var, long long *nnz, double *cell_sum) {
    return sharp_expr_stats_sub_csc(colptr, rowidx, val, ncb, nblocks, m, normalize_total, log1p, mean, var, nnz, cell_sum, nullptr, 0);
}

int sharp_expr_stats_sub_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                             int m, double normalize_total, int log1p, double *mean, double *var, long long *nnz, double *cell_sum,
                             const int *genes, int n_genes) {
    SHARP_API_BEGIN
    const std::string w("gene_stats");
    SHARP_REQUIRE(mean && var && nnz && cell_sum, w + ": null output");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    expr_check_options(w, normalize_total, m);
    SHARP_REQUIRE(expr_total_cells(w, B) >= 2, w + ": need at least 2 cells in all");
    const int mk = expr_check_genes(w, genes, n_genes, m);
    ctx();
    ExprData D;
    ExprExtra extra;
    extra.genes = genes;
    extra.n_genes = n_genes;
    extra.want_tsum = true;                                  // (over all genes, so before any subset)
    expr_load(w, B, normalize_total, log1p != 0, true, false, 0, 2, D, extra);
    D.mu.download(mean, mk);
    D.var.download(var, mk);
    D.gnnz.download(nnz, mk);
    D.tsum.download(cell_sum, D.n);
    SHARP_API_END
}

int sharp_expr_pca_transform_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                                 int m, double normalize_total, int log1p, const double *loadings, const double *center, const double *scale,
                                 int n_components, double *scores) {
    return sharp_expr_pca_transform_sub_csc(colptr, rowidx, val, ncb, nblocks, m, normalize_total, log1p, loadings, center, scale, n_components,
                                            scores, nullptr, 0);
}

int sharp_expr_pca_transform_sub_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                                     int nblocks, int m, double normalize_total, int log1p, const double *loadings, const double *center,
                                     const double *scale, int n_components, double *scores, const int *genes, int n_genes) {
    SHARP_API_BEGIN
    const std::string w("expression_pca_transform");
    SHARP_REQUIRE(loadings && center && scale && scores, w + ": null loadings / center / scale / scores");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    expr_check_options(w, normalize_total, m);
    const long long n = expr_total_cells(w, B);
    SHARP_REQUIRE(n_components >= 1 && n_components <= kExprMaxL, w + ": need 1 <= n_components <= 128");
    const int mk = expr_check_genes(w, genes, n_genes, m);   // (loadings, center and scale have a row per kept gene)
    std::vector<double> wt(mk);
    for (int g = 0; g < mk; ++g) {
        SHARP_REQUIRE(std::isfinite(scale[g]) && scale[g] > 0.0 && std::isfinite(center[g]),
                      w + ": the fit's scale must be positive and its center finite (gene " + std::to_string(g) + ", counted from 0)");
        wt[g] = 1.0 / scale[g];
    }
    ctx();
    if (n == 0) return SHARP_OK;
    ExprData D;
    ExprExtra extra;
    extra.genes = genes;
    extra.n_genes = n_genes;
    expr_load(w, B, normalize_total, log1p != 0, false, false, n_components, 0, D, extra);
    const int k = n_components;
    DevBuf<double> V(static_cast<size_t>(mk) * k), mu(mk), dw(mk), Y(static_cast<size_t>(n) * k);
    V.upload(loadings, V.n);
    mu.upload(center, mk);
    dw.upload(wt.data(), mk);
    expr_spmm_cells(D, mu.p, dw.p, V.p, k, Y.p);
    Y.download(scores, Y.n);
    SHARP_API_END
}

int sharp_expr_spmm_cells(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                          double normalize_total, int log1p, int scale, const double *Bm, int l, double *Y) {
    SHARP_API_BEGIN
    const std::string w("expr_spmm_cells");
    SHARP_REQUIRE(Bm && Y, w + ": null B / Y");
    SHARP_REQUIRE(l >= 1 && l <= kExprMaxL, w + ": need 1 <= l <= 128 columns");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    expr_check_options(w, normalize_total, m);
    SHARP_REQUIRE(expr_total_cells(w, B) >= 2, w + ": need at least 2 cells in all");
    ctx();
    ExprData D;
    expr_load(w, B, normalize_total, log1p != 0, true, scale != 0, l, 2, D);
    DevBuf<double> dB(static_cast<size_t>(m) * l), dY(static_cast<size_t>(D.n) * l);
    dB.upload(Bm, dB.n);
    expr_spmm_cells(D, D.mu.p, D.w.p, dB.p, l, dY.p);
    dY.download(Y, dY.n);
    SHARP_API_END
}

int sharp_expr_spmm_genes(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                          double normalize_total, int log1p, int scale, const double *Q, int l, double *Z) {
    SHARP_API_BEGIN
    const std::string w("expr_spmm_genes");
    SHARP_REQUIRE(Q && Z, w + ": null Q / Z");
    SHARP_REQUIRE(l >= 1 && l <= kExprMaxL, w + ": need 1 <= l <= 128 columns");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    expr_check_options(w, normalize_total, m);
    SHARP_REQUIRE(expr_total_cells(w, B) >= 2, w + ": need at least 2 cells in all");
    ctx();
    ExprData D;
    expr_load(w, B, normalize_total, log1p != 0, true, scale != 0, l, 2, D);
    DevBuf<double> dQ(static_cast<size_t>(D.n) * l), dZ(static_cast<size_t>(m) * l);
    dQ.upload(Q, dQ.n);
    expr_spmm_genes(D, dQ.p, l, dZ.p);
    dZ.download(Z, dZ.n);
    SHARP_API_END
}

int sharp_expr_orth(const double *Y, long long rows, int l, double *Q) {
    SHARP_API_BEGIN
    const std::string w("expr_orth");
    SHARP_REQUIRE(Y && Q, w + ": null Y / Q");
    SHARP_REQUIRE(l >= 1 && l <= kExprMaxL, w + ": need 1 <= l <= 128 columns");
    SHARP_REQUIRE(rows >= l && rows <= kExprMaxN, w + ": need l <= rows <= 2^31 - 2");
    ctx();
    DevBuf<double> d(static_cast<size_t>(rows) * l);
    d.upload(Y, d.n);
    expr_orth(w, d.p, rows, l);
    d.download(Q, d.n);
    SHARP_API_END
}

}  // extern "C"
