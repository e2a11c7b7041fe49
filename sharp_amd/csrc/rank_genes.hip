// rank_genes.hip -- rank_genes_groups: which genes distinguish each group of cells from the rest, or from a reference group (DESIGN.md
// §27; the specification is the project's own, restated in numpy in tests/_rank_genes_ref.py).
//   load      expr_load: upload, transform, subset, the gene-major copy (gptr / gcell / gval, cells ascending within a gene) and its
//             chunks of kExprChunk entries (chptr / chgene)
//   order     per gene, the stored entries by value: an order-preserving 64-bit image of the double (x + 0.0, so -0 is 0) as the key, the
//             cell's group as the payload, one rocPRIM segmented radix sort over the gptr segments.  The sort's order within a tie is
//             not relied on: nothing below depends on it.
//   stats     one wave per chunk.  A tie run [lo, hi) (two binary searches in the gene's segment) has 2 x average rank lo + hi + 1, plus
//             2 n_zero above the zeros; the stored zeros are one run with the implicit ones.  Per (gene, group): the exact 2R of the
//             stored entries, their count and the stored zeros; per gene: the sum of t^3 - t over the non-zero runs and the negatives.
//             The sums of x and x^2 per group: the wave takes its 64 entries group by group (a ballot picks the first lane's group, a
//             butterfly sums the lanes of that group), lane 0 adds to the workgroup's LDS table, and a gene's chunks are folded in chunk
//             order by one thread per (gene, group).  No floating-point atomic anywhere: the order of every sum is fixed by the sorted
//             list, and equal values are interchangeable, so two calls give the same bits.
//   reference a second segmented sort of the 31-bit keys (run start << 10 | group) makes the entries of one value and one group
//             contiguous.  A device-wide exclusive scan of "is a reference entry" gives, for every run, the reference entries below it
//             and in it; the head of each (run, group) sub-run adds t_g (2 below + tied) to 2U and (t_g + t_ref)^3 - (t_g + t_ref) -
//             (t_ref^3 - t_ref) to the pair's tie term, the reference's own sub-runs add t_ref^3 - t_ref to the gene's base.
//   finalize  one thread per (group, gene): the implicit zeros from the sizes, U, auc, sigma, z, erfc, the means, shares, fold change
//             and Welch's t and degrees of freedom.  The t-test's p-value (the incomplete beta function) and Benjamini-Hochberg run on the
//             host over the G x m table.
//   sort      per group by (score descending, gene ascending), NaN last: two stable device-wide radix sorts, the score's image and then
//             the group, as an LSD sort does.
#include "rank_genes.hpp"
#include "graph_prim.hpp"

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

namespace sharp {
namespace {

using u32 = unsigned int;
constexpr u64 kZeroKey = 0x8000000000000000ull;  // the image of 0.0

__device__ __forceinline__ u64 rank_key(double x) {
    const u64 b = static_cast<u64>(__double_as_longlong(x + 0.0));
    return (b >> 63) ? ~b : (b | kZeroKey);
}
__device__ __forceinline__ double rank_unkey(u64 k) { return __longlong_as_double(static_cast<long long>((k >> 63) ? (k & ~kZeroKey) : ~k)); }

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// keys[p] = the image of gval[p]; grp[p] = the group of its cell
__global__ __launch_bounds__(256) void rank_keys_kernel(const double *__restrict__ gval, const int *__restrict__ gcell,
                                                        const int *__restrict__ label, long long nnz, u64 *__restrict__ keys,
                                                        int *__restrict__ grp) {
    const long long p = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= nnz) return;
    keys[p] = rank_key(gval[p]);
    grp[p] = label[gcell[p]];
}

// the run [lo, hi) of equal keys around p within [gs, ge)
__device__ __forceinline__ void run_of(const u64 *__restrict__ keys, long long gs, long long ge, long long p, u64 k, long long &lo, long long &hi) {
    long long a = gs, b = p;
    while (a < b) { const long long mid = (a + b) >> 1; if (keys[mid] < k) a = mid + 1; else b = mid; }
    lo = a;
    a = p + 1; b = ge;
    while (a < b) { const long long mid = (a + b) >> 1; if (keys[mid] <= k) a = mid + 1; else b = mid; }
    hi = a;
}

// One wave (a workgroup of 64) per chunk of the sorted gene-major list.  LDS (dynamic, 32 G bytes): sum, sum of squares, 2R, count, zeros
// per group.  psum / psq: nch x G, the chunk's sums per group.  key2 (or null): (run start within the gene << 10) | group.
__global__ __launch_bounds__(64) void rank_stats_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr,
                                                        const int *__restrict__ chgene, const u64 *__restrict__ keys,
                                                        const int *__restrict__ grp, long long n, int G, int m, u64 *__restrict__ R2,
                                                        u32 *__restrict__ CNT, u32 *__restrict__ ZC, u64 *__restrict__ TIE,
                                                        u32 *__restrict__ NEG, u32 *__restrict__ ZS, double *__restrict__ psum,
                                                        double *__restrict__ psq, u32 *__restrict__ key2) {
    extern __shared__ double rank_lds[];
    double *lsum = rank_lds, *lsq = rank_lds + G;
    u64 *lr2 = reinterpret_cast<u64 *>(rank_lds + 2 * G);
    u32 *lcnt = reinterpret_cast<u32 *>(rank_lds + 3 * G), *lz = lcnt + G;
    const long long ch = blockIdx.x;
    const int lane = threadIdx.x;
    const int j = chgene[ch];
    long long b, e;
    chunk_range(gptr, chptr, j, ch, b, e);
    const long long gs = gptr[j], ge = gptr[j + 1];
    const long long n0 = n - (ge - gs);                      // the implicit zeros
    for (int g = lane; g < G; g += 64) { lsum[g] = 0.0; lsq[g] = 0.0; lr2[g] = 0ull; lcnt[g] = 0u; lz[g] = 0u; }
    __syncthreads();
    u64 tie = 0ull;
    u32 neg = 0u, zs = 0u;
    for (long long base = b; base < e; base += 64) {
        const long long p = base + lane;
        const bool valid = p < e;
        u64 k = kZeroKey, r2 = 0ull;
        int g = 0;
        if (valid) {
            k = keys[p];
            g = grp[p];
            long long lo, hi;
            run_of(keys, gs, ge, p, k, lo, hi);
            const long long lr = lo - gs, hr = hi - gs;
            r2 = static_cast<u64>(k > kZeroKey ? lr + hr + 1 + 2 * n0 : (k == kZeroKey ? lr + hr + n0 + 1 : lr + hr + 1));
            if (lo == p && k != kZeroKey) { const long long t = hi - lo; tie += static_cast<u64>(t * t * t - t); }
            neg += k < kZeroKey ? 1u : 0u;
            zs += k == kZeroKey ? 1u : 0u;
            if (key2) key2[p] = (static_cast<u32>(lr) << kRankGroupBits) | static_cast<u32>(g);
        }
        const double v = valid ? rank_unkey(k) : 0.0;
        const bool zero = valid && k == kZeroKey;
        bool todo = valid;
        for (;;) {
            const u64 mask = __ballot(todo);
            if (!mask) break;
            const int g0 = __shfl(g, __ffsll(static_cast<long long>(mask)) - 1);
            const bool mine = todo && g == g0;
            const double s = wave_sum(mine ? v : 0.0), q = wave_sum(mine ? v * v : 0.0);
            const u64 r = wave_sum_u64(mine ? r2 : 0ull);
            const u32 c = static_cast<u32>(__popcll(__ballot(mine))), z = static_cast<u32>(__popcll(__ballot(mine && zero)));
            if (lane == 0) { lsum[g0] += s; lsq[g0] += q; lr2[g0] += r; lcnt[g0] += c; lz[g0] += z; }
            todo = todo && !mine;
        }
    }
    __syncthreads();
    for (int g = lane; g < G; g += 64) {
        psum[ch * G + g] = lsum[g];
        psq[ch * G + g] = lsq[g];
        const size_t at = static_cast<size_t>(g) * m + j;
        if (lcnt[g]) { atomicAdd(&R2[at], lr2[g]); atomicAdd(&CNT[at], lcnt[g]); }
        if (lz[g]) atomicAdd(&ZC[at], lz[g]);
    }
    tie = wave_sum_u64(tie);
    const u64 nz = wave_sum_u64((static_cast<u64>(neg) << 32) | zs);
    if (lane == 0) {
        if (tie) atomicAdd(&TIE[j], tie);
        if (nz >> 32) atomicAdd(&NEG[j], static_cast<u32>(nz >> 32));
        if (nz & 0xffffffffull) atomicAdd(&ZS[j], static_cast<u32>(nz & 0xffffffffull));
    }
}

// S[g, j], Q[g, j] = the gene's chunks folded in chunk order; one thread per (group, gene)
__global__ __launch_bounds__(256) void rank_fold_kernel(const long long *__restrict__ chptr, int G, int m, const double *__restrict__ psum,
                                                        const double *__restrict__ psq, double *__restrict__ S, double *__restrict__ Q) {
    const long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= static_cast<long long>(G) * m) return;
    const int g = static_cast<int>(idx / m), j = static_cast<int>(idx % m);
    double s = 0.0, q = 0.0;
    for (long long ch = chptr[j]; ch < chptr[j + 1]; ++ch) { s += psum[ch * G + g]; q += psq[ch * G + g]; }
    S[idx] = s;
    Q[idx] = q;
}

// per gene, over the groups in their order: the sums of S, Q and of the non-zero counts
__global__ __launch_bounds__(256) void rank_totals_kernel(int G, int m, const double *__restrict__ S, const double *__restrict__ Q,
                                                          const u32 *__restrict__ CNT, const u32 *__restrict__ ZC, double *__restrict__ TS,
                                                          double *__restrict__ TQ, long long *__restrict__ TNZ) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double s = 0.0, q = 0.0;
    long long c = 0;
    for (int g = 0; g < G; ++g) {
        const size_t at = static_cast<size_t>(g) * m + j;
        s += S[at];
        q += Q[at];
        c += static_cast<long long>(CNT[at]) - ZC[at];
    }
    TS[j] = s;
    TQ[j] = q;
    TNZ[j] = c;
}

// flag[p] = 1 where the (run, group) key belongs to the reference; flag[nnz] = 0 closes the scan
__global__ __launch_bounds__(256) void rank_flag_kernel(const u32 *__restrict__ key2, long long nnz, int ref, u32 *__restrict__ flag) {
    const long long p = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (p > nnz) return;
    flag[p] = p < nnz && static_cast<int>(key2[p] & (kRankMaxGroups - 1)) == ref ? 1u : 0u;
}

// One wave per chunk of the list sorted by (run, group); keys: the value images in the first sort's order (a run's positions are the
// same in both).  P: the exclusive scan of the reference flags over the whole list (nnz + 1 values).
__global__ __launch_bounds__(256) void rank_ref_kernel(const long long *__restrict__ gptr, const long long *__restrict__ chptr,
                                                       const int *__restrict__ chgene, long long nch, const u64 *__restrict__ keys,
                                                       const u32 *__restrict__ key2, const u32 *__restrict__ P, int m, int ref,
                                                       long long n_ref, const u32 *__restrict__ CNT, u64 *__restrict__ U2,
                                                       u64 *__restrict__ TIEP, u64 *__restrict__ BASE, u32 *__restrict__ NEGR) {
    const long long ch = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (ch >= nch) return;
    const int lane = threadIdx.x & 63;
    const int j = chgene[ch];
    long long b, e;
    chunk_range(gptr, chptr, j, ch, b, e);
    const long long gs = gptr[j], ge = gptr[j + 1];
    const long long zr = n_ref - CNT[static_cast<size_t>(ref) * m + j];          // the reference's implicit zeros
    for (long long p = b + lane; p < e; p += 64) {
        const u32 k = key2[p];
        if (p > gs && key2[p - 1] == k) continue;            // not the head of its (run, group) sub-run
        const int g = static_cast<int>(k & (kRankMaxGroups - 1));
        const u32 run = k >> kRankGroupBits;
        long long a = p + 1, c = ge;                         // the first entry of another group or run
        while (a < c) { const long long mid = (a + c) >> 1; if (key2[mid] <= k) a = mid + 1; else c = mid; }
        const long long tg = a - p;
        const long long lo = gs + run;
        c = ge;                                              // the first entry of a later run (a is within or at the end of this one)
        while (a < c) { const long long mid = (a + c) >> 1; if ((key2[mid] >> kRankGroupBits) <= run) a = mid + 1; else c = mid; }
        const long long hi = a;
        const long long tr = static_cast<long long>(P[hi]) - P[lo], below = static_cast<long long>(P[lo]) - P[gs];
        const u64 vk = keys[lo];
        if (g == ref) {
            if (vk != kZeroKey) atomicAdd(&BASE[j], static_cast<u64>(tg * tg * tg - tg));
            if (vk < kZeroKey) atomicAdd(&NEGR[j], static_cast<u32>(tg));
            continue;
        }
        const long long below_all = vk > kZeroKey ? below + zr : below, tied = vk == kZeroKey ? tr + zr : tr;
        const size_t at = static_cast<size_t>(g) * m + j;
        atomicAdd(&U2[at], static_cast<u64>(tg * (2 * below_all + tied)));
        if (vk != kZeroKey) {
            const long long t = tg + tr;
            atomicAdd(&TIEP[at], static_cast<u64>((t * t * t - t) - (tr * tr * tr - tr)));
        }
    }
}

struct RankDev {                                             // what the kernels above leave, all zero-filled before
    DevBuf<u64> R2, TIE, U2, TIEP, BASE;
    DevBuf<u32> CNT, ZC, NEG, ZS, NEGR;
    DevBuf<double> S, Q, TS, TQ;
    DevBuf<long long> TNZ, sizes;
};

struct RankTables {                                          // finalize's outputs, G x m each
    DevBuf<long long> rank2, ties, nzc;
    DevBuf<double> score, pval, lfc, auc, mean, mean_ref, pct, pct_ref, df;
};

struct RankPtrs {
    const long long *gptr, *sizes, *TNZ;
    const u64 *R2, *TIE, *U2, *TIEP, *BASE;
    const u32 *CNT, *ZC, *NEG, *ZS, *NEGR;
    const double *S, *Q, *TS, *TQ;
    long long *rank2, *ties, *nzc;
    double *score, *pval, *lfc, *auc, *mean, *mean_ref, *pct, *pct_ref, *df;
};

__device__ __forceinline__ double rank_variance(double q, double s, double cnt) {
    const double mean = s / cnt;
    const double ss = q - cnt * (mean * mean);
    return (ss > 0.0 ? ss : 0.0) / (cnt - 1.0);
}

// One thread per (group, gene).  The reference's own row: NaN, and the integer tables are left alone.
__global__ __launch_bounds__(256) void rank_finalize_kernel(RankPtrs a, long long n, int G, int m, int ref, int method, int lg, int tie_correct,
                                                            int continuity) {
    const long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= static_cast<long long>(G) * m) return;
    const int g = static_cast<int>(idx / m), j = static_cast<int>(idx % m);
    if (g == ref) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        a.score[idx] = nan; a.pval[idx] = nan; a.lfc[idx] = nan; a.auc[idx] = nan; a.mean[idx] = nan; a.mean_ref[idx] = nan;
        a.pct[idx] = nan; a.pct_ref[idx] = nan; a.df[idx] = nan;
        return;
    }
    const long long ng = a.sizes[g], cnt = a.CNT[idx], zc = a.ZC[idx], nzc = cnt - zc;
    long long nr, N, r2, tie, u2, nzr;
    double sr, qr;
    if (ref < 0) {
        nr = n - ng;
        N = n;
        const long long t0 = n - (a.gptr[j + 1] - a.gptr[j]) + a.ZS[j];          // the zeros, implicit and stored
        r2 = static_cast<long long>(a.R2[idx]) + (ng - cnt) * (2ll * a.NEG[j] + t0 + 1);
        tie = static_cast<long long>(a.TIE[j]) + (t0 * t0 * t0 - t0);
        u2 = r2 - ng * (ng + 1);
        sr = a.TS[j] - a.S[idx];
        qr = a.TQ[j] - a.Q[idx];
        nzr = a.TNZ[j] - nzc;
    } else {
        const size_t ri = static_cast<size_t>(ref) * m + j;
        nr = a.sizes[ref];
        N = ng + nr;
        const long long zri = nr - a.CNT[ri], zsr = a.ZC[ri], zg = ng - cnt;
        u2 = static_cast<long long>(a.U2[idx]) + zg * (2ll * a.NEGR[j] + zri + zsr);
        const long long tz = zg + zc + zri + zsr;
        tie = static_cast<long long>(a.TIEP[idx] + a.BASE[j]) + (tz * tz * tz - tz);
        r2 = u2 + ng * (ng + 1);
        sr = a.S[ri];
        qr = a.Q[ri];
        nzr = static_cast<long long>(a.CNT[ri]) - zsr;
    }
    a.rank2[idx] = r2;
    a.ties[idx] = tie;
    a.nzc[idx] = nzc;
    const double dn = static_cast<double>(ng), dr = static_cast<double>(nr), dN = static_cast<double>(N);
    const double sg = a.S[idx], qg = a.Q[idx];
    const double mg = sg / dn, mr = sr / dr;
    a.auc[idx] = static_cast<double>(u2) / (2.0 * (dn * dr));
    a.mean[idx] = mg;
    a.mean_ref[idx] = mr;
    a.pct[idx] = static_cast<double>(nzc) / dn;
    a.pct_ref[idx] = static_cast<double>(nzr) / dr;
    a.lfc[idx] = lg ? log2((expm1(mg) + 1e-9) / (expm1(mr) + 1e-9)) : log2((mg + 1e-9) / (mr + 1e-9));
    if (method == 0) {
        const long long n3 = N * N * N - N;
        const double T = tie_correct ? static_cast<double>(n3 - tie) / static_cast<double>(n3) : 1.0;
        const double sig2 = ((dn * dr) * (dN + 1.0) / 12.0) * T;
        const long long d2 = u2 - ng * nr;                   // 2 (U - n_g n_ref / 2)
        double d = 0.5 * static_cast<double>(d2);
        if (continuity) d -= d2 > 0 ? 0.5 : (d2 < 0 ? -0.5 : 0.0);
        double z = 0.0, p = 1.0;
        if (sig2 > 0.0) {
            z = d / sqrt(sig2);
            p = erfc(fabs(z) * 0.70710678118654752440);
        }
        a.score[idx] = z;
        a.pval[idx] = p;
        a.df[idx] = 0.0;
    } else {
        const double vg = rank_variance(qg, sg, dn) / dn, vr = rank_variance(qr, sr, dr) / dr;
        double t = 0.0, df = 0.0;
        if (vg + vr > 0.0) {
            t = (mg - mr) / sqrt(vg + vr);
            df = ((vg + vr) * (vg + vr)) / (vg * vg / (dn - 1.0) + vr * vr / (dr - 1.0));
        }
        a.score[idx] = t;
        a.pval[idx] = 1.0;                                   // (the host fills it in from t and df)
        a.df[idx] = df;
    }
}

// keys[idx] = an image of the score whose ascending order is the score's descending one, NaN last; src[idx] = idx
__global__ __launch_bounds__(256) void rank_order_keys_kernel(const double *__restrict__ score, long long cnt, u64 *__restrict__ keys,
                                                              u32 *__restrict__ src) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= cnt) return;
    const double s = score[i];
    keys[i] = s != s ? ~0ull : ~rank_key(s);
    src[i] = static_cast<u32>(i);
}
__global__ __launch_bounds__(256) void rank_order_group_kernel(const u32 *__restrict__ src, long long cnt, int m, u32 *__restrict__ gkey) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < cnt) gkey[i] = src[i] / static_cast<u32>(m);
}
__global__ __launch_bounds__(256) void rank_order_take_kernel(const u32 *__restrict__ src, int G, int m, int n_order, long long *__restrict__ order) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= static_cast<long long>(G) * n_order) return;
    const long long g = i / n_order, r = i % n_order;
    order[i] = src[g * m + r] % static_cast<u32>(m);
}

// the checks that need no device; returns the cells in all and fills the sizes
long long rank_check(const std::string &w, const ExprBlocks &B, const int *labels, const RankOptions &o, const int *genes, int n_genes,
                     double normalize_total, std::vector<long long> &sizes, int &mk) {
    SHARP_REQUIRE(labels, w + ": null labels");
    SHARP_REQUIRE(o.G >= 2, w + ": need at least 2 groups");
    SHARP_REQUIRE(o.G <= kRankMaxGroups, w + ": at most 1024 groups are supported");
    SHARP_REQUIRE(o.method == 0 || o.method == 1, w + ": method must be 0 (wilcoxon) or 1 (t-test)");
    SHARP_REQUIRE(o.reference >= -1 && o.reference < o.G, w + ": reference must be -1 (rest) or one of the groups");
    expr_check_options(w, normalize_total, B.m);
    const long long n = expr_total_cells(w, B);
    SHARP_REQUIRE(n <= kRankMaxCells, w + ": need at most 2097151 cells in all");
    mk = expr_check_genes(w, genes, n_genes, B.m);
    SHARP_REQUIRE(static_cast<long long>(o.G) * mk < (1ll << 32), w + ": groups x genes must stay below 2^32");
    sizes.assign(o.G, 0);
    for (long long i = 0; i < n; ++i) {
        SHARP_REQUIRE(labels[i] >= 0 && labels[i] < o.G, w + ": labels must be codes in 0 .. n_groups - 1 (cell " + std::to_string(i) + ", counted from 0)");
        ++sizes[labels[i]];
    }
    for (int g = 0; g < o.G; ++g) SHARP_REQUIRE(sizes[g] > 0, w + ": group " + std::to_string(g) + " (counted from 0) has no cell");
    if (o.method == 1)
        for (int g = 0; g < o.G; ++g) {
            const long long other = o.reference < 0 ? n - sizes[g] : sizes[o.reference];
            SHARP_REQUIRE(sizes[g] >= 2 && other >= 2, w + ": t-test needs at least 2 cells in every tested group and in what it is tested against (group " +
                                                           std::to_string(g) + ", counted from 0)");
        }
    return n;
}

// load .. finalize: the tables on the device
void rank_tables(const std::string &w, const ExprBlocks &B, const int *labels, const RankOptions &o, const int *genes, int n_genes,
                 double normalize_total, const std::vector<long long> &sizes, ExprData &D, RankTables &T) {
    Ctx &c = ctx();
    ExprExtra extra;
    extra.genes = genes;
    extra.n_genes = n_genes;
    expr_load(w, B, normalize_total, o.log1p, true, false, 0, 2, D, extra);
    const int m = D.m, G = o.G;
    const long long n = D.n, nnz = D.nnz, nch = D.nch;
    SHARP_REQUIRE(nnz < (1ll << 32) - 1, w + ": more than 2^32 - 2 stored entries (the segmented sort's index type)");
    const size_t gm = static_cast<size_t>(G) * m, ne = static_cast<size_t>(std::max<long long>(nnz, 1));
    RankDev R;
    R.sizes.alloc(G);
    R.sizes.upload(sizes.data(), G);
    R.R2.alloc(gm); R.CNT.alloc(gm); R.ZC.alloc(gm); R.S.alloc(gm); R.Q.alloc(gm);
    R.TIE.alloc(m); R.NEG.alloc(m); R.ZS.alloc(m); R.TS.alloc(m); R.TQ.alloc(m); R.TNZ.alloc(m);
    R.R2.zero(); R.CNT.zero(); R.ZC.zero(); R.TIE.zero(); R.NEG.zero(); R.ZS.zero();
    const bool pair = o.reference >= 0;
    if (pair) {
        R.U2.alloc(gm); R.TIEP.alloc(gm); R.BASE.alloc(m); R.NEGR.alloc(m);
        R.U2.zero(); R.TIEP.zero(); R.BASE.zero(); R.NEGR.zero();
    }
    DevBuf<u64> keys(ne), keys_s(ne);
    DevBuf<u32> key2, key2_s;
    DevBuf<int> grp_s(ne);
    {
        KernelTimer timer("rank_genes_order");
        DevBuf<int> dlab(std::max<long long>(n, 1)), grp(ne);
        dlab.upload(labels, n);
        if (nnz) {
            hipLaunchKernelGGL(rank_keys_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, c.stream, D.gval.p, D.gcell.p, dlab.p, nnz, keys.p, grp.p);
            launch_check("rank_keys_kernel");
            Scratch tmp;
            with_scratch(tmp, false, [&](void *p, size_t &bytes) {
                return rocprim::segmented_radix_sort_pairs(p, bytes, keys.p, keys_s.p, grp.p, grp_s.p, static_cast<unsigned int>(nnz),
                                                           static_cast<unsigned int>(m), D.gptr.p, D.gptr.p + 1, 0, 64, c.stream);
            });
        }
        stream_sync();                                       // (the labels, grp and the scratch leave scope)
    }
    if (pair) { key2.alloc(ne); key2_s.alloc(ne); }
    {
        KernelTimer timer("rank_genes_stats");
        DevBuf<double> psum(std::max<long long>(nch, 1) * G), psq(std::max<long long>(nch, 1) * G);
        if (nch) {
            hipLaunchKernelGGL(rank_stats_kernel, dim3(static_cast<unsigned>(nch)), dim3(64), static_cast<size_t>(G) * 32, c.stream, D.gptr.p,
                               D.chptr.p, D.chgene.p, keys_s.p, grp_s.p, n, G, m, R.R2.p, R.CNT.p, R.ZC.p, R.TIE.p, R.NEG.p, R.ZS.p, psum.p,
                               psq.p, pair ? key2.p : nullptr);
            launch_check("rank_stats_kernel");
        }
        hipLaunchKernelGGL(rank_fold_kernel, dim3(grid_for(static_cast<long long>(gm), 256)), dim3(256), 0, c.stream, D.chptr.p, G, m, psum.p,
                           psq.p, R.S.p, R.Q.p);
        hipLaunchKernelGGL(rank_totals_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c.stream, G, m, R.S.p, R.Q.p, R.CNT.p, R.ZC.p, R.TS.p,
                           R.TQ.p, R.TNZ.p);
        launch_check("rank_totals_kernel");
        stream_sync();                                       // (the chunks' sums leave scope)
    }
    if (pair && nnz) {
        KernelTimer timer("rank_genes_ref");
        DevBuf<u32> flag(ne + 1), P(ne + 1);
        Scratch tmp;
        with_scratch(tmp, false, [&](void *p, size_t &bytes) {
            return rocprim::segmented_radix_sort_keys(p, bytes, key2.p, key2_s.p, static_cast<unsigned int>(nnz), static_cast<unsigned int>(m),
                                                      D.gptr.p, D.gptr.p + 1, 0, 32, c.stream);
        });
        hipLaunchKernelGGL(rank_flag_kernel, dim3(grid_for(nnz + 1, 256)), dim3(256), 0, c.stream, key2_s.p, nnz, o.reference, flag.p);
        exclusive_scan(flag.p, P.p, static_cast<size_t>(nnz + 1), tmp);
        hipLaunchKernelGGL(rank_ref_kernel, dim3(wave_grid(nch)), dim3(256), 0, c.stream, D.gptr.p, D.chptr.p, D.chgene.p, nch, keys_s.p, key2_s.p,
                           P.p, m, o.reference, sizes[o.reference], R.CNT.p, R.U2.p, R.TIEP.p, R.BASE.p, R.NEGR.p);
        launch_check("rank_ref_kernel");
        stream_sync();                                       // (the temporaries leave scope)
    }
    T.rank2.alloc(gm); T.ties.alloc(gm); T.nzc.alloc(gm);
    T.score.alloc(gm); T.pval.alloc(gm); T.lfc.alloc(gm); T.auc.alloc(gm); T.mean.alloc(gm); T.mean_ref.alloc(gm); T.pct.alloc(gm);
    T.pct_ref.alloc(gm); T.df.alloc(gm);
    RankPtrs a{D.gptr.p, R.sizes.p, R.TNZ.p, R.R2.p, R.TIE.p, R.U2.p, R.TIEP.p, R.BASE.p, R.CNT.p, R.ZC.p, R.NEG.p, R.ZS.p, R.NEGR.p,
               R.S.p, R.Q.p, R.TS.p, R.TQ.p, T.rank2.p, T.ties.p, T.nzc.p, T.score.p, T.pval.p, T.lfc.p, T.auc.p, T.mean.p, T.mean_ref.p,
               T.pct.p, T.pct_ref.p, T.df.p};
    hipLaunchKernelGGL(rank_finalize_kernel, dim3(grid_for(static_cast<long long>(gm), 256)), dim3(256), 0, c.stream, a, n, G, m, o.reference,
                       o.method, o.log1p ? 1 : 0, o.tie_correct ? 1 : 0, o.continuity ? 1 : 0);
    launch_check("rank_finalize_kernel");
    stream_sync();                                           // (R leaves scope)
}

// order (G x n_order, host) from the scores on the device
void rank_order(const double *score, int G, int m, int n_order, long long *order) {
    Ctx &c = ctx();
    KernelTimer timer("rank_genes_sort");
    const long long cnt = static_cast<long long>(G) * m;
    DevBuf<u64> keys(cnt), keys_s(cnt);
    DevBuf<u32> src(cnt), src_s(cnt), gkey(cnt), gkey_s(cnt);
    DevBuf<long long> out(static_cast<size_t>(G) * n_order);
    Scratch tmp;
    hipLaunchKernelGGL(rank_order_keys_kernel, dim3(grid_for(cnt, 256)), dim3(256), 0, c.stream, score, cnt, keys.p, src.p);
    launch_check("rank_order_keys_kernel");
    sort_pairs(keys.p, keys_s.p, src.p, src_s.p, static_cast<size_t>(cnt), 0, 64, tmp);                    // stable: ties stay by gene
    hipLaunchKernelGGL(rank_order_group_kernel, dim3(grid_for(cnt, 256)), dim3(256), 0, c.stream, src_s.p, cnt, m, gkey.p);
    sort_pairs(gkey.p, gkey_s.p, src_s.p, src.p, static_cast<size_t>(cnt), 0, key_bits(static_cast<u64>(G - 1)), tmp);   // stable again
    hipLaunchKernelGGL(rank_order_take_kernel, dim3(grid_for(static_cast<long long>(G) * n_order, 256)), dim3(256), 0, c.stream, src.p, G, m,
                       n_order, out.p);
    launch_check("rank_order_take_kernel");
    out.download(order, static_cast<size_t>(G) * n_order);   // (synchronises: the temporaries leave scope)
}

// Benjamini-Hochberg over one group's m p-values (NaN rows stay NaN)
void rank_bh(const double *p, int m, double *adj) {
    if (p[0] != p[0]) { std::fill(adj, adj + m, std::numeric_limits<double>::quiet_NaN()); return; }
    std::vector<int> idx(m);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return p[x] < p[y]; });
    double run = 1.0;
    for (int r = m - 1; r >= 0; --r) {
        const double v = p[idx[r]] * (static_cast<double>(m) / static_cast<double>(r + 1));
        run = std::min(run, v);
        adj[idx[r]] = run;
    }
}

}  // namespace

// I_x(a, b) by the continued fraction of the incomplete beta function (modified Lentz), on the side where it converges fast
static double betacf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int it = 1; it <= 100000; ++it) {
        const double m2 = 2.0 * it;
        double aa = it * (b - it) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + it) * (qab + it) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) <= eps) break;
    }
    return h;
}

// the regularised incomplete beta function I_x(a, b); y = 1 - x as the caller knows it, so that an x next to 1 loses nothing
static double rank_betainc(double a, double b, double x, double y) {
    if (!(x > 0.0)) return 0.0;
    if (!(y > 0.0)) return 1.0;
    const double lbt = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log(y);
    if (x < (a + 1.0) / (a + b + 2.0)) return std::exp(lbt) * betacf(a, b, x) / a;
    return 1.0 - std::exp(lbt) * betacf(b, a, y) / b;
}

// the two-sided p-value of Student's t with df degrees of freedom: I_x(df / 2, 1 / 2) at x = df / (df + t^2), with 1 - x = t^2 / (df + t^2)
// formed directly (a small t leaves no digits of it in x)
static double t_two_sided(double t, double df) {
    const double t2 = t * t;
    return rank_betainc(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2));
}

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_rank_genes_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                         const int *labels, int n_groups, int method, int reference, double normalize_total, int log1p, const int *genes,
                         int n_genes, int tie_correct, int continuity, int n_order, long long *group_sizes, double *scores, double *pvals,
                         double *pvals_adj, double *logfoldchanges, double *auc, double *means, double *means_ref, double *pct,
                         double *pct_ref, long long *order) {
    SHARP_API_BEGIN
    const std::string w("rank_genes_groups");
    SHARP_REQUIRE(group_sizes && scores && pvals && pvals_adj && logfoldchanges && auc && means && means_ref && pct && pct_ref && order,
                  w + ": null output");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    RankOptions o;
    o.G = n_groups; o.method = method; o.reference = reference;
    o.log1p = log1p != 0; o.tie_correct = tie_correct != 0; o.continuity = continuity != 0;
    std::vector<long long> sizes;
    int mk = 0;
    rank_check(w, B, labels, o, genes, n_genes, normalize_total, sizes, mk);
    SHARP_REQUIRE(n_order >= 1 && n_order <= mk, w + ": n_genes of the ordered lists must lie in 1 .. the kept genes");
    ctx();
    ExprData D;
    RankTables T;
    rank_tables(w, B, labels, o, genes, n_genes, normalize_total, sizes, D, T);
    const size_t gm = static_cast<size_t>(n_groups) * mk;
    std::copy(sizes.begin(), sizes.end(), group_sizes);
    T.score.download(scores, gm);
    T.pval.download(pvals, gm);
    T.lfc.download(logfoldchanges, gm);
    T.auc.download(auc, gm);
    T.mean.download(means, gm);
    T.mean_ref.download(means_ref, gm);
    T.pct.download(pct, gm);
    T.pct_ref.download(pct_ref, gm);
    if (method == 1) {
        std::vector<double> df(gm);
        T.df.download(df.data(), gm);
        for (size_t i = 0; i < gm; ++i) {
            if (scores[i] != scores[i]) continue;            // the reference's row
            pvals[i] = df[i] > 0.0 ? t_two_sided(scores[i], df[i]) : 1.0;
        }
    }
    for (int g = 0; g < n_groups; ++g) rank_bh(pvals + static_cast<size_t>(g) * mk, mk, pvals_adj + static_cast<size_t>(g) * mk);
    rank_order(T.score.p, n_groups, mk, n_order, order);
    SHARP_API_END
}

int sharp_rank_sums_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                        const int *labels, int n_groups, int reference, double normalize_total, int log1p, const int *genes, int n_genes,
                        long long *rank2, long long *ties, long long *nnz_counts) {
    SHARP_API_BEGIN
    const std::string w("rank_sums");
    SHARP_REQUIRE(rank2 && ties && nnz_counts, w + ": null output");
    const ExprBlocks B{colptr, rowidx, val, ncb, nblocks, m};
    RankOptions o;
    o.G = n_groups; o.reference = reference; o.log1p = log1p != 0;
    std::vector<long long> sizes;
    int mk = 0;
    rank_check(w, B, labels, o, genes, n_genes, normalize_total, sizes, mk);
    ctx();
    ExprData D;
    RankTables T;
    rank_tables(w, B, labels, o, genes, n_genes, normalize_total, sizes, D, T);
    const size_t gm = static_cast<size_t>(n_groups) * mk;
    std::vector<long long> r(gm), t(gm);
    T.rank2.download(r.data(), gm);
    T.ties.download(t.data(), gm);
    for (int g = 0; g < n_groups; ++g) {
        if (g == reference) continue;                        // (finalize left this row alone)
        std::copy(r.begin() + static_cast<size_t>(g) * mk, r.begin() + static_cast<size_t>(g + 1) * mk, rank2 + static_cast<size_t>(g) * mk);
        if (reference >= 0) std::copy(t.begin() + static_cast<size_t>(g) * mk, t.begin() + static_cast<size_t>(g + 1) * mk, ties + static_cast<size_t>(g) * mk);
    }
    if (reference < 0) std::copy(t.begin(), t.begin() + mk, ties);
    T.nzc.download(r.data(), gm);
    for (int g = 0; g < n_groups; ++g) {
        if (g == reference) continue;
        std::copy(r.begin() + static_cast<size_t>(g) * mk, r.begin() + static_cast<size_t>(g + 1) * mk, nnz_counts + static_cast<size_t>(g) * mk);
    }
    SHARP_API_END
}

}  // extern "C"
