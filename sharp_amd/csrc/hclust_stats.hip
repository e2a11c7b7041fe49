// hclust_stats.hip -- a5 of the batched get_opt_hclust (hclust.hip): cutree for k = min..max, the median silhouette and get_CH("1-corr")
// of every level (R/get_opt_hclust.R:90-187), and, at the end of the file, the launchers that hclust.hip's chunk pipeline calls.
// Third-party algorithms restated (not vendored by the reference): cutree's first-appearance numbering, cluster::silhouette,
// clues::get_CH per SURVEY.md App. A.4-A.6.
#include "hclust_task.hpp"

#include <algorithm>
#include <vector>

#include "linalg.hpp"

namespace sharp {

// ---------------------------------------------------------------------------------------------
// a5a: cutree for every level k = kmin..kmax (level index L = k - kmin), ids by first appearance.
// j2 is absorbed by i2 < j2 at its merge step, so a cluster's representative is its smallest member
// and "first appearance" order is the order of the representatives.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HC_THREADS) void cutree_kernel(const HcMeta *__restrict__ metas, const int *__restrict__ ia_all,
                                                            const int *__restrict__ ib_all, int *__restrict__ lab_all) {
    const HcMeta M = metas[blockIdx.x];
    const int n = M.n;
    const int *ia = ia_all + M.oM, *ib = ib_all + M.oM;
    int *lab = lab_all + M.oLab;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    unsigned char *lds_cursor = sm;
    CUTREE_ARRAYS(LDS_CARVE, n)                    // declares absorbed, wsum, parent, rank (hclust_task.hpp)
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += HC_THREADS) { absorbed[i] = 0x7fffffff; parent[i] = static_cast<uint16_t>(i); }
    __syncthreads();
    for (int s = tid; s < n - 1; s += HC_THREADS) { absorbed[ib[s] - 1] = s; parent[ib[s] - 1] = static_cast<uint16_t>(ia[s] - 1); }
    __syncthreads();
    const int chunk = (n + HC_THREADS - 1) / HC_THREADS;
    for (int L = 0; L < M.nk; ++L) {
        const int k = M.kmin + L;
        const int nm = n - k;                      // merges applied
        // exclusive prefix count of representatives -> 1-based id of each representative
        const int b0 = tid * chunk, b1 = min(n, b0 + chunk);
        int local = 0;
        for (int i = b0; i < b1; ++i) local += (absorbed[i] >= nm);
        int inc = local;
        const int lane = tid & 63, w = tid >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        if (tid == 0) { int run = 0; for (int q = 0; q < HC_THREADS / 64; ++q) { const int t = wsum[q]; wsum[q] = run; run += t; } }
        __syncthreads();
        int run = wsum[w] + inc - local;
        for (int i = b0; i < b1; ++i) { if (absorbed[i] >= nm) rank[i] = static_cast<uint16_t>(++run); }
        __syncthreads();
        for (int i = tid; i < n; i += HC_THREADS) {
            int r = i;
            while (absorbed[r] < nm) r = parent[r];
            lab[static_cast<long long>(L) * n + i] = rank[r];
        }
        __syncthreads();
    }
}

// one-hot membership of the finest level (k = kmax): H[i][c] = (label_i == c + 1)
__global__ void onehot_kernel(const HcMeta *__restrict__ metas, const int *__restrict__ lab_all, double *__restrict__ H_all) {
    const HcMeta M = metas[blockIdx.y];
    const int *lab = lab_all + M.oLab + static_cast<long long>(M.nk - 1) * M.n;
    double *H = H_all + M.oH;
    const long long tot = static_cast<long long>(M.n) * M.kpad;
    for (long long q = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; q < tot;
         q += static_cast<long long>(gridDim.x) * blockDim.x) {
        const int i = static_cast<int>(q / M.kpad), c = static_cast<int>(q % M.kpad);
        H[q] = (lab[i] == c + 1) ? 1.0 : 0.0;
    }
}

// The finest level's cluster sums WITHOUT the one-hot matrix and its skinny GEMM (48 clusters wide: 75 % of a 64-wide MFMA tile, a K
// loop of 2000 cells; 0.61 ms per chunk of 188 tasks, 0.43 as below, and the 0.04 ms one-hot pass goes too):
//   cluster_sums_kernel     CSt[j][c] = sum over the cells i of finest cluster c of Cr[i][j]   (p x kpad), one workgroup per (64
//                           columns, task): a wave walks every SS_WAVES-th row, adds its 64 entries to the cluster's row of the
//                           wave's LDS table (the label is wave-uniform), the tables are added in wave order at the end.
// It sums in a fixed order (rows ascending per wave, waves in order): the same bits every run.  (The rows' products with the sums,
// G = CS C^T, stay on the MFMA: one thread per cell with the 48 sums of a row j through the scalar cache took 0.77 ms against 0.50.)
__global__ __launch_bounds__(64 * SS_WAVES) void cluster_sums_kernel(const HcMeta *__restrict__ metas, const int *__restrict__ lab_all,
                                                                     const double *__restrict__ Cr_all, double *__restrict__ CSt_all) {
    const HcMeta M = metas[blockIdx.y];
    const int j0 = blockIdx.x * 64;
    if (j0 >= M.p) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_sm[];
    double *acc = reinterpret_cast<double *>(ss_sm);                       // [SS_WAVES][kpad][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kpad = M.kpad, n = M.n, p = M.p;
    for (int q = tid; q < SS_WAVES * kpad * 64; q += 64 * SS_WAVES) acc[q] = 0.0;
    __syncthreads();
    const int *lab = lab_all + M.oLab + static_cast<long long>(M.nk - 1) * n;
    const double *Cr = Cr_all + M.oCr;
    const int j = j0 + lane;
    const bool live = j < p;
    double *mine = acc + static_cast<size_t>(wave) * kpad * 64 + lane;
    int i = wave;
    for (; i + 3 * SS_WAVES < n; i += 4 * SS_WAVES) {                     // four rows' loads in flight
        double x[4];
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = __builtin_amdgcn_readfirstlane(lab[i + u * SS_WAVES]) - 1;
            x[u] = live ? Cr[static_cast<long long>(i + u * SS_WAVES) * p + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) mine[c[u] * 64] += x[u];
    }
    for (; i < n; i += SS_WAVES) {
        const int c = __builtin_amdgcn_readfirstlane(lab[i]) - 1;
        mine[c * 64] += live ? Cr[static_cast<long long>(i) * p + j] : 0.0;
    }
    __syncthreads();
    double *CSt = CSt_all + M.oCSt;
    for (int q = tid; q < kpad * 64; q += 64 * SS_WAVES) {
        const int c = q >> 6, l = q & 63;
        if (j0 + l >= p) continue;
        double v = acc[c * 64 + l];
#pragma unroll
        for (int w = 1; w < SS_WAVES; ++w) v += acc[(w * kpad + c) * 64 + l];
        CSt[static_cast<long long>(j0 + l) * kpad + c] = v;
    }
}

// copy the pristine distances of symmetric tasks (hclust updates D in place)
__global__ void copy_d_kernel(const HcMeta *__restrict__ metas, const double *__restrict__ Dall, double *__restrict__ D0all) {
    const HcMeta M = metas[blockIdx.y];
    if (M.symmetric != 1) return;
    const long long tot = static_cast<long long>(M.n) * M.nld;
    const double *D = Dall + M.oD;
    double *D0 = D0all + M.oD0;
    for (long long q = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; q < tot;
         q += static_cast<long long>(gridDim.x) * blockDim.x)
        D0[q] = D[q];
}

// ---------------------------------------------------------------------------------------------
// a5b: per (task, level): median silhouette (cluster::silhouette semantics) and CH ("1-corr").
// Everything is derived from finest-level quantities computed by MFMA GEMMs:
//   T[i][f] = sum_{j in f} d(i,j)   (symmetric tasks: D0 * H;  feature tasks: cnt_f - G[i][f])
//   G[i][f] = c_i . sum_{j in f} c_j,   Q[f][f'] = (sum_f c) . (sum_f' c)
// A level-k cluster is a union of finest clusters; its sums add the finest columns in ascending order.
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(ST_THREADS) void stats_kernel(const HcMeta *__restrict__ metas, const int *__restrict__ lab_all,
                                                           const double *__restrict__ T_all, const double *__restrict__ G_all,
                                                           const double *__restrict__ Q_all, const double *__restrict__ nrm_all,
                                                           double *__restrict__ out_all, int count, int max_nk, int kcap) {
    // One workgroup per (task, level).  The levels of a task all read the task's G (n x kpad): the linear workgroup id is
    // dealt so that the eight tasks of a group sit on the eight XCDs (workgroups go round-robin to XCDs) and G is
    // fetched into one L2 once instead of once per level (34 GB -> 0.3 GB of HBM reads per step).
    const long long B = blockIdx.x;
    const long long per_group = 8LL * max_nk;
    const int zt = static_cast<int>(B / per_group) * 8 + static_cast<int>(B % 8);
    if (zt >= count) return;
    const HcMeta M = metas[zt];
    const int L = static_cast<int>((B % per_group) / 8);
    if (L >= M.nk) return;
    const int n = M.n, k = M.kmin + L, kf = M.kmax, kpad = M.kpad;
    const int *lab = lab_all + M.oLab + static_cast<long long>(L) * n;
    const int *labF = lab_all + M.oLab + static_cast<long long>(M.nk - 1) * n;
    const double *T = T_all + M.oT, *G = G_all + M.oG, *Q = Q_all + M.oQ, *nrm = nrm_all + M.oNrm;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    int npow2 = 1; while (npow2 < n) npow2 <<= 1;
    double *sil = reinterpret_cast<double *>(sm);            // npow2
    double *part = sil + npow2;                              // ST_THREADS
    double *cn2 = part + ST_THREADS;                         // k  : |sum_c|^2
    double *ctot = cn2 + kcap;                               // k  : sum_c . total
    int *cnt = reinterpret_cast<int *>(ctot + kcap);         // k
    int *cntF = cnt + kcap;                                  // kf
    int *fm = cntF + kcap;                                   // kf : level cluster (0-based) of finest cluster f
    int *start = fm + kcap;                                  // k + 1
    int *order = start + kcap + 1;                           // kf : finest clusters grouped by level cluster
    const int tid = threadIdx.x;
    for (int c = tid; c < kcap; c += ST_THREADS) { cnt[c] = 0; cntF[c] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += ST_THREADS) {
        atomicAdd(&cnt[lab[i] - 1], 1);
        atomicAdd(&cntF[labF[i] - 1], 1);
        fm[labF[i] - 1] = lab[i] - 1;
    }
    __syncthreads();
    // finest clusters grouped by level cluster (ascending inside a group): counts, a prefix over k <= kf entries, one thread per group
    for (int c = tid; c <= k; c += ST_THREADS) start[c] = 0;
    __syncthreads();
    for (int f = tid; f < kf; f += ST_THREADS) atomicAdd(&start[fm[f] + 1], 1);
    __syncthreads();
    if (tid == 0) for (int c = 0; c < k; ++c) start[c + 1] += start[c];
    // the kf x kf Gram matrix of the finest clusters' sums goes through LDS (the space of sil[], written later): the sums below
    // re-read it up to (group size) x (group size + kf) times per group, which took 3 of the kernel's 4.5 ms as dependent global loads
    const bool q_lds = kf * kf <= npow2;
    if (q_lds) for (int e = tid; e < kf * kf; e += ST_THREADS) sil[e] = Q[static_cast<long long>(e / kf) * kpad + e % kf];
    __syncthreads();
    for (int c = tid; c < k; c += ST_THREADS) {
        int pos = start[c];
        for (int f = 0; f < kf; ++f) if (fm[f] == c) order[pos++] = f;
    }
    __syncthreads();
    double tot2 = 0.0;
    for (int c = tid; c < k; c += ST_THREADS) {
        double a = 0.0, b = 0.0;
        for (int q = start[c]; q < start[c + 1]; ++q) {
            if (q_lds) {
                const double *qr = sil + order[q] * kf;
                for (int q2 = start[c]; q2 < start[c + 1]; ++q2) a += qr[order[q2]];
                for (int f = 0; f < kf; ++f) b += qr[f];
            } else {
                const double *qr = Q + static_cast<long long>(order[q]) * kpad;
                for (int q2 = start[c]; q2 < start[c + 1]; ++q2) a += qr[order[q2]];
                for (int f = 0; f < kf; ++f) b += qr[f];
            }
        }
        cn2[c] = a; ctot[c] = b;
    }
    __syncthreads();
    for (int c = 0; c < k; ++c) tot2 += ctot[c];             // |total|^2 (every thread, same order)
    const bool tfromG = !M.symmetric;
    const int nld = M.nld;
    double wpart = 0.0;
    for (int i = tid; i < n; i += ST_THREADS) {
        const int own = lab[i] - 1;
        // T and G are stored transposed (kpad x nld): for a fixed finest cluster f the lanes read consecutive cells.
        // The kf finest clusters are walked in the order that groups them by level cluster, eight loads at a time.
        const double *Ti = T + i, *Gi = G + i;
        double a = 0.0, bmin = 0.0, gown = 0.0;
        bool have_b = false;
        int c = 0;
        while (c < k && start[c + 1] == start[c]) ++c;           // (levels never have empty clusters; defensive)
        double sc = 0.0, gc = 0.0;
        for (int q0 = 0; q0 < kf; q0 += 8) {
            double gv[8], tv[8];
            int fv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u < kf ? q0 + u : kf - 1;
                fv[u] = order[q];
                gv[u] = Gi[static_cast<long long>(fv[u]) * nld];
                tv[u] = tfromG ? 0.0 : Ti[static_cast<long long>(fv[u]) * nld];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u;
                if (q < kf) {
                    sc += tfromG ? (static_cast<double>(cntF[fv[u]]) - gv[u]) : tv[u];
                    gc += gv[u];
                    if (q + 1 == start[c + 1]) {                   // cluster c complete
                        if (c == own) { a = sc / static_cast<double>(cnt[c] - 1); gown = gc; }
                        else { const double bb = sc / static_cast<double>(cnt[c]); if (!have_b || bmin > bb) { bmin = bb; have_b = true; } }
                        sc = 0.0; gc = 0.0;
                        ++c;
                        while (c < k && start[c + 1] == start[c]) ++c;
                    }
                }
            }
        }
        double s = 0.0;
        if (cnt[own] > 1 && bmin != a) s = (bmin - a) / fmax(a, bmin);
        sil[i] = s;
        double r = gown / (nrm[i] * sqrt(cn2[own]));
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
        wpart += (1.0 - r) * (1.0 - r);
    }
    for (int i = n + tid; i < npow2; i += ST_THREADS) sil[i] = HC_INF;
    part[tid] = wpart;
    __syncthreads();
    // bitonic sort of sil[0..npow2)
    for (int size = 2; size <= npow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += ST_THREADS) {
                const int lo = ((t / stride) * stride * 2) + (t % stride);
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double x = sil[lo], y = sil[hi];
                if ((x > y) == up) { sil[lo] = y; sil[hi] = x; }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        double W = 0.0;
        for (int q = 0; q < ST_THREADS; ++q) W += part[q];
        double B = 0.0;
        for (int c = 0; c < k; ++c) {
            double r = ctot[c] / (sqrt(cn2[c]) * sqrt(tot2));
            r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
            B += static_cast<double>(cnt[c]) * (1.0 - r) * (1.0 - r);
        }
        const double ch = (B / static_cast<double>(k - 1)) / (W / static_cast<double>(n - k));
        const double med = (n & 1) ? sil[n / 2] : (sil[n / 2 - 1] + sil[n / 2]) / 2;
        double *out = out_all + M.oOut;
        out[L] = med;
        out[M.nk + L] = ch;
    }
}

#include "hclust_stats.inc"

// ---------------------------------------------------------------------------------------------
// a5b for MANY candidate levels (the cross-block sMetaC of a run of >= 1e6 cells tries k = n/50000 .. n/5000: 1801 levels at 1e7
// cells, R/sMetaC.R:110-119).  stats_kernel recomputes every level from the finest-level quantities, O(n kf) per level and a
// per-cluster O(size^2) Gram sum by one thread: 0.4 - 0.75 s for 2200 - 8000 rows.  Consecutive levels differ by ONE merge, so here the
// per-level cluster sums are carried from the finest level down:
//   ml_prep_kernel   (one workgroup per task, levels in sequence): |sum_c|^2 of the merged cluster (Gram matrix of the cluster sums
//                    updated in place), sum_c . total, the between-cluster term of CH;
//   ml_cells_kernel  (one wave per cell, all levels): the cell's sums of distances / products per cluster live in the wave's LDS and
//                    follow the merges; per level the silhouette width (own mean, minimum over the other clusters' means) and the
//                    within term of CH -> s[i][L], w[i][L];
//   ml_level_kernel  (one workgroup per level): median of s[.][L] (bitonic sort in LDS), sum of w[.][L] in a fixed order, CH.
// The merges (r1 <- r2 in finest-cluster ids, r1 < r2) come from the host (a replay of the merge list).  Sums of a merged cluster are
// (sum of r1) + (sum of r2): a different association than stats_kernel's from-scratch sums, equal to rounding.
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(1024) void ml_prep_kernel(const HcMeta *__restrict__ metas, const MlMeta *__restrict__ mls, const int *__restrict__ lab_all,
                                                       double *__restrict__ Q_all, const int *__restrict__ r1_all, const int *__restrict__ r2_all,
                                                       double *__restrict__ cn2m_all, double *__restrict__ B_all, int *__restrict__ cntF_all,
                                                       double *__restrict__ cn2F_all, double *__restrict__ tot2_all) {
    const HcMeta M = metas[blockIdx.x];
    const MlMeta X = mls[blockIdx.x];
    const int n = M.n, kf = M.kmax, kpad = M.kpad, nk = M.nk;
    const int *labF = lab_all + M.oLab + static_cast<long long>(nk - 1) * n;
    double *Q = Q_all + M.oQ;
    const int *r1s = r1_all + X.oMerge, *r2s = r2_all + X.oMerge;
    double *cn2m = cn2m_all + X.oMerge, *Bl = B_all + X.oMerge;
    int *cntF = cntF_all + X.oFin;
    double *cn2F = cn2F_all + X.oFin;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    unsigned char *lds_cursor = sm;
    ML_PREP_ARRAYS(LDS_CARVE, kf)                        // declares cn2, ctot, part, cnt (hclust_task.hpp)
    const int tid = threadIdx.x;
    for (int f = tid; f < kf; f += 1024) cnt[f] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) atomicAdd(&cnt[labF[i] - 1], 1);
    // |S_f|^2 and S_f . total (row sums of the Gram matrix of the finest clusters' sums, ascending)
    for (int f = tid; f < kf; f += 1024) {
        const double *qr = Q + static_cast<long long>(f) * kpad;
        double b = 0.0;
        for (int g = 0; g < kf; ++g) b += qr[g];
        ctot[f] = b;
        cn2[f] = qr[f];
    }
    __syncthreads();
    for (int f = tid; f < kf; f += 1024) { cntF[f] = cnt[f]; cn2F[f] = cn2[f]; }
    double tot2 = 0.0;
    for (int f = 0; f < kf; ++f) tot2 += ctot[f];        // |total|^2 (every thread, same order)
    if (tid == 0) tot2_all[blockIdx.x] = tot2;
    auto bterm = [&](int r) {
        double rc = ctot[r] / (sqrt(cn2[r]) * sqrt(tot2));
        rc = rc > 1.0 ? 1.0 : (rc < -1.0 ? -1.0 : rc);
        return static_cast<double>(cnt[r]) * (1.0 - rc) * (1.0 - rc);
    };
    // between-cluster term at the finest level: fixed assignment of clusters to threads, partial sums added in thread order
    {
        double b = 0.0;
        for (int f = tid; f < kf; f += 1024) b += bterm(f);
        part[tid] = b;
        __syncthreads();
        if (tid == 0) { double B = 0.0; for (int q = 0; q < 1024; ++q) B += part[q]; Bl[nk - 1] = B; part[0] = B; }
        __syncthreads();
    }
    double B = part[0];
    __syncthreads();
    for (int L = nk - 2; L >= 0; --L) {
        const int r1 = r1s[L], r2 = r2s[L];
        const double cross = Q[static_cast<long long>(r1) * kpad + r2];          // S_r1 . S_r2
        // Gram matrix of the cluster sums: row and column r1 take r2's (entries of dead clusters are never read again)
        for (int x = tid; x < kf; x += 1024) {
            if (x != r1 && x != r2) {
                const double v = Q[static_cast<long long>(r1) * kpad + x] + Q[static_cast<long long>(r2) * kpad + x];
                Q[static_cast<long long>(r1) * kpad + x] = v;
                Q[static_cast<long long>(x) * kpad + r1] = v;
            }
        }
        if (tid == 0) {
            const double t_old = bterm(r1) + bterm(r2);
            const double c2 = (cn2[r1] + cn2[r2]) + 2.0 * cross;
            cn2[r1] = c2; ctot[r1] = ctot[r1] + ctot[r2]; cnt[r1] = cnt[r1] + cnt[r2];
            Q[static_cast<long long>(r1) * kpad + r1] = c2;
            B = (B - t_old) + bterm(r1);
            cn2m[L] = c2; Bl[L] = B;
        }
        __syncthreads();
    }
}

// One wave per cell.  G / T: n x kpad ROW-major here (a cell's finest-level products / distance sums are one contiguous row).
__global__ __launch_bounds__(64 * ML_WAVES) void ml_cells_kernel(const HcMeta *__restrict__ metas, const MlMeta *__restrict__ mls, int task,
                                                                 const int *__restrict__ lab_all, const double *__restrict__ T_all,
                                                                 const double *__restrict__ G_all, const double *__restrict__ nrm_all,
                                                                 const int *__restrict__ r1_all, const int *__restrict__ r2_all,
                                                                 const double *__restrict__ cn2m_all, const int *__restrict__ cntF_all,
                                                                 const double *__restrict__ cn2F_all, double *__restrict__ S_all) {
    const HcMeta M = metas[task];
    const MlMeta X = mls[task];
    const int n = M.n, kf = M.kmax, kpad = M.kpad, nk = M.nk;
    const int *labF = lab_all + M.oLab + static_cast<long long>(nk - 1) * n;
    const double *T = T_all + M.oT, *G = G_all + M.oG, *nrm = nrm_all + M.oNrm;
    const int *r1s = r1_all + X.oMerge, *r2s = r2_all + X.oMerge;
    const double *cn2m = cn2m_all + X.oMerge;
    const int *cntF = cntF_all + X.oFin;
    const double *cn2F = cn2F_all + X.oFin;
    double *S = S_all + X.oS, *Wt = S + static_cast<long long>(n) * nk;
    const bool tfromG = !M.symmetric;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned char *lds_cursor = sm + ml_cells_wave_bytes(kf) * wave;
    ML_CELLS_ARRAYS(LDS_CARVE, kf)                        // declares st, sg, cnt, live, pos (hclust_task.hpp)
    for (long long i = static_cast<long long>(blockIdx.x) * ML_WAVES + wave; i < n; i += static_cast<long long>(gridDim.x) * ML_WAVES) {
        const double *Gi = G + i * kpad, *Ti = T + i * kpad;
        for (int f = lane; f < kf; f += 64) {
            const double g = Gi[f];
            sg[f] = g;
            st[f] = tfromG ? (static_cast<double>(cntF[f]) - g) : Ti[f];
            cnt[f] = static_cast<uint16_t>(cntF[f]);
            live[f] = static_cast<uint16_t>(f); pos[f] = static_cast<uint16_t>(f);
        }
        int own = labF[i] - 1, k = kf;
        double cn2own = cn2F[own];
        const double nr = nrm[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int L = nk - 1; L >= 0; --L) {
            if (L < nk - 1) {                             // the merge that leads from level L + 1 to level L
                const int r1 = r1s[L], r2 = r2s[L];
                if (lane == 0) {
                    st[r1] = st[r1] + st[r2]; sg[r1] = sg[r1] + sg[r2];
                    cnt[r1] = static_cast<uint16_t>(cnt[r1] + cnt[r2]);
                    const int p2 = pos[r2], last = live[k - 1];
                    live[p2] = static_cast<uint16_t>(last); pos[last] = static_cast<uint16_t>(p2);
                }
                --k;
                if (own == r2 || own == r1) { own = r1; cn2own = cn2m[L]; }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            // b = the smallest mean distance to another cluster (a minimum: any order)
            double bmin = HC_INF;
            for (int q = lane; q < k; q += 64) {
                const int r = live[q];
                if (r != own) { const double bb = st[r] / static_cast<double>(cnt[r]); bmin = bb < bmin ? bb : bmin; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_xor(bmin, o); bmin = y < bmin ? y : bmin; }
            if (lane == 0) {
                const int co = cnt[own];
                const double a = st[own] / static_cast<double>(co - 1);
                double s = 0.0;
                if (co > 1 && bmin != a) s = (bmin - a) / fmax(a, bmin);
                double r = sg[own] / (nr * sqrt(cn2own));
                r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
                S[i * nk + L] = s;
                Wt[i * nk + L] = (1.0 - r) * (1.0 - r);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

__global__ __launch_bounds__(ST_THREADS) void ml_level_kernel(const HcMeta *__restrict__ metas, const MlMeta *__restrict__ mls, int task,
                                                              const double *__restrict__ S_all, const double *__restrict__ B_all,
                                                              double *__restrict__ out_all) {
    const HcMeta M = metas[task];
    const MlMeta X = mls[task];
    const int n = M.n, nk = M.nk, L = blockIdx.x, k = M.kmin + L;
    const double *S = S_all + X.oS, *Wt = S + static_cast<long long>(n) * nk;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    int npow2 = 1; while (npow2 < n) npow2 <<= 1;
    unsigned char *lds_cursor = sm;
    ML_LEVEL_ARRAYS(LDS_CARVE, npow2)                        // declares sil, part (hclust_task.hpp)
    const int tid = threadIdx.x;
    double wpart = 0.0;
    for (int i = tid; i < n; i += ST_THREADS) {              // (the same assignment of cells to threads as stats_kernel)
        sil[i] = S[static_cast<long long>(i) * nk + L];
        wpart += Wt[static_cast<long long>(i) * nk + L];
    }
    for (int i = n + tid; i < npow2; i += ST_THREADS) sil[i] = HC_INF;
    part[tid] = wpart;
    __syncthreads();
    for (int size = 2; size <= npow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += ST_THREADS) {
                const int lo = ((t / stride) * stride * 2) + (t % stride);
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double x = sil[lo], y = sil[hi];
                if ((x > y) == up) { sil[lo] = y; sil[hi] = x; }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        double W = 0.0;
        for (int q = 0; q < ST_THREADS; ++q) W += part[q];
        const double B = B_all[X.oMerge + L];
        const double ch = (B / static_cast<double>(k - 1)) / (W / static_cast<double>(n - k));
        const double med = (n & 1) ? sil[n / 2] : (sil[n / 2 - 1] + sil[n / 2]) / 2;
        double *out = out_all + M.oOut;
        out[L] = med;
        out[M.nk + L] = ch;
    }
}

// gather the chosen label column of every task into one contiguous buffer
__global__ void pack_labels_kernel(const HcMeta *__restrict__ metas, const int *__restrict__ lab_all, const int *__restrict__ chosen,
                                   const long long *__restrict__ dst_off, int *__restrict__ dst) {
    const HcMeta M = metas[blockIdx.y];
    const int *src = lab_all + M.oLab + static_cast<long long>(chosen[blockIdx.y]) * M.n;
    int *d = dst + dst_off[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M.n; i += gridDim.x * blockDim.x) d[i] = src[i];
}

// ---------------------------------------------------------------------------------------------
// host side: the launch recipes (on the current stream, ctx().stream)
// ---------------------------------------------------------------------------------------------
void hclust_copy_d(const HcMeta *metas, int tasks, const double *D, double *D0) {
    hipLaunchKernelGGL(copy_d_kernel, dim3(64, tasks), dim3(256), 0, ctx().stream, metas, D, D0);
    launch_check("copy_d_kernel");
}

void hclust_pack_labels(const HcMeta *metas, int tasks, const int *lab, const int *chosen, const long long *dst_off, int *dst) {
    hipLaunchKernelGGL(pack_labels_kernel, dim3(8, tasks), dim3(256), 0, ctx().stream, metas, lab, chosen, dst_off, dst);
    launch_check("pack_labels_kernel");
}

namespace {

// a5b, many levels (the chunk is one range: setup_chunk)
void many_levels_stats(const HcStatsRange &r, const HcManyLevels &ml) {
    Ctx &c = ctx();
    hipStream_t st = c.stream;
    const int T = r.tasks, max_n = r.max_n, max_kpad = r.max_kpad;
    if (r.cnt[3]) gemm_tn_f64_batched(r.gemm + r.off[3], r.cnt[3], max_kpad, max_kpad, "cluster_gram_gemm");
    gemm_tn_f64_batched(r.gemm + ml.ml_off, ml.ml_cnt, max_n, max_kpad, "row_cluster_dot_gemm");
    if (ml.mlt_cnt) gemm_tn_f64_batched(r.gemm + ml.mlt_off, ml.mlt_cnt, max_n, max_kpad, "dist_cluster_sums_gemm");
    // the merge that leads from level L + 1 to level L, in finest-cluster ids: a replay of the merge list on the host
    std::vector<int> h_ia(ml.oM), h_ib(ml.oM);
    SHARP_HIP_CHECK(hipMemcpyAsync(h_ia.data(), r.ia, ml.oM * sizeof(int), hipMemcpyDeviceToHost, st));
    SHARP_HIP_CHECK(hipMemcpyAsync(h_ib.data(), r.ib, ml.oM * sizeof(int), hipMemcpyDeviceToHost, st));
    SHARP_HIP_CHECK(hipStreamSynchronize(st));
    const std::vector<HcMeta> &metas = *ml.metas;
    const std::vector<MlMeta> &mlmetas = *ml.mlmetas;
    long long tot_levels = 0;
    for (int t = 0; t < T; ++t) tot_levels += metas[t].nk;
    std::vector<int> h_r1(tot_levels, 0), h_r2(tot_levels, 0);
    for (int t = 0; t < T; ++t) {
        const HcMeta &M = metas[t];
        const int *ia = h_ia.data() + M.oM, *ib = h_ib.data() + M.oM;
        std::vector<int> fin(M.n, 0);                    // cell -> finest-cluster id if the cell is a representative at k = kmax
        std::vector<char> absorbed(M.n, 0);
        for (int q = 0; q < M.n - M.kmax; ++q) absorbed[ib[q] - 1] = 1;
        int f = 0;
        for (int i = 0; i < M.n; ++i) if (!absorbed[i]) fin[i] = f++;   // ids by first appearance = ascending representative
        for (int L = M.nk - 2; L >= 0; --L) {
            const int q = M.n - 1 - (M.kmin + L);         // level k has the merges 0 .. n - k - 1 applied
            h_r1[mlmetas[t].oMerge + L] = fin[ia[q] - 1];
            h_r2[mlmetas[t].oMerge + L] = fin[ib[q] - 1];
        }
    }
    SHARP_HIP_CHECK(hipMemcpyAsync(ml.r1, h_r1.data(), tot_levels * sizeof(int), hipMemcpyHostToDevice, st));
    SHARP_HIP_CHECK(hipMemcpyAsync(ml.r2, h_r2.data(), tot_levels * sizeof(int), hipMemcpyHostToDevice, st));
    KernelTimer tm("sil_ch_stats");
    const size_t lds_p = ml_prep_lds_bytes(max_kpad);
    allow_dynamic_lds(ml_prep_kernel, lds_p);
    hipLaunchKernelGGL(ml_prep_kernel, dim3(T), dim3(1024), lds_p, st, r.metas, ml.dml, r.lab, r.Q, ml.r1, ml.r2,
                       ml.cn2m, ml.B, ml.cntF, ml.cn2F, ml.tot2);
    launch_check("ml_prep_kernel");
    const size_t lds_c = ml_cells_lds_bytes(max_kpad);
    allow_dynamic_lds(ml_cells_kernel, lds_c);
    const size_t lds_l = ml_level_lds_bytes(max_n);
    allow_dynamic_lds(ml_level_kernel, lds_l);
    for (int t = 0; t < T; ++t) {
        const HcMeta &M = metas[t];
        const int blocks = std::min((M.n + ML_WAVES - 1) / ML_WAVES, c.num_cu * std::max(1, static_cast<int>(HR_LDS_CU / std::max<size_t>(lds_c, 1))));
        hipLaunchKernelGGL(ml_cells_kernel, dim3(blocks), dim3(64 * ML_WAVES), lds_c, st, r.metas, ml.dml, t, r.lab, r.T, r.G, r.nrm,
                           ml.r1, ml.r2, ml.cn2m, ml.cntF, ml.cn2F, ml.S);
        hipLaunchKernelGGL(ml_level_kernel, dim3(M.nk), dim3(ST_THREADS), lds_l, st, r.metas, ml.dml, t, ml.S, ml.B, r.out);
    }
    launch_check("ml_cells_kernel");
}

}  // namespace

void hclust_level_stats(const HcStatsRange &r, const HcManyLevels *ml) {
    hipStream_t st = ctx().stream;
    const int Ts = r.tasks, max_n = r.max_n, max_p = r.max_p, max_nk = r.max_nk, max_kpad = r.max_kpad;
    // a5a: labels for every candidate k
    {
        const size_t lds = cutree_lds_bytes(max_n);
        allow_dynamic_lds(cutree_kernel, lds);
        KernelTimer tm("cutree");
        hipLaunchKernelGGL(cutree_kernel, dim3(Ts), dim3(HC_THREADS), lds, st, r.metas, r.ia, r.ib, r.lab);
        launch_check("cutree_kernel");
    }
    // the finest level's cluster sums: a dedicated kernel (SHARP_STATS_SUMS=0: the one-hot matrix and a skinny GEMM); the many-levels
    // form and clusterings of more than SS_KMAX clusters keep the GEMM
    const bool sums = knobs().stats_sums && !ml && max_kpad <= SS_KMAX;
    if (!sums || r.any_sym) {
        KernelTimer tm("onehot");
        hipLaunchKernelGGL(onehot_kernel, dim3(64, Ts), dim3(256), 0, st, r.metas, r.lab, r.H);
        launch_check("onehot_kernel");
    }
    if (sums) {
        KernelTimer tm("cluster_sums_gemm");
        const size_t lds = cluster_sums_lds_bytes(max_kpad);
        allow_dynamic_lds(cluster_sums_kernel, lds);
        hipLaunchKernelGGL(cluster_sums_kernel, dim3((max_p + 63) / 64, Ts), dim3(64 * SS_WAVES), lds, st, r.metas, r.lab, r.Cr, r.CSt);
        launch_check("cluster_sums_kernel");
    } else if (r.cnt[1]) gemm_tn_f64_batched(r.gemm + r.off[1], r.cnt[1], max_p, max_kpad, "cluster_sums_gemm");
    if (ml) { many_levels_stats(r, *ml); return; }
    if (r.cnt[2]) gemm_tn_f64_batched(r.gemm + r.off[2], r.cnt[2], max_kpad, max_n, "row_cluster_dot_gemm");
    if (r.cnt[3]) gemm_tn_f64_batched(r.gemm + r.off[3], r.cnt[3], max_kpad, max_kpad, "cluster_gram_gemm");
    if (r.cnt[4]) gemm_tn_f64_batched(r.gemm + r.off[4], r.cnt[4], max_kpad, max_n, "dist_cluster_sums_gemm");
    // a5b: silhouette medians + CH per level
    const int kcap = std::max(max_kpad, 64);
    // at most 64 finest clusters (every call of the reference's defaults: maxN = 40): the walk over them fits one register per lane
    const bool lane_form = knobs().stats_lane && max_kpad <= 64;
    const size_t lds = lane_form ? stats_lane_lds_bytes(max_n, kcap) : stats_lds_bytes(max_n, kcap);
    const auto kern = lane_form ? stats_lane_kernel : stats_kernel;
    allow_dynamic_lds(kern, lds);
    KernelTimer tm("sil_ch_stats");
    const long long blocks = static_cast<long long>((Ts + 7) / 8) * 8 * max_nk;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(ST_THREADS), lds, st, r.metas, r.lab, r.T,
                       r.G, r.Q, r.nrm, r.out, Ts, max_nk, kcap);
    launch_check("stats_kernel");
}

}  // namespace sharp
