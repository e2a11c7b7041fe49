// a5b, the lane-program form of stats_kernel (included by hclust_stats.hip; same arguments, same grid, same outputs).
//
// One workgroup per (task, level) as in stats_kernel, and the same arithmetic per cell -- the sums over a level cluster's finest
// clusters in ascending order, one division per cluster, the same silhouette and within-cluster terms, the same fixed order of the
// workgroup's sums -- so the median silhouettes are bit for bit stats_kernel's.  What differs is how a cell gets there:
//   * the walk over the kf finest clusters is the same for every cell of the level, so it is a PROGRAM held in registers -- lane q of
//     every wave keeps (finest cluster, its count, the level cluster it belongs to, the level cluster's size if q closes it) -- and a
//     cell's loop reads it with v_readlane (scalar results: the cluster boundaries are scalar branches, the addresses scalar offsets).
//     stats_kernel re-read the walk from LDS per cell and branched per lane on it: its cells' loop was bound by those reads and
//     branches (profiles/r05_stats_kernel_phases.txt), not by the 40 adds and k divisions a cell needs.  (kf <= 64: one register each.)
//   * the median is a radix selection over the cells' silhouettes (8 bits per pass on order-preserving integer keys, the passes end as
//     soon as the rank's bin holds one key) instead of a bitonic sort of the padded array: 3 barriers per pass, 3-4 passes, against 66
//     barrier-separated compare-exchange sweeps.
//   * |sum_c|^2 and sum_c . total of a level cluster: one thread per finest cluster sums its ROW of the Gram matrix (over the cluster's
//     members; over all finest clusters), one thread per level cluster adds its rows' partial sums in ascending order.  stats_kernel's
//     single running sum per cluster took 100-230 us at k = 2 ... 5 (one thread, ~3000 dependent LDS reads).  This changes the
//     association of those two sums (CH moves in its last bits; the silhouettes do not use them).
// R/get_opt_hclust.R:112-187 (cluster::silhouette on as.dist(1 - cor), clues::get_CH with disMethod = "1-corr").
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long st_key_of(double x) {   // order-preserving: x < y  <=>  key(x) < key(y) (no NaN here)
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double st_value_of(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double(static_cast<long long>(b));
}

inline size_t stats_lane_lds_bytes(int max_n, int kcap) {
    int npow2 = 1; while (npow2 < max_n) npow2 <<= 1;
    return static_cast<size_t>(npow2) * 8 + ST_THREADS * 8 + 4 * static_cast<size_t>(kcap) * 8 + (5 * static_cast<size_t>(kcap) + 8) * 4 + 256 * 4 + 64;
}

template <bool SYM>
__device__ __forceinline__ void st_lane_cells(const int n, const int kf, const int nld, const int tid, const int *__restrict__ lab,
                                              const double *__restrict__ T, const double *__restrict__ G, const double *__restrict__ nrm,
                                              const int *cnt, const double *cn2, const int pf, const int pcnt, const int pend, const int pcid,
                                              double *sil, double &wpart) {
    for (int i = tid; i < n; i += ST_THREADS) {
        const int own = lab[i] - 1;
        const double *Ti = T + i, *Gi = G + i;
        double a = 0.0, bmin = 0.0, gown = 0.0, sc = 0.0, gc = 0.0;
        bool have_b = false;
        for (int q0 = 0; q0 < kf; q0 += 8) {
            double gv[8], tv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u < kf ? q0 + u : kf - 1;
                const long long off = static_cast<long long>(__builtin_amdgcn_readlane(pf, q)) * nld;
                gv[u] = Gi[off];
                tv[u] = SYM ? Ti[off] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u;
                if (q < kf) {
                    sc += SYM ? tv[u] : (static_cast<double>(__builtin_amdgcn_readlane(pcnt, q)) - gv[u]);
                    gc += gv[u];
                    const int e = __builtin_amdgcn_readlane(pend, q);
                    if (e) {                                     // finest cluster q closes level cluster c (size e)
                        const int c = __builtin_amdgcn_readlane(pcid, q);
                        const bool isown = c == own;
                        const double v = sc / static_cast<double>(isown ? e - 1 : e);
                        if (isown) { a = v; gown = gc; }
                        else if (!have_b || bmin > v) { bmin = v; have_b = true; }
                        sc = 0.0; gc = 0.0;
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
}

__global__ __launch_bounds__(ST_THREADS) void stats_lane_kernel(const HcMeta *__restrict__ metas, const int *__restrict__ lab_all,
                                                                const double *__restrict__ T_all, const double *__restrict__ G_all,
                                                                const double *__restrict__ Q_all, const double *__restrict__ nrm_all,
                                                                double *__restrict__ out_all, int count, int max_nk, int kcap) {
    // (task, level) of this workgroup: as stats_kernel (the eight tasks of a group on the eight XCDs, a task's levels on one L2)
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
    double *sil = reinterpret_cast<double *>(sm);            // npow2 (the Gram matrix of the finest clusters first)
    double *part = sil + npow2;                              // ST_THREADS
    double *cn2 = part + ST_THREADS;                         // k  : |sum_c|^2
    double *ctot = cn2 + kcap;                               // k  : sum_c . total
    double *rowA = ctot + kcap;                              // kf : row q of the Gram matrix summed over the members of q's level cluster
    double *rowB = rowA + kcap;                              // kf : ... over all finest clusters
    int *cnt = reinterpret_cast<int *>(rowB + kcap);         // k
    int *cntF = cnt + kcap;                                  // kf
    int *fm = cntF + kcap;                                   // kf : level cluster (0-based) of finest cluster f
    int *start = fm + kcap;                                  // k + 1
    int *order = start + kcap + 1;                           // kf : finest clusters grouped by level cluster
    int *hist = order + kcap + 7;                            // 256 bins of the selection
    unsigned long long *sel = reinterpret_cast<unsigned long long *>((reinterpret_cast<uintptr_t>(hist + 256) + 7) & ~static_cast<uintptr_t>(7));   // [5]
    const int tid = threadIdx.x, lane = tid & 63;
    for (int c = tid; c < kcap; c += ST_THREADS) { cnt[c] = 0; cntF[c] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += ST_THREADS) {
        atomicAdd(&cnt[lab[i] - 1], 1);
        atomicAdd(&cntF[labF[i] - 1], 1);
        fm[labF[i] - 1] = lab[i] - 1;
    }
    __syncthreads();
    for (int c = tid; c <= k; c += ST_THREADS) start[c] = 0;
    __syncthreads();
    for (int f = tid; f < kf; f += ST_THREADS) atomicAdd(&start[fm[f] + 1], 1);
    __syncthreads();
    if (tid == 0) for (int c = 0; c < k; ++c) start[c + 1] += start[c];
    const bool q_lds = kf * kf <= npow2;
    if (q_lds) for (int e = tid; e < kf * kf; e += ST_THREADS) sil[e] = Q[static_cast<long long>(e / kf) * kpad + e % kf];
    __syncthreads();
    for (int c = tid; c < k; c += ST_THREADS) {
        int pos = start[c];
        for (int f = 0; f < kf; ++f) if (fm[f] == c) order[pos++] = f;
    }
    __syncthreads();
    for (int q = tid; q < kf; q += ST_THREADS) {
        const int f = order[q], c = fm[f];
        const int s0 = start[c], s1 = start[c + 1];
        double ra = 0.0, rb = 0.0;
        if (q_lds) {
            const double *qr = sil + f * kf;
            for (int q2 = s0; q2 < s1; ++q2) ra += qr[order[q2]];
            for (int f2 = 0; f2 < kf; ++f2) rb += qr[f2];
        } else {
            const double *qr = Q + static_cast<long long>(f) * kpad;
            for (int q2 = s0; q2 < s1; ++q2) ra += qr[order[q2]];
            for (int f2 = 0; f2 < kf; ++f2) rb += qr[f2];
        }
        rowA[q] = ra; rowB[q] = rb;
    }
    __syncthreads();
    for (int c = tid; c < k; c += ST_THREADS) {
        double a = 0.0, b = 0.0;
        for (int q = start[c]; q < start[c + 1]; ++q) { a += rowA[q]; b += rowB[q]; }
        cn2[c] = a; ctot[c] = b;
    }
    // the walk as a program in registers: lane q < kf of every wave
    int pf = 0, pcnt = 0, pend = 0, pcid = 0;
    if (lane < kf) {
        pf = order[lane]; pcnt = cntF[pf]; pcid = fm[pf];
        pend = (lane + 1 == start[pcid + 1]) ? cnt[pcid] : 0;
    }
    __syncthreads();                                          // cn2 complete; the Gram matrix in sil[] is no longer read
    double wpart = 0.0;
    if (M.symmetric) st_lane_cells<true>(n, kf, M.nld, tid, lab, T, G, nrm, cnt, cn2, pf, pcnt, pend, pcid, sil, wpart);
    else st_lane_cells<false>(n, kf, M.nld, tid, lab, T, G, nrm, cnt, cn2, pf, pcnt, pend, pcid, sil, wpart);
    part[tid] = wpart;
    // median: the key of rank r = (n - 1) / 2 by radix selection, most significant byte first
    const int r0 = (n - 1) / 2;
    unsigned long long prefix = 0;
    int r = r0, shift = 56;
    for (;; shift -= 8) {
        for (int t = tid; t < 256; t += ST_THREADS) hist[t] = 0;
        __syncthreads();                                      // (first pass: also sil[] and part[] complete)
        for (int i = tid; i < n; i += ST_THREADS) {
            const unsigned long long key = st_key_of(sil[i]);
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[static_cast<int>(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < 64) {                                       // the bin that holds rank r: four bins per lane, a prefix sum over the lanes
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int s = h0 + h1 + h2 + h3;
            int incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); incl += lane >= d ? t : 0; }
            const int excl = incl - s;
            if (excl <= r && r < incl) {
                int rr = r - excl, bin = 4 * lane, hc = h0;
                if (rr >= h0) { rr -= h0; bin += 1; hc = h1;
                    if (rr >= h1) { rr -= h1; bin += 1; hc = h2;
                        if (rr >= h2) { rr -= h2; bin += 1; hc = h3; } } }
                sel[0] = static_cast<unsigned long long>(bin);
                sel[1] = (static_cast<unsigned long long>(static_cast<unsigned>(hc)) << 32) | static_cast<unsigned>(rr);
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        r = static_cast<int>(sel[1] & 0xffffffffull);
        const int hc = static_cast<int>(sel[1] >> 32);
        if (hc == 1 || shift == 0) break;                     // (uniform: every thread read the same sel[])
    }
    // the key itself (its low bits are not in the prefix when the passes ended early), then for even n the next one in order
    if (tid == 0) { sel[2] = 0; sel[3] = ~0ull; }
    for (int i = tid; i < n; i += ST_THREADS) {
        const unsigned long long key = st_key_of(sil[i]);
        if ((key >> shift) == (prefix >> shift)) sel[4] = key;   // (all matching keys are equal when shift == 0; one key matches otherwise; sel[0..1] may still be read)
    }
    __syncthreads();
    const unsigned long long k_lo = sel[4];
    if (!(n & 1)) {
        int le = 0;
        unsigned long long mn = ~0ull;
        for (int i = tid; i < n; i += ST_THREADS) {
            const unsigned long long key = st_key_of(sil[i]);
            le += key <= k_lo ? 1 : 0;
            if (key > k_lo && key < mn) mn = key;
        }
        if (le) atomicAdd(reinterpret_cast<int *>(&sel[2]), le);
        if (mn != ~0ull) atomicMin(&sel[3], mn);
        __syncthreads();
    }
    if (tid == 0) {
        double W = 0.0;
#pragma unroll 1
        for (int q0 = 0; q0 < ST_THREADS; q0 += 16) {        // the same running sum as stats_kernel, sixteen LDS reads in flight
            double pv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) pv[u] = part[q0 + u];
#pragma unroll
            for (int u = 0; u < 16; ++u) W += pv[u];
        }
        double tot2 = 0.0;
        for (int c = 0; c < k; ++c) tot2 += ctot[c];
        double Bs = 0.0;
        for (int c = 0; c < k; ++c) {
            double rr = ctot[c] / (sqrt(cn2[c]) * sqrt(tot2));
            rr = rr > 1.0 ? 1.0 : (rr < -1.0 ? -1.0 : rr);
            Bs += static_cast<double>(cnt[c]) * (1.0 - rr) * (1.0 - rr);
        }
        const double ch = (Bs / static_cast<double>(k - 1)) / (W / static_cast<double>(n - k));
        double med;
        if (n & 1) med = st_value_of(k_lo);
        else {
            const int le = *reinterpret_cast<int *>(&sel[2]);
            const unsigned long long k_hi = le > r0 + 1 ? k_lo : sel[3];
            med = (st_value_of(k_lo) + st_value_of(k_hi)) / 2;
        }
        double *out = out_all + M.oOut;
        out[L] = med;
        out[M.nk + L] = ch;
    }
}
