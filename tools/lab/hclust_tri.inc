// hclust_tri.inc -- the bulk-synchronous agglomeration of hclust_rnn_kernel (MODE 0: one launch, one workgroup per task) on the UPPER
// TRIANGLE of the distance matrix: half the bytes per round.  (Included by hclust_agglo.hip; R/get_opt_hclust.R:76-83, SURVEY.md App. A.4.)
//
// hclust_rnn_kernel keeps the symmetric matrix in full: every round reads n_a^2 and writes n_b^2 entries, 10.1 n^2 x 8 B per task over
// the ~45 rounds of a 2000-observation task, and its time is those bytes (4.4 of the 5 TB/s a copy reaches).  Here row A of a scratch
// matrix holds only its entries to the right, (A, B) with B > A:
//   * a new row is still ONE contiguous sweep of an old row (the unmerged clusters keep their relative order, so the entries right of
//     the diagonal stay right of it; the merged clusters take the last indices, so their columns are right of every unmerged row);
//   * what a row lacks -- its distances to the pair members k < a, which sit in row k at column a -- is 2 n_p single loads per row;
//     the rows of a workgroup are handed out in order, so neighbouring rows fetch neighbouring entries of the same 2 n_p rows and
//     the lines are served by the CU's cache: these gathers add entries, hardly bytes;
//   * a nearest neighbour is the minimum over a row AND a column: the sweep keeps the row minimum in registers as before and offers
//     every entry (A, B) to column B through one LDS atomic minimum on a packed key (the distance's 48 leading bits in an order-preserving
//     form | the row index).  After the round's barrier one thread per cluster compares the two candidates, reading the column
//     candidate's exact value back from the matrix.  Two column candidates that agree in those 48 bits (2^-36 relative) cannot be
//     ranked by the key: the returning form of the atomic lets the later one see the earlier, and the task is handed to the
//     sequential kernel like any exact tie;
//   * the rows of merged clusters only hold their entries against the LATER merged clusters (n_p^2 / 2 per round, four gathers each).
// Same pairs, same ranks, same Lance-Williams arithmetic in the same order as hclust_rnn_kernel: same merges, same heights.
// LDS: 47 B per observation (the 39 B of hclust_rnn_kernel + the column keys); the rest of the CU's 160 KB is the waves' stage.
constexpr int HT_THREADS = 1024;
constexpr int HT_MAXN = 2304;                // 47 B x 2304 = 106 KB of state: the stage still holds a round's pairs (n_p ~ n / 20)

// IEEE order -> unsigned integer order, exact and invertible (1 - cor may be -1e-16: the sign has to be handled)
__device__ __forceinline__ unsigned long long ht_ord(double v) {
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    const unsigned long long m = static_cast<unsigned long long>(static_cast<long long>(b) >> 63);      // all ones for a negative value
    return b ^ (m | 0x8000000000000000ull);
}
__device__ __forceinline__ double ht_unord(unsigned long long o) {
    const unsigned long long m = (o >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull;
    return __longlong_as_double(static_cast<long long>(o ^ m));
}
__device__ __forceinline__ unsigned long long ht_key(unsigned long long ord, int idx) {
    return (ord & ~0xffffull) | static_cast<unsigned long long>(static_cast<unsigned int>(idx) & 0xffffu);
}

// The dynamic LDS of hclust_tri_kernel (a list for LDS_CARVE / LDS_COUNT, hclust_task.hpp): hclust_rnn_kernel's state arrays with the
// column keys behind dnnA; nal = (n + 3) & ~3
#define HT_STATE_ARRAYS(X, nal)                                                                                             \
    X(double, dnnA, 2 * (nal))               /* [2][nal]  NN distance (also the pair's height) */                           \
    X(unsigned long long, colkey, nal)       /* best (distance, row) offered to a column */                                 \
    X(uint16_t, cidA, 2 * (nal))             /* [2][nal]  smallest original member */                                       \
    X(uint16_t, cszA, 2 * (nal))             /* [2][nal]  cluster size */                                                   \
    X(uint16_t, nn, nal)                                                                                                    \
    X(uint16_t, partner, nal)                /* old index of the RNN partner or NONE */                                     \
    X(uint16_t, pseq, nal)                   /* rank of the pair in the round */                                            \
    X(uint16_t, oldidx, nal)                 /* new index -> old index */                                                   \
    X(uint16_t, newidx, nal)                 /* old index -> new index */                                                   \
    X(uint16_t, plist, nal)                  /* first members of the pairs */                                               \
    X(uint16_t, colmap, nal)                 /* old column -> new column, or 0x8000 | (2 rank + member) */                  \
    X(int, ctl, 16)                          /* 0 npairs, 1 abort */                                                        \
    X(int, wsum, HT_THREADS / 64 + 1)                                                                                       \
    X(unsigned char, tie, nal)
// the launch: the state (64 unused bytes of slack behind it) or the final sort of the merges in the same memory (16 B per entry), and
// whatever else the CU has as the waves' stage
inline size_t hclust_tri_lds(int max_n) {
    const int nal = (max_n + 3) & ~3;
    size_t lds_bytes = 0;
    HT_STATE_ARRAYS(LDS_COUNT, nal)
    return std::max(std::max((lds_bytes + 64 + 15) / 16 * 16, static_cast<size_t>(hc_npow2(max_n - 1)) * 16), HR_LDS_CU);
}

__global__ __launch_bounds__(HT_THREADS) void hclust_tri_kernel(const HcMeta *__restrict__ metas, const double *__restrict__ Dall,
                                                                double *__restrict__ S0all, double *__restrict__ S1all,
                                                                int *__restrict__ ia_all, int *__restrict__ ib_all,
                                                                double *__restrict__ h_all, int *__restrict__ status, int lds_launch) {
    const HcMeta M = metas[blockIdx.x];
    const int n = M.n, nld = M.nld, method = M.method;
    const double *D = Dall + M.oD;
    double *Sb[2] = {S0all + M.oD, S1all + M.oD};
    int *ia = ia_all + M.oM, *ib = ib_all + M.oM;
    double *crit = h_all + M.oM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int nwave = HT_THREADS / 64;
    if (method == 6 || method == 7 || n > HT_MAXN) {                       // centroid / median are not reducible
        if (tid == 0) status[blockIdx.x] = 1;
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int nal = (n + 3) & ~3;
    unsigned char *lds_cursor = sm;
    HT_STATE_ARRAYS(LDS_CARVE, nal)                                         // declares dnnA, colkey, cidA, ... tie (the list above)
    const int stage_off = static_cast<int>((lds_cursor - sm + 15) & ~static_cast<long>(15));
    double *stage = reinterpret_cast<double *>(sm + stage_off);

#ifdef SHARP_LAB_HT_GUARD         // (lab build: every outer loop spends from a budget; an exhausted budget ends the thread with a code in status)
    long long ht_budget = 4000000;
#define HT_GUARD(code) do { if (--ht_budget < 0) { status[blockIdx.x] = 100 + (code); return; } } while (0)
#else
#define HT_GUARD(code) do { } while (0)
#endif
#ifdef SHARP_LAB_HT_TIMING        // (lab build: where a workgroup's cycles go; block 0 prints)
    long long tt_setup = 0, tt_rebuild = 0, tt_combine = 0, tt_pf = 0, tt_sweep = 0, tt_stash = 0, tt_mcol = 0, tt_red = 0, tt_mrow = 0, tt_r0 = 0, tt_bar = 0;
#define HT_T(var, expr) do { const long long _t0 = __builtin_readcyclecounter(); expr; var += __builtin_readcyclecounter() - _t0; } while (0)
#define HT_TICK(var) var = __builtin_readcyclecounter()
#else
#define HT_TICK(var) do { } while (0)
#endif
    int cur = 0, na = n, done = 0;
    int src = -1;                                                            // -1: D (pristine, full), else scratch index (upper triangle)
    for (int i = tid; i < n; i += HT_THREADS) { cidA[i] = static_cast<uint16_t>(i); cszA[i] = 1; colkey[i] = ~0ull; }
    if (tid == 0) { for (int q = 0; q < 16; ++q) ctl[q] = 0; }
    __syncthreads();

    // an entry (A, B), B > A, offered to column B
    // (issue and check are separate so that a batch of atomics is in flight before the first result is looked at; two keys of one
    // column differ in their row index, so "same 48 leading bits" is old ^ key < 2^16)
    auto offer_check = [&](unsigned long long old, unsigned long long key) {
        if ((old ^ key) < 65536ull) ctl[1] = 1;                              // the key cannot rank these two: the sequential kernel decides
    };
    auto offer = [&](int B, double v, int A) {
        const unsigned long long key = ht_key(ht_ord(v), A);
        offer_check(atomicMin(&colkey[B], key), key);
    };
    // After a barrier: every cluster's nearest neighbour from its row candidate (dnn / nnW / tie, written by the row's wave) and its
    // column candidate (colkey), whose exact value is read back from `mat` (upper triangle: entry (ci, X) in row ci).
    auto combine = [&](const double *mat, bool sq, int cnt, double *dnnO, uint16_t *nnO, unsigned char *tieO) {
        for (int X = tid; X < cnt; X += HT_THREADS) {
            double rv = dnnO[X];
            int ri = nnO[X], rt = tieO[X];
            const unsigned long long ck = colkey[X];
            colkey[X] = ~0ull;
            if (ck != ~0ull) {
                const int ci = static_cast<int>(ck & 0xffffull);
                double cv = ((const __attribute__((address_space(1))) double *)mat)[static_cast<long long>(ci) * nld + X];
                if (sq) cv *= cv;
                if (cv < rv) { rv = cv; ri = ci; rt = 0; }
                else if (cv == rv) rt = 1;
            }
            dnnO[X] = rv; nnO[X] = static_cast<uint16_t>(ri < cnt ? ri : 0); tieO[X] = static_cast<unsigned char>(cnt > 2 ? rt : 0);
        }
    };

    // round 0 nearest neighbours from the pristine matrix's upper triangle (squared for ward.D2): one wave per row
    {
#ifdef SHARP_LAB_HT_TIMING
        const long long r0a = __builtin_readcyclecounter();
#endif
        const bool sq0 = method == 8;
        for (int a = wave; a < n; a += nwave) {
            const double *row = D + static_cast<long long>(a) * nld;
            double mn = HC_INF, sc = HC_INF;
            int ix = 0x7fffffff;
            for (int j0 = ((a + 1) & ~7) + lane; j0 < n; j0 += 64 * 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int j = j0 + 64 * u; v[u] = row[j < n ? j : n - 1]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = j0 + 64 * u;
                    if (j < n && j > a) {
                        const double x = sq0 ? v[u] * v[u] : v[u];
                        sc = fmin(sc, fmax(mn, x));
                        if (x < mn) { mn = x; ix = j; }
                        offer(j, x, a);
                    }
                }
            }
            HrBest g;
            g.v = mn; g.i = ix; g.tie = 0;
            g = hr_wave(g);
            g.tie |= __ballot(sc == g.v) != 0ull ? 1 : 0;
            if (lane == 0) { dnnA[a] = g.v; nn[a] = static_cast<uint16_t>(g.i < n ? g.i : 0); tie[a] = static_cast<unsigned char>(g.tie); }
        }
        __syncthreads();
        combine(D, sq0, n, dnnA, nn, tie);
        __syncthreads();
#ifdef SHARP_LAB_HT_TIMING
        tt_r0 = __builtin_readcyclecounter() - r0a;
#endif
    }

#ifdef SHARP_LAB_HT_ROUNDS
    int ht_round = 0;
#endif
    while (na > 1) {
#ifdef SHARP_LAB_HT_ROUNDS       // (lab build: stop after that many rounds and hand the task to the sequential kernel)
        if (ht_round++ >= SHARP_LAB_HT_ROUNDS) { if (tid == 0) status[blockIdx.x] = 1; return; }
#endif
        HT_GUARD(2);
#ifdef SHARP_LAB_HT_TIMING
        const long long ra = __builtin_readcyclecounter();
#endif
        double *dnn = dnnA + cur * nal;
        uint16_t *cid = cidA + cur * nal, *csz = cszA + cur * nal;
        double *dnnN = dnnA + (cur ^ 1) * nal;
        uint16_t *cidN = cidA + (cur ^ 1) * nal, *cszN = cszA + (cur ^ 1) * nal;
        int np = 0, nb = 0, ns = 0;
        // (1) reciprocal pairs
        for (int a = tid; a < na; a += HT_THREADS) {
            partner[a] = HR_NONE;
            if (tie[a]) ctl[1] = 1;
        }
        __syncthreads();
        for (int a = tid; a < na; a += HT_THREADS) {
            const int b = nn[a];
            if (b > a && nn[b] == a) {
                partner[a] = static_cast<uint16_t>(b); partner[b] = static_cast<uint16_t>(a);
                plist[atomicAdd(&ctl[0], 1)] = static_cast<uint16_t>(a);
            }
        }
        __syncthreads();
        np = ctl[0];
        if (ctl[1] || np == 0) {                                            // tie or no pair: the sequential kernel takes this task
            if (tid == 0) status[blockIdx.x] = 1;
            return;
        }
        // (2) rank of each pair by (height, lower original index) = the sequential algorithm's order
        for (int q = tid; q < np; q += HT_THREADS) {
            const int a = plist[q];
            const double h = dnn[a];
            const int ida = cid[a] < cid[partner[a]] ? cid[a] : cid[partner[a]];
            int rank = 0;
            for (int q2 = 0; q2 < np; ++q2) {
                const int a2 = plist[q2];
                const double h2 = dnn[a2];
                const int id2 = cid[a2] < cid[partner[a2]] ? cid[a2] : cid[partner[a2]];
                rank += (h2 < h || (h2 == h && id2 < ida)) ? 1 : 0;
            }
            pseq[a] = static_cast<uint16_t>(rank); pseq[partner[a]] = static_cast<uint16_t>(rank);
            const int ib_ = cid[a] < cid[partner[a]] ? cid[partner[a]] : cid[a];
            ia[done + rank] = ida + 1; ib[done + rank] = ib_ + 1;
            crit[done + rank] = h;                                           // squared for ward.D2 until the final pass
        }
        // (3) new indices: the unmerged clusters keep their relative order in [0, ns), the merged clusters follow in rank order in [ns, nb)
        {
            const int chunk = (na + HT_THREADS - 1) / HT_THREADS;
            const int lo = tid * chunk, hi = lo + chunk < na ? lo + chunk : na;
            int c = 0;
            for (int a = lo; a < hi; ++a) c += partner[a] == HR_NONE ? 1 : 0;
            int incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); incl += lane >= d ? t : 0; }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            if (tid == 0) { int run = 0; for (int w = 0; w < nwave; ++w) { const int t = wsum[w]; wsum[w] = run; run += t; } wsum[nwave] = run; }
            __syncthreads();
            int pos = wsum[wave] + incl - c;
            for (int a = lo; a < hi; ++a)
                if (partner[a] == HR_NONE) { newidx[a] = static_cast<uint16_t>(pos); colmap[a] = static_cast<uint16_t>(pos); oldidx[pos++] = static_cast<uint16_t>(a); }
            ns = wsum[nwave];                                                // rows of unmerged clusters (= na - 2 np)
            for (int q = tid; q < np; q += HT_THREADS) {                     // bit 15 of oldidx: the survivor is a merged cluster
                const int a = plist[q], B = ns + pseq[a];
                newidx[a] = static_cast<uint16_t>(B);
                oldidx[B] = static_cast<uint16_t>(a | 0x8000);
                colmap[a] = static_cast<uint16_t>(0x8000 | (2 * pseq[a]));
                colmap[partner[a]] = static_cast<uint16_t>(0x8000 | (2 * pseq[a] + 1));
            }
        }
        nb = ns + np;
        // what a merged column needs of its pair, by rank: the two sizes and the height (three independent LDS reads in the rows' loops
        // instead of the chain oldidx -> partner -> csz / dnn); kept at the head of the stage
        double *pinfo = stage;
        for (int q = tid; q < np; q += HT_THREADS) {
            const int k1 = plist[q], rk = pseq[k1];
            pinfo[rk] = csz[k1]; pinfo[np + rk] = csz[partner[k1]]; pinfo[2 * np + rk] = dnn[k1];
        }
        double *wstage = stage + 3 * np;
        __syncthreads();
        const int stage_rows = std::min(2, std::max(0, lds_launch - stage_off - 24 * np) / (nwave * 16 * np));   // rows per wave whose pair entries fit the stage
        if (stage_rows == 0) {                                               // (cannot happen below HT_MAXN observations; a guard, not a path)
            if (tid == 0) status[blockIdx.x] = 1;
            return;
        }
#ifdef SHARP_LAB_HT_TIMING
        const long long rb = __builtin_readcyclecounter();
        tt_setup += rb - ra;
#endif
        // (4) next matrix: its upper triangle, one wave per NR new rows
        const double *Dsrc = src < 0 ? D : Sb[src];
        double *Ddst = Sb[src < 0 ? 0 : (src ^ 1)];
        const bool first = src < 0;
        const bool sq = first && method == 8;
        // entry (x, y) of the source matrix, any order (the pristine matrix is full, a scratch matrix holds min(x, y) -> max(x, y))
        // (Dsrc / Ddst are picked from three pointers at run time and the compiler no longer knows they are global: through plain pointers the
        // rows went out as FLAT loads and stores, which return out of order -- every one was waited for with vmcnt(0) lgkmcnt(0).)
        typedef __attribute__((address_space(1))) double gdouble;
        typedef const __attribute__((address_space(1))) double cgdouble;
        cgdouble *Gsrc = (cgdouble *)Dsrc;
        auto srcD = [&](int x, int y) -> double {
            const int lo_ = x < y ? x : y, hi_ = x < y ? y : x;
            const double v = Gsrc[static_cast<long long>(lo_) * nld + hi_];
            return sq ? v * v : v;
        };
        auto plain_rows = [&](auto NR_, auto SQ_, int A0) {
            constexpr int NR = decltype(NR_)::value;
            constexpr bool SQ = decltype(SQ_)::value;                        // ward.D2's first round: the pristine entries are squared on the way
            cgdouble *r[NR];
            gdouble *w[NR];
            double *stg[NR];
            unsigned long long mk[NR];                                       // the row's minimum so far, in integer order (exact)
            int ix[NR], ao[NR];
            unsigned tfm = 0u;                                               // bit t: row t has seen its minimum twice (a bit mask: an array indexed by t ends up in scratch memory)
#pragma unroll
            for (int t = 0; t < NR; ++t) {
                ao[t] = __builtin_amdgcn_readfirstlane(oldidx[A0 + t] & 0x7fff);
                r[t] = Gsrc + static_cast<long long>(ao[t]) * nld;
                w[t] = (gdouble *)(Ddst + static_cast<long long>(A0 + t) * nld);
                stg[t] = wstage + (static_cast<size_t>(wave) * stage_rows + t) * 2 * np;
                mk[t] = ~0ull; ix[t] = 0x7fffffff;
            }
            // The row's distances to the pair members -- entry (a, k) of row a, or (k, a) of row k left of the diagonal: scattered single
            // loads; the first 64 pairs' worth (all of them, after the first rounds) is asked for in front of the sweep (where the compiler
            // leaves them there, their latency hides behind it) and parked in the stage after it.
#ifdef SHARP_LAB_HT_TIMING
            const long long p0 = __builtin_readcyclecounter();
#endif
            constexpr int PF = 1;
            double gk[NR][PF], gl[NR][PF];
#pragma unroll
            for (int f = 0; f < PF; ++f) {
                const int q = lane + 64 * f;
                const int k1 = plist[q < np ? q : 0], l1 = partner[k1];
#pragma unroll
                for (int t = 0; t < NR; ++t) {
                    const int kl = k1 < ao[t] ? k1 : ao[t], kh = k1 < ao[t] ? ao[t] : k1;
                    const int ll = l1 < ao[t] ? l1 : ao[t], lh = l1 < ao[t] ? ao[t] : l1;
                    gk[t][f] = Gsrc[static_cast<long long>(kl) * nld + kh];
                    gl[t][f] = Gsrc[static_cast<long long>(ll) * nld + lh];
                }
            }
            // The old rows right of the diagonal, contiguous from a 64-byte boundary (ao[0] < ao[1]: the second row skips what lies left of
            // its own diagonal).  An entry of an unmerged column goes to its new column, is offered to that column and to the row's own
            // minimum; the pair members' entries are fetched after the sweep (they are in the lines the sweep has just read).
#ifdef SHARP_LAB_HT_TIMING
            const long long p1 = __builtin_readcyclecounter();
#endif
            int j0 = ((ao[0] + 1) & ~7) + lane;
            auto pass = [&](auto U_) {
                constexpr int U = decltype(U_)::value;
                for (; j0 + 64 * (U - 1) < na; j0 += 64 * U) {
                    unsigned cm[U];
                    double x[NR][U];
#pragma unroll
                    for (int u = 0; u < U; ++u) cm[u] = colmap[j0 + 64 * u];
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int t = 0; t < NR; ++t) x[t][u] = r[t][j0 + 64 * u];
                    // (all the loads of the pass are in flight -- the waves spend most of their time waiting for them --; the atomics go
                    // out two columns at a time, so that their keys and results do not cost the registers the loads need)
                    constexpr int G = U < 2 ? U : 2;
#pragma unroll
                    for (int u0 = 0; u0 < U; u0 += G) {
                        unsigned long long key[NR][G], old[NR][G];
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            const int u = u0 + g;
                            const int j = j0 + 64 * u;
                            const int B = static_cast<int>(cm[u]);
#pragma unroll
                            for (int t = 0; t < NR; ++t) {
                                key[t][g] = 0ull; old[t][g] = ~0ull;
                                if (cm[u] < 0x8000u && j > ao[t]) {
                                    const double v = SQ ? x[t][u] * x[t][u] : x[t][u];
                                    const unsigned long long o = ht_ord(v);
                                    key[t][g] = ht_key(o, A0 + t);
#ifdef SHARP_LAB_HT_NORTN           // (lab build: what waiting for the atomics' results costs -- near-ties of column candidates go unseen)
                                    (void)atomicMin(&colkey[B], key[t][g]);
#else
                                    old[t][g] = atomicMin(&colkey[B], key[t][g]);
#endif
                                    w[t][B] = v;
                                    if (o < mk[t]) { mk[t] = o; ix[t] = B; } else if (o == mk[t]) tfm |= 1u << t;
                                }
                            }
                        }
#pragma unroll
                        for (int g = 0; g < G; ++g)
#pragma unroll
                            for (int t = 0; t < NR; ++t) offer_check(old[t][g], key[t][g]);   // (a lane that offered nothing: ~0 ^ 0 is not below 2^16)
                    }
                    if (U == 1) break;
                }
            };
            pass(std::integral_constant<int, 8>());                          // (sixteen loads per lane in flight with two rows, eight with one)
            pass(std::integral_constant<int, 4>());
            pass(std::integral_constant<int, 2>());
            pass(std::integral_constant<int, 1>());
#ifdef SHARP_LAB_HT_TIMING
            const long long p2 = __builtin_readcyclecounter();
#endif
#pragma unroll
            for (int f = 0; f < PF; ++f) {
                const int q = lane + 64 * f;
                if (q < np) {
                    const int rk = pseq[plist[q]];
#pragma unroll
                    for (int t = 0; t < NR; ++t) {
                        stg[t][2 * rk] = SQ ? gk[t][f] * gk[t][f] : gk[t][f];
                        stg[t][2 * rk + 1] = SQ ? gl[t][f] * gl[t][f] : gl[t][f];
                    }
                }
            }
            for (int q = lane + 64 * PF; q < np; q += 64) {                 // (more than 128 pairs in a round: the rest, unhidden)
                const int k1 = plist[q], l1 = partner[k1], rk = pseq[k1];
#pragma unroll
                for (int t = 0; t < NR; ++t) {
#ifdef SHARP_LAB_HT_NOGATHER      // (lab build: what the pair members' gathers cost)
                    stg[t][2 * rk] = 1.0 + k1; stg[t][2 * rk + 1] = 1.0 + l1;
#else
                    stg[t][2 * rk] = srcD(k1, ao[t]);
                    stg[t][2 * rk + 1] = srcD(l1, ao[t]);
#endif
                }
            }
            // (the stage is written and read by this wave alone, and a wave's LDS operations execute in order: a compiler barrier is all the
            // ordering needed -- a release fence here also waited for every store of the sweep, 3.7 M cycles per task)
            asm volatile("" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
#ifdef SHARP_LAB_HT_TIMING
            const long long p3 = __builtin_readcyclecounter();
#endif
            double nr_[NR];
#pragma unroll
            for (int t = 0; t < NR; ++t) nr_[t] = csz[ao[t]];
            for (int B = ns + lane; B < nb; B += 64) {                      // merged columns: d(a, k u l) from d(a,k), d(a,l)
                const int rk = B - ns;
                const double nk_ = pinfo[rk], nl_ = pinfo[np + rk], hQ = pinfo[2 * np + rk];
                unsigned long long key[NR], old[NR];
#pragma unroll
                for (int t = 0; t < NR; ++t) {
                    const double v = lance_williams(method, stg[t][2 * rk], stg[t][2 * rk + 1], hQ, nk_, nl_, nr_[t]);
                    w[t][B] = v;
                    const unsigned long long o = ht_ord(v);
                    if (o < mk[t] || (o == mk[t] && B < ix[t])) { if (o == mk[t]) tfm |= 1u << t; mk[t] = o; ix[t] = B; } else if (o == mk[t]) tfm |= 1u << t;
                    key[t] = ht_key(o, A0 + t);
                    old[t] = atomicMin(&colkey[B], key[t]);
                }
#pragma unroll
                for (int t = 0; t < NR; ++t) offer_check(old[t], key[t]);
            }
            __builtin_amdgcn_wave_barrier();                                 // the stage is reused by this wave's next rows
#ifdef SHARP_LAB_HT_TIMING
            const long long p4 = __builtin_readcyclecounter();
            tt_pf += p1 - p0; tt_sweep += p2 - p1; tt_stash += p3 - p2; tt_mcol += p4 - p3;
#endif
#pragma unroll
            for (int t = 0; t < NR; ++t) {
                HrBest g;
                g.v = mk[t] == ~0ull ? HC_INF : ht_unord(mk[t]); g.i = ix[t]; g.tie = static_cast<int>((tfm >> t) & 1u);
                g = hr_wave(g);
                if (lane == 0) { cidN[A0 + t] = cid[ao[t]]; cszN[A0 + t] = csz[ao[t]]; dnnN[A0 + t] = g.v; }
                if (lane == 1) { nn[A0 + t] = static_cast<uint16_t>(g.i < nb ? g.i : 0); }
                if (lane == 2) { tie[A0 + t] = static_cast<unsigned char>(g.tie); }
            }
#ifdef SHARP_LAB_HT_TIMING
            tt_red += __builtin_readcyclecounter() - p4;
#endif
        };
        // a merged cluster's row: its entries against the merged clusters ranked after it (the four old entries of each from the source)
        auto merged_row = [&](int A) {
            const int a = __builtin_amdgcn_readfirstlane(oldidx[A] & 0x7fff);
            const int pa = __builtin_amdgcn_readfirstlane(partner[a]);
            gdouble *wr = (gdouble *)(Ddst + static_cast<long long>(A) * nld);
            const double na_ = csz[a], nj_ = csz[pa], hP = dnn[a];
            const int seqP = pseq[a];
            double mn = HC_INF, sc = HC_INF;
            int ix = 0x7fffffff;
            for (int B = A + 1 + lane; B < nb; B += 64) {
                const int k1 = oldidx[B] & 0x7fff, l1 = partner[k1];
                const double d00 = srcD(a, k1), d01 = srcD(a, l1), d10 = srcD(pa, k1), d11 = srcD(pa, l1);
                const double nk_ = csz[k1], nl_ = csz[l1], hQ = dnn[k1];
                double v;
                if (seqP < static_cast<int>(pseq[k1])) {                     // (a, j) merges first, then (k, l) against the merged cluster
                    const double t1 = lance_williams(method, d00, d10, hP, na_, nj_, nk_);
                    const double t2 = lance_williams(method, d01, d11, hP, na_, nj_, nl_);
                    v = lance_williams(method, t1, t2, hQ, nk_, nl_, na_ + nj_);
                } else {
                    const double t1 = lance_williams(method, d00, d01, hQ, nk_, nl_, na_);
                    const double t2 = lance_williams(method, d10, d11, hQ, nk_, nl_, nj_);
                    v = lance_williams(method, t1, t2, hP, na_, nj_, nk_ + nl_);
                }
                wr[B] = v;
                sc = fmin(sc, fmax(mn, v));
                if (v < mn || (v == mn && B < ix)) { mn = v; ix = B; }
                offer(B, v, A);
            }
            HrBest g;
            g.v = mn; g.i = ix; g.tie = 0;
            g = hr_wave(g);
            g.tie |= __ballot(sc == g.v) != 0ull ? 1 : 0;
            if (lane == 0) { cidN[A] = cid[a] < cid[pa] ? cid[a] : cid[pa]; cszN[A] = static_cast<uint16_t>(csz[a] + csz[pa]); dnnN[A] = g.v; }
            if (lane == 1) { nn[A] = static_cast<uint16_t>(g.i < nb ? g.i : 0); }
            if (lane == 2) { tie[A] = static_cast<unsigned char>(g.tie); }
        };
        // nn / tie of the NEW round are written here while phases (1)-(3) are done with the old ones and the rebuild reads neither: the
        // single-buffered arrays are free.  Rows are dealt to the waves round-robin: in the triangle a row is as long as its index is
        // low, so interleaved rows give every wave the same share (and the merged clusters' rows are short: n_p^2 / 2 entries in all).
        for (int q = wave * stage_rows; q < ns; q += nwave * stage_rows) {
            HT_GUARD(3);
            const bool two = stage_rows == 2 && q + 1 < ns;
            if (sq) { if (two) plain_rows(std::integral_constant<int, 2>(), std::true_type(), q); else plain_rows(std::integral_constant<int, 1>(), std::true_type(), q); }
            else    { if (two) plain_rows(std::integral_constant<int, 2>(), std::false_type(), q); else plain_rows(std::integral_constant<int, 1>(), std::false_type(), q); }
        }
#ifdef SHARP_LAB_HT_TIMING
        const long long m0 = __builtin_readcyclecounter();
#endif
        for (int q = wave; q < np; q += nwave) {
            HT_GUARD(4);
            merged_row(ns + q);
        }
#ifdef SHARP_LAB_HT_TIMING
        const long long m1 = __builtin_readcyclecounter();
        tt_mrow += m1 - m0;
#endif
        __syncthreads();
#ifdef SHARP_LAB_HT_TIMING
        tt_stash += 0; tt_r0 += 0;
        tt_combine -= 0;
        tt_bar += __builtin_readcyclecounter() - m1;
#endif
#ifdef SHARP_LAB_HT_TIMING
        const long long rc_ = __builtin_readcyclecounter();
        tt_rebuild += rc_ - rb;
#endif
        combine(Ddst, false, nb, dnnN, nn, tie);
        if (tid == 0) { ctl[0] = 0; }
        done += np; na = nb; cur ^= 1; src = src < 0 ? 0 : (src ^ 1);
        __syncthreads();
#ifdef SHARP_LAB_HT_TIMING
        tt_combine += __builtin_readcyclecounter() - rc_;
#endif
    }
    // (5) the sequential algorithm's order: ascending height, lowest index first; ward.D2 reports sqrt
    __syncthreads();
    {
        int npow2 = 1; while (npow2 < n - 1) npow2 <<= 1;
        double *kh = reinterpret_cast<double *>(sm);                        // the state is dead: reuse LDS (16 B per entry <= state size)
        int *ki = reinterpret_cast<int *>(kh + npow2);
        int *kj = ki + npow2;
        for (int q = tid; q < npow2; q += HT_THREADS) {
            if (q < n - 1) { kh[q] = crit[q]; ki[q] = ia[q]; kj[q] = ib[q]; } else { kh[q] = HC_INF; ki[q] = 0x7fffffff; kj[q] = 0; }
        }
        __syncthreads();
        for (int size = 2; size <= npow2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (npow2 >> 1); t += HT_THREADS) {
                    const int lo = ((t / stride) * stride * 2) + (t % stride), hi = lo + stride;
                    const bool up = ((lo & size) == 0);
                    const double x = kh[lo], y = kh[hi];
                    const bool gt = x > y || (x == y && ki[lo] > ki[hi]);
                    if (gt == up) {
                        kh[lo] = y; kh[hi] = x;
                        const int t1 = ki[lo]; ki[lo] = ki[hi]; ki[hi] = t1;
                        const int t2 = kj[lo]; kj[lo] = kj[hi]; kj[hi] = t2;
                    }
                }
                __syncthreads();
            }
        }
        for (int q = tid; q < n - 1; q += HT_THREADS) { crit[q] = method == 8 ? sqrt(kh[q]) : kh[q]; ia[q] = ki[q]; ib[q] = kj[q]; }
    }
#ifdef SHARP_LAB_HT_TIMING
    if (blockIdx.x == 0 && (tid == 0 || tid == 512))
        printf("tri n=%d wave %d: round0 %lld | setup %lld rebuild %lld combine %lld | wave rows: prefetch %lld sweep %lld stash %lld merged-cols %lld reduce %lld | merged rows %lld barrier %lld\n",
               n, wave, tt_r0, tt_setup, tt_rebuild, tt_combine, tt_pf, tt_sweep, tt_stash, tt_mcol, tt_red, tt_mrow, tt_bar);
#endif
    if (tid == 0) status[blockIdx.x] = 0;
}
