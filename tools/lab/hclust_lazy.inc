// hclust_lazy.inc -- included by hclust_agglo.hip (namespace sharp): the bulk-synchronous agglomeration WITHOUT a rewrite of the distance
// matrix in every round (row a4 of SURVEY.md 8; R/get_opt_hclust.R:76-83, stats::hclust restated as in hclust_kernel).
//
// hclust_rnn_kernel streams the whole matrix into a compacted copy in each of its ~45 rounds although a round merges only ~10 % of
// the clusters: 10.1 n^2 entries per task.  Here a round touches only
//   * the rows of the merged clusters: the pair's two rows are read, the new row is written where the pair's first member lived;
//   * the rows of unmerged clusters whose nearest neighbour was merged away: read once to find the new nearest neighbour
//     (a reducible update never brings a merged cluster closer to a third one than its parts were, so every other row keeps its
//     nearest neighbour -- the argument that makes the bulk rounds valid in the first place);
// and the columns are NOT patched: a row keeps the distances to the clusters that existed when it was last written (its stamp).
// A wave that reads a row copies it into its own LDS buffer and REPLAYS on it the merges of the rounds since the row's stamp -- the
// Lance-Williams updates the sequential algorithm applies to that row, round by round (the merges of one round touch disjoint
// entries) -- so every global access is a coalesced read or write of a whole row and the updates run in LDS.  When half of the
// slots are dead (or after HL_EMAX rounds) the live rows are written out compacted and a new epoch starts.
// Traffic: 5 - 6 n^2 entries per task instead of 10.1, same merges, heights equal to rounding.  Between two clusters merged in the
// same round the column's merge is applied first, then the row's (hclust_rnn_kernel orders the two by height): the two orders agree
// to rounding, like the orders across rounds.  Exact ties abandon the task to hclust_kernel as in hclust_rnn_kernel; the pristine
// matrix D is never written.

constexpr int HL_MAXN = 2048;        // LDS: 24 B per slot, 16 B per tree node (3/4 of the slots), 8 B per slot and wave (row buffers)
constexpr int HL_EMAX = 6;           // rounds per epoch at most
constexpr int HL_THREADS = 256;      // four waves, each with its own row buffer
constexpr int HL_ROWS = HL_MAXN / 64;   // entries of a row per lane
// Row pointers picked at run time (pristine matrix or a scratch matrix) are generic to the compiler, and generic (flat) loads count on
// lgkmcnt as well as vmcnt: every LDS wait would then also wait for the row loads in flight.  Global address space = global_load.
typedef __attribute__((address_space(1))) const double *hl_gcdp;
typedef __attribute__((address_space(1))) double *hl_gdp;

__global__ __launch_bounds__(HL_THREADS) void hclust_lazy_kernel(const HcMeta *__restrict__ metas, const double *__restrict__ Dall,
                                                                 double *__restrict__ S0all, double *__restrict__ S1all,
                                                                 int *__restrict__ ia_all, int *__restrict__ ib_all,
                                                                 double *__restrict__ h_all, int *__restrict__ status, int theta_pct) {
    const HcMeta M = metas[blockIdx.x];
    const int n = M.n, nld = M.nld, method = M.method;
    const double *D = Dall + M.oD;
    double *Sb[2] = {S0all + M.oD, S1all + M.oD};
    int *ia = ia_all + M.oM, *ib = ib_all + M.oM;
    double *crit = h_all + M.oM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int nwave = HL_THREADS / 64;
    if (method == 6 || method == 7 || n > HL_MAXN) {            // centroid / median are not reducible; large n: LDS
        if (tid == 0) status[blockIdx.x] = 1;
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int nal = (n + 63) & ~63, ncap = (3 * nal) / 4 + 4;
    int *ctl = reinterpret_cast<int *>(sm);                     // [8]: 0 npairs, 1 abort, 3 rows to rescan
    int *wsum = ctl + 8;                                        // [nwave + 1]
    int *estart = wsum + nwave + 1;                             // [HL_EMAX + 2] first tree node of each round of the epoch  (128 bytes in all)
    double *dnn = reinterpret_cast<double *>(sm + 128);         // [nal] nearest-neighbour distance of slot y (= the pair's height)
    double *nh = dnn + nal;                                     // [ncap] node: height
    double *rowbuf = nh + ncap;                                 // [nwave][nal] the row a wave is working on
    uint16_t *nn = reinterpret_cast<uint16_t *>(rowbuf + nwave * nal);   // [nal]
    uint16_t *csz = nn + nal;                                   // [nal] cluster size
    uint16_t *cid = csz + nal;                                  // [nal] smallest original member
    uint16_t *partner = cid + nal;                              // [nal]
    uint16_t *pseq = partner + nal;                             // [nal] rank of the pair in the round; compaction: old slot -> new slot
    uint16_t *jobs = pseq + nal;                                // [nal] pairs (first members), then the rows to rescan; compaction: live slots
    uint16_t *colinfo = jobs + nal;                             // [nal] per round: 0x8000 | size after the round for the columns that survive it
    uint16_t *nsl = colinfo + nal;                              // [ncap] node: slot of the first member (where the merged cluster lives) ...
    uint16_t *nsr = nsl + ncap;                                 //        ... and of the second (dies)
    uint16_t *nszl = nsr + ncap;                                //        their sizes
    uint16_t *nszr = nszl + ncap;
    unsigned char *stamp = reinterpret_cast<unsigned char *>(nszr + ncap);   // [nal] round of the epoch at which row y was written
    unsigned char *flags = stamp + nal;                         // [nal] 1 alive, 2 tie, 4 row lives in scratch 0 (epoch 0 only)

    for (int i = tid; i < n; i += HL_THREADS) { cid[i] = static_cast<uint16_t>(i); csz[i] = 1; stamp[i] = 0; flags[i] = 1; }
    if (tid == 0) { for (int q = 0; q < 8; ++q) ctl[q] = 0; estart[0] = 0; estart[1] = 0; }
    __syncthreads();
    const bool sq0 = method == 8;                               // ward.D2: the pristine matrix holds unsquared distances
    // round 0 nearest neighbours from the pristine matrix
    for (int a = wave; a < n; a += nwave) {
        const double *row = D + static_cast<long long>(a) * nld;
        HrBest b; b.v = HC_INF; b.i = 0x7fffffff; b.tie = 0;
        for (int j0 = lane; j0 < n; j0 += 64 * 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { const int j = j0 + 64 * u; v[u] = row[j < n ? j : n - 1]; }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = j0 + 64 * u;
                if (j < n && j != a) {
                    const double x = sq0 ? v[u] * v[u] : v[u];
                    if (x < b.v) { b.v = x; b.i = j; b.tie = 0; } else if (x == b.v) b.tie = 1;
                }
            }
        }
        b = hr_wave(b);
        if (lane == 0) { nn[a] = static_cast<uint16_t>(b.i < n ? b.i : 0); dnn[a] = b.v; if (b.tie) flags[a] |= 2; }
    }
    __syncthreads();

    int nc = n;                     // slots of the current epoch
    int na = n;                     // live clusters
    int ne = 0;                     // tree nodes of the epoch
    int round = 0;                  // rounds of the epoch so far (stamps)
    int done = 0;                   // merges so far
    int cur = -1;                   // buffer of the epoch's rows: -1 = D (+ scratch 0 for rewritten rows), else scratch index
    double *buf = rowbuf + wave * nal;
    auto row_of = [&](int y, bool &sq) -> const double * {      // where slot y's row lives (and whether it still holds unsquared input)
        if (cur < 0) {
            if (flags[y] & 4) { sq = false; return Sb[0] + static_cast<long long>(y) * nld; }
            sq = sq0; return D + static_cast<long long>(y) * nld;
        }
        sq = false; return Sb[cur] + static_cast<long long>(y) * nld;
    };
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // A row on its way into this wave's buffer: issue_row starts the loads of row y into registers (nothing waits for them), land_row
    // puts them into the buffer and brings the row (written at round `stamp[y]` of the epoch) up to date through round `upto`: the
    // merges of every later round applied in order (a round's merges are independent: one lane each).  A wave keeps the NEXT row's
    // loads in flight while it works on the current one (two register sets).
    auto issue_row = [&](int y, double (&x)[HL_ROWS]) {
        bool sq;
        hl_gcdp R = (hl_gcdp)row_of(y, sq);
        // groups of eight loads go out together (a guard per load made every load wait for the one before: 32 round trips per row);
        // the wave-uniform guard skips the groups beyond the epoch's slots
#pragma unroll
        for (int g = 0; g < HL_ROWS; g += 8)
            if (64 * g < nc) {
#pragma unroll
                for (int i = g; i < g + 8; ++i) { const int c = lane + 64 * i; x[i] = R[c < nc ? c : nc - 1]; }
            }
    };
    auto land_row = [&](int y, double (&x)[HL_ROWS], int upto) {
        bool sq;
        (void)row_of(y, sq);
        const double szrow = csz[y];
#pragma unroll
        for (int g = 0; g < HL_ROWS; g += 8)
            if (64 * g < nc) {
#pragma unroll
                for (int i = g; i < g + 8; ++i) { const int c = lane + 64 * i; if (c < nal) buf[c] = sq ? x[i] * x[i] : x[i]; }
            }
        wave_sync();
        for (int r = stamp[y] + 1; r <= upto; ++r) {
            for (int e = estart[r] + lane; e < estart[r + 1]; e += 64) {
                const int sl = nsl[e], sr = nsr[e];
                buf[sl] = lance_williams(method, buf[sl], buf[sr], nh[e], static_cast<double>(nszl[e]), static_cast<double>(nszr[e]), szrow);
            }
            wave_sync();
        }
    };
    double x0[HL_ROWS], x1[HL_ROWS];

#ifdef HL_TIMING
    long long tm_comp = 0, tm_setup = 0, tm_rows = 0, tm_tail = 0; int n_comp = 0, n_rows = 0;
#define HL_T(v) const long long v = __builtin_readcyclecounter()
#else
#define HL_T(v) do { } while (0)
#endif
    int guard = 0;
    while (na > 1) {
        HL_T(t_a);
        if (++guard > n + 8) {                                  // (every round merges at least one pair)
            if (tid == 0) status[blockIdx.x] = 1;
            return;
        }
        // ---- compaction: half of the slots dead, the epoch at its length bound, or the node table nearly full
        if (na * 100 < theta_pct * nc || round >= HL_EMAX || ne + na / 2 + 2 > ncap) {
            {   // new slots: the live ones in order
                const int chunk = (nc + HL_THREADS - 1) / HL_THREADS;
                const int lo = tid * chunk, hi = lo + chunk < nc ? lo + chunk : nc;
                int c = 0;
                for (int y = lo; y < hi; ++y) c += flags[y] & 1;
                int incl = c;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); incl += lane >= d ? t : 0; }
                if (lane == 63) wsum[wave] = incl;
                __syncthreads();
                if (tid == 0) { int run = 0; for (int w = 0; w < nwave; ++w) { const int t = wsum[w]; wsum[w] = run; run += t; } }
                __syncthreads();
                int pos = wsum[wave] + incl - c;
                for (int y = lo; y < hi; ++y) if (flags[y] & 1) { pseq[y] = static_cast<uint16_t>(pos); jobs[pos++] = static_cast<uint16_t>(y); }
                __syncthreads();
            }
            const int dst = cur < 0 ? 1 : (cur ^ 1);            // (epoch 0 keeps its rewritten rows in scratch 0)
            {
                auto crow = [&](int q, double (&xc)[HL_ROWS], double (&xn)[HL_ROWS]) {
                    if (q + nwave < na) issue_row(jobs[q + nwave], xn);
                    land_row(jobs[q], xc, round);
                    hl_gdp wr = (hl_gdp)(Sb[dst] + static_cast<long long>(q) * nld);
                    for (int X = lane; X < na; X += 64) wr[X] = X == q ? HC_INF : buf[jobs[X]];
                    wave_sync();                                 // the buffer is reused by this wave's next row
                };
                if (wave < na) issue_row(jobs[wave], x0);
                for (int q = wave; q < na; q += 2 * nwave) {
                    crow(q, x0, x1);
                    if (q + nwave < na) crow(q + nwave, x1, x0);
                }
            }
            __syncthreads();
            // the per-slot state moves to the new slots (through the row buffers, dead until the next round)
            {
                double *t_dnn = rowbuf;
                uint16_t *t_nn = reinterpret_cast<uint16_t *>(rowbuf + nal), *t_csz = t_nn + nal, *t_cid = t_csz + nal;
                unsigned char *t_fl = reinterpret_cast<unsigned char *>(t_cid + nal);
                for (int y = tid; y < nc; y += HL_THREADS)
                    if (flags[y] & 1) {
                        const int Y = pseq[y];
                        t_dnn[Y] = dnn[y]; t_nn[Y] = pseq[nn[y]]; t_csz[Y] = csz[y]; t_cid[Y] = cid[y]; t_fl[Y] = flags[y] & 3;
                    }
                __syncthreads();
                for (int Y = tid; Y < na; Y += HL_THREADS) { dnn[Y] = t_dnn[Y]; nn[Y] = t_nn[Y]; csz[Y] = t_csz[Y]; cid[Y] = t_cid[Y]; flags[Y] = t_fl[Y]; stamp[Y] = 0; }
            }
            nc = na; ne = 0; round = 0; cur = dst;
            if (tid == 0) { estart[0] = 0; estart[1] = 0; }
            __syncthreads();
        }
        ++round;
        HL_T(t_b);
        // ---- (1) reciprocal pairs
        for (int a = tid; a < nc; a += HL_THREADS) {
            partner[a] = HR_NONE;
            if ((flags[a] & 3) == 3) ctl[1] = 1;                // an exact tie for a nearest neighbour: the sequential kernel takes the task
        }
        if (tid == 0) { ctl[0] = 0; ctl[3] = 0; }
        __syncthreads();
        for (int a = tid; a < nc; a += HL_THREADS) {
            if (!(flags[a] & 1)) continue;
            const int b = nn[a];
            if (b > a && nn[b] == a) {
                partner[a] = static_cast<uint16_t>(b); partner[b] = static_cast<uint16_t>(a);
                jobs[atomicAdd(&ctl[0], 1)] = static_cast<uint16_t>(a);
            }
        }
        __syncthreads();
        const int np = ctl[0];
        if (ctl[1] || np == 0) {
            if (tid == 0) status[blockIdx.x] = 1;
            return;
        }
        // ---- (2) rank of each pair by (height, lower original index) = the sequential algorithm's order; its tree node
        for (int q = tid; q < np; q += HL_THREADS) {
            const int a = jobs[q], j = partner[a];
            const double h = dnn[a];
            const int ida = cid[a] < cid[j] ? cid[a] : cid[j];
            int rank = 0;
            for (int q2 = 0; q2 < np; ++q2) {
                const int a2 = jobs[q2];
                const double h2 = dnn[a2];
                const int id2 = cid[a2] < cid[partner[a2]] ? cid[a2] : cid[partner[a2]];
                rank += (h2 < h || (h2 == h && id2 < ida)) ? 1 : 0;
            }
            pseq[a] = static_cast<uint16_t>(rank); pseq[j] = static_cast<uint16_t>(rank);
            ia[done + rank] = ida + 1; ib[done + rank] = (cid[a] < cid[j] ? cid[j] : cid[a]) + 1;
            crit[done + rank] = h;                               // squared for ward.D2 until the final pass
            const int e = ne + rank;                             // the merged cluster lives in slot a (a < j)
            nsl[e] = static_cast<uint16_t>(a); nsr[e] = static_cast<uint16_t>(j); nszl[e] = csz[a]; nszr[e] = csz[j]; nh[e] = h;
        }
        if (tid == 0) estart[round + 1] = ne + np;               // (estart[round] = ne: set when the previous round ended)
        __syncthreads();
        // ---- (3) the columns that survive the round (with the size they will have), and the rows to rescan (unmerged, nearest
        // neighbour merged away)
        for (int y = tid; y < nc; y += HL_THREADS) {
            uint16_t ci = 0;
            if (flags[y] & 1) {
                const int py = partner[y];
                if (py == HR_NONE) {
                    ci = static_cast<uint16_t>(0x8000u | csz[y]);
                    if (partner[nn[y]] != HR_NONE) jobs[np + atomicAdd(&ctl[3], 1)] = static_cast<uint16_t>(y);
                } else if (y < py) ci = static_cast<uint16_t>(0x8000u | (csz[y] + csz[py]));
            }
            colinfo[y] = ci;
        }
        __syncthreads();
        const int nresc = ctl[3];
        HL_T(t_c);
        // ---- (4) the rows: merged clusters (two old rows each), then rescans; a wave takes every nwave-th job and walks through its rows
        // with the next row's loads in flight
        {
            const int njobs = np + nresc;
            const int mjobs = wave < np ? (np - wave + nwave - 1) / nwave : 0;      // this wave's merged jobs
            const int ajobs = wave < njobs ? (njobs - wave + nwave - 1) / nwave : 0;
            const int F = ajobs + mjobs;                                             // rows this wave fetches
            auto row_at = [&](int s2) -> int {                                       // the s2-th row of this wave
                if (s2 < 2 * mjobs) { const int a = jobs[wave + nwave * (s2 >> 1)]; return (s2 & 1) ? static_cast<int>(partner[a]) : a; }
                return jobs[wave + nwave * (s2 - mjobs)];
            };
            HrBest best; best.v = HC_INF; best.i = 0x7fffffff; best.tie = 0;
            auto consider = [&](double v, int B) {
                if (v < best.v || (v == best.v && B < best.i)) { best.tie = (v == best.v) ? 1 : 0; best.v = v; best.i = B; }
                else if (v == best.v && B != best.i) best.tie = 1;
            };
            auto finish_job = [&](int a) {
                wave_sync();                                     // the buffer is reused by this wave's next row
                best = hr_wave(best);
                if (lane == 0) {
                    dnn[a] = best.v; nn[a] = static_cast<uint16_t>(best.i < nc ? best.i : 0);
                    flags[a] = static_cast<unsigned char>((flags[a] & ~2) | ((na - np > 2 && best.tie) ? 2 : 0));
                }
                best.v = HC_INF; best.i = 0x7fffffff; best.tie = 0;
            };
            double va[HL_ROWS];
            auto step = [&](int s2, double (&xc)[HL_ROWS], double (&xn)[HL_ROWS]) {
                const int y = __builtin_amdgcn_readfirstlane(row_at(s2));
                if (s2 + 1 < F) issue_row(__builtin_amdgcn_readfirstlane(row_at(s2 + 1)), xn);
                land_row(y, xc, round);
                if (s2 < 2 * mjobs) {
                    if (!(s2 & 1)) {
                        // first old row of a merged pair, brought up to date INCLUDING this round's other merges: kept in registers
#pragma unroll
                        for (int g = 0; g < HL_ROWS; g += 8)
                            if (64 * g < nc) {
#pragma unroll
                                for (int i = g; i < g + 8; ++i) { const int c = lane + 64 * i; va[i] = buf[c < nal ? c : 0]; }
                            }
                        wave_sync();
                    } else {
                        // second old row: the row of the merged cluster a u j, written where a lived (scratch 0 in epoch 0: D stays
                        // pristine; in place later)
                        const int a = __builtin_amdgcn_readfirstlane(static_cast<int>(partner[y]));
                        const double sza = csz[a], szj = csz[y], hP = dnn[a];
                        hl_gdp wr = (hl_gdp)((cur < 0 ? Sb[0] : Sb[cur]) + static_cast<long long>(a) * nld);
#pragma unroll
                        for (int g = 0; g < HL_ROWS; g += 8)
                            if (64 * g < nc) {
#pragma unroll
                                for (int i = g; i < g + 8; ++i) {
                                    const int c = lane + 64 * i;
                                    const unsigned ci = c < nc ? colinfo[c] : 0u;
                                    if ((ci & 0x8000u) && c != a) {
                                        const double val = lance_williams(method, va[i], buf[c], hP, sza, szj, static_cast<double>(ci & 0x7fffu));
                                        wr[c] = val;
                                        consider(val, c);
                                    }
                                }
                            }
                        finish_job(a);
                    }
                } else {
                    // an unmerged cluster whose nearest neighbour was merged away: its row is read, nothing is written
                    for (int c = lane; c < nc; c += 64)
                        if ((colinfo[c] & 0x8000u) && c != y) consider(buf[c], c);
                    finish_job(y);
                }
            };
            if (F > 0) issue_row(__builtin_amdgcn_readfirstlane(row_at(0)), x0);
            for (int s2 = 0; s2 < F; s2 += 2) {
                step(s2, x0, x1);
                if (s2 + 1 < F) step(s2 + 1, x1, x0);
            }
        }
        __syncthreads();
        HL_T(t_d);
        // ---- (5) the round's transition
        for (int y = tid; y < nc; y += HL_THREADS) {
            const unsigned char f = flags[y];
            if (!(f & 1)) continue;
            const int py = partner[y];
            if (py == HR_NONE) continue;
            if (y > py) { flags[y] = 0; continue; }                // the pair's second member: its slot dies
            csz[y] = static_cast<uint16_t>(csz[y] + csz[py]);       // the merged cluster keeps the smaller original index as its name
            cid[y] = cid[y] < cid[py] ? cid[y] : cid[py];
            stamp[y] = static_cast<unsigned char>(round);
            if (cur < 0) flags[y] = f | 4;
        }
        done += np; na -= np; ne += np;
        __syncthreads();
#ifdef HL_TIMING
        { const long long t_e = __builtin_readcyclecounter(); tm_comp += t_b - t_a; tm_setup += t_c - t_b; tm_rows += t_d - t_c; tm_tail += t_e - t_d;
          n_comp += (t_b - t_a) > 2000; n_rows += 2 * np + nresc; }
#endif
    }
#ifdef HL_TIMING
    if (blockIdx.x == 0 && tid == 0)
        printf("lazy task 0 (n %d): rounds %d, compactions %d: %lld cyc; setup %lld; rows %lld (%d row fetches); tail %lld\n", n, guard, n_comp, tm_comp,
               tm_setup, tm_rows, n_rows, tm_tail);
#endif
    // ---- the sequential algorithm's order: ascending height, lowest index first; ward.D2 reports sqrt
    __syncthreads();
    {
        int npow2 = 1; while (npow2 < n - 1) npow2 <<= 1;
        double *kh = reinterpret_cast<double *>(sm);            // the state is dead: reuse LDS (16 B per entry <= state size)
        int *ki = reinterpret_cast<int *>(kh + npow2);
        int *kj = ki + npow2;
        for (int q = tid; q < npow2; q += HL_THREADS) {
            if (q < n - 1) { kh[q] = crit[q]; ki[q] = ia[q]; kj[q] = ib[q]; } else { kh[q] = HC_INF; ki[q] = 0x7fffffff; kj[q] = 0; }
        }
        __syncthreads();
        for (int size = 2; size <= npow2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (npow2 >> 1); t += HL_THREADS) {
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
        for (int q = tid; q < n - 1; q += HL_THREADS) { crit[q] = method == 8 ? sqrt(kh[q]) : kh[q]; ia[q] = ki[q]; ib[q] = kj[q]; }
    }
    if (tid == 0) status[blockIdx.x] = 0;
}

inline size_t hclust_lazy_lds(int max_n) {
    const size_t nal = (static_cast<size_t>(max_n) + 63) & ~static_cast<size_t>(63), ncap = (3 * nal) / 4 + 4;
    int npow2 = 1; while (npow2 < max_n - 1) npow2 <<= 1;
    const size_t state = 128 + nal * (8 + 2 * 7 + 2) + ncap * (8 + 2 * 4) + (HL_THREADS / 64) * nal * 8 + 64;
    return (std::max(state, static_cast<size_t>(npow2) * 16) + 15) / 16 * 16;
}
