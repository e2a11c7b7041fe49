// hclust_front.inc -- a "lazy front" for the bulk-synchronous agglomeration (SHARP_HC_FRONT=1; an experiment behind a switch, round 5;
// included by hclust_agglo.hip; R/get_opt_hclust.R:76-83, SURVEY.md App. A.4).
//
// hclust_rnn_kernel rewrites the whole distance matrix every round (read n_a^2, write n_b^2) although a round merges only ~10 % of the
// clusters; the first four rounds of a 2000-observation task are 5.5 of the 10.2 n^2 entries it moves.  This kernel runs those first
// rounds WITHOUT rewriting anything: the pristine matrix D stays the "base part" of every original row, and a round only APPENDS --
//   * one new row per reciprocal pair (read the two members' rows, write one), into a side area NR;
//   * those rows transposed into the surviving rows' "tails" (a survivor's distances to the round's new clusters are then contiguous:
//     no survivor ever walks a column), the nearest-neighbour check of the new entries done on the fly;
//   * a rescan of the survivors whose nearest neighbour was merged (for a reducible linkage nobody else's can change);
// dead rows and columns are skipped through a per-column state word.  After `max_rounds` rounds (or when the side area is full) the
// alive clusters are compacted ONCE into S0 in the layout hclust_rnn_kernel uses, the state goes into that kernel's image, and its MODE 3
// (all remaining rounds in one launch) takes over.  Same pairs, same ranks, same Lance-Williams arithmetic per entry (the matrix is
// exactly symmetric, so an entry computed once and copied equals the entry the rewrite computes on both sides): same merges, same heights.
// Priced on the real round structure (tools/sim_lazy_agglomeration.py): four lazy rounds 3.1 n^2 + the compaction 1.3 against 5.5 for the
// rewrite, i.e. -10 % of a task's bytes with rescans by nearest neighbour only.  Exact ties abandon the task to the sequential kernel,
// as everywhere.
// MEASURED (cfg2, 375 tasks, SHARP_HC_FRONT=4; profiles/r05_hc_front.txt): every cutree level and every height identical to the rewrite
// (tests/test_hclust_gpu.py::test_lazy_front_and_full_rewrite_agglomeration_agree); HBM traffic 123.8 GB per step (front 62.3 read + 14.7
// written, MODE 3 for the rest 46.8) against 128.0 -- and 45.1 ms of agglomeration against 30.5, 65 ms per step against 51: the append-only
// rounds are bound by their own instruction streams (a column-state read and a Lance-Williams division per entry, four to eight loads in
// flight per lane, work dealt statically), not by the memory system.  Off by default; kept as the measured form of VERDICT r04 item 5.
// (The work loops are counted loops over wave-strided indices: the `for (;;) { q = atomicAdd(...); if (q >= bound) break; ... }` form with
// the bound read from LDS per lane left waves spinning in the rescan phase -- found with a host-visible progress buffer, not understood.)
constexpr int HF_THREADS = 1024;
constexpr uint16_t HF_DEAD = 0, HF_PLAIN = 1;          // column state; 0x8000 | (2 rank + member): a member of this round's pair `rank`

// the side area of a task inside its S1 scratch matrix (nld x nld doubles): tails of the n original rows (n x cap), then the new rows
// (cap x ldnr, ldnr = n + cap): the largest cap (a multiple of 8) with n cap + cap (n + cap) <= nld^2, at most n / 2
__host__ __device__ inline int hf_cap(int n, int nld) {
    int cap = (n / 2) & ~7;
    while (cap > 0 && static_cast<long long>(n) * cap + static_cast<long long>(cap) * (n + cap) > static_cast<long long>(nld) * nld) cap -= 8;
    return cap;
}
inline size_t hf_lds_bytes(int n, int nld) {
    const size_t L = static_cast<size_t>(n) + hf_cap(n, nld);
    return ((L * (8 + 8 + 2 * 8 + 2) + 64 + 15) / 16 * 16);
}

__global__ __launch_bounds__(HF_THREADS) void hclust_front_kernel(const HcMeta *__restrict__ metas, const double *__restrict__ Dall,
                                                                  double *__restrict__ S0all, double *__restrict__ S1all,
                                                                  int *__restrict__ ia_all, int *__restrict__ ib_all, double *__restrict__ h_all,
                                                                  int *__restrict__ status, unsigned char *__restrict__ images,
                                                                  long long image_stride, int max_rounds) {
    const HcMeta M = metas[blockIdx.x];
    const int n = M.n, nld = M.nld, method = M.method;
    const double *D = Dall + M.oD;
    double *S0 = S0all + M.oD, *S1 = S1all + M.oD;
    int *ia = ia_all + M.oM, *ib = ib_all + M.oM;
    double *crit = h_all + M.oM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int nwave = HF_THREADS / 64;
    unsigned char *img = images + static_cast<long long>(blockIdx.x) * image_stride;
    // hclust_rnn_kernel's state image (HR_THREADS = 1024: 16 waves): the arrays this kernel fills at its end
    struct Image { double *dnn; uint16_t *cid, *csz, *nn; unsigned char *tie; int *ctl; };
    const Image IM = [&]() {
        unsigned char *lds_cursor = img;
        HR_STATE_ARRAYS(LDS_CARVE, (n + 3) & ~3, 1024 / 64)
        return Image{dnnA, cidA, cszA, nn, tie, ctl};
    }();
    int *ictl = IM.ctl;
    const int cap = hf_cap(n, nld);
    auto abandon = [&]() {                                     // (every thread of the workgroup takes this exit together)
        if (tid == 0) { status[blockIdx.x] = 1; for (int q = 0; q < 16; ++q) ictl[q] = 0; ictl[10] = 1; }
    };
    if (method == 6 || method == 7 || n > HR_MAXN || n < 64 || cap < 64) { abandon(); return; }
    const int Lmax = n + cap, ldnr = n + cap;
    double *T = S1;                                             // tails of the original rows: T[c * cap + (x - n)]
    double *NR = S1 + static_cast<long long>(n) * cap;          // new rows: NR[(c - n) * ldnr + x]
    const bool sqD = method == 8;                               // ward.D2: the pristine matrix is squared on the fly, everything derived is squared

    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    double *dnn = reinterpret_cast<double *>(sm);               // [Lmax]  nearest-neighbour distance (= a pair's height)
    double *stash = dnn + Lmax;                                 // [Lmax]  minimum over a survivor's new entries of the round (for its rescan)
    uint16_t *nn = reinterpret_cast<uint16_t *>(stash + Lmax);  // [Lmax]
    uint16_t *cid = nn + Lmax;                                  // [Lmax]  smallest original member
    uint16_t *csz = cid + Lmax;                                 // [Lmax]  cluster size
    uint16_t *partner = csz + Lmax;                             // [Lmax]
    uint16_t *pseq = partner + Lmax;                            // [Lmax]  rank of the pair in the round
    uint16_t *col = pseq + Lmax;                                // [Lmax]  HF_DEAD / HF_PLAIN / pair member; in the compaction: the new index
    uint16_t *plist = col + Lmax;                               // [Lmax]  first members of the pairs; then: the rows to rescan
    uint16_t *stashi = plist + Lmax;                            // [Lmax]  which new cluster the stash is
    unsigned char *tie = reinterpret_cast<unsigned char *>(stashi + Lmax);   // [Lmax]
    unsigned char *alive = tie + Lmax;                          // [Lmax]
    int *ctl = reinterpret_cast<int *>(sm + ((alive + Lmax - sm + 15) & ~static_cast<long>(15)));   // [16]: 0 npairs, 1 abort, 2..4 work counters, 5 rescans

    // a stored row: its first n entries (against the original clusters) and its tail (against the new ones)
    struct Row { const double *bp, *tp; bool sq; };
    auto rowof = [&](int c) -> Row {
        Row r;
        if (c < n) { r.bp = D + static_cast<long long>(c) * nld; r.tp = T + static_cast<long long>(c) * cap; r.sq = sqD; }
        else { r.bp = NR + static_cast<long long>(c - n) * ldnr; r.tp = r.bp + n; r.sq = false; }
        return r;
    };
    auto get = [&](const Row &r, int x) -> double {
        if (x < n) { const double v = r.bp[x]; return r.sq ? v * v : v; }
        return r.tp[x - n];
    };
    auto tail_of = [&](int c) -> double * { return c < n ? T + static_cast<long long>(c) * cap : NR + static_cast<long long>(c - n) * ldnr + n; };

    for (int i = tid; i < Lmax; i += HF_THREADS) { alive[i] = i < n ? 1 : 0; tie[i] = 0; cid[i] = static_cast<uint16_t>(i); csz[i] = 1; }
    if (tid < 16) ctl[tid] = 0;
    __syncthreads();
    // round 0: nearest neighbours from the pristine matrix (as hclust_rnn_kernel)
    for (int a = wave; a < n; a += nwave) {
        const double *row = D + static_cast<long long>(a) * nld;
        HrBest b; b.v = HC_INF; b.i = 0x7fffffff; b.tie = 0;
        for (int j0 = lane; j0 < n; j0 += 64 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int j = j0 + 64 * u; v[u] = row[j < n ? j : n - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + 64 * u;
                if (j < n && j != a) {
                    const double x = sqD ? v[u] * v[u] : v[u];
                    if (x < b.v) { b.v = x; b.i = j; b.tie = 0; } else if (x == b.v) b.tie = 1;
                }
            }
        }
        b = hr_wave(b);
        if (lane == 0) { nn[a] = static_cast<uint16_t>(b.i < n ? b.i : 0); dnn[a] = b.v; tie[a] = static_cast<unsigned char>(b.tie); }
    }
    __syncthreads();

    int L = n, na = n, done = 0;
    for (int round = 0; round < max_rounds && na > 256; ++round) {
        // (1) reciprocal pairs
        for (int a = tid; a < L; a += HF_THREADS) {
            partner[a] = HR_NONE;
            if (alive[a] && tie[a]) ctl[1] = 1;
        }
        __syncthreads();
        for (int a = tid; a < L; a += HF_THREADS) {
            if (!alive[a]) continue;
            const int b = nn[a];
            if (b > a && alive[b] && nn[b] == a) {
                partner[a] = static_cast<uint16_t>(b); partner[b] = static_cast<uint16_t>(a);
                plist[atomicAdd(&ctl[0], 1)] = static_cast<uint16_t>(a);
            }
        }
        __syncthreads();
        const int np = __builtin_amdgcn_readfirstlane(ctl[0]);
        if (ctl[1] || np == 0) { abandon(); return; }          // a tie or no pair: the sequential kernel takes this task
        if (L - n + np > cap) {                                 // the side area is full: nothing of this round has been applied
            __syncthreads();
            if (tid == 0) ctl[0] = 0;
            __syncthreads();
            break;
        }
        // (2) rank of each pair by (height, lower original index) = the sequential algorithm's order; the merges go on record
        for (int q = tid; q < np; q += HF_THREADS) {
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
            crit[done + rank] = h;
        }
        __syncthreads();
        // (3) column states
        for (int x = tid; x < L; x += HF_THREADS) {
            uint16_t s = HF_DEAD;
            if (alive[x]) s = partner[x] == HR_NONE ? HF_PLAIN : static_cast<uint16_t>(0x8000u | (2u * pseq[x] + (partner[x] < x ? 1u : 0u)));
            col[x] = s;
        }
        if (tid == 0) { ctl[2] = 0; ctl[3] = 0; ctl[4] = 0; ctl[5] = 0; }
        __syncthreads();
        // (4) the new rows, one wave per pair: cluster t = L + rank; its entries against the plain columns and against the round's other
        // new clusters (rank order of the two merges decides the order of the two Lance-Williams steps, as in hclust_rnn_kernel)
        for (int q = wave; q < np; q += nwave) {                    // (pairs dealt to the waves in turn: every pair costs the same two row sweeps)
            const int a = __builtin_amdgcn_readfirstlane(static_cast<int>(plist[q]));
            const int j = __builtin_amdgcn_readfirstlane(static_cast<int>(partner[a]));
            const int seqP = pseq[a];
            const int t = L + seqP;
            const Row ra = rowof(a), rj = rowof(j);
            double *out = NR + static_cast<long long>(t - n) * ldnr;
            const double na_ = csz[a], nj_ = csz[j], hP = dnn[a];
            double mn = HC_INF, sc = HC_INF;
            int ix = 0x7fffffff;
            auto upd = [&](double v, int B) { sc = fmin(sc, fmax(mn, v)); if (v < mn) { mn = v; ix = B; } };
            for (int x0 = lane; x0 < L; x0 += 64 * 4) {
                unsigned cs[4];
                double xa[4], xj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int x = x0 + 64 * u;
                    const int xc = x < L ? x : L - 1;
                    cs[u] = x < L ? col[xc] : HF_DEAD;
                    xa[u] = get(ra, xc); xj[u] = get(rj, xc);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int x = x0 + 64 * u;
                    if (cs[u] == HF_PLAIN) {
                        const double v = lance_williams(method, xa[u], xj[u], hP, na_, nj_, static_cast<double>(csz[x]));
                        out[x] = v;
                        upd(v, x);
                    } else if ((cs[u] & 0x8001u) == 0x8000u && x != a) {     // the first member k of another pair (k, l)
                        const int l = partner[x];
                        const int seqQ = (cs[u] & 0x7fffu) >> 1;
                        const double d00 = xa[u], d10 = xj[u], d01 = get(ra, l), d11 = get(rj, l);
                        const double nk_ = csz[x], nl_ = csz[l], hQ = dnn[x];
                        double v;
                        if (seqP < seqQ) {                                     // (a, j) merges first, then (k, l) against the merged cluster
                            const double t1 = lance_williams(method, d00, d10, hP, na_, nj_, nk_);
                            const double t2 = lance_williams(method, d01, d11, hP, na_, nj_, nl_);
                            v = lance_williams(method, t1, t2, hQ, nk_, nl_, na_ + nj_);
                        } else {
                            const double t1 = lance_williams(method, d00, d01, hQ, nk_, nl_, na_);
                            const double t2 = lance_williams(method, d10, d11, hQ, nk_, nl_, nj_);
                            v = lance_williams(method, t1, t2, hP, na_, nj_, nk_ + nl_);
                        }
                        out[L + seqQ] = v;
                        upd(v, L + seqQ);
                    }
                }
            }
            HrBest g;
            g.v = mn; g.i = ix; g.tie = 0;
            g = hr_wave(g);
            g.tie |= __ballot(sc == g.v) != 0ull ? 1 : 0;                      // a lane saw the minimum twice
            if (lane == 0) {
                nn[t] = static_cast<uint16_t>(g.i < Lmax ? g.i : 0); dnn[t] = g.v; tie[t] = static_cast<unsigned char>(g.tie);
                cid[t] = cid[a] < cid[j] ? cid[a] : cid[j];
                csz[t] = static_cast<uint16_t>(csz[a] + csz[j]);
                out[t] = HC_INF;
            }
        }
        __syncthreads();
        // (5) the new rows transposed into the survivors' tails, 64 survivors per wave and eight new clusters per step (every lane writes 64
        // contiguous bytes of its row's tail); the minimum of a survivor's new entries falls out: if its nearest neighbour is still there the
        // check is done (a reducible update brings nothing closer: only an exact tie can appear), else it is stashed for the rescan
        for (int g0 = wave; g0 * 64 < L; g0 += nwave) {
            const int c = g0 * 64 + lane;
            const int cc = c < L ? c : L - 1;
            const bool plain = c < L && col[cc] == HF_PLAIN;
            double *dst = tail_of(cc) + (L - n);
            double mn = HC_INF;
            int ix = 0;
            bool dup = false;
            for (int r0 = 0; r0 < np; r0 += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int r = r0 + u < np ? r0 + u : np - 1; v[u] = NR[static_cast<long long>(L - n + r) * ldnr + cc]; }
                if (plain) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        if (r0 + u < np) {
                            dst[r0 + u] = v[u];
                            if (v[u] < mn) { mn = v[u]; ix = r0 + u; dup = false; } else if (v[u] == mn) dup = true;
                        }
                    }
                }
            }
            if (plain) {
                if (col[nn[c]] == HF_PLAIN) {                                  // the nearest neighbour survives
                    if (mn < dnn[c]) { dnn[c] = mn; nn[c] = static_cast<uint16_t>(L + ix); tie[c] = dup ? 1 : 0; }
                    else if (mn == dnn[c]) tie[c] = 1;
                } else {
                    stash[c] = mn; stashi[c] = static_cast<uint16_t>(L + ix); tie[c] = dup ? 1 : 0;
                    plist[atomicAdd(&ctl[5], 1)] = static_cast<uint16_t>(c);   // (the pairs' list has been consumed)
                }
            }
        }
        __syncthreads();
        // (6) the survivors whose nearest neighbour was merged: a sweep of the stored row over the plain columns, one wave per row
        const int nres = __builtin_amdgcn_readfirstlane(ctl[5]);
        for (int q = wave; q < nres; q += nwave) {
            const int c = __builtin_amdgcn_readfirstlane(static_cast<int>(plist[q]));
            const Row rc = rowof(c);
            double mn = HC_INF, sc = HC_INF;
            int ix = 0x7fffffff;
            for (int x0 = lane; x0 < L; x0 += 64 * 8) {
                unsigned cs[8];
                double xv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int x = x0 + 64 * u;
                    const int xc = x < L ? x : L - 1;
                    cs[u] = x < L ? col[xc] : HF_DEAD;
                    xv[u] = get(rc, xc);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int x = x0 + 64 * u;
                    if (cs[u] == HF_PLAIN && x != c) { sc = fmin(sc, fmax(mn, xv[u])); if (xv[u] < mn) { mn = xv[u]; ix = x; } }
                }
            }
            HrBest g;
            g.v = mn; g.i = ix; g.tie = 0;
            g = hr_wave(g);
            g.tie |= __ballot(sc == g.v) != 0ull ? 1 : 0;
            if (lane == 0) {
                const double sv = stash[c];
                if (sv < g.v) { dnn[c] = sv; nn[c] = stashi[c]; }              // (tie[c] already says whether the new entries tie among themselves)
                else { dnn[c] = g.v; nn[c] = static_cast<uint16_t>(g.i < Lmax ? g.i : 0); tie[c] = static_cast<unsigned char>(g.tie | (sv == g.v ? 1 : 0)); }
            }
        }
        __syncthreads();
        // (7) the round's merges take effect
        for (int x = tid; x < L; x += HF_THREADS)
            if (col[x] & 0x8000u) alive[x] = 0;
        for (int q = tid; q < np; q += HF_THREADS) alive[L + q] = 1;
        if (tid == 0) ctl[0] = 0;
        L += np; na -= np; done += np;
        __syncthreads();
    }

    // ---- compaction: the alive clusters, in id order (= the order hclust_rnn_kernel would have them in), into S0 and into its state image
    {
        const int chunk = (L + HF_THREADS - 1) / HF_THREADS;
        const int lo = tid * chunk, hi = lo + chunk < L ? lo + chunk : L;
        int cnt = 0;
        for (int x = lo; x < hi; ++x) cnt += alive[x] ? 1 : 0;
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t2 = __shfl_up(incl, d); incl += lane >= d ? t2 : 0; }
        int *wsum = ctl + 8;                                    // (ctl has 16 ints: 8 .. 15 hold the waves' partial counts two at a time)
        __syncthreads();
        if (lane == 63) reinterpret_cast<unsigned short *>(wsum)[wave] = static_cast<unsigned short>(incl);
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; ++w) base += reinterpret_cast<unsigned short *>(wsum)[w];
        int pos = base + incl - cnt;
        for (int x = lo; x < hi; ++x) { if (alive[x]) { col[x] = static_cast<uint16_t>(pos); plist[pos] = static_cast<uint16_t>(x); ++pos; } else col[x] = 0xffffu; }
        __syncthreads();
    }
    double *idnn = IM.dnn;
    uint16_t *icid = IM.cid, *icsz = IM.csz;
    uint16_t *inn = IM.nn;
    unsigned char *itie = IM.tie;
    for (int A = wave; A < na; A += nwave) {
        const int c = __builtin_amdgcn_readfirstlane(static_cast<int>(plist[A]));
        const Row rc = rowof(c);
        double *dst = S0 + static_cast<long long>(A) * nld;
        for (int x0 = lane; x0 < L; x0 += 64 * 8) {
            unsigned cs[8];
            double xv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int x = x0 + 64 * u;
                const int xc = x < L ? x : L - 1;
                cs[u] = x < L ? col[xc] : 0xffffu;
                xv[u] = get(rc, xc);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int x = x0 + 64 * u;
                if (cs[u] != 0xffffu) dst[cs[u]] = x == c ? HC_INF : xv[u];
            }
        }
        if (lane == 0) {
            idnn[A] = dnn[c]; icid[A] = cid[c]; icsz[A] = csz[c];
            inn[A] = col[nn[c]]; itie[A] = tie[c];
        }
    }
    if (tid == 0) {
        for (int q = 0; q < 16; ++q) ictl[q] = 0;
        ictl[5] = 0; ictl[6] = na; ictl[7] = done; ictl[8] = 1;   // cur = 0, the matrix is scratch 0, nothing pending: MODE 3 goes on from here
    }
}
