// knn_descent.hip -- the approximate k-NN of DESIGN.md §16: a start from T sorted random projections, then NN-descent joins in a
// bulk-synchronous gather form (no atomics on anything a result depends on: the only atomic is the integer count of changed entries).
//
// A top-K list is a set operation here: knn_offer_set refuses a candidate the list already holds, so offering a row twice, or in another
// order, changes nothing, and a pair's distance is always the direct sum (x_i - x_j)^2 in column order (tile_dist; the build has
// -ffp-contract=off).  The lists are therefore a pure function of (X, K, the parameters, seed), whatever the launch split, the tile
// filling or the lossy duplicate filter of the join do.
//
// lex_less, wave_sync and the rank step are knn_dev.hpp's; mix64, iota and the sorts are graph.hpp's.
#include "knn_descent.hpp"
#include "graph_prim.hpp"
#include "knn.hpp"
#include "knn_dev.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>

namespace sharp {
namespace {

constexpr int KD_PC = 16;              // columns per panel of the gathered tile
constexpr int KD_TS = KD_PC + 1;       // doubles per tile row (odd: lane l reads row l without bank conflicts inside a half wave)
constexpr int KD_Q = 128;              // the join's candidate queue: below 64 waiting + at most 64 new
constexpr int KD_HASH = 512;           // slots of the join's per-row "already offered in this join" filter
constexpr int KD_MAXT = 32;            // projections
constexpr double KD_XMAX = 1.0e100;    // |x| above this is refused: squared distances and projections stay finite below it
constexpr unsigned long long KD_GOLD = 0x9E3779B97F4A7C15ull;

// One wave's share of the workgroup's LDS: the row's list, the gathered tile, the row's own panel, the candidate queue and (join only)
// the filter.  Bounded by K and the tile, never by d.
struct WaveLds {
    double *Ld, *tile, *xpan;
    int *Li, *q, *hash;
};
__host__ __device__ inline int lds_ints(int K, bool with_hash) { return ((K + 1) & ~1) + KD_Q + (with_hash ? KD_HASH : 0); }
__host__ __device__ inline size_t wave_lds_bytes(int K, bool with_hash) {
    return sizeof(double) * (K + 64 * KD_TS + KD_PC) + sizeof(int) * lds_ints(K, with_hash);
}
__device__ __forceinline__ WaveLds wave_lds(unsigned char *smem, int K, bool with_hash, int wave) {
    unsigned char *base = smem + wave * wave_lds_bytes(K, with_hash);
    WaveLds w;
    w.Ld = reinterpret_cast<double *>(base);
    w.tile = w.Ld + K;
    w.xpan = w.tile + 64 * KD_TS;
    w.Li = reinterpret_cast<int *>(w.xpan + KD_PC);
    w.q = w.Li + ((K + 1) & ~1);
    w.hash = w.q + KD_Q;
    return w;
}

// Squared distances of row i to the (up to) 64 rows named in q[0 .. 64) (-1: none), lane l its own: the rows are gathered by index into
// the LDS tile, a panel of KD_PC columns at a time -- lanes 16 r .. 16 r + 15 read consecutive values of one row --, and every lane
// then runs s += (x_i[c] - x_j[c])^2 over the panel's columns in order, the partial sum carried from panel to panel.
__device__ __forceinline__ double tile_dist(const double *__restrict__ X, int d, long long i, const WaveLds &w, int lane) {
    const int mine = w.q[lane];
    const int col = lane & (KD_PC - 1), rsub = lane >> 4;
    double s = 0.0;
    for (int c0 = 0; c0 < d; c0 += KD_PC) {
        const int pc = d - c0 < KD_PC ? d - c0 : KD_PC;
        if (lane < pc) w.xpan[lane] = X[i * d + c0 + lane];
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int j = w.q[4 * k + rsub];
            v[k] = (col < pc && j >= 0) ? X[static_cast<long long>(j) * d + c0 + col] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) w.tile[(4 * k + rsub) * KD_TS + col] = v[k];
        wave_sync();
        if (mine >= 0)
            for (int c = 0; c < pc; ++c) {
                const double t = w.xpan[c] - w.tile[lane * KD_TS + c];
                s += t * t;
            }
        wave_sync();
    }
    return s;
}

// knn_offer (knn_dev.hpp) with the membership test a set needs: a candidate whose index the list already holds is dropped.  A pair's
// distance is a function of the pair, so a member would come with the bits it is stored with.
// It keeps its own argmax tail: built on a tail shared with knn_offer, the join and offer kernels compiled to another instruction
// stream (profiles/knn_home_kernels.txt).
__device__ __forceinline__ void knn_offer_set(double v, int ci, bool valid, double *Ld, int *Li, int K, int lane, double &thr, int &widx,
                                              int &wpos) {
    unsigned long long m = __ballot(valid && lex_less(v, ci, thr, widx));
    while (m) {
        const int bsel = __ffsll(static_cast<long long>(m)) - 1;
        m &= m - 1;
        const double vb = __shfl(v, bsel);
        const int ib = __shfl(ci, bsel);
        if (!lex_less(vb, ib, thr, widx)) continue;
        bool member = false;
        for (int p = lane; p < K; p += 64) member |= Li[p] == ib;
        if (__any(member)) continue;
        if (lane == 0) { Ld[wpos] = vb; Li[wpos] = ib; }
        wave_sync();
        double bd = -1.0;
        int bi = -1, bp = 0;
        for (int p = lane; p < K; p += 64) {
            const double dv = Ld[p];
            const int iv = Li[p];
            if (lex_less(bd, bi, dv, iv)) { bd = dv; bi = iv; bp = p; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(bd, off);
            const int oi = __shfl_xor(bi, off), op = __shfl_xor(bp, off);
            if (lex_less(bd, bi, od, oi)) { bd = od; bi = oi; bp = op; }
        }
        thr = bd;
        widx = bi;
        wpos = __shfl(bp, 0);
    }
}

// the row's list, ranked by (distance, index), to out_idx / out_dist
__device__ __forceinline__ void write_ranked(const double *Ld, const int *Li, int K, long long i, int lane, int *__restrict__ out_idx,
                                             double *__restrict__ out_dist) {
    for (int p = lane; p < K; p += 64) {
        const double dp = Ld[p];
        const int ip = Li[p], rank = knn_rank(Ld, Li, K, dp, ip);
        out_idx[i * K + rank] = ip;
        out_dist[i * K + rank] = dp;
    }
}

__device__ __forceinline__ unsigned long long sortable(double p) {
    if (p == 0.0) p = 0.0;   // (-0 sorts with +0)
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(p));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// keys[t n + i] = the sortable image of p_t[i] = sum_c x_ic r_t[c], column after column: one pass over X for all T directions
__global__ __launch_bounds__(256) void kd_project_kernel(const double *__restrict__ X, long long n, int d, const double *__restrict__ R, int T,
                                                         unsigned long long *__restrict__ keys) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double p[KD_MAXT];
#pragma unroll
    for (int t = 0; t < KD_MAXT; ++t) p[t] = 0.0;
    for (int c = 0; c < d; ++c) {
        const double x = X[i * d + c];
#pragma unroll
        for (int t = 0; t < KD_MAXT; ++t)
            if (t < T) p[t] += x * R[static_cast<long long>(t) * d + c];
    }
#pragma unroll
    for (int t = 0; t < KD_MAXT; ++t)
        if (t < T) keys[static_cast<long long>(t) * n + i] = sortable(p[t]);
}

// pos[t n + order[t n + p]] = p
__global__ __launch_bounds__(256) void kd_pos_kernel(const int *__restrict__ order, long long n, long long total, int *__restrict__ pos) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= total) return;
    const long long t = e / n;
    pos[t * n + order[e]] = static_cast<int>(e - t * n);
}

// One wave per row i of the launch, from an empty list.  WINDOWS: the row is offered, for each of the T orders, the W rows on either
// side of its own position.  Otherwise: the K rows lists[i K ..] name.  The list leaves ranked by (distance, index).
template <bool WINDOWS>
__global__ __launch_bounds__(256) void kd_offer_kernel(const double *__restrict__ X, long long n, int d, int K, long long row0, long long rows,
                                                       const int *__restrict__ order, const int *__restrict__ pos, int T, int W,
                                                       const int *__restrict__ lists, int *__restrict__ out_idx,
                                                       double *__restrict__ out_dist) {
    extern __shared__ unsigned char kd_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = static_cast<long long>(blockIdx.x) * 4 + wave, i = row0 + r;
    if (r >= rows || i >= n) return;   // (waves are independent: no workgroup barrier below)
    const WaveLds w = wave_lds(kd_smem, K, false, wave);
    for (int p = lane; p < K; p += 64) { w.Ld[p] = KNN_INF; w.Li[p] = INT_MAX; }
    wave_sync();
    double thr = KNN_INF;
    int widx = INT_MAX, wpos = 0;
    if (WINDOWS) {
        for (int t = 0; t < T; ++t) {
            const long long p = pos[static_cast<long long>(t) * n + i];
            const long long lo = p - W > 0 ? p - W : 0, hi = p + W < n - 1 ? p + W : n - 1;
            for (long long b = lo; b <= hi; b += 64) {
                const long long q = b + lane;
                const int cand = (q <= hi && q != p) ? order[static_cast<long long>(t) * n + q] : -1;
                w.q[lane] = cand;
                wave_sync();
                const double s = tile_dist(X, d, i, w, lane);
                knn_offer_set(s, cand, cand >= 0, w.Ld, w.Li, K, lane, thr, widx, wpos);
            }
        }
    } else {
        for (int b = 0; b < K; b += 64) {
            const int cand = b + lane < K ? lists[i * K + b + lane] : -1;
            w.q[lane] = cand;
            wave_sync();
            const double s = tile_dist(X, d, i, w, lane);
            knn_offer_set(s, cand, cand >= 0, w.Ld, w.Li, K, lane, thr, widx, wpos);
        }
    }
    wave_sync();
    write_ranked(w.Ld, w.Li, K, i, lane, out_idx, out_dist);
}

// keys[e] = (target << 32 | hashed priority of (seed, iteration, target, source)), vals[e] = source, e = source K + slot: in source order,
// so a stable sort leaves equal priorities of one target by the lower source
__global__ __launch_bounds__(256) void kd_revkey_kernel(const int *__restrict__ idx, long long ne, int K, unsigned long long base,
                                                        unsigned long long *__restrict__ keys, int *__restrict__ vals) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= ne) return;
    const unsigned long long v = static_cast<unsigned long long>(e / K), u = static_cast<unsigned long long>(idx[e]);
    keys[e] = (u << 32) | (mix64(mix64(base + u) + v) >> 32);
    vals[e] = static_cast<int>(v);
}

// start[u] = the first sorted entry whose target is u (start holds -1 where there is none)
__global__ __launch_bounds__(256) void kd_segstart_kernel(const unsigned long long *__restrict__ keys, long long ne, long long *__restrict__ start) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= ne) return;
    const unsigned long long t = keys[e] >> 32;
    if (e == 0 || (keys[e - 1] >> 32) != t) start[t] = e;
}

// A(u) = the first Sf forward neighbours of u, then its (at most S) reverse neighbours of lowest priority: A[u SA ..], Acnt[u]
__global__ __launch_bounds__(256) void kd_candidates_kernel(const int *__restrict__ idx, const unsigned long long *__restrict__ keys,
                                                            const int *__restrict__ vals, const long long *__restrict__ start, long long n,
                                                            long long ne, int K, int Sf, int S, int *__restrict__ A, int *__restrict__ Acnt) {
    const long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (u >= n) return;
    const int SA = Sf + S;
    int cnt = 0;
    for (; cnt < Sf; ++cnt) A[u * SA + cnt] = idx[u * K + cnt];
    const long long s = start[u];
    if (s >= 0)
        for (long long e = s; e < ne && e < s + S && (keys[e] >> 32) == static_cast<unsigned long long>(u); ++e) A[u * SA + cnt++] = vals[e];
    Acnt[u] = cnt;
}

// The join, one wave per row i of the launch.  The row's list starts as its old (sorted) list.  The rows of A(u), u in A(i), and of
// A(i) itself pass two filters that can only drop what the list cannot gain -- a lossy per-row table of rows already queued in this
// join, and the list's own members -- and the rest is compacted into a queue; every full 64 of it is gathered into the LDS tile,
// measured and offered.  The new list leaves ranked, and the entries the old list did not hold are counted (updates[0]; updates[1]: the
// rows gathered, for the benchmark).
__global__ __launch_bounds__(256) void kd_join_kernel(const double *__restrict__ X, long long n, int d, int K, long long row0, long long rows,
                                                      int SA, const int *__restrict__ A, const int *__restrict__ Acnt,
                                                      const int *__restrict__ idx_old, const double *__restrict__ dist_old,
                                                      int *__restrict__ idx_new, double *__restrict__ dist_new,
                                                      unsigned long long *__restrict__ updates) {
    extern __shared__ unsigned char kd_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = static_cast<long long>(blockIdx.x) * 4 + wave, i = row0 + r;
    if (r >= rows || i >= n) return;   // (waves are independent: no workgroup barrier below)
    const WaveLds w = wave_lds(kd_smem, K, true, wave);
    for (int p = lane; p < K; p += 64) { w.Ld[p] = dist_old[i * K + p]; w.Li[p] = idx_old[i * K + p]; }
    for (int p = lane; p < KD_HASH; p += 64) w.hash[p] = -1;
    wave_sync();
    double thr = w.Ld[K - 1];
    int widx = w.Li[K - 1], wpos = K - 1;
    int qn = 0, gathered = 0;
    const int ci = Acnt[i];
    for (int a = 0; a <= ci; ++a) {
        const long long u = a < ci ? A[i * SA + a] : i;
        const int cu = Acnt[u];
        for (int e0 = 0; e0 < cu; e0 += 64) {
            const int cand = e0 + lane < cu ? A[u * SA + e0 + lane] : -1;
            bool keep = cand >= 0 && cand != i;
            if (keep) {
                const unsigned h = (static_cast<unsigned>(cand) * 2654435761u) >> 23;   // 512 slots
                if (w.hash[h] == cand) keep = false;
                else w.hash[h] = cand;
            }
            if (keep)
                for (int p = 0; p < K; ++p)
                    if (w.Li[p] == cand) { keep = false; break; }
            const unsigned long long m = __ballot(keep);
            if (keep) w.q[qn + __popcll(m & ((1ull << lane) - 1ull))] = cand;
            qn += __popcll(m);
            wave_sync();
            if (qn >= 64) {
                const int cq = w.q[lane];
                const double s = tile_dist(X, d, i, w, lane);
                knn_offer_set(s, cq, true, w.Ld, w.Li, K, lane, thr, widx, wpos);
                gathered += 64;
                const int moved = lane < qn - 64 ? w.q[64 + lane] : -1;
                wave_sync();
                w.q[lane] = moved;
                qn -= 64;
                wave_sync();
            }
        }
    }
    if (qn > 0) {
        if (lane >= qn) w.q[lane] = -1;
        wave_sync();
        const int cq = w.q[lane];
        const double s = tile_dist(X, d, i, w, lane);
        knn_offer_set(s, cq, cq >= 0, w.Ld, w.Li, K, lane, thr, widx, wpos);
        gathered += qn;
    }
    wave_sync();
    write_ranked(w.Ld, w.Li, K, i, lane, idx_new, dist_new);
    int changed = 0;
    for (int p = lane; p < K; p += 64) {
        const int ip = w.Li[p];
        bool found = false;
        for (int q = 0; q < K; ++q) found |= idx_old[i * K + q] == ip;
        changed += found ? 0 : 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) changed += __shfl_xor(changed, off);
    if (lane == 0 && changed) atomicAdd(updates, static_cast<unsigned long long>(changed));   // (integer counts: order-free)
    if (lane == 0 && gathered) atomicAdd(updates + 1, static_cast<unsigned long long>(gathered));
}

// Rows per launch: about 1e10 gathered bytes (cands rows of 8 d bytes per row), far below a second at any measured gather rate, a
// multiple of the 4 rows of a workgroup; `forced` > 0 overrides it.
long long rows_per_launch(long long n, double cands, int d, int forced) {
    long long rows = forced > 0 ? forced : static_cast<long long>(1e10 / (std::max(cands, 1.0) * 8.0 * std::max(d, 4)));
    rows = std::max<long long>(4, (rows + 3) / 4 * 4);
    return std::min(rows, (n + 3) / 4 * 4);
}

void check_lds(size_t bytes, const char *what) {
    SHARP_REQUIRE(bytes <= ctx().lds_per_block, std::string(what) + ": the workgroup's LDS does not hold the lists");
}

}  // namespace

// (graph.hpp declares it; it lives here, in the code object it has always been in)
void reverse_sort_by_target(const u64 *keys, u64 *keys_s, const int *vals, int *vals_s, long long n, long long ne) {
    Scratch tmp;
    with_scratch(tmp, false, [&](void *p, size_t &bytes) {   // (const inputs: the instantiation this sort has had from the start)
        return rocprim::radix_sort_pairs(p, bytes, keys, keys_s, vals, vals_s, static_cast<size_t>(ne), 0, key_bits(static_cast<u64>(n) << 32),
                                         ctx().stream);
    });
    stream_sync();   // (the sort's temporary storage leaves scope)
}

int knn_descent_candidates(int K, int max_candidates) { return max_candidates > 0 ? max_candidates : std::min(K, 30); }

void knn_descent_start(const double *dX, long long n, int d, int K, int T, unsigned long long seed, int max_rows_per_launch, DevBuf<int> &idx,
                       DevBuf<double> &dist2) {
    Ctx &c = ctx();
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, "knn_descent: need 1 <= K <= 255 and K <= n - 1");
    SHARP_REQUIRE(T >= 1 && T <= KD_MAXT, "knn_descent: n_projections must be in 1 .. 32");
    KernelTimer timer("knn_descent_start");
    std::vector<double> R(static_cast<size_t>(T) * d);
    for (int t = 0; t < T; ++t) {
        const unsigned long long bt = mix64(seed * KD_GOLD + static_cast<unsigned long long>(t));
        for (int col = 0; col < d; ++col)
            R[static_cast<size_t>(t) * d + col] =
                (static_cast<double>(mix64(bt + static_cast<unsigned long long>(col)) >> 12) + 0.5) * 0x1.0p-51 - 1.0;
    }
    DevBuf<double> dR(R.size());
    dR.upload(R.data(), R.size());
    const size_t tn = static_cast<size_t>(T) * n;
    DevBuf<unsigned long long> keys(tn), keys_s(n);
    DevBuf<int> ident(n), order(tn), pos(tn);
    hipLaunchKernelGGL(kd_project_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, dX, n, d, dR.p, T, keys.p);
    launch_check("kd_project_kernel");
    iota(ident.p, n);
    Scratch tmp;
    for (int t = 0; t < T; ++t)   // (stable: equal projections stay in index order)
        sort_pairs(keys.p + static_cast<size_t>(t) * n, keys_s.p, ident.p, order.p + static_cast<size_t>(t) * n, static_cast<size_t>(n), 0, 64, tmp, t > 0);
    hipLaunchKernelGGL(kd_pos_kernel, dim3(grid_for(static_cast<long long>(tn), 256)), dim3(256), 0, c.stream, order.p, n,
                       static_cast<long long>(tn), pos.p);
    launch_check("kd_pos_kernel");
    idx.alloc(static_cast<size_t>(n) * K);
    dist2.alloc(static_cast<size_t>(n) * K);
    const size_t lds = 4 * wave_lds_bytes(K, false);
    check_lds(lds, "knn_descent");
    const long long rows = rows_per_launch(n, static_cast<double>(T) * (2.0 * K + 1.0), d, max_rows_per_launch);
    for (long long r0 = 0; r0 < n; r0 += rows) {
        const long long r1 = std::min(n, r0 + rows);
        hipLaunchKernelGGL(kd_offer_kernel<true>, dim3(grid_for(r1 - r0, 4)), dim3(256), lds, c.stream, dX, n, d, K, r0, r1 - r0, order.p, pos.p, T,
                           K, nullptr, idx.p, dist2.p);
        launch_check("kd_offer_kernel");
    }
    stream_sync();   // (R and the buffers above leave scope)
}

void knn_descent_lists(const double *dX, long long n, int d, int K, const int *index, int max_rows_per_launch, DevBuf<int> &idx,
                       DevBuf<double> &dist2) {
    Ctx &c = ctx();
    idx.alloc(static_cast<size_t>(n) * K);
    dist2.alloc(static_cast<size_t>(n) * K);
    const size_t lds = 4 * wave_lds_bytes(K, false);
    check_lds(lds, "knn_descent");
    const long long rows = rows_per_launch(n, K, d, max_rows_per_launch);
    for (long long r0 = 0; r0 < n; r0 += rows) {
        const long long r1 = std::min(n, r0 + rows);
        hipLaunchKernelGGL(kd_offer_kernel<false>, dim3(grid_for(r1 - r0, 4)), dim3(256), lds, c.stream, dX, n, d, K, r0, r1 - r0, nullptr, nullptr,
                           0, 0, index, idx.p, dist2.p);
        launch_check("kd_offer_kernel");
    }
}

long long knn_descent_join(const double *dX, long long n, int d, int K, int S, int iteration, unsigned long long seed, int max_rows_per_launch,
                           DevBuf<int> &idx, DevBuf<double> &dist2, long long *gathered) {
    Ctx &c = ctx();
    SHARP_REQUIRE(S >= 1 && S <= 255, "knn_descent: max_candidates must be in 1 .. 255 (0: min(K, 30))");
    const int Sf = std::min(K, S), SA = Sf + S;
    const long long ne = n * K;
    DevBuf<int> A(static_cast<size_t>(n) * SA), Acnt(n);
    {
        KernelTimer timer("knn_descent_reverse");
        DevBuf<unsigned long long> keys(ne), keys_s(ne);
        DevBuf<int> vals(ne), vals_s(ne);
        DevBuf<long long> start(n);
        const unsigned long long base = mix64(seed * KD_GOLD + static_cast<unsigned long long>(iteration));
        hipLaunchKernelGGL(kd_revkey_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c.stream, idx.p, ne, K, base, keys.p, vals.p);
        launch_check("kd_revkey_kernel");
        reverse_sort_by_target(keys.p, keys_s.p, vals.p, vals_s.p, n, ne);
        SHARP_HIP_CHECK(hipMemsetAsync(start.p, 0xFF, static_cast<size_t>(n) * sizeof(long long), c.stream));
        hipLaunchKernelGGL(kd_segstart_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c.stream, keys_s.p, ne, start.p);
        launch_check("kd_segstart_kernel");
        hipLaunchKernelGGL(kd_candidates_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, idx.p, keys_s.p, vals_s.p, start.p, n, ne, K, Sf, S,
                           A.p, Acnt.p);
        launch_check("kd_candidates_kernel");
        stream_sync();   // (the sort's buffers leave scope)
    }
    KernelTimer timer("knn_descent_join");
    DevBuf<int> idx_new(static_cast<size_t>(ne));
    DevBuf<double> dist_new(static_cast<size_t>(ne));
    DevBuf<unsigned long long> upd(2);
    upd.zero();
    const size_t lds = 4 * wave_lds_bytes(K, true);
    check_lds(lds, "knn_descent");
    const long long rows = rows_per_launch(n, static_cast<double>(SA) * SA + S, d, max_rows_per_launch);
    for (long long r0 = 0; r0 < n; r0 += rows) {
        const long long r1 = std::min(n, r0 + rows);
        hipLaunchKernelGGL(kd_join_kernel, dim3(grid_for(r1 - r0, 4)), dim3(256), lds, c.stream, dX, n, d, K, r0, r1 - r0, SA, A.p, Acnt.p, idx.p,
                           dist2.p, idx_new.p, dist_new.p, upd.p);
        launch_check("kd_join_kernel");
    }
    unsigned long long h[2] = {0, 0};
    upd.download(h, 2);
    idx = std::move(idx_new);
    dist2 = std::move(dist_new);
    if (gathered) *gathered += static_cast<long long>(h[1]);
    return static_cast<long long>(h[0]);
}

void knn_descent(const double *dX, long long n, int d, int K, int n_projections, int max_candidates, int n_iters, double delta,
                 unsigned long long seed, DevBuf<int> &idx, DevBuf<double> &dist2, KnnDescentInfo &info) {
    SHARP_REQUIRE(n_iters >= 0, "knn_descent: n_iters must be >= 0");
    SHARP_REQUIRE(std::isfinite(delta) && delta >= 0.0 && delta <= 1.0, "knn_descent: delta must be in [0, 1]");
    SHARP_REQUIRE(max_candidates >= 0 && max_candidates <= 255, "knn_descent: max_candidates must be in 1 .. 255 (0: min(K, 30))");
    const int S = knn_descent_candidates(K, max_candidates);
    knn_descent_start(dX, n, d, K, n_projections, seed, 0, idx, dist2);
    info = KnnDescentInfo();
    const double stop = delta * static_cast<double>(n * K);
    for (int it = 1; it <= n_iters; ++it) {
        info.updates = knn_descent_join(dX, n, d, K, S, it, seed, 0, idx, dist2, &info.gathered);
        info.joins = it;
        if (static_cast<double>(info.updates) <= stop) { info.reason = 1; break; }
    }
}

namespace {
// X as the entries take it: finite and small enough that no squared distance or projection overflows, checked on the host
void check_rows(const double *X, long long n, int d, long long ld, int K, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(X && n >= 2 && d >= 1 && ld >= d, w + ": bad input matrix (need n >= 2 rows of d >= 1 values, ld >= d)");
    SHARP_REQUIRE(n < INT_MAX, w + ": at most 2^31 - 1 rows");
    SHARP_REQUIRE(K >= 1 && K <= 255, w + ": K must be in 1 .. 255");
    SHARP_REQUIRE(K <= n - 1, w + ": K neighbours per row need K <= n - 1");
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < d; ++c)
            if (!(std::fabs(X[i * ld + c]) <= KD_XMAX))   // (false for NaN too)
                throw sharp::Error(SHARP_ERR_ARG, w + ": the input holds NA / NaN / Inf or a value beyond 1e100 (row " + std::to_string(i + 1) +
                                                      ", column " + std::to_string(c + 1) + ")");
}

unsigned long long check_seed(double seed, const char *who) {
    SHARP_REQUIRE(seed >= 0.0 && seed < 0x1.0p53 && seed == std::floor(seed), std::string(who) + ": seed must be a whole number in [0, 2^53)");
    return static_cast<unsigned long long>(seed);
}

}  // namespace
}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_knn_descent(const double *X, long long n, int d, long long ld, int K, int n_projections, int max_candidates, int n_iters, double delta,
                      double seed, int *idx, double *dist2, long long *info) {
    SHARP_API_BEGIN
    ctx();
    const char *who = "sharp_knn_descent";
    check_rows(X, n, d, ld, K, who);
    SHARP_REQUIRE(idx && dist2, std::string(who) + ": null output");
    SHARP_REQUIRE(n_projections >= 1 && n_projections <= KD_MAXT, std::string(who) + ": n_projections must be in 1 .. 32");
    SHARP_REQUIRE(max_candidates >= 0 && max_candidates <= 255, std::string(who) + ": max_candidates must be in 1 .. 255 (0: min(K, 30))");
    SHARP_REQUIRE(n_iters >= 0, std::string(who) + ": n_iters must be >= 0");
    SHARP_REQUIRE(std::isfinite(delta) && delta >= 0.0 && delta <= 1.0, std::string(who) + ": delta must be in [0, 1]");
    const unsigned long long s = check_seed(seed, who);
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    DevBuf<int> di;
    DevBuf<double> dd;
    KnnDescentInfo inf;
    knn_descent(dX.p, n, d, K, n_projections, max_candidates, n_iters, delta, s, di, dd, inf);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist2, static_cast<size_t>(n) * K);
    if (info) { info[0] = inf.joins; info[1] = inf.updates; info[2] = inf.reason; info[3] = inf.gathered; }
    SHARP_API_END
}

int sharp_knn_descent_start(const double *X, long long n, int d, long long ld, int K, int n_projections, double seed, int max_rows_per_launch,
                            int *idx, double *dist2) {
    SHARP_API_BEGIN
    ctx();
    const char *who = "sharp_knn_descent_start";
    check_rows(X, n, d, ld, K, who);
    SHARP_REQUIRE(idx && dist2, std::string(who) + ": null output");
    SHARP_REQUIRE(n_projections >= 1 && n_projections <= KD_MAXT, std::string(who) + ": n_projections must be in 1 .. 32");
    SHARP_REQUIRE(max_rows_per_launch >= 0, std::string(who) + ": max_rows_per_launch must be >= 0");
    const unsigned long long s = check_seed(seed, who);
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    DevBuf<int> di;
    DevBuf<double> dd;
    knn_descent_start(dX.p, n, d, K, n_projections, s, max_rows_per_launch, di, dd);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist2, static_cast<size_t>(n) * K);
    SHARP_API_END
}

int sharp_knn_descent_join(const double *X, long long n, int d, long long ld, int K, const int *index, int max_candidates, int iteration,
                           double seed, int max_rows_per_launch, int *idx, double *dist2, long long *updates) {
    SHARP_API_BEGIN
    ctx();
    const char *who = "sharp_knn_descent_join";
    check_rows(X, n, d, ld, K, who);
    SHARP_REQUIRE(index && idx && dist2, std::string(who) + ": null index / output");
    SHARP_REQUIRE(max_candidates >= 0 && max_candidates <= 255, std::string(who) + ": max_candidates must be in 1 .. 255 (0: min(K, 30))");
    SHARP_REQUIRE(iteration >= 1, std::string(who) + ": iteration counts from 1");
    SHARP_REQUIRE(max_rows_per_launch >= 0, std::string(who) + ": max_rows_per_launch must be >= 0");
    const unsigned long long s = check_seed(seed, who);
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    // the caller's lists, validated on the device before an index is dereferenced (range, self, an index twice in a row)
    std::vector<double> zeros(static_cast<size_t>(n) * K, 0.0);
    DevBuf<int> given;
    DevBuf<double> unused;
    upload_neighbours(who, index, zeros.data(), n, K, true, given, unused);
    DevBuf<int> di;
    DevBuf<double> dd;
    knn_descent_lists(dX.p, n, d, K, given.p, max_rows_per_launch, di, dd);
    const long long u = knn_descent_join(dX.p, n, d, K, knn_descent_candidates(K, max_candidates), iteration, s, max_rows_per_launch, di, dd, nullptr);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist2, static_cast<size_t>(n) * K);
    if (updates) *updates = u;
    SHARP_API_END
}

}  // extern "C"
