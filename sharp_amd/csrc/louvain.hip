// louvain.hip -- Louvain community detection on the neighbour graph: DESIGN.md §18 (the project's specification; no parity with
// networkx, igraph or cuGraph is claimed).
//   quantise   q = rint(val * 2^24 / wmax) per entry, the entries with q = 0 dropped (scan + scatter), the row of every entry, the
//              strengths k by integer atomics
//   move       one round from the round's start state (comm, tot): per vertex v of an open source community the weight kin towards
//              every neighbouring community, the gain of each open target, the arg-max under (gain descending, id ascending), and
//              the move when it beats staying.  Three row classes, all exact:
//                lv_move_lds_kernel<64, 256>     rows up to kLvWaveCap entries: one wave per row, (community, kin) in an LDS hash table
//                                                (32-bit key claimed by compare-and-swap, 64-bit integer add)
//                lv_move_lds_kernel<256, 4096>   rows up to kLvBlockCap entries: one workgroup per row, a 48 KB table
//                lv_move_dense_kernel            longer rows (a hub, the rows of a coarse level): a workgroup per row, kin in a dense
//                                                n-slot row in HBM that the workgroup owns, integer atomics in, zeroed again on the way out
//              The table's slot order, the order of the atomics and the row class do not reach the result: kin is an integer sum and
//              the arg-max is a reduction under a total order.
//              (The table, the probe, the gain and the arg-max are louvain_dev.hpp's, shared with Leiden's refine kernels.)
//   state      tot and in by int64 global atomics, the surviving communities counted and ranked by a scan, the fp64 terms
//              in / 2m - gamma (tot / 2m)^2 written at their ranks and sorted by value (rocprim radix sort: Q is a function of the partition, not of its labels)
//              and summed by graph.hpp's two-stage fixed-order reduction (no floating-point atomic).  The host reads Q and the
//              number of communities once per round and decides acceptance.
//   aggregate  key = new[row] * nc + new[col], then graph.hpp's CSR builder: radix sort, equal keys merged by an integer plus, row_ptr by
//              binary search
#include "louvain.hpp"
#include "graph_prim.hpp"
#include "louvain_dev.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "graph_source.hpp"
#include "leiden.hpp"
#include "snn.hpp"

namespace sharp {
namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// quantise, rows, strengths
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_quantise_kernel(const double *__restrict__ val, long long nnz, double wmax, u64 *__restrict__ q,
                                                          long long *__restrict__ flag) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e > nnz) return;
    if (e == nnz) { flag[e] = 0; return; }                 // (the scan's last slot: the number of entries kept)
    const u64 v = static_cast<u64>(static_cast<long long>(rint(val[e] * 16777216.0 / wmax)));
    q[e] = v;
    flag[e] = v > 0 ? 1 : 0;
}

// row[e] = the row that holds entry e (the last r with row_ptr[r] <= e; empty rows are skipped)
__global__ __launch_bounds__(256) void lv_rows_kernel(const long long *__restrict__ rp, long long n, long long nnz, int *__restrict__ row) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    long long lo = 0, hi = n;                              // rp[lo] <= e < rp[hi]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (rp[mid] <= e) lo = mid; else hi = mid;
    }
    row[e] = static_cast<int>(lo);
}

__global__ __launch_bounds__(256) void lv_compact_kernel(const long long *__restrict__ pos, const int *__restrict__ col, const int *__restrict__ row,
                                                         const u64 *__restrict__ q, long long nnz, int *__restrict__ col2, int *__restrict__ row2,
                                                         u64 *__restrict__ q2) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz || q[e] == 0) return;
    const long long p = pos[e];
    col2[p] = col[e];
    row2[p] = row[e];
    q2[p] = q[e];
}

__global__ __launch_bounds__(256) void lv_rowptr_map_kernel(const long long *__restrict__ rp, const long long *__restrict__ pos, long long n,
                                                            long long *__restrict__ rp2) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v <= n) rp2[v] = pos[rp[v]];                       // (pos has nnz + 1 slots)
}

__global__ __launch_bounds__(256) void lv_strength_kernel(const int *__restrict__ row, const u64 *__restrict__ q, long long nnz, u64 *__restrict__ k) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < nnz) atomicAdd(&k[row[e]], q[e]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// move
// ---------------------------------------------------------------------------------------------------------------------------
// GROUP lanes per row (64: a wave, four rows per workgroup; 256: the workgroup), a table of SLOTS > the row's entries.  rows: the ids
// of the class's rows.  prop holds comm on entry; a vertex that moves overwrites its slot.
template <int GROUP, int SLOTS>
__global__ __launch_bounds__(256) void lv_move_lds_kernel(const int *__restrict__ rows, int nrows, const long long *__restrict__ rp,
                                                          const int *__restrict__ col, const u64 *__restrict__ q, const int *__restrict__ comm,
                                                          const u64 *__restrict__ k, const u64 *__restrict__ tot, double gamma, double m2, u64 x1,
                                                          int *__restrict__ prop) {
    constexpr int G = 256 / GROUP;
    __shared__ int keys[G][SLOTS];
    __shared__ u64 vals[G][SLOTS];
    __shared__ LvRed red;
    const int g = threadIdx.x / GROUP, lane = threadIdx.x % GROUP;
    const int ri = blockIdx.x * G + g;
    if (ri >= nrows) return;                               // (GROUP 64: whole waves leave; GROUP 256: the grid is nrows)
    const int v = rows[ri];
    const int c0 = comm[v];
    if (!lv_hbit(x1, c0)) return;                          // a closed source: v stays (uniform over the group)
    lv_table_clear<GROUP, SLOTS>(keys[g], vals[g], lane);
    lv_group_sync<GROUP>();
    const long long b0 = rp[v], e1 = rp[v + 1];
    for (long long e = b0 + lane; e < e1; e += GROUP) {
        const int u = col[e];
        if (u == v) continue;                              // v's own self-loop
        lv_table_add<SLOTS>(keys[g], vals[g], comm[u], q[e]);
    }
    lv_group_sync<GROUP>();
    const long long kv = static_cast<long long>(k[v]);
    const double gk = gamma * static_cast<double>(kv);
    LvBest b{0.0, kLvNone};
    long long kin0 = 0;
    for (int s = lane; s < SLOTS; s += GROUP) {
        const int c = keys[g][s];
        if (c < 0) continue;
        const long long kin = static_cast<long long>(vals[g][s]);
        if (c == c0) { kin0 = kin; continue; }
        if (lv_hbit(x1, c)) continue;                      // a closed target
        const double gn = lv_gain(kin, gk, static_cast<long long>(tot[c]), m2);
        if (lv_better(gn, c, b)) { b.g = gn; b.c = c; }
    }
    lv_wave_best(b, kin0);
    if (GROUP == 256) lv_block_best(b, kin0, red);
    if (lane == 0 && b.c != kLvNone) {
        const double stay = lv_gain(kin0, gk, static_cast<long long>(tot[c0]) - kv, m2);
        if (b.g > stay) prop[v] = b.c;
    }
}

// Long rows: workgroup b owns the dense row S = scratch + b * n (all zero between rows) and takes the rows b, b + gridDim.x, ...
// The row's kin are added into S by integer atomics, read back per entry (the entries of one community all read the same sum, so
// the duplicates are equal candidates), and the touched slots are zeroed again.
__global__ __launch_bounds__(256) void lv_move_dense_kernel(const int *__restrict__ rows, int nrows, const long long *__restrict__ rp,
                                                            const int *__restrict__ col, const u64 *__restrict__ q, const int *__restrict__ comm,
                                                            const u64 *__restrict__ k, const u64 *__restrict__ tot, double gamma, double m2, u64 x1,
                                                            u64 *__restrict__ scratch, long long n, int *__restrict__ prop) {
    __shared__ LvRed red;
    u64 *S = scratch + static_cast<long long>(blockIdx.x) * n;
    const int tid = threadIdx.x;
    for (int ri = blockIdx.x; ri < nrows; ri += gridDim.x) {
        const int v = rows[ri];
        const int c0 = comm[v];
        if (!lv_hbit(x1, c0)) continue;                    // (uniform over the workgroup)
        const long long b0 = rp[v], e1 = rp[v + 1];
        for (long long e = b0 + tid; e < e1; e += 256) {
            const int u = col[e];
            if (u != v) atomicAdd(&S[comm[u]], q[e]);
        }
        __syncthreads();
        const long long kv = static_cast<long long>(k[v]);
        const double gk = gamma * static_cast<double>(kv);
        LvBest b{0.0, kLvNone};
        long long kin0 = 0;
        for (long long e = b0 + tid; e < e1; e += 256) {
            const int u = col[e];
            if (u == v) continue;
            const int c = comm[u];
            // (an atomic load at device scope: the sums were made by atomics in L2)
            const long long kin = static_cast<long long>(__hip_atomic_load(&S[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (c == c0) { kin0 = kin; continue; }
            if (lv_hbit(x1, c)) continue;
            const double gn = lv_gain(kin, gk, static_cast<long long>(tot[c]), m2);
            if (lv_better(gn, c, b)) { b.g = gn; b.c = c; }
        }
        lv_wave_best(b, kin0);
        lv_block_best(b, kin0, red);
        if (tid == 0) {
            if (b.c != kLvNone) {
                const double stay = lv_gain(kin0, gk, static_cast<long long>(tot[c0]) - kv, m2);
                if (b.g > stay) prop[v] = b.c;
            }
        }
        for (long long e = b0 + tid; e < e1; e += 256) __hip_atomic_store(&S[comm[col[e]]], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                   // (the zeros are in place, red is free again)
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// state: tot, in, the ranks of the surviving communities, Q
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_tot_kernel(const int *__restrict__ comm, const u64 *__restrict__ k, long long n, u64 *__restrict__ tot,
                                                     int *__restrict__ present) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v >= n) return;
    const int c = comm[v];
    if (k[v]) atomicAdd(&tot[c], k[v]);
    present[c] = 1;
}

__global__ __launch_bounds__(256) void lv_in_kernel(const int *__restrict__ row, const int *__restrict__ col, const u64 *__restrict__ q, long long nnz,
                                                    const int *__restrict__ comm, u64 *__restrict__ in) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int c = comm[row[e]];
    if (c == comm[col[e]]) atomicAdd(&in[c], q[e]);
}

// terms[pos[c]] = in_c / 2m - gamma * (t * t), t = tot_c / 2m, for the communities with members; the slots behind them, up to the
// bound the host knows for their number, hold +inf (lv_fill_kernel), which the sort by value that follows leaves at the end
__global__ __launch_bounds__(256) void lv_fill_kernel(double *__restrict__ v, long long n, double x) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) v[i] = x;
}
__global__ __launch_bounds__(256) void lv_terms_kernel(const u64 *__restrict__ tot, const u64 *__restrict__ in, const int *__restrict__ present,
                                                       const int *__restrict__ pos, long long n, double m2, double gamma,
                                                       double *__restrict__ terms) {
    const long long c = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (c >= n || !present[c]) return;
    const double t = static_cast<double>(static_cast<long long>(tot[c])) / m2;
    terms[pos[c]] = static_cast<double>(static_cast<long long>(in[c])) / m2 - gamma * (t * t);   // (pos[c] < n: inside the buffer whatever the bound)
}

// graph.hpp's fixed_reduce with the length read on the device (*len = the number of communities): stage 1 folds chunks of
// max(256, ceil(len / 1024)) values, 256 strided running sums and a tree per workgroup; stage 2 folds the workgroups' results alike.
__device__ __forceinline__ double block_fold(double a, double *s) {
    const int tid = threadIdx.x;
    s[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s[tid] = s[tid] + s[tid + w];
        __syncthreads();
    }
    return s[0];
}
__global__ __launch_bounds__(256) void lv_reduce1_kernel(const double *__restrict__ v, const int *__restrict__ len, double *__restrict__ part) {
    __shared__ double s[256];
    const long long n = *len;
    const long long per = (n + kRedBlocks - 1) / kRedBlocks, chunk = per > 256 ? per : 256;
    const long long nb = ((n > 1 ? n : 1) + chunk - 1) / chunk;
    if (blockIdx.x >= nb) return;
    const long long b0 = static_cast<long long>(blockIdx.x) * chunk, e = b0 + chunk < n ? b0 + chunk : n;
    double a = 0.0;
    for (long long i = b0 + threadIdx.x; i < e; i += 256) a = a + v[i];
    a = block_fold(a, s);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void lv_reduce2_kernel(const double *__restrict__ part, const int *__restrict__ len, double *__restrict__ out) {
    __shared__ double s[256];
    const long long n = *len;
    const long long per = (n + kRedBlocks - 1) / kRedBlocks, chunk = per > 256 ? per : 256;
    const long long nb = ((n > 1 ? n : 1) + chunk - 1) / chunk;
    double a = 0.0;
    for (long long i = threadIdx.x; i < nb; i += 256) a = a + part[i];
    a = block_fold(a, s);
    if (threadIdx.x == 0) out[0] = a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// aggregate
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_keys_kernel(const int *__restrict__ row, const int *__restrict__ col, long long nnz, const int *__restrict__ comm,
                                                      const int *__restrict__ pos, u64 nc, u64 *__restrict__ keys) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    keys[e] = static_cast<u64>(pos[comm[row[e]]]) * nc + static_cast<u64>(pos[comm[col[e]]]);
}

__global__ __launch_bounds__(256) void lv_compose_kernel(int *__restrict__ vmap, long long n0, const int *__restrict__ comm, const int *__restrict__ pos) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v < n0) vmap[v] = pos[comm[vmap[v]]];
}

__global__ __launch_bounds__(256) void lv_new_kernel(const int *__restrict__ present, const int *__restrict__ pos, long long n, int *__restrict__ out) {
    const long long c = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (c < n) out[c] = present[c] ? pos[c] : -1;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
void lv_fill_strengths(LouvainGraph &L) {
    Ctx &c = ctx();
    L.k.alloc(L.n);
    L.k.zero();
    if (L.nnz) {
        hipLaunchKernelGGL(lv_strength_kernel, dim3(grid_for(L.nnz, 256)), dim3(256), 0, c.stream, L.row.p, L.val.p, L.nnz, L.k.p);
        launch_check("lv_strength_kernel");
    }
}

void LouvainWork::size(long long nn) {
    n = nn;
    tot.alloc(n); tot2.alloc(n); in.alloc(n);
    present.alloc(n + 1); pos.alloc(n + 1);
    terms.alloc(n); sorted.alloc(n); part.alloc(kRedBlocks); out.alloc(1);
}

void LouvainWork::classify(const LouvainGraph &L) {
    std::vector<long long> len(L.n + 1);
    L.row_ptr.download(len.data(), len.size());
    for (long long v = 0; v < L.n; ++v) len[v] = len[v + 1] - len[v];
    len.pop_back();
    rows.classify(len, kLvWaveCap, kLvBlockCap, true);   // (an empty row has nothing to move by)
    if (rows.n_dense) {                                // dense rows of n slots each: at most 1 GB in all
        scratch.alloc(static_cast<size_t>(rows.dense_grid) * L.n);
        scratch.zero();
    }
}
using Work = LouvainWork;

// tot, present / pos and Q of the membership comm; returns Q and the number of communities.  bound: a number the communities cannot
// exceed (0: n) -- a round's proposals name communities of the state they start from only, so the accepted state's count bounds them;
// only that many terms are sorted
double lv_state(const LouvainGraph &L, const int *comm, u64 *tot, Work &W, double gamma, long long *nc_out, long long bound) {
    Ctx &c = ctx();
    KernelTimer t("louvain_state");
    const long long n = L.n;
    if (bound <= 0 || bound > n) bound = n;
    SHARP_HIP_CHECK(hipMemsetAsync(tot, 0, n * sizeof(u64), c.stream));
    W.in.zero();
    W.present.zero();
    hipLaunchKernelGGL(lv_tot_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, comm, L.k.p, n, tot, W.present.p);
    launch_check("lv_tot_kernel");
    if (L.nnz) {
        hipLaunchKernelGGL(lv_in_kernel, dim3(grid_for(L.nnz, 256)), dim3(256), 0, c.stream, L.row.p, L.col.p, L.val.p, L.nnz, comm, W.in.p);
        launch_check("lv_in_kernel");
    }
    exclusive_scan(W.present.p, W.pos.p, static_cast<size_t>(n + 1), W.tmp, W.sized);
    hipLaunchKernelGGL(lv_fill_kernel, dim3(grid_for(bound, 256)), dim3(256), 0, c.stream, W.terms.p, bound, HUGE_VAL);
    hipLaunchKernelGGL(lv_terms_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, tot, W.in.p, W.present.p, W.pos.p, n,
                       static_cast<double>(L.m2), gamma, W.terms.p);
    launch_check("lv_terms_kernel");
    sort_keys(W.terms.p, W.sorted.p, static_cast<size_t>(bound), 0, 64, W.tmp_sort, W.sized);
    W.sized = true;
    hipLaunchKernelGGL(lv_reduce1_kernel, dim3(kRedBlocks), dim3(256), 0, c.stream, W.sorted.p, W.pos.p + n, W.part.p);
    hipLaunchKernelGGL(lv_reduce2_kernel, dim3(1), dim3(256), 0, c.stream, W.part.p, W.pos.p + n, W.out.p);
    launch_check("lv_reduce_kernel");
    double Q = 0.0;
    int nc = 0;
    SHARP_HIP_CHECK(hipMemcpyAsync(&Q, W.out.p, sizeof(double), hipMemcpyDeviceToHost, c.stream));
    SHARP_HIP_CHECK(hipMemcpyAsync(&nc, W.pos.p + n, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    stream_sync();
    *nc_out = nc;
    return Q;
}

// prop = the proposals of one round from (comm, tot)
void lv_move(const LouvainGraph &L, const int *comm, const u64 *tot, Work &W, double gamma, u64 x1, int *prop) {
    Ctx &c = ctx();
    KernelTimer t("louvain_move");
    SHARP_HIP_CHECK(hipMemcpyAsync(prop, comm, L.n * sizeof(int), hipMemcpyDeviceToDevice, c.stream));
    const double m2 = static_cast<double>(L.m2);
    if (W.rows.n_wave) {
        hipLaunchKernelGGL((lv_move_lds_kernel<64, 256>), dim3(grid_for(W.rows.n_wave, 4)), dim3(256), 0, c.stream, W.rows.rows_wave.p, W.rows.n_wave, L.row_ptr.p,
                           L.col.p, L.val.p, comm, L.k.p, tot, gamma, m2, x1, prop);
        launch_check("lv_move_lds_kernel<64>");
    }
    if (W.rows.n_block) {
        hipLaunchKernelGGL((lv_move_lds_kernel<256, 4096>), dim3(W.rows.n_block), dim3(256), 0, c.stream, W.rows.rows_block.p, W.rows.n_block, L.row_ptr.p,
                           L.col.p, L.val.p, comm, L.k.p, tot, gamma, m2, x1, prop);
        launch_check("lv_move_lds_kernel<256>");
    }
    if (W.rows.n_dense) {
        hipLaunchKernelGGL(lv_move_dense_kernel, dim3(W.rows.dense_grid), dim3(256), 0, c.stream, W.rows.rows_dense.p, W.rows.n_dense, L.row_ptr.p, L.col.p, L.val.p,
                           comm, L.k.p, tot, gamma, m2, x1, W.scratch.p, L.n, prop);
        launch_check("lv_move_dense_kernel");
    }
}

// the coarse graph of (L, comm) given the ranks W.pos of the surviving communities (lv_state of comm) and their number
void lv_aggregate(const LouvainGraph &L, const int *comm, const Work &W, long long nc, LouvainGraph &C) {
    Ctx &c = ctx();
    KernelTimer t("louvain_aggregate");
    const size_t ne = static_cast<size_t>(L.nnz);
    const u64 unc = static_cast<u64>(nc);
    DevBuf<u64> keys(ne), keys2(ne), vals2(ne), ukeys(ne);
    C.n = nc;
    C.m2 = L.m2;
    C.val.alloc(ne);
    hipLaunchKernelGGL(lv_keys_kernel, dim3(grid_for(L.nnz, 256)), dim3(256), 0, c.stream, L.row.p, L.col.p, L.nnz, comm, W.pos.p, unc, keys.p);
    launch_check("lv_keys_kernel");
    MergeScratch tmp;
    const size_t m = merge_by_key<u64, Plus>(keys.p, L.val.p, ne, unc * unc, keys2.p, vals2.p, ukeys.p, C.val.p, tmp);
    SHARP_REQUIRE(m >= 1 && m <= ne, "louvain: the coarse graph holds an impossible number of entries");
    C.nnz = static_cast<long long>(m);
    C.row.alloc(m);
    C.col.alloc(m);
    C.row_ptr.alloc(nc + 1);
    merged_to_csr<u64>(ukeys.p, C.nnz, nc, true, C.row_ptr.p, C.col.p, C.row.p);   // (a coarse vertex may be left without entries)
    lv_fill_strengths(C);
    stream_sync();                                         // (the sort's buffers go out of scope)
}

double lv_level(const LouvainGraph &L, const LouvainArgs &a, int lev, int *&comm, int *&prop, Work &W, int *rounds_out, long long *nc_out) {
    u64 *tot = W.tot.p, *tot2 = W.tot2.p;
    long long nc = 0;
    double Q = lv_state(L, comm, tot, W, a.resolution, &nc);
    int rounds = 0, fails = 0;
    while (rounds < a.max_rounds && fails < a.max_fails) {
        lv_move(L, comm, tot, W, a.resolution, lv_round_key(a.seed, lev, rounds), prop);
        ++rounds;
        long long nc2 = 0;
        const double Q2 = lv_state(L, prop, tot2, W, a.resolution, &nc2, nc);
        SHARP_REQUIRE(nc2 <= nc, "louvain: a round made more communities than it started from");
        if (Q2 > Q + a.tol) {
            std::swap(comm, prop);
            std::swap(tot, tot2);
            Q = Q2;
            nc = nc2;
            fails = 0;
        } else {
            ++fails;
        }
    }
    lv_state(L, comm, tot, W, a.resolution, &nc, nc);      // the ranks (W.pos) of the accepted membership
    *rounds_out = rounds;
    *nc_out = nc;
    return Q;
}

void lv_compose(int *vmap, long long n0, const int *comm, const int *pos) {
    hipLaunchKernelGGL(lv_compose_kernel, dim3(grid_for(n0, 256)), dim3(256), 0, ctx().stream, vmap, n0, comm, pos);
    launch_check("lv_compose_kernel");
}

// 1 .. G by decreasing size, ties to the community with the smallest member (SHARP_unlimited's convention)
void lv_relabel_by_size(const std::vector<int> &lab, long long nc, std::vector<int> &out) {
    std::vector<long long> size(nc, 0), first(nc, -1);
    for (size_t v = 0; v < lab.size(); ++v) {
        if (first[lab[v]] < 0) first[lab[v]] = static_cast<long long>(v);
        ++size[lab[v]];
    }
    std::vector<int> order(nc);
    for (long long c = 0; c < nc; ++c) order[c] = static_cast<int>(c);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return size[a] != size[b] ? size[a] > size[b] : first[a] < first[b]; });
    std::vector<int> rank(nc);
    for (long long r = 0; r < nc; ++r) rank[order[r]] = static_cast<int>(r) + 1;
    out.resize(lab.size());
    for (size_t v = 0; v < lab.size(); ++v) out[v] = rank[lab[v]];
}

void louvain_quantise(const Graph &G, LouvainGraph &L) {
    Ctx &c = ctx();
    SHARP_REQUIRE(G.n >= 2 && G.n <= kLvMaxN, "louvain: need 2 <= n <= 16777216 vertices");
    SHARP_REQUIRE(G.nnz >= 1 && G.nnz < kLvMaxNnz, "louvain: need 1 <= nnz < 2^38 entries");
    SHARP_REQUIRE(G.wmax > 0.0 && std::isfinite(G.wmax), "louvain: the graph holds no positive weight");
    KernelTimer t("louvain_quantise");
    const long long nnz = G.nnz;
    DevBuf<u64> q(nnz);
    DevBuf<long long> flag(nnz + 1), pos(nnz + 1);
    DevBuf<int> row(nnz);
    hipLaunchKernelGGL(lv_quantise_kernel, dim3(grid_for(nnz + 1, 256)), dim3(256), 0, c.stream, G.val.p, nnz, G.wmax, q.p, flag.p);
    hipLaunchKernelGGL(lv_rows_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, c.stream, G.row_ptr.p, G.n, nnz, row.p);
    launch_check("lv_quantise_kernel");
    Scratch tmp;
    exclusive_scan(flag.p, pos.p, static_cast<size_t>(nnz + 1), tmp);
    long long kept = 0;
    SHARP_HIP_CHECK(hipMemcpyAsync(&kept, pos.p + nnz, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
    stream_sync();
    SHARP_REQUIRE(kept >= 1 && kept <= nnz, "louvain: the quantised graph holds an impossible number of entries");
    L.n = G.n;
    L.nnz = kept;
    L.row_ptr.alloc(G.n + 1);
    L.col.alloc(kept);
    L.row.alloc(kept);
    L.val.alloc(kept);
    hipLaunchKernelGGL(lv_compact_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, c.stream, pos.p, G.col.p, row.p, q.p, nnz, L.col.p, L.row.p, L.val.p);
    hipLaunchKernelGGL(lv_rowptr_map_kernel, dim3(grid_for(G.n + 1, 256)), dim3(256), 0, c.stream, G.row_ptr.p, pos.p, G.n, L.row_ptr.p);
    launch_check("lv_compact_kernel");
    lv_fill_strengths(L);
    std::vector<u64> hk(L.n);
    L.k.download(hk.data(), hk.size());                    // (synchronises: the temporaries go out of scope)
    L.m2 = 0;
    for (u64 x : hk) L.m2 += static_cast<long long>(x);
}

void louvain_run(LouvainGraph &L0, const LouvainArgs &a, std::vector<int> &membership, std::vector<LouvainLevel> &levels,
                 std::vector<int> *level_membership) {
    ctx();
    SHARP_REQUIRE(L0.m2 > 0, "louvain: the graph holds no positive weight");
    const long long n0 = L0.n;
    DevBuf<int> vmap(n0);
    iota(vmap.p, n0);
    levels.clear();
    if (level_membership) level_membership->clear();
    LouvainGraph next, *L = &L0;
    LouvainGraph spare;
    long long nc = n0;
    for (int lev = 0; lev < a.max_levels; ++lev) {
        const long long n = L->n;
        Work W;
        W.size(n);
        W.classify(*L);
        DevBuf<int> comm_a(n), comm_b(n);
        int *comm = comm_a.p, *prop = comm_b.p;
        iota(comm, n);
        int rounds = 0;
        const double Q = lv_level(*L, a, lev, comm, prop, W, &rounds, &nc);
        lv_compose(vmap.p, n0, comm, W.pos.p);
        LouvainLevel rec;
        rec.n = n; rec.communities = nc; rec.rounds = rounds; rec.q = Q;
        levels.push_back(rec);
        if (level_membership) {
            const size_t at = level_membership->size();
            level_membership->resize(at + n0);
            vmap.download(level_membership->data() + at, n0);
        }
        if (nc == n || lev + 1 == a.max_levels) { stream_sync(); break; }
        lv_aggregate(*L, comm, W, nc, spare);
        next = std::move(spare);
        spare = LouvainGraph();
        L = &next;
    }
    std::vector<int> lab(n0);
    vmap.download(lab.data(), n0);
    lv_relabel_by_size(lab, nc, membership);
}


void lv_check_csr_shape(const std::string &w, const long long *row_ptr, const int *col, long long n) {
    SHARP_REQUIRE(row_ptr && col, w + ": null row_ptr / col");
    SHARP_REQUIRE(n >= 2 && n <= kLvMaxN, w + ": need 2 <= n <= 16777216 vertices");
    SHARP_REQUIRE(row_ptr[0] == 0, w + ": row_ptr must start at 0");
    for (long long i = 0; i < n; ++i)
        SHARP_REQUIRE(row_ptr[i] <= row_ptr[i + 1] && row_ptr[i + 1] - row_ptr[i] <= n, w + ": row_ptr is not monotone, or a row holds more than n entries");
    SHARP_REQUIRE(row_ptr[n] < kLvMaxNnz, w + ": need fewer than 2^38 entries");
    for (long long i = 0; i < n; ++i)
        for (long long e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            SHARP_REQUIRE(col[e] >= 0 && col[e] < n, w + ": a column index out of range (row " + std::to_string(i) + ", counted from 0)");
            SHARP_REQUIRE(e == row_ptr[i] || col[e - 1] < col[e], w + ": the columns of a row must ascend strictly (row " + std::to_string(i) + ", counted from 0)");
        }
}

// a float-weighted symmetric CSR without diagonal entries on the device (the input of rule 1)
void lv_upload_float_graph(const std::string &w, const long long *row_ptr, const int *col, const double *val, long long n, Graph &G) {
    lv_check_csr_shape(w, row_ptr, col, n);
    SHARP_REQUIRE(val, w + ": null val");
    const long long nnz = row_ptr[n];
    SHARP_REQUIRE(nnz >= 1, w + ": the graph holds no entry");
    double wmax = 0.0;
    for (long long i = 0; i < n; ++i)
        for (long long e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const std::string at = " (row " + std::to_string(i) + ", column " + std::to_string(col[e]) + ", counted from 0)";
            SHARP_REQUIRE(col[e] != i, w + ": a diagonal entry" + at);
            SHARP_REQUIRE(val[e] >= 0.0 && val[e] <= 1e100, w + ": a weight that is NA / NaN / Inf, negative or beyond 1e100" + at);
            const int j = col[e];
            const int *b = col + row_ptr[j], *en = col + row_ptr[j + 1];
            const int *p = std::lower_bound(b, en, static_cast<int>(i));
            SHARP_REQUIRE(p != en && *p == i && val[p - col] == val[e], w + ": the graph is not symmetric" + at);
            wmax = std::max(wmax, val[e]);
        }
    SHARP_REQUIRE(wmax > 0.0, w + ": the graph holds no positive weight");
    csr_to_device(row_ptr, col, val, n, wmax, G);
}

// an integer-weighted CSR (a level's graph: self-loops allowed) on the device, for the stage entries
void lv_upload_int_graph(const std::string &w, const long long *row_ptr, const int *col, const long long *q, long long n, LouvainGraph &L) {
    lv_check_csr_shape(w, row_ptr, col, n);
    SHARP_REQUIRE(q, w + ": null q");
    const long long nnz = row_ptr[n];
    long long m2 = 0;
    for (long long e = 0; e < nnz; ++e) {
        SHARP_REQUIRE(q[e] >= 0 && q[e] <= (1ll << 62) - m2, w + ": a negative weight, or weights that sum beyond 2^62");
        m2 += q[e];
    }
    L.n = n;
    L.nnz = nnz;
    L.m2 = m2;
    L.row_ptr.alloc(n + 1);
    L.row_ptr.upload(row_ptr, n + 1);
    L.col.alloc(nnz);
    L.row.alloc(nnz);
    L.val.alloc(nnz);
    if (nnz) {
        L.col.upload(col, nnz);
        L.val.upload(reinterpret_cast<const u64 *>(q), nnz);
        hipLaunchKernelGGL(lv_rows_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, ctx().stream, L.row_ptr.p, n, nnz, L.row.p);
        launch_check("lv_rows_kernel");
    }
    lv_fill_strengths(L);
}

void lv_upload_comm(const std::string &w, const int *comm, long long n, DevBuf<int> &d) {
    SHARP_REQUIRE(comm, w + ": null membership");
    for (long long v = 0; v < n; ++v) SHARP_REQUIRE(comm[v] >= 0 && comm[v] < n, w + ": a community id outside [0, n)");
    d.alloc(n);
    d.upload(comm, n);
}

LouvainArgs louvain_args(const std::string &w, double resolution, double tol, int max_levels, int max_rounds, int max_fails, double seed) {
    SHARP_REQUIRE(std::isfinite(resolution) && resolution > 0.0 && resolution <= 1e6, w + ": resolution must be in (0, 1e6]");
    SHARP_REQUIRE(std::isfinite(tol) && tol >= 0.0, w + ": tol must be finite and >= 0");
    SHARP_REQUIRE(max_levels >= 1 && max_levels <= 64, w + ": max_levels must be in 1 .. 64");
    SHARP_REQUIRE(max_rounds >= 1 && max_rounds <= 100000, w + ": max_rounds must be in 1 .. 100000");
    SHARP_REQUIRE(max_fails >= 1 && max_fails <= 64, w + ": max_fails must be in 1 .. 64");
    SHARP_REQUIRE(std::isfinite(seed) && std::fabs(seed) < 9.0e18, w + ": seed must be a finite integer");
    LouvainArgs a;
    a.resolution = resolution; a.tol = tol; a.max_levels = max_levels; a.max_rounds = max_rounds; a.max_fails = max_fails;
    a.seed = static_cast<u64>(static_cast<long long>(seed));
    return a;
}

void lv_check_list_shape(const std::string &w, long long n, int K) {
    SHARP_REQUIRE(n >= 2 && n <= kLvMaxN, w + ": need 2 <= n <= 16777216 rows");
    SHARP_REQUIRE(K >= 1 && K <= 255 && K <= n - 1, w + ": need 1 <= K <= 255 neighbours per row and K <= n - 1");
}

void run_and_report(const std::string &w, const Graph &G, const LouvainArgs &a, int max_refine_rounds, int *membership, double *modularity,
                    int level_cap, const LevelOut &o) {
    LouvainGraph L;
    louvain_quantise(G, L);
    std::vector<int> mem, lm;
    std::vector<LouvainLevel> levels;
    if (modularity)
        leiden_run(L, a, max_refine_rounds, mem, modularity, levels, o.membership ? &lm : nullptr);
    else
        louvain_run(L, a, mem, levels, o.membership ? &lm : nullptr);
    SHARP_REQUIRE(static_cast<int>(levels.size()) <= level_cap, w + ": level_cap is smaller than the number of levels");
    std::copy(mem.begin(), mem.end(), membership);
    for (size_t l = 0; l < levels.size(); ++l) {
        o.n[l] = levels[l].n;
        o.communities[l] = levels[l].communities;
        o.rounds[l] = levels[l].rounds;
        o.q[l] = levels[l].q;
        if (modularity) {
            o.sub_communities[l] = levels[l].sub_communities;
            o.refine_rounds[l] = levels[l].refine_rounds;
        }
    }
    *o.n_levels = static_cast<int>(levels.size());
    if (o.membership) std::copy(lm.begin(), lm.end(), o.membership);
}

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_louvain_row_caps(int *wave_cap, int *block_cap) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(wave_cap && block_cap, "sharp_louvain_row_caps: null output");
    *wave_cap = kLvWaveCap;
    *block_cap = kLvBlockCap;
    SHARP_API_END
}

int sharp_louvain_quantise(const long long *row_ptr, const int *col, const double *val, long long n, long long *q, long long *k, long long *m2) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    const std::string w("sharp_louvain_quantise");
    SHARP_REQUIRE(q && k && m2, w + ": null output");
    Graph G;
    lv_upload_float_graph(w, row_ptr, col, val, n, G);
    DevBuf<u64> dq(G.nnz);
    DevBuf<long long> flag(G.nnz + 1);
    hipLaunchKernelGGL(lv_quantise_kernel, dim3(grid_for(G.nnz + 1, 256)), dim3(256), 0, c.stream, G.val.p, G.nnz, G.wmax, dq.p, flag.p);
    launch_check("lv_quantise_kernel");
    LouvainGraph L;                                        // (the zeros stay in place here: strengths do not see them)
    L.n = n;
    L.nnz = G.nnz;
    L.row.alloc(G.nnz);
    hipLaunchKernelGGL(lv_rows_kernel, dim3(grid_for(G.nnz, 256)), dim3(256), 0, c.stream, G.row_ptr.p, n, G.nnz, L.row.p);
    launch_check("lv_rows_kernel");
    L.val = std::move(dq);
    lv_fill_strengths(L);
    L.val.download(reinterpret_cast<u64 *>(q), G.nnz);
    L.k.download(reinterpret_cast<u64 *>(k), n);
    *m2 = 0;
    for (long long v = 0; v < n; ++v) *m2 += k[v];
    SHARP_API_END
}

int sharp_louvain_move(const long long *row_ptr, const int *col, const long long *q, long long n, const int *comm, double resolution, double seed,
                       int level, int round, int *proposal) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("sharp_louvain_move");
    SHARP_REQUIRE(proposal, w + ": null output");
    SHARP_REQUIRE(level >= 0 && round >= 0, w + ": level and round must be >= 0");
    const LouvainArgs a = louvain_args(w, resolution, 0.0, 1, 1, 1, seed);
    LouvainGraph L;
    lv_upload_int_graph(w, row_ptr, col, q, n, L);
    SHARP_REQUIRE(L.m2 > 0, w + ": the graph holds no positive weight");
    DevBuf<int> dcomm, dprop(n);
    lv_upload_comm(w, comm, n, dcomm);
    Work W;
    W.size(n);
    W.classify(L);
    long long nc = 0;
    lv_state(L, dcomm.p, W.tot.p, W, a.resolution, &nc);
    lv_move(L, dcomm.p, W.tot.p, W, a.resolution, lv_round_key(a.seed, level, round), dprop.p);
    dprop.download(proposal, n);
    SHARP_API_END
}

int sharp_louvain_modularity(const long long *row_ptr, const int *col, const double *val, const long long *q, long long n, const int *membership,
                             double resolution, double *Q) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("sharp_louvain_modularity");
    SHARP_REQUIRE(Q, w + ": null output");
    SHARP_REQUIRE((val == nullptr) != (q == nullptr), w + ": give val (float weights) or q (integer weights), not both");
    const LouvainArgs a = louvain_args(w, resolution, 0.0, 1, 1, 1, 0.0);
    LouvainGraph L;
    if (val) {
        Graph G;
        lv_upload_float_graph(w, row_ptr, col, val, n, G);
        louvain_quantise(G, L);
    } else {
        lv_upload_int_graph(w, row_ptr, col, q, n, L);
        SHARP_REQUIRE(L.m2 > 0, w + ": the graph holds no positive weight");
    }
    DevBuf<int> dcomm;
    lv_upload_comm(w, membership, n, dcomm);
    Work W;
    W.size(n);
    long long nc = 0;
    *Q = lv_state(L, dcomm.p, W.tot.p, W, a.resolution, &nc);
    SHARP_API_END
}

int sharp_louvain_aggregate(const long long *row_ptr, const int *col, const long long *q, long long n, const int *comm, long long *row_ptr_out,
                            int *col_out, long long *q_out, long long *nnz_out, long long *nc_out, int *new_out) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    const std::string w("sharp_louvain_aggregate");
    SHARP_REQUIRE(row_ptr_out && col_out && q_out && nnz_out && nc_out && new_out, w + ": null output");
    LouvainGraph L, Cg;
    lv_upload_int_graph(w, row_ptr, col, q, n, L);
    SHARP_REQUIRE(L.nnz >= 1, w + ": the graph holds no entry");
    DevBuf<int> dcomm, dnew(n);
    lv_upload_comm(w, comm, n, dcomm);
    Work W;
    W.size(n);
    long long nc = 0;
    lv_state(L, dcomm.p, W.tot.p, W, 1.0, &nc);
    lv_aggregate(L, dcomm.p, W, nc, Cg);
    hipLaunchKernelGGL(lv_new_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, W.present.p, W.pos.p, n, dnew.p);
    launch_check("lv_new_kernel");
    *nc_out = nc;
    *nnz_out = Cg.nnz;
    Cg.row_ptr.download(row_ptr_out, nc + 1);              // (room for n + 1 and nnz entries: the coarse graph is never larger)
    Cg.col.download(col_out, Cg.nnz);
    Cg.val.download(reinterpret_cast<u64 *>(q_out), Cg.nnz);
    dnew.download(new_out, n);
    SHARP_API_END
}

int sharp_louvain_graph(const long long *row_ptr, const int *col, const double *val, long long n, double resolution, double tol, int max_levels,
                        int max_rounds, int max_fails, double seed, int *membership, int level_cap, long long *level_n,
                        long long *level_communities, int *level_rounds, double *level_q, int *n_levels, int *level_membership) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("louvain_graph");
    const LevelOut o{level_n, level_communities, nullptr, level_rounds, nullptr, level_q, n_levels, level_membership};
    SHARP_REQUIRE(membership && o.complete(false), w + ": null output");
    const LouvainArgs a = louvain_args(w, resolution, tol, max_levels, max_rounds, max_fails, seed);
    SHARP_REQUIRE(level_cap >= max_levels, w + ": level_cap must be at least max_levels");
    Graph G;
    lv_upload_float_graph(w, row_ptr, col, val, n, G);
    run_and_report(w, G, a, 0, membership, nullptr, level_cap, o);
    SHARP_API_END
}

int sharp_louvain_neighbors(const int *index, const double *distance, long long n, int K, int squared, double resolution, double tol, int max_levels,
                            int max_rounds, int max_fails, double seed, int *membership, int level_cap, long long *level_n,
                            long long *level_communities, int *level_rounds, double *level_q, int *n_levels, int *level_membership) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("louvain_neighbors");
    const LevelOut o{level_n, level_communities, nullptr, level_rounds, nullptr, level_q, n_levels, level_membership};
    SHARP_REQUIRE(index && distance, w + ": null index / distance");
    SHARP_REQUIRE(membership && o.complete(false), w + ": null output");
    lv_check_list_shape(w, n, K);
    const LouvainArgs a = louvain_args(w, resolution, tol, max_levels, max_rounds, max_fails, seed);
    SHARP_REQUIRE(level_cap >= max_levels, w + ": level_cap must be at least max_levels");
    Graph G;
    fuzzy_graph_from_lists(w, index, distance, n, K, squared != 0, G);
    run_and_report(w, G, a, 0, membership, nullptr, level_cap, o);
    SHARP_API_END
}

int sharp_louvain_snn(const int *index, long long n, int K, double prune, double resolution, double tol, int max_levels, int max_rounds,
                      int max_fails, double seed, int *membership, int level_cap, long long *level_n, long long *level_communities,
                      int *level_rounds, double *level_q, int *n_levels, int *level_membership) {
    SHARP_API_BEGIN
    const std::string w("louvain_snn");
    const LevelOut o{level_n, level_communities, nullptr, level_rounds, nullptr, level_q, n_levels, level_membership};
    SHARP_REQUIRE(index, w + ": null index");
    SHARP_REQUIRE(membership && o.complete(false), w + ": null output");
    snn_check_args(w, n, K, prune);
    const LouvainArgs a = louvain_args(w, resolution, tol, max_levels, max_rounds, max_fails, seed);
    SHARP_REQUIRE(level_cap >= max_levels, w + ": level_cap must be at least max_levels");
    ctx();
    Graph G;
    snn_graph_from_lists(w, index, n, K, prune, G);
    run_and_report(w, G, a, 0, membership, nullptr, level_cap, o);
    SHARP_API_END
}

}  // extern "C"
