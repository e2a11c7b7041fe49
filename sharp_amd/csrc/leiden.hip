// leiden.hip -- Leiden community detection on the neighbour graph: DESIGN.md §25 (the project's specification; no parity with
// leidenalg, igraph or scanpy is claimed).  §18's quantise, move, state, accept and aggregate are louvain.hip's, unchanged.
//   totals     per level: e_v = the weight of v towards its community of P (one entry per lane, int64 atomics), totP per community
//   subtotals  per round: stot and size per sub-community (one vertex per lane), ext = the weight of a sub-community towards the rest
//              of its community (one entry per lane); then one flag word per id: bit 0 "the vertex is eligible", bit 1 "the
//              sub-community of this id is well connected" (fp64 in the written order, no contraction)
//   refine     one round from the round's start state ref: per eligible vertex the weight kin towards every sub-community of its
//              community, the gain of each well-connected one, the arg-max under (gain descending, id ascending) over those with
//              gain > 0 and allowed bits, and whether any gain was positive at all.  The row classes, their caps, the LDS table, the
//              probe and the arg-max are the move kernels' (louvain_dev.hpp):
//                ld_refine_lds_kernel<64, 256>    one wave per row, the table keyed by ref[col] over the entries with P[col] == P[row]
//                ld_refine_lds_kernel<256, 4096>  one workgroup per row
//                ld_refine_dense_kernel           longer rows: kin in the dense n-slot row in HBM that the workgroup owns
//              The moved and the wanting vertices are counted by a ballot per wave into two counters that the host reads once a round.
//   split      the components inside a labelling: umap_spectral.hip's sweeps with the entries across two labels dropped
// Integer atomics only; every scalar is written by an ordinary vector store.
#include "leiden.hpp"
#include "louvain_dev.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "graph_source.hpp"
#include "snn.hpp"
#include "umap.hpp"

namespace sharp {
namespace {

constexpr int kEligible = 1, kWell = 2;

// ---------------------------------------------------------------------------------------------------------------------------
// totals and subtotals
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ld_totp_kernel(const int *__restrict__ P, const u64 *__restrict__ k, long long n, u64 *__restrict__ totP) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v < n && k[v]) atomicAdd(&totP[P[v]], k[v]);
}

// e[v] += q over the entries (v, u), u != v, P[u] == P[v]
__global__ __launch_bounds__(256) void ld_inside_kernel(const int *__restrict__ row, const int *__restrict__ col, const u64 *__restrict__ q, long long nnz,
                                                        const int *__restrict__ P, u64 *__restrict__ ev) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int v = row[e], u = col[e];
    if (u != v && P[u] == P[v]) atomicAdd(&ev[v], q[e]);
}

__global__ __launch_bounds__(256) void ld_members_kernel(const int *__restrict__ ref, const u64 *__restrict__ k, long long n, u64 *__restrict__ stot,
                                                         int *__restrict__ size) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v >= n) return;
    const int s = ref[v];
    if (k[v]) atomicAdd(&stot[s], k[v]);
    atomicAdd(&size[s], 1);
}

// ext[ref[v]] += q over the entries (v, u) with P[u] == P[v] and ref[u] != ref[v]
__global__ __launch_bounds__(256) void ld_subtotals_kernel(const int *__restrict__ row, const int *__restrict__ col, const u64 *__restrict__ q,
                                                           long long nnz, const int *__restrict__ P, const int *__restrict__ ref,
                                                           u64 *__restrict__ ext) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int v = row[e], u = col[e];
    const int s = ref[v];
    if (u != v && P[u] == P[v] && ref[u] != s) atomicAdd(&ext[s], q[e]);
}

// x is enough for a part of strength a inside a community of strength t: (double)x >= ((gamma * (double)a) * (double)(t - a)) / 2m
__device__ __forceinline__ bool ld_enough(u64 x, u64 a, u64 t, double gamma, double m2) {
    return static_cast<double>(static_cast<long long>(x)) >=
           ((gamma * static_cast<double>(static_cast<long long>(a))) * static_cast<double>(static_cast<long long>(t) - static_cast<long long>(a))) / m2;
}

// per id i: bit 0, the vertex i is eligible (alone in its sub-community and tied closely enough to its community); bit 1, the
// sub-community i has members and is well connected (a sub-community with members holds the vertex of its id)
__global__ __launch_bounds__(256) void ld_flags_kernel(const int *__restrict__ P, const int *__restrict__ ref, const u64 *__restrict__ k,
                                                       const u64 *__restrict__ stot, const int *__restrict__ size, const u64 *__restrict__ ext,
                                                       const u64 *__restrict__ ev, const u64 *__restrict__ totP, double gamma, double m2, long long n,
                                                       int *__restrict__ flag) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 t = totP[P[i]];
    int f = 0;
    if (size[ref[i]] == 1 && ld_enough(ev[i], k[i], t, gamma, m2)) f |= kEligible;
    if (size[i] > 0 && ld_enough(ext[i], stot[i], t, gamma, m2)) f |= kWell;
    flag[i] = f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// refine
// ---------------------------------------------------------------------------------------------------------------------------
// One candidate s of the vertex with source bit `open`: kin towards it.  want: some candidate has a positive gain, whatever the bits.
__device__ __forceinline__ void ld_candidate(int s, long long kin, int own, bool open, double gk, double m2, u64 x1, const int *__restrict__ flag,
                                             const u64 *__restrict__ stot, LvBest &b, long long &want) {
    if (s == own || !(flag[s] & kWell)) return;
    const double gn = lv_gain(kin, gk, static_cast<long long>(stot[s]), m2);
    if (!(gn > 0.0)) return;
    want = 1;
    if (!open || lv_hbit(x1, s)) return;                   // a closed source, or a closed target
    if (lv_better(gn, s, b)) { b.g = gn; b.c = s; }
}

// GROUP lanes per row, a table of SLOTS > the row's entries (lv_move_lds_kernel's shape).  prop holds ref on entry; a vertex that moves
// overwrites its slot.  want[v] = 1 where a candidate has a positive gain (zero on entry).
template <int GROUP, int SLOTS>
__global__ __launch_bounds__(256) void ld_refine_lds_kernel(const int *__restrict__ rows, int nrows, const long long *__restrict__ rp,
                                                            const int *__restrict__ col, const u64 *__restrict__ q, const int *__restrict__ P,
                                                            const int *__restrict__ ref, const int *__restrict__ flag, const u64 *__restrict__ k,
                                                            const u64 *__restrict__ stot, double gamma, double m2, u64 x1, int *__restrict__ prop,
                                                            int *__restrict__ want_out) {
    constexpr int G = 256 / GROUP;
    __shared__ int keys[G][SLOTS];
    __shared__ u64 vals[G][SLOTS];
    __shared__ LvRed red;
    const int g = threadIdx.x / GROUP, lane = threadIdx.x % GROUP;
    const int ri = blockIdx.x * G + g;
    if (ri >= nrows) return;                               // (GROUP 64: whole waves leave; GROUP 256: the grid is nrows)
    const int v = rows[ri];
    if (!(flag[v] & kEligible)) return;                    // v stays, before the table is touched (uniform over the group)
    lv_table_clear<GROUP, SLOTS>(keys[g], vals[g], lane);
    lv_group_sync<GROUP>();
    const int pv = P[v], own = ref[v];
    const long long b0 = rp[v], e1 = rp[v + 1];
    for (long long e = b0 + lane; e < e1; e += GROUP) {
        const int u = col[e];
        if (u == v || P[u] != pv) continue;                // v's own self-loop, or another community
        lv_table_add<SLOTS>(keys[g], vals[g], ref[u], q[e]);
    }
    lv_group_sync<GROUP>();
    const double gk = gamma * static_cast<double>(static_cast<long long>(k[v]));
    const bool open = lv_hbit(x1, own);
    LvBest b{0.0, kLvNone};
    long long want = 0;
    for (int s = lane; s < SLOTS; s += GROUP) {
        const int c = keys[g][s];
        if (c >= 0) ld_candidate(c, static_cast<long long>(vals[g][s]), own, open, gk, m2, x1, flag, stot, b, want);
    }
    lv_wave_best(b, want);
    if (GROUP == 256) lv_block_best(b, want, red);
    if (lane == 0) {
        if (want) want_out[v] = 1;
        if (b.c != kLvNone) prop[v] = b.c;
    }
}

// Long rows: workgroup b owns the dense row S = scratch + b * n (all zero between rows), as in lv_move_dense_kernel.
__global__ __launch_bounds__(256) void ld_refine_dense_kernel(const int *__restrict__ rows, int nrows, const long long *__restrict__ rp,
                                                              const int *__restrict__ col, const u64 *__restrict__ q, const int *__restrict__ P,
                                                              const int *__restrict__ ref, const int *__restrict__ flag, const u64 *__restrict__ k,
                                                              const u64 *__restrict__ stot, double gamma, double m2, u64 x1, u64 *__restrict__ scratch,
                                                              long long n, int *__restrict__ prop, int *__restrict__ want_out) {
    __shared__ LvRed red;
    u64 *S = scratch + static_cast<long long>(blockIdx.x) * n;
    const int tid = threadIdx.x;
    for (int ri = blockIdx.x; ri < nrows; ri += gridDim.x) {
        const int v = rows[ri];
        if (!(flag[v] & kEligible)) continue;              // (uniform over the workgroup)
        const int pv = P[v], own = ref[v];
        const long long b0 = rp[v], e1 = rp[v + 1];
        for (long long e = b0 + tid; e < e1; e += 256) {
            const int u = col[e];
            if (u != v && P[u] == pv) atomicAdd(&S[ref[u]], q[e]);
        }
        __syncthreads();
        const double gk = gamma * static_cast<double>(static_cast<long long>(k[v]));
        const bool open = lv_hbit(x1, own);
        LvBest b{0.0, kLvNone};
        long long want = 0;
        for (long long e = b0 + tid; e < e1; e += 256) {
            const int u = col[e];
            if (u == v || P[u] != pv) continue;
            const int s = ref[u];
            // (an atomic load at device scope: the sums were made by atomics in L2)
            const long long kin = static_cast<long long>(__hip_atomic_load(&S[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            ld_candidate(s, kin, own, open, gk, m2, x1, flag, stot, b, want);
        }
        lv_wave_best(b, want);
        lv_block_best(b, want, red);
        if (tid == 0) {
            if (want) want_out[v] = 1;
            if (b.c != kLvNone) prop[v] = b.c;
        }
        for (long long e = b0 + tid; e < e1; e += 256) __hip_atomic_store(&S[ref[col[e]]], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                   // (the zeros are in place, red is free again)
    }
}

// counters[0] += the vertices that moved, counters[1] += the vertices that want to
__global__ __launch_bounds__(256) void ld_count_kernel(const int *__restrict__ ref, const int *__restrict__ prop, const int *__restrict__ want, long long n,
                                                       unsigned *__restrict__ counters) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const unsigned long long moved = __ballot(v < n && prop[v] != ref[v]);
    const unsigned long long wanting = __ballot(v < n && want[v] != 0);
    if ((threadIdx.x & 63) == 0) {
        if (moved) atomicAdd(&counters[0], static_cast<unsigned>(__popcll(moved)));
        if (wanting) atomicAdd(&counters[1], static_cast<unsigned>(__popcll(wanting)));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// parents, composition
// ---------------------------------------------------------------------------------------------------------------------------
// parent[pos[ref[v]]] = P[v]: every member of a sub-community writes the same value
__global__ __launch_bounds__(256) void ld_parent_kernel(const int *__restrict__ P, const int *__restrict__ ref, const int *__restrict__ pos, long long n,
                                                        int *__restrict__ parent) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v < n) parent[pos[ref[v]]] = P[v];
}

__global__ __launch_bounds__(256) void ld_gather_kernel(const int *__restrict__ vmap, const int *__restrict__ label, long long n0, int *__restrict__ out) {
    const long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v < n0) out[v] = label[vmap[v]];
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
// the refinement's buffers of a level
struct Refine {
    DevBuf<u64> ev, totP, stot, ext;
    DevBuf<int> size, flag, want;
    DevBuf<unsigned> counters;

    void size_for(long long n) {
        ev.alloc(n); totP.alloc(n); stot.alloc(n); ext.alloc(n);
        size.alloc(n); flag.alloc(n); want.alloc(n);
        counters.alloc(2);
    }
};

// e_v and totP of the level's partition P
void ld_totals(const LouvainGraph &L, const int *P, Refine &R) {
    Ctx &c = ctx();
    KernelTimer t("leiden_subtotals");
    R.ev.zero();
    R.totP.zero();
    hipLaunchKernelGGL(ld_totp_kernel, dim3(grid_for(L.n, 256)), dim3(256), 0, c.stream, P, L.k.p, L.n, R.totP.p);
    if (L.nnz)
        hipLaunchKernelGGL(ld_inside_kernel, dim3(grid_for(L.nnz, 256)), dim3(256), 0, c.stream, L.row.p, L.col.p, L.val.p, L.nnz, P, R.ev.p);
    launch_check("ld_inside_kernel");
}

// one round from ref: prop, and the two counters (moved, wanting) read once.  W: the level's row classes and dense rows.
void ld_round(const LouvainGraph &L, const int *P, const int *ref, LouvainWork &W, Refine &R, double gamma, u64 x1, int *prop, unsigned *moved,
              unsigned *wanting) {
    Ctx &c = ctx();
    const long long n = L.n;
    const double m2 = static_cast<double>(L.m2);
    {
        KernelTimer t("leiden_subtotals");
        R.stot.zero();
        R.ext.zero();
        R.size.zero();
        hipLaunchKernelGGL(ld_members_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, ref, L.k.p, n, R.stot.p, R.size.p);
        if (L.nnz)
            hipLaunchKernelGGL(ld_subtotals_kernel, dim3(grid_for(L.nnz, 256)), dim3(256), 0, c.stream, L.row.p, L.col.p, L.val.p, L.nnz, P, ref, R.ext.p);
        hipLaunchKernelGGL(ld_flags_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, P, ref, L.k.p, R.stot.p, R.size.p, R.ext.p, R.ev.p, R.totP.p, gamma,
                           m2, n, R.flag.p);
        launch_check("ld_flags_kernel");
    }
    {
        KernelTimer t("leiden_refine");
        SHARP_HIP_CHECK(hipMemcpyAsync(prop, ref, n * sizeof(int), hipMemcpyDeviceToDevice, c.stream));
        R.want.zero();
        if (W.rows.n_wave) {
            hipLaunchKernelGGL((ld_refine_lds_kernel<64, 256>), dim3(grid_for(W.rows.n_wave, 4)), dim3(256), 0, c.stream, W.rows.rows_wave.p, W.rows.n_wave,
                               L.row_ptr.p, L.col.p, L.val.p, P, ref, R.flag.p, L.k.p, R.stot.p, gamma, m2, x1, prop, R.want.p);
            launch_check("ld_refine_lds_kernel<64>");
        }
        if (W.rows.n_block) {
            hipLaunchKernelGGL((ld_refine_lds_kernel<256, 4096>), dim3(W.rows.n_block), dim3(256), 0, c.stream, W.rows.rows_block.p, W.rows.n_block,
                               L.row_ptr.p, L.col.p, L.val.p, P, ref, R.flag.p, L.k.p, R.stot.p, gamma, m2, x1, prop, R.want.p);
            launch_check("ld_refine_lds_kernel<256>");
        }
        if (W.rows.n_dense) {
            hipLaunchKernelGGL(ld_refine_dense_kernel, dim3(W.rows.dense_grid), dim3(256), 0, c.stream, W.rows.rows_dense.p, W.rows.n_dense, L.row_ptr.p,
                               L.col.p, L.val.p, P, ref, R.flag.p, L.k.p, R.stot.p, gamma, m2, x1, W.scratch.p, n, prop, R.want.p);
            launch_check("ld_refine_dense_kernel");
        }
    }
    R.counters.zero();
    hipLaunchKernelGGL(ld_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, ref, prop, R.want.p, n, R.counters.p);
    launch_check("ld_count_kernel");
    unsigned h[2] = {0, 0};
    R.counters.download(h, 2);
    *moved = h[0];
    *wanting = h[1];
}

inline u64 refine_key(u64 seed, int lev, int r) { return lv_round_key(seed, lev, kLdRefineRound0 + r); }

// rule L2: ref (n ids, device) from the singletons; spare: n ints; on return ref is the refinement.  Returns the counted rounds.
int ld_refine(const LouvainGraph &L, const LouvainArgs &a, int max_refine_rounds, int lev, const int *P, LouvainWork &W, int *&ref, int *&spare) {
    Refine R;
    R.size_for(L.n);
    iota(ref, L.n);
    ld_totals(L, P, R);
    int rounds = 0;
    while (rounds < max_refine_rounds) {
        unsigned moved = 0, wanting = 0;
        ld_round(L, P, ref, W, R, a.resolution, refine_key(a.seed, lev, rounds), spare, &moved, &wanting);
        if (wanting == 0) break;                           // (that round is not counted)
        std::swap(ref, spare);
        ++rounds;
    }
    return rounds;
}

}  // namespace

void leiden_run(LouvainGraph &L0, const LouvainArgs &a, int max_refine_rounds, std::vector<int> &membership, double *Q_out,
                std::vector<LouvainLevel> &levels, std::vector<int> *level_membership) {
    Ctx &c = ctx();
    SHARP_REQUIRE(L0.m2 > 0, "leiden: the graph holds no positive weight");
    const long long n0 = L0.n;
    DevBuf<int> vmap(n0), final_lab(n0);
    iota(vmap.p, n0);
    levels.clear();
    if (level_membership) level_membership->clear();
    LouvainGraph next, spare, *L = &L0;
    DevBuf<int> start;                                     // the next level's comm0 (empty: the singletons)
    for (int lev = 0; lev < a.max_levels; ++lev) {
        const long long n = L->n;
        LouvainWork W;
        W.size(n);
        W.classify(*L);
        DevBuf<int> comm_a(n), comm_b(n), ref_a(n), ref_b(n);
        int *P = comm_a.p, *prop = comm_b.p, *ref = ref_a.p, *ref2 = ref_b.p;
        if (start.n)
            SHARP_HIP_CHECK(hipMemcpyAsync(P, start.p, n * sizeof(int), hipMemcpyDeviceToDevice, c.stream));
        else
            iota(P, n);
        LouvainLevel rec;
        rec.n = n;
        rec.q = lv_level(*L, a, lev, P, prop, W, &rec.rounds, &rec.communities);
        if (level_membership) {                            // the rank of P of every input vertex (W.pos: the ranks of P)
            const size_t at = level_membership->size();
            level_membership->resize(at + n0);
            SHARP_HIP_CHECK(hipMemcpyAsync(final_lab.p, vmap.p, n0 * sizeof(int), hipMemcpyDeviceToDevice, c.stream));
            lv_compose(final_lab.p, n0, P, W.pos.p);
            final_lab.download(level_membership->data() + at, n0);
        }
        rec.refine_rounds = ld_refine(*L, a, max_refine_rounds, lev, P, W, ref, ref2);
        lv_state(*L, ref, W.tot.p, W, a.resolution, &rec.sub_communities);   // the ranks (W.pos) of the sub-communities
        levels.push_back(rec);
        if (rec.sub_communities == n || lev + 1 == a.max_levels) {
            // rule L4: P split into its connected components on this level's graph, carried to the input's vertices
            DevBuf<int> label;
            csr_components(L->row_ptr.p, L->col.p, n, P, label, "leiden_split");
            hipLaunchKernelGGL(ld_gather_kernel, dim3(grid_for(n0, 256)), dim3(256), 0, c.stream, vmap.p, label.p, n0, final_lab.p);
            launch_check("ld_gather_kernel");
            stream_sync();
            break;
        }
        // rule L3: the sub-communities become vertices, the connected parts of their parents the next start
        const long long ns = rec.sub_communities;
        lv_aggregate(*L, ref, W, ns, spare);
        DevBuf<int> parent(ns);
        hipLaunchKernelGGL(ld_parent_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, P, ref, W.pos.p, n, parent.p);
        launch_check("ld_parent_kernel");
        lv_compose(vmap.p, n0, ref, W.pos.p);
        csr_components(spare.row_ptr.p, spare.col.p, ns, parent.p, start, "leiden_split");   // (synchronises)
        next = std::move(spare);
        spare = LouvainGraph();
        L = &next;
    }
    // the returned membership's Q on the input graph, by the state kernel, and its ranks
    LouvainWork W0;
    W0.size(n0);
    long long nc = 0;
    *Q_out = lv_state(L0, final_lab.p, W0.tot.p, W0, a.resolution, &nc);
    hipLaunchKernelGGL(ld_gather_kernel, dim3(grid_for(n0, 256)), dim3(256), 0, c.stream, final_lab.p, W0.pos.p, n0, vmap.p);   // (vmap is free: the ranks go there)
    launch_check("ld_gather_kernel");
    std::vector<int> lab(n0);
    vmap.download(lab.data(), n0);
    lv_relabel_by_size(lab, nc, membership);
}

}  // namespace sharp

using namespace sharp;

namespace {

int refine_rounds_arg(const std::string &w, int max_refine_rounds) {
    SHARP_REQUIRE(max_refine_rounds >= 1 && max_refine_rounds <= kLdMaxRefineRounds, w + ": max_refine_rounds must be in 1 .. 100000");
    return max_refine_rounds;
}

}  // namespace

extern "C" {

int sharp_leiden_level(const long long *row_ptr, const int *col, const long long *q, long long n, const int *comm0, double resolution, double tol,
                       int max_rounds, int max_fails, double seed, int level, int *comm, int *rounds, double *Q) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    const std::string w("sharp_leiden_level");
    SHARP_REQUIRE(comm && rounds && Q, w + ": null output");
    SHARP_REQUIRE(level >= 0, w + ": level must be >= 0");
    const LouvainArgs a = louvain_args(w, resolution, tol, 1, max_rounds, max_fails, seed);
    LouvainGraph L;
    lv_upload_int_graph(w, row_ptr, col, q, n, L);
    SHARP_REQUIRE(L.m2 > 0, w + ": the graph holds no positive weight");
    DevBuf<int> da, db(n);
    lv_upload_comm(w, comm0, n, da);
    LouvainWork W;
    W.size(n);
    W.classify(L);
    int *P = da.p, *spare = db.p;
    long long nc = 0;
    *Q = lv_level(L, a, level, P, spare, W, rounds, &nc);
    SHARP_HIP_CHECK(hipMemcpyAsync(comm, P, n * sizeof(int), hipMemcpyDeviceToHost, c.stream));
    stream_sync();
    SHARP_API_END
}

int sharp_leiden_refine(const long long *row_ptr, const int *col, const long long *q, long long n, const int *P, const int *ref, double resolution,
                        double seed, int level, int round, int *proposal, long long *moved, long long *wanting) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("sharp_leiden_refine");
    SHARP_REQUIRE(proposal && moved && wanting, w + ": null output");
    SHARP_REQUIRE(level >= 0 && round >= 0 && round < kLdMaxRefineRounds, w + ": level must be >= 0 and round in 0 .. 99999");
    const LouvainArgs a = louvain_args(w, resolution, 0.0, 1, 1, 1, seed);
    LouvainGraph L;
    lv_upload_int_graph(w, row_ptr, col, q, n, L);
    SHARP_REQUIRE(L.m2 > 0, w + ": the graph holds no positive weight");
    DevBuf<int> dP, dref, dprop(n);
    lv_upload_comm(w, P, n, dP);
    lv_upload_comm(w, ref, n, dref);
    LouvainWork W;
    W.classify(L);
    Refine R;
    R.size_for(n);
    ld_totals(L, dP.p, R);
    unsigned m = 0, wt = 0;
    ld_round(L, dP.p, dref.p, W, R, a.resolution, refine_key(a.seed, level, round), dprop.p, &m, &wt);
    dprop.download(proposal, n);
    *moved = m;
    *wanting = wt;
    SHARP_API_END
}

int sharp_leiden_split(const long long *row_ptr, const int *col, const long long *q, long long n, const int *label, int *out, long long *count) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("sharp_leiden_split");
    SHARP_REQUIRE(label && out && count, w + ": null label / output");
    LouvainGraph L;
    lv_upload_int_graph(w, row_ptr, col, q, n, L);
    DevBuf<int> dl(n), dout;
    dl.upload(label, n);
    *count = csr_components(L.row_ptr.p, L.col.p, n, dl.p, dout, "leiden_split");
    dout.download(out, n);
    SHARP_API_END
}

int sharp_leiden_graph(const long long *row_ptr, const int *col, const double *val, long long n, double resolution, double tol, int max_levels,
                       int max_rounds, int max_fails, int max_refine_rounds, double seed, int *membership, double *modularity, int level_cap,
                       long long *level_n, long long *level_communities, long long *level_sub_communities, int *level_rounds,
                       int *level_refine_rounds, double *level_q, int *n_levels, int *level_membership) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("leiden_graph");
    const LevelOut o{level_n, level_communities, level_sub_communities, level_rounds, level_refine_rounds, level_q, n_levels, level_membership};
    SHARP_REQUIRE(membership && modularity && o.complete(true), w + ": null output");
    const LouvainArgs a = louvain_args(w, resolution, tol, max_levels, max_rounds, max_fails, seed);
    refine_rounds_arg(w, max_refine_rounds);
    SHARP_REQUIRE(level_cap >= max_levels, w + ": level_cap must be at least max_levels");
    Graph G;
    lv_upload_float_graph(w, row_ptr, col, val, n, G);
    run_and_report(w, G, a, max_refine_rounds, membership, modularity, level_cap, o);
    SHARP_API_END
}

int sharp_leiden_neighbors(const int *index, const double *distance, long long n, int K, int squared, double resolution, double tol, int max_levels,
                           int max_rounds, int max_fails, int max_refine_rounds, double seed, int *membership, double *modularity, int level_cap,
                           long long *level_n, long long *level_communities, long long *level_sub_communities, int *level_rounds,
                           int *level_refine_rounds, double *level_q, int *n_levels, int *level_membership) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("leiden_neighbors");
    const LevelOut o{level_n, level_communities, level_sub_communities, level_rounds, level_refine_rounds, level_q, n_levels, level_membership};
    SHARP_REQUIRE(index && distance, w + ": null index / distance");
    SHARP_REQUIRE(membership && modularity && o.complete(true), w + ": null output");
    lv_check_list_shape(w, n, K);
    const LouvainArgs a = louvain_args(w, resolution, tol, max_levels, max_rounds, max_fails, seed);
    refine_rounds_arg(w, max_refine_rounds);
    SHARP_REQUIRE(level_cap >= max_levels, w + ": level_cap must be at least max_levels");
    Graph G;
    fuzzy_graph_from_lists(w, index, distance, n, K, squared != 0, G);
    run_and_report(w, G, a, max_refine_rounds, membership, modularity, level_cap, o);
    SHARP_API_END
}

int sharp_leiden_snn(const int *index, long long n, int K, double prune, double resolution, double tol, int max_levels, int max_rounds, int max_fails,
                     int max_refine_rounds, double seed, int *membership, double *modularity, int level_cap, long long *level_n,
                     long long *level_communities, long long *level_sub_communities, int *level_rounds, int *level_refine_rounds, double *level_q,
                     int *n_levels, int *level_membership) {
    SHARP_API_BEGIN
    const std::string w("leiden_snn");
    const LevelOut o{level_n, level_communities, level_sub_communities, level_rounds, level_refine_rounds, level_q, n_levels, level_membership};
    SHARP_REQUIRE(index, w + ": null index");
    SHARP_REQUIRE(membership && modularity && o.complete(true), w + ": null output");
    snn_check_args(w, n, K, prune);
    const LouvainArgs a = louvain_args(w, resolution, tol, max_levels, max_rounds, max_fails, seed);
    refine_rounds_arg(w, max_refine_rounds);
    SHARP_REQUIRE(level_cap >= max_levels, w + ": level_cap must be at least max_levels");
    ctx();
    Graph G;
    snn_graph_from_lists(w, index, n, K, prune, G);
    run_and_report(w, G, a, max_refine_rounds, membership, modularity, level_cap, o);
    SHARP_API_END
}

}  // extern "C"
