// snn.hip -- the SNN / Jaccard neighbour graph from k-NN lists: DESIGN.md §19 (the formula is Seurat's ComputeSNN; no run against Seurat
// is claimed).  A is the n x n 0/1 matrix with k = K + 1 ones per row, S(i) = {i} + the row's K neighbours; the graph is A A^T without
// its diagonal, s(i, j) = |S(i) n S(j)|, w = s / (2k - s), an entry kept iff s >= smin (prune turned into an integer once, on the host).
//   reverse    the lists validated (range, self, twice) and the in-degrees |R(m)| counted by integer atomics in one kernel, a scan, the
//              reverse lists R(m) = {j : m in S(j)} ascending by graph.hpp's sort of (target << 32 | source) keys, and the row
//              work t(i) = sum over m in S(i) of |R(m)|, which the host reads once to deal the rows into classes
//   count      Gustavson's row product per row: for m in S(i), for j in R(m), j != i: count[j] += 1; the entries with count >= smin are
//              counted, a scan gives row_ptr and nnz.  Three row classes by t(i), all exact:
//                snn_lds_kernel<64, 2048>     t <= 1536: one wave per row (two rows per workgroup), (j, count) in an LDS hash table, the key
//                                             claimed by a 32-bit compare-and-swap, the count an integer add
//                snn_lds_kernel<256, 8192>    t <= 6144: one workgroup per row, a 64 KB table
//                snn_dense_kernel             beyond: a workgroup per row, a dense row of n counters in HBM that the workgroup owns,
//                                             integer atomics in, every touched slot read and zeroed by one atomic exchange on the way out
//              A row uses the smallest power-of-two part of its table that t fills to at most three quarters, so a short row neither
//              clears nor scans the whole table.
//   fill       the same product again; the survivors go to the row's range as (i << 32 | j << 8 | s - 1), unsorted
//   sort       one radix sort of those words by (i, j) (keys are unique, so it is deterministic), then col, val = tab[s] and shared are
//              unpacked; tab[s] = (double)s / (double)(2k - s) is made on the host
// No floating-point atomic anywhere; the slot order of a table and the order of the atomics do not reach the result.
#include "snn.hpp"
#include "graph_prim.hpp"
#include "knn.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace sharp {
namespace {

constexpr int kSub = 16;                     // lanes that walk one R(m) together

// One thread per list entry, before anything dereferences an index: in [0, n), not the row itself, not named earlier in the row.
// *word = min over the offending entries of (row << 3 | kind).  An index in range adds 1 to its in-degree (deg starts at 1: the row itself).
__global__ __launch_bounds__(256) void snn_check_degree_kernel(const int *__restrict__ idx, long long n, int K, long long ne,
                                                               long long *__restrict__ deg, u64 *__restrict__ word) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= ne) return;
    const long long r = e / K;
    const int p = static_cast<int>(e - r * K);
    const int j = idx[e];
    int kind = 8;
    if (j < 0 || j >= n) kind = NN_RANGE;
    else if (j == r) kind = NN_SELF;
    else {
        for (int q = 0; q < p; ++q)
            if (idx[r * K + q] == j) { kind = NN_TWICE; break; }
        atomicAdd(reinterpret_cast<u64 *>(&deg[j]), 1ull);
    }
    if (kind < 8) atomicMin(word, (static_cast<u64>(r) << 3) | static_cast<u64>(kind));
}

__global__ __launch_bounds__(256) void snn_fill_ll_kernel(long long *__restrict__ v, long long n, long long x, long long last) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) v[i] = x;
    else if (i == n) v[i] = last;                            // (the scan's extra slot)
}

// keys[i k + p] = (m << 32 | i), vals = i, m the p-th member of S(i) (p = K: the row itself)
__global__ __launch_bounds__(256) void snn_revkey_kernel(const int *__restrict__ idx, long long n, int K, u64 *__restrict__ keys,
                                                         int *__restrict__ vals) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int k = K + 1;
    if (e >= n * k) return;
    const long long i = e / k;
    const int p = static_cast<int>(e - i * k);
    const u64 m = static_cast<u64>(p < K ? idx[i * K + p] : static_cast<int>(i));
    keys[e] = (m << 32) | static_cast<u64>(i);
    vals[e] = static_cast<int>(i);
}

// t[i] = sum over m in S(i) of |R(m)|
__global__ __launch_bounds__(256) void snn_work_kernel(const int *__restrict__ idx, const long long *__restrict__ deg, long long n, int K,
                                                       long long *__restrict__ t) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    long long s = deg[i];
    for (int p = 0; p < K; ++p) s += deg[idx[i * K + p]];
    t[i] = s;
}

// an entry on its way to the sort: (row << 32 | column << 8 | s - 1); n <= 2^24 and s <= 256
__device__ __forceinline__ u64 pack(long long i, int j, int s) {
    return (static_cast<u64>(i) << 32) | (static_cast<u64>(static_cast<unsigned>(j)) << 8) | static_cast<u64>(s - 1);
}

template <int GROUP>
__device__ __forceinline__ void group_sync() {
    if (GROUP == 64) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// Gustavson's row product of row i over GROUP lanes: fn(j) for every m in S(i) and every j in R(m), j != i.  kSub lanes walk one R(m).
template <int GROUP, typename F>
__device__ __forceinline__ void row_product(const int *__restrict__ idx, const long long *__restrict__ rptr, const int *__restrict__ R,
                                            long long i, int K, int lane, F fn) {
    const int sub = lane & (kSub - 1);
    for (int a = lane / kSub; a <= K; a += GROUP / kSub) {
        const long long m = a < K ? idx[i * K + a] : i;
        const long long b = rptr[m], e = rptr[m + 1];
        for (long long x = b + sub; x < e; x += kSub) {
            const int j = R[x];
            if (j != i) fn(j);
        }
    }
}

// GROUP lanes per row (64: a wave, two rows per workgroup of 128; 256: the workgroup), a table of up to SLOTS (j, count) pairs.  rows: the
// ids of the class's rows.  FILL false: cnt[i] = the survivors of row i, *smax = the largest s of a survivor.  FILL true: the survivors
// to packed[rp[i] ..] as (i << 32 | j << 8 | s - 1), in the table's order.
template <int GROUP, int SLOTS, bool FILL>
__global__ __launch_bounds__(GROUP == 64 ? 128 : 256) void snn_lds_kernel(const int *__restrict__ rows, int nrows, const int *__restrict__ idx,
                                                                         const long long *__restrict__ rptr, const int *__restrict__ R,
                                                                         const long long *__restrict__ t, int K, int smin,
                                                                         long long *__restrict__ cnt, int *__restrict__ smax,
                                                                         const long long *__restrict__ rp, u64 *__restrict__ packed) {
    constexpr int G = GROUP == 64 ? 2 : 1;
    __shared__ int2 tab[G][SLOTS];                           // (.x the key j, -1: free; .y its count)
    const int g = threadIdx.x / GROUP, lane = threadIdx.x % GROUP;
    const int ri = blockIdx.x * G + g;
    if (ri >= nrows) return;                                 // (GROUP 64: a whole wave leaves; GROUP 256: the grid is nrows)
    const long long i = rows[ri];
    const long long ti = t[i];
    int slots = 64;                                          // the part of the table this row uses: at most three quarters full
    while (slots < SLOTS && 3ll * slots < 4ll * ti) slots <<= 1;
    const unsigned shift = 32u - static_cast<unsigned>(__builtin_ctz(slots));
    for (int s = lane; s < slots; s += GROUP) tab[g][s] = make_int2(-1, 0);
    group_sync<GROUP>();
    row_product<GROUP>(idx, rptr, R, i, K, lane, [&](int j) {
        unsigned s = (static_cast<unsigned>(j) * 0x9E3779B1u) >> shift;
        for (;;) {                                           // (fewer distinct keys than slots: the probe ends)
            const int prev = atomicCAS(&tab[g][s].x, -1, j);
            if (prev == -1 || prev == j) { atomicAdd(&tab[g][s].y, 1); break; }
            s = (s + 1) & (slots - 1);
        }
    });
    group_sync<GROUP>();
    if (FILL) {
        const long long b0 = rp[i], room = rp[i + 1] - b0;
        if constexpr (GROUP == 64) {                         // (slots is a multiple of 64: the loop is uniform over the wave)
            int base = 0;
            for (int s = lane; s < slots; s += 64) {
                const int2 kv = tab[g][s];
                const bool ok = kv.x >= 0 && kv.y >= smin;
                const u64 mask = __ballot(ok);
                const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                if (ok && at < room) packed[b0 + at] = pack(i, kv.x, kv.y);
                base += __popcll(mask);
            }
        } else {
            __shared__ int pos_s;
            if (lane == 0) pos_s = 0;
            __syncthreads();
            for (int s = lane; s < slots; s += GROUP) {
                const int2 kv = tab[g][s];
                if (kv.x < 0 || kv.y < smin) continue;
                const int at = atomicAdd(&pos_s, 1);
                if (at < room) packed[b0 + at] = pack(i, kv.x, kv.y);
            }
        }
    } else {
        int c = 0, mx = 0;
        for (int s = lane; s < slots; s += GROUP) {
            const int2 kv = tab[g][s];
            if (kv.x < 0 || kv.y < smin) continue;
            ++c;
            mx = kv.y > mx ? kv.y : mx;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            c += __shfl_xor(c, off);
            const int om = __shfl_xor(mx, off);
            mx = om > mx ? om : mx;
        }
        if constexpr (GROUP == 256) {
            __shared__ int red_c[4], red_m[4];
            const int w = threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 0) { red_c[w] = c; red_m[w] = mx; }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int o = 1; o < 4; ++o) { c += red_c[o]; mx = red_m[o] > mx ? red_m[o] : mx; }
        }
        if (lane == 0) {
            cnt[i] = c;
            if (mx > 0) atomicMax(smax, mx);
        }
    }
}

// Rows beyond the workgroup class: workgroup b owns the dense row S = scratch + b * n (all zero between rows) and takes the rows b,
// b + gridDim.x, ...  The counts are added into S by integer atomics; the product is then walked again, and every increment exchanges its
// slot for 0: the one that gets the count back speaks for the slot, so each distinct j is seen once and S is zero again afterwards.
template <bool FILL>
__global__ __launch_bounds__(256) void snn_dense_kernel(const int *__restrict__ rows, int nrows, const int *__restrict__ idx,
                                                        const long long *__restrict__ rptr, const int *__restrict__ R, int K, int smin,
                                                        unsigned *__restrict__ scratch, long long n, long long *__restrict__ cnt,
                                                        int *__restrict__ smax, const long long *__restrict__ rp,
                                                        u64 *__restrict__ packed) {
    __shared__ int pos_s, max_s;
    unsigned *S = scratch + static_cast<long long>(blockIdx.x) * n;
    const int tid = threadIdx.x;
    for (int ri = blockIdx.x; ri < nrows; ri += gridDim.x) {
        const long long i = rows[ri];
        if (tid == 0) { pos_s = 0; max_s = 0; }
        row_product<256>(idx, rptr, R, i, K, tid, [&](int j) { atomicAdd(&S[j], 1u); });
        __threadfence();
        __syncthreads();
        const long long b0 = FILL ? rp[i] : 0, room = FILL ? rp[i + 1] - b0 : 0;
        row_product<256>(idx, rptr, R, i, K, tid, [&](int j) {
            const unsigned s = __hip_atomic_exchange(&S[j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (static_cast<int>(s) < smin || s == 0u) return;
            const int at = atomicAdd(&pos_s, 1);
            if (FILL) {
                if (at < room) packed[b0 + at] = pack(i, j, static_cast<int>(s));
            } else {
                atomicMax(&max_s, static_cast<int>(s));
            }
        });
        __threadfence();
        __syncthreads();                                     // (the zeros are in place)
        if (!FILL && tid == 0) {
            cnt[i] = pos_s;
            if (max_s > 0) atomicMax(smax, max_s);
        }
        __syncthreads();                                     // (pos_s / max_s are free again)
    }
}

__global__ __launch_bounds__(256) void snn_unpack_kernel(const u64 *__restrict__ sorted, long long nnz, const double *__restrict__ tab,
                                                         int *__restrict__ col, double *__restrict__ val, int *__restrict__ shared) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    const unsigned w = static_cast<unsigned>(sorted[e]);
    const int s = static_cast<int>(w & 255u) + 1;
    col[e] = static_cast<int>(w >> 8);
    val[e] = tab[s];
    if (shared) shared[e] = s;
}

// the reverse lists and the row classes of one set of lists
struct Rev {
    DevBuf<long long> rptr, t;               // n + 1, n
    DevBuf<int> R;                           // n k
    RowClasses rows;
    DevBuf<unsigned> scratch;
};

void build_reverse(const std::string &who, const DevBuf<int> &idx, long long n, int K, Rev &V) {
    Ctx &c = ctx();
    KernelTimer timer("snn_reverse");
    const long long ne = n * K, nk = n * (K + 1);
    DevBuf<long long> deg(n + 1);
    DevBuf<u64> word(1);
    SHARP_HIP_CHECK(hipMemsetAsync(word.p, 0xFF, sizeof(u64), c.stream));
    hipLaunchKernelGGL(snn_fill_ll_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, c.stream, deg.p, n, 1ll, 0ll);
    hipLaunchKernelGGL(snn_check_degree_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c.stream, idx.p, n, K, ne, deg.p, word.p);
    launch_check("snn_check_degree_kernel");
    u64 w = NN_OK;
    word.download(&w, 1);
    if (w != NN_OK) throw_list_fault(who, w);
    V.rptr.alloc(n + 1);
    Scratch tmp;
    exclusive_scan(deg.p, V.rptr.p, static_cast<size_t>(n + 1), tmp);
    {
        DevBuf<u64> keys(nk), keys_s(nk);
        DevBuf<int> vals(nk);
        V.R.alloc(nk);
        hipLaunchKernelGGL(snn_revkey_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, c.stream, idx.p, n, K, keys.p, vals.p);
        launch_check("snn_revkey_kernel");
        reverse_sort_by_target(keys.p, keys_s.p, vals.p, V.R.p, n, nk);   // (synchronises)
    }
    V.t.alloc(n);
    hipLaunchKernelGGL(snn_work_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, idx.p, deg.p, n, K, V.t.p);
    launch_check("snn_work_kernel");
    std::vector<long long> ht(n);
    V.t.download(ht.data(), ht.size());                     // (synchronises: deg and tmp leave scope)
    V.rows.classify(ht, kSnnWaveCap, kSnnBlockCap, false);
    if (V.rows.n_dense) {                                         // dense rows of n counters each: at most 512 MB in all
        V.scratch.alloc(static_cast<size_t>(V.rows.dense_grid) * n);
        V.scratch.zero();
    }
}

template <bool FILL>
void run_product(const DevBuf<int> &idx, long long n, int K, int smin, Rev &V, long long *cnt, int *smax, const long long *rp, u64 *packed) {
    Ctx &c = ctx();
    if (V.rows.n_wave) {
        hipLaunchKernelGGL((snn_lds_kernel<64, kSnnWaveSlots, FILL>), dim3(grid_for(V.rows.n_wave, 2)), dim3(128), 0, c.stream, V.rows.rows_wave.p, V.rows.n_wave,
                           idx.p, V.rptr.p, V.R.p, V.t.p, K, smin, cnt, smax, rp, packed);
        launch_check("snn_lds_kernel<64>");
    }
    if (V.rows.n_block) {
        hipLaunchKernelGGL((snn_lds_kernel<256, kSnnBlockSlots, FILL>), dim3(V.rows.n_block), dim3(256), 0, c.stream, V.rows.rows_block.p, V.rows.n_block, idx.p,
                           V.rptr.p, V.R.p, V.t.p, K, smin, cnt, smax, rp, packed);
        launch_check("snn_lds_kernel<256>");
    }
    if (V.rows.n_dense) {
        hipLaunchKernelGGL(snn_dense_kernel<FILL>, dim3(V.rows.dense_grid), dim3(256), 0, c.stream, V.rows.rows_dense.p, V.rows.n_dense, idx.p, V.rptr.p, V.R.p, K,
                           smin, V.scratch.p, n, cnt, smax, rp, packed);
        launch_check("snn_dense_kernel");
    }
}

}  // namespace

int snn_min_shared(int k, double prune) {
    for (int s = 1; s < k; ++s)
        if (static_cast<double>(s) / static_cast<double>(2 * k - s) >= prune) return s;
    return k;
}

void snn_check_args(const std::string &who, long long n, int K, double prune) {
    SHARP_REQUIRE(n >= 2 && n <= kSnnMaxN, who + ": need 2 <= n <= 16777216 rows");
    SHARP_REQUIRE(K >= 1 && K <= 255 && K <= n - 1, who + ": need 1 <= K <= 255 neighbours per row and K <= n - 1");
    SHARP_REQUIRE(prune >= 0.0 && prune <= 1.0, who + ": prune must be in [0, 1]");   // (false for NaN too)
}

void snn_graph(const std::string &who, const DevBuf<int> &idx, long long n, int K, double prune, bool count_only, Graph &G,
               DevBuf<int> *shared, long long cap) {
    Ctx &c = ctx();
    snn_check_args(who, n, K, prune);
    const int k = K + 1, smin = snn_min_shared(k, prune);
    Rev V;
    build_reverse(who, idx, n, K, V);
    DevBuf<long long> cnt(n + 1);
    DevBuf<int> smax(1);
    G.n = n;
    G.row_ptr.alloc(n + 1);
    long long nnz = 0;
    int hmax = 0;
    {
        KernelTimer timer("snn_count");
        smax.zero();
        SHARP_HIP_CHECK(hipMemsetAsync(cnt.p + n, 0, sizeof(long long), c.stream));
        run_product<false>(idx, n, K, smin, V, cnt.p, smax.p, nullptr, nullptr);
        Scratch tmp;
        exclusive_scan(cnt.p, G.row_ptr.p, static_cast<size_t>(n + 1), tmp);
        SHARP_HIP_CHECK(hipMemcpyAsync(&nnz, G.row_ptr.p + n, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
        SHARP_HIP_CHECK(hipMemcpyAsync(&hmax, smax.p, sizeof(int), hipMemcpyDeviceToHost, c.stream));
        stream_sync();
    }
    SHARP_REQUIRE(nnz >= 0 && nnz < kSnnMaxNnz, who + ": the graph holds " + std::to_string(nnz) + " entries; need fewer than 2^38");
    SHARP_REQUIRE(hmax >= 0 && hmax <= k, who + ": a pair shares an impossible number of neighbours");
    G.nnz = nnz;
    G.wmax = hmax > 0 ? static_cast<double>(hmax) / static_cast<double>(2 * k - hmax) : 0.0;
    if (count_only) return;
    SHARP_REQUIRE(cap < 0 || cap >= nnz, who + ": cap is smaller than the graph's " + std::to_string(nnz) + " entries");
    // the unsorted and the sorted words and the sort's own copy of them, col, val and shared
    size_t free_b = 0, total_b = 0;
    SHARP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    SHARP_REQUIRE(static_cast<double>(nnz) * 40.0 + 67108864.0 <= static_cast<double>(free_b),
                  who + ": the graph's " + std::to_string(nnz) + " entries do not fit the device's free memory");
    G.col.alloc(nnz);
    G.val.alloc(nnz);
    if (shared) shared->alloc(nnz);
    if (nnz == 0) return;
    DevBuf<u64> packed(nnz), sorted(nnz);
    {
        KernelTimer timer("snn_fill");
        run_product<true>(idx, n, K, smin, V, nullptr, nullptr, G.row_ptr.p, packed.p);
    }
    {
        KernelTimer timer("snn_sort");
        std::vector<double> tab(k + 1, 0.0);
        for (int s = 1; s <= k; ++s) tab[s] = static_cast<double>(s) / static_cast<double>(2 * k - s);
        DevBuf<double> dtab(tab.size());
        dtab.upload(tab.data(), tab.size());
        // by (row, column): the rows are in place already, so the sort only orders each row's range; keys are unique
        Scratch tmp;
        sort_keys(packed.p, sorted.p, static_cast<size_t>(nnz), 8, key_bits(static_cast<u64>(n) << 32), tmp);
        hipLaunchKernelGGL(snn_unpack_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, c.stream, sorted.p, nnz, dtab.p, G.col.p, G.val.p,
                           shared ? shared->p : nullptr);
        launch_check("snn_unpack_kernel");
        stream_sync();                                       // (the temporaries leave scope)
    }
}

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_snn_row_caps(int *wave_cap, int *block_cap) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(wave_cap && block_cap, "sharp_snn_row_caps: null output");
    *wave_cap = kSnnWaveCap;
    *block_cap = kSnnBlockCap;
    SHARP_API_END
}

int sharp_snn_graph(const int *index, long long n, int K, double prune, long long cap, long long *row_ptr, int *col, double *val, int *shared,
                    long long *nnz) {
    SHARP_API_BEGIN
    const std::string w("snn_graph");
    SHARP_REQUIRE(index && row_ptr && nnz, w + ": null index / row_ptr / nnz");
    SHARP_REQUIRE((col == nullptr) == (val == nullptr), w + ": give col and val together (both NULL: count only)");
    SHARP_REQUIRE(col || !shared, w + ": shared needs col and val");
    snn_check_args(w, n, K, prune);
    ctx();
    DevBuf<int> idx(static_cast<size_t>(n) * K);
    idx.upload(index, static_cast<size_t>(n) * K);
    Graph G;
    DevBuf<int> ds;
    try {
        snn_graph(w, idx, n, K, prune, col == nullptr, G, shared ? &ds : nullptr, col ? std::max<long long>(cap, 0) : -1);
    } catch (...) {
        *nnz = G.nnz;                                        // (a cap too small: the needed count)
        throw;
    }
    *nnz = G.nnz;
    G.row_ptr.download(row_ptr, n + 1);
    if (col && G.nnz) {
        G.col.download(col, G.nnz);
        G.val.download(val, G.nnz);
        if (shared) ds.download(shared, G.nnz);
    }
    SHARP_API_END
}

}  // extern "C"
