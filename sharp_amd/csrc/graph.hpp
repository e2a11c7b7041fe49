// graph.hpp -- what the neighbour-graph stages share: the CSR types and the upload of a caller's checked CSR, the
// launch-grid, butterfly and hash helpers, the fixed-order reduction, the rocprim calls behind plain host functions, the "unsorted
// (row * n + col, value) entries -> CSR" builder, the wave / workgroup / dense row classes, iota and the reverse-list sort.  t-SNE's P
// (tsne.hip), UMAP's fuzzy graph (umap.hip), Louvain's levels (louvain.hip), the SNN graph (snn.hip) and NN-descent (knn_descent.hip)
// are built from these; csr_to_device serves umap_epochs (umap.hip), the Lanczos solvers (spectral_dev.hpp) and Louvain / Leiden on a
// caller's graph (louvain.hip).  How lists become a graph on the device is graph_source.hpp's.  The rocprim wrappers are declared here
// and defined in graph_prim.hpp, which the files that sort or scan include.
#pragma once
#include <algorithm>
#include <vector>

#include "common.hpp"

namespace sharp {

using u64 = unsigned long long;

// ---- graphs on the device -------------------------------------------------------------------------------------------------------------
// rows sorted by column
template <typename V>
struct Csr {
    long long n = 0, nnz = 0;
    DevBuf<long long> row_ptr;   // n + 1
    DevBuf<int> col;             // nnz
    DevBuf<V> val;               // nnz
};
// a symmetric float-weighted graph and its largest weight: UMAP's W = A + A^T - A o A^T, the SNN graph, what louvain_quantise takes
struct Graph : Csr<double> {
    double wmax = 0.0;
};
// a caller's CSR (host; n rows, row_ptr[n] entries) that its entry has checked, placed in G on ctx().stream; val may be null (the
// pattern alone); wmax: the largest weight, found by that check.  A graph without an entry keeps one slot per array.
SHARP_LOCAL inline void csr_to_device(const long long *row_ptr, const int *col, const double *val, long long n, double wmax, Graph &G) {
    G.n = n;
    G.nnz = row_ptr[n];
    G.wmax = wmax;
    const size_t slots = static_cast<size_t>(std::max<long long>(G.nnz, 1));
    G.row_ptr.alloc(n + 1);
    G.row_ptr.upload(row_ptr, n + 1);
    G.col.alloc(slots);
    if (G.nnz) G.col.upload(col, G.nnz);
    if (val) {
        G.val.alloc(slots);
        if (G.nnz) G.val.upload(val, G.nnz);
    }
}

// ---- small helpers --------------------------------------------------------------------------------------------------------------------
// workgroups of `per` items that cover n items (one, doing nothing, for n = 0)
inline unsigned grid_for(long long n, int per) { return static_cast<unsigned>((std::max<long long>(n, 1) + per - 1) / per); }

// the 64-lane butterfly sum: every lane leaves with the same bits
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// the splitmix64 finaliser: DESIGN.md §13's mix, the hash behind every draw of UMAP, NN-descent and Louvain
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// v[i] = i
void iota(int *v, long long n);

// ---- the fixed-order reduction --------------------------------------------------------------------------------------------------------
// out[0] = the fold of v[0 .. n): workgroup b folds its chunk of max(256, ceil(n / kRedBlocks)) values (256 strided running folds, then a
// tree), one workgroup folds the workgroups' results the same way.  The order depends on n alone.  Max and AbsMax start from 0 (Max is
// for values >= 0).  part: kRedBlocks doubles, out: a device scalar.
constexpr int kRedBlocks = 1024;
enum class Fold { Sum, Max, AbsMax };
void fixed_reduce(Fold f, const double *v, long long n, double *part, double *out);
// the first stage alone, for a caller that folds the workgroups' results on the host: part[0 .. fixed_reduce_blocks(n))
unsigned fixed_reduce_blocks(long long n);
void fixed_reduce_parts(Fold f, const double *v, long long n, double *part);

// ---- rocprim behind host functions (defined in graph_prim.hpp) ------------------------------------------------------------------------
// All on ctx().stream.  The caller holds the call's temporary storage as a Scratch and lets it go where it lets its other buffers go,
// behind the stage's synchronisation, as every stage did before these wrappers existed: hipFree synchronises the device, so a wrapper
// that released the storage itself would wait for its own call before the host could enqueue the next one.  A call asks rocprim for the
// size it needs and grows the buffer when it holds less.  sized = true skips that question: for a loop (the Barnes-Hut tree, Louvain's
// rounds, NN-descent's projections) whose buffer an earlier call of the same kind and of the same or a larger count has sized, so that a
// round makes one rocprim call per operation and allocates nothing.  The inputs are only read.  They are non-const pointers, as the
// stages handed them to rocprim before: rocprim instantiates its kernels on the iterator types, so every call keeps the instantiation
// it had (reverse_sort_by_target, below, keeps its const inputs for the same reason).
// the number of low bits that hold every key <= range (at least 1): a sort's end_bit
inline unsigned key_bits(u64 range) {
    unsigned bits = 1;
    while (bits < 64 && (range >> bits) != 0) ++bits;
    return bits;
}
using Scratch = DevBuf<unsigned char>;
// stable, ascending in the bits [begin_bit, end_bit); (K, V): (u64, double), (u64, u64), (u64, int)
template <typename K, typename V>
void sort_pairs(K *keys, K *keys_out, V *vals, V *vals_out, size_t count, unsigned begin_bit, unsigned end_bit, Scratch &scratch, bool sized = false);
// K: u64, double
template <typename K>
void sort_keys(K *keys, K *keys_out, size_t count, unsigned begin_bit, unsigned end_bit, Scratch &scratch, bool sized = false);
// out[i] = in[0] + .. + in[i - 1]; T: int, unsigned, long long
template <typename T>
void exclusive_scan(T *in, T *out, size_t count, Scratch &scratch, bool sized = false);

// Reverse lists by sorted 64-bit keys: keys[e] = (target << 32 | order within the target), vals[e] = the source; the stable sort leaves
// every target's sources together, ascending in the keys' low words, in keys_s / vals_s (ne entries each; targets below n).  The join's
// reverse candidates (knn_descent.hip) and the SNN graph's reverse lists (snn.hip) are both made this way.  Synchronises.  Defined in
// knn_descent.hip, whose code object has held this sort from the start.
void reverse_sort_by_target(const u64 *keys, u64 *keys_s, const int *vals, int *vals_s, long long n, long long ne);

// ---- unsorted entries -> CSR ----------------------------------------------------------------------------------------------------------
// the ops that merge the entries of one key; both are commutative, so the sort's order of equal keys does not reach the result
struct Plus {
    template <typename T>
    __host__ __device__ T operator()(const T &x, const T &y) const { return x + y; }
};
struct FuzzyUnion {   // UMAP's x + y - x y
    __host__ __device__ double operator()(const double &x, const double &y) const { return x + y - x * y; }
};
// Step 1: ne entries (keys[e] = row * n + col < key_range, vals[e]) in any order -> sorted by key, the entries of equal keys merged by Op,
// in keys_out / vals_out (ne slots each; keys_out may be keys, vals_out may be vals); keys_s / vals_s: ne slots each for the sort;
// scratch: the two rocprim calls' temporary storage and the count on the device, let go by the caller like any Scratch.
// Returns the number of merged entries (synchronises).  (V, Op): (double, Plus), (double, FuzzyUnion), (u64, Plus).
// The caller checks the count and folds the merged values as it needs (t-SNE's total, UMAP's maximum) before step 2.
struct MergeScratch {
    Scratch tmp;
    DevBuf<size_t> count;
};
template <typename V, typename Op>
size_t merge_by_key(u64 *keys, V *vals, size_t ne, u64 key_range, u64 *keys_s, V *vals_s, u64 *keys_out, V *vals_out, MergeScratch &scratch);
// Step 2: nnz merged keys -> col (and row when wanted) and row_ptr (n + 1).  empty_rows false: one launch that also marks the row
// starts, for graphs in which every row holds an entry; true: a second launch takes row_ptr[r] = the first entry with key >= r n by
// binary search (the same numbers where no row is empty).  val (when wanted) = vals, or vals / divisor[0] with a device scalar.
// V: double, u64.
template <typename V>
void merged_to_csr(const u64 *keys, long long nnz, long long n, bool empty_rows, long long *row_ptr, int *col, int *row = nullptr,
                   const V *vals = nullptr, const V *divisor = nullptr, V *val = nullptr);

// ---- row classes ----------------------------------------------------------------------------------------------------------------------
// The rows of a graph dealt by a per-row size to three kernels: up to wave_cap one wave per row, up to block_cap one workgroup, beyond
// that a workgroup per row with a dense row of n slots in HBM; dense_grid workgroups own such a row each: at most 128 and at most 2^27
// slots in all.  The owner allocates and zeroes dense_grid * n slots of its own type when n_dense > 0.
struct RowClasses {
    DevBuf<int> rows_wave, rows_block, rows_dense;   // the ids of each class's rows, ascending
    int n_wave = 0, n_block = 0, n_dense = 0, dense_grid = 0;
    // size: one value per row (host); skip_empty: a row of size 0 joins no class.  Synchronises.
    void classify(const std::vector<long long> &size, long long wave_cap, long long block_cap, bool skip_empty);
};

}  // namespace sharp
