// graph_prim.hpp -- the rocprim wrappers that graph.hpp declares, defined here as templates: one source, but every translation unit that
// sorts or scans (tsne, umap, louvain, snn, knn_descent, graph) instantiates rocprim's kernels in its own code object, as before the
// wrappers existed.  With every instantiation in graph.hip's single code object the stages' first full-size calls were slower (umap_sym
// in tools/bench_umap.py 0.69-0.81 ms against 0.48-0.51, snn_reverse 2.97-3.30 against 2.68-2.81: profiles/graph_helpers_bench.json).
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include "graph.hpp"

namespace sharp {

// call(storage, bytes) is a rocprim entry: asked for its temporary storage (unless the buffer is sized for it already), then run on a
// scratch buffer that holds at least that
template <typename F>
void with_scratch(Scratch &s, bool sized, F call) {
    if (!sized) {
        size_t bytes = 0;
        SHARP_HIP_CHECK(call(nullptr, bytes));
        bytes = std::max<size_t>(bytes, 1);
        if (bytes > s.n) s.alloc(bytes);
    }
    size_t bytes = s.n;
    SHARP_REQUIRE(s.n > 0, "a rocprim call on a scratch buffer that no earlier call has sized");
    SHARP_HIP_CHECK(call(s.p, bytes));
}

template <typename K, typename V>
void sort_pairs(K *keys, K *keys_out, V *vals, V *vals_out, size_t count, unsigned begin_bit, unsigned end_bit, Scratch &scratch, bool sized) {
    with_scratch(scratch, sized, [&](void *p, size_t &bytes) {
        return rocprim::radix_sort_pairs(p, bytes, keys, keys_out, vals, vals_out, count, begin_bit, end_bit, ctx().stream);
    });
}

template <typename K>
void sort_keys(K *keys, K *keys_out, size_t count, unsigned begin_bit, unsigned end_bit, Scratch &scratch, bool sized) {
    with_scratch(scratch, sized, [&](void *p, size_t &bytes) {
        return rocprim::radix_sort_keys(p, bytes, keys, keys_out, count, begin_bit, end_bit, ctx().stream);
    });
}

template <typename T>
void exclusive_scan(T *in, T *out, size_t count, Scratch &scratch, bool sized) {
    with_scratch(scratch, sized, [&](void *p, size_t &bytes) {
        return rocprim::exclusive_scan(p, bytes, in, out, T(0), count, rocprim::plus<T>(), ctx().stream);
    });
}

template <typename V, typename Op>
size_t merge_by_key(u64 *keys, V *vals, size_t ne, u64 key_range, u64 *keys_s, V *vals_s, u64 *keys_out, V *vals_out, MergeScratch &s) {
    sort_pairs(keys, keys_s, vals, vals_s, ne, 0, key_bits(key_range), s.tmp);
    s.count.alloc(1);
    with_scratch(s.tmp, false, [&](void *p, size_t &bytes) {
        return rocprim::reduce_by_key(p, bytes, keys_s, vals_s, ne, keys_out, vals_out, s.count.p, Op(), rocprim::equal_to<u64>(), ctx().stream);
    });
    size_t nnz = 0;
    s.count.download(&nnz, 1);
    return nnz;
}

}  // namespace sharp
