// graph.hip -- the kernels behind graph.hpp.  Integer work and fixed-order folds only: nothing here
// depends on the order in which workgroups run.
#include "graph.hpp"

namespace sharp {
namespace {

__global__ __launch_bounds__(256) void iota_kernel(int *__restrict__ v, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) v[i] = static_cast<int>(i);
}

template <Fold F>
__device__ __forceinline__ double fold(double a, double x) {
    return F == Fold::Sum ? a + x : fmax(a, F == Fold::AbsMax ? fabs(x) : x);
}

template <Fold F>
__global__ __launch_bounds__(256) void reduce_kernel(const double *__restrict__ v, long long n, long long chunk, double *__restrict__ part) {
    __shared__ double s[256];
    const int tid = threadIdx.x;
    const long long b0 = static_cast<long long>(blockIdx.x) * chunk, e = b0 + chunk < n ? b0 + chunk : n;
    double a = 0.0;
    for (long long k = b0 + tid; k < e; k += 256) a = fold<F>(a, v[k]);
    s[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s[tid] = fold<F>(s[tid], s[tid + w]);
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = s[0];
}

inline long long reduce_chunk(long long n) { return std::max<long long>(256, (n + kRedBlocks - 1) / kRedBlocks); }

// out == nullptr: the first stage alone
template <Fold F>
void reduce_launch(const double *v, long long n, double *part, double *out) {
    const long long chunk = reduce_chunk(n);
    const unsigned nb = fixed_reduce_blocks(n);
    hipLaunchKernelGGL(reduce_kernel<F>, dim3(nb), dim3(256), 0, ctx().stream, v, n, chunk, part);
    if (out)
        hipLaunchKernelGGL(reduce_kernel<F>, dim3(1), dim3(256), 0, ctx().stream, part, static_cast<long long>(nb), static_cast<long long>(nb), out);
    launch_check("reduce_kernel");
}

template <typename V>
__global__ __launch_bounds__(256) void csr_kernel(const u64 *__restrict__ keys, long long nnz, long long n, bool mark, long long *__restrict__ rp,
                                                  int *__restrict__ col, int *__restrict__ row, const V *__restrict__ vals,
                                                  const V *__restrict__ divisor, V *__restrict__ val) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    const u64 un = static_cast<u64>(n);
    const long long r = static_cast<long long>(keys[e] / un);
    col[e] = static_cast<int>(keys[e] - static_cast<u64>(r) * un);
    if (row) row[e] = static_cast<int>(r);
    if (val) val[e] = divisor ? vals[e] / divisor[0] : vals[e];
    if (!mark) return;
    if (e == 0 || static_cast<long long>(keys[e - 1] / un) != r) rp[r] = e;   // (every row holds an entry)
    if (e == nnz - 1) rp[n] = nnz;
}

// rp[r] = the first entry whose key is >= r * n, r = 0 .. n (a row without entries gets an empty range)
__global__ __launch_bounds__(256) void csr_rowptr_kernel(const u64 *__restrict__ keys, long long nnz, long long n, long long *__restrict__ rp) {
    const long long r = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (r > n) return;
    const u64 want = static_cast<u64>(r) * static_cast<u64>(n);
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    rp[r] = lo;
}

}  // namespace

void iota(int *v, long long n) {
    hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, v, n);
    launch_check("iota_kernel");
}

unsigned fixed_reduce_blocks(long long n) { return static_cast<unsigned>((std::max<long long>(n, 1) + reduce_chunk(n) - 1) / reduce_chunk(n)); }

void fixed_reduce_parts(Fold f, const double *v, long long n, double *part) { fixed_reduce(f, v, n, part, nullptr); }

void fixed_reduce(Fold f, const double *v, long long n, double *part, double *out) {
    if (f == Fold::Sum) reduce_launch<Fold::Sum>(v, n, part, out);
    else if (f == Fold::Max) reduce_launch<Fold::Max>(v, n, part, out);
    else reduce_launch<Fold::AbsMax>(v, n, part, out);
}

template <typename V>
void merged_to_csr(const u64 *keys, long long nnz, long long n, bool empty_rows, long long *row_ptr, int *col, int *row, const V *vals,
                   const V *divisor, V *val) {
    hipLaunchKernelGGL(csr_kernel<V>, dim3(grid_for(nnz, 256)), dim3(256), 0, ctx().stream, keys, nnz, n, !empty_rows, row_ptr, col, row, vals,
                       divisor, val);
    if (empty_rows) hipLaunchKernelGGL(csr_rowptr_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, ctx().stream, keys, nnz, n, row_ptr);
    launch_check("csr_kernel");
}
template void merged_to_csr<double>(const u64 *, long long, long long, bool, long long *, int *, int *, const double *, const double *, double *);
template void merged_to_csr<u64>(const u64 *, long long, long long, bool, long long *, int *, int *, const u64 *, const u64 *, u64 *);

void RowClasses::classify(const std::vector<long long> &size, long long wave_cap, long long block_cap, bool skip_empty) {
    const long long n = static_cast<long long>(size.size());
    std::vector<int> a, b, d;
    for (long long v = 0; v < n; ++v) {
        if (skip_empty && size[v] == 0) continue;
        (size[v] <= wave_cap ? a : size[v] <= block_cap ? b : d).push_back(static_cast<int>(v));
    }
    auto up = [](DevBuf<int> &buf, const std::vector<int> &h) { buf.alloc(h.size()); if (!h.empty()) buf.upload(h.data(), h.size()); };
    up(rows_wave, a); up(rows_block, b); up(rows_dense, d);
    n_wave = static_cast<int>(a.size()); n_block = static_cast<int>(b.size()); n_dense = static_cast<int>(d.size());
    dense_grid = n_dense ? static_cast<int>(std::min<long long>(n_dense, std::max<long long>(1, std::min<long long>(128, (1ll << 27) / n)))) : 0;
    stream_sync();                                           // (the host vectors go out of scope)
}

}  // namespace sharp
