// spectral_dev.hpp -- what the two Lanczos solvers share (umap_spectral.hip; diffmap.hip): the operator
// y_i = s_i sum_j W_ij s_j x_j, the fixed-order dot products, the Gram-Schmidt update, the scaling, the hashed start vector and the
// check-and-upload of a caller's CSR.  The kernels were written for §15 and are here as they were: each translation unit that includes
// this file instantiates them in its own code object, in an unnamed namespace.
#pragma once
#include <algorithm>
#include <cfloat>
#include <string>

#include "umap.hpp"

namespace sharp {
namespace {

// y_i = s_i sum_j W_ij s_j x_j
__global__ __launch_bounds__(256) void spmv_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                   const double *__restrict__ s, const double *__restrict__ x, double *__restrict__ y, long long n) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long e1 = rp[i + 1];
    double a = 0.0;
    for (long long e = rp[i] + lane; e < e1; e += 64) { const int j = col[e]; a += val[e] * s[j] * x[j]; }
    a = wave_sum(a);
    if (lane == 0) y[i] = s[i] * a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the basis: Q holds its vectors column by column (n contiguous doubles each)
// ---------------------------------------------------------------------------------------------------------------------------
// part[j * nb + b] = sum over chunk b of Q_j[k] u[k]: strided per thread, then a tree (grid: nb x ncols)
__global__ __launch_bounds__(256) void dots_kernel(const double *__restrict__ Q, const double *__restrict__ u, long long n, long long chunk,
                                                   double *__restrict__ part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const double *q = Q + static_cast<long long>(blockIdx.y) * n;
    const long long b0 = static_cast<long long>(blockIdx.x) * chunk, e = b0 + chunk < n ? b0 + chunk : n;
    double a = 0.0;
    for (long long k = b0 + tid; k < e; k += 256) a += q[k] * u[k];
    sh[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    if (tid == 0) part[static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x] = sh[0];
}

// out[j] = the nb partials of column j folded the same way (its square root when root); the last column's sum also to *last
__global__ __launch_bounds__(256) void fold_kernel(const double *__restrict__ part, int nb, double *__restrict__ out, int root,
                                                   double *__restrict__ last) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const double *p = part + static_cast<long long>(blockIdx.x) * nb;
    double a = 0.0;
    for (int k = tid; k < nb; k += 256) a += p[k];
    sh[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        out[blockIdx.x] = root ? sqrt(sh[0]) : sh[0];
        if (last && blockIdx.x == gridDim.x - 1) *last = sh[0];
    }
}

// u_i -= sum_j Q_j[i] c_j, the columns in ascending order
__global__ __launch_bounds__(256) void apply_kernel(const double *__restrict__ Q, int ncols, const double *__restrict__ c, double *__restrict__ u,
                                                    long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double a = u[i];
    for (int j = 0; j < ncols; ++j) a -= Q[static_cast<long long>(j) * n + i] * c[j];
    u[i] = a;
}

// out = u / *nrm (zeros when the norm is zero: the Krylov space is exhausted, which the host sees in beta); out may be u
__global__ __launch_bounds__(256) void scale_kernel(const double *u, const double *__restrict__ nrm, double *out, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double b = nrm[0];
    out[i] = b > 0.0 ? u[i] / b : 0.0;
}

// x_i = (mix(0x9E3779B97F4A7C15 + i) >> 11) 2^-53 - 0.5
__global__ __launch_bounds__(256) void start_kernel(double *__restrict__ x, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) x[i] = static_cast<double>(mix64(0x9E3779B97F4A7C15ull + static_cast<unsigned long long>(i)) >> 11) * 0x1.0p-53 - 0.5;
}

struct Reducer {   // the chunking of a length-n sum and the partials' buffer
    long long n, chunk;
    unsigned nb;
    DevBuf<double> part;
    Reducer(long long n_, int max_cols) : n(n_) {
        chunk = std::max<long long>(256, (n + kRedBlocks - 1) / kRedBlocks);
        nb = static_cast<unsigned>((n + chunk - 1) / chunk);
        part.alloc(static_cast<size_t>(nb) * max_cols);
    }
    // out[j] = Q_j . u for j < ncols (root: the square root of it); last: also receives the last column's sum
    void dots(const double *Q, int ncols, const double *u, double *out, bool root = false, double *last = nullptr) {
        hipLaunchKernelGGL(dots_kernel, dim3(nb, ncols), dim3(256), 0, ctx().stream, Q, u, n, chunk, part.p);
        hipLaunchKernelGGL(fold_kernel, dim3(ncols), dim3(256), 0, ctx().stream, part.p, static_cast<int>(nb), out, root ? 1 : 0, last);
        launch_check("dots_kernel");
    }
};

void apply(const double *Q, int ncols, const double *c, double *u, long long n) {
    hipLaunchKernelGGL(apply_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, Q, ncols, c, u, n);
    launch_check("apply_kernel");
}

void scale(const double *u, const double *nrm, double *out, long long n) {
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, u, nrm, out, n);
    launch_check("scale_kernel");
}

void spmv(const UmapGraph &G, const double *s, const double *x, double *y) {
    hipLaunchKernelGGL(spmv_kernel, dim3(grid_for(G.n, 4)), dim3(256), 0, ctx().stream, G.row_ptr.p, G.col.p, G.val.p, s, x, y, G.n);
    launch_check("spmv_kernel");
}

// a caller's CSR pattern (host) checked and placed on the device; val may be null (the pattern alone)
void upload_csr(const char *who, const long long *row_ptr, const int *col, const double *val, long long n, UmapGraph &G) {
    const std::string w(who);
    SHARP_REQUIRE(row_ptr && (col || row_ptr[n] == 0), w + ": null row_ptr / col");
    SHARP_REQUIRE(row_ptr[0] == 0, w + ": row_ptr must start at 0");
    for (long long i = 0; i < n; ++i)
        SHARP_REQUIRE(row_ptr[i] <= row_ptr[i + 1] && row_ptr[i + 1] - row_ptr[i] <= n, w + ": row_ptr is not monotone, or a row holds more than n entries");
    for (long long e = 0; e < row_ptr[n]; ++e) SHARP_REQUIRE(col[e] >= 0 && col[e] < n, w + ": a column index out of range");
    double wmax = 0.0;
    if (val)
        for (long long i = 0; i < n; ++i) {
            double deg = 0.0;
            for (long long e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
                SHARP_REQUIRE(val[e] >= 0.0 && val[e] <= DBL_MAX, w + ": a weight that is NA / NaN / Inf or negative");
                deg += val[e];
                wmax = std::max(wmax, val[e]);
            }
            SHARP_REQUIRE(row_ptr[i] == row_ptr[i + 1] || (deg > 0.0 && deg <= DBL_MAX), w + ": a row whose weights sum to 0 or overflow");
        }
    csr_to_device(row_ptr, col, val, n, wmax, G);
}

}  // namespace
}  // namespace sharp
