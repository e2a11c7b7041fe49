// dist_pairs.hpp -- what the pair loops over observations share (dist_kernel in dist.hip, the matrix-free silhouette in validity.hip):
// the tile constants, the four difference metrics of R's dist() and the index into R's dist vector.  One definition, so that a
// distance computed inside the silhouette is bitwise the value sharp_dist() returns.
#pragma once
#include <hip/hip_runtime.h>

namespace sharp {

constexpr int DT = 64;          // pairs tile: DT x DT per workgroup of 256 lanes, a 4 x 4 block of pairs per lane
constexpr int DK = 32;          // features staged per pass
constexpr int DLD = DT + 2;     // LDS row stride in doubles: 16-byte aligned rows, transposed staging writes spread over the banks

struct DistEuclid {
    static __device__ __forceinline__ void acc(double &a, double d, double) { a += d * d; }
    static __device__ __forceinline__ double fin(double a, double) { return sqrt(a); }
};
struct DistMaximum {
    static __device__ __forceinline__ void acc(double &a, double d, double) { const double f = fabs(d); a = f > a ? f : a; }
    static __device__ __forceinline__ double fin(double a, double) { return a; }
};
struct DistManhattan {
    static __device__ __forceinline__ void acc(double &a, double d, double) { a += fabs(d); }
    static __device__ __forceinline__ double fin(double a, double) { return a; }
};
struct DistMinkowski {
    static __device__ __forceinline__ void acc(double &a, double d, double mp) { a += pow(fabs(d), mp); }
    static __device__ __forceinline__ double fin(double a, double mp) { return pow(a, 1.0 / mp); }
};

// R's dist vector: pair (i > j) at n j - j (j + 1) / 2 + i - j - 1 (column-wise lower triangle = scipy's pdist order)
__device__ __forceinline__ long long cond_index(int n, int j, int i) {
    return static_cast<long long>(n) * j - static_cast<long long>(j) * (j + 1) / 2 + (i - j - 1);
}

// dist.hip: R's dist vector (device, n (n - 1) / 2) -> the full symmetric matrix D (device, nld x nld with nld = dist_nld(n), n rounded
// up to 128; the diagonal and the padding are 0), on the library's stream
int dist_nld(int n);
void dist_expand(const double *cond, int n, double *D);

}  // namespace sharp
