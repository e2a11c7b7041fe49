// tsne.hip -- exact t-SNE for visualization_SHARP (R/visualization_SHARP.R:94 hands x1 to Rtsne): DESIGN.md §10.
//   before it           input preparation (prepare.hip); the exact k-NN, the selection from given distances (Rtsne(is_distance = TRUE))
//                       and the check of given neighbours (Rtsne_neighbors): knn.hip
//   calibration         one wave per row, fp64 bisection on beta (bhtsne's rule)
//   symmetrisation      COO (i, j, p) + (j, i, p), radix sort by (row, col), duplicates merged, normalised by a fixed-order sum -> CSR
//   optimiser loop      attraction over the CSR rows (fp64); exact repulsion, a workgroup owning 256 rows and streaming every y_j through
//                       LDS (fp32 pair terms, fp64 per-tile folds, launches cut so that none exceeds ~1e11 pairs); one update kernel
//                       (gains, velocity, position), mean subtraction, KL every 50 iterations
// No floating-point atomics anywhere; every reduction runs in an order fixed by n alone, so a call is bitwise reproducible.
#include "tsne.hpp"
#include "graph_prim.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

#include "knn.hpp"
#include "prepare.hpp"
#include "rrng.hpp"

namespace sharp {
namespace {

__global__ __launch_bounds__(256) void dup_flag_kernel(const double *__restrict__ dist, long long n, int K, int *__restrict__ flag) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && dist[i * K] == 0.0) *flag = 1;   // every writer stores the same value
}

// ---------------------------------------------------------------------------------------------------------------------------
// perplexity calibration: one wave per row, fp64 (bhtsne's bisection: beta from 1, doubling / halving while a bound is open, tol 1e-5
// on the entropy in nats, at most 200 steps)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void calib_kernel(const double *__restrict__ dist, long long n, int K, double logU, double *__restrict__ P) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double dv[4], pv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int p = lane + 64 * t; dv[t] = p < K ? dist[i * K + p] : 0.0; pv[t] = 0.0; }
    double beta = 1.0, minb = -DBL_MAX, maxb = DBL_MAX, sumP = DBL_MIN;
    for (int it = 0; it < 200; ++it) {
        double s = 0.0, h = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pv[t] = lane + 64 * t < K ? exp(-beta * dv[t]) : 0.0;
            s += pv[t];
            h += beta * (dv[t] * pv[t]);
        }
        s = wave_sum(s);
        h = wave_sum(h);
        sumP = DBL_MIN + s;
        const double Hdiff = (h / sumP + log(sumP)) - logU;
        if (Hdiff < 1e-5 && -Hdiff < 1e-5) break;
        if (Hdiff > 0) {
            minb = beta;
            beta = (maxb == DBL_MAX || maxb == -DBL_MAX) ? beta * 2.0 : (beta + maxb) / 2.0;
        } else {
            maxb = beta;
            beta = (minb == -DBL_MAX || minb == DBL_MAX) ? beta / 2.0 : (beta + minb) / 2.0;
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = lane + 64 * t;
        if (p < K) P[i * K + p] = pv[t] / sumP;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// symmetrisation
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coo_kernel(const int *__restrict__ idx, const double *__restrict__ Pc, long long n, int K,
                                                  unsigned long long *__restrict__ keys, double *__restrict__ vals) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * K) return;
    const unsigned long long i = static_cast<unsigned long long>(e / K), j = static_cast<unsigned long long>(idx[e]);
    const double p = Pc[e];
    keys[2 * e] = i * static_cast<unsigned long long>(n) + j;
    vals[2 * e] = p;
    keys[2 * e + 1] = j * static_cast<unsigned long long>(n) + i;
    vals[2 * e + 1] = p;
}

__global__ __launch_bounds__(256) void scale_kernel(double *__restrict__ v, long long n, double f, int divide) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < n) v[e] = divide ? v[e] / f : v[e] * f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// gradient: attraction (CSR rows, fp64), exact repulsion (fp32 pair terms, fp64 folds), Z
// ---------------------------------------------------------------------------------------------------------------------------
template <int DIMS>
__global__ __launch_bounds__(256) void attr_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                   const double *__restrict__ Y, long long n, double *__restrict__ attr) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double yi[DIMS], acc[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { yi[k] = Y[i * DIMS + k]; acc[k] = 0.0; }
    for (long long e = rp[i]; e < rp[i + 1]; ++e) {
        const long long j = col[e];
        double diff[DIMS], D = 1.0;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) { diff[k] = yi[k] - Y[j * DIMS + k]; D += diff[k] * diff[k]; }
        D = val[e] / D;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) acc[k] += D * diff[k];
    }
#pragma unroll
    for (int k = 0; k < DIMS; ++k) attr[i * DIMS + k] = acc[k];
}

constexpr int RT = 256;                 // rows per workgroup and points per LDS tile of the repulsion
constexpr double kPairsPerLaunch = 1e11;  // ~25 ms at the arithmetic rate: no repulsion launch near 0.1 s at any n

// Workgroup (blockIdx.x, blockIdx.y): rows row0 + 256 blockIdx.x + tid against the columns of chunk blockIdx.y, 256 points per LDS tile.
// Per pair (fp32, explicit fmaf): d = y_i - y_j, q = 1 / (1 + |d|^2), z += q, f += q^2 d.  Each tile's fp32 partials are folded into
// fp64; the self pair (q = 1, d = 0) is taken out of z in fp64.  part[(chunk * rows + r) * 4 + k]: f_k (k < DIMS), z (k = DIMS).
template <int DIMS>
__global__ __launch_bounds__(256) void rep_kernel(const float *__restrict__ Yf, long long n, long long row0, long long rows, long long cj,
                                                  double *__restrict__ part) {
    __shared__ float ys[RT * DIMS];
    const int tid = threadIdx.x;
    const long long r = static_cast<long long>(blockIdx.x) * RT + tid, i = row0 + r;
    const bool active = r < rows && i < n;
    float yi[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) yi[k] = active ? Yf[i * DIMS + k] : 0.0f;
    double F[DIMS + 1];
#pragma unroll
    for (int k = 0; k <= DIMS; ++k) F[k] = 0.0;
    const long long jb = static_cast<long long>(blockIdx.y) * cj, je = jb + cj < n ? jb + cj : n;
    for (long long t0 = jb; t0 < je; t0 += RT) {
        const int cnt = static_cast<int>(je - t0 < RT ? je - t0 : RT);
        __syncthreads();
        for (int e = tid; e < cnt * DIMS; e += RT) ys[e] = Yf[t0 * DIMS + e];
        __syncthreads();
        float f[DIMS], z = 0.0f;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) f[k] = 0.0f;
#pragma unroll 8
        for (int jj = 0; jj < cnt; ++jj) {
            float dv[DIMS], d2 = 0.0f;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) { dv[k] = yi[k] - ys[jj * DIMS + k]; d2 = fmaf(dv[k], dv[k], d2); }
            const float q = __builtin_amdgcn_rcpf(1.0f + d2);
            z += q;
            const float q2 = q * q;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) f[k] = fmaf(q2, dv[k], f[k]);
        }
#pragma unroll
        for (int k = 0; k < DIMS; ++k) F[k] += static_cast<double>(f[k]);
        F[DIMS] += static_cast<double>(z);
        if (i >= t0 && i < t0 + cnt) F[DIMS] -= 1.0;
    }
    if (r < rows) {
#pragma unroll
        for (int k = 0; k <= DIMS; ++k) part[(static_cast<long long>(blockIdx.y) * rows + r) * 4 + k] = F[k];
    }
}

template <int DIMS>
__global__ __launch_bounds__(256) void fold_kernel(const double *__restrict__ part, int nc, long long row0, long long rows, long long n,
                                                   double *__restrict__ rep, double *__restrict__ zrow) {
    const long long r = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x, i = row0 + r;
    if (r >= rows || i >= n) return;
    double F[DIMS + 1];
#pragma unroll
    for (int k = 0; k <= DIMS; ++k) F[k] = 0.0;
    for (int c = 0; c < nc; ++c)
#pragma unroll
        for (int k = 0; k <= DIMS; ++k) F[k] += part[(static_cast<long long>(c) * rows + r) * 4 + k];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) rep[i * DIMS + k] = F[k];
    zrow[i] = F[DIMS];
}

template <int DIMS>
__global__ __launch_bounds__(256) void grad_kernel(const double *__restrict__ attr, const double *__restrict__ rep, const double *__restrict__ Z,
                                                   long long ne, double *__restrict__ dY) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e < ne) dY[e] = attr[e] - rep[e] / Z[0];
}

__device__ __forceinline__ double sgn(double x) { return x == 0.0 ? 0.0 : (x < 0.0 ? -1.0 : 1.0); }

// gains, velocity and position of one coordinate
__global__ __launch_bounds__(256) void update_kernel(const double *__restrict__ attr, const double *__restrict__ rep, const double *__restrict__ Z,
                                                     long long ne, double momentum, double eta, double *__restrict__ gains,
                                                     double *__restrict__ uY, double *__restrict__ Y) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= ne) return;
    const double dY = attr[e] - rep[e] / Z[0];
    double g = gains[e];
    const double u = uY[e];
    g = sgn(dY) != sgn(u) ? g + 0.2 : g * 0.8;
    if (g < 0.01) g = 0.01;
    gains[e] = g;
    const double un = momentum * u - eta * g * dY;
    uY[e] = un;
    Y[e] = Y[e] + un;
}

// Y -= mean (when mean), and the fp32 copy the repulsion reads
template <int DIMS>
__global__ __launch_bounds__(256) void center_kernel(double *__restrict__ Y, long long n, const double *__restrict__ mean, float *__restrict__ Yf) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * DIMS) return;
    double v = Y[e];
    if (mean) { v = v - mean[e % DIMS]; Y[e] = v; }
    Yf[e] = static_cast<float>(v);
}

// per-row KL: sum_j P_ij log((P_ij + FLT_MIN) / (q_ij / Z + FLT_MIN))
template <int DIMS>
__global__ __launch_bounds__(256) void kl_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                 const double *__restrict__ Y, long long n, const double *__restrict__ Z, double *__restrict__ kl) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    double yi[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) yi[k] = Y[i * DIMS + k];
    const double z = Z[0];
    double c = 0.0;
    for (long long e = rp[i]; e < rp[i + 1]; ++e) {
        const long long j = col[e];
        double D = 1.0;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) { const double t = yi[k] - Y[j * DIMS + k]; D += t * t; }
        const double Q = (1.0 / D) / z;
        c += val[e] * log((val[e] + FLT_MIN) / (Q + FLT_MIN));
    }
    kl[i] = c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Barnes-Hut repulsion (DESIGN.md §10 "Barnes-Hut"): bhtsne's SPTree as a compressed 2^DIMS-ary tree over quantised Morton keys,
// rebuilt from the fp64 Y at every gradient evaluation and laid out in preorder with a skip index per node, so that one lane per point
// walks it without a stack.  fp64 throughout; every sum in an order fixed by n and the keys; no atomics, no inter-workgroup flags.
// ---------------------------------------------------------------------------------------------------------------------------
template <int DIMS> struct BhBits { static constexpr int value = DIMS == 1 ? 63 : (DIMS == 2 ? 32 : 21); };   // levels below the root
constexpr int kBhSlabs = 256;        // slabs of the bounding-box reduction
constexpr int kBhRadix = 32;         // chunk length of the layered sums behind the centres of mass
constexpr int kBhMaxLayers = 8;      // 32^7 > 2^31 rows
constexpr unsigned kBhInternal = 0xFFFFFFFFu;   // meta.z of an internal node (a leaf holds its lowest point index there)

// layer 0: the sorted Y (n x DIMS); layer l + 1: sums of kBhRadix consecutive entries of layer l, in order
struct BhLayers {
    const double *p[kBhMaxLayers];
    long long len[kBhMaxLayers];
    int nl;
};

// slab b: per-dimension sum, min and max of Y's rows [b rps, (b + 1) rps) -> part[b * 3 DIMS + {k, DIMS + k, 2 DIMS + k}]
template <int DIMS>
__global__ __launch_bounds__(256) void bh_bounds_kernel(const double *__restrict__ Y, long long n, long long rps, double *__restrict__ part) {
    __shared__ double s[3 * DIMS][256];
    const int tid = threadIdx.x;
    const long long r0 = static_cast<long long>(blockIdx.x) * rps, r1 = r0 + rps < n ? r0 + rps : n;
    double a[3 * DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { a[k] = 0.0; a[DIMS + k] = DBL_MAX; a[2 * DIMS + k] = -DBL_MAX; }
    for (long long r = r0 + tid; r < r1; r += 256)
#pragma unroll
        for (int k = 0; k < DIMS; ++k) {
            const double v = Y[r * DIMS + k];
            a[k] += v;
            a[DIMS + k] = fmin(a[DIMS + k], v);
            a[2 * DIMS + k] = fmax(a[2 * DIMS + k], v);
        }
#pragma unroll
    for (int k = 0; k < 3 * DIMS; ++k) s[k][tid] = a[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int k = 0; k < DIMS; ++k) {
                s[k][tid] += s[k][tid + w];
                s[DIMS + k][tid] = fmin(s[DIMS + k][tid], s[DIMS + k][tid + w]);
                s[2 * DIMS + k][tid] = fmax(s[2 * DIMS + k][tid], s[2 * DIMS + k][tid + w]);
            }
        __syncthreads();
    }
    if (tid < 3 * DIMS) part[static_cast<long long>(blockIdx.x) * 3 * DIMS + tid] = s[tid][0];
}

// the root cell (bhtsne's SPTree constructor): centre = mean, half-width w_d = max(max - mean, mean - min) + 1e-5.
// root[3 + k] = mean - w (the lower corner), root[6 + k] = 2^bits / (2 w) (finest cells per unit), root[9] = max_d w_d
template <int DIMS>
__global__ void bh_root_kernel(const double *__restrict__ part, int nslab, long long n, double *__restrict__ root) {
    if (threadIdx.x != 0) return;
    double wmax = 0.0;
    for (int k = 0; k < DIMS; ++k) {
        double sum = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
        for (int b = 0; b < nslab; ++b) {
            sum += part[b * 3 * DIMS + k];
            mn = fmin(mn, part[b * 3 * DIMS + DIMS + k]);
            mx = fmax(mx, part[b * 3 * DIMS + 2 * DIMS + k]);
        }
        const double mean = sum / static_cast<double>(n);
        const double w = fmax(mx - mean, mean - mn) + 1e-5;
        root[k] = mean;
        root[3 + k] = mean - w;
        root[6 + k] = ldexp(1.0, BhBits<DIMS>::value) / (2.0 * w);
        wmax = fmax(wmax, w);
    }
    root[9] = wmax;
}

// key[i]: the finest cell of y_i as a Morton key.  Per dimension c = floor((y - lower corner) * cells per unit), clamped to the grid
// (a point on a midline goes to the upper half), then inverted so that the upper half sorts first: digit L (from the top) holds bit
// (bits - L) of every dimension, dimension k at bit k -- bhtsne's child number, so ascending keys visit children in bhtsne's order.
template <int DIMS>
__global__ __launch_bounds__(256) void bh_key_kernel(const double *__restrict__ Y, long long n, const double *__restrict__ root,
                                                     unsigned long long *__restrict__ key) {
    constexpr int bits = BhBits<DIMS>::value;
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double lim = ldexp(1.0, bits);
    const unsigned long long top = (1ull << bits) - 1ull;
    unsigned long long c[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) {
        const double t = (Y[i * DIMS + k] - root[3 + k]) * root[6 + k];
        const unsigned long long u = t >= lim ? top : (t >= 0.0 ? static_cast<unsigned long long>(t) : 0ull);   // (NaN: 0)
        c[k] = top - u;
    }
    unsigned long long K = 0;
    for (int b = bits - 1; b >= 0; --b)
#pragma unroll
        for (int k = 0; k < DIMS; ++k) K |= ((c[k] >> b) & 1ull) << (b * DIMS + k);
    key[i] = K;
}

template <int DIMS>
__global__ __launch_bounds__(256) void bh_gather_kernel(const double *__restrict__ Y, const int *__restrict__ perm, long long n, double *__restrict__ Ys) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * DIMS) return;
    const long long s = e / DIMS;
    Ys[e] = Y[static_cast<long long>(perm[s]) * DIMS + (e - s * DIMS)];
}

template <int DIMS>
__global__ __launch_bounds__(256) void bh_layer_kernel(const double *__restrict__ in, long long len_in, double *__restrict__ out, long long len_out) {
    const long long c = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (c >= len_out) return;
    const long long t0 = c * kBhRadix, t1 = t0 + kBhRadix < len_in ? t0 + kBhRadix : len_in;
    double a[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) a[k] = 0.0;
    for (long long t = t0; t < t1; ++t)
#pragma unroll
        for (int k = 0; k < DIMS; ++k) a[k] += in[t * DIMS + k];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) out[c * DIMS + k] = a[k];
}

// sum of sorted rows [a, b) from the layers: the partial chunks at each end of a layer, then the whole chunks one layer up
template <int DIMS>
__device__ void bh_range_sum(const BhLayers &Ls, long long a, long long b, double *acc) {
    for (int l = 0;; ++l) {
        const double *p = Ls.p[l];
        const long long au = (a + kBhRadix - 1) / kBhRadix * kBhRadix, bd = b / kBhRadix * kBhRadix;
        if (l + 1 >= Ls.nl || au >= bd) {
            for (long long t = a; t < b; ++t)
#pragma unroll
                for (int k = 0; k < DIMS; ++k) acc[k] += p[t * DIMS + k];
            return;
        }
        for (long long t = a; t < au; ++t)
#pragma unroll
            for (int k = 0; k < DIMS; ++k) acc[k] += p[t * DIMS + k];
        for (long long t = bd; t < b; ++t)
#pragma unroll
            for (int k = 0; k < DIMS; ++k) acc[k] += p[t * DIMS + k];
        a = au / kBhRadix;
        b = bd / kBhRadix;
    }
}

// leading digits two keys share (bits when they are equal)
template <int DIMS>
__device__ __forceinline__ int bh_lcp(unsigned long long a, unsigned long long b) {
    if (a == b) return BhBits<DIMS>::value;
    return BhBits<DIMS>::value - 1 - (63 - __builtin_clzll(a ^ b)) / DIMS;
}

// the first sorted position after s outside the level-L cell of key[s]: galloping, then bisection
template <int DIMS>
__device__ long long bh_cell_end(const unsigned long long *__restrict__ key, long long n, long long s, int L) {
    if (L == 0) return n;
    const unsigned long long v = key[s] | ((1ull << ((BhBits<DIMS>::value - L) * DIMS)) - 1ull);
    long long a = s, b, step = 1;   // key[a] <= v; key[b] > v or b == n
    for (;;) {
        b = a + step;
        if (b >= n) { b = n; break; }
        if (key[b] > v) break;
        a = b;
        step *= 2;
    }
    while (b - a > 1) {
        const long long m = a + (b - a) / 2;
        if (key[m] <= v) a = m; else b = m;
    }
    return b;
}

// The nodes of the compressed tree that start at the sorted position s of a run of equal keys: f(level, end) for each internal node,
// outermost first (a chain of cells with one non-empty child is one node, at the level of its deepest cell), then f(bits, end) for the
// leaf, the run itself.  Cells at levels <= lcp(key[s - 1], key[s]) start before s.
template <int DIMS, class F>
__device__ void bh_chain(const unsigned long long *__restrict__ key, long long n, long long s, F f) {
    constexpr int bits = BhBits<DIMS>::value;
    int L = s == 0 ? 0 : bh_lcp<DIMS>(key[s - 1], key[s]) + 1;
    while (L < bits) {
        const long long e = bh_cell_end<DIMS>(key, n, s, L);
        const int g = bh_lcp<DIMS>(key[s], key[e - 1]);   // the deepest level of the chain: its cells all hold [s, e)
        if (g >= bits) break;
        f(g, e);
        L = g + 1;
    }
    f(bits, bh_cell_end<DIMS>(key, n, s, bits));
}

__device__ __forceinline__ bool bh_run_start(const unsigned long long *__restrict__ key, long long s) { return s == 0 || key[s] != key[s - 1]; }

// cnt[s]: nodes that start at sorted position s (0 unless s starts a run; cnt[n] = 0)
template <int DIMS>
__global__ __launch_bounds__(256) void bh_count_kernel(const unsigned long long *__restrict__ key, long long n, unsigned *__restrict__ cnt) {
    const long long s = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s > n) return;
    unsigned c = 0;
    if (s < n && bh_run_start(key, s)) bh_chain<DIMS>(key, n, s, [&](int, long long) { ++c; });
    cnt[s] = c;
}

// The nodes in preorder: those starting at s go to off[s], off[s] + 1, ... (off: exclusive scan of cnt, off[n] = node count).  A node
// holding sorted rows [s, e) skips to off[e], the first node that starts at or after e.  meta = (points, skip, lowest point index of a
// leaf or kBhInternal, level); com: the centre of mass (fp64 sum from the layers / count).
template <int DIMS>
__global__ __launch_bounds__(256) void bh_node_kernel(const unsigned long long *__restrict__ key, const int *__restrict__ perm, long long n,
                                                      const unsigned *__restrict__ off, BhLayers Ls, uint4 *__restrict__ meta,
                                                      double *__restrict__ com) {
    const long long s = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= n || !bh_run_start(key, s)) return;
    unsigned o = off[s];
    bh_chain<DIMS>(key, n, s, [&](int level, long long e) {
        const bool leaf = level == BhBits<DIMS>::value;
        meta[o] = make_uint4(static_cast<unsigned>(e - s), off[e], leaf ? static_cast<unsigned>(perm[s]) : kBhInternal, static_cast<unsigned>(level));
        double acc[DIMS];
#pragma unroll
        for (int k = 0; k < DIMS; ++k) acc[k] = 0.0;
        bh_range_sum<DIMS>(Ls, s, e, acc);
#pragma unroll
        for (int k = 0; k < DIMS; ++k) com[static_cast<size_t>(o) * DIMS + k] = acc[k] / static_cast<double>(e - s);
        ++o;
    });
}

// One lane per point, lanes in sorted-key order: bhtsne's computeNonEdgeForces over the preorder layout.  A leaf whose lowest index is
// i is skipped; a leaf, or an internal node with max_d(half-width) / sqrt(D) < theta, is a summary (cnt q to z, cnt q^2 (y_i - com) to
// the repulsion; k = skip); otherwise the walk enters its first child (k + 1).  rep / zrow as rep_kernel + fold_kernel leave them.
template <int DIMS>
__global__ __launch_bounds__(256) void bh_walk_kernel(const double *__restrict__ Ys, const int *__restrict__ perm, long long n,
                                                      const uint4 *__restrict__ meta, const double *__restrict__ com,
                                                      const double *__restrict__ root, double theta, double *__restrict__ rep,
                                                      double *__restrict__ zrow) {
    const long long s = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= n) return;
    const unsigned i = static_cast<unsigned>(perm[s]);
    double yi[DIMS], f[DIMS], z = 0.0;
#pragma unroll
    for (int k = 0; k < DIMS; ++k) { yi[k] = Ys[s * DIMS + k]; f[k] = 0.0; }
    const double wmax = root[9];
    const unsigned M = meta[0].y;   // the root's skip: the node count
    unsigned k = 0;
    while (k < M) {
        const uint4 m = meta[k];
        if (m.z == i) { k = m.y; continue; }
        double d[DIMS], D = 0.0;
#pragma unroll
        for (int c = 0; c < DIMS; ++c) { d[c] = yi[c] - com[static_cast<size_t>(k) * DIMS + c]; D += d[c] * d[c]; }
        if (m.z != kBhInternal || ldexp(wmax, -static_cast<int>(m.w)) / sqrt(D) < theta) {
            const double q = 1.0 / (1.0 + D);
            double mult = static_cast<double>(m.x) * q;
            z += mult;
            mult *= q;
#pragma unroll
            for (int c = 0; c < DIMS; ++c) f[c] += mult * d[c];
            k = m.y;
        } else {
            ++k;
        }
    }
#pragma unroll
    for (int c = 0; c < DIMS; ++c) rep[static_cast<long long>(i) * DIMS + c] = f[c];
    zrow[i] = z;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------------------------------------
struct RepPlan {
    long long rows = 0, cj = 0;   // rows per launch, columns per chunk
    int nc = 1;                   // chunks
};

RepPlan rep_plan(long long n) {
    RepPlan p;
    const long long n_up = (n + RT - 1) / RT * RT;
    long long rows = static_cast<long long>(kPairsPerLaunch / static_cast<double>(std::max<long long>(n, 1))) / RT * RT;
    p.rows = std::min(n_up, std::max<long long>(RT, rows));
    const long long rb = (p.rows + RT - 1) / RT;
    long long nc = std::max<long long>(1, std::min<long long>((n + RT - 1) / RT, (2048 + rb - 1) / rb));   // >= ~2048 workgroups per launch
    p.cj = ((n + nc - 1) / nc + RT - 1) / RT * RT;
    p.nc = static_cast<int>((n + p.cj - 1) / p.cj);
    return p;
}

// the Barnes-Hut tree's buffers, allocated once per call (at most 2n - 1 nodes)
struct BhTree {
    DevBuf<unsigned long long> key, key_s;
    DevBuf<int> iota, perm;
    DevBuf<double> Ys, lay, part, root, com;
    DevBuf<unsigned> cnt, off;
    DevBuf<uint4> meta;
    Scratch sort_tmp, scan_tmp;   // (sized by the first build, reused by every later one: the counts do not change)
    BhLayers L{};
    int nslab = 1, end_bit = 64;
    long long rps = 1;
    void init(long long n, int dims) {
        const size_t nn = static_cast<size_t>(n);
        key.alloc(nn); key_s.alloc(nn); iota.alloc(nn); perm.alloc(nn);
        Ys.alloc(nn * dims);
        cnt.alloc(nn + 1); off.alloc(nn + 1);
        meta.alloc(2 * nn); com.alloc(2 * nn * dims);
        root.alloc(16);
        nslab = static_cast<int>(std::min<long long>(kBhSlabs, std::max<long long>(1, n / 256)));
        rps = (n + nslab - 1) / nslab;
        nslab = static_cast<int>((n + rps - 1) / rps);
        part.alloc(static_cast<size_t>(nslab) * 3 * dims);
        std::vector<long long> len{n}, at{0};
        long long total = 0;
        while (len.back() > kBhRadix) {
            at.push_back(total);
            len.push_back((len.back() + kBhRadix - 1) / kBhRadix);
            total += len.back();
        }
        SHARP_REQUIRE(len.size() <= static_cast<size_t>(kBhMaxLayers), "tsne_bh: too many rows");
        lay.alloc(std::max<size_t>(1, static_cast<size_t>(total) * dims));
        L.nl = static_cast<int>(len.size());
        for (int l = 0; l < L.nl; ++l) {
            L.len[l] = len[l];
            L.p[l] = l == 0 ? Ys.p : lay.p + at[l] * dims;
        }
        end_bit = dims == 1 ? 63 : (dims == 2 ? 64 : 63);
        sharp::iota(iota.p, n);
    }
};

struct Work {
    long long n = 0;
    int dims = 2;
    RepPlan plan;
    DevBuf<double> Y, uY, gains, attr, rep, zrow, kl, part, red, scal, colpart;   // scal: [0] Z, [1] KL sum, [2..] mean
    DevBuf<float> Yf;
    double theta = 0.0;   // > 0: the Barnes-Hut repulsion with this theta instead of the exact one
    BhTree bh;
    void init(long long n_, int dims_, double theta_ = 0.0) {
        n = n_;
        dims = dims_;
        theta = theta_;
        plan = rep_plan(n);
        const size_t ne = static_cast<size_t>(n) * dims;
        Y.alloc(ne); uY.alloc(ne); gains.alloc(ne); attr.alloc(ne); rep.alloc(ne); Yf.alloc(ne);
        zrow.alloc(n); kl.alloc(n);
        if (theta > 0.0) bh.init(n, dims);
        else part.alloc(static_cast<size_t>(plan.nc) * plan.rows * 4);
        red.alloc(kRedBlocks);
        scal.alloc(8);
    }
};

// the tree at the current Y (DESIGN.md §10 "Barnes-Hut"): bounding box and mean, keys, stable sort, sorted Y and its layered sums,
// node counts per run start, their scan, the nodes
template <int DIMS>
void bh_build(Work &w) {
    Ctx &c = ctx();
    BhTree &t = w.bh;
    const long long n = w.n;
    KernelTimer tm("tsne_bh_tree");
    hipLaunchKernelGGL(bh_bounds_kernel<DIMS>, dim3(t.nslab), dim3(256), 0, c.stream, w.Y.p, n, t.rps, t.part.p);
    hipLaunchKernelGGL(bh_root_kernel<DIMS>, dim3(1), dim3(64), 0, c.stream, t.part.p, t.nslab, n, t.root.p);
    hipLaunchKernelGGL(bh_key_kernel<DIMS>, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, w.Y.p, n, t.root.p, t.key.p);
    launch_check("bh_key_kernel");
    sort_pairs(t.key.p, t.key_s.p, t.iota.p, t.perm.p, static_cast<size_t>(n), 0, t.end_bit, t.sort_tmp, t.sort_tmp.n > 0);
    hipLaunchKernelGGL(bh_gather_kernel<DIMS>, dim3(grid_for(n * DIMS, 256)), dim3(256), 0, c.stream, w.Y.p, t.perm.p, n, t.Ys.p);
    for (int l = 1; l < t.L.nl; ++l)
        hipLaunchKernelGGL(bh_layer_kernel<DIMS>, dim3(grid_for(t.L.len[l], 256)), dim3(256), 0, c.stream, t.L.p[l - 1], t.L.len[l - 1],
                           const_cast<double *>(t.L.p[l]), t.L.len[l]);
    hipLaunchKernelGGL(bh_count_kernel<DIMS>, dim3(grid_for(n + 1, 256)), dim3(256), 0, c.stream, t.key_s.p, n, t.cnt.p);
    launch_check("bh_count_kernel");
    exclusive_scan(t.cnt.p, t.off.p, static_cast<size_t>(n) + 1, t.scan_tmp, t.scan_tmp.n > 0);
    hipLaunchKernelGGL(bh_node_kernel<DIMS>, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, t.key_s.p, t.perm.p, n, t.off.p, t.L, t.meta.p,
                       t.com.p);
    launch_check("bh_node_kernel");
}

template <int DIMS>
void to_f32(Work &w, bool center) {
    if (center) column_stat(w.Y.p, w.n, DIMS, DIMS, nullptr, static_cast<double>(w.n), w.colpart, w.scal.p + 2);
    hipLaunchKernelGGL(center_kernel<DIMS>, dim3(grid_for(w.n * DIMS, 256)), dim3(256), 0, ctx().stream, w.Y.p, w.n, center ? w.scal.p + 2 : nullptr, w.Yf.p);
    launch_check("center_kernel");
}

// attr, rep, zrow and Z (scal[0]) at the current Y / Yf
template <int DIMS>
void gradient_terms(const TsneP &P, Work &w) {
    Ctx &c = ctx();
    {
        KernelTimer t("tsne_attr");
        hipLaunchKernelGGL(attr_kernel<DIMS>, dim3(grid_for(w.n, 256)), dim3(256), 0, c.stream, P.row_ptr.p, P.col.p, P.val.p, w.Y.p, w.n, w.attr.p);
        launch_check("attr_kernel");
    }
    if (w.theta > 0.0) {
        bh_build<DIMS>(w);
        KernelTimer t("tsne_bh_walk");
        hipLaunchKernelGGL(bh_walk_kernel<DIMS>, dim3(grid_for(w.n, 256)), dim3(256), 0, c.stream, w.bh.Ys.p, w.bh.perm.p, w.n, w.bh.meta.p,
                           w.bh.com.p, w.bh.root.p, w.theta, w.rep.p, w.zrow.p);
        launch_check("bh_walk_kernel");
        fixed_reduce(Fold::Sum, w.zrow.p, w.n, w.red.p, w.scal.p);
        return;
    }
    KernelTimer t("tsne_rep");
    for (long long r0 = 0; r0 < w.n; r0 += w.plan.rows) {
        hipLaunchKernelGGL(rep_kernel<DIMS>, dim3(grid_for(w.plan.rows, RT), w.plan.nc), dim3(RT), 0, c.stream, w.Yf.p, w.n, r0, w.plan.rows, w.plan.cj,
                           w.part.p);
        hipLaunchKernelGGL(fold_kernel<DIMS>, dim3(grid_for(w.plan.rows, 256)), dim3(256), 0, c.stream, w.part.p, w.plan.nc, r0, w.plan.rows, w.n,
                           w.rep.p, w.zrow.p);
        launch_check("rep_kernel");
    }
    fixed_reduce(Fold::Sum, w.zrow.p, w.n, w.red.p, w.scal.p);
}

template <int DIMS>
void kl_eval(const TsneP &P, Work &w, double *dst) {
    KernelTimer t("tsne_kl");
    hipLaunchKernelGGL(kl_kernel<DIMS>, dim3(grid_for(w.n, 256)), dim3(256), 0, ctx().stream, P.row_ptr.p, P.col.p, P.val.p, w.Y.p, w.n, w.scal.p, w.kl.p);
    launch_check("kl_kernel");
    fixed_reduce(Fold::Sum, w.kl.p, w.n, w.red.p, dst);
}

struct LoopArgs {
    int max_iter, stop_lying_iter, mom_switch_iter;
    double momentum, final_momentum, eta, exaggeration;
};

template <int DIMS>
void optimise(TsneP &P, Work &w, const LoopArgs &a, std::vector<double> &itercosts, double *costs) {
    Ctx &c = ctx();
    const long long ne = w.n * DIMS;
    const bool lying = a.stop_lying_iter > 0;
    if (lying) hipLaunchKernelGGL(scale_kernel, dim3(grid_for(P.nnz, 256)), dim3(256), 0, c.stream, P.val.p, P.nnz, a.exaggeration, 0);
    SHARP_HIP_CHECK(hipMemsetAsync(w.uY.p, 0, ne * sizeof(double), c.stream));
    std::vector<double> ones(static_cast<size_t>(ne), 1.0);
    w.gains.upload(ones.data(), ones.size());
    to_f32<DIMS>(w, false);
    std::vector<int> record;   // iterations whose KL is recorded
    for (int it = 0; it < a.max_iter; ++it)
        if ((it > 0 && it % 50 == 0) || it == a.max_iter - 1) record.push_back(it);
    DevBuf<double> dcost(std::max<size_t>(1, record.size()));
    size_t next_cost = 0;
    bool pending = false;     // the KL of the previous iteration's positions is due: it is evaluated with this iteration's Z
    double momentum = a.momentum;
    for (int it = 0; it < a.max_iter; ++it) {
        gradient_terms<DIMS>(P, w);
        if (pending) { kl_eval<DIMS>(P, w, dcost.p + next_cost++); pending = false; }
        {
            KernelTimer t("tsne_update");
            hipLaunchKernelGGL(update_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c.stream, w.attr.p, w.rep.p, w.scal.p, ne, momentum, a.eta,
                               w.gains.p, w.uY.p, w.Y.p);
            launch_check("update_kernel");
            to_f32<DIMS>(w, true);
        }
        if (it == a.stop_lying_iter && lying)
            hipLaunchKernelGGL(scale_kernel, dim3(grid_for(P.nnz, 256)), dim3(256), 0, c.stream, P.val.p, P.nnz, a.exaggeration, 1);
        if (it == a.mom_switch_iter) momentum = a.final_momentum;
        if (next_cost < record.size() && record[next_cost] == it) pending = true;
    }
    // the last recorded KL (the last iteration's), or the cost at the start when there are no iterations
    if (pending || costs) {
        gradient_terms<DIMS>(P, w);
        kl_eval<DIMS>(P, w, pending ? dcost.p + next_cost++ : w.scal.p + 1);
    }
    itercosts.assign(record.size(), 0.0);
    if (!record.empty()) dcost.download(itercosts.data(), record.size());
    if (costs) w.kl.download(costs, static_cast<size_t>(w.n));
}

// ---- stage helpers used by the entries -----------------------------------------------------------------------------------
int perplexity_K(double perplexity) {
    SHARP_REQUIRE(std::isfinite(perplexity) && perplexity > 0, "Rtsne: perplexity must be positive");
    SHARP_REQUIRE(perplexity <= 85.0, "Rtsne: perplexity above 85 is not supported (at most 255 neighbours per row)");
    return static_cast<int>(std::floor(3.0 * perplexity));
}

}  // namespace

void tsne_affinities(const DevBuf<int> &idx, const DevBuf<double> &dist, long long n, int K, double perplexity, TsneP &P) {
    Ctx &c = ctx();
    DevBuf<double> Pc(static_cast<size_t>(n) * K);
    {
        KernelTimer t("tsne_calib");
        hipLaunchKernelGGL(calib_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, dist.p, n, K, std::log(perplexity), Pc.p);
        launch_check("calib_kernel");
    }
    KernelTimer t("tsne_sym");
    const size_t ne = static_cast<size_t>(n) * K * 2;
    DevBuf<unsigned long long> keys(ne), keys2(ne);
    DevBuf<double> vals(ne), vals2(ne);
    hipLaunchKernelGGL(coo_kernel, dim3(grid_for(n * K, 256)), dim3(256), 0, c.stream, idx.p, Pc.p, n, K, keys.p, vals.p);
    launch_check("coo_kernel");
    Pc.release();
    // merge the (at most two) entries of a key: p_ij + p_ji
    const u64 un = static_cast<u64>(n);
    MergeScratch tmp;
    const size_t nnz = merge_by_key<double, Plus>(keys.p, vals.p, ne, un * un, keys2.p, vals2.p, keys.p, vals.p, tmp);
    DevBuf<double> red(kRedBlocks), total(1);
    fixed_reduce(Fold::Sum, vals.p, static_cast<long long>(nnz), red.p, total.p);
    P.n = n;
    P.nnz = static_cast<long long>(nnz);
    P.row_ptr.alloc(n + 1);
    P.col.alloc(nnz);
    P.val.alloc(nnz);
    merged_to_csr<double>(keys.p, P.nnz, n, false, P.row_ptr.p, P.col.p, nullptr, vals.p, total.p, P.val.p);   // (no row is empty: K entries each)
    stream_sync();
}

void tsne_gradient(const TsneP &P, const double *dY_in, int dims, double *dGrad, double theta, double *Z) {
    Work w;
    w.init(P.n, dims, theta);
    SHARP_HIP_CHECK(hipMemcpyAsync(w.Y.p, dY_in, static_cast<size_t>(P.n) * dims * sizeof(double), hipMemcpyDeviceToDevice, ctx().stream));
    const long long ne = P.n * dims;
    auto run = [&](auto tag) {
        constexpr int D = decltype(tag)::value;
        to_f32<D>(w, false);
        gradient_terms<D>(P, w);
        hipLaunchKernelGGL(grad_kernel<D>, dim3(grid_for(ne, 256)), dim3(256), 0, ctx().stream, w.attr.p, w.rep.p, w.scal.p, ne, dGrad);
        launch_check("grad_kernel");
    };
    if (dims == 1) run(std::integral_constant<int, 1>());
    else if (dims == 2) run(std::integral_constant<int, 2>());
    else run(std::integral_constant<int, 3>());
    if (Z) SHARP_HIP_CHECK(hipMemcpyAsync(Z, w.scal.p, sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    stream_sync();
}

}  // namespace sharp

using namespace sharp;

namespace {
void check_dims(int dims) { SHARP_REQUIRE(dims >= 1 && dims <= 3, "Rtsne: dims must be 1, 2 or 3"); }
void check_X(const double *X, long long n, int d, long long ld) {
    SHARP_REQUIRE(X && n >= 2 && d >= 1 && ld >= d, "Rtsne: bad input matrix (need n >= 2 rows of d >= 1 values, ld >= d)");
    SHARP_REQUIRE(n < INT_MAX, "Rtsne: at most 2^31 - 1 rows");
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < d; ++c)
            if (!std::isfinite(X[i * ld + c]))
                throw sharp::Error(SHARP_ERR_ARG, "Rtsne: the input holds NA / NaN / Inf (row " + std::to_string(i + 1) + ", column " +
                                                      std::to_string(c + 1) + ")");
}

// Rtsne's searches: a K out of range is refused under the stage's name, everything behind it under Rtsne's
void tsne_knn(const double *dX, long long n, int d, int K, DevBuf<int> &idx, DevBuf<double> &dist) {
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, "tsne_knn: need 1 <= K <= 255 and K < n");
    knn_self("Rtsne", dX, n, d, K, idx, dist);
}
void tsne_knn_dist(const double *d, int n, int K, DevBuf<int> &idx, DevBuf<double> &dist2) {
    SHARP_REQUIRE(K >= 1 && K <= 255 && n - 1 >= K, "tsne_knn_dist: need 1 <= K <= 255 and K < n");
    knn_from_dist("Rtsne", d, n, K, idx, dist2);
}

void check_loop_args(int dims, int max_iter, double momentum, double final_momentum, double eta, double exaggeration, const double *Y) {
    check_dims(dims);
    SHARP_REQUIRE(Y, "sharp_tsne: null Y");
    SHARP_REQUIRE(max_iter >= 0 && std::isfinite(eta) && std::isfinite(momentum) && std::isfinite(final_momentum), "Rtsne: bad optimiser arguments");
    SHARP_REQUIRE(std::isfinite(exaggeration) && exaggeration > 0, "Rtsne: exaggeration_factor must be positive");
}

// Everything behind the k-NN: P from the lists (idx, dist2: device, n x K, squared distances; released once P exists), the start, the
// optimiser loop.  bh_theta > 0 takes the Barnes-Hut repulsion with that theta, 0 the exact one.
void run_from_neighbours(DevBuf<int> &idx, DevBuf<double> &dist, long long n, int K, int dims, double perplexity, double bh_theta,
                         const LoopArgs &la, const double *Y_init, double seed, double *Y, double *itercosts, double *costs) {
    TsneP P;
    tsne_affinities(idx, dist, n, K, perplexity, P);
    idx.release();
    dist.release();
    Work w;
    w.init(n, dims, bh_theta);
    const size_t ne = static_cast<size_t>(n) * dims;
    std::vector<double> y0(ne);
    if (Y_init) {
        for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(std::isfinite(Y_init[e]), "Rtsne: Y_init holds NA / NaN / Inf");
        std::copy(Y_init, Y_init + ne, y0.begin());
    } else {
        // Y = 1e-4 N(0, 1): R's set.seed(seed) stream, one normal per pair of unif_rand() (polar method, the second draw discarded)
        RRng rng(static_cast<uint32_t>(static_cast<int>(seed)));
        for (size_t e = 0; e < ne; ++e) {
            double x, y, rad;
            do {
                x = 2.0 * rng.unif() - 1.0;
                y = 2.0 * rng.unif() - 1.0;
                rad = x * x + y * y;
            } while (rad >= 1.0 || rad == 0.0);
            y0[e] = x * std::sqrt(-2.0 * std::log(rad) / rad) * 1e-4;
        }
    }
    w.Y.upload(y0.data(), ne);
    std::vector<double> ic;
    if (dims == 1) optimise<1>(P, w, la, ic, costs);
    else if (dims == 2) optimise<2>(P, w, la, ic, costs);
    else optimise<3>(P, w, la, ic, costs);
    w.Y.download(Y, ne);
    if (itercosts) std::copy(ic.begin(), ic.end(), itercosts);
}

// Rtsne's body: prepare, exact k-NN, the duplicate check, then run_from_neighbours
void run_tsne(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale,
              int normalize, int check_duplicates, double perplexity, double bh_theta, int max_iter, int stop_lying_iter, int mom_switch_iter,
              double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y,
              double *itercosts, double *costs) {
    check_X(X, n, d, ld);
    check_loop_args(dims, max_iter, momentum, final_momentum, eta, exaggeration, Y);
    const int K = perplexity_K(perplexity);
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
    DevBuf<double> Xp;
    int dp = 0;
    prepare_input("Rtsne", X, n, d, ld, pca != 0, initial_dims, pca_center != 0, pca_scale != 0, normalize != 0, Xp, &dp);
    DevBuf<int> idx;
    DevBuf<double> dist;
    tsne_knn(Xp.p, n, dp, K, idx, dist);
    if (check_duplicates) {
        DevBuf<int> flag(1);
        flag.zero();
        hipLaunchKernelGGL(dup_flag_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx().stream, dist.p, n, K, flag.p);
        int f = 0;
        flag.download(&f, 1);
        SHARP_REQUIRE(f == 0, "Remove duplicates before running TSNE.");
    }
    Xp.release();
    run_from_neighbours(idx, dist, n, K, dims, perplexity, bh_theta,
                        LoopArgs{max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration}, Y_init, seed, Y,
                        itercosts, costs);
}

// Rtsne's own check on theta, as far as it is known here
void check_bh_theta(double theta) { SHARP_REQUIRE(std::isfinite(theta) && theta >= 0.0 && theta <= 1.0, "Incorrect theta."); }
}  // namespace

extern "C" {

// R/visualization_SHARP.R:94: Rtsne(x1, check_duplicates = FALSE, pca = flag, ...), with an exact repulsion (theta accepted, unused)
int sharp_tsne(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale, int normalize,
               int check_duplicates, double perplexity, double theta, int max_iter, int stop_lying_iter, int mom_switch_iter, double momentum,
               double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y, double *itercosts,
               double *costs) {
    SHARP_API_BEGIN
    (void)theta;
    ctx();
    run_tsne(X, n, d, ld, dims, initial_dims, pca, pca_center, pca_scale, normalize, check_duplicates, perplexity, 0.0, max_iter, stop_lying_iter,
             mom_switch_iter, momentum, final_momentum, eta, exaggeration, Y_init, seed, Y, itercosts, costs);
    SHARP_API_END
}

// the same with bhtsne's Barnes-Hut repulsion at theta (0 <= theta <= 1; theta == 0: the exact path above, bit for bit)
int sharp_tsne_bh(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale,
                  int normalize, int check_duplicates, double perplexity, double theta, int max_iter, int stop_lying_iter, int mom_switch_iter,
                  double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y,
                  double *itercosts, double *costs) {
    SHARP_API_BEGIN
    ctx();
    check_bh_theta(theta);
    run_tsne(X, n, d, ld, dims, initial_dims, pca, pca_center, pca_scale, normalize, check_duplicates, perplexity, theta, max_iter, stop_lying_iter,
             mom_switch_iter, momentum, final_momentum, eta, exaggeration, Y_init, seed, Y, itercosts, costs);
    SHARP_API_END
}

int sharp_tsne_prepare(const double *X, long long n, int d, long long ld, int pca, int initial_dims, int pca_center, int pca_scale, int normalize,
                       double *out, int *d_out) {
    SHARP_API_BEGIN
    ctx();
    check_X(X, n, d, ld);
    SHARP_REQUIRE(out && d_out, "sharp_tsne_prepare: null output");
    DevBuf<double> Xp;
    prepare_input("Rtsne", X, n, d, ld, pca != 0, initial_dims, pca_center != 0, pca_scale != 0, normalize != 0, Xp, d_out);
    Xp.download(out, static_cast<size_t>(n) * *d_out);
    SHARP_API_END
}

int sharp_tsne_knn(const double *X, long long n, int d, long long ld, int K, int *idx, double *dist) {
    SHARP_API_BEGIN
    ctx();
    check_X(X, n, d, ld);
    SHARP_REQUIRE(idx && dist, "sharp_tsne_knn: null output");
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_knn(dX.p, n, d, K, di, dd);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist, static_cast<size_t>(n) * K);
    SHARP_API_END
}

int sharp_tsne_affinities(const double *X, long long n, int d, long long ld, double perplexity, long long cap, long long *row_ptr, int *col,
                          double *val, long long *nnz) {
    SHARP_API_BEGIN
    ctx();
    check_X(X, n, d, ld);
    SHARP_REQUIRE(row_ptr && col && val && nnz, "sharp_tsne_affinities: null output");
    const int K = perplexity_K(perplexity);
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
    DevBuf<double> dX;
    upload_rows(X, n, d, ld, dX);
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_knn(dX.p, n, d, K, di, dd);
    TsneP P;
    tsne_affinities(di, dd, n, K, perplexity, P);
    *nnz = P.nnz;
    SHARP_REQUIRE(cap >= P.nnz, "sharp_tsne_affinities: col / val hold fewer than nnz entries (2 n floor(3 perplexity) always suffice)");
    P.row_ptr.download(row_ptr, static_cast<size_t>(n) + 1);
    P.col.download(col, static_cast<size_t>(P.nnz));
    P.val.download(val, static_cast<size_t>(P.nnz));
    SHARP_API_END
}

}  // extern "C"

namespace {
// the arguments every entry on given neighbours checks before it touches the lists
void check_neighbour_args(const int *index, const double *distance, long long n, int K, double perplexity, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(index && distance, w + ": null index / distance");
    SHARP_REQUIRE(n >= 2 && n < INT_MAX, w + ": need 2 <= n < 2^31 rows");
    SHARP_REQUIRE(K >= 1, w + ": need at least one neighbour per row (K >= 1)");
    SHARP_REQUIRE(K <= 255, w + ": at most 255 neighbours per row");
    SHARP_REQUIRE(K <= n - 1, w + ": K neighbours per row need K <= n - 1");
    SHARP_REQUIRE(std::isfinite(perplexity) && perplexity > 0, "Rtsne: perplexity must be positive");
    SHARP_REQUIRE(perplexity <= static_cast<double>(K), w + ": perplexity above K, the entropy of K neighbours cannot reach it");
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
}

// d: R's dist vector, every entry finite and >= 0, checked on the host before the upload
void check_dist_vector(const double *d, int n, const char *who) {
    const std::string w(who);
    SHARP_REQUIRE(n <= SHARP_DIST_MAX_N, w + ": more than 46340 objects (the dist vector would pass 2^30 entries) is not supported");
    SHARP_REQUIRE(n >= 2, w + ": need n >= 2 objects");
    SHARP_REQUIRE(d, w + ": null d");
    const size_t len = static_cast<size_t>(n) * (n - 1) / 2;
    for (size_t e = 0; e < len; ++e)
        SHARP_REQUIRE(d[e] >= 0.0 && d[e] <= DBL_MAX, w + ": d holds NA / NaN / Inf or a negative distance");   // (false for NaN too)
}
}  // namespace

extern "C" {

int sharp_tsne_neighbors(const int *index, const double *distance, long long n, int K, int squared, int repulsion, int dims, double perplexity,
                         double theta, int max_iter, int stop_lying_iter, int mom_switch_iter, double momentum, double final_momentum, double eta,
                         double exaggeration, const double *Y_init, double seed, double *Y, double *itercosts, double *costs) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(repulsion == 0 || repulsion == 1, "sharp_tsne_neighbors: repulsion must be 0 (exact) or 1 (Barnes-Hut)");
    if (repulsion) check_bh_theta(theta);
    check_neighbour_args(index, distance, n, K, perplexity, "sharp_tsne_neighbors");
    check_loop_args(dims, max_iter, momentum, final_momentum, eta, exaggeration, Y);
    DevBuf<int> idx;
    DevBuf<double> dist;
    upload_neighbours("Rtsne_neighbors", index, distance, n, K, squared != 0, idx, dist);
    run_from_neighbours(idx, dist, n, K, dims, perplexity, repulsion ? theta : 0.0,
                        LoopArgs{max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration}, Y_init, seed, Y,
                        itercosts, costs);
    SHARP_API_END
}

int sharp_tsne_dist(const double *d, int n, int repulsion, int dims, double perplexity, double theta, int max_iter, int stop_lying_iter,
                    int mom_switch_iter, double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init,
                    double seed, double *Y, double *itercosts, double *costs) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(n <= SHARP_DIST_MAX_N, "sharp_tsne_dist: more than 46340 objects (the dist vector would pass 2^30 entries) is not supported");
    SHARP_REQUIRE(repulsion == 0 || repulsion == 1, "sharp_tsne_dist: repulsion must be 0 (exact) or 1 (Barnes-Hut)");
    if (repulsion) check_bh_theta(theta);
    check_loop_args(dims, max_iter, momentum, final_momentum, eta, exaggeration, Y);
    const int K = perplexity_K(perplexity);
    SHARP_REQUIRE(static_cast<double>(n - 1) >= 3.0 * perplexity, "Perplexity is too large.");
    check_dist_vector(d, n, "sharp_tsne_dist");
    DevBuf<int> idx;
    DevBuf<double> dist;
    tsne_knn_dist(d, n, K, idx, dist);
    run_from_neighbours(idx, dist, n, K, dims, perplexity, repulsion ? theta : 0.0,
                        LoopArgs{max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration}, Y_init, seed, Y,
                        itercosts, costs);
    SHARP_API_END
}

int sharp_tsne_knn_dist(const double *d, int n, int K, int *idx, double *dist2) {
    SHARP_API_BEGIN
    ctx();
    check_dist_vector(d, n, "sharp_tsne_knn_dist");
    SHARP_REQUIRE(idx && dist2, "sharp_tsne_knn_dist: null output");
    DevBuf<int> di;
    DevBuf<double> dd;
    tsne_knn_dist(d, n, K, di, dd);
    di.download(idx, static_cast<size_t>(n) * K);
    dd.download(dist2, static_cast<size_t>(n) * K);
    SHARP_API_END
}

int sharp_tsne_affinities_nn(const int *index, const double *distance, long long n, int K, int squared, double perplexity, long long cap,
                             long long *row_ptr, int *col, double *val, long long *nnz) {
    SHARP_API_BEGIN
    ctx();
    check_neighbour_args(index, distance, n, K, perplexity, "sharp_tsne_affinities_nn");
    SHARP_REQUIRE(row_ptr && col && val && nnz, "sharp_tsne_affinities_nn: null output");
    DevBuf<int> di;
    DevBuf<double> dd;
    upload_neighbours("Rtsne_neighbors", index, distance, n, K, squared != 0, di, dd);
    TsneP P;
    tsne_affinities(di, dd, n, K, perplexity, P);
    *nnz = P.nnz;
    SHARP_REQUIRE(cap >= P.nnz, "sharp_tsne_affinities_nn: col / val hold fewer than nnz entries (2 n K always suffice)");
    P.row_ptr.download(row_ptr, static_cast<size_t>(n) + 1);
    P.col.download(col, static_cast<size_t>(P.nnz));
    P.val.download(val, static_cast<size_t>(P.nnz));
    SHARP_API_END
}

}  // extern "C"

namespace {
void gradient_entry(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double theta, double *dY,
                    double *Z) {
    check_dims(dims);
    SHARP_REQUIRE(row_ptr && col && val && Y && dY && n >= 2, "sharp_tsne_gradient: null argument");
    TsneP P;
    P.n = n;
    SHARP_REQUIRE(row_ptr[0] == 0 && row_ptr[n] >= 0, "sharp_tsne_gradient: row_ptr must run from 0 to nnz");
    P.nnz = row_ptr[n];
    P.row_ptr.alloc(n + 1);
    P.row_ptr.upload(row_ptr, n + 1);
    P.col.alloc(std::max<long long>(P.nnz, 1));
    P.val.alloc(std::max<long long>(P.nnz, 1));
    if (P.nnz) { P.col.upload(col, P.nnz); P.val.upload(val, P.nnz); }
    const size_t ne = static_cast<size_t>(n) * dims;
    for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(std::isfinite(Y[e]), "sharp_tsne_gradient: Y holds NA / NaN / Inf");
    for (long long i = 0; i < n; ++i) SHARP_REQUIRE(row_ptr[i] <= row_ptr[i + 1], "sharp_tsne_gradient: row_ptr is not monotone");
    for (long long e = 0; e < P.nnz; ++e) SHARP_REQUIRE(col[e] >= 0 && col[e] < n, "sharp_tsne_gradient: a column index out of range");
    DevBuf<double> dYin(ne), dG(ne);
    dYin.upload(Y, ne);
    tsne_gradient(P, dYin.p, dims, dG.p, theta, Z);
    dG.download(dY, ne);
}
}  // namespace

extern "C" {

int sharp_tsne_gradient(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double *dY) {
    SHARP_API_BEGIN
    ctx();
    gradient_entry(row_ptr, col, val, n, dims, Y, 0.0, dY, nullptr);
    SHARP_API_END
}

int sharp_tsne_gradient_bh(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double theta,
                           double *dY, double *Z) {
    SHARP_API_BEGIN
    ctx();
    check_bh_theta(theta);
    gradient_entry(row_ptr, col, val, n, dims, Y, theta, dY, Z);
    SHARP_API_END
}

}  // extern "C"
