// diffmap.hip -- diffusion maps and diffusion pseudotime on the neighbour graph: DESIGN.md §26 (the project's specification, modelled
// on scanpy's tl.diffmap / tl.dpt and Haghverdi et al. 2016; no parity with scanpy or destiny is claimed).
//   operator     q_i = sum_j W_ij; with density normalisation K = Q^-1 W Q^-1, z_i = sum_j K_ij, T = Z^-1/2 K Z^-1/2, without it
//                K = W, z = q.  T is never stored: (T x)_i = a_i sum_j W_ij a_j x_j with a_i = 1 / (q_i sqrt(z_i)) (or 1 / sqrt(q_i)),
//                which is §15's spmv_kernel with s := a.  q0 = sqrt(z) / ||sqrt(z)|| is T's eigenvector for the eigenvalue 1.
//   component    the solve runs on one connected component: its rows are flagged, two exclusive scans give the new ids and the new row
//                starts, one kernel writes the compacted row_ptr, one copies val and relabels col.
//   solver       thick-restart Lanczos on the complement of q0 with full reorthogonalisation (two classical Gram-Schmidt passes).  The
//                basis holds at most m columns.  H = Q^T T Q is taken from the first pass's coefficients, column by column, and stays
//                on the device; every kDiffmapCheckEvery applications, and whenever the basis is full, the host solves H (dense, at most
//                m x m) and reads the estimates |beta S_last,j|.  A full basis is rotated onto its top p Ritz vectors (the f64 MFMA,
//                in place) and the recurrence goes on from column p.  The true residuals of all Ritz vectors are taken in one pass
//                over W.
//   pseudotime   dpt_r(i) = sqrt(sum_l (lambda_l / (1 - lambda_l) (psi_l(r) - psi_l(i)))^2), one thread per (cell, root).
// fp64 throughout, no floating-point atomics, every sum in an order fixed by the shape alone: two calls give the same bits.
#include "diffmap.hpp"

#include <cfloat>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "graph_prim.hpp"
#include "graph_source.hpp"
#include "prepare.hpp"
#include "spectral_dev.hpp"

namespace sharp {
namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// the operator
// ---------------------------------------------------------------------------------------------------------------------------
// q_i = sum_j W_ij: one wave per row, CSR order
__global__ __launch_bounds__(256) void rowsum_kernel(const long long *__restrict__ rp, const double *__restrict__ val, long long n,
                                                     double *__restrict__ q) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long e1 = rp[i + 1];
    double s = 0.0;
    for (long long e = rp[i] + lane; e < e1; e += 64) s += val[e];
    s = wave_sum(s);
    if (lane == 0) q[i] = s;
}

// z_i = (1 / q_i) sum_j W_ij / q_j and a_i = 1 / (q_i sqrt(z_i)); without density normalisation z = q, a = 1 / sqrt(q).  One wave per
// row, lanes stride the row in passes of 64, the butterfly folds them.  An empty row: z = a = 0.
__global__ __launch_bounds__(256) void transitions_kernel(const long long *__restrict__ rp, const int *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ q, long long n, int density,
                                                          double *__restrict__ a, double *__restrict__ z, double *__restrict__ sq) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long e0 = rp[i], e1 = rp[i + 1];
    double zi = 0.0, ai = 0.0, ri = 0.0;
    if (e1 > e0) {   // (wave-uniform)
        const double qi = q[i];
        if (density) {
            double s = 0.0;
            for (long long e = e0 + lane; e < e1; e += 64) s += val[e] / q[col[e]];
            s = wave_sum(s);
            zi = s / qi;
            ri = sqrt(zi);
            ai = 1.0 / (qi * ri);
        } else {
            zi = qi;
            ri = sqrt(zi);
            ai = 1.0 / ri;
        }
    }
    if (lane == 0) {
        z[i] = zi;
        a[i] = ai;
        if (sq) sq[i] = ri;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// one component as a CSR of its own
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flag_kernel(const int *__restrict__ label, int chosen, const long long *__restrict__ rp, long long n,
                                                   int *__restrict__ flag, long long *__restrict__ len) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = label[i] == chosen;
    flag[i] = f;
    len[i] = f ? rp[i + 1] - rp[i] : 0;
}

// sub_rp[new id] = the row's start among the kept entries; new_id = -1 outside; sub_rp[ns] = the kept entries' number
__global__ __launch_bounds__(256) void rowptr_kernel(const int *__restrict__ flag, int *__restrict__ new_id, const long long *__restrict__ off,
                                                     long long n, long long ns, long long nnzs, long long *__restrict__ sub_rp) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i == 0) sub_rp[ns] = nnzs;
    if (i >= n) return;
    if (flag[i]) sub_rp[new_id[i]] = off[i];
    else new_id[i] = -1;
}

// one wave per kept row: val copied, col relabelled (a component is closed under edges: every neighbour has a new id)
__global__ __launch_bounds__(256) void extract_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                      const int *__restrict__ new_id, const long long *__restrict__ off, long long n,
                                                      int *__restrict__ sub_col, double *__restrict__ sub_val) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n || new_id[i] < 0) return;
    const long long e0 = rp[i], e1 = rp[i + 1], base = off[i];
    for (long long e = e0 + lane; e < e1; e += 64) {
        sub_col[base + (e - e0)] = new_id[col[e]];
        sub_val[base + (e - e0)] = val[e];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the projected matrix and the rotation of the basis
// ---------------------------------------------------------------------------------------------------------------------------
// column j (counted from 1) of H = Q^T T Q from the first pass's coefficients coef[0 .. j] (coef[0] is q0's), mirrored into row j
__global__ __launch_bounds__(256) void hcol_kernel(const double *__restrict__ coef, int j, double *__restrict__ H, int ld) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= j) return;
    const double v = coef[i + 1];
    H[static_cast<long long>(i) * ld + (j - 1)] = v;
    H[static_cast<long long>(j - 1) * ld + i] = v;
}

// Y = Q S in place: Q's first j columns (n contiguous doubles each) become the `keep` columns Y_c = sum_k Q_k S[k][c], k ascending in
// steps of 4 on v_mfma_f64_16x16x4_f64.  S: j rows of ldS >= 16 NT values, zero beyond column keep.  One wave owns 16 rows: it reads all
// j values of each of them before it writes (the stores depend on every load through the accumulators), and no other wave touches those
// rows, so the rotation needs no second copy of the basis.  A operand: S^T (16 output columns x 4 k), B operand: Q^T (4 k x 16 rows) --
// the 16 rows are 16 consecutive doubles of one column, for the loads and for the stores.
template <int NT>
__global__ __launch_bounds__(256) void rotate_kernel(double *Q, long long n, int j, const double *__restrict__ S, int ldS, int keep) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, kq = lane >> 4;
    const long long i0 = (static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6)) * 16;
    if (i0 >= n) return;   // (wave-uniform)
    const long long row = i0 + r16;
    const bool ok = row < n;
    v4f64 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < j; k0 += 4) {
        const int k = k0 + kq;
        const bool kok = k < j;
        const double b = (ok && kok) ? Q[static_cast<long long>(k) * n + row] : 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double a = kok ? S[static_cast<long long>(k) * ldS + t * 16 + r16] : 0.0;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = t * 16 + kq + 4 * r;
            if (ok && c < keep) Q[static_cast<long long>(c) * n + row] = acc[t][r];
        }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the Ritz vectors: norms, residuals, signs
// ---------------------------------------------------------------------------------------------------------------------------
// part[c * nb + b] = sum over chunk b of V_c[k]^2, in dots_kernel's order (grid: nb x columns)
__global__ __launch_bounds__(256) void sqnorm_kernel(const double *__restrict__ V, long long n, long long chunk, double *__restrict__ part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const double *v = V + static_cast<long long>(blockIdx.y) * n;
    const long long b0 = static_cast<long long>(blockIdx.x) * chunk, e = b0 + chunk < n ? b0 + chunk : n;
    double a = 0.0;
    for (long long k = b0 + tid; k < e; k += 256) a += v[k] * v[k];
    sh[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    if (tid == 0) part[static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x] = sh[0];
}

// V_c /= nrm[c] (grid: rows x columns)
__global__ __launch_bounds__(256) void scale_cols_kernel(double *__restrict__ V, const double *__restrict__ nrm, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double b = nrm[blockIdx.y];
    double *v = V + static_cast<long long>(blockIdx.y) * n;
    v[i] = b > 0.0 ? v[i] / b : 0.0;
}

// Vr (n rows of ld = 16 ceil(kc / 16) values) = the kc columns of V side by side, zero beyond kc: the residual pass gathers a row of it
__global__ __launch_bounds__(256) void to_rows_kernel(const double *__restrict__ V, long long n, int kc, int ld, double *__restrict__ Vr) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * ld) return;
    const long long i = e / ld;
    const int c = static_cast<int>(e - i * ld);
    Vr[e] = c < kc ? V[static_cast<long long>(c) * n + i] : 0.0;
}

// The true residuals of kc <= 64 columns in one pass over W.  A workgroup owns 256 rows, each wave 64 of them one after the other.  For a
// row the lanes are 4 entry slots x 16 column slots: lane (es, cs) takes the entries es, es + 4, ... and, of each, the columns cs, cs + 16,
// cs + 32, cs + 48; val[e] a_j is formed once per entry and lane, and the 16 column slots read 16 consecutive doubles of Vr's row j: an
// entry's gather is one 128-byte line per 16 columns.  Two butterfly steps fold the entry slots, then r = a_i sum - theta_c V_c[i] and the
// squares are added row after row.  part[c * nb + b] = the workgroup's sum (waves 0 .. 3 in order); fold_kernel folds the workgroups.
__global__ __launch_bounds__(256) void residual_kernel(const long long *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                       const double *__restrict__ a, const double *__restrict__ Vr, int ld,
                                                       const double *__restrict__ theta, long long n, int kc, double *__restrict__ part) {
    __shared__ double sh[4][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, es = lane >> 4, cs = lane & 15;
    const long long r0 = static_cast<long long>(blockIdx.x) * 256 + wave * 64;
    double racc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int rr = 0; rr < 64; ++rr) {
        const long long i = r0 + rr;
        if (i >= n) break;   // (wave-uniform)
        const long long e1 = rp[i + 1];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (long long e = rp[i] + es; e < e1; e += 4) {
            const int j = col[e];
            const double w = val[e] * a[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = cs + 16 * t;
                if (c < kc) acc[t] += w * Vr[static_cast<long long>(j) * ld + c];
            }
        }
        const double ai = a[i];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] += __shfl_xor(acc[t], 16);
            acc[t] += __shfl_xor(acc[t], 32);
            const int c = cs + 16 * t;
            if (c < kc) {
                const double r = ai * acc[t] - theta[c] * Vr[i * ld + c];
                racc[t] += r * r;
            }
        }
    }
    if (es == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) sh[wave][cs + 16 * t] = racc[t];
    }
    __syncthreads();
    if (tid < kc) part[static_cast<long long>(tid) * gridDim.x + blockIdx.x] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// the sign rule, stage 1: per chunk and column the largest |v| and its index, ties to the lowest index (grid: nb x columns)
__device__ __forceinline__ void take_larger(double &v, long long &i, double v2, long long i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__global__ __launch_bounds__(256) void absmax_kernel(const double *__restrict__ V, long long n, long long chunk, double *__restrict__ pv,
                                                     long long *__restrict__ pi) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int tid = threadIdx.x;
    const double *v = V + static_cast<long long>(blockIdx.y) * n;
    const long long b0 = static_cast<long long>(blockIdx.x) * chunk, e = b0 + chunk < n ? b0 + chunk : n;
    double m = -1.0;
    long long at = LLONG_MAX;
    for (long long k = b0 + tid; k < e; k += 256) take_larger(m, at, fabs(v[k]), k);
    sv[tid] = m;
    si[tid] = at;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) take_larger(sv[tid], si[tid], sv[tid + w], si[tid + w]);
        __syncthreads();
    }
    if (tid == 0) {
        pv[static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x] = sv[0];
        pi[static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x] = si[0];
    }
}
// stage 2: sign[c] = -1 where the column's largest |component| is negative, else 1 (grid: columns)
__global__ __launch_bounds__(256) void sign_kernel(const double *__restrict__ V, long long n, const double *__restrict__ pv,
                                                   const long long *__restrict__ pi, int nb, double *__restrict__ sign) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int tid = threadIdx.x;
    double m = -1.0;
    long long at = LLONG_MAX;
    for (int k = tid; k < nb; k += 256) take_larger(m, at, pv[static_cast<long long>(blockIdx.x) * nb + k], pi[static_cast<long long>(blockIdx.x) * nb + k]);
    sv[tid] = m;
    si[tid] = at;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) take_larger(sv[tid], si[tid], sv[tid + w], si[tid + w]);
        __syncthreads();
    }
    if (tid == 0) sign[blockIdx.x] = (si[0] < n && V[static_cast<long long>(blockIdx.x) * n + si[0]] < 0.0) ? -1.0 : 1.0;
}

// out (n x nc row-major, the full graph's rows): sign_c V_c[new id] inside the component, NaN outside; in_comp = 1 / 0
__global__ __launch_bounds__(256) void scatter_kernel(const double *__restrict__ V, long long ns, const double *__restrict__ sign,
                                                      const int *__restrict__ new_id, long long n, int nc, double *__restrict__ out,
                                                      int *__restrict__ in_comp) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * nc) return;
    const long long i = e / nc;
    const int c = static_cast<int>(e - i * nc);
    const int id = new_id[i];
    out[e] = id >= 0 ? sign[c] * V[static_cast<long long>(c) * ns + id] : __builtin_nan("");
    if (c == 0) in_comp[i] = id >= 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// pseudotime
// ---------------------------------------------------------------------------------------------------------------------------
// out[i * n_roots + r] = sqrt(sum_{l = 1}^{n_dcs - 1} (w_l (psi_l(root_r) - psi_l(i)))^2), l ascending; inf for a row of NaN
__global__ __launch_bounds__(256) void dpt_kernel(const double *__restrict__ psi, const double *__restrict__ w, long long n, int nc, int n_dcs,
                                                  const int *__restrict__ roots, int n_roots, double *__restrict__ out) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * n_roots) return;
    const long long i = e / n_roots;
    const int r = static_cast<int>(e - i * n_roots);
    const double *pi = psi + i * nc, *pr = psi + static_cast<long long>(roots[r]) * nc;
    if (isnan(pi[0])) { out[e] = HUGE_VAL; return; }
    double s = 0.0;
    for (int l = 1; l < n_dcs; ++l) {
        const double t = w[l] * (pr[l] - pi[l]);
        s += t * t;
    }
    out[e] = sqrt(s);
}

// mx[r] = the largest finite value of column r (grid: roots); a maximum does not depend on the order
__global__ __launch_bounds__(256) void dpt_max_kernel(const double *__restrict__ out, long long n, int n_roots, double *__restrict__ mx) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    double m = 0.0;
    for (long long i = tid; i < n; i += 256) {
        const double v = out[i * n_roots + blockIdx.x];
        if (v < HUGE_VAL && v > m) m = v;
    }
    sh[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && sh[tid + w] > sh[tid]) sh[tid] = sh[tid + w];
        __syncthreads();
    }
    if (tid == 0) mx[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void dpt_div_kernel(double *__restrict__ out, long long n, int n_roots, const double *__restrict__ mx) {
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n * n_roots) return;
    const double m = mx[e % n_roots];
    if (m > 0.0 && out[e] < HUGE_VAL) out[e] = out[e] / m;
}

template <int NT>
void rotate_launch(double *Q, long long n, int j, const double *S, int ldS, int keep) {
    hipLaunchKernelGGL(rotate_kernel<NT>, dim3(grid_for(n, 64)), dim3(256), 0, ctx().stream, Q, n, j, S, ldS, keep);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
void diffmap_transitions(const Graph &G, bool density, DevBuf<double> &a, DevBuf<double> &z, DevBuf<double> *sq) {
    KernelTimer t("diffmap_transitions");
    const long long n = G.n;
    DevBuf<double> q(n);
    a.alloc(n);
    z.alloc(n);
    if (sq) sq->alloc(n);
    hipLaunchKernelGGL(rowsum_kernel, dim3(grid_for(n, 4)), dim3(256), 0, ctx().stream, G.row_ptr.p, G.val.p, n, q.p);
    launch_check("rowsum_kernel");
    hipLaunchKernelGGL(transitions_kernel, dim3(grid_for(n, 4)), dim3(256), 0, ctx().stream, G.row_ptr.p, G.col.p, G.val.p, q.p, n, density ? 1 : 0,
                       a.p, z.p, sq ? sq->p : nullptr);
    launch_check("transitions_kernel");
    stream_sync();   // (q goes out of scope)
}

void diffmap_component(const Graph &G, long long root, DiffmapComponent &C) {
    const long long n = G.n;
    SHARP_REQUIRE(n >= 1 && n < INT_MAX, "diffmap: need 1 <= n < 2^31 rows");
    SHARP_REQUIRE(root >= -1 && root < n, "diffmap: root must be -1 or a row of the graph");
    DevBuf<int> label;
    C.components = csr_components(G.row_ptr.p, G.col.p, n, nullptr, label, "diffmap_components");
    std::vector<int> hl(n);
    label.download(hl.data(), n);
    int chosen;
    if (root >= 0) {
        chosen = hl[root];
    } else {   // the largest, ties to the smallest label (a label is its component's smallest vertex)
        std::vector<int> size(n, 0);
        for (long long i = 0; i < n; ++i) ++size[hl[i]];
        chosen = 0;
        for (long long l = 1; l < n; ++l)
            if (size[l] > size[chosen]) chosen = static_cast<int>(l);
    }
    C.label = chosen;

    KernelTimer t("diffmap_extract");
    Ctx &c = ctx();
    DevBuf<int> flag(n);
    DevBuf<long long> len(n), off(n);
    Scratch scratch;
    C.new_id.alloc(n);
    hipLaunchKernelGGL(flag_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, label.p, chosen, G.row_ptr.p, n, flag.p, len.p);
    launch_check("flag_kernel");
    exclusive_scan(flag.p, C.new_id.p, static_cast<size_t>(n), scratch);
    exclusive_scan(len.p, off.p, static_cast<size_t>(n), scratch);
    int last_id = 0, last_flag = 0;
    long long last_off = 0, last_len = 0;
    SHARP_HIP_CHECK(hipMemcpyAsync(&last_id, C.new_id.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost, c.stream));
    SHARP_HIP_CHECK(hipMemcpyAsync(&last_flag, flag.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost, c.stream));
    SHARP_HIP_CHECK(hipMemcpyAsync(&last_off, off.p + (n - 1), sizeof(long long), hipMemcpyDeviceToHost, c.stream));
    SHARP_HIP_CHECK(hipMemcpyAsync(&last_len, len.p + (n - 1), sizeof(long long), hipMemcpyDeviceToHost, c.stream));
    stream_sync();
    const long long ns = static_cast<long long>(last_id) + last_flag, nnzs = last_off + last_len;
    SHARP_REQUIRE(ns >= 1 && ns <= n && nnzs >= 0 && nnzs <= G.nnz, "diffmap: the component's extraction lost count");
    C.sub.n = ns;
    C.sub.nnz = nnzs;
    C.sub.wmax = G.wmax;
    C.sub.row_ptr.alloc(ns + 1);
    C.sub.col.alloc(std::max<long long>(nnzs, 1));
    C.sub.val.alloc(std::max<long long>(nnzs, 1));
    hipLaunchKernelGGL(rowptr_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, flag.p, C.new_id.p, off.p, n, ns, nnzs, C.sub.row_ptr.p);
    launch_check("rowptr_kernel");
    hipLaunchKernelGGL(extract_kernel, dim3(grid_for(n, 4)), dim3(256), 0, c.stream, G.row_ptr.p, G.col.p, G.val.p, C.new_id.p, off.p, n, C.sub.col.p,
                       C.sub.val.p);
    launch_check("extract_kernel");
    stream_sync();   // (flag, len, off and the scratch go out of scope)
}

void diffmap_solve(const Graph &G, int n_comps, bool density, double tol, int max_matvecs, DevBuf<double> &V, DiffmapSolve &R) {
    Ctx &c = ctx();
    const long long n = G.n;
    const int k = n_comps - 1;
    SHARP_REQUIRE(n_comps >= 2 && n_comps <= kDiffmapMaxComps, "diffmap: n_comps must be in 2 .. 64");
    SHARP_REQUIRE(n >= n_comps + 2 && n < INT_MAX, "diffmap: need n_comps + 2 <= n < 2^31 rows");
    SHARP_REQUIRE(!std::isnan(tol) && tol < HUGE_VAL, "diffmap: tol must be finite (<= 0: the default)");
    if (!(tol > 0.0)) tol = kDiffmapTol;
    const int cap = max_matvecs > 0 ? max_matvecs : kDiffmapMaxMatvecs;
    const int p_full = diffmap_keep(k);
    const int m = static_cast<int>(std::min<long long>(diffmap_basis(k), n - 1));   // (n - 1: the dimension of q0's complement)
    const int ldS = 16 * ((p_full + 15) / 16);
    R = DiffmapSolve();
    R.theta.assign(n_comps, 0.0);
    R.residual.assign(n_comps, 0.0);

    DevBuf<double> a, z, sq;
    diffmap_transitions(G, density, a, z, &sq);
    // columns: q0, q_1 .. q_m, and the vector beyond the basis
    DevBuf<double> Q(static_cast<size_t>(n) * (m + 2)), u(n), coef(m + 2), beta(m + 1), H(static_cast<size_t>(m) * m), Sd(static_cast<size_t>(m) * ldS);
    DevBuf<double> thetad(n_comps), scal(n_comps + 1), resd(n_comps);
    V.alloc(static_cast<size_t>(n) * n_comps);
    const int ldr = 16 * ((n_comps + 15) / 16);
    DevBuf<double> Vr(static_cast<size_t>(n) * ldr);   // the Ritz vectors once more, row by row, for the residual pass
    Reducer red(n, m + 2);
    const unsigned rblocks = grid_for(n, 256);
    DevBuf<double> rpart(static_cast<size_t>(rblocks) * n_comps);
    auto col = [&](int j) { return Q.p + static_cast<long long>(j) * n; };
    H.zero();

    {
        KernelTimer t("diffmap_lanczos");
        red.dots(sq.p, 1, sq.p, scal.p, true);
        scale(sq.p, scal.p, col(0), n);
        hipLaunchKernelGGL(start_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c.stream, u.p, n);
        launch_check("start_kernel");
        // the start orthogonalised against q0 (two passes), normalised into column 1
        for (int pass = 0; pass < 2; ++pass) {
            red.dots(Q.p, 1, u.p, coef.p);
            apply(Q.p, 1, coef.p, u.p, n);
        }
        red.dots(u.p, 1, u.p, scal.p, true);
        scale(u.p, scal.p, col(1), n);
    }
    SHARP_HIP_CHECK(hipMemcpyAsync(V.p, col(0), static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToDevice, c.stream));

    std::vector<double> hb(m + 1), hH(static_cast<size_t>(m) * m), A, w, hS(static_cast<size_t>(m) * ldS), hres(n_comps), est(k);
    std::vector<int> ord;
    int jc = 0;   // the basis' completed columns: H is jc x jc, column jc + 1 holds the next vector
    int jr = 0;   // the columns a restart left: their betas are not the recurrence's
    for (;;) {
        {
            // one step: u = T q_{jc+1}, orthogonalised against q0 and the basis; the first pass's coefficients are H's column
            KernelTimer t("diffmap_lanczos");
            const int ncols = jc + 2;
            spmv(G, a.p, col(jc + 1), u.p);
            red.dots(Q.p, ncols, u.p, coef.p);
            hipLaunchKernelGGL(hcol_kernel, dim3(grid_for(jc + 1, 256)), dim3(256), 0, c.stream, coef.p, jc + 1, H.p, m);
            launch_check("hcol_kernel");
            apply(Q.p, ncols, coef.p, u.p, n);
            red.dots(Q.p, ncols, u.p, coef.p);
            apply(Q.p, ncols, coef.p, u.p, n);
            red.dots(u.p, 1, u.p, beta.p + jc, true);
            scale(u.p, beta.p + jc, col(jc + 2), n);
        }
        ++jc;
        ++R.steps;
        const bool full = jc == m, capped = R.steps >= cap;
        if (R.steps % kDiffmapCheckEvery != 0 && !full && !capped) continue;

        SHARP_HIP_CHECK(hipMemcpyAsync(hb.data() + jr, beta.p + jr, static_cast<size_t>(jc - jr) * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        H.download(hH.data(), hH.size());
        // a beta at rounding level: the basis spans an invariant subspace, H's pairs are exact and nothing lies beyond; so they are
        // when the basis fills q0's complement
        int jj = jc;
        bool exhausted = false;
        for (int t = jr; t < jc; ++t)
            if (!(hb[t] > 64.0 * DBL_EPSILON)) { jj = t + 1; exhausted = true; break; }
        if (jj >= n - 1) exhausted = true;
        if (jj < k) {
            SHARP_REQUIRE(!exhausted, "diffmap: the Krylov space is exhausted after " + std::to_string(jj) + " steps, before n_comps - 1 pairs exist");
            if (!capped) continue;
            SHARP_REQUIRE(false, "diffmap: max_matvecs is smaller than n_comps - 1");
        }
        A.assign(static_cast<size_t>(jj) * jj, 0.0);
        for (int r = 0; r < jj; ++r)
            for (int s = 0; s < jj; ++s) A[static_cast<size_t>(r) * jj + s] = hH[static_cast<size_t>(r) * m + s];
        symmetric_eigen("diffmap", jj, A, w);   // (the vectors in A's columns, in no order)
        ord.resize(jj);
        for (int t = 0; t < jj; ++t) ord[t] = t;
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return w[x] > w[y]; });
        bool conv = true;
        for (int t = 0; t < k; ++t) {
            est[t] = exhausted ? 0.0 : std::fabs(hb[jj - 1] * A[static_cast<size_t>(jj - 1) * jj + ord[t]]);
            conv = conv && est[t] <= tol;
        }
        if (!conv && !capped && !full) continue;

        // the basis rotated onto its top `keep` Ritz vectors; H = diag(theta); the vector beyond the basis follows them
        const int keep = std::max(k, std::min(p_full, jj - 1));
        {
            KernelTimer t("diffmap_restart");
            std::fill(hS.begin(), hS.end(), 0.0);
            for (int r = 0; r < jj; ++r)
                for (int s = 0; s < keep; ++s) hS[static_cast<size_t>(r) * ldS + s] = A[static_cast<size_t>(r) * jj + ord[s]];
            Sd.upload(hS.data(), static_cast<size_t>(jj) * ldS);
            switch ((keep + 15) / 16) {
                case 1: rotate_launch<1>(col(1), n, jj, Sd.p, ldS, keep); break;
                case 2: rotate_launch<2>(col(1), n, jj, Sd.p, ldS, keep); break;
                case 3: rotate_launch<3>(col(1), n, jj, Sd.p, ldS, keep); break;
                case 4: rotate_launch<4>(col(1), n, jj, Sd.p, ldS, keep); break;
                case 5: rotate_launch<5>(col(1), n, jj, Sd.p, ldS, keep); break;
                default: rotate_launch<6>(col(1), n, jj, Sd.p, ldS, keep); break;
            }
            launch_check("rotate_kernel");
            if (keep < jj)
                SHARP_HIP_CHECK(hipMemcpyAsync(col(keep + 1), col(jj + 1), static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
            std::fill(hH.begin(), hH.end(), 0.0);
            for (int s = 0; s < keep; ++s) hH[static_cast<size_t>(s) * m + s] = w[ord[s]];
            H.upload(hH.data(), hH.size());
            stream_sync();   // (hS and hH are pageable host memory in flight)
        }
        jc = jr = keep;
        if (conv || capped) {
            KernelTimer t("diffmap_residuals");
            R.theta[0] = 1.0;
            for (int t = 0; t < k; ++t) R.theta[t + 1] = w[ord[t]];
            thetad.upload(R.theta.data(), n_comps);
            SHARP_HIP_CHECK(hipMemcpyAsync(V.p + n, col(1), static_cast<size_t>(n) * k * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
            hipLaunchKernelGGL(sqnorm_kernel, dim3(red.nb, k), dim3(256), 0, c.stream, V.p + n, n, red.chunk, red.part.p);
            hipLaunchKernelGGL(fold_kernel, dim3(k), dim3(256), 0, c.stream, red.part.p, static_cast<int>(red.nb), scal.p, 1,
                               static_cast<double *>(nullptr));
            hipLaunchKernelGGL(scale_cols_kernel, dim3(grid_for(n, 256), k), dim3(256), 0, c.stream, V.p + n, scal.p, n);
            launch_check("scale_cols_kernel");
            hipLaunchKernelGGL(to_rows_kernel, dim3(grid_for(n * ldr, 256)), dim3(256), 0, c.stream, V.p, n, n_comps, ldr, Vr.p);
            hipLaunchKernelGGL(residual_kernel, dim3(rblocks), dim3(256), 0, c.stream, G.row_ptr.p, G.col.p, G.val.p, a.p, Vr.p, ldr, thetad.p, n,
                               n_comps, rpart.p);
            hipLaunchKernelGGL(fold_kernel, dim3(n_comps), dim3(256), 0, c.stream, rpart.p, static_cast<int>(rblocks), resd.p, 1,
                               static_cast<double *>(nullptr));
            launch_check("residual_kernel");
            resd.download(hres.data(), n_comps);
            bool ok = true;
            for (int t = 0; t < n_comps; ++t) { R.residual[t] = hres[t]; ok = ok && hres[t] <= tol; }
            if (ok || capped || exhausted) {
                R.outcome = ok ? 0 : 2;
                stream_sync();
                return;
            }
        }
        ++R.restarts;
    }
}

}  // namespace sharp

using namespace sharp;

namespace {

// V (ns x nc, column by column) under the sign rule, scattered to the n rows of the full graph (row-major, NaN outside the component)
void sign_and_scatter(const DevBuf<double> &V, long long ns, int nc, const DevBuf<int> &new_id, long long n, double *evecs, int *in_component) {
    Ctx &c = ctx();
    const long long chunk = std::max<long long>(256, (ns + kRedBlocks - 1) / kRedBlocks);
    const unsigned nb = static_cast<unsigned>((ns + chunk - 1) / chunk);
    DevBuf<double> pv(static_cast<size_t>(nb) * nc), sign(nc), out(static_cast<size_t>(n) * nc);
    DevBuf<long long> pi(static_cast<size_t>(nb) * nc);
    DevBuf<int> inc(n);
    hipLaunchKernelGGL(absmax_kernel, dim3(nb, nc), dim3(256), 0, c.stream, V.p, ns, chunk, pv.p, pi.p);
    hipLaunchKernelGGL(sign_kernel, dim3(nc), dim3(256), 0, c.stream, V.p, ns, pv.p, pi.p, static_cast<int>(nb), sign.p);
    launch_check("sign_kernel");
    hipLaunchKernelGGL(scatter_kernel, dim3(grid_for(n * nc, 256)), dim3(256), 0, c.stream, V.p, ns, sign.p, new_id.p, n, nc, out.p, inc.p);
    launch_check("scatter_kernel");
    out.download(evecs, static_cast<size_t>(n) * nc);
    inc.download(in_component, static_cast<size_t>(n));
}

}  // namespace

extern "C" {

int sharp_diffmap_transitions(const long long *row_ptr, const int *col, const double *val, long long n, int density_normalize, double *a, double *z) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(n >= 1 && n < INT_MAX, "sharp_diffmap_transitions: need 1 <= n < 2^31 rows");
    SHARP_REQUIRE(val && a && z, "sharp_diffmap_transitions: null argument");
    Graph G;
    upload_csr("sharp_diffmap_transitions", row_ptr, col, val, n, G);
    DevBuf<double> da, dz;
    diffmap_transitions(G, density_normalize != 0, da, dz);
    da.download(a, static_cast<size_t>(n));
    dz.download(z, static_cast<size_t>(n));
    SHARP_API_END
}

int sharp_diffmap_component(const long long *row_ptr, const int *col, const double *val, long long n, int n_comps, long long root, int *label,
                            long long *components, long long *sub_n, long long *sub_nnz, long long *sub_row_ptr, int *sub_col, double *sub_val,
                            int *new_id) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(n >= 1 && n < INT_MAX, "sharp_diffmap_component: need 1 <= n < 2^31 rows");
    SHARP_REQUIRE(n_comps >= 2 && n_comps <= kDiffmapMaxComps, "sharp_diffmap_component: n_comps must be in 2 .. 64");
    SHARP_REQUIRE(root >= -1 && root < n, "sharp_diffmap_component: root must be -1 or a row of the graph");
    SHARP_REQUIRE(val && label && components && sub_n && sub_nnz && sub_row_ptr && sub_col && sub_val && new_id, "sharp_diffmap_component: null argument");
    Graph G;
    upload_csr("sharp_diffmap_component", row_ptr, col, val, n, G);
    DiffmapComponent C;
    diffmap_component(G, root, C);
    *label = C.label;
    *components = C.components;
    *sub_n = C.sub.n;
    *sub_nnz = C.sub.nnz;
    SHARP_REQUIRE(C.sub.n >= n_comps + 2, "sharp_diffmap_component: the component of label " + std::to_string(C.label) + " holds " +
                                              std::to_string(C.sub.n) + " rows, fewer than n_comps + 2");
    C.sub.row_ptr.download(sub_row_ptr, static_cast<size_t>(C.sub.n) + 1);
    if (C.sub.nnz) {
        C.sub.col.download(sub_col, static_cast<size_t>(C.sub.nnz));
        C.sub.val.download(sub_val, static_cast<size_t>(C.sub.nnz));
    }
    C.new_id.download(new_id, static_cast<size_t>(n));
    SHARP_API_END
}

// the whole call on a graph on the device: the component, the solve, the sign rule and the scatter to the n rows
static void run_diffmap(const std::string &w, const Graph &G, int n_comps, int density_normalize, long long root, double tol, int max_matvecs,
                        double *evals, double *evecs, double *residual, int *in_component, int *steps, int *restarts, long long *components,
                        long long *component_size, int *outcome) {
    DiffmapComponent C;
    diffmap_component(G, root, C);
    *components = C.components;
    *component_size = C.sub.n;
    SHARP_REQUIRE(C.sub.n >= n_comps + 2, w + ": the component of label " + std::to_string(C.label) + " holds " + std::to_string(C.sub.n) +
                                              " rows, fewer than n_comps + 2");
    DevBuf<double> V;
    DiffmapSolve R;
    diffmap_solve(C.sub, n_comps, density_normalize != 0, tol, max_matvecs, V, R);
    *steps = R.steps;
    *restarts = R.restarts;
    *outcome = R.outcome;
    std::copy(R.theta.begin(), R.theta.end(), evals);
    std::copy(R.residual.begin(), R.residual.end(), residual);
    sign_and_scatter(V, C.sub.n, n_comps, C.new_id, G.n, evecs, in_component);
}

static void diffmap_args(const std::string &w, long long n, int n_comps, long long root, double tol) {
    SHARP_REQUIRE(n_comps >= 2 && n_comps <= kDiffmapMaxComps, w + ": n_comps must be in 2 .. 64");
    SHARP_REQUIRE(n >= n_comps + 2 && n < INT_MAX, w + ": need n_comps + 2 <= n < 2^31 rows");
    SHARP_REQUIRE(root >= -1 && root < n, w + ": root must be -1 or a row of the graph");
    SHARP_REQUIRE(!std::isnan(tol) && tol < HUGE_VAL, w + ": tol must be finite (<= 0: the default)");
}

int sharp_diffmap_graph(const long long *row_ptr, const int *col, const double *val, long long n, int n_comps, int density_normalize, long long root,
                        double tol, int max_matvecs, double *evals, double *evecs, double *residual, int *in_component, int *steps, int *restarts,
                        long long *components, long long *component_size, int *outcome) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("sharp_diffmap_graph");
    diffmap_args(w, n, n_comps, root, tol);
    SHARP_REQUIRE(val && evals && evecs && residual && in_component && steps && restarts && components && component_size && outcome,
                  w + ": null argument");
    Graph G;
    upload_csr(w.c_str(), row_ptr, col, val, n, G);
    run_diffmap(w, G, n_comps, density_normalize, root, tol, max_matvecs, evals, evecs, residual, in_component, steps, restarts, components,
                component_size, outcome);
    SHARP_API_END
}

int sharp_diffmap_neighbors(const int *index, const double *distance, long long n, int K, int squared, int n_comps, int density_normalize,
                            long long root, double tol, int max_matvecs, double *evals, double *evecs, double *residual, int *in_component,
                            int *steps, int *restarts, long long *components, long long *component_size, int *outcome) {
    SHARP_API_BEGIN
    ctx();
    const std::string w("sharp_diffmap_neighbors");
    SHARP_REQUIRE(index && distance, w + ": null index / distance");
    SHARP_REQUIRE(K >= 1 && K <= 255 && K <= n - 1, w + ": need 1 <= K <= 255 neighbours per row and K <= n - 1");
    diffmap_args(w, n, n_comps, root, tol);
    SHARP_REQUIRE(evals && evecs && residual && in_component && steps && restarts && components && component_size && outcome, w + ": null argument");
    Graph G;
    fuzzy_graph_from_lists(w, index, distance, n, K, squared != 0, G);   // (the fuzzy union of umap_neighbors: it never leaves the device)
    run_diffmap(w, G, n_comps, density_normalize, root, tol, max_matvecs, evals, evecs, residual, in_component, steps, restarts, components,
                component_size, outcome);
    SHARP_API_END
}

int sharp_dpt(const double *evals, const double *evecs, long long n, int n_comps, int n_dcs, const int *roots, int n_roots, int normalize,
              double *out) {
    SHARP_API_BEGIN
    Ctx &c = ctx();
    SHARP_REQUIRE(evals && evecs && roots && out, "sharp_dpt: null argument");
    SHARP_REQUIRE(n >= 1 && n < INT_MAX, "sharp_dpt: need 1 <= n < 2^31 rows");
    SHARP_REQUIRE(n_comps >= 2 && n_comps <= kDiffmapMaxComps, "sharp_dpt: n_comps must be in 2 .. 64");
    SHARP_REQUIRE(n_dcs >= 2 && n_dcs <= n_comps, "sharp_dpt: n_dcs must be in 2 .. n_comps");
    SHARP_REQUIRE(n_roots >= 1 && n_roots <= 4096, "sharp_dpt: need 1 .. 4096 roots");
    std::vector<double> w(n_dcs, 0.0);
    for (int l = 1; l < n_dcs; ++l) {
        SHARP_REQUIRE(evals[l] > -1.0 && evals[l] < 1.0, "sharp_dpt: an eigenvalue beyond the trivial one must lie inside (-1, 1)");
        w[l] = evals[l] / (1.0 - evals[l]);
    }
    for (int r = 0; r < n_roots; ++r) {
        SHARP_REQUIRE(roots[r] >= 0 && roots[r] < n, "sharp_dpt: a root out of range");
        SHARP_REQUIRE(!std::isnan(evecs[static_cast<size_t>(roots[r]) * n_comps]), "sharp_dpt: a root outside the component that was solved");
    }
    KernelTimer t("dpt");
    DevBuf<double> psi(static_cast<size_t>(n) * n_comps), dw(n_dcs), dout(static_cast<size_t>(n) * n_roots), mx(n_roots);
    DevBuf<int> dr(n_roots);
    psi.upload(evecs, static_cast<size_t>(n) * n_comps);
    dw.upload(w.data(), n_dcs);
    dr.upload(roots, n_roots);
    hipLaunchKernelGGL(dpt_kernel, dim3(grid_for(n * n_roots, 256)), dim3(256), 0, c.stream, psi.p, dw.p, n, n_comps, n_dcs, dr.p, n_roots, dout.p);
    launch_check("dpt_kernel");
    if (normalize) {
        hipLaunchKernelGGL(dpt_max_kernel, dim3(n_roots), dim3(256), 0, c.stream, dout.p, n, n_roots, mx.p);
        hipLaunchKernelGGL(dpt_div_kernel, dim3(grid_for(n * n_roots, 256)), dim3(256), 0, c.stream, dout.p, n, n_roots, mx.p);
        launch_check("dpt_div_kernel");
    }
    dout.download(out, static_cast<size_t>(n) * n_roots);
    SHARP_API_END
}

}  // extern "C"
