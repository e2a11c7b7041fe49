// knn_dev.hpp -- the device helpers of every top-K list in LDS, one definition each: the exact k-NN (knn.hip), NN-descent
// (knn_descent.hip) and the neighbour ranks (neighbor_rank.hip) build their kernels from these.  __device__ __forceinline__, as
// graph.hpp's helpers are: the build has no relocatable device code.
#pragma once

namespace sharp {

constexpr int KQ = 16;       // query rows per workgroup (one MFMA row block)
constexpr int KCT = 64;      // candidates per column tile (4 waves x 16 MFMA columns)
constexpr int KDT = KCT + 1; // LDS row of the distance tile
constexpr double KNN_INF = 1.0e300;

// the order of every list: by distance, ties to the lower index
__device__ __forceinline__ bool lex_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

// a wave's LDS writes are visible to its lanes' later reads
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Offers a tile of 64 candidates (lane l: distance v, index ci, valid) to one row's top-K list in LDS (Ld / Li, K entries, unsorted; the
// row's current worst (thr, widx) at wpos).  A ballot of (dist, index) < worst leaves the few that enter; each replaces the worst and the
// new worst is found by a wave-wide argmax.
__device__ __forceinline__ void knn_offer(double v, int ci, bool valid, double *Ld, int *Li, int K, int lane, double &thr, int &widx, int &wpos) {
    unsigned long long m = __ballot(valid && lex_less(v, ci, thr, widx));
    while (m) {   // (at most 64 turns: one bit leaves per turn)
        const int bsel = __ffsll(static_cast<long long>(m)) - 1;
        m &= m - 1;
        const double vb = __shfl(v, bsel);
        const int ib = __shfl(ci, bsel);
        if (!lex_less(vb, ib, thr, widx)) continue;
        if (lane == 0) { Ld[wpos] = vb; Li[wpos] = ib; }
        wave_sync();
        double bd = -1.0;
        int bi = -1, bp = 0;
        for (int p = lane; p < K; p += 64) {
            const double dv = Ld[p];
            const int iv = Li[p];
            if (lex_less(bd, bi, dv, iv)) { bd = dv; bi = iv; bp = p; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(bd, off);
            const int oi = __shfl_xor(bi, off), op = __shfl_xor(bp, off);
            if (lex_less(bd, bi, od, oi)) { bd = od; bi = oi; bp = op; }
        }
        thr = bd;
        widx = bi;
        wpos = bp;   // (lane 0's copy is the one used: a position holding the worst)
    }
}

// The rank step of a write: how many of a row's K entries come before (dp, ip) in (distance, index) order.  The indices of a row
// differ, so the ranks of its entries are a permutation and a kernel writes entry p at its rank.
__device__ __forceinline__ int knn_rank(const double *Ld, const int *Li, int K, double dp, int ip) {
    int rank = 0;
    for (int q = 0; q < K; ++q) rank += lex_less(Ld[q], Li[q], dp, ip) ? 1 : 0;
    return rank;
}

}  // namespace sharp
