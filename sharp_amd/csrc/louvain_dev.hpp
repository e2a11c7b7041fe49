// louvain_dev.hpp -- the device code that Louvain's move kernels (louvain.hip) and Leiden's refine kernels (leiden.hip,
// §25) share: the hashed bit of a community and round, the (key, int64 sum) hash table in LDS, the gain, and the arg-max under the total
// order (gain descending, id ascending) over a wave and over a workgroup.  Nothing here depends on the order of the atomics: a table
// holds integer sums, and the arg-max is a reduction under a total order.
#pragma once
#include <climits>

#include "graph.hpp"

namespace sharp {

// x1 = mix(mix(seed * golden + level) + round); h(c) = the top bit of mix(x1 + c)
inline u64 lv_round_key(u64 seed, int level, int round) {
    return mix64(mix64(seed * 0x9E3779B97F4A7C15ull + static_cast<u64>(level)) + static_cast<u64>(round));
}
__device__ __forceinline__ bool lv_hbit(u64 x1, int c) { return (mix64(x1 + static_cast<u64>(c)) >> 63) != 0; }

constexpr int kLvNone = INT_MAX;
struct LvBest { double g; int c; };
// the total order of the arg-max: a candidate beats none; then the larger gain; then the lower id
__device__ __forceinline__ bool lv_better(double g, int c, const LvBest &b) {
    return c != kLvNone && (b.c == kLvNone || g > b.g || (g == b.g && c < b.c));
}

// the wave's best candidate and its largest `extra` (Louvain: the weight towards the vertex's own community; Leiden: a 0 / 1 flag),
// in every lane
__device__ __forceinline__ void lv_wave_best(LvBest &b, long long &extra) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(b.g, off);
        const int oc = __shfl_xor(b.c, off);
        const long long ok = __shfl_xor(extra, off);
        if (lv_better(og, oc, b)) { b.g = og; b.c = oc; }
        extra = ok > extra ? ok : extra;
    }
}

// the workgroup's (256 threads) best from its waves' (after lv_wave_best), in thread 0; ends behind a barrier only for thread 0's
// reads: the caller synchronises before red_* are written again
struct LvRed {
    double g[4];
    int c[4];
    long long k[4];
};
__device__ __forceinline__ void lv_block_best(LvBest &b, long long &extra, LvRed &red) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { red.g[tid >> 6] = b.g; red.c[tid >> 6] = b.c; red.k[tid >> 6] = extra; }
    __syncthreads();
    if (tid == 0)
        for (int o = 1; o < 4; ++o) {
            if (lv_better(red.g[o], red.c[o], b)) { b.g = red.g[o]; b.c = red.c[o]; }
            extra = red.k[o] > extra ? red.k[o] : extra;
        }
}

// gain(c) = (double)kin - ((gamma * (double)k_v) * (double)tot') / (double)(2m), in this order (gk = gamma * (double)k_v)
__device__ __forceinline__ double lv_gain(long long kin, double gk, long long totp, double m2) {
    return static_cast<double>(kin) - (gk * static_cast<double>(totp)) / m2;
}

// GROUP lanes share a table: 64 (a wave: a fence and a wave barrier) or 256 (the workgroup)
template <int GROUP>
__device__ __forceinline__ void lv_group_sync() {
    if (GROUP == 64) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// The table: SLOTS (a power of two, more than the keys it will hold) 32-bit keys >= 0 claimed by compare-and-swap, a 64-bit integer sum each
template <int GROUP, int SLOTS>
__device__ __forceinline__ void lv_table_clear(int *keys, u64 *vals, int lane) {
    for (int s = lane; s < SLOTS; s += GROUP) { keys[s] = -1; vals[s] = 0; }
}
template <int SLOTS>
__device__ __forceinline__ void lv_table_add(int *keys, u64 *vals, int c, u64 w) {
    unsigned s = (static_cast<unsigned>(c) * 0x9E3779B1u) & (SLOTS - 1);
    for (;;) {                                             // (fewer distinct keys than slots: the probe ends)
        const int prev = atomicCAS(&keys[s], -1, c);
        if (prev == -1 || prev == c) { atomicAdd(&vals[s], w); break; }
        s = (s + 1) & (SLOTS - 1);
    }
}

}  // namespace sharp
