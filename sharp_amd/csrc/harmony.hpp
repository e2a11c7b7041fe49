// harmony.hpp -- a Harmony-style batch integration of PCA scores: the limits, the two sizes the tests build their inputs
// from, and the hash that deals the cells to blocks and picks the start cells.  The C ABI entries (sharp_harmony*, include/sharp_hip.h)
// are defined in harmony.hip.
#pragma once
#include "graph.hpp"

namespace sharp {

constexpr int kHarmonySlab = 256;                // cells of a slab: the unit of every cells-major sum (one GEMM task, one column-sum workgroup)
constexpr int kHarmonyLdsTile = 6144;            // doubles of Y that the assign kernel holds in LDS at a time (48 KB): beyond that it tiles over clusters
constexpr int kHarmonyWaveCells = 4;             // cells that one wave of the assign kernel carries through the dots
constexpr int kHarmonyMaxD = 128;                // two columns per lane
constexpr int kHarmonyMaxK = 256;                // four clusters per lane
constexpr int kHarmonyMaxB = 4096;
constexpr int kHarmonyMaxBlocks = 1024;
constexpr long long kHarmonyMaxN = 2147483646ll;

// h(s, i) = mix64(mix64(seed G + s) + i): s = 0 deals cell i to a block, s = 1 ranks it as a start cell
__host__ __device__ __forceinline__ u64 harmony_hash(u64 seed, u64 s, u64 i) {
    return mix64(mix64(seed * 0x9E3779B97F4A7C15ull + s) + i);
}

}  // namespace sharp
