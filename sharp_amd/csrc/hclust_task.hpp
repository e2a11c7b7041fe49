// hclust_task.hpp -- what the translation units behind hclust.hpp share (not part of its public face):
//   hclust.hip         workspaces, the chunk pipeline (setup_chunk / enqueue_chunk / finish_chunk), hclust_tree, the C ABI
//   hclust_agglo.hip   a4: the two agglomeration kernels and their launchers
//   hclust_stats.hip   a5: cutree, the per-level statistics kernels and their launchers
//   hclust_select.hip  model selection on the host and the decision log
// The task descriptors, the constants both sides of a launch use, ONE definition of every dynamic-LDS layout (the kernel carves its
// pointers from it; the host sizes the launch, the image stride and the global-state stride from it) and the stage launchers.
#pragma once
#include <algorithm>

#include "hclust.hpp"

namespace sharp {

// launchers and host helpers that cross these units stay out of the library's dynamic symbol table
#define SHARP_HC_LOCAL __attribute__((visibility("hidden")))

struct HcMeta {
    int n, p, nld, kmin, kmax, nk, kpad, method;
    int symmetric, pad0;
    long long oD, oD0;        // working distance matrix; pristine copy (symmetric tasks only)
    long long oCr, oCt, oNrm;
    long long oM;             // ia / ib / height: n entries per task
    long long oLab;           // nk * n ints
    long long oH, oT, oG;     // n * kpad doubles each
    long long oCSt, oQ;       // p * kpad, kpad * kpad
    long long oOut;           // msil[nk] then CH[nk]
    const double *nn;         // row minima per 128-column tile written by the distance GEMM ([nld / 128 slots][nld rows], at most 16 slots); nullptr: scan D
};
struct MlMeta {               // many-levels statistics (ml_*_kernel)
    long long oS;                    // n * nk doubles: s[i][L]; w follows at oS + n * nk
    long long oMerge;                // nk entries of r1 / r2 / cn2 of the merged cluster / B of the level
    long long oFin;                  // kf entries of cntF (int) / cn2F / ctotF
};

constexpr int HC_THREADS = 512;
constexpr double HC_INF = 1.0e300;
constexpr int HR_MAXN = 4096;
constexpr size_t HR_LDS_CU = 160 * 1024;     // LDS of a gfx950 compute unit
constexpr int ST_THREADS = 512;
constexpr size_t ST_LDS_MAX = 160 * 1024;
constexpr int SS_WAVES = 2, SS_KMAX = 144;   // cluster_sums_kernel: waves per workgroup, widest clustering it takes
constexpr int ML_WAVES = 3;                  // ml_cells_kernel: cells in flight per workgroup: 44 B of LDS per finest cluster and wave

// a kernel's dynamic LDS beyond the default 64 KB has to be allowed before the launch
template <typename K>
static inline void allow_dynamic_lds(K kern, size_t bytes) {
    SHARP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
}

__host__ __device__ inline int hc_npow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// ---- dynamic-LDS layouts ------------------------------------------------------------------------------------------------------------
// One definition per layout: a list X(type, name, count) of the kernel's arrays, in order.  The kernel expands it with LDS_CARVE, which
// declares every array as a pointer taken off the cursor `lds_cursor` (an unsigned char * that the kernel sets to the start; afterwards
// it points behind the last array).  The host expands it with LDS_COUNT into `lds_bytes`, and sizes the launch, a task's image and a
// task's state in global memory from that.  An array added to a list is added to both.
#define LDS_CARVE(type, name, count) \
    [[maybe_unused]] type *name = reinterpret_cast<type *>(lds_cursor); lds_cursor = reinterpret_cast<unsigned char *>(name + (count));
#define LDS_COUNT(type, name, count) lds_bytes += sizeof(type) * static_cast<size_t>(count);

// hclust_kernel<GS>: the nearest-neighbour state, nal = (n + 1) & ~1 ...
#define HC_SEQ_STATE_ARRAYS(X, n, nal)                                                                                      \
    X(double, disnn, nal)                                                                                                   \
    X(double, pv, 32)                                                                                                       \
    X(int, nn, nal)                                                                                                         \
    X(int, membr, nal)                                                                                                      \
    X(int, list, nal)                                                                                                       \
    X(int, pi, 32)                                                                                                          \
    X(int, cnt, 2)                                                                                                          \
    X(unsigned char, flag, n)
// ... and behind it the scratch of the second block reduction of a merge (the kernel declares it where the merge loop starts)
#define HC_SEQ_SCRATCH_ARRAYS(X, n)                                                                                         \
    X(unsigned char, flag_pad, (((n) + 7) & ~7) - (n))     /* rounds flag[] up to a multiple of 8 */                        \
    X(double, pvB, 32)                                                                                                      \
    X(int, piB, 32)
// the dynamic LDS of a launch, and the stride of the per-task state in global memory (GS)
inline size_t hc_seq_state_bytes(int max_n) {
    const int nal = (max_n + 1) & ~1;
    size_t lds_bytes = 0;
    HC_SEQ_STATE_ARRAYS(LDS_COUNT, max_n, nal)
    HC_SEQ_SCRATCH_ARRAYS(LDS_COUNT, max_n)
    const size_t slack = 32 - (((max_n + 7) & ~7) - max_n);     // 32 unused bytes, less what rounds flag[] up to a multiple of 8
    return (lds_bytes + slack + 15) / 16 * 16;
}

// hclust_rnn_kernel<HR_THREADS, MODE, GS>: the state arrays (in LDS, or the task's image in global memory); nal = (n + 3) & ~3,
// nwave = HR_THREADS / 64
#define HR_STATE_ARRAYS(X, nal, nwave)                                                                                      \
    X(double, dnnA, 2 * (nal))        /* [2][nal]  NN distance (also the pair's height) */                                  \
    X(uint16_t, cidA, 2 * (nal))      /* [2][nal]  smallest original member */                                              \
    X(uint16_t, cszA, 2 * (nal))      /* [2][nal]  cluster size */                                                          \
    X(uint16_t, nn, nal)                                                                                                    \
    X(uint16_t, partner, nal)         /* old index of the RNN partner or NONE */                                            \
    X(uint16_t, pseq, nal)            /* rank of the pair in the round */                                                   \
    X(uint16_t, oldidx, nal)          /* new index -> old index */                                                          \
    X(uint16_t, newidx, nal)          /* old index -> new index (survivors) */                                              \
    X(uint16_t, plist, nal)           /* first members of the pairs */                                                      \
    X(uint16_t, colmap, nal)          /* old column -> new column, or 0x8000 | (2 rank + member) for the two members of a pair */ \
    X(int, ctl, 16)                   /* 0 npairs, 1 abort, 2/3 work counters (plain / merged rows), 4 nsingle, */          \
                                      /* 5 cur, 6 na, 7 done, 8 src + 1, 9 nb, 10 state, 11 pending  (5..11: MODE 1/2) */   \
    X(int, wsum, (nwave) + 1)                                                                                               \
    X(unsigned char, tie, nal)
// The image of a task: its state, or the (height, ia, ib) sort of the finished merges that reuses the same memory (16 B per entry).
// This is the image stride, the image copy length and, through max(., HR_LDS_CU), the dynamic-LDS request.
inline size_t hr_image_bytes(int max_n) {
    const int nal = (max_n + 3) & ~3;
    size_t lds_bytes = 0;
    HR_STATE_ARRAYS(LDS_COUNT, nal, 1024 / 64)                  // (slack: wsum of the sixteen-wave form also where the eight-wave form runs)
    const size_t slack = 64;                                    // unused
    return std::max((lds_bytes + slack + 15) / 16 * 16, static_cast<size_t>(hc_npow2(max_n - 1)) * 16);
}

// cutree_kernel
#define CUTREE_ARRAYS(X, n)                                                                                                 \
    X(int, absorbed, n)               /* merge step at which i stops being a representative */                              \
    X(int, wsum, HC_THREADS / 64 + 1)                                                                                       \
    X(uint16_t, parent, n)            /* (n <= kHcMaxN < 65536) */                                                          \
    X(uint16_t, rank, n)
inline size_t cutree_lds_bytes(int max_n) {
    size_t lds_bytes = 0;
    CUTREE_ARRAYS(LDS_COUNT, max_n)
    return lds_bytes + 16;                                      // (16: unused slack)
}

// cluster_sums_kernel: acc[SS_WAVES][kpad][64] doubles
inline size_t cluster_sums_lds_bytes(int kpad) { return static_cast<size_t>(SS_WAVES) * kpad * 64 * 8; }

// LDS of one stats workgroup: sil[npow2] (median by bitonic sort), part[ST_THREADS], and seven per-cluster arrays of kcap entries
inline size_t stats_lds_bytes(int max_n, int kcap) {
    int npow2 = 1; while (npow2 < max_n) npow2 <<= 1;
    return static_cast<size_t>(npow2) * 8 + ST_THREADS * 8 + 2 * static_cast<size_t>(kcap) * 8 + (5 * static_cast<size_t>(kcap) + 8) * 4;
}

// ml_prep_kernel (1024 threads); kf: the finest level's clusters (the host sizes the launch by kpad >= kf)
#define ML_PREP_ARRAYS(X, kf)                                                                                               \
    X(double, cn2, kf)                                                                                                      \
    X(double, ctot, kf)                                                                                                     \
    X(double, part, 1024)                                                                                                   \
    X(int, cnt, kf)
inline size_t ml_prep_lds_bytes(int kpad) {
    size_t lds_bytes = 0;
    ML_PREP_ARRAYS(LDS_COUNT, kpad)
    return lds_bytes + 64;                                      // (64: unused slack)
}

// ml_cells_kernel: one block per wave, each rounded up to 16 bytes
#define ML_CELLS_ARRAYS(X, kf)                                                                                              \
    X(double, st, kf)                 /* sum of distances to the members of cluster r (r = its smallest finest id) */       \
    X(double, sg, kf)                 /* c_i . (sum of the members' centred rows) */                                        \
    X(uint16_t, cnt, kf)                                                                                                    \
    X(uint16_t, live, kf)             /* the clusters of the current level, any order */                                    \
    X(uint16_t, pos, kf)              /* position of r in live[] */
__host__ __device__ inline size_t ml_cells_wave_bytes(int kf) {
    size_t lds_bytes = 0;
    ML_CELLS_ARRAYS(LDS_COUNT, kf)
    return (lds_bytes + 15) & ~static_cast<size_t>(15);
}
inline size_t ml_cells_lds_bytes(int kpad) { return ml_cells_wave_bytes(kpad) * ML_WAVES; }

// ml_level_kernel: the silhouettes of a level (bitonic sort) and the threads' partial sums
#define ML_LEVEL_ARRAYS(X, npow2)                                                                                           \
    X(double, sil, npow2)                                                                                                   \
    X(double, part, ST_THREADS)
inline size_t ml_level_lds_bytes(int max_n) {
    const int npow2 = hc_npow2(max_n);
    size_t lds_bytes = 0;
    ML_LEVEL_ARRAYS(LDS_COUNT, npow2)
    return lds_bytes;
}

// ---- hclust_agglo.hip ---------------------------------------------------------------------------------------------------------------
// A range of tasks on the current stream (ctx().stream): device descriptors and buffers, `metas` and `status` at the range's first task.
struct HcAggloRange {
    const HcMeta *metas;
    int tasks, max_n;
    double *D, *S0, *S1;      // the distance matrices (pristine for the bulk-synchronous kernel) and its two scratch matrices
    int *ia, *ib;
    double *height;
    int *status;              // per task: 0 = done by the bulk-synchronous kernel, else left to the sequential one
};
// Bulk-synchronous agglomeration (hclust_rnn_kernel): chooses between the one-launch forms and one round per pair of launches (`split`,
// or always beyond HR_MAXN observations).  img / remaining: scratch of the round-per-launch form, grown here since only that form needs
// it.  mid_event (optional) is recorded behind round `mid_round` of the round-per-launch form; returns whether it was recorded.
// did (optional) receives what was launched, for the plan record (sharp_hclust_batch_plan).
struct HcAggloDid {
    int form = 0;             // 1 round per launch, 2 one launch of 1024 threads, 3 one launch of 512 threads, 4 an experiment of the lab build
    int wpt = 0;              // round per launch: workgroups per task in the rebuild launches (else 0)
    int finish_at = 0;        // round per launch: the round from which one launch finishes the rest, -1 never (else 0)
};
SHARP_HC_LOCAL bool hclust_bulk_synchronous(const HcAggloRange &r, bool split, DevBuf<unsigned char> &img, DevBuf<int> &remaining,
                                            hipEvent_t mid_event, int mid_round, HcAggloDid *did = nullptr);
// Sequential NN-list agglomeration (hclust_kernel).  only_if (optional, per task of the range): tasks whose entry is 0 are skipped.
// gstate: the range's per-task state of hc_seq_state_bytes(max_n) each, for max_n > kHcLdsMaxN (else unused).
SHARP_HC_LOCAL void hclust_sequential(const HcAggloRange &r, const int *only_if, unsigned char *gstate);

// ---- hclust_stats.hip ---------------------------------------------------------------------------------------------------------------
struct GemmTask;
struct HcStatsRange {
    const HcMeta *metas;      // at the range's first task
    int tasks, max_n, max_p, max_nk, max_kpad;
    bool any_sym;
    const GemmTask *gemm;     // the chunk's GEMM descriptors; off / cnt: the range's share by kind (setup_chunk)
    const int *off, *cnt;
    const int *ia, *ib;
    int *lab;
    double *H, *Cr, *CSt, *T, *G, *Q, *nrm, *out;
};
// the many-levels form (ml_*_kernel): the chunk is one range
struct HcManyLevels {
    const std::vector<HcMeta> *metas;         // host copies of the chunk's descriptors
    const std::vector<MlMeta> *mlmetas;
    const MlMeta *dml;                        // device copy
    long long oM;                             // entries of ia / ib in the chunk
    int ml_off, ml_cnt, mlt_off, mlt_cnt;     // GEMM descriptors of the row-major G and T
    int *r1, *r2, *cntF;
    double *cn2m, *B, *cn2F, *tot2, *S;
};
SHARP_HC_LOCAL void hclust_copy_d(const HcMeta *metas, int tasks, const double *D, double *D0);
// a5: labels for every candidate k, then the median silhouette and CH of every level (ml: the many-levels form, else nullptr)
SHARP_HC_LOCAL void hclust_level_stats(const HcStatsRange &r, const HcManyLevels *ml);
SHARP_HC_LOCAL void hclust_pack_labels(const HcMeta *metas, int tasks, const int *lab, const int *chosen, const long long *dst_off, int *dst);

// ---- hclust_select.hip --------------------------------------------------------------------------------------------------------------
SHARP_HC_LOCAL void select_level(const HcParams &prm, int n, int nk, const double *msil, const double *CH, const double *height,
                                 int &oind, int &branch, int &rc);
SHARP_HC_LOCAL double host_ch_euclid(const double *y, int n, int p, const int *cl, int g);

}  // namespace sharp
