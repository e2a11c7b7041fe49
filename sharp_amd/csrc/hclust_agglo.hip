// hclust_agglo.hip -- a4 of the batched get_opt_hclust (hclust.hip): stats::hclust on the GPU (R/get_opt_hclust.R:76-83).
// Third-party algorithm restated (not vendored by the reference): stats::hclust's Fortran NN-list agglomeration with Lance-Williams
// updates (fp64, same operation order, lowest-index tie-breaks), SURVEY.md App. A.4.  Two kernels -- the sequential NN-list form
// (hclust_kernel) and the bulk-synchronous form for the reducible methods (hclust_rnn_kernel) -- and, at the end of the file, the two
// launchers that hclust.hip's chunk pipeline calls.
#include "hclust_task.hpp"

#include <algorithm>
#include <cstdlib>

namespace sharp {

constexpr int HC_RS = 16;   // loads in flight per lane in a rescan pass

struct MinPair { double v; int i; };
__device__ __forceinline__ MinPair mp_better(MinPair a, MinPair b) {
    return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
// Wave-wide lexicographic min of (value, index) with DPP moves (no LDS traffic: a ds_bpermute butterfly costs six dependent
// LDS round trips, which was 40 % of the unloaded merge latency).  The result is valid in lane 63 and broadcast from there.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ MinPair mp_dpp_step(MinPair x) {
    const int lo = __double2loint(x.v), hi = __double2hiint(x.v);
    // lanes outside ROW_MASK (and lanes whose source is invalid) keep their own value: op(x, x) = x
    const int ylo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int yhi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    MinPair y;
    y.i = __builtin_amdgcn_update_dpp(x.i, x.i, CTRL, ROW_MASK, 0xf, false);
    y.v = __hiloint2double(yhi, ylo);
    return mp_better(x, y);
}
__device__ __forceinline__ MinPair mp_wave(MinPair x) {
    x = mp_dpp_step<0xB1, 0xf>(x);     // quad_perm [1,0,3,2]
    x = mp_dpp_step<0x4E, 0xf>(x);     // quad_perm [2,3,0,1]
    x = mp_dpp_step<0x141, 0xf>(x);    // row_half_mirror
    x = mp_dpp_step<0x140, 0xf>(x);    // row_mirror: every lane of a 16-lane row holds the row's result
    x = mp_dpp_step<0x142, 0xa>(x);    // row_bcast15 into rows 1 and 3
    x = mp_dpp_step<0x143, 0xc>(x);    // row_bcast31 into rows 2 and 3: lane 63 holds the wave's result
    MinPair r;
    r.i = __builtin_amdgcn_readlane(x.i, 63);
    r.v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x.v), 63), __builtin_amdgcn_readlane(__double2loint(x.v), 63));
    return r;
}
// block-wide min; pv/pi: LDS scratch [32]; every thread returns the result.  The caller must have a
// barrier between two uses of the same scratch (there always is one in the merge loop).
__device__ __forceinline__ MinPair mp_block(MinPair x, double *pv, int *pi) {
    x = mp_wave(x);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { pv[w] = x.v; pi[w] = x.i; }
    __syncthreads();
    MinPair r; r.v = pv[0]; r.i = pi[0];
    const int nw = blockDim.x >> 6;
    for (int q = 1; q < nw; ++q) { MinPair y; y.v = pv[q]; y.i = pi[q]; r = mp_better(r, y); }
    return r;
}

__device__ __forceinline__ double lance_williams(int method, double d1, double d2, double d12, double mi, double mj, double mk) {
    switch (method) {
        case 1: case 8: {   // ward.D / ward.D2 (squared input)
            double dn = (mi + mk) * d1 + (mj + mk) * d2 - mk * d12;
            return dn / (mi + mj + mk);
        }
        case 2: return d1 < d2 ? d1 : d2;
        case 3: return d1 > d2 ? d1 : d2;
        case 4: return (mi * d1 + mj * d2) / (mi + mj);
        case 5: return (d1 + d2) / 2;
        case 6: return ((d1 + d2) - d12 / 2) / 2;
        default: return (mi * d1 + mj * d2 - mi * mj * d12 / (mi + mj)) / (mi + mj);
    }
}

// ---------------------------------------------------------------------------------------------
// a4: agglomeration.  State in LDS: disnn (nearest neighbour to the right), nn, membr, flag.
// D is the full symmetric matrix in HBM (row reads coalesced; the mirrored column write is strided).
// ---------------------------------------------------------------------------------------------
// GS: the nearest-neighbour state lives in global memory (gstate, gstride bytes per task) instead of LDS: tasks of more than
// kHcLdsMaxN observations (a cross-block sMetaC over thousands of block-level clusters).  Same code, same order of operations; the
// workgroup barriers order the global accesses as they order the LDS ones (all waves of a workgroup share the CU's L1).
template <bool GS>
__global__ __launch_bounds__(HC_THREADS) void hclust_kernel(const HcMeta *__restrict__ metas, double *__restrict__ Dall,
                                                            int *__restrict__ ia_all, int *__restrict__ ib_all,
                                                            double *__restrict__ h_all, int ablate, long long *__restrict__ dbg,
                                                            const int *__restrict__ only_if, unsigned char *gstate, long long gstride) {
    if (only_if && only_if[blockIdx.x] == 0) return;      // the bulk-synchronous kernel already did this task
    const HcMeta M = metas[blockIdx.x];
    const int n = M.n, nld = M.nld, method = M.method;
    double *D = Dall + M.oD;
    int *ia = ia_all + M.oM, *ib = ib_all + M.oM;
    double *crit = h_all + M.oM;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
    unsigned char *const sm = GS ? gstate + static_cast<long long>(blockIdx.x) * gstride : sm_lds;
    const int nal = (n + 1) & ~1;
    unsigned char *lds_cursor = sm;
    HC_SEQ_STATE_ARRAYS(LDS_CARVE, n, nal)                     // declares disnn, pv, nn, membr, list, pi, cnt, flag (hclust_task.hpp)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = HC_THREADS / 64;

    if (method == 8) {
        for (long long q = tid; q < static_cast<long long>(n) * nld; q += HC_THREADS) {
            const int r = static_cast<int>(q / nld), c = static_cast<int>(q % nld);
            if (c < n) { const double d = D[static_cast<long long>(r) * nld + c]; D[static_cast<long long>(r) * nld + c] = d * d; }
        }
    }
    for (int i = tid; i < n; i += HC_THREADS) { flag[i] = 1; membr[i] = 1; nn[i] = 0; disnn[i] = HC_INF; }
    __syncthreads();
    // initial NN list: nearest neighbour to the RIGHT of i, lowest j on ties
    for (int i = wave; i < n - 1; i += nwave) {
        const double *row = D + static_cast<long long>(i) * nld;
        MinPair b; b.v = HC_INF; b.i = 0x7fffffff;
        for (int j = i + 1 + lane; j < n; j += 64) { MinPair c; c.v = row[j]; c.i = j; if (c.v < b.v) b = c; }
        b = mp_wave(b);
        if (lane == 0) { nn[i] = b.i; disnn[i] = b.v; }
    }
    __syncthreads();

    // Four workgroup barriers per merge: the two block reductions use alternating scratch so that no
    // "scratch is free again" barrier is needed, the merged pair's bookkeeping is done by the thread that
    // owns index i2 right before it looks at its own entries, and d(i2,j2) is the NN distance just found.
    HC_SEQ_SCRATCH_ARRAYS(LDS_CARVE, n)                        // declares pvB, piB
    long long tacc[6] = {0, 0, 0, 0, 0, 0};
    for (int step = 0; step < n - 1; ++step) {
        const long long tt0 = dbg ? __builtin_readcyclecounter() : 0;
        // (1) least dissimilarity over the NN list (strict <, lowest index)
        MinPair b; b.v = HC_INF; b.i = 0x7fffffff;
        for (int i = tid; i < n - 1; i += HC_THREADS)
            if (flag[i]) { MinPair c; c.v = disnn[i]; c.i = i; if (c.v < b.v) b = c; }
        b = mp_block(b, pv, pi);
        const long long tt1 = dbg ? __builtin_readcyclecounter() : 0;
        const int i2 = b.i < n ? b.i : 0;       // NN lists look to the right, so im < nn[im]
        const int j2 = nn[i2];
        const double d12 = b.v;                  // DISNN(im) == D(im, NN(im)) is an invariant of the algorithm
        const double mi = membr[i2], mj = membr[j2];
        if (tid == 0) {
            ia[step] = i2 + 1; ib[step] = j2 + 1;
            crit[step] = method == 8 ? sqrt(b.v) : b.v;
            *cnt = 0;
        }
        // (2) Lance-Williams update of row/column i2; new NN of i2 among k > i2
        MinPair nb; nb.v = HC_INF; nb.i = 0x7fffffff;
        const double *ri = D + static_cast<long long>(i2) * nld, *rj = D + static_cast<long long>(j2) * nld;
        // loads are issued unconditionally and in batches: a load under a data-dependent branch would make
        // every iteration a separate dependent HBM round trip
        for (int k0 = tid; k0 < n; k0 += 4 * HC_THREADS) {
            double a1[4], a2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + u * HC_THREADS;
                const int kk = k < n ? k : n - 1;
                a1[u] = ri[kk]; a2[u] = rj[kk];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + u * HC_THREADS;
                if (k < n && k != i2 && k != j2 && flag[k]) {
                    const double dn = lance_williams(method, a1[u], a2[u], d12, mi, mj, static_cast<double>(membr[k]));
                    D[static_cast<long long>(i2) * nld + k] = dn;
                    if (!(ablate & 1)) D[static_cast<long long>(k) * nld + i2] = dn;
                    if (i2 < k) { if (dn < nb.v) { nb.v = dn; nb.i = k; } }
                    else if (dn < disnn[k]) { disnn[k] = dn; nn[k] = i2; }
                }
            }
        }
        const long long tt2 = dbg ? __builtin_readcyclecounter() : 0;
        nb = mp_block(nb, pvB, piB);
        const long long tt3 = dbg ? __builtin_readcyclecounter() : 0;
        if (tid == (i2 % HC_THREADS)) {          // owner of i2: merge bookkeeping before it scans its own entries
            membr[i2] = membr[i2] + membr[j2];
            disnn[i2] = nb.v;
            if (nb.i < n) nn[i2] = nb.i;
        }
        if (tid == (j2 % HC_THREADS)) flag[j2] = 0;
        // (3) rows whose nearest neighbour was i2 or j2 look again to their right
        for (int i = tid; i < n - 1; i += HC_THREADS)
            if (i != j2 && flag[i] && (nn[i] == i2 || nn[i] == j2)) list[atomicAdd(cnt, 1)] = i;
        __syncthreads();
        const long long tt4 = dbg ? __builtin_readcyclecounter() : 0;
        const int nl = (ablate & 2) ? 0 : *cnt;
        for (int q = wave; q < nl; q += nwave) {
            const int i = list[q];
            const double *row = D + static_cast<long long>(i) * nld;
            MinPair c; c.v = HC_INF; c.i = 0x7fffffff;
            for (int j0 = i + 1 + lane; j0 < n; j0 += 64 * HC_RS) {   // one pass (one HBM round trip) covers 2048 entries
                double v[HC_RS];
#pragma unroll
                for (int u = 0; u < HC_RS; ++u) { const int j = j0 + 64 * u; v[u] = row[j < n ? j : n - 1]; }
#pragma unroll
                for (int u = 0; u < HC_RS; ++u) {
                    const int j = j0 + 64 * u;
                    if (j < n && flag[j] && v[u] < c.v) { c.v = v[u]; c.i = j; }
                }
            }
            c = mp_wave(c);
            if (lane == 0) { disnn[i] = c.v; if (c.i < n) nn[i] = c.i; }
        }
        const long long tt5 = dbg ? __builtin_readcyclecounter() : 0;
        __syncthreads();
        if (dbg) { const long long tt6 = __builtin_readcyclecounter(); tacc[0] += tt1 - tt0; tacc[1] += tt2 - tt1; tacc[2] += tt3 - tt2; tacc[3] += tt4 - tt3; tacc[4] += tt5 - tt4; tacc[5] += tt6 - tt5; }
    }
    if (dbg && tid == 0) for (int q = 0; q < 6; ++q) dbg[blockIdx.x * 6 + q] = tacc[q];
}

// ---------------------------------------------------------------------------------------------
// a4, bulk-synchronous form for the reducible methods (ward.D, ward.D2, single, complete, average, mcquitty).
// For a reducible Lance-Williams update, merging a reciprocal-nearest-neighbour (RNN) pair never brings anything closer to
// any other cluster than that cluster's current nearest neighbour, so every RNN pair of the current matrix is a merge of
// the sequential algorithm, at the same height.  A round therefore (1) pairs up all RNN pairs, (2) ranks them by
// (height, lowest index) -- the order in which the sequential algorithm would perform them -- and (3) writes the next
// distance matrix compacted to the survivors, one wave per new row, reading whole old rows and writing whole new rows:
// pure streaming instead of one scattered 8-byte column write per (merge, cluster).  The nearest neighbour of every new
// row falls out of the same pass.  Entries between two clusters merged in the same round apply the two updates in rank
// order, exactly the arithmetic of the sequential algorithm; across rounds the association order can differ from the
// sequential one, so heights agree to rounding (1e-15), not bit for bit.  The merges are sorted by (height, index) at the
// end.  Any exact tie for a row minimum (or a round without a pair) abandons the task: status = 1, and the host runs
// hclust_kernel on it (R breaks ties by index order inside its nearest-neighbour lists; that is only restated there).
// D is left untouched; the rounds ping-pong between two scratch matrices.
// ---------------------------------------------------------------------------------------------
constexpr uint16_t HR_NONE = 0xffffu;

struct HrBest { double v; int i; int tie; };
__device__ __forceinline__ HrBest hr_combine(HrBest x, HrBest y) {
    HrBest r;
    if (y.v < x.v) r = y; else if (x.v < y.v) r = x;
    else { r.v = x.v; r.i = x.i < y.i ? x.i : y.i; r.tie = (x.i != y.i && x.i < 0x7fffffff && y.i < 0x7fffffff) ? 1 : (x.tie | y.tie); }
    return r;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ HrBest hr_dpp_step(HrBest x) {
    const int lo = __double2loint(x.v), hi = __double2hiint(x.v);
    HrBest y;
    y.v = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false),
                           __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false));
    y.i = __builtin_amdgcn_update_dpp(x.i, x.i, CTRL, ROW_MASK, 0xf, false);
    y.tie = __builtin_amdgcn_update_dpp(x.tie, x.tie, CTRL, ROW_MASK, 0xf, false);
    return hr_combine(x, y);
}
__device__ __forceinline__ HrBest hr_wave(HrBest x) {
    x = hr_dpp_step<0xB1, 0xf>(x);
    x = hr_dpp_step<0x4E, 0xf>(x);
    x = hr_dpp_step<0x141, 0xf>(x);
    x = hr_dpp_step<0x140, 0xf>(x);
    x = hr_dpp_step<0x142, 0xa>(x);
    x = hr_dpp_step<0x143, 0xc>(x);
    HrBest r;
    r.i = __builtin_amdgcn_readlane(x.i, 63);
    r.tie = __builtin_amdgcn_readlane(x.tie, 63);
    r.v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x.v), 63), __builtin_amdgcn_readlane(__double2loint(x.v), 63));
    return r;
}

// the same over the 16 lanes of a DPP row: every lane of the row ends with the row's result
__device__ __forceinline__ HrBest hr_row16(HrBest x) {
    x = hr_dpp_step<0xB1, 0xf>(x);
    x = hr_dpp_step<0x4E, 0xf>(x);
    x = hr_dpp_step<0x141, 0xf>(x);
    x = hr_dpp_step<0x140, 0xf>(x);
    return x;
}
template <int CTRL>
__device__ __forceinline__ double hr_min_step(double x) {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    return fmin(x, __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false)));
}
__device__ __forceinline__ double hr_min16(double x) {
    x = hr_min_step<0xB1>(x);
    x = hr_min_step<0x4E>(x);
    x = hr_min_step<0x141>(x);
    x = hr_min_step<0x140>(x);
    return x;
}

// HR_THREADS = 512: two tasks per CU (LDS state 37 B per observation, <= 128 VGPRs) when there are more tasks than CUs;
// 1024: one task per CU with twice the loads in flight when there are not (a task streams ~300 MB through ONE workgroup).
// MODE 0: the whole agglomeration in one launch, one workgroup per task.
// MODE 1 / 2: one ROUND per pair of launches, so that a task is no longer confined to the ~34 GB/s one CU can move: the
// LDS state lives as an image in global memory between launches; MODE 1 (one workgroup per task) loads it, applies the
// previous round's transition, finds and ranks the reciprocal pairs, builds the column maps and stores it back; MODE 2
// (gridDim.y workgroups per task) loads it read-only and rebuilds its share of the rows (work is handed out by counters in
// the image), writing the new rows' nearest neighbours straight into the image.
// MODE 3: picks a task up from its image and runs ALL its remaining rounds in this one launch (one workgroup per task, like MODE 0):
// once a few hundred clusters are left a round's two launches cost more than its work -- the last ~33 of the 45 rounds of a
// 2000-observation task took 3.3 ms as 66 launches.
// GS (MODE 1 / 2 / 3 only): tasks beyond HR_MAXN observations, whose state does not fit a CU's LDS -- the state arrays ARE the global
// image (no copy in or out; the same code addresses them), only the stage of the rebuild stays in LDS.
typedef __attribute__((address_space(1))) const double *hr_gcd;   // the distance matrices, in the global address space
typedef __attribute__((address_space(1))) double *hr_gd;
template <int HR_THREADS, int MODE, bool GS = false>
__global__ __launch_bounds__(HR_THREADS) void hclust_rnn_kernel(const HcMeta *__restrict__ metas, const double *__restrict__ Dall,
                                                                double *__restrict__ S0all, double *__restrict__ S1all,
                                                                int *__restrict__ ia_all, int *__restrict__ ib_all,
                                                                double *__restrict__ h_all, int *__restrict__ status,
                                                                unsigned char *__restrict__ images, long long image_stride,
                                                                int lds_bytes, int round, int *__restrict__ remaining, int lds_launch) {
    const HcMeta M = metas[blockIdx.x];
    const int n = M.n, nld = M.nld, method = M.method;
    // (global address space spelled out: left generic, every access of the matrices compiled to a FLAT instruction, which takes an LDS issue slot
    // as well and counts on lgkmcnt -- each wait for the column map in LDS then also waited for the 16 row loads in flight)
    const hr_gcd D = (hr_gcd)(Dall + M.oD);
    const hr_gd Sb[2] = {(hr_gd)(S0all + M.oD), (hr_gd)(S1all + M.oD)};
    int *ia = ia_all + M.oM, *ib = ib_all + M.oM;
    double *crit = h_all + M.oM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = HR_THREADS / 64;
    unsigned char *img = MODE ? images + static_cast<long long>(blockIdx.x) * image_stride : nullptr;
    if (method == 6 || method == 7 || n > (GS ? kHcMaxN : HR_MAXN)) {   // centroid / median are not reducible; large n: LDS
        if (MODE != 2 && (MODE == 0 || round == 0) && tid == 0) { status[blockIdx.x] = 1; if (MODE == 1) atomicSub(remaining, 1); }
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
    unsigned char *const sm = GS ? img : sm_lds;               // where the state arrays live
    const int nal = (n + 3) & ~3;
    unsigned char *lds_cursor = sm;
    // declares dnnA, cidA, cszA, nn, partner, pseq, oldidx, newidx, plist, colmap, ctl, wsum, tie (hclust_task.hpp says what each holds)
    HR_STATE_ARRAYS(LDS_CARVE, nal, nwave)
    // what is left of the workgroup's LDS stages the pair members' entries of the rows being copied (see the rebuild below)
    const int stage_off = GS ? 0 : static_cast<int>((lds_cursor - sm + 15) & ~static_cast<long>(15));
    double *stage = reinterpret_cast<double *>(sm_lds + stage_off);
    const int stage_pairs = lds_launch > stage_off ? (lds_launch - stage_off) / (nwave * 32) : 0;   // 2 rows x 2 members x 8 B per pair and wave

    int cur = 0, na = n, done = 0;
    int src = -1;                                               // -1: D (pristine), else scratch index
    const bool fresh = MODE == 0 || (MODE == 1 && round == 0);
    if (!fresh) {                                               // the state image of the previous launches
        if (!GS) {
            const uint4 *gi = reinterpret_cast<const uint4 *>(img);
            uint4 *li = reinterpret_cast<uint4 *>(sm);
            for (int q = tid; q < lds_bytes / 16; q += HR_THREADS) li[q] = gi[q];
            __syncthreads();
        }
        if (ctl[10] != 0 || (MODE == 2 && !ctl[11])) return;   // finished / abandoned, or nothing pending
        cur = ctl[5]; na = ctl[6]; done = ctl[7]; src = ctl[8] - 1;
        if ((MODE == 1 || MODE == 3) && ctl[11]) {              // apply the transition of the round that MODE 2 just rebuilt
            done += ctl[0]; na = ctl[9]; cur ^= 1; src = src < 0 ? 0 : (src ^ 1);
            __syncthreads();
            if (tid == 0) { ctl[0] = 0; ctl[11] = 0; }
            __syncthreads();
        }
    }
    if (fresh) {
    for (int i = tid; i < n; i += HR_THREADS) { cidA[i] = static_cast<uint16_t>(i); cszA[i] = 1; }
    if (tid == 0) { for (int q = 0; q < 16; ++q) ctl[q] = 0; }
    __syncthreads();
    // round 0 nearest neighbours.  With the row minima the distance GEMM left per 128-column tile (HcMeta::nn, already squared for ward.D2): a row's
    // minimum is the smallest of its tiles' minima, and only the tile(s) that hold it are scanned for the lowest column and a second one (tie) --
    // 1 KB per row instead of 16 KB.  Sixteen lanes per row, four rows per wave.
    if (M.nn) {
        const int slots = nld / 128;                            // <= 16 (setup_chunk)
        const int g = lane >> 4, l = lane & 15;
        for (int a0 = wave * 4; a0 < n; a0 += nwave * 4) {
            const int a = a0 + g < n ? a0 + g : n - 1;          // (a group beyond the last row repeats it and stores nothing)
            const double pm = l < slots ? M.nn[static_cast<long long>(l) * nld + a] : HC_INF;
            const double m = hr_min16(pm);
            unsigned cand = static_cast<unsigned>(__ballot(l < slots && pm == m) >> (16 * g)) & 0xffffu;   // this row's tiles that hold its minimum
            const hr_gcd row = D + static_cast<long long>(a) * nld;
            HrBest b; b.v = HC_INF; b.i = 0x7fffffff; b.tie = 0;
            while (__any(cand != 0u)) {
                if (cand) {
                    const int j0 = (__ffs(cand) - 1) * 128 + l;
                    cand &= cand - 1;
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int j = j0 + 16 * u; v[u] = row[j < n ? j : n - 1]; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int j = j0 + 16 * u;
                        if (j < n && j != a) {
                            const double x = method == 8 ? v[u] * v[u] : v[u];
                            if (x < b.v) { b.v = x; b.i = j; b.tie = 0; } else if (x == b.v) b.tie = 1;
                        }
                    }
                }
            }
            b = hr_row16(b);
            if (l == 0 && a0 + g < n) { nn[a] = static_cast<uint16_t>(b.i < n ? b.i : 0); dnnA[a] = b.v; tie[a] = static_cast<unsigned char>(b.tie); }
        }
    } else
    // ... or from the pristine matrix (squared for ward.D2)
    for (int a = wave; a < n; a += nwave) {
        const hr_gcd row = D + static_cast<long long>(a) * nld;
        HrBest b; b.v = HC_INF; b.i = 0x7fffffff; b.tie = 0;
        for (int j0 = lane; j0 < n; j0 += 64 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int j = j0 + 64 * u; v[u] = row[j < n ? j : n - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + 64 * u;
                if (j < n && j != a) {
                    const double x = method == 8 ? v[u] * v[u] : v[u];
                    if (x < b.v) { b.v = x; b.i = j; b.tie = 0; } else if (x == b.v) b.tie = 1;
                }
            }
        }
        b = hr_wave(b);
        if (lane == 0) { nn[a] = static_cast<uint16_t>(b.i < n ? b.i : 0); dnnA[a] = b.v; tie[a] = static_cast<unsigned char>(b.tie); }
    }
    __syncthreads();
    }   // fresh

    // where the results of a rebuilt row go: the LDS arrays (MODE 0) or the global image (MODE 2)
    auto outp = [&](auto *lds_ptr) { return (MODE == 2 && !GS) ? reinterpret_cast<decltype(lds_ptr)>(img + (reinterpret_cast<unsigned char *>(lds_ptr) - sm)) : lds_ptr; };
    int *wctl = outp(ctl);
    auto store_image = [&]() {
        __syncthreads();
        if (GS) return;
        uint4 *gi = reinterpret_cast<uint4 *>(img);
        const uint4 *li = reinterpret_cast<const uint4 *>(sm);
        for (int q = tid; q < lds_bytes / 16; q += HR_THREADS) gi[q] = li[q];
    };
#ifdef HR_TIMING
    long long hr_acc_setup = 0, hr_acc_rebuild = 0, hr_acc_barrier = 0, hr_acc_entries = 0, hr_acc_wave_busy = 0;
    int hr_rounds = 0;
    const long long hr_start = __builtin_readcyclecounter();
#endif
    while (na > 1) {
        double *dnn = dnnA + cur * nal;
        uint16_t *cid = cidA + cur * nal, *csz = cszA + cur * nal;
        double *dnnN = outp(dnnA + (cur ^ 1) * nal);
        uint16_t *cidN = outp(cidA + (cur ^ 1) * nal), *cszN = outp(cszA + (cur ^ 1) * nal);
        uint16_t *nnW = outp(nn);
        unsigned char *tieW = outp(tie);
        int np = 0, nb = 0, ns = 0;
#ifdef HR_TIMING
        const long long hr_t0 = __builtin_readcyclecounter();
#endif
        if (MODE != 2) {
        // (1) reciprocal pairs
        for (int a = tid; a < na; a += HR_THREADS) {
            partner[a] = HR_NONE;
            if (tie[a]) ctl[1] = 1;
#ifdef HR_ROUNDS
            if (tie[a] && blockIdx.x == 0) printf("tie at row %d of %d (done %d): nn %d dnn %.17g\n", a, na, done, (int)nn[a], dnn[a]);
#endif
        }
        __syncthreads();
        for (int a = tid; a < na; a += HR_THREADS) {
            const int b = nn[a];
            if (b > a && nn[b] == a) {
                partner[a] = static_cast<uint16_t>(b); partner[b] = static_cast<uint16_t>(a);
                plist[atomicAdd(&ctl[0], 1)] = static_cast<uint16_t>(a);
            }
        }
        __syncthreads();
        np = ctl[0];
        if (ctl[1] || np == 0) {                                // tie or no pair: the sequential kernel takes this task
            if (tid == 0) {
                status[blockIdx.x] = 1;
                if (MODE == 1) { reinterpret_cast<int *>(img + (reinterpret_cast<unsigned char *>(ctl) - sm))[10] = 1; atomicSub(remaining, 1); }
            }
            return;
        }
        // (2) rank of each pair by (height, lower original index) = the sequential algorithm's order
        for (int q = tid; q < np; q += HR_THREADS) {
            const int a = plist[q];
            const double h = dnn[a];
            const int ida = cid[a] < cid[partner[a]] ? cid[a] : cid[partner[a]];
            int rank = 0;
            for (int q2 = 0; q2 < np; ++q2) {
                const int a2 = plist[q2];
                const double h2 = dnn[a2];
                const int id2 = cid[a2] < cid[partner[a2]] ? cid[a2] : cid[partner[a2]];
                rank += (h2 < h || (h2 == h && id2 < ida)) ? 1 : 0;
            }
            pseq[a] = static_cast<uint16_t>(rank); pseq[partner[a]] = static_cast<uint16_t>(rank);
            const int ib_ = cid[a] < cid[partner[a]] ? cid[partner[a]] : cid[a];
            ia[done + rank] = ida + 1; ib[done + rank] = ib_ + 1;
            crit[done + rank] = h;                               // squared for ward.D2 until the final pass
        }
        // (3) new indices: the unmerged clusters keep their relative order in [0, ns), the merged clusters follow in rank order in
        // [ns, nb).  Every new row is then written as two dense runs of stores.  (With the merged clusters left in place, each
        // plain row was stored with a hole per merged column, filled later by a scattered 8-byte store: partial-line writes that
        // cost the HBM 57 % more reads and 34 % more writes than the algorithm needs -- FETCH_SIZE / WRITE_SIZE)
        // Exact ties abandon the task, so the order of the columns decides nothing.
        {
            const int chunk = (na + HR_THREADS - 1) / HR_THREADS;
            const int lo = tid * chunk, hi = lo + chunk < na ? lo + chunk : na;
            int c = 0;
            for (int a = lo; a < hi; ++a) c += partner[a] == HR_NONE ? 1 : 0;
            int incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); incl += lane >= d ? t : 0; }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            if (tid == 0) { int run = 0; for (int w = 0; w < nwave; ++w) { const int t = wsum[w]; wsum[w] = run; run += t; } wsum[nwave] = run; }
            __syncthreads();
            int pos = wsum[wave] + incl - c;
            for (int a = lo; a < hi; ++a)
                if (partner[a] == HR_NONE) { newidx[a] = static_cast<uint16_t>(pos); colmap[a] = static_cast<uint16_t>(pos); oldidx[pos++] = static_cast<uint16_t>(a); }
            ns = wsum[nwave];                                   // rows of unmerged clusters (= na - 2 np)
            for (int q = tid; q < np; q += HR_THREADS) {        // bit 15 of oldidx: the survivor is a merged cluster
                const int a = plist[q], B = ns + pseq[a];
                newidx[a] = static_cast<uint16_t>(B);
                oldidx[B] = static_cast<uint16_t>(a | 0x8000);
                colmap[a] = static_cast<uint16_t>(0x8000 | (2 * pseq[a]));
                colmap[partner[a]] = static_cast<uint16_t>(0x8000 | (2 * pseq[a] + 1));
            }
        }
        nb = ns + np;
        if (tid == 0) { ctl[2] = 0; ctl[3] = 0; ctl[4] = ns; }
        __syncthreads();
        }   // MODE != 2
        if (MODE == 1) {                                        // hand the round over to the rebuild launch
            __syncthreads();
            if (tid == 0) { ctl[5] = cur; ctl[6] = na; ctl[7] = done; ctl[8] = src + 1; ctl[9] = nb; ctl[10] = 0; ctl[11] = 1; }
            store_image();
            return;
        }
        if (MODE == 2) { np = ctl[0]; nb = ctl[9]; ns = ctl[4]; }
#ifdef HR_TIMING
        const long long hr_t1 = __builtin_readcyclecounter();
        long long hr_dual = 0, hr_slow = 0;
#endif
        // (4) next matrix, one wave per new row; nearest neighbour of the new row on the fly.
        // Rows of unmerged clusters (~90 %) are a gathered copy of the old row (eight loads in flight per lane) plus one
        // Lance-Williams value per merged column; rows of merged clusters take the general path.
        const hr_gcd Dsrc = src < 0 ? D : (hr_gcd)Sb[src];
        const hr_gd Ddst = Sb[src < 0 ? 0 : (src ^ 1)];
        const bool sq = (src < 0 && method == 8);
        auto do_row = [&](int A) {
            const int a = oldidx[A] & 0x7fff;
            const int pa = partner[a];                          // NONE or j > a
            const bool am = pa != HR_NONE;
            const hr_gcd ra = Dsrc + static_cast<long long>(a) * nld;
            const hr_gd wr = Ddst + static_cast<long long>(A) * nld;
            const double na_ = csz[a];
            HrBest best; best.v = HC_INF; best.i = 0x7fffffff; best.tie = 0;
            auto consider = [&](double v, int B) {
                if (v < best.v || (v == best.v && B < best.i)) { best.tie = (v == best.v) ? 1 : 0; best.v = v; best.i = B; }
                else if (v == best.v && B != best.i) best.tie = 1;
            };
            if (!am) {
                for (int B0 = lane; B0 < ns; B0 += 64 * 8) {   // columns of unmerged clusters
                    int bb[8];
                    double x[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int B = B0 + 64 * u;
                        bb[u] = oldidx[B < ns ? B : ns - 1];
                        x[u] = ra[bb[u]];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int B = B0 + 64 * u;
                        if (B < ns) {
                            const double v = B == A ? HC_INF : (sq ? x[u] * x[u] : x[u]);   // scratch diagonals hold +inf: no test in later rounds
                            wr[B] = v;
                            if (B != A) consider(v, B);
                        }
                    }
                }
                for (int B = ns + lane; B < nb; B += 64) {      // merged columns: d(a, k u l) from d(a,k), d(a,l)
                    const int k1 = oldidx[B] & 0x7fff, l1 = partner[k1];
                    double d1 = ra[k1], d2 = ra[l1];
                    if (sq) { d1 *= d1; d2 *= d2; }
                    const double v = lance_williams(method, d1, d2, dnn[k1], static_cast<double>(csz[k1]), static_cast<double>(csz[l1]), na_);
                    wr[B] = v;
                    consider(v, B);
                }
            } else {
                const hr_gcd rj = Dsrc + static_cast<long long>(pa) * nld;
                const double hP = dnn[a];
                const double nj_ = csz[pa];
                const int seqP = pseq[a];
                for (int B0 = lane; B0 < nb; B0 += 64 * 4) {
                    int bb[4], pbv[4];
                    double x00[4], x01[4], x10[4], x11[4];      // D[a][b], D[a][pb], D[j][b], D[j][pb]
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int B = B0 + 64 * u;
                        bb[u] = oldidx[B < nb ? B : nb - 1] & 0x7fff;
                        const int pb = partner[bb[u]];
                        pbv[u] = pb;
                        const int pbc = pb == HR_NONE ? bb[u] : pb;
                        x00[u] = ra[bb[u]]; x01[u] = ra[pbc]; x10[u] = rj[bb[u]]; x11[u] = rj[pbc];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int B = B0 + 64 * u;
                        if (B < nb) {
                            const int b = bb[u];
                            const bool bm = pbv[u] != HR_NONE;
                            double d00 = x00[u], d01 = x01[u], d10 = x10[u], d11 = x11[u];
                            if (sq) { d00 *= d00; d01 *= d01; d10 *= d10; d11 *= d11; }
                            double v;
                            if (B == A) v = HC_INF;
                            else if (!bm) v = lance_williams(method, d00, d10, hP, na_, nj_, static_cast<double>(csz[b]));
                            else {
                                const double nk_ = csz[b], nl_ = csz[pbv[u]], hQ = dnn[b];
                                if (seqP < static_cast<int>(pseq[b])) {   // (a, j) merges first, then (b, l) against the merged cluster
                                    const double t1 = lance_williams(method, d00, d10, hP, na_, nj_, nk_);
                                    const double t2 = lance_williams(method, d01, d11, hP, na_, nj_, nl_);
                                    v = lance_williams(method, t1, t2, hQ, nk_, nl_, na_ + nj_);
                                } else {
                                    const double t1 = lance_williams(method, d00, d01, hQ, nk_, nl_, na_);
                                    const double t2 = lance_williams(method, d10, d11, hQ, nk_, nl_, nj_);
                                    v = lance_williams(method, t1, t2, hP, na_, nj_, nk_ + nl_);
                                }
                            }
                            wr[B] = v;
                            if (B != A) consider(v, B);
                        }
                    }
                }
            }
            best = hr_wave(best);
            if (lane == 0) {
                // the merged cluster keeps the smaller original index as its name (R: i2 < j2)
                cidN[A] = am ? (cid[a] < cid[pa] ? cid[a] : cid[pa]) : cid[a];
                cszN[A] = static_cast<uint16_t>(csz[a] + (am ? csz[pa] : 0));
                dnnN[A] = best.v;
            }
            // nn / tie of the new round live in the single-buffered arrays: nothing reads the old ones in this phase
            if (lane == 1) { nnW[A] = static_cast<uint16_t>(best.i < nb ? best.i : 0); }
            if (lane == 2) { tieW[A] = static_cast<unsigned char>(nb > 2 ? best.tie : 0); }
        };
        // two unmerged rows at a time share the column map (one set of LDS reads) and keep 16 loads in flight per lane
        auto finish_row = [&](int A, int a, HrBest best) {
            best = hr_wave(best);
            if (lane == 0) { cidN[A] = cid[a]; cszN[A] = csz[a]; dnnN[A] = best.v; }
            if (lane == 1) { nnW[A] = static_cast<uint16_t>(best.i < nb ? best.i : 0); }
            if (lane == 2) { tieW[A] = static_cast<unsigned char>(nb > 2 ? best.tie : 0); }
        };
#ifdef HR_NO_FIRST_STAGE
        const int stage_rows = src < 0 ? 0 : (np == 0 ? 2 : std::min(2, 2 * stage_pairs / np));
#else
        const int stage_rows = np == 0 ? 2 : std::min(2, 2 * stage_pairs / np);   // rows per wave whose pair entries fit the stage
#endif
        // Plain rows, staged form.  The old rows are read ONCE, contiguously (the gathered forms further down skip the pair members'
        // entries and come back for them after the sweep, by which time the lines have left the L2: the L2's request-size counters
        // showed every row fetched twice, 12.1 n^2 entries per task instead of 6.05).  An entry of an unmerged column goes straight
        // to its new column (a dense run of stores per instruction); an entry of a pair member is parked in this wave's LDS stage,
        // from where the Lance-Williams loop takes it.  NR = 2 rows per wave when the stage holds the round's pairs twice, else 1.
        // FIRST: the source is the pristine matrix (real diagonal; squared on the fly for ward.D2).
        auto staged = [&](auto NR_, auto FIRST_, int A0) {
            constexpr int NR = decltype(NR_)::value;
            constexpr bool FIRST = decltype(FIRST_)::value;
            hr_gcd r[NR];
            hr_gd w[NR];
            double *stg[NR];
            double mn[NR], sc[NR];
            int ix[NR], ao[NR];
#pragma unroll
            for (int t = 0; t < NR; ++t) {
                ao[t] = __builtin_amdgcn_readfirstlane(oldidx[A0 + t] & 0x7fff);
                r[t] = Dsrc + static_cast<long long>(ao[t]) * nld;
                w[t] = Ddst + static_cast<long long>(A0 + t) * nld;
                stg[t] = stage + (static_cast<size_t>(wave) * stage_rows + t) * 2 * np;   // a wave's region does not depend on NR (odd last row)
                mn[t] = HC_INF; sc[t] = HC_INF; ix[t] = 0x7fffffff;
            }
            auto upd = [](double &m_, double &s_, int &i_, double v, int B) {
                s_ = fmin(s_, fmax(m_, v));
                if (v < m_) { m_ = v; i_ = B; }
            };
            int j0 = lane;
            auto pass = [&](auto U_) {
                constexpr int U = decltype(U_)::value;
                for (; j0 + 64 * (U - 1) < na; j0 += 64 * U) {
                    unsigned cm[U];
                    double x[NR][U];
#pragma unroll
                    for (int u = 0; u < U; ++u) cm[u] = colmap[j0 + 64 * u];
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int t = 0; t < NR; ++t) x[t][u] = r[t][j0 + 64 * u];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (cm[u] & 0x8000u) {
#pragma unroll
                            for (int t = 0; t < NR; ++t) stg[t][cm[u] & 0x7fffu] = (FIRST && sq) ? x[t][u] * x[t][u] : x[t][u];
                        } else {
                            const int B = static_cast<int>(cm[u]);
#pragma unroll
                            for (int t = 0; t < NR; ++t) {
                                double v = x[t][u];
                                if (FIRST) v = B == A0 + t ? HC_INF : (sq ? v * v : v);   // scratch diagonals hold +inf: no test in later rounds
                                w[t][B] = v;
                                upd(mn[t], sc[t], ix[t], v, B);
                            }
                        }
                    }
                    if (U == 1) break;
                }
            };
            if (NR == 1) pass(std::integral_constant<int, 16>());   // 16 entries per lane in flight either way (128 VGPRs, no scratch)
            pass(std::integral_constant<int, 8>());
            pass(std::integral_constant<int, 4>());
            pass(std::integral_constant<int, 2>());
            pass(std::integral_constant<int, 1>());
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double nr_[NR];
#pragma unroll
            for (int t = 0; t < NR; ++t) nr_[t] = csz[ao[t]];
            for (int B = ns + lane; B < nb; B += 64) {          // merged columns: d(a, k u l) from d(a,k), d(a,l)
                const int rk = B - ns;
                const int k1 = oldidx[B] & 0x7fff, l1 = partner[k1];
                const double nk_ = csz[k1], nl_ = csz[l1], hQ = dnn[k1];
#pragma unroll
                for (int t = 0; t < NR; ++t) {
                    const double v = lance_williams(method, stg[t][2 * rk], stg[t][2 * rk + 1], hQ, nk_, nl_, nr_[t]);
                    w[t][B] = v;
                    sc[t] = fmin(sc[t], fmax(mn[t], v));
                    if (v < mn[t] || (v == mn[t] && B < ix[t])) { mn[t] = v; ix[t] = B; }
                }
            }
            __builtin_amdgcn_wave_barrier();                     // the stage is reused by this wave's next rows
#pragma unroll
            for (int t = 0; t < NR; ++t) {
                HrBest g;
                g.v = mn[t]; g.i = ix[t]; g.tie = 0;
                g = hr_wave(g);
                g.tie |= __ballot(sc[t] == g.v) != 0ull ? 1 : 0; // a lane saw the minimum twice
                if (lane == 0) { cidN[A0 + t] = cid[ao[t]]; cszN[A0 + t] = csz[ao[t]]; dnnN[A0 + t] = g.v; }
                if (lane == 1) { nnW[A0 + t] = static_cast<uint16_t>(g.i < nb ? g.i : 0); }
                if (lane == 2) { tieW[A0 + t] = static_cast<unsigned char>(nb > 2 ? g.tie : 0); }
            }
        };
        // Rows of merged clusters, staged form (needs the two-row stage): the two old rows a and j of the pair are read once,
        // contiguously; an unmerged column gets its Lance-Williams value at once, the four entries of a merged column (a, j) x (k, l)
        // wait in the stage.  (The gathered form in do_row fetches d(a,l), d(j,l) from wherever column l lies: one more 128-byte
        // line per entry, 2.6 x the row's own bytes.)
        auto staged_merged = [&](int A) {
            const int a = __builtin_amdgcn_readfirstlane(oldidx[A] & 0x7fff);
            const int pa = __builtin_amdgcn_readfirstlane(partner[a]);
            const hr_gcd ra = Dsrc + static_cast<long long>(a) * nld, rj = Dsrc + static_cast<long long>(pa) * nld;
            const hr_gd wr = Ddst + static_cast<long long>(A) * nld;
            const double na_ = csz[a], nj_ = csz[pa], hP = dnn[a];
            const int seqP = pseq[a];
            double *sa = stage + static_cast<size_t>(wave) * 4 * np, *sj = sa + 2 * np;
            double mn = HC_INF, sc = HC_INF;
            int ix = 0x7fffffff;
            int j0 = lane;
            auto pass = [&](auto U_) {
                constexpr int U = decltype(U_)::value;
                for (; j0 + 64 * (U - 1) < na; j0 += 64 * U) {
                    unsigned cm[U];
                    double xa[U], xj[U], nc[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) { cm[u] = colmap[j0 + 64 * u]; nc[u] = csz[j0 + 64 * u]; }
#pragma unroll
                    for (int u = 0; u < U; ++u) { xa[u] = ra[j0 + 64 * u]; xj[u] = rj[j0 + 64 * u]; }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (sq) { xa[u] *= xa[u]; xj[u] *= xj[u]; }
                        if (cm[u] & 0x8000u) { sa[cm[u] & 0x7fffu] = xa[u]; sj[cm[u] & 0x7fffu] = xj[u]; }
                        else {
                            const int B = static_cast<int>(cm[u]);
                            const double v = lance_williams(method, xa[u], xj[u], hP, na_, nj_, nc[u]);
                            wr[B] = v;
                            sc = fmin(sc, fmax(mn, v));
                            if (v < mn) { mn = v; ix = B; }
                        }
                    }
                    if (U == 1) break;
                }
            };
            pass(std::integral_constant<int, 8>());
            pass(std::integral_constant<int, 4>());
            pass(std::integral_constant<int, 2>());
            pass(std::integral_constant<int, 1>());
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int B = ns + lane; B < nb; B += 64) {
                const int rk = B - ns;
                double v = HC_INF;                              // own column: the scratch diagonal
                if (B != A) {
                    const int k1 = oldidx[B] & 0x7fff, l1 = partner[k1];
                    const double d00 = sa[2 * rk], d01 = sa[2 * rk + 1], d10 = sj[2 * rk], d11 = sj[2 * rk + 1];
                    const double nk_ = csz[k1], nl_ = csz[l1], hQ = dnn[k1];
                    if (seqP < static_cast<int>(pseq[k1])) {    // (a, j) merges first, then (k, l) against the merged cluster
                        const double t1 = lance_williams(method, d00, d10, hP, na_, nj_, nk_);
                        const double t2 = lance_williams(method, d01, d11, hP, na_, nj_, nl_);
                        v = lance_williams(method, t1, t2, hQ, nk_, nl_, na_ + nj_);
                    } else {
                        const double t1 = lance_williams(method, d00, d01, hQ, nk_, nl_, na_);
                        const double t2 = lance_williams(method, d10, d11, hQ, nk_, nl_, nj_);
                        v = lance_williams(method, t1, t2, hP, na_, nj_, nk_ + nl_);
                    }
                    sc = fmin(sc, fmax(mn, v));
                    if (v < mn || (v == mn && B < ix)) { mn = v; ix = B; }
                }
                wr[B] = v;
            }
            __builtin_amdgcn_wave_barrier();
            HrBest g;
            g.v = mn; g.i = ix; g.tie = 0;
            g = hr_wave(g);
            g.tie |= __ballot(sc == g.v) != 0ull ? 1 : 0;
            if (lane == 0) { cidN[A] = cid[a] < cid[pa] ? cid[a] : cid[pa]; cszN[A] = static_cast<uint16_t>(csz[a] + csz[pa]); dnnN[A] = g.v; }
            if (lane == 1) { nnW[A] = static_cast<uint16_t>(g.i < nb ? g.i : 0); }
            if (lane == 2) { tieW[A] = static_cast<unsigned char>(nb > 2 ? g.tie : 0); }
        };
        // work is handed out dynamically (the rows of merged clusters cost about twice a pair of plain rows, and a static
        // split left a quarter of the phase waiting at the barrier): merged rows first, then plain rows two at a time
        for (;;) {
            int q = 0;
            if (lane == 0) q = atomicAdd(wctl + 3, 1);
            q = __builtin_amdgcn_readfirstlane(q);
            if (q >= np) break;
#ifdef HR_TIMING
            const long long q0 = __builtin_readcyclecounter();
#endif
            if (stage_rows == 2) staged_merged(newidx[plist[q]]); else do_row(newidx[plist[q]]);
#ifdef HR_TIMING
            hr_slow += __builtin_readcyclecounter() - q0;
#endif
        }
        if (stage_rows > 0) {
            const int step = stage_rows;
            for (;;) {
                int q = 0;
                if (lane == 0) q = atomicAdd(wctl + 2, step);
                q = __builtin_amdgcn_readfirstlane(q);
                if (q >= ns) break;
                const bool two = step == 2 && q + 1 < ns;
#ifdef HR_TIMING
                const long long q2 = __builtin_readcyclecounter();
#endif
                if (src < 0) { if (two) staged(std::integral_constant<int, 2>(), std::true_type(), q); else staged(std::integral_constant<int, 1>(), std::true_type(), q); }
                else         { if (two) staged(std::integral_constant<int, 2>(), std::false_type(), q); else staged(std::integral_constant<int, 1>(), std::false_type(), q); }
#ifdef HR_TIMING
                hr_dual += __builtin_readcyclecounter() - q2;
#endif
            }
        }
        // the gathered forms: rounds whose pairs do not fit the stage even one row at a time (large tasks with little LDS to spare)
        for (;;) {
            if (stage_rows > 0) break;
            int q = 0;
            if (lane == 0) q = atomicAdd(wctl + 2, 2);
            q = __builtin_amdgcn_readfirstlane(q);
            if (q >= ns) break;
            const int A = q;
            if (q + 1 >= ns) { do_row(A); break; }
            const int A2 = q + 1;
            const int a1 = __builtin_amdgcn_readfirstlane(oldidx[A] & 0x7fff), a2 = __builtin_amdgcn_readfirstlane(oldidx[A2] & 0x7fff);
#ifdef HR_TIMING
            const long long q1 = __builtin_readcyclecounter();
#endif
            const hr_gcd r1 = Dsrc + static_cast<long long>(a1) * nld, r2 = Dsrc + static_cast<long long>(a2) * nld;
            const hr_gd w1 = Ddst + static_cast<long long>(A) * nld, w2 = Ddst + static_cast<long long>(A2) * nld;
            if (src >= 0) {
                // Later rounds (the bulk of the work): the source is a scratch matrix whose diagonal holds +inf, so a plain
                // gathered copy needs no diagonal test; per element: one LDS read (old column | merged flag), two loads, two
                // stores and a six-instruction running (min, second min, arg min) per row -- the kernel is bound by the vector
                // ALU (53 instructions per element before this path: SQ_INSTS_VALU, tools/pmc_hclust.sh), not by memory.
                double m1 = HC_INF, s1 = HC_INF, m2 = HC_INF, s2 = HC_INF;
                int i1 = 0x7fffffff, i2 = 0x7fffffff;
                auto upd = [](double &mn, double &sc, int &ix, double v, int B) {
                    sc = fmin(sc, fmax(mn, v));
                    if (v < mn) { mn = v; ix = B; }
                };
                int B0 = lane;
                // passes of 8, 4, 2, 1 columns per lane, none with bounds tests: the waves spend most of their time parked
                // on these loads (SQ_WAIT_ANY 64 % of the wave cycles), so as many as the registers allow go out together
                auto pass = [&](auto U_) {
                    constexpr int U = decltype(U_)::value;
                    for (; B0 + 64 * (U - 1) < ns; B0 += 64 * U) {
                        unsigned mm[U];
                        double x1[U], x2[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) mm[u] = oldidx[B0 + 64 * u];
#pragma unroll
                        for (int u = 0; u < U; ++u) { x1[u] = r1[mm[u]]; x2[u] = r2[mm[u]]; }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int B = B0 + 64 * u;
                            w1[B] = x1[u]; w2[B] = x2[u];
                            upd(m1, s1, i1, x1[u], B); upd(m2, s2, i2, x2[u], B);
                        }
                        if (U == 1) break;
                    }
                };
                pass(std::integral_constant<int, 8>());
                pass(std::integral_constant<int, 4>());
                pass(std::integral_constant<int, 2>());
                pass(std::integral_constant<int, 1>());
                const double n1 = csz[a1], n2 = csz[a2];
                for (int B = ns + lane; B < nb; B += 64) {      // merged columns: d(a, k u l) from d(a,k), d(a,l)
                    const int k1 = oldidx[B] & 0x7fff, l1 = partner[k1];
                    const double nk_ = csz[k1], nl_ = csz[l1], hQ = dnn[k1];
                    const double v1 = lance_williams(method, r1[k1], r1[l1], hQ, nk_, nl_, n1);
                    const double v2 = lance_williams(method, r2[k1], r2[l1], hQ, nk_, nl_, n2);
                    w1[B] = v1; w2[B] = v2;
                    // equal values: the lower column wins, like the ascending sweep above
                    s1 = fmin(s1, fmax(m1, v1)); if (v1 < m1 || (v1 == m1 && B < i1)) { m1 = v1; i1 = B; }
                    s2 = fmin(s2, fmax(m2, v2)); if (v2 < m2 || (v2 == m2 && B < i2)) { m2 = v2; i2 = B; }
                }
                HrBest g1, g2;
                g1.v = m1; g1.i = i1; g1.tie = 0; g2.v = m2; g2.i = i2; g2.tie = 0;
                g1 = hr_wave(g1); g2 = hr_wave(g2);
                g1.tie |= __ballot(s1 == g1.v) != 0ull ? 1 : 0;     // a lane saw the minimum twice
                g2.tie |= __ballot(s2 == g2.v) != 0ull ? 1 : 0;
                if (lane == 0) { cidN[A] = cid[a1]; cszN[A] = csz[a1]; dnnN[A] = g1.v; cidN[A2] = cid[a2]; cszN[A2] = csz[a2]; dnnN[A2] = g2.v; }
                if (lane == 1) { nnW[A] = static_cast<uint16_t>(g1.i < nb ? g1.i : 0); nnW[A2] = static_cast<uint16_t>(g2.i < nb ? g2.i : 0); }
                if (lane == 2) { tieW[A] = static_cast<unsigned char>(nb > 2 ? g1.tie : 0); tieW[A2] = static_cast<unsigned char>(nb > 2 ? g2.tie : 0); }
#ifdef HR_TIMING
                hr_dual += __builtin_readcyclecounter() - q1;
#endif
                continue;
            }
            HrBest b1, b2;
            b1.v = b2.v = HC_INF; b1.i = b2.i = 0x7fffffff; b1.tie = b2.tie = 0;
            for (int B0 = lane; B0 < ns; B0 += 64 * 8) {
                int bb[8];
                double x1[8], x2[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int B = B0 + 64 * u;
                    bb[u] = oldidx[B < ns ? B : ns - 1];
                    x1[u] = r1[bb[u]]; x2[u] = r2[bb[u]];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int B = B0 + 64 * u;
                    if (B < ns) {
                        const double v1 = B == A ? HC_INF : (sq ? x1[u] * x1[u] : x1[u]);
                        const double v2 = B == A2 ? HC_INF : (sq ? x2[u] * x2[u] : x2[u]);
                        w1[B] = v1; w2[B] = v2;
                        if (B != A) { if (v1 < b1.v) { b1.v = v1; b1.i = B; b1.tie = 0; } else if (v1 == b1.v) b1.tie = 1; }
                        if (B != A2) { if (v2 < b2.v) { b2.v = v2; b2.i = B; b2.tie = 0; } else if (v2 == b2.v) b2.tie = 1; }
                    }
                }
            }
            const double n1 = csz[a1], n2 = csz[a2];
            for (int B = ns + lane; B < nb; B += 64) {          // merged columns: d(a, k u l) from d(a,k), d(a,l)
                const int k1 = oldidx[B] & 0x7fff, l1 = partner[k1];
                double d1 = r1[k1], d2 = r1[l1], e1 = r2[k1], e2 = r2[l1];
                if (sq) { d1 *= d1; d2 *= d2; e1 *= e1; e2 *= e2; }
                const double nk_ = csz[k1], nl_ = csz[l1], hQ = dnn[k1];
                const double v1 = lance_williams(method, d1, d2, hQ, nk_, nl_, n1);
                const double v2 = lance_williams(method, e1, e2, hQ, nk_, nl_, n2);
                w1[B] = v1; w2[B] = v2;
                if (v1 < b1.v || (v1 == b1.v && B < b1.i)) { b1.tie = (v1 == b1.v) ? 1 : 0; b1.v = v1; b1.i = B; } else if (v1 == b1.v && B != b1.i) b1.tie = 1;
                if (v2 < b2.v || (v2 == b2.v && B < b2.i)) { b2.tie = (v2 == b2.v) ? 1 : 0; b2.v = v2; b2.i = B; } else if (v2 == b2.v && B != b2.i) b2.tie = 1;
            }
            finish_row(A, a1, b1);
            finish_row(A2, a2, b2);
#ifdef HR_TIMING
            hr_dual += __builtin_readcyclecounter() - q1;
#endif
        }
#ifdef HR_TIMING
        const long long hr_t2 = __builtin_readcyclecounter();
#endif
        if (MODE == 2) return;                                  // the next MODE 1 launch applies the transition
        __syncthreads();
        if (tid == 0) { ctl[0] = 0; }
#ifdef HR_TIMING
        hr_acc_setup += hr_t1 - hr_t0; hr_acc_rebuild += hr_t2 - hr_t1; hr_acc_barrier += (long long)__builtin_readcyclecounter() - hr_t2;
        hr_acc_entries += static_cast<long long>(na) * na + static_cast<long long>(nb) * nb; ++hr_rounds;
        hr_acc_wave_busy += hr_dual + hr_slow;
        if (blockIdx.x == 0 && tid == 0 && (done == 0 || (na < 1200 && na > 1100) || (na < 600 && na > 560) || (na < 300 && na > 280) || (na < 100 && na > 90)))
            printf("round na=%d np=%d nb=%d: setup %lld  rebuild %lld (wave0: plain rows %lld merged rows %lld)  tail-barrier %lld cycles\n", na, np, nb,
                   hr_t1 - hr_t0, hr_t2 - hr_t1, hr_dual, hr_slow, (long long)__builtin_readcyclecounter() - hr_t2);
#endif
#ifdef HR_ROUNDS
        if (blockIdx.x == 0 && tid == 0) printf("R %d %d %d\n", na, np, nb);      // round sizes of task 0 (traffic model)
#endif
        done += np; na = nb; cur ^= 1; src = src < 0 ? 0 : (src ^ 1);
        __syncthreads();
    }
#ifdef HR_TIMING
    if ((blockIdx.x == 0 || blockIdx.x == 100) && tid == 0)
        printf("task %d: %d rounds, total %lld cycles: setup %lld  rebuild(wave 0 view) %lld (in row work %lld)  end-of-round barrier wait %lld; entries read+written %lld (%.3f cycles per entry)\n",
               (int)blockIdx.x, hr_rounds, (long long)__builtin_readcyclecounter() - hr_start, hr_acc_setup, hr_acc_rebuild, hr_acc_wave_busy, hr_acc_barrier, hr_acc_entries,
               (double)((long long)__builtin_readcyclecounter() - hr_start) / (double)hr_acc_entries);
#endif
    // (5) the sequential algorithm's order: ascending height, lowest index first; ward.D2 reports sqrt
    __syncthreads();
    {
        int npow2 = 1; while (npow2 < n - 1) npow2 <<= 1;
        double *kh = reinterpret_cast<double *>(sm);            // the state is dead: reuse LDS (16 B per entry <= state size)
        int *ki = reinterpret_cast<int *>(kh + npow2);
        int *kj = ki + npow2;
        for (int q = tid; q < npow2; q += HR_THREADS) {
            if (q < n - 1) { kh[q] = crit[q]; ki[q] = ia[q]; kj[q] = ib[q]; } else { kh[q] = HC_INF; ki[q] = 0x7fffffff; kj[q] = 0; }
        }
        __syncthreads();
        for (int size = 2; size <= npow2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (npow2 >> 1); t += HR_THREADS) {
                    const int lo = ((t / stride) * stride * 2) + (t % stride), hi = lo + stride;
                    const bool up = ((lo & size) == 0);
                    const double x = kh[lo], y = kh[hi];
                    const bool gt = x > y || (x == y && ki[lo] > ki[hi]);
                    if (gt == up) {
                        kh[lo] = y; kh[hi] = x;
                        const int t1 = ki[lo]; ki[lo] = ki[hi]; ki[hi] = t1;
                        const int t2 = kj[lo]; kj[lo] = kj[hi]; kj[hi] = t2;
                    }
                }
                __syncthreads();
            }
        }
        for (int q = tid; q < n - 1; q += HR_THREADS) { crit[q] = method == 8 ? sqrt(kh[q]) : kh[q]; ia[q] = ki[q]; ib[q] = kj[q]; }
    }
    if (tid == 0) {
        status[blockIdx.x] = 0;
        if (MODE == 1) { reinterpret_cast<int *>(img + (reinterpret_cast<unsigned char *>(ctl) - sm))[10] = 2; atomicSub(remaining, 1); }
    }
}

#ifdef SHARP_LAB       // lab builds only (make LAB=1 -> sharp_amd/variants/libsharp_hip_lab.so; LAB_NOTES.md): the agglomeration forms that were
#include "../../tools/lab/hclust_tri.inc"      // measured and not adopted -- on the upper triangle, append-only first rounds, lazy rows
#include "../../tools/lab/hclust_front.inc"
#include "../../tools/lab/hclust_lazy.inc"
#endif

// ---------------------------------------------------------------------------------------------
// host side: the launch recipes of the two kernels (on the current stream, ctx().stream)
// ---------------------------------------------------------------------------------------------
namespace {
// every form of hclust_rnn_kernel takes the same arguments; image_bytes is the image stride (with an image) and the copy length
template <typename K>
void launch_rnn(K kern, dim3 grid, int threads, size_t lds_launch, const HcAggloRange &r, unsigned char *img, size_t image_bytes,
                int round, int *remaining) {
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds_launch, ctx().stream, r.metas, r.D, r.S0, r.S1, r.ia, r.ib, r.height, r.status,
                       img, img ? static_cast<long long>(image_bytes) : 0LL, static_cast<int>(image_bytes), round, remaining,
                       static_cast<int>(lds_launch));
}
}  // namespace

// a4: agglomeration.  Reducible methods go through the bulk-synchronous kernel (streams whole rows between two scratch
// matrices, D stays pristine); whatever it abandons (exact ties, centroid/median, n > 4096) is done by the
// sequential NN-list kernel, which skips the tasks whose status is 0 -- no host round trip in between.
bool hclust_bulk_synchronous(const HcAggloRange &r, bool split_chunk, DevBuf<unsigned char> &img, DevBuf<int> &remaining,
                             hipEvent_t mid_event, int mid_round, HcAggloDid *did) {
    Ctx &c = ctx();
    hipStream_t st = c.stream;
    const int Ts = r.tasks, max_n = r.max_n;
    bool mid_recorded = false;
    const bool gs = max_n > HR_MAXN;                    // state arrays in global memory (always round per launch)
    const size_t lds = hr_image_bytes(max_n);
    const bool mono = knobs().hc_mono;                 // SHARP_HC_MONO=1 (cross-check): the whole agglomeration in one launch
    // Few tasks (one projection, the wMetaC / sMetaC similarity tasks, a cross-block sMetaC of thousands of meta-clusters):
    // one round per pair of launches, every task spread over several workgroups -- 25 tasks of 2000: 4.7 ms against
    // 10.3 ms in one launch, 50 tasks 6.5 against 11.3.  Many tasks (kHcSplitMaxTasks): one launch is faster (the chip is
    // then at its memory limit either way and the per-round launches only add their gaps).  SHARP_HC_SPLIT = 1 / 0 forces
    // the choice; it is made for the whole chunk (a range of a larger chunk stays one launch).
    const bool split = split_chunk || gs;
    if (did) did->form = (!mono || gs) && split ? 1 : 4;
    if ((!mono || gs) && split) {
        // workgroups per task in the rebuild launches: eight when there are tens of tasks (measured, 25 - 136 tasks of 2000);
        // a lone big task (a per-block or cross-block sMetaC of thousands of clusters) gets up to a quarter of the chip
        int wpt = std::max(1, std::min(8, (5 * c.num_cu / 2 + Ts - 1) / Ts));
        if (Ts <= 8) wpt = std::max(wpt, std::min(64, c.num_cu / (4 * Ts)));
        if (knobs().hc_wpt > 0) wpt = knobs().hc_wpt;
        img.ensure(static_cast<size_t>(Ts) * lds);
        remaining.ensure(1);
        const int rem0 = Ts;
        remaining.upload(&rem0, 1);
        auto ka = gs ? hclust_rnn_kernel<1024, 1, true> : hclust_rnn_kernel<1024, 1, false>;
        auto kb = gs ? hclust_rnn_kernel<1024, 2, true> : hclust_rnn_kernel<1024, 2, false>;
        // the rebuild launches stage the pair members' entries like MODE 0: whatever the CU has beyond the state (all of it
        // when the state is global)
        const size_t ldsa = gs ? 0 : lds;
        const size_t ldsl = gs ? HR_LDS_CU : std::max(lds, HR_LDS_CU);
        allow_dynamic_lds(ka, ldsa);
        allow_dynamic_lds(kb, ldsl);
        const int max_rounds = max_n + 8;               // every round merges at least one pair
        // after `finish_at` rounds (about a quarter of the clusters left at the usual 10 % per round) the rest runs in ONE launch
        const int finish_at = knobs().hc_finish_at;
        if (did) { did->wpt = wpt; did->finish_at = finish_at >= 0 ? finish_at : -1; }
        auto kc = gs ? hclust_rnn_kernel<1024, 3, true> : hclust_rnn_kernel<1024, 3, false>;
        if (finish_at >= 0) allow_dynamic_lds(kc, ldsl);
        for (int round = 0; round < max_rounds; ++round) {
            if (mid_event && round == mid_round) { SHARP_HIP_CHECK(hipEventRecord(mid_event, st)); mid_recorded = true; }
            if (finish_at >= 0 && round == finish_at) {
                launch_rnn(kc, dim3(Ts), 1024, ldsl, r, img.p, lds, round, remaining.p);
                break;
            }
            launch_rnn(ka, dim3(Ts), 1024, ldsa, r, img.p, lds, round, remaining.p);
            launch_rnn(kb, dim3(Ts, wpt), 1024, ldsl, r, img.p, lds, round, remaining.p);
            if ((round & 7) == 7) {                     // a finished task costs two empty workgroups per round: look now and then
                int rem = 0;
                remaining.download(&rem, 1);
                if (rem <= 0) break;
            }
        }
#ifdef SHARP_LAB
    } else if (Ts <= c.num_cu && max_n <= HL_MAXN && lab_env("SHARP_HC_LAZY") && lab_env("SHARP_HC_LAZY")[0] == '1') {
        // SHARP_HC_LAZY=1 (an experiment kept for reference): one workgroup per task, rows rewritten only
        // when their cluster merges (hclust_lazy.inc) -- half the bytes of hclust_rnn_kernel, same merges, but at four waves
        // per CU (a 16 KB LDS row buffer each) it runs at a quarter of the bandwidth: 62 ms against 30 ms at cfg2
        const size_t ldsz = hclust_lazy_lds(max_n);
        allow_dynamic_lds(hclust_lazy_kernel, ldsz);
        int theta = 50;
        if (const char *e = lab_env("SHARP_HC_LAZY_THETA")) theta = std::max(10, std::min(95, atoi(e)));
        hipLaunchKernelGGL(hclust_lazy_kernel, dim3(Ts), dim3(HL_THREADS), ldsz, st, r.metas, r.D, r.S0, r.S1, r.ia, r.ib,
                           r.height, r.status, theta);
    } else if (Ts <= c.num_cu && max_n <= HT_MAXN && knobs().hc_tri) {
        // one workgroup per CU on the upper triangle of the matrix (hclust_tri.inc): half the bytes of hclust_rnn_kernel
        const size_t ldsl = hclust_tri_lds(max_n);
        allow_dynamic_lds(hclust_tri_kernel, ldsl);
        hipLaunchKernelGGL(hclust_tri_kernel, dim3(Ts), dim3(HT_THREADS), ldsl, st, r.metas, r.D, r.S0, r.S1, r.ia, r.ib,
                           r.height, r.status, static_cast<int>(ldsl));
    } else if (Ts <= c.num_cu && knobs().hc_front > 0 && max_n <= 2400) {
        // SHARP_HC_FRONT=c (an experiment, hclust_front.inc): the first c rounds without rewriting the matrix -- new rows and the
        // survivors' tails appended beside the pristine D -- then one compaction into S0 and hclust_rnn_kernel's MODE 3 for the rest
        const size_t ldsf = (static_cast<size_t>(max_n) * 3 / 2 + 8) * 34 + 96;
        allow_dynamic_lds(hclust_front_kernel, ldsf);
        img.ensure(static_cast<size_t>(Ts) * lds);
        remaining.ensure(1);
        hipLaunchKernelGGL(hclust_front_kernel, dim3(Ts), dim3(HF_THREADS), ldsf, st, r.metas, r.D, r.S0, r.S1, r.ia, r.ib, r.height,
                           r.status, img.p, static_cast<long long>(lds), knobs().hc_front);
        launch_check("hclust_front_kernel");
        auto kc = hclust_rnn_kernel<1024, 3, false>;
        const size_t ldsl = std::max(lds, HR_LDS_CU);
        allow_dynamic_lds(kc, ldsl);
        launch_rnn(kc, dim3(Ts), 1024, ldsl, r, img.p, lds, 1, remaining.p);
#endif
    } else if (Ts <= c.num_cu && !knobs().hc_half) {
        auto k0 = hclust_rnn_kernel<1024, 0>;
        if (did) did->form = 2;
        // one workgroup per CU: everything the CU has beyond the state stages the pair members' entries
        const size_t ldsl = std::max(lds, HR_LDS_CU);
        allow_dynamic_lds(k0, ldsl);
        launch_rnn(k0, dim3(Ts), 1024, ldsl, r, nullptr, lds, 0, nullptr);
    } else {
        // (also SHARP_HC_HALF=1 with at most one task per CU: the eight-wave form then leaves half of every CU's registers and LDS to a
        // workgroup of the next chunk's distance GEMM -- an experiment)
        auto k0 = hclust_rnn_kernel<512, 0>;
        if (did) did->form = 3;
        const size_t ldsl = std::max(lds, HR_LDS_CU / 2);      // two workgroups per CU
        allow_dynamic_lds(k0, ldsl);
        launch_rnn(k0, dim3(Ts), 512, ldsl, r, nullptr, lds, 0, nullptr);
    }
    launch_check("hclust_rnn_kernel");
    return mid_recorded;
}

void hclust_sequential(const HcAggloRange &r, const int *only_if, unsigned char *gstate) {
    hipStream_t st = ctx().stream;
    const int Ts = r.tasks, max_n = r.max_n;
    const size_t lds = hc_seq_state_bytes(max_n);
    DevBuf<long long> dbg;
#ifdef SHARP_LAB                                                // (lab build, tools/build_variant.sh: phase ablation and per-phase cycle counts)
    const char *abl = lab_env("SHARP_HC_ABLATE");
    const char *tim = lab_env("SHARP_HC_TIMING");
    if (tim) { dbg.alloc(static_cast<size_t>(Ts) * 6); dbg.zero(); }
#else
    const char *abl = nullptr;
#endif
    if (max_n <= kHcLdsMaxN) {
        allow_dynamic_lds(hclust_kernel<false>, lds);
        hipLaunchKernelGGL(hclust_kernel<false>, dim3(Ts), dim3(HC_THREADS), lds, st, r.metas, r.D, r.ia, r.ib, r.height,
                           abl ? atoi(abl) : 0, dbg.p, only_if, nullptr, 0LL);
    } else {                                            // state in global memory
        hipLaunchKernelGGL(hclust_kernel<true>, dim3(Ts), dim3(HC_THREADS), 0, st, r.metas, r.D, r.ia, r.ib, r.height,
                           abl ? atoi(abl) : 0, dbg.p, only_if, gstate, static_cast<long long>(lds));
    }
    launch_check("hclust_kernel");
#ifdef SHARP_LAB
    if (tim) {
        std::vector<long long> h(static_cast<size_t>(Ts) * 6);
        dbg.download(h.data(), h.size());
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int t = 0; t < Ts; ++t) for (int q = 0; q < 6; ++q) acc[q] += static_cast<double>(h[static_cast<size_t>(t) * 6 + q]);
        fprintf(stderr, "hclust phases T=%d n=%d, mean shader cycles per task: argmin %.0f | loads+LW+stores %.0f | nb reduce %.0f | "
                        "list+barrier %.0f | rescans %.0f | end barrier %.0f\n", Ts, max_n, acc[0] / Ts, acc[1] / Ts, acc[2] / Ts,
                acc[3] / Ts, acc[4] / Ts, acc[5] / Ts);
    }
#endif
}

}  // namespace sharp
