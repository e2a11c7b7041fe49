// hclust.hip -- batched get_opt_hclust on the GPU (R/get_opt_hclust.R:33-244):
//   a3  distance build      row_prep + fp64-MFMA correlation GEMM (linalg.hip)                          :66-74
//   a4  stats::hclust       the agglomeration kernels and their launchers (hclust_agglo.hip)            :76-83
//   a5  cutree k=min..max, median silhouette, get_CH("1-corr") (hclust_stats.hip), model selection
//       on the host (hclust_select.hip)                                                                 :90-231
// This file: the workspaces, the pipeline that runs a batch of tasks as chunks on several streams (setup_chunk / enqueue_chunk /
// finish_chunk; every launch recipe is behind a stage launcher of hclust_task.hpp), hclust_tree, and the C ABI.
#include "hclust_task.hpp"

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>

#include "linalg.hpp"

namespace sharp {

namespace {

// grow-only pinned host buffer: the per-chunk result downloads (heights 3 MB, labels 1.5 MB at cfg2) go through it at PCIe speed
// instead of through the driver's staging of pageable memory
template <typename T>
struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    void ensure(size_t count) {
        if (count <= n) return;
        if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
        SHARP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), hipHostMallocDefault));
        n = count;
    }
};

struct Workspace {
    PinnedBuf<double> h_out, h_height;
    PinnedBuf<int> h_packed;
    DevBuf<double> D, D0, S0, S1, Cr, Ct, nrm, height, H, T, G, CSt, Q, out;
    DevBuf<int> ia, ib, lab, chosen, packed, status, remaining;
    DevBuf<unsigned char> img;          // LDS state images of the round-per-launch agglomeration
    DevBuf<double> nnp;                 // per-tile row minima of the distance matrices (HcMeta::nn)
    DevBuf<unsigned char> seqstate;     // nearest-neighbour state of the sequential kernel for tasks beyond kHcLdsMaxN observations
    // many-levels statistics (ml_*_kernel)
    DevBuf<MlMeta> mlmeta;
    DevBuf<double> mlS, mlcn2m, mlB, mlcn2F, mltot2;
    DevBuf<int> mlr1, mlr2, mlcntF;
    DevBuf<long long> packoff;
    DevBuf<HcMeta> meta;
    DevBuf<RowPrepTask> prep;
    DevBuf<GemmTask> gemm;
#ifdef SHARP_LAB
    DevBuf<DistI8Task> i8;              // the sliced-integer form of the distance GEMM (tools/lab/gemm_i8.hip): descriptors, digits, row scales
    DevBuf<signed char> sl;
    DevBuf<double> slscale;
#endif
};
// Two sets of buffers so that consecutive chunks of tasks can be in flight together (run_chunks); the scratch of the agglomeration
// itself (S0, S1, img, remaining) is only ever used by one chunk at a time and always comes from set 0.
// Slot 3: the third set of a batch of three chunks or more; slot 2: a batch started from another batch's progress callback;
// slots 4 and 5: batches whose distance matrices are built ahead of time for the NEXT block of a SHARP_unlimited run (hc_prefetch_*).
struct WorkspaceSets { Workspace w[6]; };
Workspace &ws(int slot = 0) { return per_slot<WorkspaceSets>().w[slot]; }
// The device buffers of every set of the calling thread's slot go back to the driver (sharp_trim for worker and helper slots: a process
// that ran several slots on ONE GPU -- the tests do -- otherwise keeps tens of GB per slot); the caller has synchronised the device.
static void release_workspaces_of_slot() {
    for (Workspace &W : per_slot<WorkspaceSets>().w) {
        for (DevBuf<double> *b : {&W.D, &W.D0, &W.S0, &W.S1, &W.Cr, &W.Ct, &W.nrm, &W.height, &W.H, &W.T, &W.G, &W.CSt, &W.Q, &W.out,
                                  &W.mlS, &W.mlcn2m, &W.mlB, &W.mlcn2F, &W.mltot2}) b->release();
        for (DevBuf<int> *b : {&W.ia, &W.ib, &W.lab, &W.chosen, &W.packed, &W.status, &W.remaining, &W.mlr1, &W.mlr2, &W.mlcntF}) b->release();
        W.img.release(); W.seqstate.release(); W.nnp.release();
#ifdef SHARP_LAB
        W.sl.release(); W.slscale.release();
#endif
    }
}

inline long long rup(long long v, long long a) { return (v + a - 1) / a * a; }

// Batches of at most this many tasks run the round-per-launch agglomeration (a task spread over several workgroups); above, one
// workgroup per task in one launch.  Measured at 2000 observations per task: 75 tasks 8.7 vs 11.7 ms, 125 tasks 11.1 vs 12.1 ms,
// 150 tasks 14.0 vs 13.2 ms, 175 tasks 15.3 vs 14.4 ms (tools/bench_hc.py, SHARP_HC_SPLIT=1 / 0).
constexpr int kHcSplitMaxTasks = 136;
// more candidate levels than this in a chunk: the incremental per-level statistics (ml_*_kernel) instead of stats_kernel
constexpr int kMlMinLevels = 256;
static int ml_min_levels() { return knobs().ml_min_levels > 0 ? knobs().ml_min_levels : kMlMinLevels; }   // (SHARP_ML_MIN_LEVELS: tests)
constexpr int kHcSplitMinObs = 1000;

// One chunk of tasks: enqueue_chunk() puts all its device work on streams, finish_chunk() fetches the statistics, selects the
// levels on the host and fetches the labels.  `pipe` = the chunk is one of several in flight (run on its slot's own stream, ordered
// against its neighbours by events, see get_opt_hclust_batch); otherwise everything is relative to the library's main stream.
struct ChunkJob {
    size_t i0 = 0, i1 = 0;
    int T = 0, slot = 0;
    bool pipe = false, first = true;
    hipEvent_t input_ready = nullptr;          // pipelined: what the chunk's stream waits for before it reads its tasks' inputs (nullptr: EV.in)
    bool i8 = false;          // the distance matrices through the sliced-integer GEMM
    std::vector<HcMeta> metas;
    std::vector<RowPrepTask> prep;
    std::vector<GemmTask> g;
    long long oOut = 0, oM = 0, oLab = 0;
    int max_n = 0, max_p = 0, max_nk = 0, max_kpad = 0, NS = 1;
    bool split = false;                        // round-per-launch agglomeration (few tasks)
    bool ml = false;                           // many candidate levels: the incremental statistics kernels
    std::vector<MlMeta> mlmetas;
    int ml_off = 0, ml_cnt = 0, mlt_off = 0, mlt_cnt = 0;   // GEMM descriptors of the row-major G and T
    bool seq_pending = false;                  // the sequential fallback kernel is still to be launched (with the statistics phase)
    bool has_next = false;                     // pipelined: another chunk follows (its distance GEMM is enqueued before this one's tail)
    bool one_range = false;                    // everything on the current stream (a batch prepared ahead of time, hc_prefetch_begin)
    int scratch_slot = 0;                      // whose S0 / S1 / img / remaining the agglomeration uses (set 0 unless the batch is nested)
    int prev_slot = 1, next_slot = 1;          // pipelined: the slots of the chunk before and after this one (two or three slots in rotation)
    int plan_row = -1;                         // this chunk's row of the slot's plan record (plan_add), -1: not recorded
    int next2_slot = -1;                       // three slots: the chunk after the next, whose distance GEMM the statistics also let pass
    hipEvent_t mid_event = nullptr;            // recorded behind round `mid_round` of the round-per-launch agglomeration (if it gets that far)
    int mid_round = 8;
    bool mid_recorded = false;
    struct Range { int t0, t1; int off[5], cnt[5]; int off8 = 0; bool any_sym, any_feat; };
    std::vector<Range> ranges;
};
enum : int { PH_DIST = 1, PH_AGGLO = 2, PH_STATS = 4, PH_ALL = 7 };
struct PipeEvents {
    hipEvent_t in = nullptr, out[8] = {nullptr}, gemm[6] = {nullptr}, hc[6] = {nullptr}, done[6] = {nullptr}, prep[6] = {nullptr};   // (per workspace slot)
};
PipeEvents &pipe_events() {
    PipeEvents &e = per_slot<PipeEvents>();
    if (!e.in) {
        SHARP_HIP_CHECK(hipEventCreateWithFlags(&e.in, hipEventDisableTiming));
        for (auto &x : e.out) SHARP_HIP_CHECK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
        for (int q = 0; q < 6; ++q) {
            SHARP_HIP_CHECK(hipEventCreateWithFlags(&e.gemm[q], hipEventDisableTiming));
            SHARP_HIP_CHECK(hipEventCreateWithFlags(&e.hc[q], hipEventDisableTiming));
            SHARP_HIP_CHECK(hipEventCreateWithFlags(&e.done[q], hipEventDisableTiming));
            SHARP_HIP_CHECK(hipEventCreateWithFlags(&e.prep[q], hipEventDisableTiming));
        }
    }
    return e;
}

// What the last get_opt_hclust_batch of the calling slot did, one row per chunk (sharp_hclust_batch_plan; include/sharp_hip.h names the
// columns): written on the host as the chunks are set up and their agglomeration is enqueued, no device work.  A batch started from the
// progress callback of another adds its row (nested = 1) to the outer batch's record.
struct BatchPlan { std::vector<std::array<int, kHcPlanCols>> rows; };
BatchPlan &batch_plan() { return per_slot<BatchPlan>(); }
void plan_add(ChunkJob &J, bool nested) {
    std::vector<std::array<int, kHcPlanCols>> &rows = batch_plan().rows;
    J.plan_row = static_cast<int>(rows.size());
    rows.push_back({static_cast<int>(J.i0), static_cast<int>(J.i1), J.slot, J.pipe, J.split, J.NS, J.ml, J.max_n, J.max_kpad, 0, 0,
                    J.max_n > HR_MAXN, nested, J.max_nk, 0, 0});
}

// Descriptors, workspace and uploads of a chunk (before its first phase).
void setup_chunk(const std::vector<HcTask> &tasks, ChunkJob &J) {
    Ctx &c = ctx();
    Workspace &W = ws(J.slot);
    Workspace &W0 = ws(J.scratch_slot);        // agglomeration scratch: shared, one chunk's agglomeration runs at a time
    PipeEvents &EV = pipe_events();
    const size_t i0 = J.i0;
    const int T = J.T = static_cast<int>(J.i1 - J.i0);
    std::vector<HcMeta> &metas = J.metas;
    metas.assign(T, HcMeta());
    // a pipelined chunk lives on its slot's stream from its first upload on (the slot's buffers are reused by the chunk after next,
    // which is on the same stream); its inputs come from the main stream (EV.in, recorded by the caller)
    hipStream_t chunk_stream = J.pipe ? c.aux_stream(J.slot) : c.stream;
    if (J.pipe) SHARP_HIP_CHECK(hipStreamWaitEvent(chunk_stream, J.input_ready ? J.input_ready : EV.in, 0));
    StreamScope chunk_scope(chunk_stream);
    long long oD = 0, oD0 = 0, oCr = 0, oCt = 0, oN = 0, oM = 0, oLab = 0, oK = 0, oCS = 0, oQ = 0, oOut = 0;
    int max_n = 0, max_p = 0, max_nk = 0, max_kpad = 0;
    for (int t = 0; t < T; ++t) {
        const HcTask &tk = tasks[i0 + t];
        HcMeta &M = metas[t];
        SHARP_REQUIRE(tk.n >= 3, "get_opt_hclust: need at least 3 observations");
        SHARP_REQUIRE(tk.n <= kHcMaxN, "get_opt_hclust: more than 16384 observations in one clustering task is not supported");
        SHARP_REQUIRE(tk.prm.hmethod >= 1 && tk.prm.hmethod <= 8, "get_opt_hclust: unknown agglomeration method");
        M.n = tk.n; M.p = tk.symmetric ? tk.n : tk.p; M.nld = static_cast<int>(rup(tk.n, 128));
        M.method = tk.prm.hmethod; M.symmetric = tk.symmetric ? (tk.distance ? 2 : 1) : 0; M.pad0 = 0;   // 2: a distance matrix as it is (hclust_tree)
        if (tk.prm.N_cluster > 0) {
            SHARP_REQUIRE(tk.prm.N_cluster >= 2, "The given N.cluster is less than 2, which is not suitable for clustering!");
            SHARP_REQUIRE(tk.prm.N_cluster <= tk.n - 1, "N.cluster must be smaller than the number of observations");
            M.kmin = M.kmax = tk.prm.N_cluster;
        } else {
            M.kmin = tk.prm.minN;
            M.kmax = std::min(tk.prm.maxN, tk.n - 1);
            SHARP_REQUIRE(M.kmin >= 2 && M.kmax >= M.kmin, "get_opt_hclust: empty range of cluster numbers (minN.cluster..maxN.cluster)");
        }
        M.nk = M.kmax - M.kmin + 1;
        M.kpad = static_cast<int>(rup(M.kmax, 16));
        M.oD = oD; oD += static_cast<long long>(M.nld) * M.nld;
        M.oD0 = oD0; if (M.symmetric == 1) oD0 += static_cast<long long>(M.nld) * M.nld;
        M.oCr = oCr; if (M.symmetric != 2) oCr += static_cast<long long>(M.n) * M.p;      // (a distance task has no feature rows: no statistics)
        M.oCt = oCt; if (M.symmetric != 2) oCt += rup(M.p, 16) * M.nld;
        M.oNrm = oN; oN += M.n;
        M.oM = oM; oM += M.n;
        M.oLab = oLab; oLab += static_cast<long long>(M.nk) * M.n;
        M.oH = M.oT = M.oG = oK; oK += static_cast<long long>(M.nld) * M.kpad;   // H: n x kpad; T, G: kpad x nld (transposed)
        M.oCSt = oCS; oCS += static_cast<long long>(M.p) * M.kpad;
        M.oQ = oQ; oQ += static_cast<long long>(M.kpad) * M.kpad;
        M.oOut = oOut; oOut += 2LL * M.nk;
        max_n = std::max(max_n, M.n); max_p = std::max(max_p, M.p); max_nk = std::max(max_nk, M.nk);
        max_kpad = std::max(max_kpad, M.kpad);
    }
    J.oOut = oOut; J.oM = oM; J.oLab = oLab; J.max_n = max_n; J.max_p = max_p; J.max_nk = max_nk; J.max_kpad = max_kpad;
    SHARP_REQUIRE(max_nk > ml_min_levels() ||
                  stats_lds_bytes(max_n, std::max(max_kpad, 64)) <= ST_LDS_MAX,
                  "get_opt_hclust: this many observations with this many candidate cluster numbers does not fit the silhouette kernel "
                  "(LDS: 8 B per observation rounded up to a power of two + 36 B per candidate cluster)");
    { HostTimer ht("hc_workspace_alloc");
    W.D.ensure(oD); W0.S0.ensure(oD); W0.S1.ensure(oD); W.D0.ensure(std::max<long long>(oD0, 1)); W.Cr.ensure(oCr); W.Ct.ensure(oCt); W.nrm.ensure(oN);
    W.height.ensure(oM); W.ia.ensure(oM); W.ib.ensure(oM); W.lab.ensure(oLab);
    W.H.ensure(oK); W.T.ensure(oK); W.G.ensure(oK); W.CSt.ensure(oCS); W.Q.ensure(oQ); W.out.ensure(oOut); }
    { HostTimer ht("hc_workspace_alloc");
    W.meta.ensure(T); W.prep.ensure(T); W.gemm.ensure(5 * static_cast<size_t>(T)); W.status.ensure(T); }
    // feature tasks of at most 2048 observations: the distance GEMM also leaves every row's minimum per column tile (SHARP_HC_NN_GEMM=0: the
    // agglomeration's first round scans D)
    {
        bool parts = knobs().hc_nn_gemm;
#ifdef SHARP_LAB
        if (knobs().dist_i8 && max_p <= 8192) parts = false;   // (the sliced-integer GEMM of the lab build writes none)
#endif
        long long oNN = 0;
        if (parts) for (int t = 0; t < T; ++t) if (!metas[t].symmetric && metas[t].nld <= 2048) oNN += static_cast<long long>(metas[t].nld / 128) * metas[t].nld;
        if (oNN > 0) {
            W.nnp.ensure(oNN);
            oNN = 0;
            for (int t = 0; t < T; ++t) if (!metas[t].symmetric && metas[t].nld <= 2048) { metas[t].nn = W.nnp.p + oNN; oNN += static_cast<long long>(metas[t].nld / 128) * metas[t].nld; }
        }
    }
    W.meta.upload(metas.data(), T);

    // Every descriptor of the chunk goes up once; the device work is then enqueued per RANGE of tasks, each range on its
    // own stream: the agglomeration is a memory-latency/scatter-bound kernel and the correlation GEMM an MFMA-bound one,
    // so a range's GEMM, cutree and silhouette statistics run underneath the agglomeration of the other ranges.
    int NS = T >= 194 ? 2 : 1;  // two ranges of more than 96 tasks each (the one-launch agglomeration); 3 or more are slower than one
    {
        // the round-per-launch agglomeration synchronises with the host every few rounds: one range at a time
        // (small tasks -- the similarity matrices of wMetaC and of a per-block sMetaC, a few hundred meta-clusters -- have nothing to
        // spread over several workgroups: the per-round launches and the host's look every eight rounds only cost, 0.27 ms per SHARP() call)
        const bool split = knobs().hc_split >= 0 ? knobs().hc_split == 1 : (T <= kHcSplitMaxTasks && max_n >= kHcSplitMinObs);
        J.split = split;
        if (!knobs().hc_seq && ((!knobs().hc_mono && split) || max_n > HR_MAXN)) NS = 1;
    }
    if (knobs().hc_ranges > 0) NS = std::max(1, std::min(8, knobs().hc_ranges));
    if (J.pipe || J.one_range) NS = 1;          // the overlap comes from the neighbouring chunks / blocks
    if (J.max_nk > ml_min_levels()) NS = 1;   // many levels: one range
    NS = std::min(NS, T);
    std::vector<RowPrepTask> &prep = J.prep;
    prep.assign(T, RowPrepTask());
    for (int t = 0; t < T; ++t) {
        const HcTask &tk = tasks[i0 + t];
        const HcMeta &M = metas[t];
        prep[t] = RowPrepTask{tk.d_mat, tk.ld, M.n, M.p, M.nld, static_cast<int>(rup(M.p, 16)), M.symmetric, W.Cr.p + M.oCr,
                              W.Ct.p + M.oCt, W.nrm.p + M.oNrm, W.D.p + M.oD};
    }
    W.prep.upload(prep.data(), T);
    typedef ChunkJob::Range Range;
    J.NS = NS;
    std::vector<Range> &ranges = J.ranges;
    ranges.assign(NS, Range());
    std::vector<GemmTask> &g = J.g;
    g.clear();
    g.reserve(5 * static_cast<size_t>(T));
    for (int s = 0; s < NS; ++s) {
        Range &R = ranges[s];
        R.t0 = static_cast<int>(static_cast<long long>(T) * s / NS);
        R.t1 = static_cast<int>(static_cast<long long>(T) * (s + 1) / NS);
        R.any_sym = R.any_feat = false;
        for (int kind = 0; kind < 5; ++kind) {
            R.off[kind] = static_cast<int>(g.size());
            for (int t = R.t0; t < R.t1; ++t) {
                const HcMeta &M = metas[t];
                R.any_sym |= M.symmetric != 0; R.any_feat |= M.symmetric == 0;
                switch (kind) {
                    case 0:   // D = 1 - U U^T (feature tasks)
                        if (!M.symmetric) g.push_back(GemmTask{W.Ct.p + M.oCt, W.Ct.p + M.oCt, W.D.p + M.oD, M.n, M.n, M.p, M.nld, M.nld, M.nld, 1, 1, 1,
                                                               const_cast<double *>(M.nn), M.method == 8});
                        break;
                    case 1:   // finest-level sums on the MFMA:  CSt = Cr^T H
                        g.push_back(GemmTask{W.Cr.p + M.oCr, W.H.p + M.oH, W.CSt.p + M.oCSt, M.p, M.kpad, M.n, M.p, M.kpad, M.kpad, 0, 0, 0});
                        break;
                    case 2:   // G^T = CS C^T  (kpad x nld: the statistics kernel reads it with lanes along the cells)
                        g.push_back(GemmTask{W.CSt.p + M.oCSt, W.Ct.p + M.oCt, W.G.p + M.oG, M.kpad, M.n, M.p, M.kpad, M.nld, M.nld, 0, 0, 0});
                        break;
                    case 3:   // Q = CS CS^T
                        g.push_back(GemmTask{W.CSt.p + M.oCSt, W.CSt.p + M.oCSt, W.Q.p + M.oQ, M.kpad, M.kpad, M.p, M.kpad, M.kpad, M.kpad, 0, 0, 0});
                        break;
                    default:  // (symmetric) T^T = H^T D0  (kpad x nld)
                        if (M.symmetric == 1) g.push_back(GemmTask{W.H.p + M.oH, W.D0.p + M.oD0, W.T.p + M.oT, M.kpad, M.n, M.n, M.kpad, M.nld, M.nld, 0, 0, 0});
                        break;
                }
            }
            R.cnt[kind] = static_cast<int>(g.size()) - R.off[kind];
        }
    }
#ifdef SHARP_LAB
    J.i8 = knobs().dist_i8 && max_p <= 8192;
    if (J.i8) {
        std::vector<DistI8Task> d8;
        size_t oSl = 0, oSc = 0;
        for (int t = 0; t < T; ++t) if (!metas[t].symmetric) { oSl += dist_i8_slice_bytes(metas[t].nld, metas[t].p); oSc += metas[t].nld; }
        W.sl.ensure(std::max<size_t>(oSl, 1)); W.slscale.ensure(std::max<size_t>(oSc, 1));
        oSl = 0; oSc = 0;
        for (int s = 0; s < NS; ++s) {
            ranges[s].off8 = static_cast<int>(d8.size());
            for (int t = ranges[s].t0; t < ranges[s].t1; ++t) {
                const HcMeta &M = metas[t];
                if (M.symmetric) continue;
                d8.push_back(DistI8Task{W.Cr.p + M.oCr, W.D.p + M.oD, W.sl.p + oSl, W.slscale.p + oSc, M.n, M.p, M.nld, (M.p + 31) / 32});
                oSl += dist_i8_slice_bytes(M.nld, M.p); oSc += M.nld;
            }
        }
        W.i8.ensure(std::max<size_t>(d8.size(), 1));
        if (!d8.empty()) W.i8.upload(d8.data(), d8.size());
    }
#endif
    // many candidate levels (> kMlMinLevels; SHARP_ML_MIN_LEVELS for tests): G and T of the whole chunk row-major (n x kpad)
    J.ml = max_nk > ml_min_levels();
    if (J.ml) {
        SHARP_REQUIRE(static_cast<size_t>(max_kpad) * 22 + 64 <= HR_LDS_CU, "get_opt_hclust: too many candidate cluster numbers (more than ~7400)");
        J.ml_off = static_cast<int>(g.size());
        for (int t = 0; t < T; ++t) {                      // G = C CS^T  (n x kpad)
            const HcMeta &M = metas[t];
            g.push_back(GemmTask{W.Ct.p + M.oCt, W.CSt.p + M.oCSt, W.G.p + M.oG, M.n, M.kpad, M.p, M.nld, M.kpad, M.kpad, 0, 0, 0});
        }
        J.ml_cnt = T;
        J.mlt_off = static_cast<int>(g.size());
        for (int t = 0; t < T; ++t) {                      // (symmetric) T = D0 H  (n x kpad)
            const HcMeta &M = metas[t];
            if (M.symmetric == 1) g.push_back(GemmTask{W.D0.p + M.oD0, W.H.p + M.oH, W.T.p + M.oT, M.n, M.kpad, M.n, M.nld, M.kpad, M.kpad, 0, 0, 0});
        }
        J.mlt_cnt = static_cast<int>(g.size()) - J.mlt_off;
        W.gemm.ensure(g.size());
        J.mlmetas.assign(T, MlMeta());
        long long oS = 0, oMg = 0, oFin = 0;
        for (int t = 0; t < T; ++t) {
            const HcMeta &M = metas[t];
            J.mlmetas[t].oS = oS; oS += 2LL * M.n * M.nk;
            J.mlmetas[t].oMerge = oMg; oMg += M.nk;
            J.mlmetas[t].oFin = oFin; oFin += M.kmax;
        }
        W.mlmeta.ensure(T); W.mlS.ensure(oS); W.mlcn2m.ensure(oMg); W.mlB.ensure(oMg); W.mlr1.ensure(oMg); W.mlr2.ensure(oMg);
        W.mlcntF.ensure(oFin); W.mlcn2F.ensure(oFin); W.mltot2.ensure(T);
        W.mlmeta.upload(J.mlmetas.data(), T);
    }
    W.gemm.upload(g.data(), g.size());
    if (NS > 1) SHARP_HIP_CHECK(hipEventRecord(EV.in, chunk_stream));     // inputs and descriptors are ready
}

// Device work of a chunk, in three phases (`phases`: any contiguous set, in order): PH_DIST rows -> distance matrix, PH_AGGLO the
// agglomeration, PH_STATS cutree and the per-level statistics.  A pipelined chunk has one range on its slot's stream.
void enqueue_chunk(ChunkJob &J, int phases) {
    Ctx &c = ctx();
    Workspace &W = ws(J.slot);
    Workspace &W0 = ws(J.scratch_slot);
    PipeEvents &EV = pipe_events();
    const int NS = J.NS, max_n = J.max_n, max_p = J.max_p, max_kpad = J.max_kpad;
    hipStream_t main_stream = c.stream;
    hipStream_t chunk_stream = J.pipe ? c.aux_stream(J.slot) : main_stream;
    hipEvent_t ev_in = EV.in, *ev_out = EV.out;

    for (int s = 0; s < NS; ++s) {
        const ChunkJob::Range &R = J.ranges[s];
        const int Ts = R.t1 - R.t0;
        hipStream_t st = NS > 1 ? c.aux_stream(s) : chunk_stream;
        StreamScope scope(st);
        const HcMeta *dmeta = W.meta.p + R.t0;
        const HcAggloRange agglo{dmeta, Ts, max_n, W.D.p, W0.S0.p, W0.S1.p, W.ia.p, W.ib.p, W.height.p, W.status.p + R.t0};
        auto launch_sequential = [&](bool fallback_only) {
            KernelTimer tm("hclust_sequential");
            unsigned char *gstate = nullptr;
            if (max_n > kHcLdsMaxN) {                           // state in global memory (W.seqstate is per slot, like D)
                const size_t stride = hc_seq_state_bytes(max_n);
                W.seqstate.ensure(static_cast<size_t>(J.T) * stride);
                gstate = W.seqstate.p + static_cast<size_t>(R.t0) * stride;
            }
            hclust_sequential(agglo, fallback_only ? agglo.status : nullptr, gstate);
        };
        if (phases & PH_DIST) {
        if (NS > 1) SHARP_HIP_CHECK(hipStreamWaitEvent(st, ev_in, 0));
        // pipelined: this chunk's row preparation (HBM-bound, 0.75 ms alone) follows the previous chunk's at once, i.e. it runs beside the
        // previous chunk's distance GEMM (MFMA-bound) -- behind that GEMM it ran beside the previous chunk's agglomeration, took 2.5 ms
        // there and delayed this chunk's GEMM, which the NEXT agglomeration waits for, by as much (r03 timeline: the second
        // agglomeration of a cfg2 step started 1.9 ms after the first had ended);
        if (J.pipe && !J.first) SHARP_HIP_CHECK(hipStreamWaitEvent(st, knobs().hc_prep_early ? EV.prep[J.prev_slot] : EV.gemm[J.prev_slot], 0));
        // a3: rows -> centred/normalised (+ 1 - S for similarity input), then D = 1 - U U^T
        row_prep_batched(W.prep.p + R.t0, Ts, max_n, max_p, !R.any_sym);
        if (J.pipe) SHARP_HIP_CHECK(hipEventRecord(EV.prep[J.slot], st));
        // this chunk's distance GEMM starts when the previous chunk's has finished, i.e. together with the previous chunk's
        // agglomeration, and fills the CUs that one leaves free (it holds a whole CU per task)
        if (J.pipe && !J.first) SHARP_HIP_CHECK(hipStreamWaitEvent(st, EV.gemm[J.prev_slot], 0));
#ifdef SHARP_LAB
        if (R.cnt[0] && J.i8) dist_i8_batched(W.i8.p + R.off8, R.cnt[0], max_n);
        else
#endif
        if (R.cnt[0]) gemm_tn_f64_batched(W.gemm.p + R.off[0], R.cnt[0], max_n, max_n, "corr_dist_gemm", true, true);
        if (J.pipe) SHARP_HIP_CHECK(hipEventRecord(EV.gemm[J.slot], st));
        if (R.any_sym) {
            KernelTimer tm("copy_d");
            hclust_copy_d(dmeta, Ts, W.D.p, W.D0.p);
        }
        }
        if (phases & PH_AGGLO) {
        if (J.pipe && !J.first) SHARP_HIP_CHECK(hipStreamWaitEvent(st, EV.hc[J.prev_slot], 0));   // one agglomeration at a time (S0 / S1)
        // a4: agglomeration.  The bulk-synchronous kernel first (SHARP_HC_SEQ=1, a cross-check: the sequential kernel only); whatever
        // it abandons (status != 0: exact ties, centroid / median) is done by the sequential kernel, which skips the other tasks -- no
        // host round trip in between.
        {
            const bool use_rnn = !knobs().hc_seq;
            KernelTimer tm("hclust");
            HcAggloDid did;
            if (use_rnn && hclust_bulk_synchronous(agglo, J.split, W0.img, W0.remaining, J.mid_event, J.mid_round, &did)) J.mid_recorded = true;
            // When the sequential kernel is only the fallback, a pipelined chunk with a successor launches it with its statistics
            // phase: its (normally idle) workgroups would otherwise take CU slots from the successor's distance GEMM, which is on the
            // critical path.
            if (!use_rnn || !(J.pipe && J.has_next)) launch_sequential(use_rnn);
            else J.seq_pending = true;
            if (J.plan_row >= 0 && s == 0) {                // (the ranges of a chunk are equal to within one task: the first one's form)
                std::array<int, kHcPlanCols> &row = batch_plan().rows[J.plan_row];
                row[9] = J.seq_pending; row[10] = did.form; row[14] = did.wpt; row[15] = did.finish_at;
            }
        }
        if (J.pipe) SHARP_HIP_CHECK(hipEventRecord(EV.hc[J.slot], st));
        if (J.pipe && knobs().step_marks)
            SHARP_HIP_CHECK(hipLaunchHostFunc(st, [](void *) { step_mark("    (device) an agglomeration ends"); }, nullptr));
        }
        if (!(phases & PH_STATS)) continue;
        // pipelined: the next chunk's distance GEMM (already enqueued) is on the critical path -- its agglomeration cannot start
        // before it -- and this tail is not: it waits for that GEMM and then runs beside the next agglomeration, whose stream has
        // the higher priority or is served first, on the CUs that one leaves free
        if (J.pipe && J.has_next) SHARP_HIP_CHECK(hipStreamWaitEvent(st, EV.gemm[J.next_slot], 0));
        if (J.pipe && J.next2_slot >= 0) SHARP_HIP_CHECK(hipStreamWaitEvent(st, EV.gemm[J.next2_slot], 0));
        if (J.seq_pending) { launch_sequential(true); J.seq_pending = false; }
        // a5: labels for every candidate k, then the statistics of every level (many levels: the chunk is one range, see setup_chunk)
        const HcStatsRange stats{dmeta, Ts, max_n, max_p, J.max_nk, max_kpad, R.any_sym, W.gemm.p, R.off, R.cnt, W.ia.p, W.ib.p, W.lab.p,
                                 W.H.p, W.Cr.p, W.CSt.p, W.T.p, W.G.p, W.Q.p, W.nrm.p, W.out.p};
        const HcManyLevels many{&J.metas, &J.mlmetas, W.mlmeta.p, J.oM, J.ml_off, J.ml_cnt, J.mlt_off, J.mlt_cnt, W.mlr1.p, W.mlr2.p, W.mlcntF.p,
                                W.mlcn2m.p, W.mlB.p, W.mlcn2F.p, W.mltot2.p, W.mlS.p};
        hclust_level_stats(stats, J.ml ? &many : nullptr);
        if (NS > 1) {
            SHARP_HIP_CHECK(hipEventRecord(ev_out[s], st));
            SHARP_HIP_CHECK(hipStreamWaitEvent(main_stream, ev_out[s], 0));
        }
    }
    if (J.pipe && (phases & PH_STATS)) SHARP_HIP_CHECK(hipEventRecord(EV.done[J.slot], chunk_stream));
    if (J.pipe && (phases & PH_STATS) && knobs().step_marks)
        SHARP_HIP_CHECK(hipLaunchHostFunc(chunk_stream, [](void *) { step_mark("    (device) a chunk's statistics end"); }, nullptr));
}

void finish_chunk(const std::vector<HcTask> &tasks, ChunkJob &J, bool want_v, std::vector<HcResult> &out, bool want_status) {
    Ctx &c = ctx();
    Workspace &W = ws(J.slot);
    const size_t i0 = J.i0;
    const int T = J.T;
    const long long oOut = J.oOut, oM = J.oM, oLab = J.oLab;
    const std::vector<HcMeta> &metas = J.metas;
    if (J.pipe) SHARP_HIP_CHECK(hipStreamWaitEvent(c.stream, pipe_events().done[J.slot], 0));
    W.h_out.ensure(std::max<long long>(oOut, 1)); W.h_height.ensure(std::max<long long>(oM, 1));
    double *h_out = W.h_out.p, *h_height = W.h_height.p;
    if (c.profiling || want_status) {      // which agglomeration kernel did the work (tests assert on it)
        std::vector<int> st(T, 1);
        if (!knobs().hc_seq) W.status.download(st.data(), T);
        int fallback = 0;
        for (int v : st) fallback += v != 0;
        if (c.profiling) {
            c.stats["host:hclust_tasks_bulk_synchronous"].launches += T - fallback;
            c.stats["host:hclust_tasks_sequential"].launches += fallback;
        }
        if (want_status) for (int t = 0; t < T; ++t) out[i0 + t].sequential = st[t] != 0;
    }
    HostTimer ht_tail("hc_download_select");
    W.out.download(h_out, oOut);
    W.height.download(h_height, oM);
    // model selection on the host (a few dozen numbers per task)
    std::vector<int> chosen(T);
    std::vector<long long> poff(T);
    long long ptot = 0;
    for (int t = 0; t < T; ++t) { poff[t] = ptot; ptot += metas[t].n; }
    host_parallel_for(T, T >= 16 ? 16 : 1, [&](int t) {     // (each task writes its own result only)
        const HcTask &tk = tasks[i0 + t];
        const HcMeta &M = metas[t];
        HcResult &R = out[i0 + t];
        R.rc = 0; R.nk = M.nk;
        R.msil.assign(h_out + M.oOut, h_out + M.oOut + M.nk);
        R.CHind.assign(h_out + M.oOut + M.nk, h_out + M.oOut + 2 * M.nk);
        R.height.assign(h_height + M.oM, h_height + M.oM + M.n - 1);
        int oind = 1;
        if (tk.prm.N_cluster > 0) {
            R.branch = 0; R.maxsil = R.msil[0];
            R.CHind[0] = std::numeric_limits<double>::quiet_NaN();   // intCriteria value: filled by the single-task wrapper
        } else {
            select_level(tk.prm, M.n, M.nk, R.msil.data(), R.CHind.data(), R.height.data(), oind, R.branch, R.rc);
            R.maxsil = *std::max_element(R.msil.begin(), R.msil.end());
        }
        if (decision_log_on()) {
            double row[kDecisionCols];
            decision_row(tk.prm, M.n, M.kmin, M.nk, R.msil.data(), R.CHind.data(), R.height.data(), oind, R.branch, row);
            decision_log_add(row);
        }
        chosen[t] = oind - 1;
    });
    if (c.profiling) {      // which rule of R/get_opt_hclust.R:162-229 decided each task's level (bench.py reports the split per data set)
        static const char *const rule[3] = {"silhouette", "CH", "height"};
        for (int t = 0; t < T; ++t) {
            if (tasks[i0 + t].prm.N_cluster > 0) continue;
            const std::string key = std::string(tasks[i0 + t].symmetric ? "host:level_meta_by_" : "host:level_base_by_") + rule[std::min(2, std::max(0, out[i0 + t].branch))];
            c.stats[key].launches += 1;
        }
    }
    W.chosen.ensure(T); W.packoff.ensure(T); W.packed.ensure(ptot);
    W.chosen.upload(chosen.data(), T);
    W.packoff.upload(poff.data(), T);
    hclust_pack_labels(W.meta.p, T, W.lab.p, W.chosen.p, W.packoff.p, W.packed.p);
    W.h_packed.ensure(std::max<long long>(ptot, 1));
    int *h_packed = W.h_packed.p;
    W.packed.download(h_packed, ptot);
    std::vector<int> h_lab;
    if (want_v) { h_lab.resize(oLab); W.lab.download(h_lab.data(), oLab); }
    host_parallel_for(T, T >= 16 ? 16 : 1, [&](int t) {
        const HcMeta &M = metas[t];
        HcResult &R = out[i0 + t];
        R.f.assign(h_packed + poff[t], h_packed + poff[t] + M.n);
        R.optN = *std::max_element(R.f.begin(), R.f.end());
        if (want_v) R.v.assign(h_lab.begin() + M.oLab, h_lab.begin() + M.oLab + static_cast<long long>(M.nk) * M.n);
    });
}

}  // namespace

namespace { thread_local int g_batch_depth = 0; }         // > 0 while a batch's progress callback runs: a batch started from there is nested
namespace {
struct AfterAgglo { std::function<void(hipEvent_t)> fn; bool fired = false; };
AfterAgglo &after_agglo() { return per_slot<AfterAgglo>(); }
}  // namespace
void hc_release_workspaces() { release_workspaces_of_slot(); }
int hc_batch_plan_fetch(int *rows, int cap_rows) {
    const std::vector<std::array<int, kHcPlanCols>> &have = batch_plan().rows;
    for (size_t r = 0; r < have.size() && r < static_cast<size_t>(cap_rows); ++r) std::copy(have[r].begin(), have[r].end(), rows + r * kHcPlanCols);
    return static_cast<int>(have.size());
}
void hc_set_after_last_agglomeration(std::function<void(hipEvent_t)> fn) { after_agglo().fn = std::move(fn); after_agglo().fired = false; }
bool hc_after_last_agglomeration_fired() { return after_agglo().fired; }

void get_opt_hclust_batch(const std::vector<HcTask> &tasks, bool want_v, std::vector<HcResult> &out,
                          const std::function<void(size_t)> *progress, const std::function<hipEvent_t(size_t)> *prepare, bool want_status) {
    out.assign(tasks.size(), HcResult());
    if (g_batch_depth == 0) batch_plan().rows.clear();
    if (tasks.empty()) return;
    ctx();
    if (g_batch_depth > 0) {
        // A batch started from another batch's progress callback (the per-fold wMetaC and the sMetaC of a finished block while later
        // chunks of the outer batch are in flight): one chunk on the current stream, with the third set of buffers and its OWN
        // agglomeration scratch -- the outer batch's chunks own sets 0 and 1 and share set 0's scratch.
        SHARP_REQUIRE(!progress && tasks.size() <= static_cast<size_t>(ctx().num_cu) * 4, "get_opt_hclust: nested batch too large");
        ChunkJob J;
        J.i0 = 0; J.i1 = tasks.size();
        J.slot = 2; J.scratch_slot = 2; J.one_range = true;
        setup_chunk(tasks, J);
        plan_add(J, true);
        enqueue_chunk(J, PH_ALL);
        finish_chunk(tasks, J, want_v, out, want_status);
        return;
    }
    size_t free_b = 0, total_b = 0;
    { HostTimer ht("hc_mem_info"); SHARP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b)); }
    const double budget = std::max(0.5 * static_cast<double>(free_b), 2.0e9);
    // More tasks than CUs: equal chunks of at most one task per CU.  The agglomeration kernel then runs its 1024-thread form
    // (one task per CU, twice the loads in flight) chunk after chunk -- as fast as all tasks at once with two per CU -- and the
    // workspaces (three distance-matrix-sized buffers per task) are sized for a chunk: 18 GB instead of 36 GB at cfg2, which
    // is what the first call pays in hipMalloc time.
    size_t max_tasks = tasks.size();
    {
        const size_t ncu = static_cast<size_t>(ctx().num_cu);
        if (knobs().hc_chunk > 0) max_tasks = static_cast<size_t>(knobs().hc_chunk);
        else if (tasks.size() > ncu) {
            size_t nch = (tasks.size() + ncu - 1) / ncu;
            // Many chunks (the blocks of a SHARP_unlimited call as one batch): what counts is the steady state, where chunk j + 1's distance
            // GEMM has only the CUs chunk j's agglomeration leaves free -- with 250 tasks per chunk that is 6 CUs and the two run one after
            // the other (36 ms per chunk); at most 3/4 of the CUs per chunk leaves the GEMM a quarter of the chip (18 ms per chunk of 179).
            // Two chunks (cfg2, cfg4's share) are better off as large as they can be: an agglomeration of 137 tasks takes as long as one of 188.
            if (nch >= 3) nch = (tasks.size() + ncu * 3 / 4 - 1) / (ncu * 3 / 4);
            max_tasks = (tasks.size() + nch - 1) / nch;
        }
    }
    std::vector<std::pair<size_t, size_t>> bounds;
    size_t i0 = 0;
    // SHARP_HC_FIRST_CHUNK=n: a first chunk of n tasks (its distance GEMM has the chip to itself and nothing to run beside: a short one
    // starts the first agglomeration earlier), the rest in equal chunks as above
    // (cfg3, 1250 tasks: 140 + 7 x 159 against 7 x 179: 162.2 against 164.4 ms per call, medians of 7 and 8 interleaved runs; a first chunk
    // of at most kHcSplitMaxTasks tasks takes the round-per-launch agglomeration, which wants the whole chip: 173 ms.)  Default with three
    // chunks or more: four fifths of a chunk, above that threshold; SHARP_HC_FIRST_CHUNK=-1: equal chunks.
    size_t first_tasks = 0;
    int first_knob = knobs().hc_first_chunk;
    if (first_knob == 0 && knobs().hc_chunk <= 0 && tasks.size() > 2 * max_tasks)
        first_knob = std::max(kHcSplitMaxTasks + 4, static_cast<int>(max_tasks) * 4 / 5);
    if (first_knob > 0 && static_cast<size_t>(first_knob) < max_tasks && tasks.size() > max_tasks) {
        first_tasks = static_cast<size_t>(first_knob);
        const size_t rest = tasks.size() - first_tasks, nch = (rest + max_tasks - 1) / max_tasks;
        max_tasks = (rest + nch - 1) / nch;
    }
    while (i0 < tasks.size()) {
        double bytes = 0;
        size_t i1 = i0;
        while (i1 < tasks.size() && i1 - i0 < (i0 == 0 && first_tasks ? first_tasks : max_tasks)) {
            const HcTask &t = tasks[i1];
            const double nld = static_cast<double>(rup(t.n, 128));
            const double p = t.symmetric ? t.n : t.p;
            const double b = 8.0 * (nld * nld * (t.symmetric ? 4 : 3) + 2 * nld * p + 4.0 * 64 * t.n) + 4.0 * 64 * t.n;   // D, two scratch matrices (+ D0)
            if (i1 > i0 && bytes + b > budget) break;
            bytes += b;
            ++i1;
        }
        bounds.push_back({i0, i1});
        i0 = i1;
    }
    // Several chunks: two in flight.  Chunk j + 1's row preparation and distance GEMM (MFMA-bound) run beside chunk j's
    // agglomeration (HBM-bound, one workgroup per task holding a whole CU: 188 of 256 CUs at cfg2) on the CUs that one leaves free,
    // chunk j's cutree / cluster sums / silhouette statistics beside chunk j + 1's agglomeration, and the host's level selection and
    // label download of chunk j under chunk j + 1's device work.  SHARP_HC_PIPE=0: one chunk at a time.
    const bool pipe = bounds.size() > 1 && knobs().hc_pipe;
    if (!pipe) {
        if (prepare) (void)(*prepare)(tasks.size());                         // (everything on the caller's stream: its order is the dependency)
        for (const auto &b : bounds) {
            ChunkJob J;
            J.i0 = b.first; J.i1 = b.second;
            { HostTimer ht("hc_single_setup"); setup_chunk(tasks, J); plan_add(J, false); }
            { HostTimer ht("hc_single_enqueue"); enqueue_chunk(J, PH_ALL); }
            { HostTimer ht("hc_single_finish"); finish_chunk(tasks, J, want_v, out, want_status); }
        }
        return;
    }
    SHARP_HIP_CHECK(hipEventRecord(pipe_events().in, ctx().stream));        // the tasks' inputs are ready
    // Two chunks: two sets of buffers, host order  dist(0) agglo(0) | dist(1) stats(0) agglo(1) | fetch(0) fetch(1).
    // Three chunks or more: THREE sets in rotation (0, 1, 3), host order  ... | dist(j) stats(j-1) agglo(j) fetch(j-2) | ... : with two sets
    // chunk j's distance GEMM could only be enqueued once chunk j - 2's statistics -- which run beside chunk j - 1's agglomeration -- had
    // been fetched, i.e. when that agglomeration was over: GEMM and agglomeration then took turns (27.5 ms per chunk of 179 tasks).
    auto call_progress = [&](size_t done) {
        if (!progress) return;
        ++g_batch_depth;
        try { (*progress)(done); } catch (...) { --g_batch_depth; throw; }
        --g_batch_depth;
    };
    const size_t nb = bounds.size();
    const size_t R = nb >= 3 ? 3 : 2;
    static const int slot_of[3] = {0, 1, 3};
    ChunkJob jobs[3];
    size_t fetched = 0;                                                     // chunks 0 .. fetched - 1 are finished
    auto fetch_upto = [&](size_t upto) {                                    // finish chunks in order, report
        for (; fetched < upto; ++fetched) { finish_chunk(tasks, jobs[fetched % R], want_v, out, want_status); step_mark("chunk fetched", static_cast<int>(fetched)); }
    };
    auto start_chunk = [&](size_t j) {                                      // descriptors, uploads, rows and distance matrices of chunk j
        ChunkJob &J = jobs[j % R];
        J = ChunkJob();
        J.i0 = bounds[j].first; J.i1 = bounds[j].second;
        J.slot = slot_of[j % R]; J.prev_slot = slot_of[(j + R - 1) % R]; J.next_slot = slot_of[(j + 1) % R];
        J.pipe = true; J.first = j == 0; J.has_next = j + 1 < nb;
        if (prepare) J.input_ready = (*prepare)(J.i1);                    // (whatever prepare_ahead has not asked for already)
        setup_chunk(tasks, J);
        plan_add(J, false);
        enqueue_chunk(J, PH_DIST);
    };
    const bool stats_last = R == 3;
    try {
    start_chunk(0);
    for (size_t j = 0; j < nb; ++j) {
        if (j >= 1 && !stats_last) enqueue_chunk(jobs[(j - 1) % R], PH_STATS);
        enqueue_chunk(jobs[j % R], PH_AGGLO);
        step_mark("agglomeration enqueued, chunk", static_cast<int>(j));
        // the inputs of the chunk after the next are asked for NOW, behind this agglomeration's launch: start_chunk(j + 1) below has to wait
        // for chunk j - 2's statistics first (its buffers), and inputs produced only then sat on the critical path in front of that chunk's GEMM
        if (prepare && j + 2 < nb) (void)(*prepare)(bounds[j + 2].second);
        if (j + 1 == nb && after_agglo().fn && g_batch_depth == 0) {        // the caller's side work behind the last agglomeration
            std::function<void(hipEvent_t)> fn = std::move(after_agglo().fn);
            after_agglo().fn = nullptr;
            fn(pipe_events().hc[jobs[j % R].slot]);
            after_agglo().fired = true;
        }
        // chunk j - 2's statistics ran beside chunk j - 1's agglomeration: fetched now, which also frees its set for chunk j + 1, whose
        // distance matrices are enqueued at once (they wait, on the device, for chunk j's GEMM); then the caller's work on finished
        // tasks, with chunk j's agglomeration and chunk j + 1's GEMM for the device to chew on
        if (R == 3 && j >= 2) fetch_upto(j - 1);
        if (j + 1 < nb) start_chunk(j + 1);
        // three sets: chunk j - 1's statistics go behind chunk j + 1's distance GEMM as well -- that GEMM decides when the next agglomeration
        // can start, the statistics only when a finished block's tail can; beside one agglomeration both crawled
        if (j >= 1 && stats_last) {
            ChunkJob &P = jobs[(j - 1) % R];
            P.next2_slot = j + 1 < nb ? jobs[(j + 1) % R].slot : -1;
            enqueue_chunk(P, PH_STATS);
        }
        if (fetched > 0) call_progress(bounds[fetched - 1].second);
    }
    enqueue_chunk(jobs[(nb - 1) % R], PH_STATS);
    if (nb >= 2) { fetch_upto(nb - 1); call_progress(bounds[nb - 2].second); }
    fetch_upto(nb);
    } catch (...) {
        (void)hipDeviceSynchronize();                                       // chunks are in flight on their own streams: nothing of this batch
        throw;                                                              // may still be running when the caller sees the error
    }
}

// ---- a batch whose distance matrices are built ahead of time (SHARP_unlimited: the next block's front under the current block's tail)
struct HcPrefetch {
    std::vector<HcTask> tasks;
    ChunkJob J;
    hipEvent_t ready = nullptr, agglo_done = nullptr;
    bool agglo_enqueued = false;
    ~HcPrefetch() { if (ready) (void)hipEventDestroy(ready); if (agglo_done) (void)hipEventDestroy(agglo_done); }
};

bool hc_prefetch_possible(const std::vector<HcTask> &tasks) {
    if (tasks.empty() || tasks.size() > static_cast<size_t>(ctx().num_cu) || knobs().hc_chunk > 0) return false;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    double bytes = 0;
    for (const HcTask &t : tasks) {
        const double nld = static_cast<double>(rup(t.n, 128));
        bytes += 8.0 * (nld * nld * 4 + 2 * nld * (t.symmetric ? t.n : t.p));
    }
    return bytes < 0.25 * static_cast<double>(free_b);          // (always against the memory that is free NOW: the GPU may be shared)
}

std::shared_ptr<HcPrefetch> hc_prefetch_begin(std::vector<HcTask> tasks, int slot) {
    auto P = std::make_shared<HcPrefetch>();
    P->tasks = std::move(tasks);
    P->J.i0 = 0; P->J.i1 = P->tasks.size();
    P->J.slot = 4 + (slot & 1);
    P->J.one_range = true;
    setup_chunk(P->tasks, P->J);
    enqueue_chunk(P->J, PH_DIST);                           // on the stream that is current here (the caller's prefetch stream)
    SHARP_HIP_CHECK(hipEventCreateWithFlags(&P->ready, hipEventDisableTiming));
    SHARP_HIP_CHECK(hipEventRecord(P->ready, ctx().stream));
    return P;
}

hipEvent_t hc_prefetch_agglomerate(HcPrefetch &P) {
    SHARP_HIP_CHECK(hipStreamWaitEvent(ctx().stream, P.ready, 0));
    if (!P.agglo_done) SHARP_HIP_CHECK(hipEventCreateWithFlags(&P.agglo_done, hipEventDisableTiming));
    // round-per-launch form: the event sits behind the large rounds (the first eight move 3/4 of the bytes); the remaining small
    // rounds leave most of the chip idle, and the next block's front may as well start there
    P.J.mid_event = P.agglo_done;
    enqueue_chunk(P.J, PH_AGGLO);
    P.J.mid_event = nullptr;
    if (!P.J.mid_recorded) SHARP_HIP_CHECK(hipEventRecord(P.agglo_done, ctx().stream));
    P.agglo_enqueued = true;
    return P.agglo_done;
}

void hc_prefetch_stamp_block(HcPrefetch &P, int block) { for (HcTask &t : P.tasks) t.prm.dec_block = block; }   // (decision log: the call that uses the batch names its block)
void hc_prefetch_finish(HcPrefetch &P, bool want_v, std::vector<HcResult> &out) {
    out.assign(P.tasks.size(), HcResult());
    if (!P.agglo_enqueued) hc_prefetch_agglomerate(P);
    enqueue_chunk(P.J, PH_STATS);
    finish_chunk(P.tasks, P.J, want_v, out, false);
}

// stats::hclust alone: one distance task through setup_chunk / enqueue_chunk (rows copied as they are, agglomeration), no statistics
void hclust_tree(const double *d_dist, long long ld, int n, int hmethod, HcTree &out) {
    Ctx &c = ctx();
    SHARP_REQUIRE(d_dist && n >= 3 && n <= kHcMaxN && ld >= n, "hclust: bad arguments");
    HcTask tk;
    tk.d_mat = d_dist; tk.ld = ld; tk.n = n; tk.p = n; tk.symmetric = true; tk.distance = true;
    tk.prm.hmethod = hmethod;
    tk.prm.N_cluster = 2;                                   // (sizes the unused statistics buffers at their smallest)
    std::vector<HcTask> tasks{tk};
    ChunkJob J;
    J.i0 = 0; J.i1 = 1; J.one_range = true;
    setup_chunk(tasks, J);
    enqueue_chunk(J, PH_DIST | PH_AGGLO);
    Workspace &W = ws(J.slot);
    out.ia.assign(n - 1, 0); out.ib.assign(n - 1, 0); out.crit.assign(n - 1, 0.0);
    int st = 1;
    if (!knobs().hc_seq) W.status.download(&st, 1);
    out.sequential = st != 0;
    W.ia.download(out.ia.data(), n - 1);
    W.ib.download(out.ib.data(), n - 1);
    W.height.download(out.crit.data(), n - 1);
    if (c.profiling) c.stats[out.sequential ? "host:hclust_tasks_sequential" : "host:hclust_tasks_bulk_synchronous"].launches += 1;
    if (static_cast<size_t>(J.metas[0].nld) * J.metas[0].nld > (64u << 20)) {   // three matrices of more than 512 MB each: not kept between calls
        Workspace &W0 = ws(J.scratch_slot);
        W.D.release(); W0.S0.release(); W0.S1.release();
    }
}

}  // namespace sharp

using namespace sharp;

// ---------------------------------------------------------------------------------------------
// C ABI: single-problem wrappers (the reference's exported functions take one matrix at a time)
// ---------------------------------------------------------------------------------------------
namespace {

bool host_is_symmetric(const double *mat, int n, int p) {   // isSymmetric(): square + all.equal(m, t(m), 100*eps)
    if (n != p) return false;
    long double num = 0, den = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            num += fabsl(static_cast<long double>(mat[static_cast<size_t>(i) * n + j]) - mat[static_cast<size_t>(j) * n + i]);
            den += fabsl(static_cast<long double>(mat[static_cast<size_t>(i) * n + j]));
        }
    const double tol = 100 * 2.220446049250313e-16;
    long double xy = num;
    if (den > 0 && den / (static_cast<long double>(n) * n) > tol) xy = num / den;
    return xy < tol;
}

}  // namespace

extern "C" {

int sharp_get_opt_hclust(const double *mat, int n, int p, int hmethod, int N_cluster, int minN, int maxN, double sil_thre,
                         double height_Ntimes, int *f, int *v, double *msil, double *CHind, double *maxsil, double *height,
                         int *optN, int *nk, int *branch) {
    int warn = 0;
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(mat && f, "sharp_get_opt_hclust: null argument");
    SHARP_REQUIRE(n >= 3 && p >= 1, "sharp_get_opt_hclust: need n >= 3 and p >= 1");
    if (N_cluster != 0) {
        SHARP_REQUIRE(N_cluster >= 2, "The given N.cluster is less than 2, which is not suitable for clustering!");
    }
    HcTask t;
    t.n = n; t.p = p; t.ld = p;
    t.symmetric = host_is_symmetric(mat, n, p);
    t.prm.hmethod = hmethod > 0 ? hmethod : 1;
    t.prm.N_cluster = N_cluster;
    t.prm.minN = minN > 0 ? minN : 2;
    t.prm.maxN = maxN > 0 ? maxN : 40;
    t.prm.sil_thre = sil_thre;
    t.prm.height_Ntimes = height_Ntimes > 0 ? height_Ntimes : 2.0;
    DevBuf<double> dm(static_cast<size_t>(n) * p);
    dm.upload(mat, static_cast<size_t>(n) * p);
    t.d_mat = dm.p;
    std::vector<HcTask> tasks{t};
    std::vector<HcResult> res;
    get_opt_hclust_batch(tasks, v != nullptr, res);
    HcResult &R = res[0];
    warn = R.rc;
    std::copy(R.f.begin(), R.f.end(), f);
    if (v) std::copy(R.v.begin(), R.v.end(), v);
    if (N_cluster > 0) {
        // CH of the N.cluster branch is clusterCrit's Euclidean index on the (scaled) matrix
        std::vector<double> y(mat, mat + static_cast<size_t>(n) * p);
        if (!t.symmetric) {
            for (int i = 0; i < n; ++i) {
                double *r = y.data() + static_cast<size_t>(i) * p;
                long double s = 0; for (int k = 0; k < p; ++k) s += r[k];
                const double mean = static_cast<double>(s / p);
                long double ss = 0; for (int k = 0; k < p; ++k) { r[k] -= mean; ss += static_cast<long double>(r[k] * r[k]); }
                const double sd = std::sqrt(static_cast<double>(ss) / std::max(1, p - 1));
                for (int k = 0; k < p; ++k) r[k] /= sd;
            }
        }
        R.CHind[0] = host_ch_euclid(y.data(), n, p, R.f.data(), R.optN);
        R.optN = N_cluster;
    }
    if (msil) std::copy(R.msil.begin(), R.msil.end(), msil);
    if (CHind) std::copy(R.CHind.begin(), R.CHind.end(), CHind);
    if (height) std::copy(R.height.begin(), R.height.end(), height);
    if (maxsil) *maxsil = R.maxsil;
    if (optN) *optN = R.optN;
    if (nk) *nk = R.nk;
    if (branch) *branch = R.branch;
    }
    catch (const sharp::Error &e) { sharp::set_error(e.what()); return e.code; }
    catch (const std::exception &e) { sharp::set_error(e.what()); return SHARP_ERR; }
    return warn;
}

/* Test entry: `count` tasks through ONE get_opt_hclust_batch call (include/sharp_hip.h). */
int sharp_get_opt_hclust_batch(int count, const int *n, const int *p, const int *kind, const int *hmethod, const int *N_cluster,
                               const int *minN, const int *maxN, const double *sil_thre, const double *height_Ntimes, const double *mats,
                               int want_v, int nested, int *f, int *v, double *msil, double *CHind, double *height, int *optN, int *nk,
                               int *branch, int *rc, int *sequential) {
    SHARP_API_BEGIN
    ctx();
    const std::string w = "sharp_get_opt_hclust_batch";
    SHARP_REQUIRE(count >= 1, w + ": count must be at least 1");
    SHARP_REQUIRE(n && p && kind && hmethod && N_cluster && minN && maxN && sil_thre && height_Ntimes && mats, w + ": null input");
    SHARP_REQUIRE(f && msil && CHind && height && optN && nk && branch && rc && sequential && (v || !want_v), w + ": null output");
    SHARP_REQUIRE(!nested || static_cast<size_t>(count) <= static_cast<size_t>(ctx().num_cu) * 4, w + ": nested needs count <= 4 * CUs");
    // offsets of every task in the matrices and in each output; the sets of outputs (two with `nested`) follow one another
    std::vector<size_t> oMat(count + 1, 0), oF(count + 1, 0), oV(count + 1, 0), oK(count + 1, 0), oH(count + 1, 0);
    for (int t = 0; t < count; ++t) {
        SHARP_REQUIRE(n[t] >= 1 && p[t] >= 1, w + ": n and p of every task must be at least 1");
        SHARP_REQUIRE(kind[t] == 0 || (kind[t] == 1 && p[t] == n[t]), w + ": kind must be 0 (feature rows) or 1 (similarity, p == n)");
        const int nk_t = N_cluster[t] > 0 ? 1 : std::max(1, std::min(maxN[t], n[t] - 1) - minN[t] + 1);
        oMat[t + 1] = oMat[t] + static_cast<size_t>(n[t]) * p[t];
        oF[t + 1] = oF[t] + n[t];
        oV[t + 1] = oV[t] + static_cast<size_t>(nk_t) * n[t];
        oK[t + 1] = oK[t] + nk_t;
        oH[t + 1] = oH[t] + n[t] - 1;
    }
    const size_t sets = nested ? 2 : 1;
    double nan_sentinel;
    const unsigned long long bits = 0x7ff8c0de5eed0001ULL;     // (the sentinel of the linalg batch entries)
    std::memcpy(&nan_sentinel, &bits, sizeof bits);
    std::fill_n(f, sets * oF[count], INT_MIN);
    if (want_v) std::fill_n(v, sets * oV[count], INT_MIN);
    std::fill_n(msil, sets * oK[count], nan_sentinel);
    std::fill_n(CHind, sets * oK[count], nan_sentinel);
    std::fill_n(height, sets * oH[count], nan_sentinel);
    for (int *o : {optN, nk, branch, rc, sequential}) std::fill_n(o, sets * count, INT_MIN);
    // every matrix in a device buffer of its own, as sharp_get_opt_hclust uploads its one
    std::vector<DevBuf<double>> dm(count);
    std::vector<HcTask> tasks(count);
    for (int t = 0; t < count; ++t) {
        dm[t].alloc(oMat[t + 1] - oMat[t]);
        dm[t].upload(mats + oMat[t], oMat[t + 1] - oMat[t]);
        HcTask &tk = tasks[t];
        tk.d_mat = dm[t].p; tk.n = n[t]; tk.p = p[t]; tk.ld = p[t];
        tk.symmetric = kind[t] == 1;
        tk.prm.hmethod = hmethod[t]; tk.prm.N_cluster = N_cluster[t]; tk.prm.minN = minN[t]; tk.prm.maxN = maxN[t];
        tk.prm.sil_thre = sil_thre[t]; tk.prm.height_Ntimes = height_Ntimes[t];
    }
    // results of tasks [t0, t0 + res.size()) into output set `set`: what a result does not hold stays the sentinel
    auto store = [&](const std::vector<HcResult> &res, size_t t0, size_t set) {
        for (size_t i = 0; i < res.size(); ++i) {
            const HcResult &R = res[i];
            const size_t t = t0 + i;
            auto fits = [](size_t have, size_t room) { return std::min(have, room); };
            std::copy_n(R.f.begin(), fits(R.f.size(), oF[t + 1] - oF[t]), f + set * oF[count] + oF[t]);
            if (want_v) std::copy_n(R.v.begin(), fits(R.v.size(), oV[t + 1] - oV[t]), v + set * oV[count] + oV[t]);
            std::copy_n(R.msil.begin(), fits(R.msil.size(), oK[t + 1] - oK[t]), msil + set * oK[count] + oK[t]);
            std::copy_n(R.CHind.begin(), fits(R.CHind.size(), oK[t + 1] - oK[t]), CHind + set * oK[count] + oK[t]);
            std::copy_n(R.height.begin(), fits(R.height.size(), oH[t + 1] - oH[t]), height + set * oH[count] + oH[t]);
            const size_t o = set * count + t;
            if (R.f.empty()) continue;                      // (a task the batch never reached)
            optN[o] = R.optN; nk[o] = R.nk; branch[o] = R.branch; rc[o] = R.rc;
            if (R.sequential >= 0) sequential[o] = R.sequential;
        }
    };
    std::vector<HcResult> res;
    // nested: the tasks that the outer batch reports finished run again, from its progress callback, as a batch of their own (slot 2)
    size_t redone = 0;
    const std::function<void(size_t)> progress = [&](size_t done) {
        if (done <= redone) return;
        std::vector<HcTask> part(tasks.begin() + redone, tasks.begin() + done);
        std::vector<HcResult> again;
        get_opt_hclust_batch(part, want_v != 0, again, nullptr, nullptr, true);
        store(again, redone, 1);
        redone = done;
    };
    get_opt_hclust_batch(tasks, want_v != 0, res, nested ? &progress : nullptr, nullptr, true);
    store(res, 0, 0);
    stream_sync();                                          // (dm goes away)
    SHARP_API_END
}

int sharp_hclust_batch_plan(int *rows, int cap_rows, int *n_rows) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(n_rows && (rows || cap_rows == 0) && cap_rows >= 0, "sharp_hclust_batch_plan: null argument");
    *n_rows = hc_batch_plan_fetch(rows, cap_rows);
    SHARP_API_END
}

/* the decision log (hclust.hpp says what a row holds) */
int sharp_decision_log(int enable) {
    SHARP_API_BEGIN
    decision_log_set(enable != 0);
    SHARP_API_END
}
int sharp_last_decisions(double *rows, int cap_rows, int *n_rows) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(n_rows && (rows || cap_rows == 0) && cap_rows >= 0, "sharp_last_decisions: null argument");
    *n_rows = decision_log_fetch(rows, cap_rows);
    SHARP_API_END
}

int sharp_getrowColor(const double *E, int n, int p, int hmethod, int indN_cluster, int minN, int maxN, double sil_thre,
                      double height_Ntimes, int *rowColor, double *maxsil) {
    std::vector<int> f(static_cast<size_t>(n > 0 ? n : 1));
    const int rc = sharp_get_opt_hclust(E, n, p, hmethod, indN_cluster, minN, maxN, sil_thre, height_Ntimes > 0 ? height_Ntimes : 1.0,
                                        f.data(), nullptr, nullptr, nullptr, maxsil, nullptr, nullptr, nullptr, nullptr);
    if (rc != SHARP_OK && rc != SHARP_WARN_RANGE) return rc;
    // colorL has 40 names; cluster j > 40 wraps onto colour ((j-1) %% 40) + 1 (R/getrowColor.R:59-68)
    for (int i = 0; i < n; ++i) rowColor[i] = f[i] > 40 ? ((f[i] - 1) % 40) + 1 : f[i];
    return rc;
}

}  // extern "C"
