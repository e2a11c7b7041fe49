// unlimited.hip -- SHARP_unlimited (R/SHARP_unlimited.R:29-242, row a11) and SHARP_unlimited2 (R/SHARP_unlimited2.R:29-292): everything
// that concerns a LIST of blocks.  A block itself -- SHARP() on it, its table of cluster centroids, a window of blocks as one pipelined
// batch -- is driver.hip (driver.hpp); here are
//   the view of a call (the arm of sharp_unlimited_view_dim, take_view / make_view),
//   the call header (p from the global cell count, ensize.K, the projector seeds),
//   the blocks of one GPU in turn (unlimited_blocks_loop), the cross-block sMetaC on their centroids (unlimited_merge) and the relabel,
//   the three runs: resident blocks (unlimited_run), SHARP_unlimited2 (unlimited2_run), blocks dealt to several GPUs with their
//   uploads beside the clustering (unlimited_run_multi, its Feed and timeline),
//   and every sharp_unlimited_* / sharp_SHARP_unlimited* entry point.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <ctime>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "driver.hpp"
#include "meta.hpp"
#include "projector.hpp"
#include "upload.hpp"

namespace sharp {

// Which view a call takes (the reduction itself: unlimited_block_summary, driver.hip).  The entries that carry a view_dim argument say so
// themselves; for the others sharp_unlimited_view_dim() arms it for the NEXT SHARP_unlimited call OF THE CALLING THREAD (the arm is
// thread-local: a call on another thread never takes it, and nothing of a running call is shared).  take_view() at the top of a run
// turns the arm into that run's ViewCall -- whatever the run then does, the arm is spent.
thread_local int tl_view_pending = 0;
static double fresh_view_seed() {                        // an unseeded run: one integer seed for the call's z0 (set.seed() of a random word)
    std::random_device rd;
    return static_cast<double>(rd() & 0x7fffffffu);
}
static ViewCall make_view(int kdim, double rN_seed, int K) {
    ViewCall v;
    v.kdim = kdim > 0 ? kdim : 0;
    // `50 + rN.seed + k` at :222 reads a `k` that only exists inside the foreach at :96 (an R error whenever a seed
    // is given); fixed as the next seed of that sequence, k = ensize.K + 1
    if (v.kdim > 0) v.seed = rN_seed == 0.5 ? fresh_view_seed() : 50 + rN_seed + K + 1;
    return v;
}
static ViewCall take_view(double rN_seed, int K) {
    const int kdim = tl_view_pending;
    tl_view_pending = 0;
    return make_view(kdim, rN_seed, K);
}

inline int ensemble_size(int ensize_K) { return ensize_K > 0 ? ensize_K : 5; }                                 // :92-94, unlimited2 :39-41

// What every run derives from its arguments before it touches a block: p from the GLOBAL cell count unless the caller names it
// (:65-66, unlimited2 :42-44), ensize.K, and the K projector seeds (:97-104, unlimited2 :130-137) -- after the refusal of a seed that
// is no integer (:80-90, unlimited2 :117-127).
struct CallHeader { int p = 0, K = 0; std::vector<double> seeds; };
static CallHeader call_header(long long ncells, int ensize_K, int reduced_ndim, double rN_seed) {
    if (rN_seed != 0.5) SHARP_REQUIRE(std::fmod(rN_seed, 1.0) == 0.0, "The rN.seed should be an integer!");
    CallHeader h;
    h.p = reduced_ndim > 0 ? reduced_ndim : static_cast<int>(std::ceil(std::log2(static_cast<double>(ncells)) / (0.2 * 0.2)));
    h.K = ensemble_size(ensize_K);
    h.seeds.resize(h.K);
    for (int k = 0; k < h.K; ++k) h.seeds[k] = (rN_seed == 0.5) ? 0.5 : 50 + rN_seed + (k + 1);
    return h;
}

inline bool lex_less_id(int a, int b) {
    char sa[16], sb[16];
    snprintf(sa, sizeof sa, "%d", a);
    snprintf(sb, sizeof sb, "%d", b);
    return strcmp(sa, sb) < 0;
}

// cross-block sMetaC on the gathered centroids, small-cluster merge and size-ordered relabel (:163-183)
void unlimited_merge(const double *means, const long long *counts, int nC, int p, long long ncells, int N_cluster, int minN, int maxN,
                     std::vector<int> &final_id, int &n_final, int hmethod = 1, double sil_thre = 0.35, double height_Ntimes = 2.0) {
    HcParams prm;                                                               // hmethod/sil.thre/height.Ntimes of y[[1]]$paras = defaults
    prm.hmethod = hmethod; prm.N_cluster = N_cluster;
    prm.minN = minN > 0 ? minN : 2;                                             // :70-72
    prm.maxN = maxN > 0 ? maxN : static_cast<int>(std::max<long long>(40, (ncells + 4999) / 5000));   // :75-77
    prm.sil_thre = sil_thre; prm.height_Ntimes = height_Ntimes;
    prm.dec_level = 3;
    DevBuf<double> dm;                                                          // (from the block cache: no hipMalloc / hipFree per call; smetac_from_means
    dm.alloc_pooled(static_cast<size_t>(nC) * p);                               //  returns with its stream drained, so the block may go back)
    dm.upload(means, static_cast<size_t>(nC) * p);
    SmResult sr = smetac_from_means(dm.p, nC, p, ncells, prm);
    final_id = sr.tf;
    int mx = *std::max_element(final_id.begin(), final_id.end());
    std::vector<long long> cnt(mx + 1, 0);
    for (int q = 0; q < nC; ++q) cnt[final_id[q]] += counts[q];
    if (N_cluster <= 0 && ncells > 10000) {                                     // :168-177
        int mn = -1;
        for (int q = 1; q <= mx; ++q) if (cnt[q] > 0 && cnt[q] < 10) { mn = q; break; }
        if (mn >= 0) {
            for (int &v : final_id) if (cnt[v] < 10) v = mn;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int q = 0; q < nC; ++q) cnt[final_id[q]] += counts[q];
        }
    }
    // x = sort(table(finalrowColor), decreasing = TRUE): size order, ties in string order of the ids (:180-183)
    std::vector<int> ids;
    for (int q = 1; q <= mx; ++q) if (cnt[q] > 0) ids.push_back(q);
    std::stable_sort(ids.begin(), ids.end(), [&](int x, int y) { return lex_less_id(x, y); });
    std::stable_sort(ids.begin(), ids.end(), [&](int x, int y) { return cnt[x] > cnt[y]; });
    std::vector<int> map(mx + 1, 0);
    for (size_t q = 0; q < ids.size(); ++q) map[ids[q]] = static_cast<int>(q) + 1;
    for (int &v : final_id) v = map[v];
    n_final = static_cast<int>(ids.size());
}

// The end of every run (:163-183): the tables of all blocks, in block order, through ONE merge, and every block's labels through the
// merge's map into the caller's pred (the blocks' cells one behind the other).  Returns the number of final clusters.
static int merge_and_relabel(const std::vector<BlockTable> &tabs, int p, int N_cluster, int minN, int maxN, int *pred, int hmethod = 1,
                             double sil_thre = 0.35, double height_Ntimes = 2.0) {
    const int nblocks = static_cast<int>(tabs.size());
    std::vector<double> means;
    std::vector<long long> counts;
    std::vector<int> first(nblocks + 1, 0);               // block b's rows of the gathered table: [first[b], first[b + 1])
    std::vector<long long> offs(nblocks + 1, 0);          // and its cells
    for (int b = 0; b < nblocks; ++b) {
        means.insert(means.end(), tabs[b].means.begin(), tabs[b].means.end());
        counts.insert(counts.end(), tabs[b].counts.begin(), tabs[b].counts.end());
        first[b + 1] = first[b] + static_cast<int>(tabs[b].counts.size());
        offs[b + 1] = offs[b] + static_cast<long long>(tabs[b].pred.size());
    }
    step_mark("blocks done, projector dropped: merge of centroids", first[nblocks]);
    std::vector<int> fid;
    int nf = 0;
    unlimited_merge(means.data(), counts.data(), first[nblocks], p, offs[nblocks], N_cluster, minN, maxN, fid, nf, hmethod, sil_thre, height_Ntimes);
    step_mark("merge done, clusters", nf);
    host_parallel_for(nblocks, 16, [&](int b) {                  // (every block's cells through the merge's map: 0.3 ms for 500 000 cells on one thread)
        int *pb = pred + offs[b];
        const int *map = fid.data() + first[b], *lab = tabs[b].pred.data();
        for (long long i = 0; i < offs[b + 1] - offs[b]; ++i) pb[i] = map[lab[i] - 1];
    });
    return nf;
}

// The blocks of a SHARP_unlimited call (R/SHARP_unlimited.R:125-149) on one GPU, each one the SHARP() call of :135: several large-path
// blocks whose base tasks outnumber the CUs go as ONE pipelined batch (unlimited_batch_window), in windows of at most ~16 GB of
// projections; SHARP_UNLIMITED_BATCH=0 or blocks that do not qualify: block after block, each preparing the next under its tail.
// take(b, table) is called once per block, in block order; the table is the callee's to move from.
static void unlimited_blocks_loop(const XRef *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m, int p, int proj, int K,
                                  double rN_seed, double *const *viE_of,   // NULL, or per block where its E1 rows go (NULL: not wanted)
                                  const ViewCall &view, const std::function<void(int, BlockTable &)> &take,
                                  const int *gids = nullptr,     // (decision log: the blocks' indices in the caller's list; NULL: 0, 1, ...)
                                  bool small_windows = false) {  // a batch also for a few blocks whose tasks merely fill the chip (host blocks taken as they arrive)
    int b = 0;
    while (b < nblocks) {                                                                                  // :125-149
        // Several large-path blocks whose base tasks outnumber the CUs: one pipelined batch (unlimited_batch_window), in windows of
        // at most ~16 GB of projections.  SHARP_UNLIMITED_BATCH=0: block after block, each preparing the next under its tail.
        int e = b;
        long long rows = 0, ntasks = 0;
        long long window_bytes = 16LL << 30;
        if (knobs().unlimited_window_mb > 0) window_bytes = static_cast<long long>(knobs().unlimited_window_mb) << 20;   // (tests: several windows)
        if (knobs().unlimited_batch) {
            while (e < nblocks && ncb[e] >= 5000 && ncb[e] < (1LL << 31) &&
                   (rows + ncb[e]) * static_cast<long long>(K) * p * 8 <= window_bytes) {
                rows += ncb[e];
                ntasks += static_cast<long long>(K) * ((ncb[e] + 1999) / 2000);
                ++e;
            }
        }
        if (e - b >= 2 && ntasks > (small_windows ? 3LL * ctx().num_cu / 4 : 2LL * ctx().num_cu)) {
            std::vector<BlockTable> got(e - b);                             // (the window's tails finish on helper threads, in any order)
            unlimited_batch_window(dX_blocks, ncb, ldb, b, e, m, p, proj, K, rN_seed, viE_of, view, got.data(), gids);
            for (int q = b; q < e; ++q) take(q, got[q - b]);
            b = e;
            continue;
        }
        BlockTable t;
        const bool more = b + 1 < nblocks;
        unlimited_block_dev(dX_blocks[b], m, ncb[b], ldb[b], p, proj, K, rN_seed, t, viE_of ? viE_of[b] : nullptr, view, 1, nullptr,
                            more ? dX_blocks[b + 1] : XRef(), more ? ncb[b + 1] : 0, more ? ldb[b + 1] : 0, gids ? gids[b] : b);
        take(b, t);
        ++b;
    }
}

}  // namespace sharp

using namespace sharp;

// SHARP_unlimited on resident blocks (fp32 or fp64 each)
static int unlimited_run(const XRef *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                         int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used,
                         double *viE, const ViewCall *view_in = nullptr) {
    SHARP_API_BEGIN
    const ViewCall view = view_in ? *view_in : take_view(rN_seed, ensemble_size(ensize_K));   // (first: a call that fails its argument checks spends the arm too)
    ctx();
    SHARP_REQUIRE(dX_blocks && ncb && ldb && pred, "The input should be a LIST of partitioned scRNA-seq expression matrices!");
    SHARP_REQUIRE(nblocks >= 2, "SHARP is used instead of SHARP_unlimited because the length of the input is 1!");
    long long ncells = 0;
    for (int b = 0; b < nblocks; ++b) ncells += ncb[b];
    const CallHeader h = call_header(ncells, ensize_K, 0, rN_seed);
    const int p = h.p, K = h.K;
    step_mark("SHARP_unlimited begins, blocks", nblocks);
    shuffle_ahead(ncb[0], rN_seed);                        // (the first block's shuffle beside the projector build)
    const int proj = register_projector(build_projector(m, p, K, h.seeds.data()));
    std::vector<BlockTable> tabs(nblocks);
    try {
        std::vector<double *> viE_of(nblocks, nullptr);
        long long at = 0;
        for (int b = 0; b < nblocks; ++b) { if (viE) viE_of[b] = viE + static_cast<size_t>(at) * view.cols(p); at += ncb[b]; }
        unlimited_blocks_loop(dX_blocks, ncb, ldb, nblocks, m, p, proj, K, rN_seed, viE ? viE_of.data() : nullptr, view,
                              [&](int b, BlockTable &t) { tabs[b] = std::move(t); });
    } catch (...) { drop_projector(proj); throw; }
    drop_projector(proj);
    const int nf = merge_and_relabel(tabs, p, N_cluster, minN, maxN, pred);
    if (n_pred) *n_pred = nf;
    if (p_used) *p_used = p;
    step_mark("SHARP_unlimited returns", 0);
    step_marks_dump();
    SHARP_API_END
}

// SHARP_unlimited2 (R/SHARP_unlimited2.R:29-292): SHARP_fpart per block, then ONE sMetaC over the fold-level ensemble
// clusters of all blocks -- which, like every sMetaC, only needs their centroids in E1 = enE/K.
static int unlimited2_run(const XRef *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                          int ensize_K, int reduced_ndim, int partition_ncells, int hmethod, int N_cluster, int enpN, int indN,
                          int minN, int maxN, double sil_thre, double height_Ntimes, int flag, double rN_seed, int *pred,
                          int *n_pred, int *p_used, double *viE) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(dX_blocks && ncb && ldb && pred && nblocks >= 1, "No expression data is provided!");
    long long ncells = 0;
    for (int b = 0; b < nblocks; ++b) ncells += ncb[b];
    const CallHeader h = call_header(ncells, ensize_K, reduced_ndim, rN_seed);
    const int p = h.p, K = h.K;
    SharpArgs fa;
    fa.partition_ncells = partition_ncells; fa.hmethod = hmethod; fa.enpN = enpN; fa.indN = indN;
    fa.minN = minN > 0 ? minN : 2;                                                                             // :51-53
    fa.maxN = maxN > 0 ? maxN : static_cast<int>(std::max<long long>(40, (ncells + 4999) / 5000));             // :54-56 (total cells)
    fa.sil_thre = sil_thre; fa.height_Ntimes = height_Ntimes;
    fa.N_cluster = 0;                                                                                          // fpart does not cut; the final sMetaC does
    step_mark("SHARP_unlimited begins, blocks", nblocks);
    const int proj = register_projector(build_projector(m, p, K, h.seeds.data()));
    std::vector<BlockTable> tabs(nblocks);
    long long off = 0;
    try {
        for (int b = 0; b < nblocks; ++b) {                                                                    // :146-163
            const bool more = b + 1 < nblocks;
            unlimited_block_dev(dX_blocks[b], m, ncb[b], ldb[b], p, proj, K, rN_seed, tabs[b],
                                viE ? viE + static_cast<size_t>(off) * p : nullptr, ViewCall(), flag ? 2 : 0, &fa, more ? dX_blocks[b + 1] : XRef(),
                                more ? ncb[b + 1] : 0, more ? ldb[b + 1] : 0);
            off += ncb[b];
        }
    } catch (...) { drop_projector(proj); throw; }
    drop_projector(proj);
    const int nf = merge_and_relabel(tabs, p, N_cluster, minN, maxN, pred, hmethod > 0 ? hmethod : 1, sil_thre >= 0 ? sil_thre : 0.35,
                                     height_Ntimes > 0 ? height_Ntimes : 2.0);                               // :184-205
    if (n_pred) *n_pred = nf;
    if (p_used) *p_used = p;
    SHARP_API_END
}

namespace {

struct NextHint { const float *dX = nullptr; long long nb = 0, ld = 0; };
NextHint &next_hint() { return per_slot<NextHint>(); }

// One block's table into a caller's buffers: labels, the G rows of means and sizes, and G itself -- if G rows fit into the cap_rows the
// caller still has.  entry: the name the refusal carries.
void table_to_caller(const BlockTable &t, const char *entry, int *pred, double *means, long long *counts, int *n_clusters, int cap_rows) {
    SHARP_REQUIRE(static_cast<int>(t.counts.size()) <= cap_rows, std::string(entry) + ": centroid buffer too small");
    std::copy(t.pred.begin(), t.pred.end(), pred);
    std::copy(t.means.begin(), t.means.end(), means);
    std::copy(t.counts.begin(), t.counts.end(), counts);
    *n_clusters = static_cast<int>(t.counts.size());
}

// The body of the five per-block entries.  name: what its refusals carry; view_in: the view the caller names, or NULL = the calling
// thread's arm (sharp_unlimited_view_dim); takes_hint: the entry reads and clears the hint of sharp_unlimited_next_block_dev.
int unlimited_block_entry(const char *name, const void *dXv, bool f64, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                          double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows, long long *counts, double *viE,
                          const ViewCall *view_in, bool takes_hint) {
    SHARP_API_BEGIN
    // (a caller that arms sharp_unlimited_view_dim per block gets its E1 rows back reduced; block by block an UNSEEDED run must say which z0
    // its blocks share: sharp_unlimited_block_viewk_dev)
    const ViewCall view = view_in ? *view_in : take_view(rN_seed, ensemble_size(ensize_K));
    ctx();
    SHARP_REQUIRE(pred && n_clusters && means && counts, std::string(name) + ": null output");
    NextHint h;
    if (takes_hint) std::swap(h, next_hint());
    const XRef dX = f64 ? dev64_ref(static_cast<const double *>(dXv), m, nb, ld) : XRef(static_cast<const float *>(dXv));
    BlockTable t;
    unlimited_block_dev(dX, m, nb, ld, p, projector, ensemble_size(ensize_K), rN_seed, t, viE, view, flag != 0, nullptr,
                        h.dX ? XRef(h.dX) : XRef(), h.nb, h.ld);
    table_to_caller(t, name, pred, means, counts, n_clusters, cap_rows);
    SHARP_API_END
}

// the two entries that name their view: view_dim columns per cell of viE, from the z0 of view_seed
int unlimited_block_viewk_entry(const char *name, const void *dX, bool f64, int m, long long nb, long long ld, int p, int projector,
                                int ensize_K, double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                long long *counts, int view_dim, double view_seed, double *viE) {
    if (view_dim < 0 || view_dim > 4096 || (view_dim > 0 && std::fmod(view_seed, 1.0) != 0.0)) {
        sharp::set_error(std::string(name) + ": view_dim must lie in 0 .. 4096 and view_seed must be an integer (the seed of the run's z0)");
        return SHARP_ERR_ARG;
    }
    ViewCall v;
    v.kdim = viE ? view_dim : 0;
    v.seed = view_seed;
    return unlimited_block_entry("sharp_unlimited_block_view_dev", dX, f64, m, nb, ld, p, projector, ensize_K, rN_seed, flag, pred, n_clusters,
                                 means, cap_rows, counts, viE, &v, true);
}

}  // namespace

extern "C" {

/* One-shot hint for a caller that runs its blocks one call at a time (a rank of the sharded run with several blocks): the block that
 * the NEXT-BUT-ONE call will bring (same genes, projector and parameters as the next call's block), already resident in HBM.  The next
 * sharp_unlimited_block_view*_dev call prepares it under its own tail.  dX = NULL clears the hint. */
int sharp_unlimited_next_block_dev(const float *dX_next, long long nb_next, long long ld_next) {
    NextHint &h = next_hint();
    h.dX = dX_next; h.nb = nb_next; h.ld = ld_next;
    return SHARP_OK;
}

int sharp_unlimited_block_view_dev(const float *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                   double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                   long long *counts, double *viE) {
    return unlimited_block_entry("sharp_unlimited_block_view_dev", dX, false, m, nb, ld, p, projector, ensize_K, rN_seed, flag, pred, n_clusters,
                                 means, cap_rows, counts, viE, nullptr, true);
}

int sharp_unlimited_block_viewk_dev(const float *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                    double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                    long long *counts, int view_dim, double view_seed, double *viE) {
    return unlimited_block_viewk_entry("sharp_unlimited_block_viewk_dev", dX, false, m, nb, ld, p, projector, ensize_K, rN_seed, flag, pred,
                                       n_clusters, means, cap_rows, counts, view_dim, view_seed, viE);
}

/* the same for a resident fp64 block (TPM / CPM-like values: 16-byte aligned, even leading dimension) */
int sharp_unlimited_block_viewk_dev64(const double *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                      double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                      long long *counts, int view_dim, double view_seed, double *viE) {
    return unlimited_block_viewk_entry("sharp_unlimited_block_viewk_dev64", dX, true, m, nb, ld, p, projector, ensize_K, rN_seed, flag, pred,
                                       n_clusters, means, cap_rows, counts, view_dim, view_seed, viE);
}

/* no view, and the hint of sharp_unlimited_next_block_dev is left for a view entry */
int sharp_unlimited_block_dev(const float *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K, double rN_seed,
                              int *pred, int *n_clusters, double *means, int cap_rows, long long *counts) {
    const ViewCall none;
    return unlimited_block_entry("sharp_unlimited_block_dev", dX, false, m, nb, ld, p, projector, ensize_K, rN_seed, 1, pred, n_clusters, means,
                                 cap_rows, counts, nullptr, &none, false);
}

int sharp_unlimited_block_dev64(const double *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K, double rN_seed,
                                int *pred, int *n_clusters, double *means, int cap_rows, long long *counts) {
    const ViewCall none;
    return unlimited_block_entry("sharp_unlimited_block_dev64", dX, true, m, nb, ld, p, projector, ensize_K, rN_seed, 1, pred, n_clusters, means,
                                 cap_rows, counts, nullptr, &none, false);
}

int sharp_unlimited_merge(const double *means, const long long *counts, int nC, int p, long long ncells, int N_cluster, int minN,
                          int maxN, int *final_id, int *n_final) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(means && counts && final_id && n_final, "sharp_unlimited_merge: null argument");
    std::vector<int> fid;
    int nf = 0;
    unlimited_merge(means, counts, nC, p, ncells, N_cluster, minN, maxN, fid, nf);
    std::copy(fid.begin(), fid.end(), final_id);
    *n_final = nf;
    SHARP_API_END
}

// SEVERAL blocks of one rank of a sharded SHARP_unlimited run in one call (sharp_unlimited_block_dev per block, but with the base
// clustering of all of them as one pipelined batch and their tails on helper threads: 17 instead of 25 ms per 50 000-cell block).
int sharp_unlimited_blocks_dev(const void *const *dX_blocks, const int *is_f64, const long long *ncb, const long long *ldb, int nblocks, int m,
                               int p, int projector, int ensize_K, double rN_seed, int *pred, int *n_clusters, double *means, int cap_rows,
                               long long *counts) {
    SHARP_API_BEGIN
    ctx();
    SHARP_REQUIRE(dX_blocks && ncb && ldb && pred && n_clusters && means && counts && nblocks >= 1, "sharp_unlimited_blocks_dev: null argument");
    SHARP_REQUIRE(p >= 1 && cap_rows >= 1, "sharp_unlimited_blocks_dev: bad sizes");
    std::vector<XRef> refs(nblocks);
    for (int b = 0; b < nblocks; ++b) {
        SHARP_REQUIRE(dX_blocks[b] && ncb[b] >= 1 && ldb[b] >= m, "sharp_unlimited_blocks_dev: bad block");
        refs[b] = (is_f64 && is_f64[b]) ? dev64_ref(static_cast<const double *>(dX_blocks[b]), m, ncb[b], ldb[b])
                                        : XRef(static_cast<const float *>(dX_blocks[b]));
    }
    long long off = 0;
    int rows = 0;                                          // the running row offset into the caller's table
    unlimited_blocks_loop(refs.data(), ncb, ldb, nblocks, m, p, projector, ensemble_size(ensize_K), rN_seed, nullptr, ViewCall(),
                          [&](int b, BlockTable &t) {
        table_to_caller(t, "sharp_unlimited_blocks_dev", pred + off, means + static_cast<size_t>(rows) * p, counts + rows, &n_clusters[b], cap_rows - rows);
        rows += n_clusters[b];
        off += ncb[b];
    });
    SHARP_API_END
}
}  // extern "C"

namespace {
// host blocks of a list-of-matrices call: each is stored as fp32 or fp64 on its own merits
struct HostBlocks {
    std::vector<HostBlock> bufs;
    std::vector<XRef> refs;
    std::vector<long long> lds;
    int upload(const double *const *X_blocks, const long long *ncb, int nblocks, int m) {
        return api_guarded([&] {
            ctx();
            if (!X_blocks || !ncb || nblocks < 1) throw sharp::Error(SHARP_ERR_ARG, "No expression data is provided!");
            bufs.resize(nblocks);
            for (int b = 0; b < nblocks; ++b) {
                upload_block(X_blocks[b], m, ncb[b], m, bufs[b]);
                refs.push_back(bufs[b].ref());
                lds.push_back(bufs[b].ld);
            }
        });
    }
};
// One block of a list-of-blocks call, wherever it lives: a dense host matrix (R's numeric matrix), the three slots of a dgCMatrix,
// or a block already resident on one of the call's GPUs.
struct BlockSrc {
    enum Kind { HostDense, HostCsc, DevF32, DevF64 } kind = HostDense;
    const double *host = nullptr;                          // HostDense: m x n doubles, column stride m
    const int *colptr = nullptr, *rowidx = nullptr;        // HostCsc: @p (n + 1), @i
    const double *val = nullptr;                           //          @x
    const void *dev = nullptr;                             // DevF32 / DevF64
    long long ld = 0;
    int worker = -1;                                       // DevF32 / DevF64: index into the call's device list (the GPU the block lives on)
    long long n = 0;
    bool on_host() const { return kind == HostDense || kind == HostCsc; }
};

HostBlockPair &host_block_pair() { return per_slot<HostBlockPair>(); }

// What the last in-process multi-device call did when: one row per block -- worker, block, upload start / end, clustering start / end,
// seconds since the call began (sharp_multi_timeline; profiles/r04_multi_timeline.txt).
struct MultiTimeline { std::mutex mu; std::vector<double> rows; };
MultiTimeline &multi_timeline() { static MultiTimeline *t = new MultiTimeline; return *t; }
double wall_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

// The upload thread of one worker of unlimited_run_multi: the worker's host blocks into the resident copies of a slot of its own, in block
// order, a ring of copies ahead of the compute thread.  my: the worker's blocks (indices into blocks), positions i below are into my.
struct Feed {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> ready;                      // per position in my: uploaded
    std::vector<XRef> ref;
    std::vector<long long> ld;
    int consumed = 0;                             // host blocks the compute thread has finished with
    bool stop = false;
    std::string err;
    int rc = SHARP_OK;
    const std::vector<BlockSrc> &blocks;
    const std::vector<int> &my;
    const int m;
    std::vector<int> hostpos;                     // positions in `my` that hold host blocks
    int group_max = 1, ring = 0;
    std::thread up;

    Feed(const std::vector<BlockSrc> &blocks_, const std::vector<int> &my_, int m_)
        : ready(my_.size(), 0), ref(my_.size()), ld(my_.size(), 0), blocks(blocks_), my(my_), m(m_) {
        for (size_t i = 0; i < my.size(); ++i) if (blocks[my[i]].on_host()) hostpos.push_back(static_cast<int>(i));
        // resident copies the upload rotates through: three (block after block, each prepared under the previous one's tail: the default), four when
        // SHARP_HOST_GROUP >= 2 asks for groups of arrived blocks as one pipelined batch (measured: no gain at two or three blocks)
        long long big = 0;
        for (int i : hostpos) big = std::max<long long>(big, blocks[my[i]].n);
        group_max = std::max(1, std::min(knobs().host_group, kHostRing - 1));
        // (three when block follows block: with two, block i + 2 could only start its upload when block i was done, i.e. when block i + 1 began -- so
        // no block was ever on the GPU in time to have its front prepared under its predecessor's tail, and a cfg3 block cost 26 ms instead of 20)
        ring = static_cast<double>(big) * m * 4.0 > 8e9 ? 2 : (group_max == 1 ? 3 : kHostRing);
    }
    ~Feed() { stop_now(); }
    // starts the upload thread (a worker without host blocks has none); tl: the call's timeline rows, in seconds since t_begin
    void start(int device, int occurrence, double *tl, double t_begin) {
        if (hostpos.empty()) return;
        up = std::thread([this, device, occurrence, tl, t_begin] {
            try {
                init_slot(acquire_slot(device, occurrence, 1), device, true);   // (high-priority stream: a block's expansion takes the CUs the clustering leaves free ahead of the next chunk's distance GEMM, which nothing waits for yet)
                HostBlockPair &P = host_block_pair();
                for (size_t h = 0; h < hostpos.size(); ++h) {
                    {   // copy h % ring is free once the compute thread is done with host block h - ring
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return stop || consumed + ring > static_cast<int>(h); });
                        if (stop) return;
                    }
                    const int i = hostpos[h], b = my[i];
                    const BlockSrc &s = blocks[b];
                    HostBlock &hb = P.hb[h % ring];
                    tl[static_cast<size_t>(b) * 6 + 2] = wall_s() - t_begin;
                    if (s.kind == BlockSrc::HostDense) upload_block(s.host, m, s.n, m, hb);
                    else upload_block_csc(s.colptr, s.rowidx, s.val, m, s.n, hb);
                    stream_sync();
                    tl[static_cast<size_t>(b) * 6 + 3] = wall_s() - t_begin;
                    std::lock_guard<std::mutex> lk(mu);
                    ref[i] = hb.ref(); ld[i] = hb.ld; ready[i] = 1;
                    cv.notify_all();
                }
            }
            catch (const sharp::Error &e) { std::lock_guard<std::mutex> lk(mu); err = e.what(); rc = e.code; cv.notify_all(); }
            catch (const std::exception &e) { std::lock_guard<std::mutex> lk(mu); err = e.what(); rc = SHARP_ERR; cv.notify_all(); }
        });
    }
    // where block position i of this worker is, once it is on the GPU (wait: for its upload; a resident block is there already)
    bool block(size_t i, bool wait, XRef &r, long long &l) {
        const BlockSrc &s = blocks[my[i]];
        if (!s.on_host()) {
            r = s.kind == BlockSrc::DevF64 ? dev64_ref(static_cast<const double *>(s.dev), m, s.n, s.ld) : XRef(static_cast<const float *>(s.dev));
            l = s.ld;
            return true;
        }
        std::unique_lock<std::mutex> lk(mu);
        if (wait) cv.wait(lk, [&] { return ready[i] || rc != SHARP_OK; });
        if (rc != SHARP_OK) throw sharp::Error(rc, err);
        if (!ready[i]) return false;
        r = ref[i]; l = ld[i];
        return true;
    }
    void done_with(int n) {                       // the compute thread has finished with n more host blocks: their copies are free
        std::lock_guard<std::mutex> lk(mu);
        consumed += n;
        cv.notify_all();
    }
    void stop_now() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        if (up.joinable()) up.join();
    }
};

// SHARP_unlimited over several GPUs inside one process (R/SHARP_unlimited.R:125-183): the serial block loop of the reference
// (:125-163) is dealt out, block b to worker b mod W (a resident block: to the worker of the GPU it lives on).  A worker is a host thread
// bound to a device slot of its own (context, streams, workspaces, projector handles: common.hpp): it builds the K projectors on its GPU
// (a pure function of m, p and the seeds, :97-104; p from the GLOBAL cell count, :65-66) and clusters its blocks one after the other, each
// prepared under the previous one's tail when it is already resident.  Host blocks -- dense or sparse -- reach the GPU through a second
// thread per worker with a slot of its own (own stream, pinned staging, three resident copies in rotation: Feed): block i + W crosses PCIe
// while block i is clustered.  Per block the worker keeps the labels and the per-cluster centroid means and sizes -- all the final sMetaC
// uses of E1 (R/sMetaC.R:58-63); the tables (a few hundred rows x p doubles per block) meet in host memory, worker 0 runs the merge
// (:163-183) once the others are done, and every block's labels are mapped through it.  No other data crosses between devices.
// MultiRun: what the workers of one such call share.
struct MultiRun {
    const std::vector<BlockSrc> &blocks;
    int m = 0, N_cluster = 0, minN = 0, maxN = 0, W = 0;
    double rN_seed = 0;
    const int *devices = nullptr;
    int *pred = nullptr;
    double *viE = nullptr;
    ViewCall view;                                        // (by value into every worker: one z0 on all devices)
    CallHeader h;
    std::vector<long long> cell0;                         // the first cell of each block
    std::vector<std::vector<int>> mine;                   // the blocks of each worker, in block order
    std::vector<int> occ;                                 // which occurrence of its device a worker is (a device may be listed repeatedly)
    std::vector<BlockTable> tabs;
    std::vector<std::string> err;
    std::vector<int> rcs;
    double t_begin = 0;
    std::vector<double> tl;
    std::mutex done_mu;
    std::condition_variable done_cv;
    int done_workers = 0;
    std::atomic<int> failed{0};
    int nf = 0;

    explicit MultiRun(const std::vector<BlockSrc> &b) : blocks(b) {}
    double *viE_at(int b) const { return viE ? viE + static_cast<size_t>(cell0[b]) * view.cols(h.p) : nullptr; }   // E1 rows of this block (:153), viewflag only
    void timeline_row(int b, int w, double t_go) {
        double *r = tl.data() + static_cast<size_t>(b) * 6;
        r[0] = w; r[1] = b; r[4] = t_go; r[5] = wall_s() - t_begin;
    }
    void run_range(int w, Feed &feed, int proj, size_t i, size_t j, bool small_windows);
    void worker(int w);
};

// Positions [i, j) of worker w's blocks, all on its GPU by now, in one call: pipelined batch windows where the blocks qualify, tails on
// helper threads, instead of block after block.
void MultiRun::run_range(int w, Feed &feed, int proj, size_t i, size_t j, bool small_windows) {
    const std::vector<int> &my = mine[w];
    std::vector<XRef> refs(j - i);
    std::vector<long long> nn(j - i), ll(j - i);
    std::vector<double *> vo(j - i, nullptr);
    for (size_t q = i; q < j; ++q) {
        feed.block(q, true, refs[q - i], ll[q - i]);
        nn[q - i] = blocks[my[q]].n;
        vo[q - i] = viE_at(my[q]);
    }
    const double t_go = wall_s() - t_begin;
    unlimited_blocks_loop(refs.data(), nn.data(), ll.data(), static_cast<int>(j - i), m, h.p, proj, h.K, rN_seed, viE ? vo.data() : nullptr, view,
                          [&](int q, BlockTable &t) {
        const int b = my[i + q];
        tabs[b] = std::move(t);
        timeline_row(b, w, t_go);
    }, my.data() + i, small_windows);
}

void MultiRun::worker(int w) {
    const std::vector<int> &my = mine[w];
    Feed feed(blocks, my, m);
    try {
        feed.start(devices[w], occ[w], tl.data(), t_begin);
        init_slot(acquire_slot(devices[w], occ[w], 0), devices[w]);
        const int proj = my.empty() ? 0 : register_projector(build_projector(m, h.p, h.K, h.seeds.data()));
        try {
            // all of this worker's blocks are on its GPU already: one call for the lot
            const bool all_resident = feed.hostpos.empty() && my.size() >= 2;
            if (all_resident) run_range(w, feed, proj, 0, my.size(), false);
            for (size_t i = all_resident ? my.size() : 0; i < my.size(); ++i) {
                if (failed.load()) break;
                const int b = my[i];
                XRef ref, nref;
                long long ld = 0, nld = 0;
                feed.block(i, true, ref, ld);
                // SHARP_HOST_GROUP >= 2: the blocks that arrived go TOGETHER as one pipelined batch (unlimited_batch_window).  Whatever the
                // grouping, every block is the same SHARP() call: same labels.
                if (feed.group_max > 1 && feed.ring > 2 && blocks[b].on_host()) {
                    size_t j = i + 1;
                    // (the SECOND block of a group is waited for -- one upload, 15-20 ms, against the 25 ms a lone block costs while half of the
                    // chip idles; its successor's upload then runs under the pair's 44 ms -- a third is taken only if it is there already)
                    while (j < my.size() && static_cast<int>(j - i) < std::min(feed.group_max, feed.ring - 1) && blocks[my[j]].on_host() &&
                           feed.block(j, j - i < 2 && blocks[my[j]].n >= 5000 && blocks[b].n >= 5000, nref, nld))
                        ++j;
                    if (j - i >= 2) {
                        run_range(w, feed, proj, i, j, true);
                        feed.done_with(static_cast<int>(j - i));
                        i = j - 1;
                        continue;
                    }
                }
                // the next block's front goes under this block's tail if that block is on the GPU by now (a resident block always is)
                const bool more = i + 1 < my.size() && feed.block(i + 1, false, nref, nld);
                const double t_go = wall_s() - t_begin;
                unlimited_block_dev(ref, m, blocks[b].n, ld, h.p, proj, h.K, rN_seed, tabs[b], viE_at(b), view, 1, nullptr, more ? nref : XRef(),
                                    more ? blocks[my[i + 1]].n : 0, more ? nld : 0, b);
                timeline_row(b, w, t_go);
                if (blocks[b].on_host()) feed.done_with(1);
            }
        } catch (...) { drop_pending_front(); if (proj) drop_projector(proj); throw; }
        drop_pending_front();
        if (proj) drop_projector(proj);
        stream_sync();
        feed.stop_now();
        if (w == 0) {
            // the one exchange step: worker 0 waits for the others, then the centroid tables in global block order and the merge on its GPU
            {
                std::unique_lock<std::mutex> lk(done_mu);
                done_cv.wait(lk, [&] { return done_workers == W - 1; });
            }
            if (!failed.load()) {
                nf = merge_and_relabel(tabs, h.p, N_cluster, minN, maxN, pred);   // labels scattered back (:165-183 through the merge's map)
                stream_sync();
            }
        }
    }
    catch (const sharp::Error &e) { err[w] = e.what(); rcs[w] = e.code; failed.store(1); feed.stop_now(); }
    catch (const std::exception &e) { err[w] = e.what(); rcs[w] = SHARP_ERR; failed.store(1); feed.stop_now(); }
    if (w != 0) {
        std::lock_guard<std::mutex> lk(done_mu);
        ++done_workers;
        done_cv.notify_all();
    } else if (rcs[0] != SHARP_OK) {                  // (worker 0 failed before it waited: the others still have to be counted out)
        std::unique_lock<std::mutex> lk(done_mu);
        done_cv.wait(lk, [&] { return done_workers == W - 1; });
    }
}

int unlimited_run_multi(const std::vector<BlockSrc> &blocks, int m, int ensize_K, int N_cluster, int minN, int maxN, double rN_seed,
                        const int *devices, int ndev, int *pred, int *n_pred, int *p_used, double *viE) {
    SHARP_API_BEGIN
    MultiRun R(blocks);
    R.view = take_view(rN_seed, ensemble_size(ensize_K));
    const int nblocks = static_cast<int>(blocks.size());
    SHARP_REQUIRE(pred, "The input should be a LIST of partitioned scRNA-seq expression matrices!");
    SHARP_REQUIRE(nblocks >= 2, "SHARP is used instead of SHARP_unlimited because the length of the input is 1!");
    SHARP_REQUIRE(devices && ndev >= 1 && ndev <= 16, "SHARP_unlimited: the device list must name between 1 and 16 GPUs");
    R.cell0.assign(nblocks + 1, 0);
    for (int b = 0; b < nblocks; ++b) R.cell0[b + 1] = R.cell0[b] + blocks[b].n;
    R.h = call_header(R.cell0[nblocks], ensize_K, 0, rN_seed);
    bool resident = false;
    for (const BlockSrc &s : blocks) {
        SHARP_REQUIRE(s.n >= 3 && (s.kind == BlockSrc::HostDense ? s.host != nullptr : s.kind == BlockSrc::HostCsc ? s.colptr != nullptr : s.dev != nullptr),
                      "SHARP_unlimited: empty block");
        SHARP_REQUIRE(s.on_host() || (s.worker >= 0 && s.worker < ndev), "SHARP_unlimited: a resident block names a device outside the device list");
        resident |= !s.on_host();
    }
    const int W = resident ? ndev : std::min(ndev, nblocks);
    SHARP_REQUIRE(rN_seed != 0.5 || W == 1, "SHARP_unlimited on several GPUs needs a seed: unseeded projectors would differ between the devices");
    R.m = m; R.N_cluster = N_cluster; R.minN = minN; R.maxN = maxN; R.W = W; R.rN_seed = rN_seed;
    R.devices = devices; R.pred = pred; R.viE = viE;
    R.mine.resize(W);
    for (int b = 0; b < nblocks; ++b) R.mine[blocks[b].on_host() ? b % W : blocks[b].worker].push_back(b);
    R.occ.assign(W, 0);
    for (int w = 0; w < W; ++w) for (int v = 0; v < w; ++v) R.occ[w] += devices[v] == devices[w];
    R.tabs.resize(nblocks);
    R.err.resize(W);
    R.rcs.assign(W, SHARP_OK);
    R.t_begin = wall_s();
    R.tl.assign(static_cast<size_t>(nblocks) * 6, 0.0);
    {
        std::vector<std::thread> th;
        for (int w = 0; w < W; ++w) th.emplace_back([&R, w] { R.worker(w); });
        for (auto &t : th) t.join();
    }
    {
        MultiTimeline &T = multi_timeline();
        std::lock_guard<std::mutex> lk(T.mu);
        T.rows = R.tl;
    }
    step_marks_dump();
    for (int w = 0; w < W; ++w)
        if (R.rcs[w] != SHARP_OK) throw sharp::Error(R.rcs[w], "device " + std::to_string(devices[w]) + ": " + R.err[w]);
    if (n_pred) *n_pred = R.nf;
    if (p_used) *p_used = R.h.p;
    SHARP_API_END
}

std::vector<BlockSrc> dense_sources(const double *const *X_blocks, const long long *ncb, int nblocks) {
    std::vector<BlockSrc> v;
    for (int b = 0; X_blocks && ncb && b < nblocks; ++b) { BlockSrc s; s.kind = BlockSrc::HostDense; s.host = X_blocks[b]; s.n = ncb[b]; v.push_back(s); }
    return v;
}
std::vector<BlockSrc> csc_sources(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks) {
    std::vector<BlockSrc> v;
    for (int b = 0; colptr && rowidx && val && ncb && b < nblocks; ++b) {
        BlockSrc s;
        s.kind = BlockSrc::HostCsc; s.colptr = colptr[b]; s.rowidx = rowidx[b]; s.val = val[b]; s.n = ncb[b];
        v.push_back(s);
    }
    return v;
}
// the devices of a host-block call: the caller's list, else SHARP_DEVICES, else the caller's own device (one worker: upload and clustering still overlap)
std::vector<int> call_devices(const int *devices, int ndevices) {
    if (devices && ndevices > 0) return std::vector<int>(devices, devices + ndevices);
    if (!knobs().devices.empty()) return knobs().devices;
    return std::vector<int>(1, ctx().device);
}

std::vector<XRef> f32_refs(const float *const *dX_blocks, int nblocks) {
    std::vector<XRef> r;
    for (int b = 0; dX_blocks && b < nblocks; ++b) r.emplace_back(dX_blocks[b]);
    return r;
}
}  // namespace

extern "C" {

int sharp_SHARP_unlimited_view_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                                   int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used,
                                   double *viE) {
    const std::vector<XRef> refs = f32_refs(dX_blocks, nblocks);
    return unlimited_run(dX_blocks ? refs.data() : nullptr, ncb, ldb, nblocks, m, ensize_K, N_cluster, minN, maxN, rN_seed, pred, n_pred, p_used, viE);
}

int sharp_unlimited_view_dim(int kdim) {
    SHARP_API_BEGIN
    SHARP_REQUIRE(kdim >= 0 && kdim <= 4096, "sharp_unlimited_view_dim: the view dimension must lie in 0 .. 4096");
    tl_view_pending = kdim;
    SHARP_API_END
}

int sharp_SHARP_unlimited_viewk_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                                    int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used,
                                    int view_dim, double *viE) {
    if (view_dim < 0 || view_dim > 4096) { sharp::set_error("sharp_SHARP_unlimited_viewk_dev: the view dimension must lie in 0 .. 4096"); return SHARP_ERR_ARG; }
    tl_view_pending = 0;                                                       // (the explicit argument wins over an earlier arm)
    const ViewCall view = make_view(viE ? view_dim : 0, rN_seed, ensemble_size(ensize_K));
    const std::vector<XRef> refs = f32_refs(dX_blocks, nblocks);
    return unlimited_run(dX_blocks ? refs.data() : nullptr, ncb, ldb, nblocks, m, ensize_K, N_cluster, minN, maxN, rN_seed, pred, n_pred, p_used, viE, &view);
}

int sharp_SHARP_unlimited2_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                               int ensize_K, int reduced_ndim, int partition_ncells, int hmethod, int N_cluster, int enpN, int indN,
                               int minN, int maxN, double sil_thre, double height_Ntimes, int flag, double rN_seed, int *pred,
                               int *n_pred, int *p_used, double *viE) {
    const std::vector<XRef> refs = f32_refs(dX_blocks, nblocks);
    return unlimited2_run(dX_blocks ? refs.data() : nullptr, ncb, ldb, nblocks, m, ensize_K, reduced_ndim, partition_ncells, hmethod, N_cluster,
                          enpN, indN, minN, maxN, sil_thre, height_Ntimes, flag, rN_seed, pred, n_pred, p_used, viE);
}

int sharp_SHARP_unlimited2(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K, int reduced_ndim,
                           int partition_ncells, int hmethod, int N_cluster, int enpN, int indN, int minN, int maxN, double sil_thre,
                           double height_Ntimes, int flag, double rN_seed, int *pred, int *n_pred, int *p_used, double *viE) {
    HostBlocks H;
    if (const int rc = H.upload(X_blocks, ncb, nblocks, m)) return rc;
    return unlimited2_run(H.refs.data(), ncb, H.lds.data(), nblocks, m, ensize_K, reduced_ndim, partition_ncells, hmethod,
                          N_cluster, enpN, indN, minN, maxN, sil_thre, height_Ntimes, flag, rN_seed, pred, n_pred, p_used, viE);
}

int sharp_SHARP_unlimited_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                              int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used) {
    return sharp_SHARP_unlimited_view_dev(dX_blocks, ncb, ldb, nblocks, m, ensize_K, N_cluster, minN, maxN, rN_seed, pred, n_pred,
                                          p_used, nullptr);
}

int sharp_SHARP_unlimited_view(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K, int N_cluster,
                               int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used, double *viE) {
    // A list of host matrices never sits in HBM as a whole: the blocks cross PCIe one after the other into a ring of resident copies while the
    // earlier ones are clustered (unlimited_run_multi), on the caller's GPU or dealt to the GPUs of SHARP_DEVICES=0,1,2,... (one host thread
    // each; an unseeded call stays on the caller's GPU: every device would draw its own projectors).
    if (!X_blocks || !ncb || nblocks < 1) { sharp::set_error("No expression data is provided!"); return SHARP_ERR_ARG; }
    std::vector<int> dv;
    if (const int rc = api_guarded([&] { dv = call_devices(nullptr, 0); })) return rc;
    if (rN_seed == 0.5 && dv.size() > 1) dv.resize(1);
    return unlimited_run_multi(dense_sources(X_blocks, ncb, nblocks), m, ensize_K, N_cluster, minN, maxN, rN_seed, dv.data(),
                               static_cast<int>(dv.size()), pred, n_pred, p_used, viE);
}

int sharp_SHARP_unlimited_multi(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K, int N_cluster,
                                int minN, int maxN, double rN_seed, const int *devices, int ndevices, int *pred, int *n_pred, int *p_used,
                                double *viE) {
    if (!X_blocks || !ncb) { sharp::set_error("The input should be a LIST of partitioned scRNA-seq expression matrices!"); return SHARP_ERR_ARG; }
    return unlimited_run_multi(dense_sources(X_blocks, ncb, nblocks), m, ensize_K, N_cluster, minN, maxN, rN_seed, devices, ndevices, pred, n_pred, p_used, viE);
}

/* a list of dgCMatrix blocks: only the non-zeros of a block cross PCIe, block i + W while block i is clustered */
int sharp_SHARP_unlimited_csc_multi(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                                    int nblocks, int m, int ensize_K, int N_cluster, int minN, int maxN, double rN_seed,
                                    const int *devices, int ndevices, int *pred, int *n_pred, int *p_used, double *viE) {
    if (!colptr || !rowidx || !val || !ncb) { sharp::set_error("The input should be a LIST of partitioned scRNA-seq expression matrices!"); return SHARP_ERR_ARG; }
    std::vector<int> dv;
    if (const int rc = api_guarded([&] { dv = call_devices(devices, ndevices); })) return rc;
    if (rN_seed == 0.5 && dv.size() > 1) dv.resize(1);
    return unlimited_run_multi(csc_sources(colptr, rowidx, val, ncb, nblocks), m, ensize_K, N_cluster, minN, maxN, rN_seed, dv.data(),
                               static_cast<int>(dv.size()), pred, n_pred, p_used, viE);
}
int sharp_SHARP_unlimited_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                              int nblocks, int m, int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred,
                              int *n_pred, int *p_used, double *viE) {
    return sharp_SHARP_unlimited_csc_multi(colptr, rowidx, val, ncb, nblocks, m, ensize_K, N_cluster, minN, maxN, rN_seed, nullptr, 0,
                                           pred, n_pred, p_used, viE);
}

/* blocks already resident on the GPUs of the device list: block b lives on devices[device_of_block[b]] */
int sharp_SHARP_unlimited_multi_dev(const void *const *dX_blocks, const int *is_f64, const long long *ncb, const long long *ldb,
                                    const int *device_of_block, int nblocks, int m, int ensize_K, int N_cluster, int minN, int maxN,
                                    double rN_seed, const int *devices, int ndevices, int *pred, int *n_pred, int *p_used, double *viE) {
    if (!dX_blocks || !ncb || !ldb || !device_of_block) { sharp::set_error("The input should be a LIST of partitioned scRNA-seq expression matrices!"); return SHARP_ERR_ARG; }
    std::vector<BlockSrc> v;
    for (int b = 0; b < nblocks; ++b) {
        BlockSrc s;
        s.kind = (is_f64 && is_f64[b]) ? BlockSrc::DevF64 : BlockSrc::DevF32;
        s.dev = dX_blocks[b]; s.ld = ldb[b]; s.worker = device_of_block[b]; s.n = ncb[b];
        v.push_back(s);
    }
    return unlimited_run_multi(v, m, ensize_K, N_cluster, minN, maxN, rN_seed, devices, ndevices, pred, n_pred, p_used, viE);
}

/* the last in-process multi-device call, block by block: rows of (worker, block, upload start, upload end, clustering start, clustering end),
 * seconds since the call began */
int sharp_multi_timeline(double *rows, int cap_rows, int *nrows) {
    MultiTimeline &T = multi_timeline();
    std::lock_guard<std::mutex> lk(T.mu);
    const int n = static_cast<int>(T.rows.size() / 6);
    if (nrows) *nrows = n;
    if (rows) std::copy(T.rows.begin(), T.rows.begin() + static_cast<size_t>(std::min(n, cap_rows)) * 6, rows);
    return SHARP_OK;
}

int sharp_SHARP_unlimited(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K, int N_cluster,
                          int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used) {
    return sharp_SHARP_unlimited_view(X_blocks, ncb, nblocks, m, ensize_K, N_cluster, minN, maxN, rN_seed, pred, n_pred, p_used, nullptr);
}

}  // extern "C"
