// driver.hpp -- what crosses between driver.hip (one block: SHARP(), its small and large paths, a batched window of blocks) and
// unlimited.hip (lists of blocks: the SHARP_unlimited runs and every sharp_unlimited_* entry).  Everything else of either unit is private.
#pragma once
#include <vector>

#include "common.hpp"

namespace sharp {

struct SharpArgs {
    int K = 0, reduced_ndim = 0, base_ncells = 0, partition_ncells = 0, hmethod = 0;
    int N_cluster = 0, enpN = 0, indN = 0, minN = 0, maxN = 0;
    double sil_thre = -1, height_Ntimes = 0;
    int flag = 1;            // log-transform
    int projector = 0;       // handle of a shared rM list, 0 = draw from rN_seed
    double rN_seed = 0.5;    // 0.5 = the reference's "unseeded" sentinel
    bool want_viE = false, want_x0 = false;
    // the caller wants viE on the HOST (forview = TRUE, R/SHARP.R:46,844): SHARP_large then sends it on its way -- un-shuffle, copy into a pinned
    // staging block on the mean stream -- as soon as the ensemble mean exists, under the per-fold wMetaC and the sMetaC, instead of behind them
    bool view_to_host = false;
    // SHARP_fpart (R/SHARP_unlimited2.R:297-544): the large path with log10 (flag = 2), E1 rounded to one decimal before
    // clustering, maxN.cluster = 40 for the base tasks, and NO sMetaC: the per-fold ensemble labels go up to the caller
    bool fpart = false;
    int block = 0;           // the block's index in its SHARP_unlimited call (decision log only)
    // SHARP_unlimited with several blocks on this GPU: the block that comes next (same genes, projector, parameters).  Its projection,
    // row preparation and distance matrices are enqueued on a side stream before this block's agglomeration starts, so that they run
    // under this block's (HBM-bound, then host-bound) tail; the next call finds them done.
    XRef next_dX; long long next_n = 0, next_ld = 0;
};

// The view reduction of ONE SHARP_unlimited call (R/SHARP_unlimited.R:216-228), fixed when the call begins and handed down by value to
// everything that works for it (block loops, tail helpers, device workers): kdim > 0 = the caller's viE takes kdim columns per cell, the
// product E1 %*% ranM2(p, kdim, seed) taken per block on the device; seed = the ONE seed of that call's z0 (an integer, also for an
// unseeded run: the reference draws z0 once and multiplies all of E1 by it, :219-225).
struct ViewCall {
    int kdim = 0;
    double seed = 0;
    int cols(int p) const { return kdim > 0 ? kdim : p; }
};

// One finished block of a SHARP_unlimited call: what the cross-block sMetaC needs of it (R/SHARP_unlimited.R:153-163)
struct BlockTable {
    std::vector<int> pred;           // the block's labels, 1..G by first appearance
    std::vector<double> means;       // G x p: the colMeans of its viE per predicted cluster
    std::vector<long long> counts;   // G cluster sizes
};

// one block: y[[i]] = SHARP(mat, reduced.ndim = p, prep = FALSE, logflag = FALSE, rM = rM, ensize.K, rN.seed)
// (:135) and the colMeans of its viE per predicted cluster -- all sMetaC ever uses of E1 (:163, R/sMetaC.R:58-63)
// viE_host: NULL, or where the block's E1 rows go (view.cols(p) columns per cell)
void unlimited_block_dev(XRef dX, int m, long long nb, long long ld, int p, int projector, int K, double rN_seed, BlockTable &out,
                         double *viE_host, const ViewCall &view, int flag = 1, const SharpArgs *fpart_args = nullptr, XRef next_dX = XRef(),
                         long long next_n = 0, long long next_ld = 0, int block = 0);
// blocks [b0, b1) of a list as ONE pipelined batch (driver.hip); tables[b - b0] receives block b's table, viE_of as for unlimited_blocks_loop
void unlimited_batch_window(const XRef *dX, const long long *ncb, const long long *ldb, int b0, int b1, int m, int p, int proj, int K,
                            double rN_seed, double *const *viE_of, const ViewCall &view, BlockTable *tables, const int *gids = nullptr);
// asks for the shuffle of an n-cell block on a thread of its own, for the next large front of this slot
void shuffle_ahead(long long n, double rN_seed);

}  // namespace sharp
