// dotc.hip -- the entry points of include/sharp_hip.h once more in R's .C() calling convention: every argument a
// pointer (R hands .C() copies of its vectors: double* for numeric, int* for integer/logical), void return, the status in the last
// argument.  With these the reference's exported functions (NAMESPACE:3-28) can call the library from plain R --
//     .C("sharp_C_SHARP", as.double(scExp), nrow(scExp), as.double(ncol(scExp)), ..., status = integer(1))
// -- with no glue compiled against R.h; r/sharp_hip.R holds those R lines, r/sharp_glue.c the .Call shim that avoids .C()'s copies.
// Conventions on top of sharp_hip.h's:
//   - a dimension that can exceed 2^31 - 1 (cells) travels as double*, since R has no 64-bit integer;
//   - R cannot pass NULL: an optional output is a buffer of length >= 1 plus a bit in *want (documented per function);
//   - "missing" scalar arguments are 0 (integers) / negative (sil.thre) like in sharp_hip.h;
//   - *status receives what the plain entry point returns (0, warning bits, or an error code: then sharp_C_last_error()
//     gives the text for R's stop()).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

namespace {

inline long long as_ll(const double *v) { return v ? static_cast<long long>(std::llround(*v)) : 0; }

// R/get_opt_hclust.R:76-83: flashmark = TRUE takes flashClust(d, "ward"), the ward.D criterion, and the test
// `hmethod == "ward.D" || "ward.D2"` that guards it is an error in R for every other method (reference quirk 6)
int flashmark_method(int flashmark, int hmethod, int *status) {
    if (!flashmark) return hmethod;
    const int hm = hmethod > 0 ? hmethod : 1;
    if (hm != 1) {
        sharp::set_error("invalid 'y' type in 'x || y' (flashmark = TRUE with hmethod other than \"ward.D\": R/get_opt_hclust.R:79)");
        *status = SHARP_ERR_ARG;
        return -1;
    }
    return 1;
}

/* dense blocks one after the other (unlist(lapply(scExp, as.double)): block b is m x ncb[b] column-major) as the pointer list of the
 * plain entries */
struct DenseList {
    std::vector<const double *> ptrs;
    std::vector<long long> nc;
    bool ok = false;
    DenseList(double *Xcat, int B, double *ncb, int m, int *status) {
        if (B < 1) { sharp::set_error("No expression data is provided!"); *status = SHARP_ERR_ARG; return; }
        ptrs.resize(B); nc.resize(B);
        long long off = 0;
        for (int b = 0; b < B; ++b) { ptrs[b] = Xcat + off * m; nc[b] = as_ll(ncb + b); off += nc[b]; }
        ok = true;
    }
};

/* a list of dgCMatrix blocks laid out as sharp_C_SHARP_unlimited_csc takes it, as the pointer lists of the plain entries */
struct CscList {
    std::vector<const int *> cp, ri;
    std::vector<const double *> vx;
    std::vector<long long> nc;
    bool ok = false;
    CscList(int *pcat, int *icat, double *xcat, int B, double *ncb, int *status) {
        if (B < 1) { sharp::set_error("No expression data is provided!"); *status = SHARP_ERR_ARG; return; }
        cp.resize(B); ri.resize(B); vx.resize(B); nc.resize(B);
        long long poff = 0, eoff = 0;
        for (int b = 0; b < B; ++b) {
            nc[b] = as_ll(ncb + b);
            if (nc[b] < 0) { sharp::set_error("a block with a negative number of cells"); *status = SHARP_ERR_ARG; return; }
            cp[b] = pcat + poff; ri[b] = icat + eoff; vx[b] = xcat + eoff;
            eoff += static_cast<long long>(cp[b][nc[b]]) - cp[b][0];
            poff += nc[b] + 1;
        }
        ok = true;
    }
};

/* what the Louvain and Leiden entries write per level, and the caller's table made of it: level_cap rows of (n, communities, rounds,
 * modularity), for Leiden of (n, communities, sub-communities, rounds, refine rounds, modularity) */
struct LevelsOut {
    const bool leiden;
    std::vector<long long> ln, lc, ls;
    std::vector<int> lr, lf;
    std::vector<double> lq;
    LevelsOut(int level_cap, bool leiden_) : leiden(leiden_) {
        const size_t cap = level_cap > 0 ? static_cast<size_t>(level_cap) : 1;
        ln.resize(cap); lc.resize(cap); ls.resize(cap); lr.resize(cap); lf.resize(cap); lq.resize(cap);
    }
    void write(int status, int nl, double *levels) const {
        if (status != 0) return;
        for (int l = 0; l < nl; ++l) {
            double *row = levels + (leiden ? 6 : 4) * l;
            *row++ = static_cast<double>(ln[l]);
            *row++ = static_cast<double>(lc[l]);
            if (leiden) *row++ = static_cast<double>(ls[l]);
            *row++ = static_cast<double>(lr[l]);
            if (leiden) *row++ = static_cast<double>(lf[l]);
            *row = lq[l];
        }
    }
};

}  // namespace

extern "C" {

void sharp_C_init(int *device, int *status) { *status = sharp_init(*device); }
void sharp_C_shutdown(int *status) { *status = sharp_shutdown(); }
void sharp_C_trim(int *status) { *status = sharp_trim(); }
void sharp_C_reload_options(int *status) { *status = sharp_reload_options(); }
void sharp_C_device_count(int *count, int *status) { *status = sharp_device_count(count); }

/* .C("sharp_C_last_error", msg = paste(rep(" ", 1024), collapse = ""), len = 1024L)$msg : the text is copied into the caller's string */
void sharp_C_last_error(char **msg, int *len) {
    const char *e = sharp_last_error();
    if (!msg || !msg[0] || !len || *len <= 0) return;
    std::strncpy(msg[0], e ? e : "", static_cast<size_t>(*len));
    msg[0][*len - 1] = '\0';
}

/* ---- a1: ranM / ranM2 / RPmat's projector (R/ranM.R:11-33, R/ranM2.R:11-35, R/RPmat.R:14-31) */
void sharp_C_projector_create(int *m, int *p, int *K, double *seeds, int *handle, int *status) {
    *status = sharp_projector_create(*m, *p, *K, seeds, handle);
}
void sharp_C_projector_destroy(int *handle, int *status) { *status = sharp_projector_destroy(*handle); }
/* nnz: in = capacity of gene / col / sign (0: only the count is wanted), out = the number of non-zeros of projector *k */
void sharp_C_projector_triplets(int *handle, int *k, int *gene, int *col, int *sign, double *nnz, int *status) {
    long long nn = 0;
    *status = sharp_projector_triplets(*handle, *k, nullptr, nullptr, nullptr, &nn);
    const long long cap = as_ll(nnz);
    *nnz = static_cast<double>(nn);
    if (*status != SHARP_OK || cap <= 0) return;
    if (cap < nn) { sharp::set_error("sharp_C_projector_triplets: buffers too small"); *status = SHARP_ERR_ARG; return; }
    std::vector<signed char> s(static_cast<size_t>(nn));
    *status = sharp_projector_triplets(*handle, *k, gene, col, s.data(), &nn);
    for (long long i = 0; i < nn; ++i) sign[i] = s[static_cast<size_t>(i)];
}

/* ---- a2: projmat of RPmat (R/RPmat.R:32; R/SHARP.R:343-345,363,579-585).  X: m x n column-major as R holds it; E: n x (K p) row-major
 * = R's (K p) x n matrix */
void sharp_C_project(int *proj, double *X, int *m, int *n, int *log_flag, double *E, int *status) {
    *status = sharp_project(*proj, X, *m, *n, static_cast<long long>(*m), *log_flag, E);
}

/* ---- a3-a5: get_opt_hclust (R/get_opt_hclust.R:33-244).  mat: n x p ROW-major, i.e. t(mat) of the R matrix.
 * want: bit 0 v (n x nk column-major; room for n * (min(maxN, n - 1) - minN + 1)), bit 1 msil/CHind, bit 2 height (n - 1) */
void sharp_C_get_opt_hclust(double *mat, int *n, int *p, int *hmethod, int *N_cluster, int *minN, int *maxN, double *sil_thre,
                            double *height_Ntimes, int *flashmark, int *f, int *v, double *msil, double *CHind, double *maxsil,
                            double *height, int *optN, int *nk, int *branch, int *want, int *status) {
    const int hm = flashmark_method(*flashmark, *hmethod, status);
    if (hm < 0) return;
    const int w = *want;
    *status = sharp_get_opt_hclust(mat, *n, *p, hm, *N_cluster, *minN, *maxN, *sil_thre, *height_Ntimes, f, (w & 1) ? v : nullptr,
                                   (w & 2) ? msil : nullptr, (w & 2) ? CHind : nullptr, maxsil, (w & 4) ? height : nullptr, optN, nk, branch);
}

/* ---- a6: getrowColor (R/getrowColor.R:17-121): rowColor[i] = index into colorL */
void sharp_C_getrowColor(double *E, int *n, int *p, int *hmethod, int *indN_cluster, int *minN, int *maxN, double *sil_thre,
                         double *height_Ntimes, int *flashmark, int *rowColor, double *maxsil, int *status) {
    const int hm = flashmark_method(*flashmark, *hmethod, status);
    if (hm < 0) return;
    *status = sharp_getrowColor(E, *n, *p, hm, *indN_cluster, *minN, *maxN, *sil_thre, *height_Ntimes, rowColor, maxsil);
}

/* ---- a9: wMetaC (R/wMetaC.R:15-226).  nC: N x C column-major integer labels (apply(nC, 2, function(x) match(x, unique(x)))).
 * want bit 0: x0 (N x *ncl column-major; room for N * (maxN + 2)) */
void sharp_C_wMetaC(int *nC, int *N, int *C, int *hmethod, int *enN_cluster, int *minN, int *maxN, double *sil_thre,
                    double *height_Ntimes, int *finalC, double *x0, int *ncl, int *want, int *status) {
    *status = sharp_wMetaC(nC, *N, *C, *hmethod, *enN_cluster, *minN, *maxN, *sil_thre, *height_Ntimes, finalC, (*want & 1) ? x0 : nullptr,
                           ncl, nullptr, nullptr, nullptr, nullptr);
}

/* ---- a10: sMetaC (R/sMetaC.R:17-210).  labels: match(rerowColor, unique(rerowColor)); sE1: n x p ROW-major (t(sE1) of the R matrix);
 * n as double.  tf: room for n entries (the first *nC are written) */
void sharp_C_sMetaC(int *labels, double *sE1, double *n, int *p, int *hmethod, int *finalN_cluster, int *minN, int *maxN,
                    double *sil_thre, double *height_Ntimes, int *finalColor, int *tf, int *nC, int *status) {
    *status = sharp_sMetaC(labels, sE1, as_ll(n), *p, *hmethod, *finalN_cluster, *minN, *maxN, *sil_thre, *height_Ntimes, finalColor, tf, nC);
}

/* ---- a7, a8, a12: SHARP / SHARP_small / SHARP_large (R/SHARP.R:44-318, 339-454, 478-851) on a prepared matrix.
 * X: genes x cells column-major (as.double(scExp)); n as double.  want: bit 0 viE (n x p row-major = R's p x n; room for n * p with
 * p = reduced.ndim or ceiling(log2(n)/0.04)), bit 1 x0 (n x *x0_cols column-major, room for n * *x0_cap_cols).
 * info[5]: n_pred, x0_cols, p_used, K_used, path (0 SHARP_small, 1 SHARP_large). */
void sharp_C_SHARP(double *X, int *m, double *n, int *ensize_K, int *reduced_ndim, int *base_ncells, int *partition_ncells, int *hmethod,
                   int *N_cluster, int *enpN_cluster, int *indN_cluster, int *minN, int *maxN, double *sil_thre, double *height_Ntimes,
                   int *flashmark, int *log_flag, int *projector, double *rN_seed, int *pred, double *viE, double *x0, int *x0_cap_cols,
                   int *info, int *want, int *status) {
    const int hm = flashmark_method(*flashmark, *hmethod, status);
    if (hm < 0) return;
    const int w = *want;
    *status = sharp_SHARP(X, *m, as_ll(n), static_cast<long long>(*m), *ensize_K, *reduced_ndim, *base_ncells, *partition_ncells, hm,
                          *N_cluster, *enpN_cluster, *indN_cluster, *minN, *maxN, *sil_thre, *height_Ntimes, *log_flag, *projector,
                          *rN_seed, pred, &info[0], (w & 1) ? viE : nullptr, (w & 2) ? x0 : nullptr, *x0_cap_cols, &info[1], &info[2],
                          &info[3], &info[4]);
}
/* the same for a Matrix::dgCMatrix: colptr = scExp@p, rowidx = scExp@i, val = scExp@x */
void sharp_C_SHARP_csc(int *colptr, int *rowidx, double *val, int *m, double *n, int *ensize_K, int *reduced_ndim, int *base_ncells,
                       int *partition_ncells, int *hmethod, int *N_cluster, int *enpN_cluster, int *indN_cluster, int *minN, int *maxN,
                       double *sil_thre, double *height_Ntimes, int *flashmark, int *log_flag, int *projector, double *rN_seed, int *pred,
                       double *viE, double *x0, int *x0_cap_cols, int *info, int *want, int *status) {
    const int hm = flashmark_method(*flashmark, *hmethod, status);
    if (hm < 0) return;
    const int w = *want;
    *status = sharp_SHARP_csc(colptr, rowidx, val, *m, as_ll(n), *ensize_K, *reduced_ndim, *base_ncells, *partition_ncells, hm, *N_cluster,
                              *enpN_cluster, *indN_cluster, *minN, *maxN, *sil_thre, *height_Ntimes, *log_flag, *projector, *rN_seed, pred,
                              &info[0], (w & 1) ? viE : nullptr, (w & 2) ? x0 : nullptr, *x0_cap_cols, &info[1], &info[2], &info[3], &info[4]);
}
/* allrpinfo of the last SHARP_small run (R/SHARP.R:350-387,446): dims[3] = n, K, p; want bit 0: enrp (n x K column-major colour
 * indices = the rowColor of every random projection), bit 1: indE (n x (K p) row-major: projection k is columns [k p, (k+1) p)) */
void sharp_C_last_rpinfo(int *dims, int *enrp, double *indE, int *want, int *status) {
    *status = sharp_last_rpinfo(&dims[0], &dims[1], &dims[2], (*want & 1) ? enrp : nullptr, (*want & 2) ? indE : nullptr);
}

/* ---- a11: SHARP_unlimited (R/SHARP_unlimited.R:29-242).  Xcat: the blocks one after the other, each m x ncb[b] column-major
 * (unlist(lapply(scExp, as.double))); ncb as doubles.  want bit 0: viE (ncells x p row-major, p = ceiling(log2(ncells)/0.04)).
 * info[2]: n_pred, p_used */
void sharp_C_SHARP_unlimited(double *Xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *N_cluster, int *minN, int *maxN,
                             double *rN_seed, int *pred, double *viE, int *info, int *want, int *status) {
    const DenseList L(Xcat, *nblocks, ncb, *m, status);
    if (!L.ok) return;
    *status = sharp_SHARP_unlimited_view(L.ptrs.data(), L.nc.data(), *nblocks, *m, *ensize_K, *N_cluster, *minN, *maxN, *rN_seed, pred, &info[0],
                                         &info[1], (*want & 1) ? viE : nullptr);
}
/* arms the device-side view reduction for the NEXT sharp_C_SHARP_unlimited* call (sharp_unlimited_view_dim; R/SHARP_unlimited.R:216-228): its viE
 * buffer is then ncells x *kdim */
void sharp_C_unlimited_view_dim(int *kdim, int *status) { *status = sharp_unlimited_view_dim(*kdim); }
void sharp_C_decision_log(int *enable, int *status) { *status = sharp_decision_log(*enable); }
void sharp_C_last_decisions(double *rows, int *cap_rows, int *n_rows, int *status) { *status = sharp_last_decisions(rows, *cap_rows, n_rows); }
/* the same on several GPUs (sharp_SHARP_unlimited_multi): devices = integer vector of device indices, block b on devices[b mod ndev] */
void sharp_C_SHARP_unlimited_multi(double *Xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *N_cluster, int *minN, int *maxN,
                                   double *rN_seed, int *devices, int *ndevices, int *pred, double *viE, int *info, int *want, int *status) {
    const DenseList L(Xcat, *nblocks, ncb, *m, status);
    if (!L.ok) return;
    *status = sharp_SHARP_unlimited_multi(L.ptrs.data(), L.nc.data(), *nblocks, *m, *ensize_K, *N_cluster, *minN, *maxN, *rN_seed, devices, *ndevices,
                                          pred, &info[0], &info[1], (*want & 1) ? viE : nullptr);
}
/* a list of dgCMatrix blocks (R/SHARP_unlimited.R:125-135 hands each block to SHARP() as it is; R/SHARP.R:343-345,579 take a dgCMatrix):
 * pcat = the blocks' @p one after the other (ncb[b] + 1 ints each), icat / xcat = their @i / @x one after the other.  *ndevices = 0: the
 * caller's GPU (or SHARP_DEVICES); else block b on devices[b mod *ndevices]. */
void sharp_C_SHARP_unlimited_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *N_cluster,
                                 int *minN, int *maxN, double *rN_seed, int *devices, int *ndevices, int *pred, double *viE, int *info,
                                 int *want, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    *status = sharp_SHARP_unlimited_csc_multi(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *ensize_K, *N_cluster, *minN, *maxN, *rN_seed,
                                              *ndevices > 0 ? devices : nullptr, *ndevices, pred, &info[0], &info[1], (*want & 1) ? viE : nullptr);
}
/* SHARP_unlimited2 (R/SHARP_unlimited2.R:29-292); same block layout */
void sharp_C_SHARP_unlimited2(double *Xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *reduced_ndim, int *partition_ncells,
                              int *hmethod, int *N_cluster, int *enpN, int *indN, int *minN, int *maxN, double *sil_thre,
                              double *height_Ntimes, int *flag, double *rN_seed, int *pred, double *viE, int *info, int *want, int *status) {
    const DenseList L(Xcat, *nblocks, ncb, *m, status);
    if (!L.ok) return;
    *status = sharp_SHARP_unlimited2(L.ptrs.data(), L.nc.data(), *nblocks, *m, *ensize_K, *reduced_ndim, *partition_ncells, *hmethod, *N_cluster, *enpN,
                                     *indN, *minN, *maxN, *sil_thre, *height_Ntimes, *flag, *rN_seed, pred, &info[0], &info[1],
                                     (*want & 1) ? viE : nullptr);
}
/* the merge step of a sharded run (R/SHARP_unlimited.R:163-183) on gathered centroid tables; counts and ncells as doubles */
void sharp_C_unlimited_merge(double *means, double *counts, int *nC, int *p, double *ncells, int *N_cluster, int *minN, int *maxN,
                             int *final_id, int *n_final, int *status) {
    std::vector<long long> cn(static_cast<size_t>(std::max(*nC, 0)));
    for (int q = 0; q < *nC; ++q) cn[q] = as_ll(counts + q);
    *status = sharp_unlimited_merge(means, cn.data(), *nC, *p, as_ll(ncells), *N_cluster, *minN, *maxN, final_id, n_final);
}

/* ---- get_marker_genes' per-gene pass (R/get_marker_genes.R:120-152); out: m x 5 row-major */
void sharp_C_marker_genes(double *X, int *m, double *n, int *label, int *n_cluster, double *theta, int *ng, double *out, int *status) {
    *status = sharp_marker_genes(X, *m, as_ll(n), static_cast<long long>(*m), label, *n_cluster, *theta, *ng, out);
}

/* ---- Rtsne, as visualization_SHARP calls it (R/visualization_SHARP.R:94); X: as.double(t(x1)), rows of d values */
void sharp_C_tsne(double *X, double *n, int *d, int *dims, int *initial_dims, int *pca, int *pca_center, int *pca_scale, int *normalize,
                  int *check_duplicates, double *perplexity, double *theta, int *max_iter, int *stop_lying_iter, int *mom_switch_iter,
                  double *momentum, double *final_momentum, double *eta, double *exaggeration, int *has_Y_init, double *Y_init, double *seed,
                  double *Y, double *itercosts, double *costs, int *status) {
    *status = sharp_tsne(X, as_ll(n), *d, static_cast<long long>(*d), *dims, *initial_dims, *pca, *pca_center, *pca_scale, *normalize,
                         *check_duplicates, *perplexity, *theta, *max_iter, *stop_lying_iter, *mom_switch_iter, *momentum, *final_momentum, *eta,
                         *exaggeration, *has_Y_init ? Y_init : nullptr, *seed, Y, itercosts, costs);
}

/* ---- Rtsne with its Barnes-Hut repulsion (sharp_tsne_bh), sharp_C_tsne's arguments */
void sharp_C_tsne_bh(double *X, double *n, int *d, int *dims, int *initial_dims, int *pca, int *pca_center, int *pca_scale, int *normalize,
                     int *check_duplicates, double *perplexity, double *theta, int *max_iter, int *stop_lying_iter, int *mom_switch_iter,
                     double *momentum, double *final_momentum, double *eta, double *exaggeration, int *has_Y_init, double *Y_init, double *seed,
                     double *Y, double *itercosts, double *costs, int *status) {
    *status = sharp_tsne_bh(X, as_ll(n), *d, static_cast<long long>(*d), *dims, *initial_dims, *pca, *pca_center, *pca_scale, *normalize,
                            *check_duplicates, *perplexity, *theta, *max_iter, *stop_lying_iter, *mom_switch_iter, *momentum, *final_momentum, *eta,
                            *exaggeration, *has_Y_init ? Y_init : nullptr, *seed, Y, itercosts, costs);
}

/* ---- Rtsne_neighbors / Rtsne(is_distance = TRUE) / the exact k-NN (sharp_tsne_neighbors, sharp_tsne_dist, sharp_tsne_knn): index
 * 0-based, n x K row-major (as.integer(t(index)) - 1L); X = as.double(t(X)) */
void sharp_C_tsne_neighbors(int *index, double *distance, double *n, int *K, int *squared, int *repulsion, int *dims, double *perplexity,
                            double *theta, int *max_iter, int *stop_lying_iter, int *mom_switch_iter, double *momentum,
                            double *final_momentum, double *eta, double *exaggeration, int *has_Y_init, double *Y_init, double *seed, double *Y,
                            double *itercosts, double *costs, int *status) {
    *status = sharp_tsne_neighbors(index, distance, as_ll(n), *K, *squared, *repulsion, *dims, *perplexity, *theta, *max_iter, *stop_lying_iter,
                                   *mom_switch_iter, *momentum, *final_momentum, *eta, *exaggeration, *has_Y_init ? Y_init : nullptr, *seed, Y,
                                   itercosts, costs);
}
void sharp_C_tsne_dist(double *d, int *n, int *repulsion, int *dims, double *perplexity, double *theta, int *max_iter, int *stop_lying_iter,
                       int *mom_switch_iter, double *momentum, double *final_momentum, double *eta, double *exaggeration, int *has_Y_init,
                       double *Y_init, double *seed, double *Y, double *itercosts, double *costs, int *status) {
    *status = sharp_tsne_dist(d, *n, *repulsion, *dims, *perplexity, *theta, *max_iter, *stop_lying_iter, *mom_switch_iter, *momentum,
                              *final_momentum, *eta, *exaggeration, *has_Y_init ? Y_init : nullptr, *seed, Y, itercosts, costs);
}
void sharp_C_tsne_knn(double *X, double *n, int *d, int *K, int *idx, double *dist, int *status) {
    *status = sharp_tsne_knn(X, as_ll(n), *d, static_cast<long long>(*d), *K, idx, dist);
}
void sharp_C_knn_descent(double *X, double *n, int *d, int *K, int *n_projections, int *max_candidates, int *n_iters, double *delta,
                         double *seed, int *idx, double *dist2, double *info, int *status) {
    long long inf[4] = {0, 0, 0, 0};
    *status = sharp_knn_descent(X, as_ll(n), *d, static_cast<long long>(*d), *K, *n_projections, *max_candidates, *n_iters, *delta, *seed, idx,
                                dist2, inf);
    for (int k = 0; k < 4; ++k) info[k] = static_cast<double>(inf[k]);
}

/* ---- uwot::umap beside Rtsne (sharp_umap, sharp_umap_neighbors, sharp_umap_ab): X = as.double(t(X)); index 0-based, n x K row-major */
void sharp_C_umap(double *X, double *n, int *d, int *n_neighbors, int *dims, int *n_epochs, double *learning_rate, double *min_dist,
                  double *spread, double *ab, int *negative_sample_rate, double *repulsion_strength, int *init, double *Y_init, int *pca,
                  int *pca_center, double *seed, double *Y, int *want_nn, int *nn_index, double *nn_distance, int *status) {
    *status = sharp_umap(X, as_ll(n), *d, static_cast<long long>(*d), *n_neighbors, *dims, *n_epochs, *learning_rate, *min_dist, *spread, ab,
                         *negative_sample_rate, *repulsion_strength, *init, *init == 2 ? Y_init : nullptr, *pca, *pca_center, *seed, Y,
                         *want_nn ? nn_index : nullptr, *want_nn ? nn_distance : nullptr);
}
void sharp_C_umap_neighbors(int *index, double *distance, double *n, int *K, int *squared, int *dims, int *n_epochs, double *learning_rate,
                            double *min_dist, double *spread, double *ab, int *negative_sample_rate, double *repulsion_strength, int *init,
                            double *Y_init, double *seed, double *Y, int *status) {
    *status = sharp_umap_neighbors(index, distance, as_ll(n), *K, *squared, *dims, *n_epochs, *learning_rate, *min_dist, *spread, ab,
                                   *negative_sample_rate, *repulsion_strength, *init, *init == 2 ? Y_init : nullptr, *seed, Y);
}
void sharp_C_umap_ab(double *spread, double *min_dist, double *a, double *b, int *status) { *status = sharp_umap_ab(*spread, *min_dist, a, b); }
/* umap_transform (sharp_umap_model_create, sharp_umap_model_free, sharp_umap_transform): X_ref / Xq = as.double(t(X)) */
void sharp_C_umap_model_create(double *X_ref, double *n_ref, int *d, double *Y_ref, int *dims, int *n_neighbors, double *a, double *b,
                               int *n_epochs, int *handle, int *status) {
    *status = sharp_umap_model_create(X_ref, as_ll(n_ref), *d, static_cast<long long>(*d), Y_ref, *dims, *n_neighbors, *a, *b, *n_epochs, handle);
}
void sharp_C_umap_model_free(int *handle, int *status) { *status = sharp_umap_model_free(*handle); }
void sharp_C_umap_transform(int *handle, double *Xq, double *nq, int *d, int *n_epochs, double *learning_rate, int *negative_sample_rate,
                            double *repulsion_strength, double *seed, double *row_offset, double *Yq, int *want_nn, int *nn_index,
                            double *nn_distance, int *status) {
    *status = sharp_umap_transform(*handle, Xq, as_ll(nq), static_cast<long long>(*d), *n_epochs, *learning_rate, *negative_sample_rate,
                                   *repulsion_strength, *seed, as_ll(row_offset), Yq, *want_nn ? nn_index : nullptr,
                                   *want_nn ? nn_distance : nullptr);
}

/* the spectral start's stages (sharp_umap_components, sharp_umap_spectral, sharp_umap_init_info): row_ptr, n and the counts as double */
static std::vector<long long> row_ptr_ll(const double *row_ptr, long long n) {   // (an n the library refuses: nothing is read)
    std::vector<long long> rp(n >= 1 && n < INT_MAX ? static_cast<size_t>(n) + 1 : 1, 0);
    for (size_t i = 0; rp.size() > 1 && i < rp.size(); ++i) rp[i] = as_ll(row_ptr + i);
    return rp;
}
void sharp_C_umap_components(double *row_ptr, int *col, double *n, int *label, double *count, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    long long k = 0;
    *status = sharp_umap_components(rp.data(), col, nn, label, &k);
    *count = static_cast<double>(k);
}
void sharp_C_umap_spectral(double *row_ptr, int *col, double *val, double *n, int *dims, double *tol, int *max_steps, double *V, double *theta,
                           double *residual, int *steps, double *components, int *outcome, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    long long k = 0;
    *status = sharp_umap_spectral(rp.data(), col, val, nn, *dims, *tol, *max_steps, V, theta, residual, steps, &k, outcome);
    *components = static_cast<double>(k);
}
void sharp_C_umap_init_info(int *requested, int *used, double *components, int *steps, double *residual, int *status) {
    long long k = 0;
    *status = sharp_umap_init_info(requested, used, &k, steps, residual);
    *components = static_cast<double>(k);
}

/* ---- dist / hclust (the clustering pheatmap does inside plot_markers, R/plot_markers.R:214-237): x = as.double(t(x)) */
void sharp_C_dist(double *x, int *n, int *p, int *method, double *minkowski_p, double *d_out, int *status) {
    *status = sharp_dist(x, *n, *p, static_cast<long long>(*p), *method, *minkowski_p, d_out);
}
void sharp_C_hclust_dist(double *d, int *n, int *hmethod, int *merge, double *height, int *order, int *status) {
    *status = sharp_hclust_dist(d, *n, *hmethod, merge, height, order);
}
void sharp_C_hclust(double *x, int *n, int *p, int *dist_method, double *minkowski_p, int *hmethod, int *merge, double *height, int *order,
                    int *status) {
    *status = sharp_hclust(x, *n, *p, static_cast<long long>(*p), *dist_method, *minkowski_p, *hmethod, merge, height, order);
}

/* ---- cluster::silhouette and the Calinski-Harabasz index on any labelling (validity.hip): x = as.double(t(x)), n as double; cl = the
 * codes 1 .. k (as.integer(factor(labels))) */
void sharp_C_silhouette_dist(double *d, int *n, int *cl, int *k, int *neighbor, double *width, int *status) {
    *status = sharp_silhouette_dist(d, *n, cl, *k, neighbor, width);
}
void sharp_C_silhouette(double *x, double *n, int *p, int *dist_method, double *minkowski_p, int *cl, int *k, int *neighbor, double *width,
                        int *status) {
    *status = sharp_silhouette(x, as_ll(n), *p, static_cast<long long>(*p), *dist_method, *minkowski_p, cl, *k,
                               neighbor, width);
}
void sharp_C_calinski_harabasz(double *x, double *n, int *p, int *cl, int *k, int *kind, double *out, int *status) {
    *status = sharp_calinski_harabasz(x, as_ll(n), *p, static_cast<long long>(*p), cl, *k, *kind, out);
}
void sharp_C_neighbor_ranks(double *X, double *n, int *d, int *K, int *index, int *max_rows_per_launch, int *rank_out, int *status) {
    *status = sharp_neighbor_ranks(X, as_ll(n), *d, static_cast<long long>(*d), *K, index, *max_rows_per_launch, rank_out);
}

/* Louvain on a graph or on neighbour lists (sharp_louvain_graph, sharp_louvain_neighbors, sharp_louvain_modularity): row_ptr and n as
 * double; levels: level_cap rows of (n, communities, rounds, modularity) */
void sharp_C_louvain_graph(double *row_ptr, int *col, double *val, double *n, double *resolution, double *tol, int *max_levels, int *max_rounds,
                           int *max_fails, double *seed, int *membership, int *level_cap, double *levels, int *n_levels, int *want_levels,
                           int *level_membership, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    LevelsOut o(*level_cap, false);
    *status = sharp_louvain_graph(rp.data(), col, val, nn, *resolution, *tol, *max_levels, *max_rounds, *max_fails, *seed, membership, *level_cap,
                                  o.ln.data(), o.lc.data(), o.lr.data(), o.lq.data(), n_levels, *want_levels ? level_membership : nullptr);
    o.write(*status, *n_levels, levels);
}
void sharp_C_louvain_neighbors(int *index, double *distance, double *n, int *K, int *squared, double *resolution, double *tol, int *max_levels,
                               int *max_rounds, int *max_fails, double *seed, int *membership, int *level_cap, double *levels, int *n_levels,
                               int *want_levels, int *level_membership, int *status) {
    LevelsOut o(*level_cap, false);
    *status = sharp_louvain_neighbors(index, distance, as_ll(n), *K, *squared, *resolution, *tol, *max_levels, *max_rounds, *max_fails, *seed,
                                      membership, *level_cap, o.ln.data(), o.lc.data(), o.lr.data(), o.lq.data(), n_levels,
                                      *want_levels ? level_membership : nullptr);
    o.write(*status, *n_levels, levels);
}
void sharp_C_louvain_modularity(double *row_ptr, int *col, double *val, double *n, int *membership, double *resolution, double *Q, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    *status = sharp_louvain_modularity(rp.data(), col, val, nullptr, nn, membership, *resolution, Q);
}

/* Leiden (sharp_leiden_graph, sharp_leiden_neighbors, sharp_leiden_snn): as the Louvain entries; levels: level_cap rows of (n,
 * communities, sub-communities, rounds, refine rounds, modularity) */
void sharp_C_leiden_graph(double *row_ptr, int *col, double *val, double *n, double *resolution, double *tol, int *max_levels, int *max_rounds,
                          int *max_fails, int *max_refine_rounds, double *seed, int *membership, double *modularity, int *level_cap, double *levels,
                          int *n_levels, int *want_levels, int *level_membership, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    LevelsOut o(*level_cap, true);
    *status = sharp_leiden_graph(rp.data(), col, val, nn, *resolution, *tol, *max_levels, *max_rounds, *max_fails, *max_refine_rounds, *seed,
                                 membership, modularity, *level_cap, o.ln.data(), o.lc.data(), o.ls.data(), o.lr.data(), o.lf.data(), o.lq.data(),
                                 n_levels, *want_levels ? level_membership : nullptr);
    o.write(*status, *n_levels, levels);
}
void sharp_C_leiden_neighbors(int *index, double *distance, double *n, int *K, int *squared, double *resolution, double *tol, int *max_levels,
                              int *max_rounds, int *max_fails, int *max_refine_rounds, double *seed, int *membership, double *modularity,
                              int *level_cap, double *levels, int *n_levels, int *want_levels, int *level_membership, int *status) {
    LevelsOut o(*level_cap, true);
    *status = sharp_leiden_neighbors(index, distance, as_ll(n), *K, *squared, *resolution, *tol, *max_levels, *max_rounds, *max_fails,
                                     *max_refine_rounds, *seed, membership, modularity, *level_cap, o.ln.data(), o.lc.data(), o.ls.data(),
                                     o.lr.data(), o.lf.data(), o.lq.data(), n_levels, *want_levels ? level_membership : nullptr);
    o.write(*status, *n_levels, levels);
}
void sharp_C_leiden_snn(int *index, double *n, int *K, double *prune, double *resolution, double *tol, int *max_levels, int *max_rounds,
                        int *max_fails, int *max_refine_rounds, double *seed, int *membership, double *modularity, int *level_cap, double *levels,
                        int *n_levels, int *want_levels, int *level_membership, int *status) {
    LevelsOut o(*level_cap, true);
    *status = sharp_leiden_snn(index, as_ll(n), *K, *prune, *resolution, *tol, *max_levels, *max_rounds, *max_fails, *max_refine_rounds, *seed,
                               membership, modularity, *level_cap, o.ln.data(), o.lc.data(), o.ls.data(), o.lr.data(), o.lf.data(), o.lq.data(),
                               n_levels, *want_levels ? level_membership : nullptr);
    o.write(*status, *n_levels, levels);
}

/* The SNN graph (sharp_snn_graph: the same count-then-fill protocol) and Louvain on it (sharp_louvain_snn): n, cap, nnz and row_ptr
 * as double; want: 1 fill col / val (0: the count alone), 2 shared as well */
void sharp_C_snn_graph(int *index, double *n, int *K, double *prune, double *cap, double *row_ptr, int *col, double *val, int *shared, int *want,
                       double *nnz, int *status) {
    const long long nn = as_ll(n);
    std::vector<long long> rp(nn > 0 && nn <= (1ll << 24) ? static_cast<size_t>(nn) + 1 : 1, 0);   // (another n is refused before row_ptr is written)
    long long z = 0;
    const bool fill = (*want & 1) != 0;
    *status = sharp_snn_graph(index, nn, *K, *prune, as_ll(cap), rp.data(), fill ? col : nullptr, fill ? val : nullptr,
                              fill && (*want & 2) ? shared : nullptr, &z);
    *nnz = static_cast<double>(z);
    if (*status == 0)
        for (long long i = 0; i <= nn; ++i) row_ptr[i] = static_cast<double>(rp[i]);
}
void sharp_C_louvain_snn(int *index, double *n, int *K, double *prune, double *resolution, double *tol, int *max_levels, int *max_rounds,
                         int *max_fails, double *seed, int *membership, int *level_cap, double *levels, int *n_levels, int *want_levels,
                         int *level_membership, int *status) {
    LevelsOut o(*level_cap, false);
    *status = sharp_louvain_snn(index, as_ll(n), *K, *prune, *resolution, *tol, *max_levels, *max_rounds, *max_fails, *seed, membership,
                                *level_cap, o.ln.data(), o.lc.data(), o.lr.data(), o.lq.data(), n_levels, *want_levels ? level_membership : nullptr);
    o.write(*status, *n_levels, levels);
}

/* The truncated PCA of sparse expression blocks: the plain entries' bits */
void sharp_C_expr_pca_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *n_components, int *oversample,
                          int *n_iter, double *normalize_total, int *log1p, int *scale, double *seed, double *scores, double *loadings,
                          double *singular_values, double *sdev, double *center, double *scale_out, double *gene_var, double *total_var,
                          int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    *status = sharp_expr_pca_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *n_components, *oversample, *n_iter,
                                 *normalize_total, *log1p, *scale, as_ll(seed), scores, loadings, singular_values, sdev, center, scale_out,
                                 gene_var, total_var);
}
void sharp_C_expr_stats_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total, int *log1p,
                            double *mean, double *var, double *nnz, double *cell_sum, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    std::vector<long long> z(*m > 0 ? static_cast<size_t>(*m) : 1, 0);
    *status = sharp_expr_stats_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *normalize_total, *log1p, mean, var,
                                   z.data(), cell_sum);
    if (*status == 0)
        for (int g = 0; g < *m; ++g) nnz[g] = static_cast<double>(z[g]);
}
void sharp_C_expr_pca_transform_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total, int *log1p,
                                    double *loadings, double *center, double *scale, int *n_components, double *scores, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    *status = sharp_expr_pca_transform_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *normalize_total, *log1p,
                                           loadings, center, scale, *n_components, scores);
}

/* Gene subsets and variable-gene selection: *n_genes = 0 stands for all genes */
void sharp_C_expr_pca_sub_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *n_components, int *oversample,
                              int *n_iter, double *normalize_total, int *log1p, int *scale, double *seed, double *scores, double *loadings,
                              double *singular_values, double *sdev, double *center, double *scale_out, double *gene_var, double *total_var,
                              int *genes, int *n_genes, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    *status = sharp_expr_pca_sub_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *n_components, *oversample, *n_iter,
                                     *normalize_total, *log1p, *scale, as_ll(seed), scores, loadings, singular_values, sdev, center,
                                     scale_out, gene_var, total_var, *n_genes ? genes : nullptr, *n_genes);
}
void sharp_C_expr_stats_sub_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total, int *log1p,
                                double *mean, double *var, double *nnz, double *cell_sum, int *genes, int *n_genes, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    std::vector<long long> z(*m > 0 ? static_cast<size_t>(*m) : 1, 0);
    *status = sharp_expr_stats_sub_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *normalize_total, *log1p, mean, var,
                                       z.data(), cell_sum, *n_genes ? genes : nullptr, *n_genes);
    if (*status == 0)
        for (int g = 0; g < (*n_genes ? *n_genes : *m); ++g) nnz[g] = static_cast<double>(z[g]);
}
void sharp_C_expr_pca_transform_sub_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total,
                                        int *log1p, double *loadings, double *center, double *scale, int *n_components, double *scores,
                                        int *genes, int *n_genes, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    *status = sharp_expr_pca_transform_sub_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *normalize_total, *log1p,
                                               loadings, center, scale, *n_components, scores, *n_genes ? genes : nullptr, *n_genes);
}
void sharp_C_expr_hvg_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *n_top_genes, double *span, double *means,
                          double *variances, double *variances_expected, double *variances_norm, int *rank, int *highly_variable, int *genes,
                          int *n_selected, int *q, int *degree_counts, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    *status = sharp_expr_hvg_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *n_top_genes, *span, means, variances,
                                 variances_expected, variances_norm, rank, highly_variable, genes, n_selected, q, degree_counts);
}

/* The batch integration of PCA scores: the plain entry's bits */
void sharp_C_harmony(double *Z, double *n, int *d, int *batch, int *n_batches, int *n_clusters, double *sigma, double *theta, double *lam,
                     int *max_iter, int *max_iter_cluster, int *n_blocks, double *epsilon_cluster, double *epsilon_harmony, int *init_iter,
                     double *seed, double *Z_corr, double *Y, double *objective, int *rounds, int *n_iter, int *converged, int *want_R, double *R,
                     int *status) {
    *status = sharp_harmony(Z, as_ll(n), *d, batch, *n_batches, *n_clusters, *sigma, *theta, *lam, *max_iter, *max_iter_cluster, *n_blocks,
                            *epsilon_cluster, *epsilon_harmony, *init_iter, as_ll(seed), Z_corr, Y, objective, rounds, n_iter, converged,
                            *want_R ? R : nullptr);
}

/* Doublet detection: the plain entry's bits */
void sharp_C_scrublet_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *sim_doublet_ratio,
                          double *expected_doublet_rate, int *n_neighbors, int *n_prin_comps, int *n_top_genes, int *genes, int *n_genes,
                          int *have_fit, double *fit_scores, double *fit_loadings, double *fit_center, double *fit_scale,
                          double *normalize_total, int *log1p, int *scale, double *threshold, int *nn_method, int *have_nn_args,
                          double *nn_args, double *seed, int *max_doublets_per_slab, double *doublet_scores, double *doublet_scores_sim,
                          int *predicted, double *threshold_out, int *threshold_found, double *rates, int *n_neighbors_out, int *k_adj_out,
                          int *parents, int *genes_out, int *n_genes_out, int *neighbor_counts, int *want_sim_pca, double *sim_pca,
                          int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    long long n = 0, n_sim = 0;
    for (int b = 0; b < *nblocks; ++b) n += L.nc[b];
    int nn = 0, ka = 0;
    *status = sharp_doublet_plan(n, *sim_doublet_ratio, *n_neighbors, &n_sim, &nn, &ka);
    if (*status != 0) return;
    std::vector<long long> par(static_cast<size_t>(n_sim) * 2);
    const bool fit = *have_fit != 0;
    *status = sharp_scrublet_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, *sim_doublet_ratio, *expected_doublet_rate,
                                 *n_neighbors, *n_prin_comps, *n_top_genes, *n_genes ? genes : nullptr, *n_genes, fit ? fit_scores : nullptr,
                                 fit ? fit_loadings : nullptr, fit ? fit_center : nullptr, fit ? fit_scale : nullptr, *normalize_total, *log1p,
                                 *scale, *threshold, *nn_method, *have_nn_args ? nn_args : nullptr, as_ll(seed), *max_doublets_per_slab,
                                 doublet_scores, doublet_scores_sim, predicted, threshold_out, threshold_found, rates, n_neighbors_out,
                                 k_adj_out, par.data(), genes_out, n_genes_out, neighbor_counts, *want_sim_pca ? sim_pca : nullptr);
    if (*status == 0)
        for (size_t e = 0; e < par.size(); ++e) parents[e] = static_cast<int>(par[e]);
}

/* Diffusion maps and pseudotime: the plain entries' bits; row_ptr, n, root and the counts as double */
void sharp_C_diffmap_graph(double *row_ptr, int *col, double *val, double *n, int *n_comps, int *density_normalize, double *root, double *tol,
                           int *max_matvecs, double *evals, double *evecs, double *residual, int *in_component, int *steps, int *restarts,
                           double *components, double *component_size, int *outcome, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    long long k = 0, cs = 0;
    *status = sharp_diffmap_graph(rp.data(), col, val, nn, *n_comps, *density_normalize, as_ll(root), *tol, *max_matvecs, evals, evecs, residual,
                                  in_component, steps, restarts, &k, &cs, outcome);
    *components = static_cast<double>(k);
    *component_size = static_cast<double>(cs);
}
void sharp_C_diffmap_neighbors(int *index, double *distance, double *n, int *K, int *squared, int *n_comps, int *density_normalize, double *root,
                               double *tol, int *max_matvecs, double *evals, double *evecs, double *residual, int *in_component, int *steps,
                               int *restarts, double *components, double *component_size, int *outcome, int *status) {
    long long k = 0, cs = 0;
    *status = sharp_diffmap_neighbors(index, distance, as_ll(n), *K, *squared, *n_comps, *density_normalize, as_ll(root), *tol, *max_matvecs,
                                      evals, evecs, residual, in_component, steps, restarts, &k, &cs, outcome);
    *components = static_cast<double>(k);
    *component_size = static_cast<double>(cs);
}
void sharp_C_diffmap_transitions(double *row_ptr, int *col, double *val, double *n, int *density_normalize, double *a, double *z, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    *status = sharp_diffmap_transitions(rp.data(), col, val, nn, *density_normalize, a, z);
}
void sharp_C_diffmap_component(double *row_ptr, int *col, double *val, double *n, int *n_comps, double *root, int *label, double *components,
                               double *sub_n, double *sub_nnz, double *sub_row_ptr, int *sub_col, double *sub_val, int *new_id, int *status) {
    const long long nn = as_ll(n);
    const std::vector<long long> rp = row_ptr_ll(row_ptr, nn);
    std::vector<long long> srp(rp.size(), 0);
    long long k = 0, sn = 0, snnz = 0;
    *status = sharp_diffmap_component(rp.data(), col, val, nn, *n_comps, as_ll(root), label, &k, &sn, &snnz, srp.data(), sub_col, sub_val, new_id);
    *components = static_cast<double>(k);
    *sub_n = static_cast<double>(sn);
    *sub_nnz = static_cast<double>(snnz);
    if (*status == 0)
        for (long long i = 0; i <= sn; ++i) sub_row_ptr[i] = static_cast<double>(srp[i]);
}
void sharp_C_dpt(double *evals, double *evecs, double *n, int *n_comps, int *n_dcs, int *roots, int *n_roots, int *normalize, double *out,
                 int *status) {
    *status = sharp_dpt(evals, evecs, as_ll(n), *n_comps, *n_dcs, roots, *n_roots, *normalize, out);
}

/* rank_genes_groups: the plain entry's bits; group_sizes as double, order as int */
void sharp_C_rank_genes_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *labels, int *n_groups, int *method,
                            int *reference, double *normalize_total, int *log1p, int *genes, int *n_genes, int *tie_correct, int *continuity,
                            int *n_order, double *group_sizes, double *scores, double *pvals, double *pvals_adj, double *logfoldchanges,
                            double *auc, double *means, double *means_ref, double *pct, double *pct_ref, int *order, int *status) {
    const CscList L(pcat, icat, xcat, *nblocks, ncb, status);
    if (!L.ok) return;
    const size_t G = static_cast<size_t>(std::max(*n_groups, 0)), no = static_cast<size_t>(std::max(*n_order, 0));
    std::vector<long long> sizes(G + 1), ord(G * no + 1);                 // (never empty: a bad count is refused by name inside)
    *status = sharp_rank_genes_csc(L.cp.data(), L.ri.data(), L.vx.data(), L.nc.data(), *nblocks, *m, labels, *n_groups, *method, *reference,
                                   *normalize_total, *log1p, *n_genes ? genes : nullptr, *n_genes, *tie_correct, *continuity, *n_order,
                                   sizes.data(), scores, pvals, pvals_adj, logfoldchanges, auc, means, means_ref, pct, pct_ref, ord.data());
    if (*status != 0) return;
    for (size_t g = 0; g < G; ++g) group_sizes[g] = static_cast<double>(sizes[g]);
    for (size_t e = 0; e < G * no; ++e) order[e] = static_cast<int>(ord[e]);
}

}  // extern "C"
