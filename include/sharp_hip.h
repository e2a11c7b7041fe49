/*
 * sharp_hip.h -- C ABI of libsharp_hip.so: the MI355X (gfx950) implementation of
 * SHARP's ensemble random-projection + meta-clustering hot path.
 *
 * The reference (shibiaowan/SHARP) is pure R with no FFI (NAMESPACE has no
 * useDynLib), so the drop-in boundary is the set of exported R functions
 * (SURVEY.md 8b).  Each entry point below replaces the body of one of them and
 * cites it; INTEGRATION.md shows the R glue (.C / .Call) and the ctypes binding.
 *
 * Conventions
 *   - plain C, pointers + sizes only; no R, torch or C++ types in any signature.
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from sharp_last_error() (reference convention: stop("..."),
 *     R/SHARP.R:52-54,171-176; R/get_opt_hclust.R:91-99).  Nothing aborts.
 *   - the caller owns every host buffer; the library owns device memory and the
 *     state behind integer handles.
 *   - matrices: X is genes x cells, COLUMN-major (a cell is a contiguous m-vector),
 *     exactly R's layout.  E / viE are cells x p ROW-major (= R's p x n column-major
 *     projmat before the transpose at R/SHARP.R:363,583).  Label matrices (enrp, v)
 *     are column-major like R.
 *   - cluster ids are 1-based like R.  "NULL" integer arguments are passed as 0.
 *   - hmethod codes follow stats::hclust's method table:
 *       1 ward.D  2 single  3 complete  4 average  5 mcquitty  6 median  7 centroid  8 ward.D2
 *   - functions ending in _dev take DEVICE pointers (HBM-resident data, e.g. from
 *     hipMalloc or a torch tensor's data_ptr()) and run on the library's stream.
 *   - single-threaded callers (R's main thread); the library never calls back.
 *   - the `sharp_C_*` entry points at the end of this header are the same calls in R's .C()
 *     convention (every argument a pointer, void return, int* status out), so the reference's
 *     R functions can call the library with no glue compiled against R.h (r/sharp_hip.R);
 *     r/sharp_glue.c is the .Call shim that avoids .C()'s argument copies.
 */
#ifndef SHARP_HIP_H
#define SHARP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SHARP_OK 0
#define SHARP_ERR 1          /* generic failure, see sharp_last_error()           */
#define SHARP_ERR_ARG 2      /* argument rejected (what R's stop() checks reject) */
#define SHARP_ERR_NO_DEVICE 3
#define SHARP_WARN_RANGE 16  /* model selection ran off the candidate range (reference quirk 8) */
#define SHARP_WARN_NA_VOTE 32/* wMetaC single-cluster fallback met a cell with one vote value (quirk 11) */

/* ---- runtime -------------------------------------------------------------- */
const char *sharp_last_error(void);
int sharp_version(void);
int sharp_device_count(int *count);
/* Select the GPU and create the library's stream/workspace.  Idempotent per device. */
int sharp_init(int device);
int sharp_shutdown(void);
int sharp_synchronize(void);
/* The library reads its tuning switches (SHARP_* environment variables: kernel forms, chunk sizes, pipeline depths -- none changes a
 * result) ONCE, at its first use; this re-reads them, for a host that changes its environment afterwards (the tests do). */
int sharp_reload_options(void);
/* Per-kernel HIP-event timing on the library's stream (used by bench.py's roofline). */
int sharp_profile_enable(int on);
int sharp_profile_reset(void);
/* name: e.g. "rp_scatter"; returns total milliseconds and launch count since reset. */
int sharp_profile_get(const char *name, double *total_ms, long long *launches);
/* writes a '\n'-separated "name total_ms launches" table into buf (NUL-terminated). */
int sharp_profile_dump(char *buf, int buflen);

/* ---- a1: ranM / ranM2 / projector half of RPmat ---------------------------- */
/* R/ranM.R:11-33, R/ranM2.R:11-35, R/RPmat.R:14-31.
 * Builds K sparse ternary projectors R_k (m x p) with R's own RNG stream:
 * set.seed(seeds[k]); sample(c(sqrt(s),0,-sqrt(s)), m*p, TRUE, c(1/2s,1-1/s,1/2s));
 * byrow fill.  seeds[k] must be integer-valued (50 + rN.seed + k at the call sites
 * R/SHARP.R:360,545, R/SHARP_unlimited.R:101); a non-integer seed (the reference's
 * 0.5 "unseeded" sentinel) draws a seed from the OS entropy source.
 * The projectors are kept on the device as gene-major packed row lists. */
int sharp_projector_create(int m, int p, int K, const double *seeds, int *handle);
int sharp_projector_destroy(int handle);
int sharp_projector_info(int handle, int *m, int *p, int *K, long long *nnz_total);
/* ranM() drop-in: the k-th (0-based) projector as COO triplets sorted row-major
 * (gene, then column): gene[i], col[i] 0-based, sign[i] = +1/-1; value = sign*sqrt(sqrt(m)).
 * Call with gene == NULL to get *nnz only. */
int sharp_projector_triplets(int handle, int k, int *gene, int *col, signed char *sign, long long *nnz);

/* ---- a2: RP matmul  E1 = t( 1/sqrt(p) * t(R_k) %*% log2(X+1) ) -------------- */
/* R/RPmat.R:32, R/SHARP.R:343-345,363,569-571,579-585.
 * Host variant: X double, m x n column-major with leading dimension ld (>= m).
 * E: n x (K*p) row-major, component k*p + c = projector k, column c.
 * X is kept on the device as fp32 when every value is fp32-exact, else as fp64 (sharp_x_storage(),
 * DESIGN.md "Numerics").  log_flag: 1 = log2(x+1) (flag TRUE), 0 = raw. */
int sharp_project(int proj, const double *X, int m, int n, long long ld, int log_flag, double *E);
/* Device variant: dX fp32 (m x n, leading dimension ld elements, 16-byte aligned columns
 * when ld % 4 == 0), dE fp64 n x ldE row-major (ldE >= K*p). */
int sharp_project_dev(int proj, const float *dX, int m, int n, long long ld, int log_flag,
                      double *dE, long long ldE);
/* The same for an fp64 block that is already resident: TPM / CPM-like doubles (the reference's own example data, README.md:88,114;
 * R/SHARP.R:110-117 computes log2(X + 1) and the projection in double), which the fp32 form would perturb by 6e-8 relative.
 * dX must be 16-byte aligned with an even ld >= m and hold finite values (one pass over it finds max |x| and checks that).  The
 * *_dev64 entry points below take the same kind of block. */
int sharp_project_dev64(int proj, const double *dX, int m, int n, long long ld, int log_flag,
                        double *dE, long long ldE);

/* ---- a3-a5: get_opt_hclust --------------------------------------------------- */
/* R/get_opt_hclust.R:33-244.  mat: n x p ROW-major feature rows, or an n x n symmetric similarity
 * (detected like isSymmetric(): square and all.equal(mat, t(mat), 100*eps)); then d = 1 - mat.
 * Feature rows: t(scale(t(mat))), d = 1 - cor(t(mat)) (fp64 MFMA), hclust(d, method), cutree for
 * k = minN..min(maxN, n-1), median silhouette, get_CH(.., "1-corr"), and the reference's choice rule
 * (middle arg-max of msil; CH when max(msil) <= sil_thre; height gap when CH picks the first k).
 * N_cluster: 0 = NULL, else a single cutree(k = N_cluster).
 * Outputs (caller-allocated; any of v, msil, CHind, maxsil, height, optN, nk, branch may be NULL):
 *   f[n] chosen labels (1-based, numbered by first appearance); v[n * nk] column-major;
 *   msil[nk], CHind[nk]; height[n-1]; branch: 0 silhouette, 1 CH, 2 height gap.
 * Returns SHARP_OK, SHARP_WARN_RANGE (choice clamped into the candidate range, reference quirk 8:
 * R would raise "subscript out of bounds") or an error code. */
int sharp_get_opt_hclust(const double *mat, int n, int p, int hmethod, int N_cluster, int minN, int maxN,
                         double sil_thre, double height_Ntimes, int *f, int *v, double *msil, double *CHind,
                         double *maxsil, double *height, int *optN, int *nk, int *branch);

/* ---- a6: getrowColor ----------------------------------------------------------- */
/* ---- the decision log -------------------------------------------------
 * Every choice of a number of clusters on the path is an arg-max over doubles compared with `==` (R/get_opt_hclust.R:162-168: the middle one of
 * the exact ties of the median silhouette; :194-195: which.max(CHind) when max(msil) <= sil.thre; :196-210: the height-gap rule;
 * R/sMetaC.R:139-148: the two-cluster override).  sharp_decision_log(1) (or SHARP_DECISION_LOG=1 in the environment) makes every
 * get_opt_hclust call of the process leave one row of SHARP_DECISION_COLS doubles; sharp_decision_log(0) stops and clears.
 * sharp_last_decisions copies up to cap_rows rows, sorted by (level, block, k, fold), and returns the number held in *n_rows.  Row:
 *  [0] level: 0 base clustering of one projection of one fold (getrowColor, R/SHARP.R:366,592), 1 a fold's wMetaC (R/wMetaC.R:98-99),
 *      2 the sMetaC across a block's folds (R/SHARP.R:754), 3 SHARP_unlimited's sMetaC across blocks (R/SHARP_unlimited.R:163), -1 a direct call
 *  [1] block (index in the SHARP_unlimited list; 0 for SHARP())  [2] k (projection, 0-based)  [3] fold (0-based)  [4] observations
 *  [5] branch: 0 median silhouette, 1 CH, 2 height gap, 3 N.cluster given   [6] chosen number of clusters
 *  [7] exact ties at the deciding maximum  [8] that maximum (msil: branch 0 / 3, CH: 1 / 2)  [9] largest value strictly below it (NaN: none)
 *  [10] max(msil) - sil.thre  [11] height rule, when CH's first level won: gap / ((height.Ntimes - 1) * height) of the deciding step
 *       (branch 2: > 1) or its maximum over the last ten merges (branch 1: <= 1); NaN otherwise
 *  [12] sMetaC's two-cluster override: the number of clusters of the column taken instead (0: not applied)  [13] candidate levels
 * oracle/sharp_oracle.c writes the same rows (oracle_decision_log / oracle_last_decisions): tests compare the two logs entry by entry. */
#define SHARP_DECISION_COLS 14
int sharp_decision_log(int enable);
int sharp_last_decisions(double *rows /* cap_rows x SHARP_DECISION_COLS */, int cap_rows, int *n_rows);

/* R/getrowColor.R:17-121.  rowColor[i] in 1..40 is the index into the reference's colorL table
 * (cluster j > 40 wraps and collides exactly like :59-68); height_Ntimes <= 0 -> 1 (:28-30). */
int sharp_getrowColor(const double *E, int n, int p, int hmethod, int indN_cluster, int minN, int maxN,
                      double sil_thre, double height_Ntimes, int *rowColor, double *maxsil);

/* ---- a9: wMetaC ------------------------------------------------------------------ */
/* R/wMetaC.R:15-226 (+ getA :242-283, getss :299-311, getnewk :313-320).
 * nC: N x C column-major integer labels (the reference's strings only ever compare for equality
 * within a column).  finalC[N]: meta-cluster id per cell (the number R stores as a string; ties in the
 * vote go to the id whose decimal string sorts first, like names(sort(table(d), decreasing=TRUE)[1])).
 * x0 (optional): N x *ncl column-major soft matrix (caller buffer of N * min(maxN, allC-1) doubles).
 * Optional intermediates for stage-wise checks: w1_out[N], S_out[allC*allC], tf_out[allC], *allC_out.
 * Returns SHARP_OK, or warning bits SHARP_WARN_RANGE / SHARP_WARN_NA_VOTE, or an error code. */
int sharp_wMetaC(const int *nC, int N, int C, int hmethod, int enN_cluster, int minN, int maxN, double sil_thre,
                 double height_Ntimes, int *finalC, double *x0, int *ncl, double *w1_out, double *S_out, int *allC_out,
                 int *tf_out);

/* ---- a10: sMetaC ----------------------------------------------------------------- */
/* R/sMetaC.R:17-210.  labels[n]: integers, equal <=> same label string; sE1: n x p row-major.
 * finalColor[n]: meta id per cell; tf_out[nC] (optional): meta id per unique label in
 * first-appearance order; `folds` is unused by the reference and has no counterpart here. */
int sharp_sMetaC(const int *labels, const double *sE1, long long n, int p, int hmethod, int finalN_cluster, int minN,
                 int maxN, double sil_thre, double height_Ntimes, int *finalColor, int *tf_out, int *nC_out);

/* ---- a7, a8, a12: SHARP / SHARP_small / SHARP_large -------------------------------- */
/* R/SHARP.R:44-318 (front door), :339-454 (SHARP_small), :478-851 (SHARP_large), for a matrix that
 * already went through the host-side preparation (dedupe, prep, CPM: the Python/R glue does those).
 * Arguments <= 0 (sil_thre < 0) take the reference defaults: ensize_K 15 (small) / 5 (large),
 * reduced_ndim ceiling(log2(n)/0.2^2), base_ncells 5000, partition_ncells 2000, hmethod ward.D,
 * minN 2, maxN max(40, ceiling(n/5000)), sil_thre 0.35, height_Ntimes 2.  *_cluster: 0 = NULL.
 * log_flag: the `flag` of R/SHARP.R:211-228 (1 = log2(x+1)).  projector: handle of a shared `rM` list
 * (sharp_projector_create) or 0 to draw it from rN_seed (seeds 50 + rN_seed + k); rN_seed = 0.5 is the
 * reference's "not reproducible" sentinel.  n < base_ncells runs SHARP_small, else SHARP_large
 * (with N_cluster given and n < base_ncells the reference's reroute at :181-191 applies).
 * Outputs: pred[n] (1..*n_pred, numbered by first appearance); viE (optional) n x p row-major;
 * x0 (optional) n x *x0_cols column-major with room for x0_cap_cols columns; *path 0 small / 1 large. */
int sharp_SHARP_dev(const float *dX, int m, long long n, long long ld, int ensize_K, int reduced_ndim, int base_ncells,
                    int partition_ncells, int hmethod, int N_cluster, int enpN_cluster, int indN_cluster, int minN, int maxN,
                    double sil_thre, double height_Ntimes, int log_flag, int projector, double rN_seed, int *pred,
                    int *n_pred, double *viE, double *x0, int x0_cap_cols, int *x0_cols, int *p_used, int *K_used, int *path);
/* a resident fp64 block (see sharp_project_dev64) */
int sharp_SHARP_dev64(const double *dX, int m, long long n, long long ld, int ensize_K, int reduced_ndim, int base_ncells,
                      int partition_ncells, int hmethod, int N_cluster, int enpN_cluster, int indN_cluster, int minN, int maxN,
                      double sil_thre, double height_Ntimes, int log_flag, int projector, double rN_seed, int *pred,
                      int *n_pred, double *viE, double *x0, int x0_cap_cols, int *x0_cols, int *p_used, int *K_used, int *path);
/* host matrix: X double, m x n column-major (ld >= m); kept in HBM as fp32 when that is exact, else as fp64 (sharp_x_storage) */
int sharp_SHARP(const double *X, int m, long long n, long long ld, int ensize_K, int reduced_ndim, int base_ncells,
                int partition_ncells, int hmethod, int N_cluster, int enpN_cluster, int indN_cluster, int minN, int maxN,
                double sil_thre, double height_Ntimes, int log_flag, int projector, double rN_seed, int *pred,
                int *n_pred, double *viE, double *x0, int x0_cap_cols, int *x0_cols, int *p_used, int *K_used, int *path);

/* How the most recent host-matrix entry point (sharp_SHARP, sharp_SHARP_csc, sharp_SHARP_unlimited*, sharp_project) stored its block
 * in HBM: 32 = fp32, chosen when every value survives the round trip through float (counts, UMI data: half the bytes of the one pass
 * over X); 64 = fp64 (TPM / CPM-like doubles), so that log2(X + 1) and the projection see the numbers the reference computes with
 * (R/SHARP.R:110-117,343-345).  0: nothing uploaded yet.  The environment variable SHARP_X_STORAGE = fp32 | fp64 forces the choice. */
int sharp_x_storage(void);
/* what a value of the most recently uploaded host block was on PCIe: 8 or 16 (counts: every value an integer in 0 .. 255 / 0 .. 65535, sent
 * as unsigned integers of that width and stored as fp32), 32 (other fp32-exact values), 64 (doubles).  A sparse block also sends 16-bit row
 * indices when it has at most 65 536 genes: 3 bytes per non-zero for typical count data against the 12 of R's dgCMatrix slots
 * (R/SHARP_unlimited.R:125-143 hands the blocks over as they are). */
int sharp_x_wire(void);

/* allrpinfo of the most recent call that took the SHARP_small path (R/SHARP.R:350-387,446: per random projection k its tag, the
 * rowColor of every cell, N.cluster and indE = the projected matrix): enrp n x K column-major colour indices (1..40, the index into the
 * reference's colorL), indE n x (K p) row-major with projection k in columns [k p, (k+1) p).  Any output may be NULL (sizes only).
 * Valid until the next sharp_SHARP* call; an error if the last call took the SHARP_large path (the reference returns no allrpinfo there). */
int sharp_last_rpinfo(int *n, int *K, int *p, int *enrp, double *indE);

/* Releases the resident copy of the last host matrix, the pinned staging buffers that sharp_SHARP / sharp_SHARP_csc keep
 * between calls and the projections of the last batched sharp_SHARP_unlimited window; the worker and helper slots that in-process
 * multi-GPU runs and batched windows have left behind also give back their clustering workspaces (the analogue of R's gc() after a
 * run; no reference counterpart). */
int sharp_trim(void);

/* Sparse input: the reference takes whatever `log2(scExp + 1)` and `%*%` accept (R/SHARP.R:343-345,579), which includes the
 * Matrix package's dgCMatrix -- the usual container of scRNA-seq counts.  colptr = @p (n + 1 ints), rowidx = @i (0-based),
 * val = @x; canonical CSC (no duplicated entries).  Only the non-zeros cross PCIe; the dense block (fp32 or fp64 like the dense
 * entry points choose, sharp_x_storage) is built on the device, so results are bit-identical to the dense entry points.
 * sharp_csc_to_dense_dev fills a caller-owned device block (m x n fp32, column stride ld >= m; values narrowed to fp32) for the
 * *_dev entry points. */
int sharp_csc_to_dense_dev(const int *colptr, const int *rowidx, const double *val, int m, long long n, float *dX, long long ld);
/* The same for a block that is ALREADY PACKED and ALREADY IN DEVICE MEMORY: d_colptr n + 1 int64, d_idx row indices of idx_bits (16 or 32),
 * d_val values of val_bits (8 / 16: unsigned integers, 32: float, 64: double) -- what a block file of the compact format holds
 * (sharp_amd/blocks.py; the directory-of-partitions input of R/SHARP_unlimited3.R:59-62,103-105), DMA'd as it is.  dX: m x n, column stride
 * ld, fp32 or (dx_is_f64) fp64; zeroed and filled on the library's stream. */
int sharp_csc_packed_expand_dev(const long long *d_colptr, const void *d_idx, int idx_bits, const void *d_val, int val_bits, int m,
                                long long n, void *dX, long long ld, int dx_is_f64);
int sharp_SHARP_csc(const int *colptr, const int *rowidx, const double *val, int m, long long n, int ensize_K, int reduced_ndim,
                    int base_ncells, int partition_ncells, int hmethod, int N_cluster, int enpN_cluster, int indN_cluster,
                    int minN, int maxN, double sil_thre, double height_Ntimes, int log_flag, int projector, double rN_seed,
                    int *pred, int *n_pred, double *viE, double *x0, int x0_cap_cols, int *x0_cols, int *p_used, int *K_used,
                    int *path);

/* ---- a11: SHARP_unlimited ---------------------------------------------------------- */
/* R/SHARP_unlimited.R:29-242.  Whole call on one GPU: blocks are device (or host) matrices sharing m
 * genes; p = ceiling(log2(sum ncb)/0.04); shared projectors; per-block SHARP(); cross-block sMetaC on
 * the per-(block, cluster) centroid means of viE; < 10-cell merge; ids by decreasing size. */
int sharp_SHARP_unlimited_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                              int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred,
                              int *p_used);
int sharp_SHARP_unlimited(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K,
                          int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used);
/* The same over several GPUs of this node, inside the calling process: the serial block loop of R/SHARP_unlimited.R:125-163
 * is dealt out, block b to devices[b mod ndevices]; one host thread per device (each with its own context, streams and workspaces) builds
 * the projectors -- a pure function of m, p and the seeds, :97-104 -- and clusters its blocks; p comes from the GLOBAL cell count (:65-66);
 * the per-(block, cluster) centroid tables (a few hundred rows x p doubles per block: all sMetaC uses of E1, R/sMetaC.R:58-63) meet in
 * host memory, the final sMetaC / small-cluster merge / size-ordered relabel (:163-183) run once, on devices[0], and every block's labels
 * are mapped through the result.  Labels identical to sharp_SHARP_unlimited on one GPU.  A device may be named more than once (several
 * slots on one GPU: the tests), and successive calls may name different lists (a worker's context is found by device, not by position).
 * rN_seed must be a seed (0.5, the unseeded sentinel, would give every device different projectors).  Each GPU has a second host thread
 * that uploads block b + ndevices while block b is clustered.  sharp_SHARP_unlimited / _view themselves take this path when the
 * environment names several devices (SHARP_DEVICES=0,1,2,...) and the call is seeded; an unseeded call stays on the caller's GPU.
 * sharp_trim() / sharp_shutdown() release what every worker context keeps between calls, on every GPU. */
int sharp_SHARP_unlimited_multi(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K,
                                int N_cluster, int minN, int maxN, double rN_seed, const int *devices, int ndevices,
                                int *pred, int *n_pred, int *p_used, double *viE /* ncells x p row-major, or NULL */);
/* A list of SPARSE blocks (R/SHARP_unlimited.R:125-135 hands each block to SHARP() as it is, and log2(scExp + 1) / %*% take a
 * Matrix::dgCMatrix, R/SHARP.R:343-345,579): colptr[b] = block b's @p (ncb[b] + 1 ints), rowidx[b] = @i (0-based), val[b] = @x.  Only
 * a block's non-zeros cross PCIe (8 bytes each for count data); csc_expand_kernel builds the dense block on its GPU, the very block the
 * dense entry builds, so labels and viE are those of sharp_SHARP_unlimited_multi on the same values.  Block b + W is uploaded (second
 * host thread per GPU, own stream and pinned staging, two resident copies in rotation) while block b is clustered.  devices = NULL /
 * ndevices = 0 (and sharp_SHARP_unlimited_csc): the caller's GPU, or the SHARP_DEVICES list. */
int sharp_SHARP_unlimited_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                              int nblocks, int m, int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred,
                              int *n_pred, int *p_used, double *viE /* or NULL */);
int sharp_SHARP_unlimited_csc_multi(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                                    int nblocks, int m, int ensize_K, int N_cluster, int minN, int maxN, double rN_seed,
                                    const int *devices, int ndevices, int *pred, int *n_pred, int *p_used, double *viE /* or NULL */);
/* Blocks ALREADY resident on the GPUs of the device list (the foreach loop of R/SHARP_unlimited.R:125-163 over data that never leaves
 * HBM): block b is an m x ncb[b] column-major matrix (column stride ldb[b]; fp32, or fp64 where is_f64[b] != 0: 16-byte aligned, even
 * stride) on devices[device_of_block[b]].  Every GPU's worker runs its blocks in list order, each block's RP stage and first distance
 * matrices prepared under the previous block's tail.  is_f64 = NULL: all fp32. */
int sharp_SHARP_unlimited_multi_dev(const void *const *dX_blocks, const int *is_f64, const long long *ncb, const long long *ldb,
                                    const int *device_of_block, int nblocks, int m, int ensize_K, int N_cluster, int minN, int maxN,
                                    double rN_seed, const int *devices, int ndevices, int *pred, int *n_pred, int *p_used,
                                    double *viE /* or NULL */);
/* What the most recent in-process multi-device call did when: one row per block -- worker, block, upload start, upload end, clustering
 * start, clustering end (seconds since the call began; the upload columns are 0 for a resident block).  rows: room for cap_rows x 6. */
int sharp_multi_timeline(double *rows, int cap_rows, int *nrows);
/* The same with the viewflag output (R/SHARP_unlimited.R:153,216-228): viE = the blocks' ensemble-mean projections E1,
 * ncells x p row-major in block order (NULL: not wanted).  The 50-dimension reduction the reference applies above 1e5
 * cells is one more sharp_project() call on this matrix (host side: sharp_amd/api.py). */
int sharp_SHARP_unlimited_view(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K,
                               int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred, int *p_used,
                               double *viE);
int sharp_SHARP_unlimited_view_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                                   int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred,
                                   int *p_used, double *viE);
/* viewflag above 1e5 cells (R/SHARP_unlimited.R:216-228): enresults$viE is not E1 but 1/sqrt(kdim) * E1 %*% ranM2(p, kdim, seed), kdim = 50.
 * Every block's product is taken on its GPU as soon as the block's viE exists and the caller's viE receives ncells x kdim doubles
 * (row-major) instead of ncells x p.  sharp_SHARP_unlimited_viewk_dev carries kdim as an argument.  For the other entries that take a viE
 * buffer sharp_unlimited_view_dim(kdim) arms it for the NEXT SHARP_unlimited call OF THE CALLING THREAD (one-shot and thread-local: a call
 * made by another thread never takes it; the call that takes it keeps kdim and its seed as state of its own, so overlapping calls of one
 * process do not see each other).  Arm it immediately before the call; kdim = 0 disarms.  ONE z0 per call: seed 50 + rN.seed + ensize.K + 1
 * (the expression of :222 reads an undefined `k`, an R error whenever rN.seed is given: taken as the next seed of the projector sequence),
 * or, for an unseeded call, one random integer seed drawn when the call begins and used for every block, helper thread and device (:219-225
 * draw z0 once and multiply all of E1 by it). */
int sharp_unlimited_view_dim(int kdim);
int sharp_SHARP_unlimited_viewk_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                                    int ensize_K, int N_cluster, int minN, int maxN, double rN_seed, int *pred, int *n_pred,
                                    int *p_used, int view_dim, double *viE /* ncells x (view_dim > 0 ? view_dim : p) row-major */);
/* The same split for one-block-per-GPU sharding: every rank runs its blocks through
 * sharp_unlimited_block_dev (block labels 1..*n_clusters by first appearance, the cluster means of viE,
 * n_clusters x p row-major into `means` with room for cap_rows rows, and the cluster sizes), the
 * (means, counts) tables are all-gathered in block order, and every rank calls sharp_unlimited_merge,
 * which returns the final 1-based id of each gathered (block, cluster) row. */
int sharp_unlimited_block_dev(const float *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                              double rN_seed, int *pred, int *n_clusters, double *means, int cap_rows, long long *counts);
int sharp_unlimited_block_dev64(const double *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                double rN_seed, int *pred, int *n_clusters, double *means, int cap_rows, long long *counts);
/* Several resident blocks of ONE rank in one call: what sharp_unlimited_block_dev returns for each of them (labels back to back in
 * `pred`, n_clusters[b] rows of `means` / `counts` per block, back to back; cap_rows: room for all of them), with the base clustering
 * of all blocks as one pipelined batch and the blocks' tails on helper threads (R/SHARP_unlimited.R:125-149: the loop over blocks a rank
 * owns; 17 instead of 25 ms per 50 000-cell block).  is_f64[b] != 0: block b holds doubles (NULL: all fp32). */
int sharp_unlimited_blocks_dev(const void *const *dX_blocks, const int *is_f64, const long long *ncb, const long long *ldb, int nblocks, int m,
                               int p, int projector, int ensize_K, double rN_seed, int *pred, int *n_clusters, double *means, int cap_rows,
                               long long *counts);
/* SHARP_unlimited2 (R/SHARP_unlimited2.R:29-292, with SHARP_fpart :297-544): log10 instead of log2, E1 rounded to one
 * decimal before the base clustering (maxN.cluster = 40 there), and a single sMetaC over the per-fold ensemble clusters of
 * all blocks.  flag: log-transform (the reference's testlog decision); viE: ncells x p row-major E1 or NULL.  0 / negative
 * parameters take the reference defaults (:39-69). */
int sharp_SHARP_unlimited2(const double *const *X_blocks, const long long *ncb, int nblocks, int m, int ensize_K,
                           int reduced_ndim, int partition_ncells, int hmethod, int N_cluster, int enpN, int indN, int minN,
                           int maxN, double sil_thre, double height_Ntimes, int flag, double rN_seed, int *pred, int *n_pred,
                           int *p_used, double *viE);
int sharp_SHARP_unlimited2_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                               int ensize_K, int reduced_ndim, int partition_ncells, int hmethod, int N_cluster, int enpN,
                               int indN, int minN, int maxN, double sil_thre, double height_Ntimes, int flag, double rN_seed,
                               int *pred, int *n_pred, int *p_used, double *viE);
/* The block step with the log flag of the per-block SHARP() call (SHARP_unlimited3 leaves it to testlog,
 * R/SHARP_unlimited3.R:122) and, optionally, the block's viE rows (nb x p row-major, host; NULL: not wanted). */
int sharp_unlimited_block_view_dev(const float *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                   double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                   long long *counts, double *viE);
/* The same with the view reduction as arguments (a caller that runs its blocks one call at a time, e.g. a rank of the sharded run): viE
 * receives nb x view_dim doubles (view_dim = 0: nb x p); view_seed: the integer seed of the RUN's z0 = ranM2(p, view_dim, view_seed),
 * the same for every block and rank (50 + rN.seed + ensize.K + 1, or one random integer per run when the run is unseeded). */
int sharp_unlimited_block_viewk_dev(const float *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                    double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                    long long *counts, int view_dim, double view_seed, double *viE);
/* ... and for a resident fp64 block (values fp32 cannot hold: 16-byte aligned, even leading dimension) */
int sharp_unlimited_block_viewk_dev64(const double *dX, int m, long long nb, long long ld, int p, int projector, int ensize_K,
                                      double rN_seed, int flag, int *pred, int *n_clusters, double *means, int cap_rows,
                                      long long *counts, int view_dim, double view_seed, double *viE);
int sharp_unlimited_merge(const double *means, const long long *counts, int nC, int p, long long ncells, int N_cluster,
                          int minN, int maxN, int *final_id, int *n_final);
/* One-shot hint for a caller that runs its blocks one call at a time (a rank of the sharded run with several blocks per GPU): the block
 * of the call AFTER the next one (same genes, projector, parameters), already resident in HBM.  The next sharp_unlimited_block_view_dev
 * call enqueues that block's projection and distance matrices on a side stream under its own host-bound tail (what
 * sharp_SHARP_unlimited_dev does between its blocks); the call after it finds them done.  NULL clears the hint.  Results do not change. */
int sharp_unlimited_next_block_dev(const float *dX_next, long long nb_next, long long ld_next);

/* ---- get_marker_genes (R/get_marker_genes.R:25-264), the per-gene pass :120-152 ---------------- */
/* X genes x cells column-major (host, leading dimension ld) or dX fp32 on the device; label[n] in 1..n_cluster
 * (y$pred_clusters after the match() of :96-99).  out: m x 5 row-major = auc, icluster, pvalue (before p.adjust),
 * sparsity, FC for every gene; genes with sparsity <= theta get (0, 0, 1, sparsity, 0) like :146-149.  ng: how many
 * of the clusters with the highest mean rank are tried (:118).  Filtering, Holm adjustment and ordering (:153-187)
 * are host work (sharp_amd/api.py). */
int sharp_marker_genes(const double *X, int m, long long n, long long ld, const int *label, int n_cluster, double theta, int ng,
                       double *out);
int sharp_marker_genes_dev(const float *dX, int m, long long n, long long ld, const int *label, int n_cluster, double theta, int ng,
                           double *out);
/* The same per-gene pass over the cells of a LIST of blocks, as get_marker_genes_unlimited runs it on the list SHARP_unlimited
 * clustered (R/get_marker_genes_unlimited.R:95-118: a gene's values across every block, one rank over all cells; ng = 1 there) and as
 * get_marker_genes_unlimited2 runs it (R/get_marker_genes_unlimited2.R:152-190, ng = min(10, N.cluster)).  label: the labels of all
 * cells in block order.  _dev: resident fp32 blocks (m x ncb[b], column stride ldb[b]); _csc: dgCMatrix blocks on the host
 * (colptr[b] = @p, rowidx[b] = @i, val[b] = @x) -- the stored entries go over as they are and are scattered straight into the
 * per-gene lists of non-zero cells, no dense block is built.  Values are compared as fp32, like sharp_marker_genes. */
int sharp_marker_genes_blocks_dev(const float *const *dX_blocks, const long long *ncb, const long long *ldb, int nblocks, int m,
                                  const int *label, int n_cluster, double theta, int ng, double *out);
int sharp_marker_genes_blocks_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                                  int nblocks, int m, const int *label, int n_cluster, double theta, int ng, double *out);

/* ---- Rtsne for visualization_SHARP (R/visualization_SHARP.R:94: Rtsne(x1, check_duplicates = FALSE, pca = flag, ...)) ---------
 * Exact t-SNE: PCA / normalisation of the input, exact k-NN (K = floor(3 perplexity), perplexity <= 85), per-row
 * perplexity calibration, P = (P_cond + P_cond^T) / sum, then max_iter steps of bhtsne's optimiser with the repulsion computed EXACTLY
 * (the theta -> 0 limit of Barnes-Hut; theta is accepted and unused): O(n^2) work per iteration.
 * X: n rows of d values, row i at X + i * ld (R's t(X), column-major).  Y (out) and Y_init (NULL: 1e-4 N(0, 1) from R's set.seed(seed)
 * stream): n x dims row-major, dims 1..3.  itercosts (NULL or one slot per iteration iter > 0 with iter % 50 == 0, plus the last
 * iteration): the KL divergence there; costs (NULL or n): the per-point KL at the end.  Bitwise reproducible on one GPU. */
int sharp_tsne(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale,
               int normalize, int check_duplicates, double perplexity, double theta, int max_iter, int stop_lying_iter, int mom_switch_iter,
               double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y,
               double *itercosts, double *costs);
/* Its stages one at a time (tests, tools).  _prepare: out (n x d) receives n x *d_out (the PCA / normalised input).  _knn: the K nearest
 * rows of every row (self excluded, ties by the lower index), sorted; dist = sum (x_i - x_j)^2; idx 0-based.  _affinities: P in CSR
 * (row_ptr n + 1, col / val with room for cap >= 2 n floor(3 perplexity) entries; *nnz out) for the already prepared X.  _gradient: dY
 * (n x dims) at Y for that P. */
int sharp_tsne_prepare(const double *X, long long n, int d, long long ld, int pca, int initial_dims, int pca_center, int pca_scale,
                       int normalize, double *out, int *d_out);
int sharp_tsne_knn(const double *X, long long n, int d, long long ld, int K, int *idx, double *dist);
int sharp_tsne_affinities(const double *X, long long n, int d, long long ld, double perplexity, long long cap, long long *row_ptr, int *col,
                          double *val, long long *nnz);
int sharp_tsne_gradient(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double *dY);
/* The host eigensolver behind _prepare's PCA, expression_pca's and diffmap's Rayleigh-Ritz step (Householder tridiagonalisation +
 * implicit QL), on its own (tests); needs no device.  A: d x d row-major, symmetric (the lower triangle is what is read).  w (d): the
 * eigenvalues ascending; V (d x d row-major): their eigenvectors as columns.  A matrix with a NaN is refused ("did not converge"). */
int sharp_symmetric_eigen(int d, const double *A, double *w, double *V);
/* sharp_tsne with bhtsne's Barnes-Hut repulsion (DESIGN.md §10 "Barnes-Hut"): theta is honoured.  0 < theta <= 1: a quadtree (octree
 * in 3-D) of Y rebuilt at every gradient evaluation, O(n log n) work per iteration; theta == 0: exactly sharp_tsne; theta outside
 * [0, 1] or not finite: "Incorrect theta." (SHARP_ERR_ARG).  Same arguments and outputs as sharp_tsne; bitwise reproducible on one GPU. */
int sharp_tsne_bh(const double *X, long long n, int d, long long ld, int dims, int initial_dims, int pca, int pca_center, int pca_scale,
                  int normalize, int check_duplicates, double perplexity, double theta, int max_iter, int stop_lying_iter, int mom_switch_iter,
                  double momentum, double final_momentum, double eta, double exaggeration, const double *Y_init, double seed, double *Y,
                  double *itercosts, double *costs);
/* The gradient stage with that repulsion: dY (n x dims) at Y for P; Z (NULL or one double) receives the normalisation Z it used. */
int sharp_tsne_gradient_bh(const long long *row_ptr, const int *col, const double *val, long long n, int dims, const double *Y, double theta,
                           double *dY, double *Z);
/* Rtsne's two other ways in (DESIGN.md §10 "Given neighbours, given distances").  Both skip PCA, normalisation and the duplicate check
 * and run sharp_tsne's calibration, symmetrisation and optimiser unchanged; repulsion: 0 exact (theta unused), 1 Barnes-Hut (theta
 * checked as sharp_tsne_bh checks it); Y_init, seed, Y, itercosts, costs as in sharp_tsne.
 * sharp_tsne_neighbors = Rtsne_neighbors(index, distance, ...): index / distance n x K row-major, index 0-based; 1 <= K <= 255,
 * K <= n - 1; squared = 0: Euclidean distances, squared on the device; 1: already squared (what sharp_tsne_knn returns).  perplexity
 * <= K (this library's rule: the entropy of K neighbours cannot pass log K) and n - 1 >= 3 perplexity ("Perplexity is too large.").
 * A kernel validates the lists before anything dereferences an index: every index in [0, n), none its own row, none twice in a row,
 * every distance finite and >= 0; the message names the first offending row.  A row's neighbours are used in the caller's order, so
 * sharp_tsne_knn's lists give sharp_tsne(pca = 0, normalize = 0)'s bits.
 * sharp_tsne_dist = Rtsne(d, is_distance = TRUE, ...): d = R's dist vector as sharp_dist returns it, every entry finite and >= 0,
 * 2 <= n <= SHARP_DIST_MAX_N (checked before d is read).  The K = floor(3 perplexity) nearest objects of each (perplexity <= 85) are
 * selected on the distances as given -- exact comparisons, ties to the lower index, self excluded --, P uses d^2. */
int sharp_tsne_neighbors(const int *index, const double *distance, long long n, int K, int squared, int repulsion, int dims, double perplexity,
                         double theta, int max_iter, int stop_lying_iter, int mom_switch_iter, double momentum, double final_momentum, double eta,
                         double exaggeration_factor, const double *Y_init, double seed, double *Y, double *itercosts, double *costs);
int sharp_tsne_dist(const double *d, int n, int repulsion, int dims, double perplexity, double theta, int max_iter, int stop_lying_iter,
                    int mom_switch_iter, double momentum, double final_momentum, double eta, double exaggeration_factor, const double *Y_init,
                    double seed, double *Y, double *itercosts, double *costs);
/* Their stages (tests, users who want P).  _knn_dist: idx (n x K, 0-based) and dist2 = d^2 of the K nearest objects, sorted by
 * (distance, index).  _affinities_nn: sharp_tsne_affinities from given lists (cap >= 2 n K always suffices). */
int sharp_tsne_knn_dist(const double *d, int n, int K, int *idx, double *dist2);
int sharp_tsne_affinities_nn(const int *index, const double *distance, long long n, int K, int squared, double perplexity, long long cap,
                             long long *row_ptr, int *col, double *val, long long *nnz);

/* ---- The approximate k-NN beside sharp_tsne_knn (DESIGN.md §16 is the specification: this project's own NN-descent; no parity with
 * pynndescent or uwot is claimed).  X: n rows of d values, row i at X + i * ld, every |x| <= 1e100 (NA / NaN / Inf refused by row and
 * column); 1 <= K <= 255, K <= n - 1, n < 2^31.  idx (n x K, 0-based) / dist2 (n x K): each row's list, self excluded, no index twice,
 * sorted by (distance, index) with ties to the lower index; dist2 = sum (x_i - x_j)^2 summed in column order, bitwise what sharp_tsne_knn
 * returns for the same pair.  The lists are a pure function of the arguments: bitwise reproducible.
 * sharp_knn_descent: the start (n_projections in 1 .. 32 sorted random projections; each row is offered the K rows on either side of it
 * in each order), then at most n_iters >= 0 joins with max_candidates (1 .. 255; 0: min(K, 30)) sampled reverse neighbours, stopping
 * when a join changes <= delta n K entries (0 <= delta <= 1).  seed: a whole number in [0, 2^53).  info (NULL or four values): joins
 * run, entries the last join changed, stop reason (0: n_iters reached, 1: the delta rule), candidate rows the joins gathered.  With K = n - 1 the lists are the exact ones.
 * Stages (tests, tools): _start: the start alone.  _join: join number `iteration` (>= 1) from the caller's lists `index` (n x K, 0-based,
 * validated as sharp_tsne_neighbors validates them, any order: they are measured and sorted first); *updates (NULL or one value): the
 * entries that changed.  max_rows_per_launch (0: the library's choice) only cuts the work into launches; no result depends on it. */
int sharp_knn_descent(const double *X, long long n, int d, long long ld, int K, int n_projections, int max_candidates, int n_iters,
                      double delta, double seed, int *idx, double *dist2, long long *info);
int sharp_knn_descent_start(const double *X, long long n, int d, long long ld, int K, int n_projections, double seed, int max_rows_per_launch,
                            int *idx, double *dist2);
int sharp_knn_descent_join(const double *X, long long n, int d, long long ld, int K, const int *index, int max_candidates, int iteration,
                           double seed, int max_rows_per_launch, int *idx, double *dist2, long long *updates);

/* ---- UMAP beside t-SNE (uwot::umap's arguments; DESIGN.md §13 is the specification: this project's, modelled on umap-learn's algorithm
 * and uwot's batch = TRUE mode, with no bit parity claimed).  Euclidean metric, set_op_mix_ratio = local_connectivity = bandwidth = 1.
 * sharp_umap_ab: a, b minimising sum (1 / (1 + a x^(2b)) - y(x))^2 over x = linspace(0, 3 spread, 300), y = 1 below min_dist, else
 * exp(-(x - min_dist) / spread); a host Levenberg-Marquardt in fp64, NO device needed.  spread > 0, 0 <= min_dist < 3 spread, finite.
 * sharp_umap: X n rows of d values (leading dimension ld, finite); n_neighbors in 2 .. 256 and <= n - 1 (it counts the point itself:
 * the lists hold K = n_neighbors - 1 others); dims 1 .. 3; n_epochs < 0: 500 if n <= 10000 else 200; ab: two doubles, in and out --
 * both positive: used as given, else fitted from (spread, min_dist) and written back; negative_sample_rate 0 .. 64; init: 0 the first
 * dims principal components of the prepared input, 1 runif(-10, 10) from R's set.seed(seed) stream (row by row), 2 Y_init (n x dims);
 * in every case each coordinate is then mapped affinely onto [0, 10].  pca: 0, or that many components through sharp_tsne_prepare's PCA
 * (centred when pca_center) before the k-NN.  Y: n x dims.  nn_index / nn_distance: both NULL, or n x (n_neighbors - 1) buffers that
 * receive the k-NN lists (0-based, Euclidean distances, sorted by (distance, index)).  Two calls with the same input and seed give
 * bitwise-identical Y on the same GPU.
 * sharp_umap_neighbors: the same from lists the caller has (index / distance n x K row-major, 0-based, n_neighbors = K + 1; squared =
 * 1: squared distances, as sharp_tsne_knn returns them), validated as sharp_tsne_neighbors validates them; init 1, 2 or 3 (below).
 * Stages: sharp_umap_graph: lists -> the fuzzy graph W = A + A^T - A o A^T as a CSR with rows sorted by column (cap >= 2 n K always
 * suffices), rho and sigma (n each).  sharp_umap_epochs: epochs [ep0, ep1) of n_epochs on Y (n x dims, in and out) for a CSR whose
 * mirrored entries carry equal weights; the schedule is stateless, so [0, e) then [e, n_epochs) gives the bits of [0, n_epochs). */
int sharp_umap_ab(double spread, double min_dist, double *a, double *b);
int sharp_umap(const double *X, long long n, int d, long long ld, int n_neighbors, int dims, int n_epochs, double learning_rate, double min_dist,
               double spread, double *ab, int negative_sample_rate, double repulsion_strength, int init, const double *Y_init, int pca,
               int pca_center, double seed, double *Y, int *nn_index, double *nn_distance);
int sharp_umap_neighbors(const int *index, const double *distance, long long n, int K, int squared, int dims, int n_epochs, double learning_rate,
                         double min_dist, double spread, double *ab, int negative_sample_rate, double repulsion_strength, int init,
                         const double *Y_init, double seed, double *Y);
int sharp_umap_graph(const int *index, const double *distance, long long n, int K, int squared, long long cap, long long *row_ptr, int *col,
                     double *val, long long *nnz, double *rho, double *sigma);
int sharp_umap_epochs(const long long *row_ptr, const int *col, const double *val, long long n, int dims, double *Y, int n_epochs, int ep0,
                      int ep1, double learning_rate, double a, double b, int negative_sample_rate, double repulsion_strength, double seed);

/* ---- UMAP's spectral start, init = 3 "normlaplacian" (DESIGN.md §15 is the specification: uwot's "normlaplacian" -- its "spectral"
 * without the noise -- with no bit parity claimed).  sharp_umap and sharp_umap_neighbors accept init = 3: after the graph stage the
 * bottom eigenvectors of the graph's normalised Laplacian are the start (through the same mapping onto [0, 10] as a given Y_init);
 * where the graph is not connected or the solve does not converge, sharp_umap falls back to init = 0 and sharp_umap_neighbors to
 * init = 1, each exactly as that code would have run.  sharp_umap_init_info tells which: the calling context's last sharp_umap /
 * sharp_umap_neighbors call asked for *requested and started from *used (0 .. 3; -1: no call yet); *components, *steps and *residual
 * (the largest true residual, or the last estimate on a fallback) are the spectral stage's, 0 where it did not run.
 * Stages.  sharp_umap_components: the connected components of a CSR pattern (row_ptr n + 1, col; an edge counts in both directions):
 * label[i] = the smallest vertex of i's component, *count = their number; an empty row is a component of its own.
 * sharp_umap_spectral: for a symmetric CSR W (weights >= 0, finite, every non-empty row's sum positive) the dims (1 .. 3, n >= dims +
 * 2) largest eigenvalues theta of M = D^-1/2 W D^-1/2 below the trivial 1 -- the smallest non-zero ones of L = I - M -- and their unit
 * eigenvectors V (n x dims row-major, each vector's largest |component| positive, ties to the lowest index), by Lanczos with full
 * reorthogonalisation on the complement of sqrt(deg).  tol <= 0 / max_steps <= 0: the defaults, 1e-6 and 400; max_steps is capped at
 * n - 2.  *outcome: 0 converged (every true residual ||M v - theta v|| <= tol, in residual), 1 not connected (nothing is solved; V,
 * theta, residual untouched), 2 not converged after *steps steps (residual: the last estimates; V, theta untouched).  Neither 1 nor 2 is
 * an error status.  Two calls give the same bits. */
int sharp_umap_components(const long long *row_ptr, const int *col, long long n, int *label, long long *count);
int sharp_umap_spectral(const long long *row_ptr, const int *col, const double *val, long long n, int dims, double tol, int max_steps, double *V,
                        double *theta, double *residual, int *steps, long long *components, int *outcome);
int sharp_umap_init_info(int *requested, int *used, long long *components, int *steps, double *residual);

/* ---- umap_transform: new rows placed in a fitted UMAP map (DESIGN.md §14 is the specification: this project's, modelled on umap-learn's
 * transform and uwot's umap_transform, with no bit parity claimed).
 * sharp_umap_model_create: a device-resident model of the calling context: X_ref n_ref rows of d values (leading dimension ld,
 * finite, squared norms that do not overflow), Y_ref n_ref x dims (dims 1 .. 3, finite) its fitted map, n_neighbors in 1 .. 255 and
 * <= n_ref (the K of a transform's lists), a, b > 0 the curve, n_epochs >= 0 the fit's epochs.  *handle receives the model;
 * sharp_umap_model_free releases it, sharp_shutdown releases what is left.  A handle is refused in any other context and once freed.
 * sharp_umap_transform: Xq nq rows of the model's d values (leading dimension ld) -> Yq nq x dims.  n_epochs < 0: a third of the
 * fit's (rounded down); 0 returns the start (the weighted mean of the neighbours' positions).  negative_sample_rate 0 .. 64.
 * row_offset >= 0 numbers the rows for the negative-sample draw: a long table transformed block by block with each block's first row
 * as row_offset gives the bits of one call.  nn_index / nn_distance: both NULL, or nq x n_neighbors buffers that receive the lists
 * (0-based into the reference, Euclidean, sorted by (distance, index)).  A row's result depends on that row, the model, the arguments
 * and row_offset + its number alone; two calls give bitwise-identical results on the same GPU.
 * Stages: sharp_knn_cross: the K nearest reference rows of every query row (any K in 1 .. 255, <= n_ref; max_rows_per_launch 0: the
 * library's choice, else the rows of one launch, rounded down to a multiple of 16, at least 16 -- the lists do not depend on it).
 * sharp_umap_transform_weights: lists -> sigma (nq), w (nq x K) and the start Y0 (nq x dims).  sharp_umap_transform_epochs: epochs
 * [ep0, ep1) of n_epochs on Yq (in and out); [0, e) then [e, n_epochs) gives the bits of [0, n_epochs). */
int sharp_umap_model_create(const double *X_ref, long long n_ref, int d, long long ld, const double *Y_ref, int dims, int n_neighbors, double a,
                            double b, int n_epochs, int *handle);
int sharp_umap_model_free(int handle);
int sharp_umap_transform(int handle, const double *Xq, long long nq, long long ld, int n_epochs, double learning_rate, int negative_sample_rate,
                         double repulsion_strength, double seed, long long row_offset, double *Yq, int *nn_index, double *nn_distance);
int sharp_knn_cross(int handle, const double *Xq, long long nq, long long ld, int K, int max_rows_per_launch, int *idx, double *dist);
int sharp_umap_transform_weights(int handle, const int *idx, const double *dist, long long nq, int K, double *sigma, double *w, double *Y0);
int sharp_umap_transform_epochs(int handle, const int *idx, const double *w, long long nq, int K, double *Yq, int n_epochs, int ep0, int ep1,
                                double learning_rate, int negative_sample_rate, double repulsion_strength, double seed, long long row_offset);

/* ---- dist / hclust as a tree: what pheatmap(cluster_rows = T, cluster_cols = T, clustering_method = "ward.D") computes inside
 * plot_markers (R/plot_markers.R:214-237), i.e. hclust(dist(sm), "ward.D") over the marker genes and hclust(dist(t(sm)), "ward.D") over up
 * to ~10 000 cells (:136-143).  DESIGN.md §11.
 * sharp_dist = stats::dist(x, method, p = minkowski_p): x n x p ROW-major observations (leading dimension ld); d_out the dist object,
 * n (n - 1) / 2 doubles in R's order (column-wise lower triangle = scipy's pdist order).  method (R's own codes): 1 euclidean, 2 maximum,
 * 3 manhattan, 6 minkowski -- computed from the differences x_ik - x_jk summed in fp64 in the order k = 0 .. p - 1, so duplicate rows are
 * at distance exactly 0 --, 7 "correlation" = as.dist(1 - cor(t(x))) (pheatmap's clustering_distance; the fp64-MFMA GEMM of
 * get_opt_hclust); 4 canberra and 5 binary are refused (SHARP_ERR_ARG), and so is NA / NaN / Inf in x.  2 <= n <= SHARP_DIST_MAX_N: the
 * full n x n matrix is built in device memory (17 GB at the limit) and the dist vector has at most 2^30 entries. */
#define SHARP_DIST_MAX_N 46340
int sharp_dist(const double *x, int n, int p, long long ld, int method, double minkowski_p, double *d_out);
/* stats::hclust(d, method): d a dist object as above, 2 <= n <= 16384; hmethod as in sharp_get_opt_hclust (1 ward.D .. 8 ward.D2; as in
 * R, centroid / median take the distances they are given and ward.D2 squares them and reports the root).  Outputs = R's hclust object:
 * merge (n - 1) x 2 COLUMN-major (observations negative, earlier steps positive; a singleton before a cluster, otherwise ascending:
 * hclust.f's HCASS2), height n - 1 in R's step order, order n (the dendrogram's leaves from left to right, 1-based). */
int sharp_hclust_dist(const double *d, int n, int hmethod, int *merge, double *height, int *order);
/* hclust(dist(x, dist_method, p = minkowski_p), hmethod) with the distance matrix kept in device memory (arguments of sharp_dist and
 * sharp_hclust_dist; 2 <= n <= 16384).  Bitwise the same tree as sharp_hclust_dist on sharp_dist's output. */
int sharp_hclust(const double *x, int n, int p, long long ld, int dist_method, double minkowski_p, int hmethod, int *merge, double *height,
                 int *order);

/* ---- cutree, silhouette, Calinski-Harabasz: what is done with a tree and with a labelling (validity.hip) ---------------------------
 * stats::cutree(tree, k) as the reference calls it on every tree it builds (R/get_opt_hclust.R:101,132,207): merge as sharp_hclust
 * writes it ((n - 1) x 2 column-major), k[0 .. nk) numbers of clusters, each between 1 and n; out: n x nk column-major, column q = the
 * labels of the partition after the first n - k[q] merges, 1-based and numbered by first appearance in observation order (R_cutree:
 * observation 1 is in cluster 1).  Host only: runs WITHOUT a device context, O(n) per k.  (cutree(tree, h = ) is k = n + 1 - the first
 * index where c(height, Inf) > h; sharp_amd.cutree and R's own cutree do that step.) */
int sharp_cutree(const int *merge, int n, const int *k, int nk, int *out);
/* cluster::silhouette(x, dist) (its C code sildist(); R/get_opt_hclust.R:103,134-137 take the median of column 3): cl = the cluster codes
 * 1 .. k of the n observations (every code occurs, 2 <= k <= n - 1), d = R's dist vector as sharp_dist returns it (3 <= n <=
 * SHARP_DIST_MAX_N).  neighbor[i] = the code of the nearest other cluster -- the first smallest mean distance in code order on an exact
 * tie --, width[i] = (b - a) / max(a, b) with a(i) over the n_c - 1 other members of the own cluster and b(i) the smallest mean over
 * another cluster; 0 when a == b and for an observation alone in its cluster.  Deterministic: the same input gives the same bits. */
int sharp_silhouette_dist(const double *d, int n, const int *cl, int k, int *neighbor, double *width);
/* The same from the observations (x: n rows of p features, leading dimension ld; dist_method / minkowski_p as in sharp_dist), MATRIX-FREE:
 * no n x n and no n x k array; device memory: n p doubles, 24 bytes per observation and 12 more per observation and workgroup part (at
 * most 32 parts).  Any 2 <= k <= n - 1, 3 <= n <= 16777216.  The four difference metrics give bitwise sharp_dist's distances (duplicates at exactly 0); the
 * correlation distance is 1 - the dot product of the centred unit rows.  Deterministic as above. */
int sharp_silhouette(const double *x, long long n, int p, long long ld, int dist_method, double minkowski_p, const int *cl, int k,
                     int *neighbor, double *width);
/* kind 0: clusterCrit::intCriteria(x, cl, "Calinski_Harabasz") = [B / (k - 1)] / [W / (n - k)] with squared Euclidean between / within
 * sums (R/get_opt_hclust.R:105); kind 1: clues::get_CH(x, cl, disMethod = "1-corr") (R/get_opt_hclust.R:144; d = 1 - Pearson
 * correlation in both sums).  O(n p), 3 <= n <= 16777216, 2 <= k <= n - 1; W == 0 gives +Inf as in R. */
int sharp_calinski_harabasz(const double *x, long long n, int p, long long ld, const int *cl, int k, int kind, double *out);

/* ---- Scores of a map: neighbour ranks (sharp_amd/csrc/neighbor_rank.hip) --------------------------------------
 * X: n rows of d values (row-major, ld >= d); index: n x K row-major, 0-based, each row K other rows (sharp_tsne_knn's list format),
 * validated as sharp_tsne_neighbors validates an index (range, no row naming itself, no index twice in a row).
 * rank_out[i * K + k] = 1 + the number of rows l != i with (d2(i, l), l) < (d2(i, j), j) lexicographically, j = index[i * K + k], where
 * d2 is the direct sum of (x_ic - x_lc)^2 in column order, bitwise the squared distance sharp_tsne_knn gives the pair: 1 .. n - 1, ties
 * to the lower index.  Matrix-free, O(n^2 d); everything the device computes is an integer, so two calls give the same bits whatever
 * the launch split.  3 <= n <= 16777216, d >= 1, 1 <= K <= 255, K <= n - 1, |x| <= 1e100 (NA / NaN / Inf and larger values are refused
 * by row and column).  max_rows_per_launch: 0 = by the library's pair budget (a test forces a split with a small value). */
int sharp_neighbor_ranks(const double *X, long long n, int d, long long ld, int K, const int *index, int max_rows_per_launch, int *rank_out);

/* ---- Louvain community detection on the neighbour graph (sharp_amd/csrc/louvain.hip) --------------------------
 * The project's own synchronous form of the method: a call is a pure function of its arguments, and two calls give the same bits.
 * The graph is a symmetric CSR: row_ptr (n + 1, from 0), col (0-based, strictly ascending within a row, no diagonal entry), val (finite,
 * >= 0, <= 1e100, val[i,j] == val[j,i], at least one positive) -- what sharp_umap_graph returns.  2 <= n <= 16777216, nnz < 2^38.
 * Weights become integers q = rint(val * 2^24 / max val) (entries with q = 0 are dropped) and every sum of weights is an int64 sum.
 * resolution in (0, 1e6]; tol >= 0 (a round is kept when the modularity rises by more than tol); max_levels 1 .. 64, max_rounds
 * 1 .. 100000 (rounds per level), max_fails 1 .. 64 (discarded rounds in a row that end a level); seed: a finite integer.
 * membership[n]: 1 .. G by decreasing size, ties to the community with the smallest member.  Per level l < *n_levels (level_cap >=
 * max_levels): level_n (vertices), level_communities, level_rounds, level_q (the modularity reached); the last level's are the
 * result's.  level_membership: NULL, or level_cap * n ints: the 0-based coarse vertex of every input vertex after each level. */
int sharp_louvain_graph(const long long *row_ptr, const int *col, const double *val, long long n, double resolution, double tol, int max_levels,
                        int max_rounds, int max_fails, double seed, int *membership, int level_cap, long long *level_n,
                        long long *level_communities, int *level_rounds, double *level_q, int *n_levels, int *level_membership);
/* the same from neighbour lists (index, distance: n x K as sharp_umap_neighbors takes them): sharp_umap_graph's fuzzy union is built on
 * the device and never leaves it */
int sharp_louvain_neighbors(const int *index, const double *distance, long long n, int K, int squared, double resolution, double tol,
                            int max_levels, int max_rounds, int max_fails, double seed, int *membership, int level_cap, long long *level_n,
                            long long *level_communities, int *level_rounds, double *level_q, int *n_levels, int *level_membership);
/* The stages one at a time (tests).  A level's graph is an integer-weighted CSR (q: int64 >= 0, self-loop entries allowed: a coarse
 * vertex's internal weight); comm / membership: ids in [0, n).
 * quantise: q (nnz, zeros kept in place), the strengths k (n) and 2m of a float-weighted graph.
 * move: the proposals of one round (level, round >= 0) from the state comm.
 * modularity: Q of a membership; give val (a float-weighted graph, quantised first: the public modularity) or q, the other NULL.
 * aggregate: the coarse CSR of comm (row_ptr_out: room for n + 1, col_out / q_out: room for nnz), its entries, the number of
 * communities, and new_out[c] = the coarse vertex of community c (-1: no member).
 * row_caps: the longest row of the wave class and of the workgroup class of the move kernel. */
int sharp_louvain_quantise(const long long *row_ptr, const int *col, const double *val, long long n, long long *q, long long *k, long long *m2);
int sharp_louvain_move(const long long *row_ptr, const int *col, const long long *q, long long n, const int *comm, double resolution, double seed,
                       int level, int round, int *proposal);
int sharp_louvain_modularity(const long long *row_ptr, const int *col, const double *val, const long long *q, long long n, const int *membership,
                             double resolution, double *Q);
int sharp_louvain_aggregate(const long long *row_ptr, const int *col, const long long *q, long long n, const int *comm, long long *row_ptr_out,
                            int *col_out, long long *q_out, long long *nnz_out, long long *nc_out, int *new_out);
int sharp_louvain_row_caps(int *wave_cap, int *block_cap);

/* ---- Leiden community detection on the neighbour graph (sharp_amd/csrc/leiden.hip) ----------------------------
 * Louvain's levels with a refinement between a level's move phase and its aggregation: the level's partition P is re-partitioned into
 * well-connected sub-communities, the coarse graph is built from those, and the next level starts from the connected parts of P.  The
 * returned communities are connected.  The project's own deterministic form: a pure function of its arguments, two calls give the
 * same bits; no parity with leidenalg, igraph or scanpy is claimed.  The three entries take the arguments of their sharp_louvain_*
 * counterparts plus max_refine_rounds (1 .. 100000; 200 in the front ends), refuse what those refuse, and fill the same outputs plus
 * modularity (Q of the returned membership on the input graph: sharp_louvain_modularity of it, bit for bit), level_sub_communities and
 * level_refine_rounds (level_cap values each).  level_communities and level_q describe a level's P; level_membership: NULL, or
 * level_cap * n ints, the 0-based rank of the community P of every input vertex at each level. */
int sharp_leiden_graph(const long long *row_ptr, const int *col, const double *val, long long n, double resolution, double tol, int max_levels,
                       int max_rounds, int max_fails, int max_refine_rounds, double seed, int *membership, double *modularity, int level_cap,
                       long long *level_n, long long *level_communities, long long *level_sub_communities, int *level_rounds,
                       int *level_refine_rounds, double *level_q, int *n_levels, int *level_membership);
int sharp_leiden_neighbors(const int *index, const double *distance, long long n, int K, int squared, double resolution, double tol, int max_levels,
                           int max_rounds, int max_fails, int max_refine_rounds, double seed, int *membership, double *modularity, int level_cap,
                           long long *level_n, long long *level_communities, long long *level_sub_communities, int *level_rounds,
                           int *level_refine_rounds, double *level_q, int *n_levels, int *level_membership);
int sharp_leiden_snn(const int *index, long long n, int K, double prune, double resolution, double tol, int max_levels, int max_rounds, int max_fails,
                     int max_refine_rounds, double seed, int *membership, double *modularity, int level_cap, long long *level_n,
                     long long *level_communities, long long *level_sub_communities, int *level_rounds, int *level_refine_rounds, double *level_q,
                     int *n_levels, int *level_membership);
/* The stages one at a time (tests), on an integer-weighted CSR (a level's graph, as sharp_louvain_move takes it).
 * level: rule L1, the move phase of a level from the membership comm0 (ids in [0, n)) -> the accepted membership, the rounds and its Q.
 * refine: one round of rule L2 from the state ref inside the partition P (ids in [0, n) both; round: r, counted from 0) -> the
 * proposals, the number of vertices that moved, and the number that hold a candidate with a positive gain whatever the round's bits.
 * split: out[v] = the smallest vertex of v's component in the graph restricted to the entries whose two ends carry the same label
 * (any ints; self-loops ignored); count = the number of such components. */
int sharp_leiden_level(const long long *row_ptr, const int *col, const long long *q, long long n, const int *comm0, double resolution, double tol,
                       int max_rounds, int max_fails, double seed, int level, int *comm, int *rounds, double *Q);
int sharp_leiden_refine(const long long *row_ptr, const int *col, const long long *q, long long n, const int *P, const int *ref, double resolution,
                        double seed, int level, int round, int *proposal, long long *moved, long long *wanting);
int sharp_leiden_split(const long long *row_ptr, const int *col, const long long *q, long long n, const int *label, int *out, long long *count);

/* ---- Diffusion maps and diffusion pseudotime on the neighbour graph (sharp_amd/csrc/diffmap.hip) ---------------
 * The project's own specification, modelled on scanpy's tl.diffmap / tl.dpt and Haghverdi et al. 2016; no parity with scanpy or destiny
 * is claimed.  W: a symmetric CSR (sharp_umap_spectral's input: weights >= 0, finite, every non-empty row's sum positive), q_i =
 * sum_j W_ij.  density_normalize != 0: K = Q^-1 W Q^-1, z_i = sum_j K_ij, T = Z^-1/2 K Z^-1/2; 0: K = W, z = q (T is then
 * sharp_umap_spectral's M).  T is applied as (T x)_i = a_i sum_j W_ij a_j x_j with a_i = 1 / (q_i sqrt(z_i)) (or 1 / sqrt(q_i)).
 * sharp_diffmap_graph: the solve runs on ONE connected component: root's when root >= 0, the largest when root = -1 (ties to the
 * smallest label, a label being the component's smallest vertex); a component with fewer than n_comps + 2 rows is refused.  evals
 * (n_comps): 1.0, then the n_comps - 1 largest eigenvalues of T below it, descending; evecs (n x n_comps row-major): sqrt(z) / ||sqrt(z)||,
 * then their unit eigenvectors (each vector's largest |component| positive, ties to the lowest index), NaN in the rows outside the
 * component; residual (n_comps): the true ||T v - theta v||; in_component (n): 1 / 0.  2 <= n_comps <= 64.  Thick-restart Lanczos with
 * full reorthogonalisation; tol <= 0: 1e-6; max_matvecs <= 0: 4000 operator applications.  *outcome: 0 every residual <= tol, 2 the cap
 * was reached (the last Ritz vectors and their true residuals are still returned; not an error status).  *steps: operator applications
 * of the recurrence; *restarts: rotations of the basis onto its top Ritz vectors.  Two calls give the same bits.
 * sharp_diffmap_neighbors: the same on the fuzzy graph of neighbour lists (sharp_umap_neighbors' input and graph: index n x K row-major,
 * 0-based, distance Euclidean, or squared with squared != 0); the graph is built on the device and never leaves it; the result is
 * sharp_diffmap_graph's on sharp_umap_graph's CSR, bit for bit.
 * Stages (tests).  sharp_diffmap_transitions: a and z (n each; 0 for an empty row).  sharp_diffmap_component: the chosen label, the
 * number of components, the component as a CSR of its own (sub_row_ptr: room for n + 1, sub_col / sub_val: room for row_ptr[n]; rows and
 * columns renumbered in ascending order of the old ids) and new_id (n; -1 outside); the same refusal by size.
 * sharp_dpt: out (n x n_roots row-major) = sqrt(sum_{l=1}^{n_dcs-1} (evals_l / (1 - evals_l) (evecs[root, l] - evecs[i, l]))^2), l
 * ascending; inf for a row of NaN; normalize != 0: each root's column divided by its largest finite value.  2 <= n_dcs <= n_comps;
 * roots 0-based, inside the solved component. */
int sharp_diffmap_graph(const long long *row_ptr, const int *col, const double *val, long long n, int n_comps, int density_normalize, long long root,
                        double tol, int max_matvecs, double *evals, double *evecs, double *residual, int *in_component, int *steps, int *restarts,
                        long long *components, long long *component_size, int *outcome);
int sharp_diffmap_neighbors(const int *index, const double *distance, long long n, int K, int squared, int n_comps, int density_normalize,
                            long long root, double tol, int max_matvecs, double *evals, double *evecs, double *residual, int *in_component,
                            int *steps, int *restarts, long long *components, long long *component_size, int *outcome);
int sharp_diffmap_transitions(const long long *row_ptr, const int *col, const double *val, long long n, int density_normalize, double *a, double *z);
int sharp_diffmap_component(const long long *row_ptr, const int *col, const double *val, long long n, int n_comps, long long root, int *label,
                            long long *components, long long *sub_n, long long *sub_nnz, long long *sub_row_ptr, int *sub_col, double *sub_val,
                            int *new_id);
int sharp_dpt(const double *evals, const double *evecs, long long n, int n_comps, int n_dcs, const int *roots, int n_roots, int normalize,
              double *out);

/* ---- The SNN / Jaccard neighbour graph (sharp_amd/csrc/snn.hip) ------------------------------------------------
 * index: n x K row-major, 0-based, each row K other rows, no index twice in a row (sharp_tsne_knn's and sharp_knn_descent's lists;
 * validated on the device before an index is dereferenced: range, self, twice).  2 <= n <= 16777216, 1 <= K <= 255, K <= n - 1.
 * k = K + 1 (Seurat's k.param: the row itself counts), S(i) = {i} + the row's neighbours, s(i, j) = |S(i) n S(j)| for i != j,
 * w(i, j) = (double)s / (double)(2k - s) (Seurat's ComputeSNN).  An entry exists iff s >= 1 and w >= prune (prune in [0, 1]; a weight
 * equal to prune stays).  The result is sharp_louvain_graph's input: row_ptr (n + 1), col strictly ascending within a row, no diagonal
 * entry, val[i,j] == val[j,i] bit for bit; a row may be empty.  Everything the device computes is an integer: two calls give the
 * same bits.  The formula is Seurat's; no run against Seurat is claimed.
 * col == NULL (then val and shared NULL too): the count alone -- row_ptr and *nnz are written and the caller allocates.  Otherwise
 * cap (the room of col / val / shared) must be >= nnz, or the call is refused with the needed count in the message and in *nnz.
 * shared: NULL, or the s of every entry.  nnz >= 2^38, or a result beyond the device's free memory, is refused by name.
 * row_caps: the largest row work t(i) = sum over m in S(i) of |{j : m in S(j)}| of the one-wave and of the one-workgroup class of the
 * product kernels (rows beyond the second use a dense counter row in device memory). */
int sharp_snn_graph(const int *index, long long n, int K, double prune, long long cap, long long *row_ptr, int *col, double *val, int *shared,
                    long long *nnz);
int sharp_snn_row_caps(int *wave_cap, int *block_cap);
/* lists -> the SNN graph -> Louvain (sharp_louvain_neighbors' arguments and outputs from resolution on): the graph never leaves the
 * device.  A pruned graph without any entry is refused ("holds no positive weight"). */
int sharp_louvain_snn(const int *index, long long n, int K, double prune, double resolution, double tol, int max_levels, int max_rounds,
                      int max_fails, double seed, int *membership, int level_cap, long long *level_n, long long *level_communities,
                      int *level_rounds, double *level_q, int *n_levels, int *level_membership);

/* ---- A truncated PCA of sparse expression blocks (sharp_amd/csrc/expr_pca.hip) --------------------------------
 * The blocks are sharp_SHARP_unlimited_csc's: colptr[b] (ncb[b] + 1 ints from 0), rowidx[b] (0-based genes, strictly ascending within
 * a cell), val[b] (finite; a stored zero counts as a zero); a block may hold no cell.  2 <= n <= 2^31 - 2 cells in all, 1 <= m <=
 * 16777216 genes, fewer than 2^38 stored entries.  A kernel validates range, order and values before an index is dereferenced; the
 * message names the first offending cell (counted from 0 over all blocks).
 * Transform: t = x; normalize_total = T > 0: t = x (T / L_c), L_c the cell's sum (a cell whose sum is 0 stays 0); log1p != 0:
 * t = log1p(.) after that; with either, a negative value is refused.  Gene statistics: mu = (sum t) / n, var = (sum over the stored
 * entries of (t - mu)^2 + (n - stored) mu^2) / (n - 1); a gene whose n values are all equal has mu = that value and var = 0 exactly.
 * w = 1, or with scale 1 / sqrt(var) (0 where var = 0).  A = (T^T - 1 mu^T) diag(w), n x m, is never formed.
 * sharp_expr_pca_csc: randomised subspace iteration with l = n_components + oversample columns (1 <= l <= 128, l <= min(n, m)),
 * Omega[g, j] = (mix(mix(seed * 0x9E3779B97F4A7C15 + g) + j) >> 11) 2^-53 - 0.5; Y = A Omega; n_iter times Q = orth(Y), Z = orth(A^T Q),
 * Y = A Z; then Q = orth(Y), Z = A^T Q, Z^T Z = W diag(lambda) W^T (host), s = sqrt(lambda) descending, loadings = Z W_k diag(1 / s) (m x k
 * row-major; each component's loading of largest magnitude positive, on ties the lowest gene decides), scores = A loadings (n x k
 * row-major: the cell-side product once more, so sharp_expr_pca_transform_csc on the fitted cells gives the same scores; the subspace's
 * Q W_k diag(s) = Q Q^T A loadings agrees with it as far as a component has converged), sdev = s / sqrt(n - 1), center = mu, scale_out = 1 / w (1 where w = 0), gene_var, *total_var = sum w^2 var.  orth is
 * CholeskyQR2; a pivot that is not finite, <= 0 or within l 2^-52 of the Gram's diagonal, or an eigenvalue <= 0, is refused:
 * "numerical rank below n_components + oversample".  Bitwise reproducible: no floating-point atomic, every sum in an order that
 * the input's shape fixes; one block and the same cells cut into several blocks give the same bits.  The data and the workspaces
 * beyond the device's free memory are refused by name before anything is allocated.
 * sharp_expr_stats_csc: mean, var (m each), nnz (m: the non-zero values of a gene) and cell_sum (n) after the transform.
 * sharp_expr_pca_transform_csc: scores (n x n_components) of new cells (n >= 0) from a fit's loadings, center and scale: a cell's row
 * depends on that cell and the fit alone.
 * Stage entries for the tests: sharp_expr_spmm_cells (Y (n x l) = A B, B m x l row-major), sharp_expr_spmm_genes (Z (m x l) = A^T Q,
 * Q n x l), sharp_expr_orth (Q = orth(Y), rows x l, rows >= l), sharp_expr_row_caps (the entries of a gene that one wave sums, the
 * rows of a slab of the Gram; needs no device). */
int sharp_expr_pca_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                       int n_components, int oversample, int n_iter, double normalize_total, int log1p, int scale, long long seed,
                       double *scores, double *loadings, double *singular_values, double *sdev, double *center, double *scale_out,
                       double *gene_var, double *total_var);
int sharp_expr_stats_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                         double normalize_total, int log1p, double *mean, double *var, long long *nnz, double *cell_sum);
int sharp_expr_pca_transform_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                                 int m, double normalize_total, int log1p, const double *loadings, const double *center, const double *scale,
                                 int n_components, double *scores);
int sharp_expr_spmm_cells(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                          double normalize_total, int log1p, int scale, const double *Bm, int l, double *Y);
int sharp_expr_spmm_genes(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                          double normalize_total, int log1p, int scale, const double *Q, int l, double *Z);
int sharp_expr_orth(const double *Y, long long rows, int l, double *Q);
int sharp_expr_row_caps(int *chunk, int *slab_rows);

/* ---- Variable-gene selection and gene subsets (sharp_amd/csrc/hvg.hip, expr_pca.hip) -----------------------------------
 * The *_sub_* entries are the three above with a gene subset: genes = n_genes strictly ascending indices within [0, m) (anything else
 * is refused by name); NULL and 0 mean all genes, which is what the entries above pass.  The whole blocks are uploaded and validated,
 * the cells' sums L_c are taken over all m genes and the transform runs; then the entries of the other genes are dropped and the kept
 * genes renumbered by their position in `genes`, and the fit is the one above on n_genes genes (Omega keyed by the new index; l <=
 * min(n, n_genes)): loadings, center, scale_out, gene_var (mean, var, nnz) have n_genes rows.  cell_sum stays the sum over all genes.
 * sharp_expr_pca_transform_sub_csc: the new cells have m genes, the fit's loadings / center / scale n_genes rows.
 * sharp_expr_hvg_csc: raw counts (a negative value is refused), n >= 2.  mu, var = the gene statistics above of the untransformed
 * values; over the N genes with var > 0 (1 <= N <= 2^20), x = log10 mu, y = log10 var, fit = a local quadratic (tricube weights,
 * bandwidth = the q-th smallest |x_j - x_i|, q = min(N, max(3, ceil(span N))), span in (0, 1], no robustness iterations; the
 * degree falls to 1 / 0 when the pivot p2 / p1 of the unpivoted LDL^T of the moment matrix is <= 2^-30 S0; bandwidth 0: the mean
 * of y over the points with x_j = x_i); sigma^2 = 10^fit, clip = mu + sigma sqrt(n), variances_norm = (sum over the stored
 * entries of (min(x, clip) - mu)^2 + (n - stored) mu^2) / ((n - 1) sigma^2), 0 for a constant gene.  The first min(n_top_genes, N)
 * genes by variances_norm descending (ties: the lower gene) are selected: rank (0-based, -1: not selected), highly_variable (0 / 1),
 * genes (the selected, ascending; room for min(n_top_genes, m)), *n_selected, *q, degree_counts (3: fits of degree 0, 1, 2).
 * variances_expected = sigma^2 (0 for a constant gene).  Bitwise reproducible like the entries above.
 * sharp_hvg_loess (stage entry for the tests): the fit at every one of the caller's points (1 <= npts <= 2^20, finite), with its
 * bandwidth and degree, in the caller's order. */
int sharp_expr_pca_sub_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                           int m, int n_components, int oversample, int n_iter, double normalize_total, int log1p, int scale, long long seed,
                           double *scores, double *loadings, double *singular_values, double *sdev, double *center, double *scale_out,
                           double *gene_var, double *total_var, const int *genes, int n_genes);
int sharp_expr_stats_sub_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                             int m, double normalize_total, int log1p, double *mean, double *var, long long *nnz, double *cell_sum,
                             const int *genes, int n_genes);
int sharp_expr_pca_transform_sub_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb,
                                     int nblocks, int m, double normalize_total, int log1p, const double *loadings, const double *center,
                                     const double *scale, int n_components, double *scores, const int *genes, int n_genes);
int sharp_expr_hvg_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                       int n_top_genes, double span, double *means, double *variances, double *variances_expected, double *variances_norm,
                       int *rank, int *highly_variable, int *genes, int *n_selected, int *q, int *degree_counts);
int sharp_hvg_loess(const double *x, const double *y, int npts, double span, double *fit, double *bandwidth, int *degree);

/* ---- batch integration of PCA scores (the specification is the project's own, modelled on Harmony) ---- */
/* sharp_harmony: Z n x d (rows of d values, finite, no zero row; 2 <= d <= 128), batch the dense codes 0 .. n_batches - 1 (2 <= n_batches
 * <= 4096, every code present), 2 <= n_clusters <= min(n, 256), sigma > 0, theta >= 0, lam > 0, 1 <= n_blocks <= 1024.  A soft k-means
 * on the unit rows with a penalty on batch-pure clusters (up to max_iter_cluster rounds over n_blocks hashed blocks of cells), then a
 * per-cluster ridge correction of the original Z, up to max_iter times.  Out: Z_corr (n x d, the caller's row order), Y (n_clusters x d),
 * objective and rounds (max_iter slots each, n_iter filled), n_iter, converged, and R (n x n_clusters, or NULL).  Every sum's order is
 * fixed by the input's shape: two calls give the same bits.
 * Stage entries for the tests, every array in the caller's order:
 * sharp_harmony_assign: for the cells [i0, i1), R[i, k] = exp(-(D_ik - min_k D_ik) / sigma) * P[batch[i], k] normalised over k, with
 *   D_ik = 2 (1 - Y_k . Zhat_i) and P (n_batches x n_clusters) or NULL for 1; argmax != 0: a[i] = the k of the largest Y_k . Zhat_i (ties to
 *   the lower k) instead.  The other rows of R / a are left as they are.
 * sharp_harmony_sums: O (n_blocks x n_batches x n_clusters) = the per-block column sums of R by batch, with block(i) = h(0, i) mod
 *   n_blocks of the seed; S (n_batches x n_clusters x d) = sum over the batch's cells of R[i, k] X[i, :].
 * sharp_harmony_correct: Z_corr[i, :] = Z[i, :] - sum_k R[i, k] W[batch[i], k, :], W n_batches x n_clusters x d.
 * sharp_harmony_ridge: W (n_batches x n_clusters x d) from N (n_batches x n_clusters, finite, >= 0) and S (n_batches x n_clusters x d):
 *   the host function that the whole call runs between its sums and its correction, W_k = 0 where s <= 0; needs no device.
 * sharp_harmony_caps: the cells of a slab of the sums and the doubles of Y that the assign kernel stages at a time; needs no device. */
int sharp_harmony(const double *Z, long long n, int d, const int *batch, int n_batches, int n_clusters, double sigma, double theta, double lam,
                  int max_iter, int max_iter_cluster, int n_blocks, double epsilon_cluster, double epsilon_harmony, int init_iter, long long seed,
                  double *Z_corr, double *Y, double *objective, int *rounds, int *n_iter, int *converged, double *R);
int sharp_harmony_assign(const double *Zhat, const double *Y, const int *batch, const double *P, long long n, int d, int K, int B, long long i0,
                         long long i1, double sigma, int argmax, double *R, int *a);
int sharp_harmony_sums(const double *R, const double *X, const int *batch, long long n, int d, int K, int B, long long seed, int n_blocks, double *O,
                       double *S);
int sharp_harmony_correct(const double *Z, const double *R, const int *batch, const double *W, long long n, int d, int K, int B, double *Z_corr);
int sharp_harmony_ridge(const double *N, const double *S, int B, int K, int d, double lam, double *W);
int sharp_harmony_caps(int *slab, int *lds_tile);

/* ---- doublet detection from sparse count blocks (sharp_amd/csrc/doublets.hip; the specification is the project's own,
 * modelled on Scrublet, with no parity with the scrublet or scanpy packages claimed) ----
 * The blocks are raw counts as sharp_expr_pca_csc takes them; a negative or non-finite value is refused before anything is allocated.
 * round(x) = floor(x + 0.5) throughout.
 * sharp_doublet_plan (no device): n_sim = round(ratio n); n_neighbors 0: the default min(round(0.5 sqrt(n)), the largest value whose
 *   k_adj fits); k_adj = round(n_neighbors (1 + n_sim / n)), the K of the k-NN, which must be <= 255 and <= n + n_sim - 1: an explicit
 *   n_neighbors beyond that is refused by name.
 * sharp_doublet_pairs (no device): parents[2 s + j] = floor((double)(h(s, j) >> 11) 2^-53 (double)n), h(s, j) = mix(mix(seed G + s) + j)
 *   with Omega's 64-bit mix; 0 <= seed < 2^53.  A doublet may have the same parent twice.
 * sharp_doublet_synth_csc: doublet s = column parents[2 s] + column parents[2 s + 1] over all m genes, made on the device slab after
 *   slab (max_doublets_per_slab 0: the library's memory budget alone cuts the slabs; no result depends on it) and brought back as
 *   colptr_out (n_sim + 1), rowidx_out / val_out (capacity entries: a smaller capacity than the doublets need is refused by name; the
 *   parents' entries added up always suffice), genes strictly ascending, a gene of both parents stored once; cell_sum_out (n_sim or
 *   NULL) = L_a + L_b.
 * sharp_doublet_project_csc: the doublets' scores (n_sim x n_components) in a fit of sharp_expr_pca_sub_csc (loadings, center, scale with
 *   a row per kept gene; genes / n_genes its subset, NULL and 0 for all genes): per slab the transform, the subset and the cell-side
 *   product of sharp_expr_pca_transform_sub_csc.  On integer counts the scores are bit for bit that entry's on the host-built blocks.
 * sharp_doublet_neighbor_counts: counts[i] = the entries of row i of index (rows x K, 0-based) that are >= n_obs.
 * sharp_doublet_score_table (no device): table[c] = q rho / r / (1 - rho - q (1 - rho - rho / r)), q = (c + 1) / (k_adj + 2), c = 0 ..
 *   k_adj, r = n_sim / n, rho the expected doublet rate.
 * sharp_doublet_threshold (no device): threshold_in NaN: the minimum between the two modes of the simulated scores' 256-bin histogram
 *   over [min, max], smoothed by three-bin means ((a + b) + c) / 3 with reflected ends until at most two local maxima remain (at most
 *   10000 times); *found = 0 and *threshold = NaN when two maxima never stand, and predicted / rates are then left alone.  Otherwise
 *   predicted[i] = scores_obs[i] > threshold, rates = {detected (share of observed above), detectable (share of simulated above),
 *   overall = detected / detectable}.  A given threshold is used as it is (*found stays 0).
 * sharp_scrublet_csc: the whole call.  fit_* all NULL: variable genes (n_top_genes, unless genes is given) and the sparse PCA of the
 *   observed cells (n_prin_comps components, oversample 10, 4 iterations, seed 0) are computed first; otherwise the caller's fit
 *   (fit_scores n x n_prin_comps, the rest as for sharp_doublet_project_csc) is used as it is.  nn_method 0: the exact k-NN, 1:
 *   NN-descent with nn_args = {n_projections, max_candidates, n_iters, delta, seed} (NULL: 8, 0, 12, 0.001, 10).  threshold NaN: find
 *   it.  Out: doublet_scores (n), doublet_scores_sim (n_sim), predicted (n; left alone without a threshold), threshold_out (NaN
 *   without one), threshold_found, rates (3), n_neighbors_out, k_adj_out, parents (2 n_sim), genes_out (room for min(n_top_genes, m) or
 *   n_genes values) and n_genes_out (0: all genes), neighbor_counts (n + n_sim), sim_pca (n_sim x n_prin_comps, or NULL). */
int sharp_doublet_plan(long long n, double sim_doublet_ratio, int n_neighbors, long long *n_sim, int *n_neighbors_out, int *k_adj);
int sharp_doublet_pairs(long long n, long long n_sim, long long seed, long long *parents);
int sharp_doublet_synth_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                            int m, const long long *parents, long long n_sim, int max_doublets_per_slab, long long capacity,
                            long long *colptr_out, int *rowidx_out, double *val_out, double *cell_sum_out);
int sharp_doublet_project_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks,
                              int m, const long long *parents, long long n_sim, double normalize_total, int log1p, const double *loadings,
                              const double *center, const double *scale, int n_components, const int *genes, int n_genes,
                              int max_doublets_per_slab, double *scores);
int sharp_doublet_neighbor_counts(const int *index, long long rows, int K, long long n_obs, int *counts);
int sharp_doublet_score_table(int k_adj, double r, double expected_doublet_rate, double *table);
int sharp_doublet_threshold(const double *scores_obs, long long n, const double *scores_sim, long long n_sim, double threshold_in,
                            double *threshold, int *found, int *predicted, double *rates, int *passes);
int sharp_scrublet_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                       double sim_doublet_ratio, double expected_doublet_rate, int n_neighbors, int n_prin_comps, int n_top_genes,
                       const int *genes, int n_genes, const double *fit_scores, const double *fit_loadings, const double *fit_center,
                       const double *fit_scale, double normalize_total, int log1p, int scale, double threshold, int nn_method,
                       const double *nn_args, long long seed, int max_doublets_per_slab, double *doublet_scores, double *doublet_scores_sim,
                       int *predicted, double *threshold_out, int *threshold_found, double *rates, int *n_neighbors_out, int *k_adj_out,
                       long long *parents, int *genes_out, int *n_genes_out, int *neighbor_counts, double *sim_pca);

/* ---- rank_genes_groups: per-cluster differential expression (sharp_amd/csrc/rank_genes.hip; the specification is the
 * project's own, no parity with scanpy or Seurat is claimed) ------------------------------------------------------------------------
 * The blocks, normalize_total, log1p and genes / n_genes as sharp_expr_pca_sub_csc takes them (the transform runs over all m genes, then
 * the subset is applied; mk = the kept genes).  labels: one dense code 0 .. n_groups - 1 per cell in the blocks' order, 2 <= n_groups <=
 * 1024, every code present, n <= 2 097 151 cells.  reference: -1 = each group against all other cells ("rest"), or a code: every other
 * group against that group alone, ranks taken among the cells of the two groups, the reference's own row NaN.  method: 0 = Wilcoxon
 * rank sum (normal approximation; tie_correct, continuity 0 / 1), 1 = Welch's t-test (every tested group and the reference side need 2
 * cells).  Stored and implicit zeros (and -0.0) are one tie group; values are ranked by the full 64-bit double.
 * Outputs, n_groups x mk row-major (a group's genes are contiguous): scores (z or t), pvals (two-sided), pvals_adj (Benjamini-Hochberg
 * per group over the mk genes), logfoldchanges, auc (U / (n_g n_ref)), means, means_ref, pct, pct_ref (shares of non-zero values);
 * group_sizes (n_groups); order (n_groups x n_order, 1 <= n_order <= mk): the genes of each group by score descending, ties to the lower
 * gene, NaN scores last.  Bitwise reproducible; one block and the same cells cut into several give the same bits.
 * sharp_rank_sums_csc (stage entry for the tests): the exact integers behind the Wilcoxon test.  rank2 (n_groups x mk) = 2 x the sum of
 * the group's average ranks within the comparison; ties = the sum of t^3 - t over the comparison's tie groups: mk values for "rest",
 * n_groups x mk for a reference; nnz_counts (n_groups x mk) = the group's cells with a non-zero value.  With a reference the reference's
 * rows of all three are left as the caller filled them. */
int sharp_rank_genes_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                         const int *labels, int n_groups, int method, int reference, double normalize_total, int log1p, const int *genes,
                         int n_genes, int tie_correct, int continuity, int n_order, long long *group_sizes, double *scores, double *pvals,
                         double *pvals_adj, double *logfoldchanges, double *auc, double *means, double *means_ref, double *pct,
                         double *pct_ref, long long *order);
int sharp_rank_sums_csc(const int *const *colptr, const int *const *rowidx, const double *const *val, const long long *ncb, int nblocks, int m,
                        const int *labels, int n_groups, int reference, double normalize_total, int log1p, const int *genes, int n_genes,
                        long long *rank2, long long *ties, long long *nnz_counts);

/* ---- synthetic inputs (bench / tests; not part of the reference) ------------ */
/* Counter-based generator, value = f(seed, gene, cell): bit-identical to
 * oracle_synth_value().  Fills dX (fp32, m x ncell column-major, leading dim ld). */
int sharp_synth_fill_dev(unsigned seed, int m, long long cell0, int ncell, int G, int nmark,
                         float *dX, long long ld);
int sharp_synth_labels(unsigned seed, long long cell0, int ncell, int G, int *labels);

/* Test entry for the fp64 MFMA GEMM kernels behind the correlation distance and the per-cluster sums (tests/test_linalg_gpu.py):
 * C (M x N row-major) = sum_k At[k][i] * Bt[k][j], At K x M and Bt K x N row-major host arrays.  epilogue: 0 plain, 1 = 1 - clamp(v)
 * with a zero diagonal (correlation distance), 2 = clamp(v) with a unit diagonal; symmetric: Bt is ignored (C = At^T At, upper
 * triangle computed and mirrored); fast: the 128 x 128-tile kernel on zero-padded copies, else the generic 64 x 64 kernel. */
int sharp_gemm_tn_f64(const double *At, const double *Bt, double *C, int M, int N, int K, int epilogue, int symmetric, int fast);

/* Test entries for a whole BATCH of the kernels above and of the row preparation in front of them (tests/test_linalg_gpu.py): one
 * descriptor array, one gemm_tn_f64_batched / row_prep_batched call, operands padded as the production callers pad them.  Every output
 * buffer is filled with the NaN of bit pattern 0x7ff8c0de5eed0001 (the sentinel) before the call and comes back whole, so
 * the caller sees what was written and what was not.
 *
 * sharp_gemm_tn_f64_batch: task t is C_t (M[t] x N[t]) = At_t^T Bt_t with At_t (K[t] x M[t]) and Bt_t (K[t] x N[t]) row-major, the
 * tasks' operands one after the other in At / Bt (symmetric: Bt is not read, N must equal M).  epilogue, symmetric, fast and nn_square
 * hold for every task.  fast: the operands' K rows are padded to a multiple of 16 and their leading dimensions to a multiple of 128,
 * with zeros.  ldc_t = N[t] rounded up to 128 with ldc_pad, else N[t].  C receives the tasks' M[t] x ldc_t buffers one after the other;
 * with want_nn (needs fast, symmetric and ldc_pad) nn receives their (ldc_t / 128) x ldc_t row minima (GemmTask::nn), else it may be
 * null.  polite: the call is made as for a block prepared under another block's tail (sliced launches, SHARP_GEMM_SLICE).
 *
 * sharp_row_prep_batch: task t prepares the n[t] x p[t] matrix (leading dimension lds[t]) that follows its predecessors' n x lds values
 * in src, in mode[t] (0 feature rows, 1 symmetric similarity, 2 symmetric distance; 1 and 2 need n == p), with nld = n rounded up to 128
 * and p_pad = p rounded up to 16.  all_feature_rows as row_prep_batched takes it (every task mode 0 with p <= 512).  Each of Cr, Ct, nrm
 * and D receives every task's buffer (n x p, p_pad x nld, n, nld x nld), one after the other in task order, whatever the task's mode. */
int sharp_gemm_tn_f64_batch(int count, const int *M, const int *N, const int *K, const double *At, const double *Bt, int epilogue,
                            int symmetric, int fast, int nn_square, int want_nn, int polite, int ldc_pad, double *C, double *nn);
int sharp_row_prep_batch(int count, const int *n, const int *p, const long long *lds, const int *mode, const double *src,
                         int all_feature_rows, double *Cr, double *Ct, double *nrm, double *D);

/* Test entry for a whole BATCH of get_opt_hclust tasks (tests/test_hclust_batch_gpu.py): ONE call of the batch driver that every base
 * clustering, wMetaC and sMetaC goes through, over `count` tasks given as parallel arrays.  Task t is the n[t] x p[t] row-major matrix
 * that follows its predecessors' n x p values in mats; kind[t] says what it is (0 feature rows, 1 symmetric similarity with p == n; no
 * guess is made); hmethod .. height_Ntimes as sharp_get_opt_hclust takes them, per task and without defaults.  Every matrix is uploaded
 * to a device buffer of its own.
 * Outputs, each concatenated in task order with nk_t = 1 where N_cluster[t] > 0, else max(1, min(maxN, n - 1) - minN + 1):
 * f (sum n), v (sum nk n, level-major per task; only with want_v, else it may be null), msil and CHind (sum nk), height (sum (n - 1)),
 * and per task optN, nk, branch, rc (0 or SHARP_WARN_RANGE) and sequential (1: the sequential agglomeration kernel did the task,
 * 0: the bulk-synchronous one).  Every output is filled with the sentinel before the call -- the NaN of the linalg batch entries for
 * doubles, INT_MIN for ints -- so what the batch did not write shows.  Where N_cluster[t] > 0, CHind keeps the NaN the batch leaves
 * (the Euclidean index is sharp_get_opt_hclust's own work) and optN is the largest label.
 * nested: every output array holds TWO sets, one after the other.  The second receives the same tasks run again as batches started
 * from the first batch's progress callback -- the tasks reported finished since the previous callback, while later chunks are in
 * flight -- which is how a fold's wMetaC runs inside SHARP_large.  The tasks of the last chunk are never reported that way: their
 * entries of the second set keep the sentinel, as does the whole set when the batch is one chunk.  Refused for count > 4 x CUs.
 *
 * sharp_hclust_batch_plan: what the calling context's last batch did (any caller's, not only the entry's), one row of 16 ints per
 * chunk in the order the chunks were set up: 0 i0, 1 i1 (tasks [i0, i1)), 2 slot (set of buffers), 3 pipe (one of several chunks in
 * flight), 4 split (the chunk asked for the round-per-launch agglomeration), 5 NS (ranges, each on its own stream), 6 ml (many-levels
 * statistics), 7 max_n, 8 max_kpad, 9 the sequential fallback was deferred to the statistics phase, 10 form of the bulk-synchronous
 * agglomeration (0 none: sequential kernel only, 1 round per launch, 2 one launch of 1024 threads, 3 one launch of 512 threads, 4 an
 * experiment of the lab build),
 * 11 gs (state in global memory: max_n > 4096), 12 nested (started from another batch's progress callback; i0, i1 count within that
 * batch), 13 max_nk, and for form 1 (else 0) 14 wpt (workgroups per task in the rebuild launches; SHARP_HC_WPT) and 15 finish_at (the
 * round from which one launch finishes the rest, -1 never; SHARP_HC_FINISH_AT).  rows receives at most cap_rows rows, *n_rows the number held.  Written on the host; no device work. */
int sharp_get_opt_hclust_batch(int count, const int *n, const int *p, const int *kind, const int *hmethod, const int *N_cluster,
                               const int *minN, const int *maxN, const double *sil_thre, const double *height_Ntimes, const double *mats,
                               int want_v, int nested, int *f, int *v, double *msil, double *CHind, double *height, int *optN, int *nk,
                               int *branch, int *rc, int *sequential);
int sharp_hclust_batch_plan(int *rows, int cap_rows, int *n_rows);

/* Test entries for the meta-clustering stage (sharp_amd/csrc/meta.hip; tests/test_meta_gpu.py).  Doubles are filled with the sentinel NaN
 * above and ints with INT_MIN over the WHOLE capacity the caller states, before anything else is done, so the caller sees what was
 * written, that nothing was written behind it, and after a refusal that nothing was written at all.  A buffer that is too small for
 * what the call produced is refused ("an output buffer is too small"), never written past.
 *
 * sharp_wMetaC_batch: `count` wMetaC tasks given as parallel arrays through ONE wmetac_batch call, with the soft matrix and the
 * intermediates -- how the folds of SHARP_large reach that driver.  Task t is the N[t] x C[t] column-major label matrix that follows its
 * predecessors' N x C values in labels; hmethod .. height_Ntimes as sharp_wMetaC takes them, per task and without defaults.  labels may
 * be null: the driver then refuses the tasks as it refuses an empty label matrix.
 * cap[8]: the capacities, in values, of rc, allC, ncl, finalC, w1, S, tf, x0 in that order.  Outputs, each concatenated in task order:
 * rc (0 or the warning bits of sharp_wMetaC), allC and ncl (count each), finalC and w1 (sum N), S (sum allC^2, row-major per task),
 * tf (sum allC) and x0 (sum N ncl, column-major per task).
 *
 * sharp_cluster_means: means (nC x p row-major, cap values) = the mean row of every cluster of the host matrix E (n rows of p values,
 * leading dimension ld >= p), through ONE cluster_means_dev call -- sMetaC's centroids, the tails of SHARP_large and
 * sharp_calinski_harabasz.  uid[n]: the cluster of every row, 0 .. nC - 1, every cluster with at least one row.
 *
 * sharp_ensemble_mean: viE (n x p row-major, cap values) = (sum over k of E[:, k p .. (k + 1) p)) / K for the host matrix E (n rows of
 * K p values, leading dimension ldE >= K p), through ONE ensemble_mean_dev call. */
int sharp_wMetaC_batch(int count, const int *N, const int *C, const int *hmethod, const int *enN_cluster, const int *minN, const int *maxN,
                       const double *sil_thre, const double *height_Ntimes, const int *labels, const long long *cap, int *rc, int *allC,
                       int *ncl, int *finalC, double *w1, double *S, int *tf, double *x0);
int sharp_cluster_means(const double *E, long long ld, int n, int p, const int *uid, int nC, double *means, long long cap);
int sharp_ensemble_mean(const double *E, long long ldE, int n, int p, int K, double *viE, long long cap);

/* ---- device memory helpers for non-torch hosts (R glue, tests) -------------- */
int sharp_dev_alloc(long long bytes, void **dptr);
int sharp_dev_free(void *dptr);
int sharp_dev_upload(void *dptr, const void *host, long long bytes);
int sharp_dev_download(void *host, const void *dptr, long long bytes);

/* ---- the same entry points in R's .C() calling convention (sharp_amd/csrc/dotc.hip) -------------------------------------------
 * What R's  .C("sharp_C_SHARP", as.double(scExp), nrow(scExp), as.double(ncol(scExp)), ..., status = integer(1))  binds: every
 * argument is a pointer into a vector R owns (double* for numeric, int* for integer / logical, char** for character), the return is
 * void and *status receives what the plain entry point returns.  Dimensions that can exceed 2^31 - 1 (numbers of cells) travel as
 * double.  R cannot pass NULL, so optional outputs are buffers of length >= 1 selected by bits of *want.  "Missing" arguments are 0
 * (negative for sil.thre) as above.  `flashmark` (R/get_opt_hclust.R:76-83): TRUE takes flashClust(d, "ward") = the ward.D criterion;
 * with any other hmethod the reference's test `hmethod == "ward.D" || "ward.D2"` is an R error, reproduced as SHARP_ERR_ARG.
 * r/sharp_hip.R holds the R side of every one of these. */
void sharp_C_init(int *device, int *status);
void sharp_C_shutdown(int *status);
void sharp_C_trim(int *status);
void sharp_C_reload_options(int *status);   /* sharp_reload_options(): after Sys.setenv() of a SHARP_* switch in a session that has already called sharp_C_init */
void sharp_C_device_count(int *count, int *status);
void sharp_C_last_error(char **msg, int *len);                     /* copies the message into the caller's string of *len bytes */
/* R/ranM.R:11-33, R/ranM2.R:11-35, R/RPmat.R:14-31 */
void sharp_C_projector_create(int *m, int *p, int *K, double *seeds, int *handle, int *status);
void sharp_C_projector_destroy(int *handle, int *status);
/* nnz: in = capacity of gene/col/sign (0: count only), out = non-zeros of projector *k; sign[i] = +1 / -1 */
void sharp_C_projector_triplets(int *handle, int *k, int *gene, int *col, int *sign, double *nnz, int *status);
/* R/RPmat.R:32: X m x n column-major, E n x (K p) row-major */
void sharp_C_project(int *proj, double *X, int *m, int *n, int *log_flag, double *E, int *status);
/* R/get_opt_hclust.R:33-244; mat n x p ROW-major; want: 1 v, 2 msil + CHind, 4 height */
void sharp_C_get_opt_hclust(double *mat, int *n, int *p, int *hmethod, int *N_cluster, int *minN, int *maxN, double *sil_thre,
                            double *height_Ntimes, int *flashmark, int *f, int *v, double *msil, double *CHind, double *maxsil,
                            double *height, int *optN, int *nk, int *branch, int *want, int *status);
/* R/getrowColor.R:17-121 */
void sharp_C_getrowColor(double *E, int *n, int *p, int *hmethod, int *indN_cluster, int *minN, int *maxN, double *sil_thre,
                         double *height_Ntimes, int *flashmark, int *rowColor, double *maxsil, int *status);
/* R/wMetaC.R:15-226; want: 1 x0 (room for N * (maxN + 2)) */
void sharp_C_wMetaC(int *nC, int *N, int *C, int *hmethod, int *enN_cluster, int *minN, int *maxN, double *sil_thre,
                    double *height_Ntimes, int *finalC, double *x0, int *ncl, int *want, int *status);
/* R/sMetaC.R:17-210; n as double; tf: room for n entries */
void sharp_C_sMetaC(int *labels, double *sE1, double *n, int *p, int *hmethod, int *finalN_cluster, int *minN, int *maxN,
                    double *sil_thre, double *height_Ntimes, int *finalColor, int *tf, int *nC, int *status);
/* R/SHARP.R:44-318 (and :339-454, :478-851); want: 1 viE, 2 x0; info[5] = n_pred, x0_cols, p_used, K_used, path */
void sharp_C_SHARP(double *X, int *m, double *n, int *ensize_K, int *reduced_ndim, int *base_ncells, int *partition_ncells, int *hmethod,
                   int *N_cluster, int *enpN_cluster, int *indN_cluster, int *minN, int *maxN, double *sil_thre, double *height_Ntimes,
                   int *flashmark, int *log_flag, int *projector, double *rN_seed, int *pred, double *viE, double *x0, int *x0_cap_cols,
                   int *info, int *want, int *status);
void sharp_C_SHARP_csc(int *colptr, int *rowidx, double *val, int *m, double *n, int *ensize_K, int *reduced_ndim, int *base_ncells,
                       int *partition_ncells, int *hmethod, int *N_cluster, int *enpN_cluster, int *indN_cluster, int *minN, int *maxN,
                       double *sil_thre, double *height_Ntimes, int *flashmark, int *log_flag, int *projector, double *rN_seed, int *pred,
                       double *viE, double *x0, int *x0_cap_cols, int *info, int *want, int *status);
/* allrpinfo (R/SHARP.R:350-387,446); dims[3] = n, K, p; want: 1 enrp, 2 indE */
void sharp_C_last_rpinfo(int *dims, int *enrp, double *indE, int *want, int *status);
/* R/SHARP_unlimited.R:29-242; Xcat: the blocks one after the other (each m x ncb[b] column-major), ncb as doubles; want: 1 viE;
 * info[2] = n_pred, p_used */
void sharp_C_SHARP_unlimited(double *Xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *N_cluster, int *minN, int *maxN,
                             double *rN_seed, int *pred, double *viE, int *info, int *want, int *status);
/* sharp_SHARP_unlimited_multi: devices = integer vector of GPU indices (block b on devices[b mod *ndevices]) */
void sharp_C_unlimited_view_dim(int *kdim, int *status);      /* sharp_unlimited_view_dim: the next sharp_C_SHARP_unlimited* call's viE is ncells x *kdim */
void sharp_C_decision_log(int *enable, int *status);          /* sharp_decision_log */
void sharp_C_last_decisions(double *rows, int *cap_rows, int *n_rows, int *status);   /* sharp_last_decisions */
void sharp_C_SHARP_unlimited_multi(double *Xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *N_cluster, int *minN, int *maxN,
                                   double *rN_seed, int *devices, int *ndevices, int *pred, double *viE, int *info, int *want, int *status);
/* sharp_SHARP_unlimited_csc_multi for a list of dgCMatrix blocks: pcat / icat / xcat = the blocks' @p / @i / @x one after the other;
 * *ndevices = 0: the caller's GPU (R/SHARP_unlimited.R:125-135, R/SHARP.R:343-345,579) */
void sharp_C_SHARP_unlimited_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *N_cluster,
                                 int *minN, int *maxN, double *rN_seed, int *devices, int *ndevices, int *pred, double *viE, int *info,
                                 int *want, int *status);
/* R/SHARP_unlimited2.R:29-292 */
void sharp_C_SHARP_unlimited2(double *Xcat, int *nblocks, double *ncb, int *m, int *ensize_K, int *reduced_ndim, int *partition_ncells,
                              int *hmethod, int *N_cluster, int *enpN, int *indN, int *minN, int *maxN, double *sil_thre,
                              double *height_Ntimes, int *flag, double *rN_seed, int *pred, double *viE, int *info, int *want, int *status);
/* R/SHARP_unlimited.R:163-183 on gathered centroid tables; counts, ncells as doubles */
void sharp_C_unlimited_merge(double *means, double *counts, int *nC, int *p, double *ncells, int *N_cluster, int *minN, int *maxN,
                             int *final_id, int *n_final, int *status);
/* R/get_marker_genes.R:120-152 */
void sharp_C_marker_genes(double *X, int *m, double *n, int *label, int *n_cluster, double *theta, int *ng, double *out, int *status);
/* R/visualization_SHARP.R:94 (Rtsne): sharp_tsne with X = as.double(t(x1)) (rows of d values), n as double; has_Y_init = 0: Y_init is
 * ignored (a buffer of length >= 1); itercosts / costs: buffers of the sizes sharp_tsne documents */
void sharp_C_tsne(double *X, double *n, int *d, int *dims, int *initial_dims, int *pca, int *pca_center, int *pca_scale, int *normalize,
                  int *check_duplicates, double *perplexity, double *theta, int *max_iter, int *stop_lying_iter, int *mom_switch_iter,
                  double *momentum, double *final_momentum, double *eta, double *exaggeration, int *has_Y_init, double *Y_init, double *seed,
                  double *Y, double *itercosts, double *costs, int *status);
/* sharp_tsne_neighbors / sharp_tsne_dist / sharp_tsne_knn in the same convention (index 0-based here too: r/sharp_hip.R subtracts 1) */
void sharp_C_tsne_neighbors(int *index, double *distance, double *n, int *K, int *squared, int *repulsion, int *dims, double *perplexity,
                            double *theta, int *max_iter, int *stop_lying_iter, int *mom_switch_iter, double *momentum,
                            double *final_momentum, double *eta, double *exaggeration, int *has_Y_init, double *Y_init, double *seed, double *Y,
                            double *itercosts, double *costs, int *status);
void sharp_C_tsne_dist(double *d, int *n, int *repulsion, int *dims, double *perplexity, double *theta, int *max_iter, int *stop_lying_iter,
                       int *mom_switch_iter, double *momentum, double *final_momentum, double *eta, double *exaggeration, int *has_Y_init,
                       double *Y_init, double *seed, double *Y, double *itercosts, double *costs, int *status);
void sharp_C_tsne_knn(double *X, double *n, int *d, int *K, int *idx, double *dist, int *status);
/* sharp_knn_descent in the same convention; info: a numeric(4) (joins run, entries the last join changed, stop reason, rows gathered) */
void sharp_C_knn_descent(double *X, double *n, int *d, int *K, int *n_projections, int *max_candidates, int *n_iters, double *delta,
                         double *seed, int *idx, double *dist2, double *info, int *status);
/* sharp_tsne_bh in the same convention: sharp_C_tsne's arguments, theta honoured */
void sharp_C_tsne_bh(double *X, double *n, int *d, int *dims, int *initial_dims, int *pca, int *pca_center, int *pca_scale, int *normalize,
                     int *check_duplicates, double *perplexity, double *theta, int *max_iter, int *stop_lying_iter, int *mom_switch_iter,
                     double *momentum, double *final_momentum, double *eta, double *exaggeration, int *has_Y_init, double *Y_init, double *seed,
                     double *Y, double *itercosts, double *costs, int *status);
/* sharp_umap / sharp_umap_neighbors / sharp_umap_ab in the same convention: X = as.double(t(X)), n as double, index 0-based; ab: a
 * numeric(2), c(0, 0) to have it fitted; Y_init is read with init = 2 only (else a buffer of length >= 1); want_nn = 0: nn_index / nn_distance
 * are buffers of length >= 1 that are left alone */
void sharp_C_umap(double *X, double *n, int *d, int *n_neighbors, int *dims, int *n_epochs, double *learning_rate, double *min_dist,
                  double *spread, double *ab, int *negative_sample_rate, double *repulsion_strength, int *init, double *Y_init, int *pca,
                  int *pca_center, double *seed, double *Y, int *want_nn, int *nn_index, double *nn_distance, int *status);
void sharp_C_umap_neighbors(int *index, double *distance, double *n, int *K, int *squared, int *dims, int *n_epochs, double *learning_rate,
                            double *min_dist, double *spread, double *ab, int *negative_sample_rate, double *repulsion_strength, int *init,
                            double *Y_init, double *seed, double *Y, int *status);
void sharp_C_umap_ab(double *spread, double *min_dist, double *a, double *b, int *status);
/* sharp_umap_model_create / _free / sharp_umap_transform in the same convention: X_ref / Xq = as.double(t(X)) (rows of d values), n_ref,
 * nq and row_offset as double; want_nn = 0: nn_index / nn_distance are buffers of length >= 1 that are left alone */
void sharp_C_umap_model_create(double *X_ref, double *n_ref, int *d, double *Y_ref, int *dims, int *n_neighbors, double *a, double *b,
                               int *n_epochs, int *handle, int *status);
void sharp_C_umap_model_free(int *handle, int *status);
void sharp_C_umap_transform(int *handle, double *Xq, double *nq, int *d, int *n_epochs, double *learning_rate, int *negative_sample_rate,
                            double *repulsion_strength, double *seed, double *row_offset, double *Yq, int *want_nn, int *nn_index,
                            double *nn_distance, int *status);
/* sharp_umap_components / sharp_umap_spectral / sharp_umap_init_info in the same convention: row_ptr (n + 1 values), n, count and
 * components as double; col 0-based */
void sharp_C_umap_components(double *row_ptr, int *col, double *n, int *label, double *count, int *status);
void sharp_C_umap_spectral(double *row_ptr, int *col, double *val, double *n, int *dims, double *tol, int *max_steps, double *V, double *theta,
                           double *residual, int *steps, double *components, int *outcome, int *status);
void sharp_C_umap_init_info(int *requested, int *used, double *components, int *steps, double *residual, int *status);
/* stats::dist / stats::hclust for pheatmap inside plot_markers (R/plot_markers.R:214-237): x = as.double(t(x)) (rows of p values) */
void sharp_C_dist(double *x, int *n, int *p, int *method, double *minkowski_p, double *d_out, int *status);
void sharp_C_hclust_dist(double *d, int *n, int *hmethod, int *merge, double *height, int *order, int *status);
void sharp_C_hclust(double *x, int *n, int *p, int *dist_method, double *minkowski_p, int *hmethod, int *merge, double *height, int *order,
                    int *status);
/* cluster::silhouette / Calinski-Harabasz (sharp_silhouette_dist, sharp_silhouette, sharp_calinski_harabasz): x = as.double(t(x)),
 * n as double, cl = as.integer(factor(labels)) */
void sharp_C_silhouette_dist(double *d, int *n, int *cl, int *k, int *neighbor, double *width, int *status);
void sharp_C_silhouette(double *x, double *n, int *p, int *dist_method, double *minkowski_p, int *cl, int *k, int *neighbor, double *width,
                        int *status);
void sharp_C_calinski_harabasz(double *x, double *n, int *p, int *cl, int *k, int *kind, double *out, int *status);
/* sharp_neighbor_ranks in the same convention: X = as.double(t(X)), n as double, index 0-based (r/sharp_hip.R subtracts 1) */
void sharp_C_neighbor_ranks(double *X, double *n, int *d, int *K, int *index, int *max_rows_per_launch, int *rank_out, int *status);
/* sharp_louvain_graph / sharp_louvain_neighbors / sharp_louvain_modularity in the same convention: row_ptr (n + 1 values) and n as
 * double, col and index 0-based; levels: a numeric matrix of level_cap rows x 4 (n, communities, rounds, modularity; row-major);
 * want_levels = 0: level_membership is a buffer of length >= 1 that is left alone */
void sharp_C_louvain_graph(double *row_ptr, int *col, double *val, double *n, double *resolution, double *tol, int *max_levels, int *max_rounds,
                           int *max_fails, double *seed, int *membership, int *level_cap, double *levels, int *n_levels, int *want_levels,
                           int *level_membership, int *status);
void sharp_C_louvain_neighbors(int *index, double *distance, double *n, int *K, int *squared, double *resolution, double *tol, int *max_levels,
                               int *max_rounds, int *max_fails, double *seed, int *membership, int *level_cap, double *levels, int *n_levels,
                               int *want_levels, int *level_membership, int *status);
void sharp_C_louvain_modularity(double *row_ptr, int *col, double *val, double *n, int *membership, double *resolution, double *Q, int *status);
/* sharp_leiden_graph / sharp_leiden_neighbors / sharp_leiden_snn in the same convention; levels: level_cap rows x 6 (n, communities,
 * sub-communities, rounds, refine rounds, modularity; row-major) */
void sharp_C_leiden_graph(double *row_ptr, int *col, double *val, double *n, double *resolution, double *tol, int *max_levels, int *max_rounds,
                          int *max_fails, int *max_refine_rounds, double *seed, int *membership, double *modularity, int *level_cap, double *levels,
                          int *n_levels, int *want_levels, int *level_membership, int *status);
void sharp_C_leiden_neighbors(int *index, double *distance, double *n, int *K, int *squared, double *resolution, double *tol, int *max_levels,
                              int *max_rounds, int *max_fails, int *max_refine_rounds, double *seed, int *membership, double *modularity,
                              int *level_cap, double *levels, int *n_levels, int *want_levels, int *level_membership, int *status);
void sharp_C_leiden_snn(int *index, double *n, int *K, double *prune, double *resolution, double *tol, int *max_levels, int *max_rounds,
                        int *max_fails, int *max_refine_rounds, double *seed, int *membership, double *modularity, int *level_cap, double *levels,
                        int *n_levels, int *want_levels, int *level_membership, int *status);
/* sharp_snn_graph / sharp_louvain_snn in the same convention: n, cap, nnz and row_ptr (n + 1 values) as double, index 0-based;
 * want: 1 = fill col / val (0: the count alone, col / val / shared are buffers of length >= 1 that are left alone), 2 = shared too */
void sharp_C_snn_graph(int *index, double *n, int *K, double *prune, double *cap, double *row_ptr, int *col, double *val, int *shared, int *want,
                       double *nnz, int *status);
void sharp_C_louvain_snn(int *index, double *n, int *K, double *prune, double *resolution, double *tol, int *max_levels, int *max_rounds,
                         int *max_fails, double *seed, int *membership, int *level_cap, double *levels, int *n_levels, int *want_levels,
                         int *level_membership, int *status);
/* sharp_expr_pca_csc / sharp_expr_stats_csc / sharp_expr_pca_transform_csc for a list of dgCMatrix blocks laid out as
 * sharp_C_SHARP_unlimited_csc takes them (pcat / icat / xcat = the blocks' @p / @i / @x one after the other, ncb as double); seed and
 * the genes' nnz as double */
void sharp_C_expr_pca_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *n_components, int *oversample,
                          int *n_iter, double *normalize_total, int *log1p, int *scale, double *seed, double *scores, double *loadings,
                          double *singular_values, double *sdev, double *center, double *scale_out, double *gene_var, double *total_var,
                          int *status);
void sharp_C_expr_stats_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total, int *log1p,
                            double *mean, double *var, double *nnz, double *cell_sum, int *status);
void sharp_C_expr_pca_transform_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total, int *log1p,
                                    double *loadings, double *center, double *scale, int *n_components, double *scores, int *status);
/* the *_sub_* entries and sharp_expr_hvg_csc in the same convention: genes 0-based, *n_genes = 0 for all genes (genes is then a buffer
 * of length >= 1 that is left alone) */
void sharp_C_expr_pca_sub_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *n_components, int *oversample,
                              int *n_iter, double *normalize_total, int *log1p, int *scale, double *seed, double *scores, double *loadings,
                              double *singular_values, double *sdev, double *center, double *scale_out, double *gene_var, double *total_var,
                              int *genes, int *n_genes, int *status);
void sharp_C_expr_stats_sub_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total, int *log1p,
                                double *mean, double *var, double *nnz, double *cell_sum, int *genes, int *n_genes, int *status);
void sharp_C_expr_pca_transform_sub_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *normalize_total,
                                        int *log1p, double *loadings, double *center, double *scale, int *n_components, double *scores,
                                        int *genes, int *n_genes, int *status);
void sharp_C_expr_hvg_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *n_top_genes, double *span, double *means,
                          double *variances, double *variances_expected, double *variances_norm, int *rank, int *highly_variable, int *genes,
                          int *n_selected, int *q, int *degree_counts, int *status);
/* sharp_harmony in the same convention: Z = as.double(t(Z)) (rows of d values), n and seed as double, batch 0-based; *want_R = 0: R is a
 * buffer of length >= 1 that is left alone */
void sharp_C_harmony(double *Z, double *n, int *d, int *batch, int *n_batches, int *n_clusters, double *sigma, double *theta, double *lam,
                     int *max_iter, int *max_iter_cluster, int *n_blocks, double *epsilon_cluster, double *epsilon_harmony, int *init_iter,
                     double *seed, double *Z_corr, double *Y, double *objective, int *rounds, int *n_iter, int *converged, int *want_R, double *R,
                     int *status);
/* sharp_scrublet_csc in the same convention, the blocks as sharp_C_expr_pca_sub_csc takes them: seed as double; *n_genes = 0: no gene list
 * (genes is a buffer that is left alone); *have_fit = 0: the fit_* are buffers that are left alone; *threshold NA / NaN: find it;
 * *have_nn_args = 0: the defaults; parents as int (n_sim x 2, rows of two, 0-based); *want_sim_pca = 0: sim_pca is left alone */
void sharp_C_scrublet_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, double *sim_doublet_ratio,
                          double *expected_doublet_rate, int *n_neighbors, int *n_prin_comps, int *n_top_genes, int *genes, int *n_genes,
                          int *have_fit, double *fit_scores, double *fit_loadings, double *fit_center, double *fit_scale,
                          double *normalize_total, int *log1p, int *scale, double *threshold, int *nn_method, int *have_nn_args,
                          double *nn_args, double *seed, int *max_doublets_per_slab, double *doublet_scores, double *doublet_scores_sim,
                          int *predicted, double *threshold_out, int *threshold_found, double *rates, int *n_neighbors_out, int *k_adj_out,
                          int *parents, int *genes_out, int *n_genes_out, int *neighbor_counts, int *want_sim_pca, double *sim_pca,
                          int *status);
/* sharp_diffmap_graph / sharp_diffmap_transitions / sharp_diffmap_component / sharp_dpt in the same convention: row_ptr (n + 1 values),
 * n, root, the counts and sub_row_ptr as double; col, roots and new_id 0-based */
void sharp_C_diffmap_graph(double *row_ptr, int *col, double *val, double *n, int *n_comps, int *density_normalize, double *root, double *tol,
                           int *max_matvecs, double *evals, double *evecs, double *residual, int *in_component, int *steps, int *restarts,
                           double *components, double *component_size, int *outcome, int *status);
void sharp_C_diffmap_neighbors(int *index, double *distance, double *n, int *K, int *squared, int *n_comps, int *density_normalize, double *root,
                               double *tol, int *max_matvecs, double *evals, double *evecs, double *residual, int *in_component, int *steps,
                               int *restarts, double *components, double *component_size, int *outcome, int *status);
void sharp_C_diffmap_transitions(double *row_ptr, int *col, double *val, double *n, int *density_normalize, double *a, double *z, int *status);
void sharp_C_diffmap_component(double *row_ptr, int *col, double *val, double *n, int *n_comps, double *root, int *label, double *components,
                               double *sub_n, double *sub_nnz, double *sub_row_ptr, int *sub_col, double *sub_val, int *new_id, int *status);
void sharp_C_dpt(double *evals, double *evecs, double *n, int *n_comps, int *n_dcs, int *roots, int *n_roots, int *normalize, double *out,
                 int *status);
/* sharp_rank_genes_csc in the same convention, the blocks as sharp_C_expr_pca_sub_csc takes them: labels 0-based codes, *reference = -1
 * for "rest", *n_genes = 0 for all genes; group_sizes as double, order as int (0-based genes) */
void sharp_C_rank_genes_csc(int *pcat, int *icat, double *xcat, int *nblocks, double *ncb, int *m, int *labels, int *n_groups, int *method,
                            int *reference, double *normalize_total, int *log1p, int *genes, int *n_genes, int *tie_correct, int *continuity,
                            int *n_order, double *group_sizes, double *scores, double *pvals, double *pvals_adj, double *logfoldchanges,
                            double *auc, double *means, double *means_ref, double *pct, double *pct_ref, int *order, int *status);

#ifdef __cplusplus
}
#endif
#endif /* SHARP_HIP_H */
