# sharp_hip.R -- R side of libsharp_hip.so for the reference package (shibiaowan/SHARP): drop-in bodies for the exported
# functions on the hot path (NAMESPACE:3-28).  Source this file after the package (or paste the bodies into R/*.R):
# the functions keep the reference's names, argument lists, defaults, messages and return lists, and hand the computation
# to the MI355X library in ONE native call each, so no foreach/%dopar% worker ever touches the GPU context.
#
# Two bindings of the same C ABI (include/sharp_hip.h):
#   .C()    -- sharp_C_* entry points: needs nothing but dyn.load("libsharp_hip.so") (no code compiled against R.h);
#              R copies every argument, so a 50 000 x 20 000 matrix costs one extra 8 GB copy.
#   .Call() -- r/sharp_glue.c (R CMD SHLIB sharp_glue.c -L. -lsharp_hip): no copies; used when sharp_glue is loaded.
# NOT run in the build image (no R there): the ctypes tests call the sharp_C_* symbols with exactly these argument lists
# (tests/test_dotc_gpu.py).

sharp_hip_load <- function(libdir = ".", device = 0L) {
    dyn.load(file.path(libdir, paste0("libsharp_hip", .Platform$dynlib.ext)))
    glue <- file.path(libdir, paste0("sharp_glue", .Platform$dynlib.ext))
    if (file.exists(glue)) dyn.load(glue)
    st <- .C("sharp_C_init", as.integer(device), status = integer(1))$status
    .sharp_check(st)
    invisible(TRUE)
}

.sharp_has_glue <- function() is.loaded("R_sharp_SHARP")

.sharp_hmethods <- c(ward.D = 1L, single = 2L, complete = 3L, average = 4L, mcquitty = 5L, median = 6L, centroid = 7L, ward.D2 = 8L)
.sharp_hmethod <- function(h) {
    if (missing(h) || is.null(h)) return(1L)
    if (!h %in% names(.sharp_hmethods)) stop("invalid clustering method '", h, "'")
    .sharp_hmethods[[h]]
}
# a numeric matrix in DOUBLE storage: an integer count matrix (common with prep = FALSE) is INTSXP, and the .Call glue takes REAL()
# of what it is handed -- the .C route coerces with as.double, so both bindings accept the same inputs
.sharp_dmat <- function(x) { x <- data.matrix(x); storage.mode(x) <- "double"; x }

.sharp_int <- function(x) if (missing(x) || is.null(x)) 0L else as.integer(x)

# status -> R condition: 0 ok; 16 / 32 warning bits (reference quirks 8 and 11, DESIGN.md 9); anything else stop()
.sharp_check <- function(status) {
    if (status == 0L) return(invisible(0L))
    if (bitwAnd(status, bitwNot(48L)) == 0L) {
        if (bitwAnd(status, 16L) != 0L) warning("SHARP: the model selection left the range of candidate cluster numbers (clamped)")
        if (bitwAnd(status, 32L) != 0L) warning("SHARP: wMetaC's single-cluster fallback met a cell with one vote value")
        return(invisible(status))
    }
    msg <- .C("sharp_C_last_error", msg = paste(rep(" ", 2048), collapse = ""), len = 2048L)$msg
    stop(sub(" +$", "", msg), call. = FALSE)
}

# the 40 colour names of R/getrowColor.R:52-58
.sharp_colorL <- c("red", "purple", "blue", "yellow", "green", "orange", "brown", "gray", "black", "coral", "beige", "cyan",
    "turquoise", "pink", "khaki", "magenta", "violet", "salmon", "goldenrod", "orchid", "seagreen", "slategray", "darkred",
    "darkblue", "darkcyan", "darkgreen", "darkgray", "darkkhaki", "darkorange", "darkmagenta", "darkviolet", "darkturquoise",
    "darksalmon", "darkgoldenrod", "darkorchid", "darkseagreen", "darkslategray", "deeppink", "lightcoral", "lightcyan")

# ---- ranM / ranM2 / RPmat (R/ranM.R:11-33, R/ranM2.R:11-35, R/RPmat.R:14-47) --------------------------------------------
.sharp_projector <- function(m, p, seeds) {
    r <- .C("sharp_C_projector_create", as.integer(m), as.integer(p), length(seeds), as.double(seeds), handle = integer(1),
            status = integer(1))
    .sharp_check(r$status)
    r$handle
}
.sharp_projector_matrix <- function(h, m, p, k = 0L) {
    nn <- .C("sharp_C_projector_triplets", h, as.integer(k), integer(1), integer(1), integer(1), nnz = 0, status = integer(1))
    .sharp_check(nn$status)
    r <- .C("sharp_C_projector_triplets", h, as.integer(k), gene = integer(nn$nnz), col = integer(nn$nnz), sign = integer(nn$nnz),
            nnz = as.double(nn$nnz), status = integer(1))
    .sharp_check(r$status)
    Matrix::sparseMatrix(i = r$gene + 1L, j = r$col + 1L, x = r$sign * sqrt(sqrt(m)), dims = c(m, p))
}
ranM2 <- function(m, p, seedn) {
    if (!is.numeric(seedn)) stop("The seed should be a numeric!")
    h <- .sharp_projector(m, p, seedn)
    on.exit(.C("sharp_C_projector_destroy", h, integer(1)))
    .sharp_projector_matrix(h, m, p)
}
ranM <- function(scdata, p, seedn) ranM2(nrow(scdata), p, seedn)
RPmat <- function(scdata, p, seedn) {
    m <- nrow(scdata); n <- ncol(scdata)
    h <- .sharp_projector(m, p, seedn)
    on.exit(.C("sharp_C_projector_destroy", h, integer(1)))
    r <- .C("sharp_C_project", h, as.double(data.matrix(scdata)), m, n, 0L, E = double(n * p), status = integer(1))
    .sharp_check(r$status)
    list(R = .sharp_projector_matrix(h, m, p), projmat = matrix(r$E, nrow = p, ncol = n))    # p x n, like 1/sqrt(p) * t(x) %*% scdata
}

# ---- get_opt_hclust (R/get_opt_hclust.R:33-244) --------------------------------------------------------------------------
get_opt_hclust <- function(mat, hmethod, N.cluster, minN.cluster, maxN.cluster, sil.thre, height.Ntimes, flashmark) {
    if (missing(hmethod) || is.null(hmethod)) hmethod <- "ward.D"
    if (missing(minN.cluster) || is.null(minN.cluster)) minN.cluster <- 2
    if (missing(maxN.cluster) || is.null(maxN.cluster)) maxN.cluster <- 40
    if (missing(sil.thre) || is.null(sil.thre)) sil.thre <- 0.35
    if (missing(height.Ntimes) || is.null(height.Ntimes)) height.Ntimes <- 2
    if (missing(flashmark) || is.null(flashmark)) flashmark <- FALSE
    if (missing(N.cluster)) N.cluster <- NULL
    if (is.numeric(N.cluster)) {
        if (N.cluster %% 1 != 0) stop("The given N.cluster is not an integer!")
        if (N.cluster < 2) stop("The given N.cluster is less than 2, which is not suitable for clustering!")
    } else if (!is.null(N.cluster)) stop("The given N.cluster is not a numeric!")
    n <- nrow(mat); p <- ncol(mat)
    nk <- if (is.numeric(N.cluster)) 1L else max(1L, min(maxN.cluster, n - 1) - minN.cluster + 1)
    r <- .C("sharp_C_get_opt_hclust", as.double(t(mat)), n, p, .sharp_hmethod(hmethod), .sharp_int(N.cluster), as.integer(minN.cluster),
            as.integer(maxN.cluster), as.double(sil.thre), as.double(height.Ntimes), as.integer(flashmark), f = integer(n),
            v = integer(n * nk), msil = double(nk), CHind = double(nk), maxsil = double(1), height = double(max(n - 1, 1)),
            optN = integer(1), nk = integer(1), branch = integer(1), 7L, status = integer(1))
    .sharp_check(r$status)
    list(f = r$f, v = matrix(r$v[seq_len(n * r$nk)], nrow = n), maxsil = r$maxsil, msil = r$msil[seq_len(r$nk)],
         CHind = r$CHind[seq_len(r$nk)], height = r$height[seq_len(n - 1)], optN.cluster = r$optN)
}

# ---- getrowColor (R/getrowColor.R:17-121) ---------------------------------------------------------------------------------
getrowColor <- function(Emat, hmethod, indN.cluster, minN.cluster, maxN.cluster, sil.thre, height.Ntimes, flashmark) {
    if (missing(height.Ntimes) || is.null(height.Ntimes) || height.Ntimes <= 0) height.Ntimes <- 1
    if (missing(flashmark)) flashmark <- FALSE
    if (missing(indN.cluster)) indN.cluster <- NULL
    n <- nrow(Emat); p <- ncol(Emat)
    r <- .C("sharp_C_getrowColor", as.double(t(Emat)), n, p, .sharp_hmethod(hmethod), .sharp_int(indN.cluster), as.integer(minN.cluster),
            as.integer(maxN.cluster), as.double(sil.thre), as.double(height.Ntimes), as.integer(flashmark), rowColor = integer(n),
            maxsil = double(1), status = integer(1))
    .sharp_check(r$status)
    list(rowColor = .sharp_colorL[r$rowColor], maxsil = r$maxsil, mat = Emat)
}

# ---- wMetaC (R/wMetaC.R:15-226) ----------------------------------------------------------------------------------------------
wMetaC <- function(nC, hmethod, enN.cluster, minN.cluster, maxN.cluster, sil.thre, height.Ntimes) {
    if (missing(sil.thre) || is.null(sil.thre)) sil.thre <- 0                 # :94-97
    if (missing(height.Ntimes) || is.null(height.Ntimes)) height.Ntimes <- 2
    if (missing(enN.cluster)) enN.cluster <- NULL
    if (missing(minN.cluster) || is.null(minN.cluster)) minN.cluster <- 2
    if (missing(maxN.cluster) || is.null(maxN.cluster)) maxN.cluster <- 40
    N <- nrow(nC); C <- ncol(nC)
    nCi <- apply(nC, 2, function(x) match(x, unique(x)))                       # labels only ever compare for equality inside a column
    r <- .C("sharp_C_wMetaC", as.integer(nCi), N, C, .sharp_hmethod(hmethod), .sharp_int(enN.cluster), as.integer(minN.cluster),
            as.integer(maxN.cluster), as.double(sil.thre), as.double(height.Ntimes), finalC = integer(N),
            x0 = double(N * (maxN.cluster + 2)), ncl = integer(1), 1L, status = integer(1))
    .sharp_check(r$status)
    list(finalC = as.character(r$finalC), x0 = matrix(r$x0[seq_len(N * r$ncl)], nrow = N))
}

# ---- sMetaC (R/sMetaC.R:17-210) ----------------------------------------------------------------------------------------------
sMetaC <- function(rerowColor, sE1, folds, hmethod, finalN.cluster, minN.cluster, maxN.cluster, sil.thre, height.Ntimes) {
    if (missing(finalN.cluster)) finalN.cluster <- NULL
    n <- length(rerowColor); p <- ncol(sE1)
    r <- .C("sharp_C_sMetaC", match(rerowColor, unique(rerowColor)), as.double(t(sE1)), as.double(n), p, .sharp_hmethod(hmethod),
            .sharp_int(finalN.cluster), as.integer(minN.cluster), as.integer(maxN.cluster), as.double(sil.thre), as.double(height.Ntimes),
            finalColor = integer(n), tf = integer(n), nC = integer(1), status = integer(1))
    .sharp_check(r$status)
    list(finalColor = as.character(r$finalColor), tf = r$tf[seq_len(r$nC)])
}

# ---- the body of SHARP() between its argument handling and its result list (replaces R/SHARP.R:251-280) ---------------------
# scExp: the prepared matrix (after :48-117); the arguments are those SHARP() holds at :251; returns what SHARP_small / SHARP_large
# return (pred_clusters, unique_pred_clusters, distr_pred_clusters, N.pred_cluster, x0, viE, allrpinfo for the small path).
.sharp_run <- function(scExp, ensize.K, reduced.ndim, base.ncells, partition.ncells, hmethod, N.cluster, enpN.cluster, indN.cluster,
                       minN.cluster, maxN.cluster, sil.thre, height.Ntimes, flashmark, flag, forview, rM, rN.seed) {
    m <- nrow(scExp); n <- ncol(scExp)
    p <- if (is.null(reduced.ndim) || reduced.ndim <= 0) ceiling(log2(n)/(0.2^2)) else reduced.ndim
    capc <- max(.sharp_int(maxN.cluster), 40L, ceiling(n/5000)) + 2L
    proj <- if (is.numeric(rM)) as.integer(rM) else 0L                       # rM: a projector handle from .sharp_projector()
    ipar <- c(.sharp_int(ensize.K), .sharp_int(reduced.ndim), .sharp_int(base.ncells), .sharp_int(partition.ncells),
              .sharp_hmethod(hmethod), .sharp_int(N.cluster), .sharp_int(enpN.cluster), .sharp_int(indN.cluster),
              .sharp_int(minN.cluster), .sharp_int(maxN.cluster), as.integer(flashmark), as.integer(flag), proj)
    dpar <- c(if (is.null(sil.thre)) -1 else sil.thre, if (is.null(height.Ntimes)) 0 else height.Ntimes, rN.seed)
    sparse <- methods::is(scExp, "dgCMatrix")
    if (.sharp_has_glue()) {
        r <- if (sparse) .Call("R_sharp_SHARP_csc", scExp@p, scExp@i, scExp@x, dim(scExp), ipar, dpar, as.logical(forview))
             else .Call("R_sharp_SHARP", .sharp_dmat(scExp), ipar, dpar, as.logical(forview))
    } else {
        want <- if (forview) 3L else 0L
        args <- list(ipar[1], ipar[2], ipar[3], ipar[4], ipar[5], ipar[6], ipar[7], ipar[8], ipar[9], ipar[10], dpar[1], dpar[2],
                     ipar[11], ipar[12], ipar[13], dpar[3], pred = integer(n), viE = double(if (forview) n * p else 1),
                     x0 = double(if (forview) n * capc else 1), as.integer(capc), info = integer(5), want, status = integer(1))
        r <- if (sparse) do.call(.C, c(list("sharp_C_SHARP_csc", scExp@p, scExp@i, as.double(scExp@x), m, as.double(n)), args))
             else do.call(.C, c(list("sharp_C_SHARP", as.double(data.matrix(scExp)), m, as.double(n)), args))
        .sharp_check(r$status)
        r <- list(pred = r$pred, viE = if (forview) t(matrix(r$viE[seq_len(n * r$info[3])], nrow = r$info[3])) else NULL,
                  x0 = if (forview) matrix(r$x0[seq_len(n * r$info[2])], nrow = n) else NULL, p = r$info[3], K = r$info[4], path = r$info[5])
    }
    y <- r$pred
    tn <- table(y)
    en <- list(pred_clusters = y, unique_pred_clusters = sort(unique(y)), distr_pred_clusters = tn[order(as.numeric(names(tn)))],
               N.pred_cluster = length(unique(y)))
    if (forview) {
        if (r$path == 0L) {                                                   # SHARP_small only (R/SHARP.R:446)
            d <- .C("sharp_C_last_rpinfo", dims = integer(3), integer(1), double(1), 0L, status = integer(1))$dims
            q <- .C("sharp_C_last_rpinfo", dims = integer(3), enrp = integer(d[1] * d[2]), indE = double(d[1] * d[2] * d[3]), 3L,
                    status = integer(1))
            .sharp_check(q$status)
            enrp <- matrix(q$enrp, nrow = d[1]); indE <- matrix(q$indE, nrow = d[2] * d[3])   # (K p) x n
            en$allrpinfo <- lapply(seq_len(d[2]), function(k) {
                rc <- .sharp_colorL[enrp[, k]]
                list(tag = paste("_RP", d[3], "_", k, sep = ""), rowColor = rc, N.cluster = length(unique(rc)),
                     indE = t(indE[(k - 1) * d[3] + seq_len(d[3]), , drop = FALSE]))
            })
        }
        en$x0 <- r$x0
        en$viE <- r$viE
    }
    en$.reduced.dim <- r$p; en$.ensize.K <- r$K
    en
}
# In R/SHARP.R the maintainer replaces :251-280 by
#     enresults = .sharp_run(scExp, ensize.K, reduced.ndim, base.ncells, partition.ncells, hmethod, N.cluster, enpN.cluster,
#                            indN.cluster, minN.cluster, maxN.cluster, sil.thre, height.Ntimes, flashmark, flag, forview, rM, rN.seed)
# (with the `missing()` arguments passed as NULL) and keeps :48-249 (checks, prep, CPM, defaults, testlog) and :282-317 (N.cells,
# N.genes, reduced.dim, ensize.K, time, paras).  SHARP_small / SHARP_large are the same call with base.ncells = ncells + 1 / 1.

# ---- SHARP_unlimited (R/SHARP_unlimited.R:29-242): replaces :96-183 -----------------------------------------------------------
# devices: integer vector of GPU indices (default: getOption("sharp.devices"), e.g. options(sharp.devices = 0:7)); the serial block loop
# of :125-163 is dealt out, block b to devices[b mod N], inside this R process (sharp_SHARP_unlimited_multi: per GPU one host thread that
# clusters and one that uploads the next block meanwhile; nothing crosses between GPUs but the per-block centroid tables).
# With the .Call glue loaded (r/sharp_glue.c) the list -- numeric matrices or Matrix::dgCMatrix blocks -- is read in place by
# R_sharp_unlimited_multi, whatever the number of devices.  The .C() fallback duplicates its arguments, needs the blocks unlist()-ed into
# ONE vector and does not take long vectors: it carries at most 2^31 - 1 values per call (a list of 1.3 M cells x 27 000 genes, 3.5e10
# values, cannot pass -- one cfg4 block, 4.39e9, already cannot), i.e. it is for small inputs and for installations without a compiler.
.sharp_block <- function(b) {                          # a block as the glue takes it: a double matrix, or the slots of a dgCMatrix
    if (inherits(b, "dgCMatrix")) list(p = b@p, i = b@i, x = b@x, dim = b@Dim)
    else if (inherits(b, "sparseMatrix")) { b <- methods::as(b, "CsparseMatrix"); list(p = b@p, i = b@i, x = as.double(b@x), dim = b@Dim) }
    else .sharp_dmat(b)
}
.sharp_unlimited_run <- function(scExp, ensize.K, N.cluster, minN.cluster, maxN.cluster, rN.seed, viewflag,
                                 devices = getOption("sharp.devices"), view.reduce = TRUE) {
    nb <- length(scExp); m <- nrow(scExp[[1]])
    ncb <- vapply(scExp, ncol, 1)
    ncells <- sum(ncb)
    p <- ceiling(log2(ncells)/(0.2^2))
    # R/SHARP_unlimited.R:216-228: above 1e5 cells enresults$viE is 1/sqrt(50) * E1 %*% ranM2(p, 50, seed), never E1.  With view.reduce the
    # library takes that product per block on the GPU (sharp_unlimited_view_dim) and r$viE comes back ncells x 50: the caller then sets
    # enresults$viE = r$viE instead of running lines 216-228 on a ncells x p matrix it no longer has.
    kdim <- if (isTRUE(view.reduce) && viewflag && ncells > 1e5) 50L else 0L
    vcols <- if (kdim > 0L) kdim else p
    arm <- function() if (kdim > 0L) .sharp_check(.C("sharp_C_unlimited_view_dim", kdim, status = integer(1))$status)
    ipar <- c(.sharp_int(ensize.K), .sharp_int(N.cluster), .sharp_int(minN.cluster), .sharp_int(maxN.cluster))
    sparse <- all(vapply(scExp, function(b) inherits(b, "sparseMatrix"), TRUE))
    if (.sharp_has_glue()) {
        blocks <- if (sparse) lapply(scExp, .sharp_block) else lapply(scExp, .sharp_dmat)
        r <- .Call("R_sharp_unlimited_multi", blocks, ipar, as.double(rN.seed), as.logical(viewflag), as.integer(devices), kdim)
    } else if (sparse) {
        cs <- lapply(scExp, .sharp_block)
        if (sum(as.numeric(vapply(cs, function(b) length(b$x), 1))) >= 2^31) stop("SHARP_unlimited: this input needs the .Call glue (r/sharp_glue.c): .C() carries at most 2^31 - 1 values")
        arm()
        r <- .C("sharp_C_SHARP_unlimited_csc", unlist(lapply(cs, `[[`, "p")), unlist(lapply(cs, `[[`, "i")), unlist(lapply(cs, `[[`, "x")), nb,
                as.double(ncb), m, ipar[1], ipar[2], ipar[3], ipar[4], as.double(rN.seed), as.integer(c(devices, 0L)), length(devices),
                pred = integer(ncells), viE = double(if (viewflag) ncells * vcols else 1), info = integer(2), as.integer(viewflag), status = integer(1))
        .sharp_check(r$status)
        r <- list(pred = r$pred, viE = if (viewflag) t(matrix(r$viE, nrow = vcols)) else NULL, p = r$info[2])
    } else {
        if (as.numeric(m) * ncells >= 2^31) stop("SHARP_unlimited: this input needs the .Call glue (r/sharp_glue.c): .C() carries at most 2^31 - 1 values")
        xcat <- unlist(lapply(scExp, function(b) as.double(data.matrix(b))))
        arm()
        if (length(devices) >= 2)
            r <- .C("sharp_C_SHARP_unlimited_multi", xcat, nb, as.double(ncb), m, ipar[1], ipar[2], ipar[3], ipar[4], as.double(rN.seed),
                    as.integer(devices), length(devices), pred = integer(ncells), viE = double(if (viewflag) ncells * vcols else 1),
                    info = integer(2), as.integer(viewflag), status = integer(1))
        else
            r <- .C("sharp_C_SHARP_unlimited", xcat, nb, as.double(ncb), m, ipar[1], ipar[2], ipar[3], ipar[4], as.double(rN.seed),
                    pred = integer(ncells), viE = double(if (viewflag) ncells * vcols else 1), info = integer(2), as.integer(viewflag),
                    status = integer(1))
        .sharp_check(r$status)
        r <- list(pred = r$pred, viE = if (viewflag) t(matrix(r$viE, nrow = vcols)) else NULL, p = r$info[2])
    }
    r$view.dim <- kdim                                                        # > 0: r$viE IS enresults$viE (ncells x 50); 0: r$viE is E1
    r                                                                         # finalrowColor = r$pred (ids by decreasing size)
}

# ---- the decision log (include/sharp_hip.h: sharp_decision_log / sharp_last_decisions; SURVEY.md 7, App. D.2) -------------------------
# sharp_decision_log(TRUE); res <- SHARP(...); d <- sharp_last_decisions(); sharp_decision_log(FALSE)
# One row per get_opt_hclust call of the run: which rule of R/get_opt_hclust.R:162-229 chose the number of clusters, how many levels tied
# exactly at the maximum (the reference takes the middle one), the maximum and the runner-up.  To attribute a label difference between this
# library and the reference to ONE decision, print the same quantities from the reference's own get_opt_hclust and compare row by row.
sharp_decision_log <- function(enable = TRUE) invisible(.sharp_check(.C("sharp_C_decision_log", as.integer(enable), status = integer(1))$status))
sharp_last_decisions <- function(cap = 65536L) {
    r <- .C("sharp_C_last_decisions", rows = double(14L * cap), as.integer(cap), n = integer(1), status = integer(1))
    .sharp_check(r$status)
    d <- as.data.frame(t(matrix(r$rows[seq_len(14L * min(r$n, cap))], nrow = 14L)))
    names(d) <- c("level", "block", "k", "fold", "n", "branch", "chosen.k", "ties", "best", "runner.up", "sil.minus.thre", "height.ratio",
                  "smetac.override.k", "levels")
    d$level <- c("direct", "base", "wMetaC", "sMetaC", "merge")[d$level + 2L]
    d$branch <- c("silhouette", "CH", "height", "N.cluster")[d$branch + 1L]
    d
}

# Rtsne(x1, ...) as R/visualization_SHARP.R:94 calls it: replace `Rtsne(` there by `sharp_Rtsne(`.  Rtsne's formals and return list;
# Y drawn from set.seed(seed)'s stream when Y_init is NULL.  repulsion = "exact": the exact repulsion on the GPU (theta accepted and
# unused, DESIGN.md 10); "barnes_hut": bhtsne's Barnes-Hut repulsion with theta honoured (sharp_C_tsne_bh).
# is_distance = TRUE: X is a `dist` object (sharp_dist's, stats::dist's) or a square symmetric matrix with finite entries >= 0; the
# floor(3 perplexity) nearest objects are selected on the distances as given and pca, initial_dims, normalize and check_duplicates
# are ignored (sharp_C_tsne_dist).
.sharp_ncost <- function(max_iter) { iters <- seq_len(max_iter) - 1L; sum((iters > 0 & iters %% 50 == 0) | iters == max_iter - 1L) }
.sharp_repulsion <- function(repulsion, who)
    switch(repulsion, exact = 0L, barnes_hut = 1L, stop(who, ": repulsion must be \"exact\" or \"barnes_hut\""))
.sharp_tsne_list <- function(n, Y, costs, itercosts, origD, perplexity, theta, max_iter, stop_lying_iter, mom_switch_iter, momentum,
                             final_momentum, eta, exaggeration_factor)
    list(N = n, Y = Y, costs = costs, itercosts = itercosts, origD = origD, perplexity = perplexity, theta = theta, max_iter = max_iter,
         stop_lying_iter = stop_lying_iter, mom_switch_iter = mom_switch_iter, momentum = momentum, final_momentum = final_momentum,
         eta = eta, exaggeration_factor = exaggeration_factor)
# R's dist vector and its size from a dist object or a square matrix (which must equal its transpose exactly; the diagonal is ignored)
.sharp_as_dist <- function(X) {
    if (inherits(X, "dist")) return(list(d = as.double(X), n = attr(X, "Size")))
    X <- .sharp_dmat(X)
    if (nrow(X) != ncol(X) || nrow(X) < 2) stop("Rtsne: with is_distance = TRUE, X must be a dist object or a square matrix")
    if (!identical(unname(X), unname(t(X)))) stop("Rtsne: the distance matrix is not symmetric (it must equal its transpose exactly)")
    list(d = X[lower.tri(X)], n = nrow(X))
}
sharp_Rtsne <- function(X, dims = 2, initial_dims = 50, perplexity = 30, theta = 0.5, check_duplicates = TRUE, pca = TRUE,
                        partial_pca = FALSE, max_iter = 1000, verbose = getOption("verbose", FALSE), is_distance = FALSE, Y_init = NULL,
                        pca_center = TRUE, pca_scale = FALSE, normalize = TRUE,
                        stop_lying_iter = ifelse(is.null(Y_init), 250L, 0L), mom_switch_iter = ifelse(is.null(Y_init), 250L, 0L),
                        momentum = 0.5, final_momentum = 0.8, eta = 200, exaggeration_factor = 12, num_threads = 1, seed = 10,
                        repulsion = "exact", ...) {
    rep_code <- .sharp_repulsion(repulsion, "sharp_Rtsne")
    has_init <- !is.null(Y_init)
    ncost <- .sharp_ncost(max_iter)
    if (is_distance) {
        dd <- .sharp_as_dist(X)
        n <- dd$n
        if (n > 46340) stop("Rtsne: more than 46340 objects (the dist vector would pass 2^30 entries) is not supported")
        if (anyNA(dd$d) || any(!is.finite(dd$d)) || any(dd$d < 0)) stop("Rtsne: the distances hold NA / NaN / Inf or a negative value")
        if (has_init && !all(dim(Y_init) == c(n, dims))) stop("Y_init must be an n x dims matrix")
        if (is.loaded("R_sharp_tsne_dist")) {
            r <- .Call("R_sharp_tsne_dist", dd$d, as.integer(n),
                       as.integer(c(0L, rep_code, dims, max_iter, stop_lying_iter, mom_switch_iter)),
                       as.double(c(perplexity, theta, momentum, final_momentum, eta, exaggeration_factor, seed)),
                       if (has_init) .sharp_dmat(Y_init) else double(0))
            Y <- r$Y; costs <- r$costs; ic <- r$itercosts
        } else {
            r <- .C("sharp_C_tsne_dist", dd$d, as.integer(n), rep_code, as.integer(dims), as.double(perplexity), as.double(theta),
                    as.integer(max_iter), as.integer(stop_lying_iter), as.integer(mom_switch_iter), as.double(momentum),
                    as.double(final_momentum), as.double(eta), as.double(exaggeration_factor), as.integer(has_init),
                    if (has_init) as.double(t(Y_init)) else double(1), as.double(seed),
                    Y = double(n * dims), itercosts = double(max(ncost, 1)), costs = double(n), status = integer(1))
            .sharp_check(r$status)
            Y <- matrix(r$Y, n, dims, byrow = TRUE); costs <- r$costs; ic <- r$itercosts[seq_len(ncost)]
        }
        return(.sharp_tsne_list(n, Y, costs, ic, NULL, perplexity, theta, max_iter, stop_lying_iter, mom_switch_iter, momentum,
                                final_momentum, eta, exaggeration_factor))
    }
    entry <- if (rep_code == 1L) "sharp_C_tsne_bh" else "sharp_C_tsne"
    X <- .sharp_dmat(X)
    n <- nrow(X); d <- ncol(X)
    if (has_init && !all(dim(Y_init) == c(n, dims))) stop("Y_init must be an n x dims matrix")
    r <- .C(entry, as.double(t(X)), as.double(n), as.integer(d), as.integer(dims), as.integer(initial_dims), as.integer(pca),
            as.integer(pca_center), as.integer(pca_scale), as.integer(normalize), as.integer(check_duplicates), as.double(perplexity),
            as.double(theta), as.integer(max_iter), as.integer(stop_lying_iter), as.integer(mom_switch_iter), as.double(momentum),
            as.double(final_momentum), as.double(eta), as.double(exaggeration_factor), as.integer(has_init),
            if (has_init) as.double(t(Y_init)) else double(1), as.double(seed),
            Y = double(n * dims), itercosts = double(max(ncost, 1)), costs = double(n), status = integer(1))
    .sharp_check(r$status)
    .sharp_tsne_list(n, matrix(r$Y, n, dims, byrow = TRUE), r$costs, r$itercosts[seq_len(ncost)], if (pca) min(initial_dims, d) else d,
                     perplexity, theta, max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration_factor)
}

# Rtsne_neighbors(index, distance, ...): index an n x K integer matrix of 1-BASED neighbour indices, distance their n x K Euclidean
# distances (squared = TRUE: already squared, as sharp_knn(X, K, squared = TRUE) returns them).  1 <= K <= 255, K <= n - 1,
# perplexity <= K.  The library validates the lists on the GPU and uses every row in the caller's order (sharp_C_tsne_neighbors).
sharp_Rtsne_neighbors <- function(index, distance, dims = 2, perplexity = 30, theta = 0.5, max_iter = 1000,
                                  verbose = getOption("verbose", FALSE), Y_init = NULL,
                                  stop_lying_iter = ifelse(is.null(Y_init), 250L, 0L), mom_switch_iter = ifelse(is.null(Y_init), 250L, 0L),
                                  momentum = 0.5, final_momentum = 0.8, eta = 200, exaggeration_factor = 12, num_threads = 1, seed = 10,
                                  repulsion = "exact", squared = FALSE, ...) {
    rep_code <- .sharp_repulsion(repulsion, "sharp_Rtsne_neighbors")
    distance <- .sharp_dmat(distance)
    index <- as.matrix(index)
    if (!all(dim(index) == dim(distance))) stop("Rtsne_neighbors: index and distance differ in shape")
    storage.mode(index) <- "integer"
    n <- nrow(distance); K <- ncol(distance)
    has_init <- !is.null(Y_init)
    if (has_init && !all(dim(Y_init) == c(n, dims))) stop("Y_init must be an n x dims matrix")
    ncost <- .sharp_ncost(max_iter)
    if (is.loaded("R_sharp_tsne_neighbors")) {
        r <- .Call("R_sharp_tsne_neighbors", index, distance,
                   as.integer(c(squared, rep_code, dims, max_iter, stop_lying_iter, mom_switch_iter)),
                   as.double(c(perplexity, theta, momentum, final_momentum, eta, exaggeration_factor, seed)),
                   if (has_init) .sharp_dmat(Y_init) else double(0))
        Y <- r$Y; costs <- r$costs; ic <- r$itercosts
    } else {
        i0 <- as.integer(t(index)) - 1L
        i0[is.na(i0)] <- -1L                                    # an NA index is out of range: the library names its row
        r <- .C("sharp_C_tsne_neighbors", i0, as.double(t(distance)), as.double(n), as.integer(K), as.integer(squared), rep_code,
                as.integer(dims), as.double(perplexity), as.double(theta), as.integer(max_iter), as.integer(stop_lying_iter),
                as.integer(mom_switch_iter), as.double(momentum), as.double(final_momentum), as.double(eta),
                as.double(exaggeration_factor), as.integer(has_init), if (has_init) as.double(t(Y_init)) else double(1),
                as.double(seed), Y = double(n * dims), itercosts = double(max(ncost, 1)), costs = double(n), status = integer(1), NAOK = TRUE)
        .sharp_check(r$status)
        Y <- matrix(r$Y, n, dims, byrow = TRUE); costs <- r$costs; ic <- r$itercosts[seq_len(ncost)]
    }
    .sharp_tsne_list(n, Y, costs, ic, NULL, perplexity, theta, max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta,
                     exaggeration_factor)
}

# the K nearest neighbours Rtsne itself computes: list(index = n x K, 1-based; distance = n x K Euclidean, or squared), each row
# sorted by (distance, index), ties to the lower index.  Computed once, they serve every later sharp_Rtsne_neighbors call on the data.
# method = "exact" (the default): the exact lists.  method = "descent" ("nndescent"): the approximate lists of NN-descent on the GPU
# (DESIGN.md 16; sharp_C_knn_descent) in the same layout -- every kept pair with the exact search's distance bits -- with
# attr(, "info") = list(joins, updates, reason); max_candidates NULL: min(K, 30); seed a whole number.
sharp_knn <- function(X, K, squared = FALSE, method = "exact", n_projections = 8L, max_candidates = NULL, n_iters = 12L, delta = 0.001,
                      seed = 10) {
    X <- .sharp_dmat(X)
    n <- nrow(X)
    if (!method %in% c("exact", "descent", "nndescent")) stop("sharp_knn: method must be \"exact\" or \"descent\" (\"nndescent\")")
    if (method == "exact") {
        r <- .C("sharp_C_tsne_knn", as.double(t(X)), as.double(n), ncol(X), as.integer(K), idx = integer(n * K), dist = double(n * K),
                status = integer(1))
    } else {
        r <- .C("sharp_C_knn_descent", as.double(t(X)), as.double(n), ncol(X), as.integer(K), as.integer(n_projections),
                as.integer(if (is.null(max_candidates)) 0L else max_candidates), as.integer(n_iters), as.double(delta), as.double(seed),
                idx = integer(n * K), dist = double(n * K), info = double(4), status = integer(1))
    }
    .sharp_check(r$status)
    d2 <- matrix(r$dist, n, K, byrow = TRUE)
    out <- list(index = matrix(r$idx, n, K, byrow = TRUE) + 1L, distance = if (squared) d2 else sqrt(d2))
    if (method != "exact")
        attr(out, "info") <- list(joins = r$info[1], updates = r$info[2], reason = c("n_iters", "delta")[r$info[3] + 1], gathered = r$info[4])
    out
}

# ---- uwot::umap beside Rtsne (DESIGN.md 13) -------------------------------------------------------------------------------------------------
# uwot's argument names and defaults; the algorithm is this project's specification (modelled on umap-learn's and on uwot's batch = TRUE
# mode; no bit parity with either).  Only metric = "euclidean" and set_op_mix_ratio = local_connectivity = bandwidth = 1 are built.
# n_threads, n_sgd_threads, verbose and batch are accepted and ignored.  Returns the n x n_components matrix, or with ret_nn = TRUE
# list(embedding =, nn = list(euclidean = list(idx = n x n_neighbors, dist =))) in uwot's layout (column 1 is the point itself).
.sharp_umap_refuse <- function(metric, set_op_mix_ratio, local_connectivity, bandwidth) {
    if (!identical(metric, "euclidean")) stop("umap: metric '", metric, "' is not supported (only \"euclidean\")")
    if (set_op_mix_ratio != 1) stop("umap: set_op_mix_ratio other than 1 is not supported")
    if (local_connectivity != 1) stop("umap: local_connectivity other than 1 is not supported")
    if (bandwidth != 1) stop("umap: bandwidth other than 1 is not supported")
}
.sharp_umap_init <- function(init, n, dims, allow_pca) {
    if (is.character(init)) {
        code <- match(init, c("pca", "random", NA, "normlaplacian")) - 1L    # ("normlaplacian" is code 3; 2 is a matrix)
        if (is.na(init) || is.na(code)) stop("umap: init must be one of \"pca\", \"random\", \"normlaplacian\" or an n x n_components matrix")
        if (code == 0L && !allow_pca) stop("umap_neighbors: init = \"pca\" needs the data; give \"random\", \"normlaplacian\" or a matrix")
        if (code == 3L && n < dims + 2L) stop("umap: init = \"normlaplacian\" needs at least n_components + 2 rows")
        return(list(code = code, Y = double(1)))
    }
    init <- .sharp_dmat(init)
    if (!all(dim(init) == c(n, dims))) stop("umap: init must be \"pca\", \"random\" or an n x n_components matrix")
    list(code = 2L, Y = as.double(t(init)))
}
# What the last sharp_umap / sharp_umap_neighbors call of this session started from (DESIGN.md 15): list(requested =, used =, components =,
# steps =, residual =).  init = "normlaplacian" is the spectral start (uwot's "normlaplacian"); where the graph is in pieces or the
# eigensolver does not converge the call falls back ("pca" with the data, "random" with lists alone) and warns.
.sharp_umap_init_info <- function(who) {
    r <- .C("sharp_C_umap_init_info", requested = integer(1), used = integer(1), components = double(1), steps = integer(1),
            residual = double(1), status = integer(1))
    .sharp_check(r$status)
    nm <- c("pca", "random", "matrix", "normlaplacian")
    info <- list(requested = nm[r$requested + 1L], used = nm[r$used + 1L], components = r$components, steps = r$steps, residual = r$residual)
    if (r$used != r$requested)
        warning(who, ": init = \"", info$requested, "\" fell back to \"", info$used, "\": ",
                if (r$components != 1) paste0("the graph has ", r$components, " connected components")
                else paste0("the eigensolver did not converge in ", r$steps, " steps (residual estimate ", signif(r$residual, 3), ")"))
    info
}
sharp_umap_ab <- function(spread = 1, min_dist = 0.01) {
    r <- .C("sharp_C_umap_ab", as.double(spread), as.double(min_dist), a = double(1), b = double(1), status = integer(1))
    .sharp_check(r$status)
    c(a = r$a, b = r$b)
}
sharp_umap <- function(X, n_neighbors = 15, n_components = 2, metric = "euclidean", n_epochs = NULL, learning_rate = 1, init = "pca",
                       spread = 1, min_dist = 0.01, set_op_mix_ratio = 1, local_connectivity = 1, bandwidth = 1, repulsion_strength = 1,
                       negative_sample_rate = 5, a = NULL, b = NULL, pca = NULL, pca_center = TRUE, seed = 10, ret_nn = FALSE,
                       n_threads = NULL, n_sgd_threads = 0, verbose = FALSE, batch = TRUE, ...) {
    .sharp_umap_refuse(metric, set_op_mix_ratio, local_connectivity, bandwidth)
    X <- .sharp_dmat(X)
    n <- nrow(X); dims <- as.integer(n_components); K <- as.integer(n_neighbors) - 1L
    if (is.null(a) != is.null(b)) stop("umap: give both a and b, or neither")
    ini <- .sharp_umap_init(init, n, dims, TRUE)
    r <- .C("sharp_C_umap", as.double(t(X)), as.double(n), ncol(X), as.integer(n_neighbors), dims,
            as.integer(if (is.null(n_epochs)) -1L else n_epochs), as.double(learning_rate), as.double(min_dist), as.double(spread),
            ab = as.double(if (is.null(a)) c(0, 0) else c(a, b)), as.integer(negative_sample_rate), as.double(repulsion_strength), ini$code,
            ini$Y, as.integer(if (is.null(pca)) 0L else pca), as.integer(pca_center), as.double(seed), Y = double(n * dims),
            as.integer(ret_nn), idx = integer(if (ret_nn) n * K else 1L), dist = double(if (ret_nn) n * K else 1L), status = integer(1))
    .sharp_check(r$status)
    Y <- matrix(r$Y, n, dims, byrow = TRUE)
    info <- if (ini$code == 3L) .sharp_umap_init_info("umap") else NULL     # (attr(Y, "init"), or $init beside the lists)
    if (!ret_nn) { attr(Y, "init") <- info; return(Y) }
    out <- list(embedding = Y, nn = list(euclidean = list(idx = cbind(seq_len(n), matrix(r$idx, n, K, byrow = TRUE) + 1L),
                                                          dist = cbind(0, matrix(r$dist, n, K, byrow = TRUE)))))
    out$init <- info
    out
}
# umap from neighbour lists the caller has: index n x K, 1-BASED, self excluded (what sharp_knn returns); distance their Euclidean
# distances, or squares with squared = TRUE.  n_neighbors is K + 1.  init: "random", "normlaplacian" (then attr(, "init") tells what the
# map started from) or a matrix.
sharp_umap_neighbors <- function(index, distance, squared = FALSE, n_components = 2, n_epochs = NULL, learning_rate = 1, init = "random",
                                 spread = 1, min_dist = 0.01, repulsion_strength = 1, negative_sample_rate = 5, a = NULL, b = NULL,
                                 seed = 10, metric = "euclidean", set_op_mix_ratio = 1, local_connectivity = 1, bandwidth = 1, ...) {
    .sharp_umap_refuse(metric, set_op_mix_ratio, local_connectivity, bandwidth)
    distance <- .sharp_dmat(distance)
    index <- as.matrix(index)
    if (!all(dim(index) == dim(distance))) stop("umap_neighbors: index and distance differ in shape")
    storage.mode(index) <- "integer"
    n <- nrow(distance); K <- ncol(distance); dims <- as.integer(n_components)
    if (is.null(a) != is.null(b)) stop("umap: give both a and b, or neither")
    ini <- .sharp_umap_init(init, n, dims, FALSE)
    i0 <- as.integer(t(index)) - 1L
    i0[is.na(i0)] <- -1L                                        # an NA index is out of range: the library names its row
    r <- .C("sharp_C_umap_neighbors", i0, as.double(t(distance)), as.double(n), as.integer(K), as.integer(squared), dims,
            as.integer(if (is.null(n_epochs)) -1L else n_epochs), as.double(learning_rate), as.double(min_dist), as.double(spread),
            ab = as.double(if (is.null(a)) c(0, 0) else c(a, b)), as.integer(negative_sample_rate), as.double(repulsion_strength), ini$code,
            ini$Y, as.double(seed), Y = double(n * dims), status = integer(1), NAOK = TRUE)
    .sharp_check(r$status)
    Y <- matrix(r$Y, n, dims, byrow = TRUE)
    if (ini$code == 3L) attr(Y, "init") <- .sharp_umap_init_info("umap_neighbors")
    Y
}

# ---- uwot::umap_transform: new rows placed in a fitted map (DESIGN.md 14) -----------------------------------------------------------------
# sharp_umap_model(X, embedding, ...) keeps the reference rows and their map on the device and returns a handle (class "sharp_umap_model");
# n_neighbors (1 .. 255, <= nrow(X)) counts the reference rows a new row is placed by; a, b: the fit's curve (sharp_umap_ab), n_epochs the
# fit's epochs.  sharp_umap_transform(X_new, model) returns the nrow(X_new) x n_components matrix, or with ret_nn = TRUE
# list(embedding =, nn = list(euclidean = list(idx =, dist =))) with 1-BASED indices into the reference.  n_epochs NULL: a third of the
# fit's; row_offset: the number of the block's first row (0-based) when a long table is transformed block by block, which then gives the
# bits of one call.  sharp_umap_model_free(model) releases the handle (sharp_shutdown releases what is left).
sharp_umap_model <- function(X, embedding, n_neighbors = 15, a = NULL, b = NULL, n_epochs = 500, spread = 1, min_dist = 0.01) {
    X <- .sharp_dmat(X)
    embedding <- .sharp_dmat(embedding)
    if (nrow(embedding) != nrow(X)) stop("umap_model: embedding must have one row per row of X")
    if (is.null(a) != is.null(b)) stop("umap_model: give both a and b, or neither")
    ab <- if (is.null(a)) sharp_umap_ab(spread, min_dist) else c(a = a, b = b)
    r <- .C("sharp_C_umap_model_create", as.double(t(X)), as.double(nrow(X)), ncol(X), as.double(t(embedding)), ncol(embedding),
            as.integer(n_neighbors), as.double(ab[["a"]]), as.double(ab[["b"]]), as.integer(n_epochs), handle = integer(1),
            status = integer(1))
    .sharp_check(r$status)
    structure(list(handle = r$handle, n_ref = nrow(X), d = ncol(X), n_components = ncol(embedding), n_neighbors = as.integer(n_neighbors),
                   a = ab[["a"]], b = ab[["b"]], n_epochs = as.integer(n_epochs)), class = "sharp_umap_model")
}
sharp_umap_model_free <- function(model) {
    r <- .C("sharp_C_umap_model_free", as.integer(model$handle), status = integer(1))
    .sharp_check(r$status)
    invisible(NULL)
}
sharp_umap_transform <- function(X_new, model, n_epochs = NULL, learning_rate = 1, negative_sample_rate = 5, repulsion_strength = 1,
                                 seed = 10, row_offset = 0, ret_nn = FALSE, ...) {
    if (!inherits(model, "sharp_umap_model")) stop("umap_transform: model must come from sharp_umap_model")
    X_new <- .sharp_dmat(X_new)
    if (ncol(X_new) != model$d) stop("umap_transform: X_new must have the model's ", model$d, " columns")
    n <- nrow(X_new); dims <- model$n_components; K <- model$n_neighbors
    r <- .C("sharp_C_umap_transform", as.integer(model$handle), as.double(t(X_new)), as.double(n), as.integer(model$d),
            as.integer(if (is.null(n_epochs)) -1L else n_epochs), as.double(learning_rate), as.integer(negative_sample_rate),
            as.double(repulsion_strength), as.double(seed), as.double(row_offset), Y = double(n * dims), as.integer(ret_nn),
            idx = integer(if (ret_nn) n * K else 1L), dist = double(if (ret_nn) n * K else 1L), status = integer(1))
    .sharp_check(r$status)
    Y <- matrix(r$Y, n, dims, byrow = TRUE)
    if (!ret_nn) return(Y)
    list(embedding = Y, nn = list(euclidean = list(idx = matrix(r$idx, n, K, byrow = TRUE) + 1L, dist = matrix(r$dist, n, K, byrow = TRUE))))
}

# ---- dist / hclust / plot_markers (R/plot_markers.R:38-242; DESIGN.md 11) ----------------------------------------------------------------
# pheatmap(cluster_rows = T, cluster_cols = T, clustering_method = "ward.D") at R/plot_markers.R:214-237 computes hclust(dist(sm), "ward.D")
# over the marker genes and hclust(dist(t(sm)), "ward.D") over up to ~10 000 cells.  sharp_dist / sharp_hclust do that on the GPU;
# sharp_hclust returns an object of class "hclust", which pheatmap(cluster_rows = , cluster_cols = ) accepts directly.
.sharp_dist_methods <- c(euclidean = 1L, maximum = 2L, manhattan = 3L, canberra = 4L, binary = 5L, minkowski = 6L, correlation = 7L)

# stats::dist(x, method, p = p) (+ method = "correlation": as.dist(1 - cor(t(x))), pheatmap's clustering_distance)
sharp_dist <- function(x, method = "euclidean", diag = FALSE, upper = FALSE, p = 2) {
    if (!method %in% names(.sharp_dist_methods)) stop("invalid distance method")
    x <- .sharp_dmat(x)
    n <- nrow(x)
    r <- .C("sharp_C_dist", as.double(t(x)), n, ncol(x), .sharp_dist_methods[[method]], as.double(p), d = double(n * (n - 1) / 2),
            status = integer(1))
    .sharp_check(r$status)
    structure(r$d, Size = n, Labels = rownames(x), Diag = diag, Upper = upper, method = method, call = match.call(), class = "dist")
}

# stats::hclust(d, method) for a dist object d, or -- x given -- hclust(dist(x, distance, p = p), method) with the distances kept on the GPU
sharp_hclust <- function(d = NULL, method = "ward.D", x = NULL, distance = "euclidean", p = 2) {
    hm <- .sharp_hmethod(method)
    if (is.null(x)) {
        n <- as.integer(attr(d, "Size"))
        r <- .C("sharp_C_hclust_dist", as.double(d), n, hm, merge = integer(2L * (n - 1L)), height = double(n - 1L), order = integer(n),
                status = integer(1))
        labels <- attr(d, "Labels"); dm <- attr(d, "method")
    } else {
        if (!distance %in% names(.sharp_dist_methods)) stop("invalid distance method")
        x <- .sharp_dmat(x)
        n <- nrow(x)
        r <- .C("sharp_C_hclust", as.double(t(x)), n, ncol(x), .sharp_dist_methods[[distance]], as.double(p), hm,
                merge = integer(2L * (n - 1L)), height = double(n - 1L), order = integer(n), status = integer(1))
        labels <- rownames(x); dm <- distance
    }
    .sharp_check(r$status)
    structure(list(merge = matrix(r$merge, ncol = 2L), height = r$height, order = r$order, labels = labels, method = method,
                   call = match.call(), dist.method = dm), class = "hclust")
}

# plot_markers (R/plot_markers.R:38): the reference's formals.  Keep :40-213 (selection, file type and name, colours) as they are and call
# pheatmap at :214-237 with cluster_rows = sharp_hclust(x = sm, method = "ward.D") and cluster_cols = sharp_hclust(x = t(sm), method =
# "ward.D") in place of cluster_rows = T, cluster_cols = T; `select` stands for those kept lines and returns list(sm, sortmarker, ...).
sharp_plot_markers <- function(sginfo, label, N.marker, sN.cluster, filename, filetype, nratio, n.cores, width = 900, height = 900, ...) {
    s <- .sharp_plot_markers_select(sginfo, label, N.marker, sN.cluster, nratio)                     # R/plot_markers.R:46-151
    if (ncol(s$sm) > 16384L) stop("plot_markers: more than 16384 cells selected: give a smaller nratio")
    if (missing(filetype)) filetype <- if (s$ncells < 5000) "pdf" else "png"                          # :184-190
    if (missing(filename)) filename <- paste0("markers_heatmap.", filetype)                          # :193-195
    if (filetype == "pdf") pdf(filename) else if (filetype == "png") png(filename, width = width, height = height)
    pheatmap::pheatmap(mat = s$sm, color = gplots::colorpanel(400, "blue", "white", "red"), border_color = NA,
                       cluster_rows = sharp_hclust(x = s$sm, method = "ward.D"), cluster_cols = sharp_hclust(x = t(s$sm), method = "ward.D"),
                       show_colnames = FALSE, show_rownames = TRUE, annotation_col = s$mat_col, annotation_colors = s$mat_colors,
                       drop_levels = TRUE, fontsize = 12, scale = "row", ...)
    dev.off()
    cat("Marker-genes heatmap saved into", filename, "\n")
    s$sortmarker
}

# R/plot_markers.R:46-181 without the foreach: markers, cells, log2 / z-score, annotation colours
.sharp_plot_markers_select <- function(sginfo, label, N.marker, sN.cluster, nratio) {
    if (missing(label)) label <- sginfo$label
    if (missing(nratio)) nratio <- 1e4 / length(label)
    mginfo <- sginfo$mginfo
    d <- cbind(genes = rownames(mginfo), mginfo)
    d <- d[order(d$icluster, d$pvalue), ]
    sortmarker <- d[order(d$icluster, -rank(d$auc), d$pvalue), ]
    if (missing(N.marker)) N.marker <- 10
    if (missing(sN.cluster)) sN.cluster <- length(unique(mginfo$icluster))
    kk <- sort(unique(mginfo$icluster))[1:sN.cluster]
    ssmarker <- do.call(rbind, lapply(kk, function(k) { x <- sortmarker[sortmarker$icluster == k, ]; x[seq_len(min(nrow(x), N.marker)), ] }))
    cellind <- order(label)
    newc <- label[cellind]
    sm <- sginfo$mat[rownames(ssmarker), cellind]
    scind <- which(newc %in% kk)
    newc <- newc[scind]; sm <- sm[, scind]
    if (length(cellind) > 1e4) {
        kt <- ceiling(table(newc) * nratio)
        xu <- unique(newc)
        ki <- unlist(lapply(seq_along(xu), function(i) which(newc == xu[i])[1:kt[i]]))
        sm <- sm[, ki]; newc <- newc[ki]
    }
    my <- if (sginfo$logmark) log2(sm + 1) else sm
    my <- my[apply(my, 1, function(x) sd(x) != 0), ]
    sm <- t(scale(t(my)))
    k0 <- colnames(sm); k1 <- duplicated(k0)
    if (any(k1)) k0[k1] <- paste0("d", seq_len(sum(k1)))
    colnames(sm) <- k0
    mat_col <- data.frame(cell_type = newc, row.names = k0)
    cols <- RColorBrewer::brewer.pal(length(unique(newc)), "Set1")
    names(cols) <- unique(newc)
    list(sm = sm, sortmarker = sortmarker, ncells = length(cellind), mat_col = mat_col, mat_colors = list(cell_type = cols))
}

# ---- silhouette / Calinski-Harabasz on any labelling (R/get_opt_hclust.R:103-105,134-144; DESIGN.md 12) ---------------------------------
# cluster::silhouette(x, dist): x = integer labels (or a SHARP result: its pred_clusters).  Either `dist` (a dist object, at most 46340
# observations) or `data` (observations in rows: matrix-free on the GPU, no n x n matrix, any number of cells).  Returns an object of
# class "silhouette" (columns cluster, neighbor, sil_width) as cluster::silhouette does, NA with fewer than 2 or more than n - 1 clusters.
# (A tree from sharp_hclust is cut with R's own cutree.)
sharp_silhouette <- function(x, dist = NULL, data = NULL, distance = "euclidean", p = 2) {
    if (is.list(x)) x <- x$pred_clusters
    if (is.null(dist) == is.null(data)) stop("give either dist (a dist object) or data (observations in rows)")
    n <- length(x)
    if (!all(x == round(x))) stop("'x' must only have integer codes")
    f <- factor(x)
    k <- nlevels(f)
    if (k <= 1 || k >= n) return(NA)
    cl <- as.integer(f)
    if (!is.null(dist)) {
        if (as.integer(attr(dist, "Size")) != n) stop("clustering 'x' and dissimilarity 'dist' are incompatible")
        r <- .C("sharp_C_silhouette_dist", as.double(dist), n, cl, k, neighbor = integer(n), width = double(n), status = integer(1))
    } else {
        if (!distance %in% names(.sharp_dist_methods)) stop("invalid distance method")
        data <- .sharp_dmat(data)
        if (nrow(data) != n) stop("the number of labels differs from the number of observations")
        r <- .C("sharp_C_silhouette", as.double(t(data)), as.double(n), ncol(data), .sharp_dist_methods[[distance]], as.double(p), cl, k,
                neighbor = integer(n), width = double(n), status = integer(1))
    }
    .sharp_check(r$status)
    lev <- as.numeric(levels(f))
    structure(cbind(cluster = lev[cl], neighbor = lev[r$neighbor], sil_width = r$width), Ordered = FALSE, call = match.call(),
              class = "silhouette")
}

# clusterCrit::intCriteria(data, labels, "Calinski_Harabasz") (distance = "euclidean", R/get_opt_hclust.R:105) and
# clues::get_CH(data, labels, disMethod = "1-corr") (distance = "1-corr", R/get_opt_hclust.R:144); observations in rows
sharp_calinski_harabasz <- function(data, labels, distance = "euclidean") {
    kind <- match(distance, c("euclidean", "1-corr")) - 1L
    if (is.na(kind)) stop("distance must be \"euclidean\" or \"1-corr\"")
    data <- .sharp_dmat(data)
    f <- factor(labels)
    if (length(f) != nrow(data)) stop("the number of labels differs from the number of observations")
    r <- .C("sharp_C_calinski_harabasz", as.double(t(data)), as.double(nrow(data)), ncol(data), as.integer(f), nlevels(f), kind,
            out = double(1), status = integer(1))
    .sharp_check(r$status)
    r$out
}

# ---- trustworthiness / continuity of a map (DESIGN.md 17) ---------------------------------------------------------------------------------
# rank[i, k] = 1 + the number of rows l != i with (d2(i, l), l) < (d2(i, j), j), j = index[i, k]: where the rows a list names stand among
# all rows of X, by sharp_knn's squared distances, ties to the lower index.  index: n x K, 1-based here (sharp_knn(X, K)$index), each row
# K other rows.  Matrix-free on the GPU (sharp_C_neighbor_ranks): no n x n matrix.
sharp_neighbor_ranks <- function(X, index, max_rows_per_launch = 0L) {
    X <- .sharp_dmat(X)
    n <- nrow(X)
    if (is.list(index)) index <- index$index
    index <- as.matrix(index)
    if (nrow(index) != n) stop("the neighbour lists and the data differ in their number of rows")
    K <- ncol(index)
    r <- .C("sharp_C_neighbor_ranks", as.double(t(X)), as.double(n), ncol(X), as.integer(K), as.integer(t(index) - 1L),
            as.integer(max_rows_per_launch), rank = integer(n * K), status = integer(1))
    .sharp_check(r$status)
    matrix(r$rank, n, K, byrow = TRUE)
}

.sharp_map_score <- function(ranked, listed, n_neighbors) {
    n <- nrow(ranked)
    K <- as.integer(n_neighbors)
    if (nrow(listed) != n) stop("X and Y differ in their number of rows: a map has one row per row of X")
    if (K >= n / 2) stop(sprintf("n_neighbors (%d) should be less than n_samples / 2 (%s)", K, format(n / 2)))
    rank <- sharp_neighbor_ranks(ranked, sharp_knn(listed, K)$index)
    penalty <- sum(as.numeric(pmax(rank - K, 0L)))                # (a double: exact far beyond any total that can occur)
    1 - penalty * (2 / (as.numeric(n) * K * (2 * n - 3 * K - 1)))
}

# sklearn.manifold.trustworthiness(X, Y, n_neighbors) (Venna and Kaski): the ranks in X of each row's n_neighbors nearest rows in the
# map Y; sharp_continuity: the ranks in Y of each row's nearest rows in X
sharp_trustworthiness <- function(X, Y, n_neighbors = 5L) .sharp_map_score(.sharp_dmat(X), .sharp_dmat(Y), n_neighbors)
sharp_continuity <- function(X, Y, n_neighbors = 5L) .sharp_map_score(.sharp_dmat(Y), .sharp_dmat(X), n_neighbors)

# ---- Louvain on the neighbour graph (DESIGN.md 18) -----------------------------------------------------------------------------------------
.sharp_louvain_result <- function(r, n, ret_levels) {
    nl <- r$n_levels
    lev <- matrix(r$levels, ncol = 4, byrow = TRUE)[seq_len(nl), , drop = FALSE]
    colnames(lev) <- c("n", "communities", "rounds", "modularity")
    out <- list(membership = r$membership, n_communities = lev[nl, "communities"], modularity = lev[nl, "modularity"], levels = lev)
    if (ret_levels) out$level_membership <- matrix(r$lm[seq_len(nl * n)], nl, n, byrow = TRUE) + 1L
    out
}

# A clustering read off the neighbour graph, as sc.tl.louvain and Seurat's FindClusters run it: X (observations in rows; the exact
# k-NN is sharp_knn's) or the lists sharp_knn returned (a list with $index, 1-based, and $distance).  graph = "fuzzy": the fuzzy union
# sharp_umap builds (scanpy's connectivities); graph = "snn": the SNN / Jaccard graph of the same lists (n_neighbors is Seurat's k.param,
# prune its prune.SNN; DESIGN.md 19).  membership: 1 .. G by decreasing size; levels: one row (n, communities, rounds, modularity) per
# level.  The method is the project's own synchronous form of Louvain; two calls give the same bits.
sharp_louvain <- function(X, n_neighbors = 15L, resolution = 1, seed = 10, tol = 1e-7, max_levels = 20L, max_rounds = 200L, max_fails = 4L,
                          ret_levels = FALSE, graph = c("fuzzy", "snn"), prune = NULL) {
    graph <- match.arg(graph)
    if (graph == "fuzzy" && !is.null(prune)) stop("prune belongs to graph = \"snn\"")
    nn <- if (is.list(X) && !is.null(X$index)) X else sharp_knn(.sharp_dmat(X), as.integer(n_neighbors) - 1L)
    index <- as.matrix(nn$index)
    n <- nrow(index)
    K <- ncol(index)
    cap <- as.integer(max_levels)
    if (graph == "snn") {
        r <- .C("sharp_C_louvain_snn", as.integer(t(index) - 1L), as.double(n), as.integer(K), as.double(if (is.null(prune)) 1 / 15 else prune),
                as.double(resolution), as.double(tol), cap, as.integer(max_rounds), as.integer(max_fails), as.double(seed),
                membership = integer(n), cap, levels = double(4 * cap), n_levels = integer(1), as.integer(ret_levels),
                lm = integer(if (ret_levels) cap * n else 1L), status = integer(1))
    } else {
        r <- .C("sharp_C_louvain_neighbors", as.integer(t(index) - 1L), as.double(t(as.matrix(nn$distance))), as.double(n), as.integer(K), 0L,
                as.double(resolution), as.double(tol), cap, as.integer(max_rounds), as.integer(max_fails), as.double(seed),
                membership = integer(n), cap, levels = double(4 * cap), n_levels = integer(1), as.integer(ret_levels),
                lm = integer(if (ret_levels) cap * n else 1L), status = integer(1))
    }
    .sharp_check(r$status)
    .sharp_louvain_result(r, n, ret_levels)
}

# The SNN / Jaccard graph of neighbour lists (Seurat's ComputeSNN formula; DESIGN.md 19): index as sharp_knn returns it (n x K, 1-based,
# self excluded), k = K + 1, w = s / (2k - s) for the s shared members of the two rows' lists (each with the row itself), entries with
# w < prune dropped, no diagonal.  Returns the 1-based triplet list(i, j, x, n) for Matrix::sparseMatrix(i = i, j = j, x = x,
# dims = c(n, n)), by rows with ascending columns; two .C calls: the count, then the fill.
sharp_snn_graph <- function(index, prune = 1 / 15) {
    index <- as.matrix(index)
    n <- nrow(index)
    K <- ncol(index)
    idx <- as.integer(t(index) - 1L)
    r <- .C("sharp_C_snn_graph", idx, as.double(n), as.integer(K), as.double(prune), 0, row_ptr = double(n + 1), integer(1), double(1),
            integer(1), 0L, nnz = double(1), status = integer(1))
    .sharp_check(r$status)
    nnz <- r$nnz
    r <- .C("sharp_C_snn_graph", idx, as.double(n), as.integer(K), as.double(prune), as.double(nnz), row_ptr = double(n + 1),
            col = integer(max(nnz, 1)), val = double(max(nnz, 1)), integer(1), 1L, nnz = double(1), status = integer(1))
    .sharp_check(r$status)
    list(i = rep.int(seq_len(n), diff(r$row_ptr)), j = r$col[seq_len(nnz)] + 1L, x = r$val[seq_len(nnz)], n = n)
}

# A truncated PCA of sparse expression blocks (DESIGN.md 21): scExp a dgCMatrix or a list of them, genes x cells, as SHARP_unlimited
# takes them (a dense block is converted).  Cells are scaled to normalize.total counts (NULL: not), log1p is taken, genes are centred
# and, with scale, divided by their standard deviation.  Returns list(scores (cells x n.components: the input of sharp_knn, sharp_umap
# (pca = NULL) and sharp_louvain), loadings (genes x n.components), singular.values, sdev, center, scale, gene.var, total.var).
.sharp_csc_cat <- function(scExp, who) {
    if (!is.list(scExp)) scExp <- list(scExp)
    if (length(scExp) < 1) stop("No expression data is provided!")
    cs <- lapply(scExp, function(b) .sharp_block(if (inherits(b, "sparseMatrix")) b else methods::as(methods::as(data.matrix(b), "CsparseMatrix"), "dgCMatrix")))
    if (sum(as.numeric(vapply(cs, function(b) length(b$x), 1))) >= 2^31) stop(paste0(who, ": .C() carries at most 2^31 - 1 values"))
    list(p = unlist(lapply(cs, `[[`, "p")), i = unlist(lapply(cs, `[[`, "i")), x = as.double(unlist(lapply(cs, `[[`, "x"))), nb = length(cs),
         ncb = as.double(vapply(cs, function(b) b$dim[2], 1L)), m = as.integer(cs[[1]]$dim[1]))
}
sharp_expression_pca <- function(scExp, n.components = 50L, oversample = 10L, n.iter = 4L, normalize.total = 1e4, log1p = TRUE, scale = FALSE,
                                 seed = 0) {
    b <- .sharp_csc_cat(scExp, "sharp_expression_pca")
    n <- sum(b$ncb); k <- as.integer(n.components)
    r <- .C("sharp_C_expr_pca_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m, k, as.integer(oversample), as.integer(n.iter),
            as.double(if (is.null(normalize.total)) 0 else normalize.total), as.integer(log1p), as.integer(scale), as.double(seed),
            scores = double(n * k), loadings = double(b$m * k), sv = double(k), sdev = double(k), center = double(b$m), scale = double(b$m),
            gene_var = double(b$m), total_var = double(1), status = integer(1))
    .sharp_check(r$status)
    list(scores = t(matrix(r$scores, nrow = k)), loadings = t(matrix(r$loadings, nrow = k)), singular.values = r$sv, sdev = r$sdev,
         center = r$center, scale = r$scale, gene.var = r$gene_var, total.var = r$total_var, normalize.total = normalize.total, log1p = log1p)
}
# the scores of new cells in a fit of sharp_expression_pca
sharp_expression_pca_transform <- function(scExp.new, fit) {
    b <- .sharp_csc_cat(scExp.new, "sharp_expression_pca_transform")
    n <- sum(b$ncb); k <- ncol(fit$loadings)
    if (nrow(fit$loadings) != b$m) stop("the new cells and the fit do not have the same genes")
    r <- .C("sharp_C_expr_pca_transform_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m,
            as.double(if (is.null(fit$normalize.total)) 0 else fit$normalize.total), as.integer(fit$log1p), as.double(t(fit$loadings)),
            as.double(fit$center), as.double(fit$scale), as.integer(k), scores = double(max(n * k, 1)), status = integer(1))
    .sharp_check(r$status)
    t(matrix(r$scores[seq_len(n * k)], nrow = k))
}
# per gene, after that transform: mean, var (n - 1 in the denominator), nnz (cells with a non-zero value); per cell cell.sum
sharp_gene_stats <- function(scExp, normalize.total = 1e4, log1p = TRUE) {
    b <- .sharp_csc_cat(scExp, "sharp_gene_stats")
    r <- .C("sharp_C_expr_stats_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m,
            as.double(if (is.null(normalize.total)) 0 else normalize.total), as.integer(log1p), mean = double(b$m), var = double(b$m),
            nnz = double(b$m), cell_sum = double(sum(b$ncb)), status = integer(1))
    .sharp_check(r$status)
    list(mean = r$mean, var = r$var, nnz = r$nnz, cell.sum = r$cell_sum)
}

# Variable-gene selection and gene subsets (DESIGN.md 22).  genes: 1-based, strictly ascending indices, or a logical mask of length m.
.sharp_genes0 <- function(genes, m, who) {
    if (is.logical(genes)) {
        if (length(genes) != m) stop(paste0(who, ": the genes mask must have one entry per gene"))
        genes <- which(genes)
    }
    genes <- as.integer(genes)
    if (length(genes) < 1) stop(paste0(who, ": genes is empty (it must keep at least one gene)"))
    genes - 1L                                   # (the library refuses unsorted, repeated and out-of-range genes by name)
}
# the n.top.genes most variable genes of raw counts: list(means, variances, variances.expected, variances.norm, rank (1-based among
# the selected, NA otherwise), highly.variable, genes (1-based, ascending: what sharp_expression_pca_genes takes), n.selected, q,
# degree.counts)
sharp_highly_variable_genes <- function(scExp, n.top.genes = 2000L, span = 0.3) {
    b <- .sharp_csc_cat(scExp, "sharp_highly_variable_genes")
    top <- as.integer(n.top.genes)
    r <- .C("sharp_C_expr_hvg_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m, top, as.double(span), means = double(b$m),
            variances = double(b$m), ve = double(b$m), vn = double(b$m), rank = integer(b$m), hv = integer(b$m),
            genes = integer(max(min(top, b$m), 1L)), ns = integer(1), q = integer(1), dc = integer(3), status = integer(1))
    .sharp_check(r$status)
    list(means = r$means, variances = r$variances, variances.expected = r$ve, variances.norm = r$vn,
         rank = ifelse(r$rank < 0L, NA_integer_, r$rank + 1L), highly.variable = r$hv != 0L, genes = r$genes[seq_len(r$ns)] + 1L,
         n.selected = r$ns, span = span, q = r$q, degree.counts = r$dc)
}
# sharp_expression_pca on the genes `genes` alone: the cells are normalised by their sums over all genes, then the others are dropped
sharp_expression_pca_genes <- function(scExp, genes, n.components = 50L, oversample = 10L, n.iter = 4L, normalize.total = 1e4, log1p = TRUE,
                                       scale = FALSE, seed = 0) {
    b <- .sharp_csc_cat(scExp, "sharp_expression_pca_genes")
    g <- .sharp_genes0(genes, b$m, "sharp_expression_pca_genes")
    n <- sum(b$ncb); k <- as.integer(n.components); mk <- length(g)
    r <- .C("sharp_C_expr_pca_sub_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m, k, as.integer(oversample),
            as.integer(n.iter), as.double(if (is.null(normalize.total)) 0 else normalize.total), as.integer(log1p), as.integer(scale),
            as.double(seed), scores = double(n * k), loadings = double(mk * k), sv = double(k), sdev = double(k), center = double(mk),
            scale = double(mk), gene_var = double(mk), total_var = double(1), g, mk, status = integer(1))
    .sharp_check(r$status)
    list(scores = t(matrix(r$scores, nrow = k)), loadings = t(matrix(r$loadings, nrow = k)), singular.values = r$sv, sdev = r$sdev,
         center = r$center, scale = r$scale, gene.var = r$gene_var, total.var = r$total_var, normalize.total = normalize.total, log1p = log1p,
         genes = g + 1L, n.genes.in = b$m)
}
# the scores of new cells (with all n.genes.in genes) in a fit of sharp_expression_pca_genes
sharp_expression_pca_genes_transform <- function(scExp.new, fit) {
    b <- .sharp_csc_cat(scExp.new, "sharp_expression_pca_genes_transform")
    if (b$m != fit$n.genes.in) stop("the new cells and the fit do not have the same genes")
    g <- as.integer(fit$genes) - 1L
    n <- sum(b$ncb); k <- ncol(fit$loadings)
    r <- .C("sharp_C_expr_pca_transform_sub_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m,
            as.double(if (is.null(fit$normalize.total)) 0 else fit$normalize.total), as.integer(fit$log1p), as.double(t(fit$loadings)),
            as.double(fit$center), as.double(fit$scale), as.integer(k), scores = double(max(n * k, 1)), g, length(g), status = integer(1))
    .sharp_check(r$status)
    t(matrix(r$scores[seq_len(n * k)], nrow = k))
}
# sharp_gene_stats of the genes `genes` alone; cell.sum stays the sum over all genes
sharp_gene_stats_genes <- function(scExp, genes, normalize.total = 1e4, log1p = TRUE) {
    b <- .sharp_csc_cat(scExp, "sharp_gene_stats_genes")
    g <- .sharp_genes0(genes, b$m, "sharp_gene_stats_genes")
    mk <- length(g)
    r <- .C("sharp_C_expr_stats_sub_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m,
            as.double(if (is.null(normalize.total)) 0 else normalize.total), as.integer(log1p), mean = double(mk), var = double(mk),
            nnz = double(mk), cell_sum = double(sum(b$ncb)), g, mk, status = integer(1))
    .sharp_check(r$status)
    list(mean = r$mean, var = r$var, nnz = r$nnz, cell.sum = r$cell_sum)
}

# A Harmony-style batch integration of PCA scores (DESIGN.md 23): Z cells x d (what sharp_expression_pca's $scores holds), batch one
# label per cell of any kind (factor() orders them).  list(Z.corr (cells x d, Z's row order), Y (n.clusters x d), objective, rounds, n.iter,
# converged, n.clusters, n.batches, batch.levels, and R (cells x n.clusters) with ret.R).  Nothing here is an index, so nothing is 1-based.
sharp_harmony <- function(Z, batch, n.clusters = NULL, sigma = 0.1, theta = 2, lam = 1, max.iter = 10L, max.iter.cluster = 20L,
                          n.blocks = 20L, epsilon.cluster = 1e-5, epsilon.harmony = 1e-4, init.iter = 10L, seed = 1, ret.R = FALSE) {
    Z <- as.matrix(Z)
    n <- nrow(Z); d <- ncol(Z)
    if (length(batch) != n) stop("sharp_harmony: batch must hold one label per cell")
    f <- factor(batch)
    B <- nlevels(f)
    K <- as.integer(if (is.null(n.clusters)) min(round(n / 30), 100) else n.clusters)
    it <- as.integer(max.iter)
    r <- .C("sharp_C_harmony", as.double(t(Z)), as.double(n), as.integer(d), as.integer(f) - 1L, as.integer(B), K, as.double(sigma),
            as.double(theta), as.double(lam), it, as.integer(max.iter.cluster), as.integer(n.blocks), as.double(epsilon.cluster),
            as.double(epsilon.harmony), as.integer(init.iter), as.double(seed), Zc = double(n * d), Y = double(max(K, 1L) * d),
            objective = double(max(it, 1L)), rounds = integer(max(it, 1L)), n_iter = integer(1), converged = integer(1), as.integer(ret.R),
            R = double(if (ret.R) n * max(K, 1L) else 1L), status = integer(1))
    .sharp_check(r$status)
    out <- list(Z.corr = t(matrix(r$Zc, nrow = d)), Y = t(matrix(r$Y, nrow = d)), objective = r$objective[seq_len(r$n_iter)],
                rounds = r$rounds[seq_len(r$n_iter)], n.iter = r$n_iter, converged = r$converged != 0L, n.clusters = K, n.batches = B,
                batch.levels = levels(f))
    if (ret.R) out$R <- t(matrix(r$R, nrow = K))
    out
}
# the block number of every cell of a list of genes x cells blocks, in sharp_expression_pca's order: the batch of sharp_harmony
sharp_batch_of_blocks <- function(blocks) rep(seq_along(blocks), vapply(blocks, ncol, 1L))

# Scrublet-style doublet detection on raw counts (DESIGN.md 24): scExp as sharp_expression_pca takes it.  round(sim.doublet.ratio n)
# doublets are simulated on the GPU as sums of two cells, placed in the observed cells' PCA (fitted here on n.top.genes variable genes,
# or on `genes`, 1-based; or the caller's pca = a result of sharp_expression_pca_genes / sharp_expression_pca, used as it is) and every
# cell is scored by the simulated share of its k.adj = round(n.neighbors (1 + n.sim / n)) nearest neighbours.  k.adj must be <= 255 (the
# k-NN's limit): the default n.neighbors is min(round(0.5 sqrt(n)), the largest value that fits), an explicit one beyond it is refused.
# threshold NULL: the minimum between the two modes of the simulated scores' histogram; when it never shows two modes a warning says so
# and threshold, predicted.doublets and the rates are NA / NULL.  list(doublet.scores, doublet.scores.sim, predicted.doublets,
# threshold, threshold.found, detected.doublet.rate, detectable.doublet.fraction, overall.doublet.rate, n.neighbors, k.adj, n.sim,
# parents (n.sim x 2, 1-based), genes (1-based, or NULL), neighbor.counts, and sim.pca with ret.sim).
sharp_scrublet <- function(scExp, sim.doublet.ratio = 2, expected.doublet.rate = 0.1, n.neighbors = NULL, n.prin.comps = 30L,
                           n.top.genes = 2000L, genes = NULL, pca = NULL, normalize.total = 1e4, log1p = TRUE, scale = TRUE, threshold = NULL,
                           nn.method = c("exact", "descent"), nn.args = NULL, seed = 0, ret.sim = FALSE) {
    who <- "sharp_scrublet"
    nn.method <- match.arg(nn.method)
    b <- .sharp_csc_cat(scExp, who)
    n <- sum(b$ncb)
    n.sim <- floor(sim.doublet.ratio * n + 0.5)
    if (!is.finite(n.sim) || n.sim < 1) stop("scrublet: sim_doublet_ratio gives fewer than 1 simulated doublet")
    have.fit <- !is.null(pca)
    if (have.fit) {
        if (!is.null(genes)) stop("scrublet: genes belongs to the fit; with pca the pca's own gene subset is used")
        m.fit <- if (is.null(pca$genes)) nrow(pca$loadings) else pca$n.genes.in
        if (m.fit != b$m) stop(paste0("scrublet: the pca was fitted on ", m.fit, " genes, the blocks have ", b$m))
        if (nrow(pca$scores) != n) stop(paste0("scrublet: the pca's scores are ", nrow(pca$scores), " cells, the blocks have ", n))
        g <- if (is.null(pca$genes)) NULL else as.integer(pca$genes) - 1L
        k <- ncol(pca$loadings)
        normalize.total <- pca$normalize.total; log1p <- pca$log1p
        fit <- list(as.double(t(pca$scores)), as.double(t(pca$loadings)), as.double(pca$center), as.double(pca$scale))
    } else {
        g <- if (is.null(genes)) NULL else .sharp_genes0(genes, b$m, who)
        k <- as.integer(n.prin.comps)
        fit <- list(double(1), double(1), double(1), double(1))
    }
    top <- as.integer(n.top.genes)
    ng <- length(g)
    nn <- c(8, 0, 12, 0.001, 10)
    names(nn) <- c("n_projections", "max_candidates", "n_iters", "delta", "seed")
    if (!is.null(nn.args)) {
        if (nn.method != "descent") stop("scrublet: nn_args belong to nn_method = \"descent\"")
        if (!all(names(nn.args) %in% names(nn))) stop("scrublet: nn.args takes n_projections, max_candidates, n_iters, delta, seed")
        nn[names(nn.args)] <- as.double(unlist(nn.args))
    }
    r <- .C("sharp_C_scrublet_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m, as.double(sim.doublet.ratio),
            as.double(expected.doublet.rate), as.integer(if (is.null(n.neighbors)) 0L else n.neighbors), as.integer(k), top,
            if (ng) g else integer(1), as.integer(ng), as.integer(have.fit), fit[[1]], fit[[2]], fit[[3]], fit[[4]],
            as.double(if (is.null(normalize.total)) 0 else normalize.total), as.integer(log1p), as.integer(scale),
            as.double(if (is.null(threshold)) NA_real_ else threshold), as.integer(nn.method == "descent"), as.integer(!is.null(nn.args)),
            as.double(nn), as.double(seed), 0L, scores = double(n), scores_sim = double(n.sim), predicted = integer(n), threshold = double(1),
            found = integer(1), rates = double(3), nn = integer(1), k_adj = integer(1), parents = integer(2 * n.sim),
            genes = integer(max(ng, min(top, b$m), 1L)), n_genes = integer(1), counts = integer(n + n.sim), as.integer(ret.sim),
            sim_pca = double(if (ret.sim) n.sim * k else 1L), status = integer(1), NAOK = TRUE)
    .sharp_check(r$status)
    have <- !is.nan(r$threshold)
    if (!have) warning("scrublet: no threshold found: the histogram of the simulated doublets' scores never shows two modes; predicted.doublets is NULL")
    out <- list(doublet.scores = r$scores, doublet.scores.sim = r$scores_sim, predicted.doublets = if (have) r$predicted != 0L else NULL,
                threshold = if (have) r$threshold else NA_real_, threshold.found = r$found != 0L,
                detected.doublet.rate = if (have) r$rates[1] else NA_real_, detectable.doublet.fraction = if (have) r$rates[2] else NA_real_,
                overall.doublet.rate = if (have) r$rates[3] else NA_real_, n.neighbors = r$nn, k.adj = r$k_adj, n.sim = n.sim,
                parents = t(matrix(r$parents, nrow = 2)) + 1L, genes = if (r$n_genes > 0) r$genes[seq_len(r$n_genes)] + 1L else NULL,
                neighbor.counts = r$counts)
    if (ret.sim) out$sim.pca <- t(matrix(r$sim_pca, nrow = k))
    out
}

# the same on any symmetric graph: a dgCMatrix-like triple (row_ptr 0-based with n + 1 values, col 0-based, val)
sharp_louvain_graph <- function(row_ptr, col, val, resolution = 1, seed = 10, tol = 1e-7, max_levels = 20L, max_rounds = 200L,
                                max_fails = 4L, ret_levels = FALSE) {
    n <- length(row_ptr) - 1L
    cap <- as.integer(max_levels)
    r <- .C("sharp_C_louvain_graph", as.double(row_ptr), as.integer(col), as.double(val), as.double(n), as.double(resolution),
            as.double(tol), cap, as.integer(max_rounds), as.integer(max_fails), as.double(seed), membership = integer(n), cap,
            levels = double(4 * cap), n_levels = integer(1), as.integer(ret_levels), lm = integer(if (ret_levels) cap * n else 1L),
            status = integer(1))
    .sharp_check(r$status)
    .sharp_louvain_result(r, n, ret_levels)
}

# Q of a labelling of that graph, on the integer weights and in the order sharp_louvain sums them
sharp_modularity <- function(row_ptr, col, val, membership, resolution = 1) {
    n <- length(row_ptr) - 1L
    if (length(membership) != n) stop("membership must hold one label per vertex")
    r <- .C("sharp_C_louvain_modularity", as.double(row_ptr), as.integer(col), as.double(val), as.double(n),
            as.integer(factor(membership)) - 1L, as.double(resolution), Q = double(1), status = integer(1))
    .sharp_check(r$status)
    r$Q
}

# ---- Leiden on the neighbour graph (DESIGN.md 25) ------------------------------------------------------------------------------------------
.sharp_leiden_result <- function(r, n, ret_levels) {
    nl <- r$n_levels
    lev <- matrix(r$levels, ncol = 6, byrow = TRUE)[seq_len(nl), , drop = FALSE]
    colnames(lev) <- c("n", "communities", "sub_communities", "rounds", "refine_rounds", "modularity")
    out <- list(membership = r$membership, n_communities = max(r$membership), modularity = r$Q, levels = lev)
    if (ret_levels) out$level_membership <- matrix(r$lm[seq_len(nl * n)], nl, n, byrow = TRUE) + 1L
    out
}

# sharp_louvain's arguments and graphs with Leiden's refinement between a level's move phase and its aggregation (scanpy's sc.tl.leiden,
# Seurat's FindClusters(algorithm = 4)): every returned community is connected.  levels: one row (n, communities, sub_communities, rounds,
# refine_rounds, modularity) per level; modularity: of the returned membership (sharp_modularity of it).  The project's own deterministic
# form of the method: no random choice among the candidates, one iteration; no parity with leidenalg or igraph is claimed.
sharp_leiden <- function(X, n_neighbors = 15L, resolution = 1, seed = 10, tol = 1e-7, max_levels = 20L, max_rounds = 200L, max_fails = 4L,
                         max_refine_rounds = 200L, ret_levels = FALSE, graph = c("fuzzy", "snn"), prune = NULL) {
    graph <- match.arg(graph)
    if (graph == "fuzzy" && !is.null(prune)) stop("prune belongs to graph = \"snn\"")
    nn <- if (is.list(X) && !is.null(X$index)) X else sharp_knn(.sharp_dmat(X), as.integer(n_neighbors) - 1L)
    index <- as.matrix(nn$index)
    n <- nrow(index)
    K <- ncol(index)
    cap <- as.integer(max_levels)
    if (graph == "snn") {
        r <- .C("sharp_C_leiden_snn", as.integer(t(index) - 1L), as.double(n), as.integer(K), as.double(if (is.null(prune)) 1 / 15 else prune),
                as.double(resolution), as.double(tol), cap, as.integer(max_rounds), as.integer(max_fails), as.integer(max_refine_rounds),
                as.double(seed), membership = integer(n), Q = double(1), cap, levels = double(6 * cap), n_levels = integer(1),
                as.integer(ret_levels), lm = integer(if (ret_levels) cap * n else 1L), status = integer(1))
    } else {
        r <- .C("sharp_C_leiden_neighbors", as.integer(t(index) - 1L), as.double(t(as.matrix(nn$distance))), as.double(n), as.integer(K), 0L,
                as.double(resolution), as.double(tol), cap, as.integer(max_rounds), as.integer(max_fails), as.integer(max_refine_rounds),
                as.double(seed), membership = integer(n), Q = double(1), cap, levels = double(6 * cap), n_levels = integer(1),
                as.integer(ret_levels), lm = integer(if (ret_levels) cap * n else 1L), status = integer(1))
    }
    .sharp_check(r$status)
    .sharp_leiden_result(r, n, ret_levels)
}

# the same on any symmetric graph: sharp_louvain_graph's triple
sharp_leiden_graph <- function(row_ptr, col, val, resolution = 1, seed = 10, tol = 1e-7, max_levels = 20L, max_rounds = 200L,
                               max_fails = 4L, max_refine_rounds = 200L, ret_levels = FALSE) {
    n <- length(row_ptr) - 1L
    cap <- as.integer(max_levels)
    r <- .C("sharp_C_leiden_graph", as.double(row_ptr), as.integer(col), as.double(val), as.double(n), as.double(resolution),
            as.double(tol), cap, as.integer(max_rounds), as.integer(max_fails), as.integer(max_refine_rounds), as.double(seed),
            membership = integer(n), Q = double(1), cap, levels = double(6 * cap), n_levels = integer(1), as.integer(ret_levels),
            lm = integer(if (ret_levels) cap * n else 1L), status = integer(1))
    .sharp_check(r$status)
    .sharp_leiden_result(r, n, ret_levels)
}

# ---- diffusion maps and diffusion pseudotime on the neighbour graph (DESIGN.md 26; scanpy's tl.diffmap / tl.dpt without the branchings).
# The project's own specification; no parity with scanpy or destiny is claimed.  These wrappers have not been run in R.
.sharp_diffmap_result <- function(r, n, n_comps, who, density_normalize) {
    .sharp_check(r$status)
    if (r$components > 1)
        warning(sprintf("%s: the graph has %d connected components; the one of %d cells was solved and %d cells are left out", who,
                        as.integer(r$components), as.integer(r$size), as.integer(n - r$size)))
    if (r$outcome != 0)
        warning(sprintf("%s: not converged after %d operator applications: the largest residual is %.3e", who, r$steps, max(r$residual)))
    list(evals = r$evals, evecs = matrix(r$evecs, n, n_comps, byrow = TRUE), residual = r$residual, converged = r$outcome == 0,
         steps = r$steps, restarts = r$restarts, components = r$components, component_size = r$size,
         in_component = as.logical(r$inside), density_normalize = density_normalize)
}

# X: a matrix (rows are cells), or sharp_knn's list (1-based index, Euclidean distance).  root: NULL (the largest component) or a
# 1-based cell whose component is solved.  evecs: n x n_comps, NaN in the rows outside the solved component; evals[1] = 1.
sharp_diffmap <- function(X, n_neighbors = 15L, n_comps = 15L, density_normalize = TRUE, root = NULL, tol = 0, max_matvecs = 0L) {
    nn <- if (is.list(X) && !is.null(X$index)) X else sharp_knn(.sharp_dmat(X), as.integer(n_neighbors) - 1L)
    index <- as.matrix(nn$index)
    n <- nrow(index)
    nc <- as.integer(n_comps)
    r <- .C("sharp_C_diffmap_neighbors", as.integer(t(index) - 1L), as.double(t(as.matrix(nn$distance))), as.double(n), as.integer(ncol(index)),
            0L, nc, as.integer(density_normalize), as.double(if (is.null(root)) -1 else root - 1), as.double(tol), as.integer(max_matvecs),
            evals = double(nc), evecs = double(n * nc), residual = double(nc), inside = integer(n), steps = integer(1),
            restarts = integer(1), components = double(1), size = double(1), outcome = integer(1), status = integer(1))
    .sharp_diffmap_result(r, n, nc, "sharp_diffmap", density_normalize)
}

# the same on any symmetric graph: sharp_louvain_graph's triple (row_ptr and col 0-based)
sharp_diffmap_graph <- function(row_ptr, col, val, n_comps = 15L, density_normalize = TRUE, root = NULL, tol = 0, max_matvecs = 0L) {
    n <- length(row_ptr) - 1L
    nc <- as.integer(n_comps)
    r <- .C("sharp_C_diffmap_graph", as.double(row_ptr), as.integer(col), as.double(val), as.double(n), nc, as.integer(density_normalize),
            as.double(if (is.null(root)) -1 else root - 1), as.double(tol), as.integer(max_matvecs), evals = double(nc),
            evecs = double(n * nc), residual = double(nc), inside = integer(n), steps = integer(1), restarts = integer(1),
            components = double(1), size = double(1), outcome = integer(1), status = integer(1))
    .sharp_diffmap_result(r, n, nc, "sharp_diffmap_graph", density_normalize)
}

# pseudotime from a sharp_diffmap result: roots 1-based cells inside the solved component -> n x length(roots) (a vector for one root);
# Inf outside the component; normalize: each root's values divided by their largest finite one
sharp_dpt <- function(dm, roots, n_dcs = 10L, normalize = TRUE) {
    n <- nrow(dm$evecs)
    nc <- ncol(dm$evecs)
    r <- .C("sharp_C_dpt", as.double(dm$evals), as.double(t(dm$evecs)), as.double(n), as.integer(nc), as.integer(n_dcs),
            as.integer(roots - 1L), length(roots), as.integer(normalize), out = double(n * length(roots)), status = integer(1), NAOK = TRUE)   # (evecs holds NaN outside the component)
    .sharp_check(r$status)
    out <- matrix(r$out, n, length(roots), byrow = TRUE)
    if (length(roots) == 1L) out[, 1] else out
}

# per-group differential expression (DESIGN.md 27): scExp as sharp_expression_pca takes it, groups one label per cell (sort(unique())
# orders them).  method "wilcoxon" or "t-test"; reference "rest" or one of the labels (its own row is NA).  Returns the levels, the
# sizes and G x m matrices scores, pvals, pvals.adj, logfoldchanges, auc, means, means.ref, pct, pct.ref; order: G x n.genes, each
# group's genes (1-based among the kept genes) by score descending, ties to the lower gene.
sharp_rank_genes_groups <- function(scExp, groups, method = "wilcoxon", reference = "rest", normalize.total = 1e4, log1p = TRUE,
                                    genes = NULL, tie.correct = TRUE, continuity = FALSE, n.genes = NULL) {
    who <- "sharp_rank_genes_groups"
    b <- .sharp_csc_cat(scExp, who)
    if (length(groups) != sum(b$ncb)) stop(paste0(who, ": groups must hold one label per cell"))
    levels <- sort(unique(groups))
    codes <- match(groups, levels) - 1L
    G <- length(levels)
    meth <- match(method, c("wilcoxon", "t-test")) - 1L
    if (is.na(meth)) stop(paste0(who, ": method must be \"wilcoxon\" or \"t-test\""))
    ref <- if (identical(reference, "rest") && !("rest" %in% levels)) -1L else match(reference, levels) - 1L
    if (is.na(ref)) stop(paste0(who, ": reference must be \"rest\" or one of the group labels"))
    g <- if (is.null(genes)) integer(1) else .sharp_genes0(genes, b$m, who)
    mk <- if (is.null(genes)) b$m else length(g)
    no <- if (is.null(n.genes)) mk else as.integer(n.genes)
    tab <- function() double(max(G * mk, 1))
    r <- .C("sharp_C_rank_genes_csc", as.integer(b$p), as.integer(b$i), b$x, b$nb, b$ncb, b$m, as.integer(codes), G, meth, ref,
            as.double(if (is.null(normalize.total) || identical(normalize.total, FALSE)) 0 else normalize.total), as.integer(log1p), g,
            if (is.null(genes)) 0L else mk, as.integer(tie.correct), as.integer(continuity), no, sizes = double(max(G, 1)), scores = tab(),
            pvals = tab(), padj = tab(), lfc = tab(), auc = tab(), means = tab(), mref = tab(), pct = tab(), pref = tab(),
            order = integer(max(G * no, 1)), status = integer(1))
    .sharp_check(r$status)
    mat <- function(v) matrix(v, G, mk, byrow = TRUE, dimnames = list(levels, NULL))
    list(groups = levels, group.sizes = r$sizes, scores = mat(r$scores), pvals = mat(r$pvals), pvals.adj = mat(r$padj),
         logfoldchanges = mat(r$lfc), auc = mat(r$auc), means = mat(r$means), means.ref = mat(r$mref), pct = mat(r$pct), pct.ref = mat(r$pref),
         order = matrix(r$order, G, no, byrow = TRUE) + 1L, method = method, reference = reference,
         genes = if (is.null(genes)) NULL else g + 1L)
}
