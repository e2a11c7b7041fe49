"""dist(), hclust() and plot_markers(): the last step of the reference's workflow (SHARP -> visualization_SHARP -> get_marker_genes ->
plot_markers, R/plot_markers.R:38-242) and its small companion get_percluster_exp (R/get_percluster_exp.R:24-78).

plot_markers is not only drawing: pheatmap(cluster_rows = T, cluster_cols = T, clustering_method = "ward.D") computes
hclust(dist(sm), "ward.D") over the marker genes and hclust(dist(t(sm)), "ward.D") over up to ~10 000 cells.  Both run on the GPU here
(sharp_dist / sharp_hclust, csrc/dist.hip + the agglomeration kernels of csrc/hclust_agglo.hip behind hclust_tree of csrc/hclust.hip;
DESIGN.md 11); the selection of markers and cells is host-side numpy and runs without a device."""
import math

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, lib
from .api import HMETHODS, _dense, _is_sparse

__all__ = ["hclust", "plot_markers", "get_percluster_exp", "DIST_METHODS", "set1_colors"]

# R's own codes (its C code's enum) + "correlation" = as.dist(1 - cor(t(x))) (pheatmap's clustering_distance)
DIST_METHODS = {"euclidean": 1, "maximum": 2, "manhattan": 3, "canberra": 4, "binary": 5, "minkowski": 6, "correlation": 7}
# RColorBrewer's Set1 (brewer.pal(9, "Set1")); beyond nine clusters, where R's brewer.pal call fails, the colours repeat
set1_colors = ["#E41A1C", "#377EB8", "#4DAF4A", "#984EA3", "#FF7F00", "#FFFF33", "#A65628", "#F781BF", "#999999"]


def _dist_code(method):
    if method not in DIST_METHODS:
        raise SharpError(f"invalid distance method '{method}'")
    if method in ("canberra", "binary"):
        raise SharpError(f"dist: the \"{method}\" distance is not supported (its NA rules are out of scope)")
    return DIST_METHODS[method]


def _obs(x):
    a = np.ascontiguousarray(_dense(x), np.float64)
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 1:
        raise SharpError("x must be a matrix of at least 2 observations (rows)")
    return a


def dist(x, method="euclidean", p=2):
    """stats::dist(x, method, p = p): rows of x are observations.  Returns R's dist object as a vector of n (n - 1) / 2 doubles in R's
    order (column-wise lower triangle = scipy's pdist order).  "euclidean", "maximum", "manhattan", "minkowski" are computed from the
    differences in fp64 (duplicate rows are at distance exactly 0); "correlation" is as.dist(1 - cor(t(x))).
    (sharp_amd.dist is also the multi-GPU module of that name: the module is callable and forwards here.)"""
    code = _dist_code(method)
    a = _obs(x)
    n, d = a.shape
    if n > 46340:
        raise SharpError("dist: more than 46340 observations (the dist vector would pass 2^30 entries) is not supported")
    _lib.ensure_init()
    out = np.empty(n * (n - 1) // 2, np.float64)
    check(lib().sharp_dist(f64(a), n, d, d, code, float(p), f64(out)))
    return out


def hclust(d=None, x=None, method="ward.D", distance="euclidean", p=2):
    """stats::hclust on the GPU.  Either d (a dist vector as dist() returns it) or x (observations in rows: hclust(dist(x, distance),
    method) with the distance matrix kept in device memory).  Returns R's hclust object as a dict: merge ((n - 1, 2), observations
    negative, earlier steps positive), height (n - 1), order (n, 1-based leaves from left to right), method, dist_method, n."""
    if method not in HMETHODS:
        raise SharpError(f"invalid clustering method '{method}'")
    if (d is None) == (x is None):
        raise SharpError("hclust: give either d (a dist vector) or x (observations)")
    if d is not None:
        dv = np.ascontiguousarray(d, np.float64).ravel()
        n = int(round((1 + math.sqrt(1 + 8 * dv.size)) / 2))
        if n < 2 or n * (n - 1) // 2 != dv.size:
            raise SharpError("hclust: d is not a dist vector (its length is not n (n - 1) / 2)")
        dist_method = None
    else:
        code = _dist_code(distance)
        a = _obs(x)
        n = a.shape[0]
        dist_method = distance
    _lib.ensure_init()
    merge = np.zeros((2, n - 1), np.int32)
    height = np.zeros(n - 1)
    order = np.zeros(n, np.int32)
    if d is not None:
        check(lib().sharp_hclust_dist(f64(dv), n, HMETHODS[method], i32(merge), f64(height), i32(order)))
    else:
        check(lib().sharp_hclust(f64(a), n, a.shape[1], a.shape[1], code, float(p), HMETHODS[method], i32(merge), f64(height),
                                 i32(order)))
    return {"merge": merge.T.copy(), "height": height, "order": order, "method": method, "dist_method": dist_method, "n": n}


# ---- get_percluster_exp (R/get_percluster_exp.R:24-78): host-side regrouping ------------------------------------------------------------
def get_percluster_exp(scExp, y, n_cores=None):
    """scExp: the LIST of (genes, cells) blocks SHARP_unlimited clustered (dense arrays or scipy sparse); y: its result (or the labels).
    Returns a list with one (genes, cells of the cluster) matrix per cluster, cluster j being the j-th of sort(unique(pred_clusters)),
    columns in block order and then cell order; sparse when every contributing block is; None for a cluster absent from every block
    (labels given for more cells than the blocks hold).  n_cores is accepted and ignored."""
    label = np.asarray(y["pred_clusters"] if isinstance(y, dict) else y).ravel()
    lens = [b.shape[1] for b in scExp]
    if sum(lens) > label.size:
        raise SharpError("get_percluster_exp: the blocks hold more cells than there are labels")
    uy = np.unique(label)
    xx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = []
    for u in uy:
        parts = []
        for k, b in enumerate(scExp):
            idx = np.flatnonzero(label[xx[k]:xx[k + 1]] == u)
            if idx.size:
                parts.append(b.tocsc()[:, idx] if _is_sparse(b) else np.asarray(b)[:, idx])
        if not parts:
            out.append(None)
        elif all(_is_sparse(q) for q in parts):
            import scipy.sparse as sp

            out.append(sp.hstack(parts, format="csc"))
        else:
            out.append(np.hstack([_dense(q) for q in parts]))
    return out


# ---- plot_markers (R/plot_markers.R:38-242) -----------------------------------------------------------------------------------------
def _rank_average(v):
    """R's rank(): average ranks for ties"""
    v = np.asarray(v, np.float64)
    o = np.argsort(v, kind="stable")
    r = np.empty(v.size)
    s = v[o]
    i = 0
    while i < s.size:
        j = i
        while j + 1 < s.size and s[j + 1] == s[i]:
            j += 1
        r[o[i:j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return r


def _plot_markers_select(sginfo, label=None, N_marker=10, sN_cluster=None, nratio=None, logmark=None):
    """The host part of plot_markers, R/plot_markers.R:46-151 (no device needed): returns sortmarker (the whole table, :61), sm (the
    z-scored markers x cells matrix pheatmap receives), genes (its rows), cells (0-based indices of its columns in `label`), newc (their
    labels) and ncells (length(cellind), which decides the file type)."""
    if label is None:
        label = sginfo["label"]
    label = np.asarray(label).ravel()
    if nratio is None:
        nratio = 1e4 / label.size                                              # :50-52 (only used above 10 000 cells, where it is < 1)
    elif not (nratio > 0 and nratio <= 1):
        raise SharpError("plot_markers: nratio must be in (0, 1] (R would index with NA)")
    mg = sginfo["mginfo"]
    icl = np.asarray(mg["icluster"])
    # :61 order(icluster, -rank(auc), pvalue) on the table already ordered by (icluster, pvalue) (:57); both orders are stable
    o1 = np.lexsort((np.asarray(mg["pvalue"]), icl))
    o2 = np.lexsort((np.asarray(mg["pvalue"])[o1], -_rank_average(np.asarray(mg["auc"])[o1]), icl[o1]))
    rows = o1[o2]
    sortmarker = {k: np.asarray(v)[rows] for k, v in mg.items()}
    ucl = np.unique(icl)
    if sN_cluster is None:
        sN_cluster = ucl.size                                                   # :71-73
    sN_cluster = int(sN_cluster)
    if sN_cluster < 1 or sN_cluster > ucl.size:
        raise SharpError("plot_markers: sN.cluster must be between 1 and the number of clusters with markers")
    kk = ucl[:sN_cluster]                                                       # :75
    pick = np.concatenate([np.flatnonzero(sortmarker["icluster"] == c)[:int(N_marker)] for c in kk])   # :91-95
    cellind = np.argsort(label, kind="stable")                                  # :105 order(cc)
    newc = label[cellind]
    mat = _dense(sginfo["mat"])
    sm = mat[rows[pick]][:, cellind]                                            # :129-130
    scind = np.flatnonzero(np.isin(newc, kk))                                   # :132-134
    cells, newc, sm = cellind[scind], newc[scind], sm[:, scind]
    if cellind.size > 1e4:                                                      # :136-143: the first ceiling(count * nratio) cells per cluster
        ki = np.concatenate([np.flatnonzero(newc == u)[:int(math.ceil(np.count_nonzero(newc == u) * nratio))] for u in np.unique(newc)])
        cells, newc, sm = cells[ki], newc[ki], sm[:, ki]
    if logmark is None:
        logmark = sginfo.get("logmark")
    if logmark is None:
        raise SharpError("plot_markers: neither the logmark argument nor sginfo[\"logmark\"] is given (log2(x + 1) or not?)")
    my = np.log2(sm + 1) if logmark else np.array(sm, np.float64)               # :146-148
    sd = my.std(1, ddof=1) if my.shape[1] > 1 else np.zeros(my.shape[0])
    keep = sd != 0                                                              # :149
    my = my[keep]
    my = (my - my.mean(1, keepdims=True)) / my.std(1, ddof=1, keepdims=True)    # :150 t(scale(t(my)))
    genes = np.asarray(sortmarker["gene"])[pick][keep]
    return {"sortmarker": sortmarker, "sm": np.ascontiguousarray(my), "genes": genes, "cells": cells, "newc": newc,
            "ncells": int(cellind.size)}


def _dendrogram_segments(tree):
    """line segments ((x0, y0), (x1, y1)) of the dendrogram of an hclust dict, leaves at x = 0.5, 1.5, ... in `order`"""
    n = tree["n"]
    pos = np.empty(n + 1)
    pos[np.asarray(tree["order"])] = np.arange(n) + 0.5
    cx, cy, segs = np.zeros(n), np.zeros(n), []
    for i in range(n - 1):
        pts = []
        for v in tree["merge"][i]:
            pts.append((pos[-v], 0.0) if v < 0 else (cx[v], cy[v]))
        h = float(tree["height"][i])
        (xa, ya), (xb, yb) = pts
        segs += [((xa, ya), (xa, h)), ((xa, h), (xb, h)), ((xb, h), (xb, yb))]
        cx[i + 1], cy[i + 1] = (xa + xb) / 2, h
    return segs


def _draw_markers_heatmap(sm, genes, newc, row_tree, col_tree, filename, filetype, width=900, height=900):
    """the heat map pheatmap draws at R/plot_markers.R:214-237, with matplotlib's Agg canvas (pyplot's state is left alone): rows and
    columns in dendrogram order, blue-white-red in 400 steps over [min, max], both dendrograms, a Set1 cluster bar, gene names"""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.collections import LineCollection
    from matplotlib.colors import LinearSegmentedColormap, ListedColormap
    from matplotlib.figure import Figure

    ro, co = np.asarray(row_tree["order"]) - 1, np.asarray(col_tree["order"]) - 1
    fig = Figure(figsize=(7, 7) if filetype == "pdf" else (width / 100.0, height / 100.0), dpi=100)
    FigureCanvasAgg(fig)
    gs = fig.add_gridspec(3, 3, width_ratios=[0.12, 1, 0.05], height_ratios=[0.15, 0.03, 1], wspace=0.01, hspace=0.01,
                          left=0.02, right=0.9, top=0.98, bottom=0.03)
    ax = fig.add_subplot(gs[2, 1])
    cmap = LinearSegmentedColormap.from_list("bwr400", ["blue", "white", "red"], N=400)
    im = ax.imshow(sm[ro][:, co], aspect="auto", cmap=cmap, vmin=float(sm.min()), vmax=float(sm.max()), interpolation="nearest",
                   extent=(0, co.size, ro.size, 0))
    ax.set_xticks([])
    ax.yaxis.tick_right()
    ax.set_yticks(np.arange(ro.size) + 0.5)
    ax.set_yticklabels([str(g) for g in np.asarray(genes)[ro]], fontsize=max(3, min(12, 500 // max(ro.size, 1))))
    at = fig.add_subplot(gs[0, 1])
    at.add_collection(LineCollection(_dendrogram_segments(col_tree), colors="black", linewidths=0.4))
    at.set_xlim(0, co.size)
    at.set_ylim(0, float(np.max(col_tree["height"])) * 1.02 or 1.0)
    at.axis("off")
    al = fig.add_subplot(gs[2, 0])
    al.add_collection(LineCollection([((y0, x0), (y1, x1)) for (x0, y0), (x1, y1) in _dendrogram_segments(row_tree)], colors="black",
                                     linewidths=0.4))
    al.set_ylim(ro.size, 0)
    al.set_xlim(float(np.max(row_tree["height"])) * 1.02 or 1.0, 0)
    al.axis("off")
    ab = fig.add_subplot(gs[1, 1])
    uc = np.unique(newc)
    ab.imshow(np.searchsorted(uc, np.asarray(newc)[co])[None, :] % len(set1_colors), aspect="auto", cmap=ListedColormap(set1_colors),
              vmin=-0.5, vmax=len(set1_colors) - 0.5, interpolation="nearest")
    ab.axis("off")
    fig.colorbar(im, cax=fig.add_subplot(gs[0, 2]))
    fig.savefig(filename, format=filetype)


def plot_markers(sginfo, label=None, N_marker=10, sN_cluster=None, filename=None, filetype=None, nratio=None, n_cores=None, width=900,
                 height=900, logmark=None, plot=True, clustering_distance="euclidean", clustering_method="ward.D"):
    """R/plot_markers.R:38-242.  sginfo: what get_marker_genes returned.  The markers x cells matrix sm (top N_marker markers of the first
    sN_cluster clusters; above 10 000 cells the first ceiling(count * nratio) cells of each cluster; log2(x + 1) when logmark; rows
    z-scored) is clustered both ways on the GPU -- row_tree = hclust(x = sm), col_tree = hclust(x = t(sm)), as pheatmap does with
    clustering_method = "ward.D" -- and drawn in dendrogram order (pdf below 5 000 cells, png otherwise; markers_heatmap.<type>).
    Returns {"sortmarker" (R's return value), "sm", "genes", "cells", "row_tree", "col_tree", "filename"}."""
    s = _plot_markers_select(sginfo, label, N_marker, sN_cluster, nratio, logmark)
    sm = s["sm"]
    if sm.shape[1] > 16384:
        raise SharpError(f"plot_markers: {sm.shape[1]} cells selected, more than the 16384 one clustering holds: give a smaller nratio")
    if sm.shape[0] < 2 or sm.shape[1] < 2:
        raise SharpError("plot_markers: fewer than 2 marker genes or cells left to cluster")
    _lib.ensure_init()
    row_tree = hclust(x=sm, method=clustering_method, distance=clustering_distance)
    col_tree = hclust(x=np.ascontiguousarray(sm.T), method=clustering_method, distance=clustering_distance)
    if filetype is None:
        filetype = "pdf" if s["ncells"] < 5000 else "png"                       # :184-190
    if filename is None:
        filename = f"markers_heatmap.{filetype}"                                # :193-195
    if plot:
        _draw_markers_heatmap(sm, s["genes"], s["newc"], row_tree, col_tree, filename, filetype, width, height)
    return {"sortmarker": s["sortmarker"], "sm": sm, "genes": s["genes"], "cells": s["cells"], "row_tree": row_tree,
            "col_tree": col_tree, "filename": filename if plot else None}
