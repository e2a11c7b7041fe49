"""cutree(), silhouette() and calinski_harabasz(): what is done with a tree and with a labelling.

The reference cuts every tree it builds (cutree(h, k = ...), cutree(h, h = ...): R/get_opt_hclust.R:101,132,207) and scores the cuts with
cluster::silhouette and the Calinski-Harabasz index (R/get_opt_hclust.R:103-105,134-144).  Inside get_opt_hclust those steps are fused into
its kernels and only a median / a value per level leaves the device; here they are functions of their own: cutree on the dict hclust()
returns (host only, no device needed), silhouette on a dist vector or -- matrix-free, for any number of cells -- on the observations
themselves (csrc/validity.hip), and the Calinski-Harabasz index in its Euclidean and "1-corr" forms."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, lib
from .api import _dense
from .tree import _dist_code

__all__ = ["cutree", "silhouette", "calinski_harabasz"]


def cutree(tree, k=None, h=None):
    """stats::cutree(tree, k, h) on the dict hclust() returns.  k (numbers of clusters) or h (heights), each a scalar or a sequence; k
    wins when both are given.  A scalar gives an int32 vector of n labels, a sequence an (n, len) matrix with one column per value in
    the order given.  Labels are 1-based and numbered by first appearance in observation order (observation 1 is in cluster 1).
    h needs increasing heights (centroid / median trees can have inversions: R's error); k works on every tree."""
    if k is None and h is None:
        raise SharpError("either 'k' or 'h' must be specified")
    merge = np.asarray(tree["merge"])
    n = merge.shape[0] + 1
    if merge.ndim != 2 or merge.shape[1] != 2 or n < 2:
        raise SharpError("invalid 'tree' ('merge' component)")
    if k is None:
        height = np.asarray(tree["height"], np.float64)
        if np.any(np.diff(height) < 0):
            raise SharpError("the 'height' component of 'tree' is not sorted (increasingly)")
        scalar = np.ndim(h) == 0
        hv = np.atleast_1d(np.asarray(h, np.float64))
        # k <- n + 1L - apply(outer(c(tree$height, Inf), h, `>`), 2, which.max)
        kv = n + 1 - (np.argmax(np.append(height, np.inf)[:, None] > hv[None, :], axis=0) + 1)
    else:
        scalar = np.ndim(k) == 0
        kv = np.atleast_1d(np.asarray(k))
        if kv.size and not np.all(kv == np.floor(kv)):
            kv = np.floor(kv)                                                       # as.integer(k)
    if kv.size == 0:
        raise SharpError("either 'k' or 'h' must be specified")
    if np.any(kv < 1) or np.any(kv > n):
        raise SharpError(f"elements of 'k' must be between 1 and {n}")
    kv = np.ascontiguousarray(kv, np.int32)
    mcol = np.ascontiguousarray(merge.T, np.int32)                                  # (n - 1) x 2 column-major, as sharp_hclust writes it
    out = np.zeros((kv.size, n), np.int32)
    check(lib().sharp_cutree(i32(mcol), n, i32(kv), int(kv.size), i32(out)))       # (no device context needed)
    return out[0].copy() if scalar else np.ascontiguousarray(out.T)


def _codes(x, who):
    """R's factor(): the distinct labels in sorted order -> codes 1 .. k.  Returns (codes int32, levels)"""
    if isinstance(x, dict):
        x = x["pred_clusters"]
    lab = np.asarray(x).ravel()
    if lab.dtype.kind == "f":
        if not (np.all(np.isfinite(lab)) and np.all(lab == np.round(lab))):
            raise SharpError("'x' must only have integer codes")
    elif lab.dtype.kind not in "iub":
        raise SharpError("'x' must only have integer codes")
    levels, inv = np.unique(lab, return_inverse=True)
    return np.ascontiguousarray(inv.ravel() + 1, np.int32), levels


def silhouette(x, d=None, data=None, distance="euclidean", p=2):
    """cluster::silhouette(x, dist).  x: integer labels, or a SHARP* result (then its pred_clusters).  Exactly one of d (a dist vector
    as dist() returns it, at most 46340 observations) and data (observations in rows; matrix-free: no n x n matrix is built, any number
    of cells up to 16777216).  distance / p as in dist() (with data only).

    Returns a dict with R's columns and summary: cluster, neighbor (both in the caller's label codes), sil_width, clus_sizes,
    clus_avg_widths (per distinct label in sorted order, `clusters`), avg_width.  Labels need not be 1 .. k.  As in sildist(): a(i) is
    the mean over the n_c - 1 other members, b(i) the smallest mean over another cluster (the first one in sorted label order on an
    exact tie), the width (b - a) / max(a, b), 0 when a == b and for a cell alone in its cluster.  Two calls on the same input give
    bitwise the same widths.

    With fewer than 2 clusters or more than n - 1, where R returns NA, this returns None."""
    if (d is None) == (data is None):
        raise SharpError("silhouette: give either d (a dist vector) or data (observations in rows)")
    cl, levels = _codes(x, "silhouette")
    n, k = cl.size, levels.size
    if d is not None:
        dv = np.asarray(d)
        nd = int(round((1 + math.sqrt(1 + 8 * dv.size)) / 2))
        if dv.ndim != 1 or nd * (nd - 1) // 2 != dv.size:
            raise SharpError("silhouette: d is not a dist vector (its length is not n (n - 1) / 2)")
        if nd > 46340:
            raise SharpError("silhouette: a dist vector of more than 46340 observations is not supported: give the observations "
                             "themselves (data=), which needs no n x n matrix")
        if nd != n:
            raise SharpError("clustering 'x' and dissimilarity 'dist' are incompatible")
        dv = np.ascontiguousarray(dv, np.float64)
        if not np.all(np.isfinite(dv)):
            raise SharpError("silhouette: d holds NA / NaN / Inf")
    else:
        code = _dist_code(distance)
        a = np.ascontiguousarray(_dense(data), np.float64)
        if a.ndim != 2 or a.shape[1] < 1:
            raise SharpError("silhouette: data must be a matrix of observations (rows)")
        if a.shape[0] != n:
            raise SharpError("silhouette: the number of labels differs from the number of observations (rows of data)")
        if not np.all(np.isfinite(a)):
            raise SharpError("silhouette: data holds NA / NaN / Inf")
    if k < 2 or k > n - 1:
        return None
    _lib.ensure_init()
    neighbor = np.zeros(n, np.int32)
    width = np.zeros(n, np.float64)
    if d is not None:
        check(lib().sharp_silhouette_dist(f64(dv), n, i32(cl), k, i32(neighbor), f64(width)))
    else:
        check(lib().sharp_silhouette(f64(a), n, a.shape[1], a.shape[1], code, float(p), i32(cl), k, i32(neighbor), f64(width)))
    sizes = np.bincount(cl - 1, minlength=k)
    return {"cluster": levels[cl - 1], "neighbor": levels[neighbor - 1], "sil_width": width, "clusters": levels, "clus_sizes": sizes,
            "clus_avg_widths": np.bincount(cl - 1, weights=width, minlength=k) / sizes, "avg_width": float(width.mean())}


def calinski_harabasz(data, labels, distance="euclidean"):
    """The Calinski-Harabasz index [B / (k - 1)] / [W / (n - k)] of a labelling of the rows of data.  distance = "euclidean":
    clusterCrit::intCriteria(data, labels, "Calinski_Harabasz"), squared Euclidean between / within sums (= sklearn's
    calinski_harabasz_score); "1-corr": clues::get_CH(data, labels, disMethod = "1-corr"), both sums over (1 - Pearson correlation)^2
    (R/get_opt_hclust.R:105,144).  labels as in silhouette().  A within sum of exactly 0 gives inf, as in R."""
    kinds = {"euclidean": 0, "1-corr": 1}
    if distance not in kinds:
        raise SharpError(f"calinski_harabasz: distance must be \"euclidean\" or \"1-corr\", not '{distance}'")
    cl, levels = _codes(labels, "calinski_harabasz")
    a = np.ascontiguousarray(_dense(data), np.float64)
    if a.ndim != 2 or a.shape[1] < 1:
        raise SharpError("calinski_harabasz: data must be a matrix of observations (rows)")
    n, k = a.shape[0], levels.size
    if cl.size != n:
        raise SharpError("calinski_harabasz: the number of labels differs from the number of observations (rows of data)")
    if not np.all(np.isfinite(a)):
        raise SharpError("calinski_harabasz: data holds NA / NaN / Inf")
    if k < 2 or k > n - 1:
        raise SharpError("calinski_harabasz: the number of clusters must be between 2 and n - 1")
    _lib.ensure_init()
    out = C.c_double()
    check(lib().sharp_calinski_harabasz(f64(a), n, a.shape[1], a.shape[1], i32(cl), k, kinds[distance], C.byref(out)))
    return out.value
