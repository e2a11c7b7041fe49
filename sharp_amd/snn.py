"""snn_graph() and snn(): the shared-nearest-neighbour graph with Jaccard weights, the graph Seurat's FindNeighbors /
FindClusters and PhenoGraph cluster.

From k-NN lists index (n x K; self excluded): k = K + 1 is Seurat's k.param (the row itself counts), S(i) = {i} + the row's neighbours,
s(i, j) = |S(i) n S(j)| and w(i, j) = s / (2k - s) -- Seurat's ComputeSNN.  An entry exists iff s >= 1 and w >= prune (Seurat zeroes
value < prune, so a weight equal to prune stays); the diagonal is not stored.  The result is louvain_graph()'s input.  Everything the
device computes is an integer, so a call is a pure function of its arguments: two calls give the same bits.  The formula is Seurat's;
no run against Seurat is claimed.  Computed by libsharp_hip.so (csrc/snn.hip); there is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, i64, lib

__all__ = ["snn", "snn_graph"]

_MAX_N = 16777216
PRUNE = 1.0 / 15.0                                             # Seurat's prune.SNN


def _prune(prune, who):
    prune = float(prune)
    if not 0.0 <= prune <= 1.0:                                # (false for NaN too)
        raise SharpError(f"{who}: prune must be in [0, 1]")
    return prune


def _lists(index, who):
    """index as int32, n x K and C-contiguous; the refusals that need no device"""
    index = np.asarray(index)
    if index.ndim != 2:
        raise SharpError(f"{who}: index must be an n x K matrix")
    if not np.issubdtype(index.dtype, np.integer):
        raise SharpError(f"{who}: index must hold integers, not {index.dtype}")
    n, K = index.shape
    if not 2 <= n <= _MAX_N:
        raise SharpError(f"{who}: need 2 <= n <= {_MAX_N} rows")
    if not (1 <= K <= 255 and K <= n - 1):
        raise SharpError(f"{who}: need 1 <= K <= 255 neighbours per row and K <= n - 1")
    if index.dtype != np.int32:
        # an index that int32 cannot hold is out of range whatever n is: keep it so (the library names its row)
        index = np.where((index < -1) | (index > 2 ** 31 - 1), -1, index)
    return np.ascontiguousarray(index, np.int32)


def _row_caps():
    """the largest row work t of the one-wave and of the one-workgroup class (sharp_snn_row_caps; needs no device)"""
    a, b = C.c_int(), C.c_int()
    check(lib().sharp_snn_row_caps(C.byref(a), C.byref(b)))
    return a.value, b.value


def _count(index, prune):
    """(row_ptr, nnz) of the count pass alone (sharp_snn_graph with col = NULL)"""
    n, K = index.shape
    rp, nnz = np.zeros(n + 1, np.int64), C.c_longlong()
    check(lib().sharp_snn_graph(i32(index), n, int(K), prune, 0, i64(rp), None, None, None, C.byref(nnz)))
    return rp, nnz.value


def snn_graph(index, prune=PRUNE, ret_shared=False):
    """The SNN graph of neighbour lists the caller has -- what knn(X, K) and knn_descent(X, K) return: index (n x K, integers, 0-based,
    self excluded, no index twice in a row; distances are not used).  Returns {"row_ptr" (int64, n + 1), "col" (int32, strictly
    ascending within a row, no diagonal entry), "val" (float64, val[i, j] == val[j, i] bit for bit), "n", "k" (= K + 1), "nnz"}, with
    ret_shared also "shared" (int32: the s of every entry).  A row may be empty.  prune in [0, 1]: 0 keeps every pair that shares a
    neighbour, 1 only the pairs with S(i) = S(j).  Two library calls: the count, then the fill into arrays of that size."""
    who = "snn_graph"
    prune = _prune(prune, who)
    index = _lists(index, who)
    n, K = index.shape
    _lib.ensure_init()
    _, nnz = _count(index, prune)
    rp = np.zeros(n + 1, np.int64)
    col, val = np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.float64)
    sh = np.zeros(max(nnz, 1), np.int32) if ret_shared else None
    got = C.c_longlong()
    check(lib().sharp_snn_graph(i32(index), n, int(K), prune, int(nnz), i64(rp), i32(col), f64(val), i32(sh), C.byref(got)))
    out = {"row_ptr": rp, "col": col[:nnz], "val": val[:nnz], "n": n, "k": int(K) + 1, "nnz": int(nnz)}
    if ret_shared:
        out["shared"] = sh[:nnz]
    return out


def _search(X, n_neighbors, nn_method, nn_args, pca, pca_center, who, name="n_neighbors"):
    """the rows of X prepared and searched as umap() does it -> (index, distance, method); n_neighbors counts the row itself"""
    from .tsne import _nn_method, _prepare, _rows, knn, knn_descent

    method = _nn_method(nn_method, who)
    if nn_args and method != "descent":
        raise SharpError(f"{who}: nn_args belong to nn_method = \"descent\"")
    X = _rows(X)
    if X.ndim != 2:
        raise SharpError(f"{who}: X must be a matrix")
    n = X.shape[0]
    n_neighbors = int(n_neighbors)
    if not 2 <= n_neighbors <= 256:
        raise SharpError(f"{who}: {name} must be in 2 .. 256")
    if n_neighbors >= n:
        raise SharpError(f"{who}: {name} must be smaller than the number of rows")
    pca = 0 if pca is None else int(pca)
    if pca < 0:
        raise SharpError(f"{who}: pca must be None or a positive number of components")
    if not np.isfinite(X).all():
        r, c = np.argwhere(~np.isfinite(X))[0]
        raise SharpError(f"{who}: the input holds NA / NaN / Inf (row {r + 1}, column {c + 1})")
    xp = _prepare(X, pca=True, initial_dims=pca, pca_center=pca_center, pca_scale=False, normalize=False) if pca else X
    if method == "descent":
        idx, dist = knn_descent(xp, n_neighbors - 1, **dict(nn_args or {}, squared=False, ret_info=False))
    else:
        idx, dist = knn(xp, n_neighbors - 1)
    return idx, dist, method


def snn(X, k_param=20, prune=PRUNE, nn_method="exact", nn_args=None, pca=None, pca_center=True, ret_nn=False):
    """The SNN graph of the rows of X, as Seurat's FindNeighbors(k.param, prune.SNN) defines it.  The input is prepared and searched as
    louvain() does it (pca None or a number of components, centred when pca_center; nn_method "exact" or "descent", nn_args
    knn_descent()'s keywords) with K = k_param - 1 neighbours per row (k_param 2 .. 256, below n).  The result is snn_graph()'s on those
    lists, bit for bit; with ret_nn it also carries "nn": {"index", "distance"}."""
    who = "snn"
    prune = _prune(prune, who)
    idx, dist, method = _search(X, k_param, nn_method, nn_args, pca, pca_center, who, "k_param")
    out = snn_graph(idx, prune)
    if ret_nn:
        out["nn"] = {"index": idx, "distance": dist}
        if method == "descent":
            out["nn"]["method"] = "descent"
    return out
