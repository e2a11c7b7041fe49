"""trustworthiness(), continuity(), neighbor_ranks() and knn_recall(): whether a map is any good.

validity.py scores a labelling; these score a map Y of the rows of X.  Trustworthiness (Venna and Kaski; sklearn.manifold.trustworthiness)
punishes rows that are close in the map and far in the input, continuity the reverse.  Both come from one question -- where do the K rows
a list names stand among ALL rows, ordered by distance? -- which csrc/neighbor_rank.hip answers without an n x n matrix: one O(n^2 d) pass
over the pairs, so the scores can be had at the sizes the maps are built for.  Distances are knn()'s (the direct sum in column order,
ties to the lower index), everything the device counts is an integer, and two calls give the same bits."""
import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, lib
from .tsne import _rows, knn

__all__ = ["neighbor_ranks", "trustworthiness", "continuity", "knn_recall"]


def _index(index, n, who):
    """an n x K int32 index matrix from a matrix or knn()'s (index, distance) pair; refusals that need no device"""
    if isinstance(index, dict):
        index = index["index"]
    elif isinstance(index, (tuple, list)) and len(index) == 2 and np.ndim(index[0]) == 2:
        index = index[0]
    a = np.asarray(index)
    if a.ndim != 2:
        raise SharpError(f"{who}: the neighbour lists must be an n x K index matrix (or the (index, distance) pair knn() returns)")
    if not np.issubdtype(a.dtype, np.integer):
        raise SharpError(f"{who}: the neighbour index must hold integers, not {a.dtype}")
    if a.shape[0] != n:
        raise SharpError(f"{who}: the neighbour lists have {a.shape[0]} rows, the data {n}")
    K = a.shape[1]
    if K < 1:
        raise SharpError(f"{who}: need at least one neighbour per row (K >= 1)")
    if K > 255:
        raise SharpError(f"{who}: at most 255 neighbours per row")
    if K > n - 1:
        raise SharpError(f"{who}: K neighbours per row need K <= n - 1")
    if a.dtype != np.int32:
        # an index that int32 cannot hold is out of range whatever n is: keep it so (the library names its row)
        a = np.where((a < 0) | (a > np.iinfo(np.int32).max), -1, a)
    return np.ascontiguousarray(a, np.int32)


def _data(X, who):
    X = _rows(X)
    if X.shape[0] < 3 or X.shape[1] < 1:
        raise SharpError(f"{who}: need n >= 3 rows of d >= 1 values")
    if X.shape[0] > 16777216:
        raise SharpError(f"{who}: more than 16777216 rows is not supported")
    bad = ~(np.abs(X) <= 1e100)                                                     # (true for NaN too)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise SharpError(f"{who}: the input holds NA / NaN / Inf or a value beyond 1e100 (row {r + 1}, column {c + 1})")
    return X


def neighbor_ranks(X, index, max_rows_per_launch=0):
    """Where the rows a list names stand among all rows.  X: n x d; index: n x K, 0-based, each row K other rows (knn()'s list format:
    every entry in [0, n), no row naming itself, no index twice in a row).  Returns (n, K) int32:
    rank[i, k] = 1 + #{ l != i : (d2(i, l), l) < (d2(i, j), j) }, j = index[i, k], with d2 the squared distance knn(X, K, squared=True)
    gives the pair, bit for bit, and ties going to the lower index: 1 .. n - 1, and neighbor_ranks(X, knn(X, K)[0]) is 1 .. K in every
    row.  3 <= n <= 16777216, 1 <= K <= 255, K <= n - 1, |x| <= 1e100.  max_rows_per_launch: 0 = by the library's pair budget."""
    X = _data(X, "neighbor_ranks")
    n, d = X.shape
    index = _index(index, n, "neighbor_ranks")
    if int(max_rows_per_launch) < 0:
        raise SharpError("neighbor_ranks: max_rows_per_launch must be >= 0")
    _lib.ensure_init()
    out = np.zeros(index.shape, np.int32)
    check(lib().sharp_neighbor_ranks(f64(X), n, d, d, index.shape[1], i32(index), int(max_rows_per_launch), i32(out)))
    return out


def _score(ranked, listed, n_neighbors, neighbors, ret_points, who):
    """ranks in `ranked` of the K nearest rows in `listed` (or of the given lists of `listed`) -> the score"""
    ranked = _data(ranked, who)
    n = ranked.shape[0]
    if neighbors is None:
        K = int(n_neighbors)
        if K < 1:
            raise SharpError(f"{who}: n_neighbors must be at least 1")
    else:
        neighbors = _index(neighbors, n, who)
        K = neighbors.shape[1]
    if K >= n / 2:
        raise SharpError(f"n_neighbors ({K}) should be less than n_samples / 2 ({n / 2})")            # (sklearn's wording)
    if K > 255:
        raise SharpError(f"{who}: at most 255 neighbours per row")
    if neighbors is None:
        neighbors = knn(_data(listed, who), K)[0]
    rank = neighbor_ranks(ranked, neighbors)
    penalty = np.maximum(rank.astype(np.int64) - K, 0).sum(axis=1)
    norm = K * (2 * n - 3 * K - 1)
    score = 1.0 - float(int(penalty.sum())) * (2.0 / (n * norm))   # from the integer total, not the mean of the rows' values
    if not ret_points:
        return score
    return {"score": score, "points": 1.0 - 2.0 / norm * penalty, "penalty": penalty, "n_neighbors": K}


def _same_rows(X, Y, who):
    nx, ny = np.shape(X)[0] if np.ndim(X) == 2 else -1, np.shape(Y)[0] if np.ndim(Y) == 2 else -1
    if nx < 0 or ny < 0:
        raise SharpError(f"{who}: X and Y must be matrices (rows = observations)")
    if nx != ny:
        raise SharpError(f"{who}: X has {nx} rows and Y {ny}: a map has one row per row of X")


def trustworthiness(X, Y, n_neighbors=5, neighbors=None, ret_points=False):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=5) (Euclidean) on the GPU, without its two n x n matrices:
    1 - 2 / (n K (2n - 3K - 1)) * sum_i sum_k max(0, rank_X(i, j_ik) - K), j_ik the K nearest rows of row i in the map Y, rank_X their
    ranks among all rows in X (neighbor_ranks).  neighbors: Y's lists, if they are at hand (an index matrix or knn()'s (index, distance)
    pair; their width is then K) -- otherwise knn(Y, n_neighbors).  Returns the score; with ret_points a dict: score, points (the
    per-row values 1 - 2 / (K (2n - 3K - 1)) * penalty), penalty (int64 per row), n_neighbors.  K >= n / 2 is refused as in sklearn."""
    _same_rows(X, Y, "trustworthiness")
    return _score(X, Y, n_neighbors, neighbors, ret_points, "trustworthiness")


def continuity(X, Y, n_neighbors=5, neighbors=None, ret_points=False):
    """trustworthiness with the roles swapped: the ranks in the map Y of each row's K nearest rows in X.  neighbors: X's lists -- what
    umap(..., ret_nn=True)["nn"] and visualization_SHARP(..., return_neighbors=True) hand back, so the continuity of a finished map
    costs one rank pass at d = 2 and no second k-NN."""
    _same_rows(X, Y, "continuity")
    return _score(Y, X, n_neighbors, neighbors, ret_points, "continuity")


def knn_recall(index, index_true):
    """The mean share of each row's true neighbours (index_true, n x K_true) that the row of index (n x K) holds: 1.0 when every list
    holds all of them.  Host numpy, no device.  The widths may differ and the comparison is by set: no order, no leading columns
    are assumed."""
    a, t = np.asarray(index), np.asarray(index_true)
    if a.ndim != 2 or t.ndim != 2 or a.shape[0] != t.shape[0]:
        raise SharpError("knn_recall: index and index_true must be matrices with the same number of rows")
    if a.shape[1] < 1 or t.shape[1] < 1 or a.shape[0] < 1:
        raise SharpError("knn_recall: empty lists")
    if not (np.issubdtype(a.dtype, np.integer) and np.issubdtype(t.dtype, np.integer)):
        raise SharpError("knn_recall: the lists must hold integers")
    a, t = np.sort(a.astype(np.int64), axis=1), t.astype(np.int64)
    # membership of t's entries in a's sorted rows: one searchsorted over row-offset keys
    span = int(max(a.max(), t.max())) - int(min(a.min(), t.min())) + 1
    lo = int(min(a.min(), t.min()))
    off = np.arange(a.shape[0], dtype=np.int64)[:, None] * span
    ka, kt = (a - lo + off).ravel(), (t - lo + off).ravel()
    p = np.searchsorted(ka, kt)
    hit = ka[np.minimum(p, ka.size - 1)] == kt
    return float(hit.mean())
