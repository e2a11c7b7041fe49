"""Neighbour ranks, trustworthiness and continuity of DESIGN.md §17 in numpy fp64: the specification the GPU tests compare
libsharp_hip.so with, entry for entry.  Every distance is the direct sum s = 0; s += (x_ic - x_lc)^2 for c = 0 .. d-1 (a column loop:
no einsum, no GEMM), rows are ordered by (distance, index), and the scores are formed from the integer penalty total."""
import numpy as np


# ---- inputs the tests share -----------------------------------------------------------------------------------------------------------
def blobs(n, d, seed, centres=6):
    """tests/_knn_descent_ref.py's blobs: six Gaussian blobs of sigma 1 with centres N(0, 6^2)"""
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(centres, d)) * 6.0
    return np.ascontiguousarray(mu[rng.integers(0, centres, size=n)] + rng.normal(size=(n, d)))


def gaussian(n, d, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).normal(size=(n, d)))


def lattice(n=257, d=3, levels=4, seed=7):
    """integers 0 .. levels - 1: at most levels^d distinct rows, so most rows copy an earlier one and every row sees many exact ties"""
    return np.ascontiguousarray(np.random.default_rng(seed).integers(0, levels, size=(n, d)).astype(np.float64))


def map_of(X, seed, noise=0.5):
    """a stand-in for a map: the first two columns plus Gaussian noise"""
    return np.ascontiguousarray(X[:, :2] + noise * np.random.default_rng(seed).normal(size=(X.shape[0], 2)))


def random_lists(n, K, seed):
    """well-formed lists that know nothing of X: K distinct rows other than the row itself"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, K), np.int32)
    for i in range(n):
        c = rng.choice(n - 1, size=K, replace=False)
        out[i] = c + (c >= i)
    return out


def random_lists_large(n, K, seed):
    """random_lists for many rows and K far below n: drawn for all rows at once, rows with a repeated index drawn again"""
    rng = np.random.default_rng(seed)
    own = np.arange(n)[:, None]
    c = rng.integers(0, n - 1, size=(n, K))
    while True:
        s = np.sort(c, axis=1)
        again = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
        if again.size == 0:
            return (c + (c >= own)).astype(np.int32)
        c[again] = rng.integers(0, n - 1, size=(again.size, K))


# the three tie-free cases of the comparison with sklearn: (name, X, K)
def sklearn_cases():
    return [("blobs 1025 x 10", blobs(1025, 10, 1), 15), ("gaussian 1025 x 50", gaussian(1025, 50, 2), 5),
            ("gaussian 257 x 3", gaussian(257, 3, 4), 90)]


# ---- distances, orders, ranks ---------------------------------------------------------------------------------------------------------
def d2_rows(X, rows):
    """squared distances of the given rows to every row, column after column: (len(rows), n)"""
    rows = np.asarray(rows, np.int64)
    s = np.zeros((rows.size, X.shape[0]))
    for c in range(X.shape[1]):
        col = X[:, c]
        t = col[rows][:, None] - col[None, :]
        s += t * t
    return s


def _places(X, rows):
    """place[r, l]: the position of row l in the (distance, index) order of ALL rows seen from rows[r] (row rows[r] itself included,
    at whatever place its distance 0 and its index give it)"""
    D = d2_rows(X, rows)
    order = np.argsort(D, axis=1, kind="stable")                  # (the columns ascend: equal distances stay by the lower index)
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(X.shape[0]), order.shape), axis=1)
    return D, place


def ranks(X, index, rows=None, chunk=1024):
    """rank[r, k] = 1 + #{ l != i : (d2(i, l), l) < (d2(i, j), j) }, i = rows[r], j = index[i, k]; rows None: every row"""
    index = np.asarray(index, np.int64)
    rows = np.arange(X.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    out = np.empty((rows.size, index.shape[1]), np.int32)
    for a in range(0, rows.size, chunk):
        rr = rows[a:a + chunk]
        _, place = _places(X, rr)
        pj = np.take_along_axis(place, index[rr], axis=1)
        pi = place[np.arange(rr.size), rr][:, None]
        out[a:a + chunk] = pj + 1 - (pi < pj)                      # row i itself never counts
    return out


def knn_lists(X, K, chunk=1024):
    """the K nearest other rows of every row by (distance, index): (n, K) int32"""
    n = X.shape[0]
    out = np.empty((n, K), np.int32)
    for a in range(0, n, chunk):
        rr = np.arange(a, min(n, a + chunk))
        D = d2_rows(X, rr)
        D[np.arange(rr.size), rr] = np.inf                         # (behind every finite distance: |x| <= 1e100)
        out[a:a + chunk] = np.argsort(D, axis=1, kind="stable")[:, :K]
    return out


def min_relative_gap(X, chunk=1024):
    """the smallest (b - a) / b over consecutive distances a <= b from a row to the other rows"""
    n, g = X.shape[0], np.inf
    for a in range(0, n, chunk):
        rr = np.arange(a, min(n, a + chunk))
        D = d2_rows(X, rr)
        D[np.arange(rr.size), rr] = -1.0
        D = np.sort(D, axis=1)[:, 1:]
        g = min(g, float(((D[:, 1:] - D[:, :-1]) / D[:, 1:]).min()))
    return g


# ---- scores ---------------------------------------------------------------------------------------------------------------------------
def penalties(rank, K):
    return np.maximum(np.asarray(rank, np.int64) - K, 0).sum(axis=1)


def score(penalty, n, K):
    """1 - 2 / (n K (2n - 3K - 1)) * sum of the penalties, from the integer total"""
    return 1.0 - float(int(np.asarray(penalty, np.int64).sum())) * (2.0 / (n * K * (2.0 * n - 3.0 * K - 1.0)))


def points(penalty, n, K):
    return 1.0 - 2.0 / (K * (2 * n - 3 * K - 1)) * np.asarray(penalty, np.int64)


def trustworthiness(X, Y, K, lists=None):
    """(score, penalty per row); lists: Y's lists where they are given"""
    lists = knn_lists(Y, K) if lists is None else lists
    pen = penalties(ranks(X, lists), K)
    return score(pen, X.shape[0], K), pen


def continuity(X, Y, K, lists=None):
    return trustworthiness(Y, X, K, lists)
