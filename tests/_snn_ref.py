"""The SNN / Jaccard graph of DESIGN.md §19 (Seurat's ComputeSNN formula) written two independent ways, and the tests' case builders.

index: n x K, 0-based, self excluded, no index twice in a row.  k = K + 1, S(i) = {i} + index[i], s(i, j) = |S(i) n S(j)| for i != j,
w = (double)s / (double)(2k - s); an entry exists iff s >= 1 and w >= prune (compared in fp64); the diagonal is not stored.  Both
functions return (row_ptr int64, col int32 ascending within a row, val float64, shared int32).  Everything is an integer up to the one
division, so the GPU tests ask for equal bits."""
import functools

import numpy as np

PRUNE = 1.0 / 15.0


def weight(s, k):
    return np.asarray(s, np.float64) / (2.0 * k - np.asarray(s, np.float64))


def _csr(n, row, col, s, k):
    o = np.lexsort((col, row))
    row, col, s = row[o], col[o], s[o]
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(row, minlength=n))
    return rp, col.astype(np.int32), weight(s, k), s.astype(np.int32)


def snn_scipy(index, prune=PRUNE, chunk=4096):
    """(a) A A^T of the 0/1 matrix with k ones per row (scipy, a block of rows at a time), the diagonal removed"""
    import scipy.sparse as sp

    index = np.asarray(index, np.int64)
    n, K = index.shape
    k = K + 1
    cols = np.c_[np.arange(n), index].ravel()
    A = sp.csr_matrix((np.ones(n * k, np.int64), cols, np.arange(n + 1) * k), shape=(n, n))
    At = A.T.tocsc()
    rows, colsout, ss = [], [], []
    for r0 in range(0, n, chunk):
        P = (A[r0:r0 + chunk] @ At).tocoo()
        keep = (P.row + r0 != P.col) & (P.data >= 1) & (weight(P.data, k) >= prune)
        rows.append(P.row[keep].astype(np.int64) + r0)
        colsout.append(P.col[keep].astype(np.int64))
        ss.append(P.data[keep].astype(np.int64))
    return _csr(n, np.concatenate(rows), np.concatenate(colsout), np.concatenate(ss), k)


def snn_loop(index, prune=PRUNE):
    """(b) a plain loop over the pairs that intersects the Python sets"""
    index = np.asarray(index)
    n, K = index.shape
    k = K + 1
    S = [set(index[i].tolist()) | {i} for i in range(n)]
    row, col, ss = [], [], []
    for i in range(n):
        for j in range(i + 1, n):
            s = len(S[i] & S[j])
            if s >= 1 and float(s) / float(2 * k - s) >= prune:
                row += [i, j]
                col += [j, i]
                ss += [s, s]
    return _csr(n, np.array(row, np.int64), np.array(col, np.int64), np.array(ss, np.int64), k)


def work(index):
    """t(i) = sum over m in S(i) of |R(m)|, R(m) = {j : m in S(j)} (m itself included): the candidate increments of row i"""
    index = np.asarray(index, np.int64)
    n = index.shape[0]
    deg = 1 + np.bincount(index.ravel(), minlength=n)
    return deg + deg[index].sum(1)


def same_graph(got, want):
    """got: snn_graph()'s dict with "shared"; want: a reference tuple.  Exact: row_ptr, col, shared and the bytes of val."""
    rp, col, val, sh = want
    assert got["row_ptr"].dtype == np.int64 and got["col"].dtype == np.int32 and got["val"].dtype == np.float64
    assert got["nnz"] == int(rp[-1]) and got["n"] == rp.size - 1
    assert np.array_equal(got["row_ptr"], rp) and np.array_equal(got["col"], col)
    assert got["val"].tobytes() == val.tobytes()
    if "shared" in got:
        assert got["shared"].dtype == np.int32 and np.array_equal(got["shared"], sh)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def ring(n, K):
    """row i names i + 1 .. i + K mod n: every in-degree is k and t = k^2"""
    return ((np.arange(n)[:, None] + np.arange(1, K + 1)[None, :]) % n).astype(np.int32)


def with_hub(lists, h, rows, slot=-1):
    """the lists with the neighbour in column `slot` of the given rows replaced by h: h gains len(rows) reverse neighbours, which
    raises t of exactly the rows that name h"""
    out = np.array(lists, np.int32, copy=True)
    rows = np.asarray(rows, np.int64)
    assert not (out[rows] == h).any() and not (rows == h).any()
    out[rows, slot] = h
    return out


def hub_rows(n, K, hubs, m, first=0, spacing=None):
    """A ring of n rows in which m rows (first, first + spacing, ...; spacing 2k unless given) name the `hubs` last rows of the ring in
    their last columns.  With the spacing 2k and the rows clear of the hubs, t of each of them is k^2 + hubs * m.  Returns (lists, the
    m rows)."""
    k = K + 1
    spacing = 2 * k if spacing is None else spacing
    rows = first + spacing * np.arange(m)
    assert 1 <= hubs <= K and spacing > K and rows[-1] + 2 * k < n - hubs - 2 * k
    lists = ring(n, K)
    for c in range(hubs):
        lists = with_hub(lists, n - 1 - c, rows, K - 1 - c)
    return lists, rows


def split(total):
    """(hubs, m) with hubs * m == total, hubs <= 9 the largest such divisor"""
    hubs = max(c for c in range(1, 10) if total % c == 0)
    return hubs, total // hubs


@functools.lru_cache(maxsize=None)
def boundary_case(t):
    """K = 9 lists in which a set of rows has t exactly `t`: (lists, those rows)"""
    hubs, m = split(t - 100)
    n = 20 * m + 200
    return hub_rows(n, 9, hubs, m)


@functools.lru_cache(maxsize=None)
def blobs_lists(K=19):
    """the exact lists of the six blobs of §13 (1 500 x 10): (index, labels, X)"""
    import _umap_ref as U

    X, lab = U.blobs(1500, 10, 6, 0)
    return U.knn_lists(X, 19)[0][:, :K].astype(np.int32), lab, X


@functools.lru_cache(maxsize=None)
def gaussian_lists(K=19):
    import _umap_ref as U

    X = np.random.default_rng(1).normal(size=(2000, 50))
    return U.knn_lists(X, K)[0].astype(np.int32), X


def complete_lists(n):
    """n = K + 1: every row names every other row, every count is k"""
    return np.array([[j for j in range(n) if j != i] for i in range(n)], np.int32)


def isolated_pair_lists(n=64, K=1):
    """K = 1: rows 20 and 21 name only each other (S(20) = S(21): the one pair that prune = 1 keeps); every other row names the next
    one, so no other two rows have equal sets and rows come out empty on both sides of the pair"""
    lists = ((np.arange(n) + 1) % n).reshape(n, 1).astype(np.int32)
    lists[20, 0], lists[21, 0] = 21, 20
    return lists


def graph_csr(ref):
    return ref[0], ref[1], ref[2]
