"""numpy helpers for t-SNE from given distances or given neighbours (DESIGN.md §10 "Given neighbours, given distances"), on top of
tests/_tsne_ref.py.  Test infrastructure only: the product never imports it."""
import numpy as np

import _tsne_ref as ref


def knn_from_dist(D, K):
    """the K nearest objects of each from the full distance matrix D: a stable argsort of every row with self removed, so ties go to
    the lower index; returns (idx (n, K), D[i, idx])"""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    M = D.copy()
    M[np.arange(n), np.arange(n)] = np.inf
    o = np.argsort(M, axis=1, kind="stable")[:, :K]
    return o, np.take_along_axis(D, o, 1)


def joint_p_from_neighbours(idx, dist2, perplexity):
    """P = (P_cond + P_cond^T) / sum as a scipy CSR matrix (rows sorted by column) from neighbour lists and their squared distances:
    ref.calibrate plus the symmetrisation of ref.joint_p"""
    import scipy.sparse as sp

    idx = np.asarray(idx)
    n, K = idx.shape
    Pc = ref.calibrate(np.asarray(dist2, np.float64), perplexity)
    M = sp.csr_matrix((Pc.ravel(), (np.repeat(np.arange(n), K), idx.ravel())), shape=(n, n))
    S = (M + M.T).tocsr()
    S.sort_indices()
    return S / S.sum()


def square_form(d, n):
    """the full symmetric matrix of R's dist vector (column-wise lower triangle = row-wise upper triangle), zero diagonal"""
    D = np.zeros((n, n))
    D[np.triu_indices(n, 1)] = d
    return D + D.T
