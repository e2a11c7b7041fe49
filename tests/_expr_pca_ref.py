"""The truncated PCA of sparse expression blocks of DESIGN.md §21, restated in numpy / scipy, and the tests' case builders.

Input: a list of CSC blocks, genes x cells, all with the same m genes (scipy csc_matrix; stored zeros are kept and count as zeros).
Transform: t = x; with normalize_total = T > 0, t = x * (T / L_c), L_c the cell's sum (a cell whose sum is 0 stays 0); with log1p,
t = log1p(.) after that.  Gene statistics: mu = (sum t) / n, var = (sum over the stored entries of (t - mu)^2 + (n - stored) mu^2) /
(n - 1); a gene whose n values are all equal has mu = that value and var = 0 exactly.  w = 1 without scale, else 1 / sqrt(var) (0
where var = 0).  The sums of the statistics are taken in extended precision.  A = (T^T - 1 mu^T) diag(w), n x m, never formed.  Randomised subspace iteration with l = k +
oversample columns, Omega a hash of (seed, gene, column), orth = CholeskyQR2; the result as in the module's pca().  The specification is
the project's own (modelled on Halko, Martinsson and Tropp and on what scanpy / Seurat compute); no parity with sklearn, scanpy, Seurat
or irlba is claimed.  The components beyond the planted ones of a noisy input do not converge, as for any randomised PCA."""
import functools

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

U = 2.0 ** -53
GOLD = np.uint64(0x9E3779B97F4A7C15)
DEFAULTS = {"n_components": 50, "oversample": 10, "n_iter": 4, "normalize_total": 1e4, "log1p": True, "center": True, "scale": False}


class RankError(ValueError):
    pass


def mix(z):
    """DESIGN.md §13's mix (the splitmix64 finaliser) on uint64 arrays"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def omega(seed, genes, l):
    """Omega[g, j] = (mix(mix(seed * golden + g) + j) >> 11) 2^-53 - 0.5 for the gene ids `genes`: every step is exact in fp64"""
    g = np.asarray(genes, np.uint64)
    with np.errstate(over="ignore"):
        a = mix(np.uint64(seed) * GOLD + g)
        h = mix(a[:, None] + np.arange(l, dtype=np.uint64)[None, :])
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def concat(blocks):
    """the blocks side by side as one csc_matrix, stored entries untouched"""
    blocks = [blocks] if sp.issparse(blocks) or isinstance(blocks, np.ndarray) else list(blocks)
    blocks = [b if sp.issparse(b) else sp.csc_matrix(np.asarray(b, np.float64)) for b in blocks]
    m = blocks[0].shape[0]
    ptr, off = [np.zeros(1, np.int64)], 0
    for b in blocks:
        assert b.shape[0] == m
        ptr.append(np.asarray(b.indptr[1:], np.int64) + off)
        off += int(b.indptr[-1])
    idx = np.concatenate([np.asarray(b.indices, np.int64) for b in blocks])
    dat = np.concatenate([np.asarray(b.data, np.float64) for b in blocks])
    X = sp.csc_matrix((dat, idx, np.concatenate(ptr)), shape=(m, sum(b.shape[1] for b in blocks)))
    return X


def segment_sums(values, ptr):
    """the sums of values[ptr[i] : ptr[i + 1]] in extended precision (an empty segment: 0), so that the reference's statistics carry
    one rounding where the device's carry those of its summation order"""
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros(ptr.size - 1, np.longdouble)
    some = np.diff(ptr) > 0
    if some.any():
        out[some] = np.add.reduceat(np.asarray(values, np.longdouble), ptr[:-1][some])
    return out


def cell_sums(X):
    """per cell, the sum of its stored values"""
    return segment_sums(X.data, X.indptr).astype(np.float64)


def transform(X, normalize_total=1e4, log1p=True):
    """(T, L): T = X's pattern with the transformed values, L = the cells' sums before it"""
    X = concat(X)
    L = cell_sums(X)
    t = X.data.copy()
    if (normalize_total or log1p) and (t < 0).any():
        raise ValueError("a negative value")
    if normalize_total and normalize_total > 0:
        with np.errstate(divide="ignore"):
            f = np.where(L > 0, normalize_total / np.where(L > 0, L, 1.0), 0.0)
        t = t * np.repeat(f, np.diff(X.indptr))
    if log1p:
        t = np.log1p(t)
    return sp.csc_matrix((t, X.indices, X.indptr), shape=X.shape), L


def gene_stats(T):
    """mu, var, the number of non-zero values per gene, and the stored entries per gene, of the transformed matrix T (m x n)"""
    m, n = T.shape
    gene = np.asarray(T.indices, np.int64)
    stored = np.bincount(gene, minlength=m)
    R = T.tocsr()                                               # (stored zeros stay)
    S = segment_sums(R.data, R.indptr)
    lo = np.full(m, np.inf)
    hi = np.full(m, -np.inf)
    np.minimum.at(lo, gene, T.data)
    np.maximum.at(hi, gene, T.data)
    full = stored == n
    mn = np.where(stored == 0, 0.0, np.where(full, lo, np.minimum(lo, 0.0)))
    mx = np.where(stored == 0, 0.0, np.where(full, hi, np.maximum(hi, 0.0)))
    const = mn == mx
    mu = np.where(const, mn, (S / n).astype(np.float64))
    mul = mu.astype(np.longdouble)
    SS = segment_sums((R.data.astype(np.longdouble) - np.repeat(mul, np.diff(R.indptr))) ** 2, R.indptr)
    var = np.where(const, 0.0, ((SS + (n - stored) * mul * mul) / (n - 1)).astype(np.float64))
    nnz = np.bincount(gene, weights=(T.data != 0), minlength=m).astype(np.int64)
    return mu, var, nnz, stored


def weights(var, scale):
    """(the result's `scale`, w): without scale both are 1; with it sd = sqrt(var) and w = 1 / sd, and sd = 1, w = 0 where var = 0"""
    if not scale:
        return np.ones_like(var), np.ones_like(var)
    sd = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), 1.0)
    return sd, np.where(var > 0, 1.0 / sd, 0.0)


def spmm_cells(T, mu, w, B):
    """Y = A B: Y[c, :] = sum over the cell's stored entries of t_gc Bs[g, :] - mu^T Bs, Bs = diag(w) B"""
    Bs = w[:, None] * B
    return np.asarray(T.T @ Bs) - (mu[:, None] * Bs).sum(0)[None, :]


def spmm_cells_bound(T, mu, w, B):
    """(N + 8) 2^-53 (|T|^T |Bs| + |mu|^T |Bs|) per entry, N the cell's stored entries (the 8: the transform's division and log1p)"""
    Bs = np.abs(w[:, None] * B)
    N = np.diff(T.indptr).astype(np.float64)
    return (N[:, None] + 8) * U * (np.asarray(abs(T).T @ Bs) + (np.abs(mu)[:, None] * Bs).sum(0)[None, :])


def spmm_genes(T, mu, w, Q):
    """Z = A^T Q: Z[g, :] = w_g (sum over the gene's stored entries of t_gc Q[c, :] - mu_g colsum(Q))"""
    return w[:, None] * (np.asarray(T @ Q) - mu[:, None] * Q.sum(0)[None, :])


def spmm_genes_bound(T, mu, w, Q, stored):
    aQ = np.abs(Q)
    return (stored[:, None] + 8.0) * U * np.abs(w)[:, None] * (np.asarray(abs(T) @ aQ) + np.abs(mu)[:, None] * aQ.sum(0)[None, :])


def chol_upper(G, what="numerical rank below n_components + oversample"):
    """R upper triangular with G = R^T R; a pivot that is not finite, <= 0 or within l 2^-52 of G's diagonal (rounding alone) refuses"""
    l = G.shape[0]
    R = np.zeros_like(G)
    for j in range(l):
        d = G[j, j] - R[:j, j] @ R[:j, j]
        if not np.isfinite(d) or not d > l * 2.0 ** -52 * G[j, j]:
            raise RankError(what)
        R[j, j] = np.sqrt(d)
        R[j, j + 1:] = (G[j, j + 1:] - R[:j, j] @ R[:j, j + 1:]) / R[j, j]
    return R


def orth(Y):
    """CholeskyQR2"""
    Q = Y
    for _ in range(2):
        R = chol_upper(Q.T @ Q)
        Q = sl.solve_triangular(R, Q.T, trans="T", lower=False).T
    return Q


def sign_fix(scores, loadings):
    """each component's loading of largest magnitude positive; on ties the lowest gene decides"""
    arg = np.argmax(np.abs(loadings), axis=0)                  # (the first of equal maxima)
    sg = np.where(loadings[arg, np.arange(loadings.shape[1])] < 0, -1.0, 1.0)
    return scores * sg, loadings * sg


def pca(blocks, n_components=50, oversample=10, n_iter=4, normalize_total=1e4, log1p=True, scale=False, seed=0, gene_ids=None, info=None):
    """the fit of DESIGN.md §21; gene_ids: the ids that Omega is drawn for (default 0 .. m - 1)"""
    T, _ = transform(blocks, normalize_total, log1p)
    m, n = T.shape
    k, l = int(n_components), int(n_components) + int(oversample)
    assert 1 <= k and 1 <= l <= 128 and l <= min(n, m)
    mu, var, _, _ = gene_stats(T)
    sd, w = weights(var, scale)
    total_var = float((w * w * var).sum())
    if not total_var > 0:
        raise RankError("numerical rank below n_components + oversample")
    Tr = T.tocsr()
    conds = []

    def north(Y):
        conds.append(np.linalg.cond(Y.T @ Y))
        return orth(Y)

    Y = spmm_cells(T, mu, w, omega(seed, np.arange(m) if gene_ids is None else gene_ids, l))
    for _ in range(int(n_iter)):
        Q = north(Y)
        Z = north(spmm_genes(Tr, mu, w, Q))
        Y = spmm_cells(T, mu, w, Z)
    Q = north(Y)
    Z = spmm_genes(Tr, mu, w, Q)
    lam, W = np.linalg.eigh(Z.T @ Z)
    lam, W = lam[::-1][:k], W[:, ::-1][:, :k]
    if not (lam > 0).all():
        raise RankError("numerical rank below n_components + oversample")
    s = np.sqrt(lam)
    # scores = A loadings (the projection of the cells on the components, what pca_transform gives for any cell) rather than the
    # subspace's Q W diag(s) = Q Q^T A loadings: the two agree as far as a component has converged
    _, loadings = sign_fix(np.zeros((1, k)), (Z @ W) * (1.0 / s))
    scores = spmm_cells(T, mu, w, loadings)
    if info is not None:
        info["max_cond"] = max(conds)
    return {"scores": scores, "loadings": loadings, "singular_values": s, "sdev": s / np.sqrt(n - 1.0), "center": mu, "scale": sd,
            "gene_var": var, "total_var": total_var, "normalize_total": normalize_total, "log1p": log1p}


def pca_transform(blocks, fit):
    """scores of new cells: the cell-side product with the loadings in place of Omega"""
    T, _ = transform(blocks, fit["normalize_total"], fit["log1p"])
    return spmm_cells(T, fit["center"], 1.0 / fit["scale"], fit["loadings"])


def dense_A(blocks, normalize_total=1e4, log1p=True, scale=False):
    T, _ = transform(blocks, normalize_total, log1p)
    mu, var, _, _ = gene_stats(T)
    _, w = weights(var, scale)
    return (T.toarray().T - mu[None, :]) * w[None, :]


def dense_singular_values(blocks, k, **kw):
    """the k largest singular values of the dense A, from the eigenvalues of the smaller Gram"""
    A = dense_A(blocks, **kw)
    G = A @ A.T if A.shape[0] <= A.shape[1] else A.T @ A
    d = G.shape[0]
    lam = sl.eigvalsh(G, subset_by_index=[d - k, d - 1])[::-1]
    return np.sqrt(lam)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(n, m, G, seed=1):
    """Poisson counts with G planted clusters: gamma(0.3) base rates, a tenth of the genes raised 3 - 8 x per cluster (genes x cells, CSC)"""
    rng = np.random.default_rng(seed)
    base = rng.gamma(0.3, size=m) * 1.1
    rate = np.repeat(base[:, None], G, axis=1)
    for c in range(G):
        up = rng.choice(m, m // 10, replace=False)
        rate[up, c] *= rng.uniform(3.0, 8.0, size=up.size)
    lab = rng.integers(0, G, size=n)
    X = rng.poisson(rate[:, lab]).astype(np.float64)
    return sp.csc_matrix(X), lab


PLANTED = {"small": (1500, 800, 6, 10), "large": (3000, 2000, 12, 50)}       # name: n, m, clusters, k


def planted_case(name):
    n, m, G, k = PLANTED[name]
    return planted(n, m, G)[0], G - 1, k


def permuted(X, seed):
    """X with its cells and genes stored in a random order: (Xp, gene order, cell order), Xp[i, j] = X[go[i], co[j]]"""
    rng = np.random.default_rng(seed)
    go, co = rng.permutation(X.shape[0]), rng.permutation(X.shape[1])
    Xp = X.tocsr()[go][:, co].tocsc()
    Xp.sort_indices()
    return Xp, go, co


@functools.lru_cache(maxsize=None)
def reference_run(name, scale):
    """the reference fit of a planted input, its error against the dense singular values over the planted components, and its own
    rounding spread: the same input with cells and genes stored in three random orders, Omega tied to the gene's original id"""
    X, planted_k, k = planted_case(name)
    info = {}
    fit = pca(X, k, scale=scale, info=info)
    dense = dense_singular_values(X, k, scale=scale)
    err = np.abs(fit["singular_values"] - dense) / dense
    spread = {"s": 0.0, "scores": 0.0, "loadings": 0.0}
    for sd in (11, 12, 13):
        Xp, go, co = permuted(X, sd)
        f = pca(Xp, k, scale=scale, gene_ids=go)
        sc = np.empty_like(f["scores"])
        sc[co] = f["scores"]
        ld = np.empty_like(f["loadings"])
        ld[go] = f["loadings"]
        # the sign rule looks at loadings, which a permutation only reorders; a tie of magnitudes would be decided by another gene
        sc, ld = sign_fix(sc, ld)
        spread["s"] = max(spread["s"], np.abs(f["singular_values"] - fit["singular_values"]).max() / fit["singular_values"][0])
        spread["scores"] = max(spread["scores"], np.abs(sc - fit["scores"]).max() / np.abs(fit["scores"]).max())
        spread["loadings"] = max(spread["loadings"], np.abs(ld - fit["loadings"]).max())
    return {"fit": fit, "dense": dense, "err": err, "planted": planted_k, "spread": spread, "max_cond": info["max_cond"]}


def random_csc(m, n, density, seed, counts=None, kind="mixed"):
    """a random m x n CSC block: with `counts`, cell c holds exactly counts[c] entries; values: counts, multiples of 0.1 that fp32 cannot
    hold, and stored zeros"""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = rng.binomial(m, density, size=n)
    counts = np.asarray(counts, np.int64)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(counts)
    idx = np.concatenate([np.sort(rng.choice(m, int(c), replace=False)) for c in counts] + [np.zeros(0, np.int64)])
    nnz = int(ptr[-1])
    val = rng.integers(1, 9, size=nnz).astype(np.float64)
    if kind == "mixed":
        tenth = rng.random(nnz) < 0.3
        val[tenth] = 0.1 * rng.integers(1, 40, size=int(tenth.sum()))
        val[rng.random(nnz) < 0.05] = 0.0
    return sp.csc_matrix((val, idx.astype(np.int32), ptr), shape=(m, n))


def from_gene_counts(gcounts, n, seed):
    """an m x n CSC block in which gene g holds exactly gcounts[g] entries (cells chosen at random)"""
    rows = sp.csr_matrix(random_csc(n, len(gcounts), 0.0, seed, counts=gcounts).T)
    X = rows.tocsc()
    X.sort_indices()
    return X


def stage_cases(chunk, slab):
    """the boundary shapes of the product kernels, built from the library's chunk length and Gram slab rows"""
    m = 130
    cases = {
        "cells": random_csc(m, 200, 0.0, 1, counts=[0, 1, 63, 64, 65, m] + list(np.random.default_rng(2).integers(0, m, size=194))),
        "genes": from_gene_counts([0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1] + list(np.random.default_rng(3).integers(0, 90, size=34)),
                                  2 * chunk + 50, 4),
        "m70000": random_csc(70000, 50, 0.0, 6, counts=np.random.default_rng(7).integers(0, 120, size=50)),
        "n2": random_csc(40, 2, 0.4, 8),
    }
    full = random_csc(30, 4099, 0.05, 5).tolil()
    full[0, :] = np.random.default_rng(9).integers(1, 5, size=4099).astype(np.float64)
    cases["full"] = sp.csc_matrix(full.tocsc())
    for d in (-1, 0, 1):
        cases["slab%+d" % d] = random_csc(20, slab + d, 0.1, 20 + d)
    return cases


def ragged(X, cuts):
    """X cut into column blocks at `cuts` (a cut repeated, or at 0 / n, leaves an empty block)"""
    edges = [0] + list(cuts) + [X.shape[1]]
    return [X[:, a:b] for a, b in zip(edges[:-1], edges[1:])]
