"""numpy fp64 reference of the t-SNE specification in DESIGN.md §10 (test infrastructure only: the product never imports it).

Written straight from the specification, not for speed: brute-force k-NN, vectorised bisection, dense exact repulsion."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny).item()
DBL_MIN = np.finfo(np.float64).tiny
DBL_MAX = np.finfo(np.float64).max


def pca(X, k, center=True, scale=False):
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0) if center else X.copy()
    if scale:
        sd = np.sqrt((Xc ** 2).sum(0) / (X.shape[0] - 1))
        Xc = Xc / sd
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, np.argsort(-w, kind="stable")[:k]]
    arg = np.abs(V).argmax(0)
    V = V * np.where(V[arg, np.arange(V.shape[1])] < 0, -1.0, 1.0)
    return Xc @ V, V


def normalize(X):
    X = X - X.mean(0)
    return X / np.abs(X).max()


def prepare(X, pca_on=True, initial_dims=50, pca_center=True, pca_scale=False, normalize_on=True):
    X = np.asarray(X, np.float64)
    if pca_on:
        X, _ = pca(X, min(initial_dims, X.shape[1]), pca_center, pca_scale)
    if normalize_on:
        X = normalize(X)
    return X


def sqdist_rows(X, rows):
    return ((X[rows, None, :] - X[None, :, :]) ** 2).sum(-1)


def knn(X, K, chunk=256):
    """K nearest rows of every row by sum (x_i - x_j)^2, self excluded, ties by the lower index"""
    n = X.shape[0]
    idx = np.zeros((n, K), np.int64)
    dist = np.zeros((n, K))
    for r0 in range(0, n, chunk):
        rows = np.arange(r0, min(n, r0 + chunk))
        D = sqdist_rows(X, rows)
        D[np.arange(rows.size), rows] = np.inf
        o = np.argsort(D, axis=1, kind="stable")[:, :K]
        idx[rows] = o
        dist[rows] = np.take_along_axis(D, o, 1)
    return idx, dist


def calibrate(dist, perplexity, tol=1e-5, steps=200, return_trace=False):
    """bhtsne's bisection on beta per row (entropy in nats); returns P_cond (n x K).  With return_trace also, per row, the number of
    steps taken (entropy evaluations, the one that stops included) and the smallest | |Hdiff| - tol | met: the margin of the row's stop
    decisions.  A row whose margin is far above the rounding error of H takes the same steps under any faithful evaluation."""
    n, K = dist.shape
    logU = np.log(perplexity)
    beta = np.ones(n)
    minb = np.full(n, -DBL_MAX)
    maxb = np.full(n, DBL_MAX)
    active = np.ones(n, bool)
    P = np.zeros_like(dist)
    sumP = np.full(n, DBL_MIN)
    taken = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    for _ in range(steps):
        a = np.flatnonzero(active)
        if a.size == 0:
            break
        Pa = np.exp(-beta[a, None] * dist[a])
        s = DBL_MIN + Pa.sum(1)
        H = (beta[a, None] * (dist[a] * Pa)).sum(1) / s + np.log(s)
        P[a] = Pa
        sumP[a] = s
        Hdiff = H - logU
        taken[a] += 1
        margin[a] = np.minimum(margin[a], np.abs(np.abs(Hdiff) - tol))
        done = (Hdiff < tol) & (-Hdiff < tol)
        up = ~done & (Hdiff > 0)
        dn = ~done & ~(Hdiff > 0)
        b = beta[a]
        minb[a[up]] = b[up]
        open_up = (maxb[a[up]] == DBL_MAX) | (maxb[a[up]] == -DBL_MAX)
        beta[a[up]] = np.where(open_up, b[up] * 2.0, (b[up] + maxb[a[up]]) / 2.0)
        maxb[a[dn]] = b[dn]
        open_dn = (minb[a[dn]] == -DBL_MAX) | (minb[a[dn]] == DBL_MAX)
        beta[a[dn]] = np.where(open_dn, b[dn] / 2.0, (b[dn] + minb[a[dn]]) / 2.0)
        active[a[done]] = False
    Pc = P / sumP[:, None]
    return (Pc, taken, margin) if return_trace else Pc


def joint_p(X, perplexity):
    """P = (P_cond + P_cond^T) / sum as a scipy CSR matrix (rows sorted by column)"""
    import scipy.sparse as sp

    n = X.shape[0]
    K = int(np.floor(3 * perplexity))
    idx, dist = knn(X, K)
    Pc = calibrate(dist, perplexity)
    M = sp.csr_matrix((Pc.ravel(), (np.repeat(np.arange(n), K), idx.ravel())), shape=(n, n))
    S = (M + M.T).tocsr()
    S.sort_indices()
    return S / S.sum()


def _pairs(P):
    P = P.tocoo()
    return P.row, P.col, P.data


def gradient(P, Y, return_z=False):
    """dY_i = sum_j P_ij q_ij (y_i - y_j) - (1/Z) sum_j q_ij^2 (y_i - y_j), exact"""
    n, dims = Y.shape
    r, c, p = _pairs(P)
    diff = Y[r] - Y[c]
    q = p / (1.0 + (diff ** 2).sum(1))
    attr = np.zeros_like(Y)
    for k in range(dims):
        attr[:, k] = np.bincount(r, weights=q * diff[:, k], minlength=n)
    D = np.zeros((n, n))
    for k in range(dims):
        D += (Y[:, k, None] - Y[None, :, k]) ** 2
    Q = 1.0 / (1.0 + D)
    np.fill_diagonal(Q, 0.0)
    Z = Q.sum()
    Q2 = Q * Q
    rep = Q2.sum(1)[:, None] * Y - Q2 @ Y
    g = attr - rep / Z
    return (g, Z) if return_z else g


def kl(P, Y, per_point=False):
    n, dims = Y.shape
    D = np.zeros((n, n))
    for k in range(dims):
        D += (Y[:, k, None] - Y[None, :, k]) ** 2
    Q = 1.0 / (1.0 + D)
    np.fill_diagonal(Q, 0.0)
    Z = Q.sum()
    r, c, p = _pairs(P)
    terms = p * np.log((p + FLT_MIN) / (Q[r, c] / Z + FLT_MIN))
    return np.bincount(r, weights=terms, minlength=n) if per_point else terms.sum()


def multiset_repulsion(pos, cnt, chunk=32, threads=8):
    """The exact repulsion of the n = sum(cnt) points Y = pos[assign] in which the distinct position a occurs cnt[a] times, at
    O(m^2 dims) for m positions instead of O(n^2).  With q_ab = 1 / (1 + |y_a - y_b|^2) it returns, per position,
        rep[a]  = sum_b c_b q_ab^2 (y_a - y_b)            (the point's own copies add nothing: their difference is 0)
        z[a]    = sum_b c_b q_ab - 1                      (the self pair taken out; the other c_a - 1 copies stay, at q = 1)
        A[a, k] = sum_b c_b q_ab^2 |y_a,k - y_b,k|        (the sum of the magnitudes of rep's terms: what a rounding bound scales with)
    so a point at position a has repulsion rep[a] and row sum z[a], and Z = sum_a c_a z[a].  Plain fp64; the rows go in chunks small
    enough for the cache, a few chunks at a time on threads (numpy releases the lock; a chunk's result does not depend on the others)."""
    pos = np.asarray(pos, np.float64)
    w = np.asarray(cnt, np.float64)
    m, dims = pos.shape
    rep = np.zeros((m, dims))
    A = np.zeros((m, dims))
    z = np.zeros(m)
    cols = [np.ascontiguousarray(pos[:, k]) for k in range(dims)]

    def block(r0):
        r1 = min(m, r0 + chunk)
        d = [cols[k][r0:r1, None] - cols[k][None, :] for k in range(dims)]
        t = np.empty_like(d[0])
        D = np.ones_like(t)
        for k in range(dims):
            np.multiply(d[k], d[k], out=t)
            D += t
        q = np.divide(w[None, :], D)             # c_b q_ab
        z[r0:r1] = q.sum(1) - 1.0
        q /= D                                   # c_b q_ab^2
        for k in range(dims):
            np.multiply(q, d[k], out=t)
            rep[r0:r1, k] = t.sum(1)
            np.abs(t, out=t)
            A[r0:r1, k] = t.sum(1)

    with ThreadPoolExecutor(max(1, min(threads, os.cpu_count() or 1))) as ex:
        list(ex.map(block, range(0, m, chunk)))
    return rep, z, A


def exact_repulsion(Y, chunk=32):
    """rep (n x dims), z (n) and A (n x dims) of multiset_repulsion for the rows of Y themselves, every row counted once: the dense
    exact repulsion in row chunks, without an n x n matrix"""
    Y = np.asarray(Y, np.float64)
    return multiset_repulsion(Y, np.ones(Y.shape[0]), chunk)


def init_y(n, dims, seed, runif):
    """1e-4 N(0, 1): polar method on pairs of R's unif_rand() after set.seed(seed), the second draw of a pair discarded.
    runif(seed, count): the first `count` values of that stream."""
    need = n * dims
    u = runif(seed, 4 * need + 64)
    out = np.zeros(need)
    k = 0
    for e in range(need):
        while True:
            if k + 2 > u.size:
                u = runif(seed, 2 * u.size)
            x = 2.0 * u[k] - 1.0
            y = 2.0 * u[k + 1] - 1.0
            k += 2
            rad = x * x + y * y
            if not (rad >= 1.0 or rad == 0.0):
                break
        out[e] = x * np.sqrt(-2.0 * np.log(rad) / rad) * 1e-4
    return out.reshape(n, dims)


def optimise(P, Y0, max_iter=1000, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5, final_momentum=0.8, eta=200.0,
             exaggeration=12.0):
    P = P.copy()
    Y = np.array(Y0, np.float64)
    uY = np.zeros_like(Y)
    gains = np.ones_like(Y)
    lying = stop_lying_iter > 0
    if lying:
        P.data = P.data * exaggeration
    costs = []
    for it in range(max_iter):
        dY = gradient(P, Y)
        gains = np.where(np.sign(dY) != np.sign(uY), gains + 0.2, gains * 0.8)
        gains[gains < 0.01] = 0.01
        uY = momentum * uY - eta * gains * dY
        Y = Y + uY
        Y = Y - Y.mean(0)
        if it == stop_lying_iter and lying:
            P.data = P.data / exaggeration
        if it == mom_switch_iter:
            momentum = final_momentum
        if (it > 0 and it % 50 == 0) or it == max_iter - 1:
            costs.append(kl(P, Y))
    return Y, np.array(costs)
