"""The UMAP specification of DESIGN.md §13 in numpy fp64: the a / b curve, the fuzzy graph, the negative-sample draw, one epoch and a
full run.  This is the project's own specification (modelled on umap-learn's algorithm and uwot's batch = TRUE mode); it claims no bit
parity with either.  The GPU tests compare every stage of libsharp_hip.so with these functions on the stage's own input."""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ---- curve ----------------------------------------------------------------------------------------------------------------------------
def curve_points(spread=1.0, min_dist=0.01):
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    return x, y


def curve_residual_jacobian(a, b, spread=1.0, min_dist=0.01):
    """r (300) and J (300 x 2) of r_k = 1 / (1 + a x_k^(2b)) - y_k at (a, b)"""
    x, y = curve_points(spread, min_dist)
    xp = x[1:]
    p = xp ** (2.0 * b)
    q = 1.0 + a * p
    r = np.concatenate([[1.0], 1.0 / q]) - y
    J = np.zeros((300, 2))
    J[1:, 0] = -p / q ** 2
    J[1:, 1] = -(a * p * 2.0 * np.log(xp)) / q ** 2
    return r, J


# ---- graph ----------------------------------------------------------------------------------------------------------------------------
def smooth_knn(d, order=None):
    """rho, sigma, the weights A (n x K) and the bisection's step counts from the lists' Euclidean distances d (n x K, self excluded);
    n_neighbors = K + 1.  order: a permutation of the K columns in which every sum runs (the result must not depend on it beyond
    rounding)."""
    d = np.asarray(d, np.float64)
    n, K = d.shape
    if order is not None:
        d = d[:, order]
    nn = K + 1
    target = np.log2(nn)
    rho = np.zeros(n)
    sigma = np.zeros(n)
    steps = np.zeros(n, np.int64)
    A = np.zeros((n, K))
    total = d.sum()
    for i in range(n):
        pos = d[i][d[i] > 0]
        rho[i] = pos.min() if pos.size else 0.0
        dv = d[i] - rho[i]
        lo, hi, mid = 0.0, np.inf, 1.0
        it = 0
        while it < 64:
            with np.errstate(under="ignore", over="ignore"):
                s = np.where(dv > 0, np.exp(-dv / mid), 1.0).sum()
            if abs(s - target) < 1e-5:
                break
            if s > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
            it += 1
        steps[i] = it
        m = d[i].sum() / nn if rho[i] > 0 else total / (n * nn)
        sigma[i] = max(mid, 1e-3 * m)
        with np.errstate(under="ignore", over="ignore"):
            A[i] = np.where(dv > 0, np.exp(-dv / sigma[i]), 1.0)
    if order is not None:
        inv = np.argsort(order)
        A = A[:, inv]
    return rho, sigma, A, steps


def row_sum_at(d_row, rho, sigma):
    """the bisection's sum of one row at sigma"""
    dv = np.asarray(d_row, np.float64) - rho
    with np.errstate(under="ignore", over="ignore"):
        return np.where(dv > 0, np.exp(-dv / sigma), 1.0).sum()


def union_parts(idx, A, n):
    """the pattern of A + A^T as a CSR with rows sorted by column, and per entry (i, j) the two values it is made of:
    (row_ptr, col, x = A_ij, y = A_ji), NaN where that direction is absent"""
    idx = np.asarray(idx, np.int64)
    K = idx.shape[1]
    i = np.repeat(np.arange(n, dtype=np.int64), K)
    j = idx.reshape(-1)
    w = np.asarray(A, np.float64).reshape(-1)
    kf, kr = i * n + j, j * n + i
    keys = np.union1d(kf, kr)
    x = np.full(keys.size, np.nan)
    y = np.full(keys.size, np.nan)
    x[np.searchsorted(keys, kf)] = w
    y[np.searchsorted(keys, kr)] = w
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, keys // n + 1, 1)
    return np.cumsum(rp), (keys % n).astype(np.int32), x, y


def fuzzy_union(idx, A, n):
    """W = A + A^T - A o A^T as a CSR with rows sorted by column: (row_ptr, col, val)"""
    rp, col, x, y = union_parts(idx, A, n)
    both = x + y - x * y
    return rp, col, np.where(np.isnan(y), x, np.where(np.isnan(x), y, both))


def weights(d, rho, sigma):
    """A (n x K) from the lists' distances at given rho and sigma"""
    dv = np.asarray(d, np.float64) - np.asarray(rho)[:, None]
    with np.errstate(under="ignore", over="ignore"):
        return np.where(dv > 0, np.exp(-dv / np.asarray(sigma)[:, None]), 1.0)


def graph(idx, d):
    rho, sigma, A, _ = smooth_knn(d)
    rp, col, val = fuzzy_union(idx, A, np.asarray(d).shape[0])
    return rp, col, val, rho, sigma


# ---- draw -----------------------------------------------------------------------------------------------------------------------------
def mix(z):
    """the splitmix64 finaliser on uint64 arrays (arithmetic mod 2^64)"""
    z = np.asarray(z, np.uint64).copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def draw(seed, ep, e, s, n):
    """the vertex drawn for (seed, epoch ep, edge e, sample s): e and s arrays (broadcast)"""
    with np.errstate(over="ignore"):
        x0 = mix(np.uint64(((int(seed) & MASK) * GOLDEN + int(ep)) & MASK))
        x = mix(x0 + np.asarray(e, np.uint64))
        x = mix(x + np.asarray(s, np.uint64))
    return np.floor((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 * float(n)).astype(np.int64)


def fires(ep, r):
    """whether an edge of rate r = w / wmax fires in epoch ep"""
    r = np.asarray(r, np.float64)
    if ep < 1:
        return np.zeros(r.shape, bool)
    return np.floor(float(ep) * r) > np.floor(float(ep - 1) * r)


# ---- epochs ---------------------------------------------------------------------------------------------------------------------------
def epoch(rp, col, val, Y, ep, n_epochs, a, b, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0, seed=10,
          return_terms=False):
    """Y after epoch ep (all rows from the old positions); return_terms: also the number of terms every row received and the number
    of coordinates the clip acted on"""
    Y = np.asarray(Y, np.float64)
    n, dims = Y.shape
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    val = np.asarray(val, np.float64)
    wmax = val.max()
    alpha = learning_rate * (1.0 - ep / n_epochs)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    f = np.nonzero(fires(ep, val / wmax))[0]
    delta = np.zeros_like(Y)
    terms = np.zeros(n, np.int64)
    clipped = 0
    if f.size:
        i, j = row[f], col[f]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            diff = Y[i] - Y[j]
            D = (diff * diff).sum(1)
            c = np.where(D > 0, (-2.0 * a * b * D ** (b - 1.0)) / (a * D ** b + 1.0), 0.0)
            g = np.where((D > 0)[:, None], 2.0 * np.clip(c[:, None] * diff, -4.0, 4.0), 0.0)
            clipped += int((np.abs(c[:, None] * diff)[D > 0] > 4.0).sum())
            np.add.at(delta, i, g)
            np.add.at(terms, i, 1)
            for s in range(negative_sample_rate):
                k = draw(seed, ep, f, s, n)
                diff = Y[i] - Y[k]
                D = (diff * diff).sum(1)
                ok = (k != i) & (D > 0)
                c = (2.0 * repulsion_strength * b) / ((0.001 + D) * (a * D ** b + 1.0))
                g = np.where(ok[:, None], np.clip(c[:, None] * diff, -4.0, 4.0), 0.0)
                clipped += int((np.abs(c[:, None] * diff)[ok] > 4.0).sum())
                np.add.at(delta, i, g)
                np.add.at(terms, i, 1)
    out = Y + alpha * delta
    return (out, terms, clipped) if return_terms else out


def scale_start(Y):
    """every coordinate mapped affinely onto [0, 10]; a constant coordinate becomes 0"""
    Y = np.asarray(Y, np.float64)
    mn, mx = Y.min(0), Y.max(0)
    w = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0, (Y - mn) / w * 10.0, 0.0)


def pca_start(X, dims):
    """the first dims principal components of X (centred), the sign making each vector's largest |component| positive"""
    Xc = np.asarray(X, np.float64) - np.mean(X, axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, np.argsort(-w, kind="stable")[:dims]]
    V = V * np.where(V[np.abs(V).argmax(0), np.arange(dims)] < 0, -1.0, 1.0)
    return Xc @ V


def knn_lists(X, K):
    """exact K nearest neighbours, self excluded, sorted by (distance, index): (idx, Euclidean distances)"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    idx = np.zeros((n, K), np.int64)
    d = np.zeros((n, K))
    for i in range(n):
        d2 = ((X - X[i]) ** 2).sum(1)
        d2[i] = np.inf
        o = np.lexsort((np.arange(n), d2))[:K]
        idx[i], d[i] = o, np.sqrt(d2[o])
    return idx, d


def run(X, n_neighbors=15, dims=2, n_epochs=None, a=None, b=None, ab=None, learning_rate=1.0, negative_sample_rate=5,
        repulsion_strength=1.0, seed=10, init=None):
    """the full reference run; ab = (a, b) of the curve (sharp_umap_ab's, or any fit of it); init: None (the PCA start) or a matrix"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    if n_epochs is None:
        n_epochs = 500 if n <= 10000 else 200
    if ab is not None:
        a, b = ab
    idx, d = knn_lists(X, n_neighbors - 1)
    rp, col, val, _, _ = graph(idx, d)
    Y = scale_start(pca_start(X, dims) if init is None else init)
    for ep in range(n_epochs):
        Y = epoch(rp, col, val, Y, ep, n_epochs, a, b, learning_rate, negative_sample_rate, repulsion_strength, seed)
    return Y


# ---- quality measures -----------------------------------------------------------------------------------------------------------------
def blobs(n=1500, d=10, k=6, seed=0):
    """k Gaussian blobs of sigma = 1 with centres N(0, 6^2): (X, labels)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 6.0, size=(k, d))
    lab = np.arange(n) % k
    return centres[lab] + rng.normal(size=(n, d)), lab


def graph_case(n=1025, kmax=255, seed=5):
    """the graph tests' lists (idx, d: n x kmax, sorted, so the first K columns are the K-NN lists): six blobs plus a 300-row clump at
    sigma = 1e-4, four copies of one row (some duplicates: rho from the first positive distance), an isolated far row whose neighbours' distances are set 50 apart
    (the doubling branch: sigma > 1), and one row whose distances are all set to 0 (its K nearest are exact duplicates: rho = 0, the global floor).
    Returns (idx, d, {"dup_all": row, "dup_some": row, "far": row})."""
    rng = np.random.default_rng(seed)
    X, _ = blobs(n, 10, 6, seed)
    X[:300] = X[0] + 1e-4 * rng.normal(size=(300, 10))
    X[401:404] = X[400]
    X[n - 1] = 0.0
    X[n - 1, 0] = 1000.0
    idx, d = knn_lists(X, kmax)
    d[500] = 0.0
    d[n - 1] = d[n - 1, 0] + 50.0 * np.arange(kmax)
    return idx, d, {"dup_all": 500, "dup_some": 400, "far": n - 1}


def knn_purity(Y, lab, k=15):
    """the share of every point's k nearest neighbours in the map that carry its label, averaged"""
    idx, _ = knn_lists(Y, k)
    return float((lab[idx] == lab[:, None]).mean())
