"""numpy restatements used by the cutree / silhouette / Calinski-Harabasz tests: cluster::silhouette's sildist(), the
Euclidean Calinski-Harabasz index, and the seeded inputs of the GPU tests.  Test infrastructure."""
import numpy as np

EPS = 2.0 ** -53
SCIPY_METRIC = {"euclidean": "euclidean", "maximum": "chebyshev", "manhattan": "cityblock", "minkowski": "minkowski"}


def recode(labels):
    """R's factor(): codes 1 .. k in sorted order of the distinct labels"""
    levels, inv = np.unique(np.asarray(labels), return_inverse=True)
    return inv.ravel().astype(np.int64) + 1, levels


def sildist(rows, cl, k, block=1024):
    """sildist() (cluster/src/sildist.c) from the rows of a distance matrix.  rows(i0, i1) returns the (i1 - i0, n) block of distances
    of the cells i0 .. i1 - 1 to all cells (its diagonal entries 0).  cl: codes 1 .. k.  Returns width, neighbor (codes), a, b and gap =
    (second smallest other mean - smallest) / smallest (inf with two clusters): the margin by which the neighbour is decided."""
    cl = np.asarray(cl, np.int64)
    n = cl.size
    counts = np.bincount(cl - 1, minlength=k).astype(np.float64)
    onehot = np.zeros((n, k))
    onehot[np.arange(n), cl - 1] = 1.0
    width, nb, av, bv, gap = np.zeros(n), np.zeros(n, np.int64), np.zeros(n), np.zeros(n), np.full(n, np.inf)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        diC = np.asarray(rows(i0, i1)) @ onehot                  # sum of the distances to every cluster (the own distance is 0)
        ci = cl[i0:i1] - 1
        r = np.arange(i1 - i0)
        den = np.broadcast_to(counts, diC.shape).copy()
        den[r, ci] -= 1.0                                        # a(i) divides by n_c - 1
        single = den[r, ci] == 0
        den[r[single], ci[single]] = 1.0
        m = diC / den
        a = m[r, ci].copy()
        m[r, ci] = np.inf
        j = np.argmin(m, axis=1)                                 # the FIRST smallest: sildist's strict >
        b = m[r, j]
        if k > 2:
            m2 = m.copy()
            m2[r, j] = np.inf
            gap[i0:i1] = (m2.min(axis=1) - b) / b
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(single | (a == b), 0.0, (b - a) / np.maximum(a, b))
        width[i0:i1], nb[i0:i1], av[i0:i1], bv[i0:i1] = w, j + 1, a, b
    return {"width": width, "neighbor": nb, "a": av, "b": bv, "gap": gap}


def sildist_full(D, cl, k):
    D = np.asarray(D)
    return sildist(lambda i0, i1: D[i0:i1], cl, k)


def cdist_rows(x, metric, p=3.0):
    """rows(i0, i1) over scipy's cdist (computed from the differences) for the four difference metrics"""
    from scipy.spatial.distance import cdist

    kw = {"p": p} if metric == "minkowski" else {}

    def rows(i0, i1):
        d = cdist(x[i0:i1], x, SCIPY_METRIC[metric], **kw)
        d[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
        return d
    return rows


def squareform_rows(dcond, n):
    from scipy.spatial.distance import squareform

    D = squareform(np.asarray(dcond))
    return lambda i0, i1: D[i0:i1]


def ch_euclid(x, cl, k):
    """clusterCrit's Calinski_Harabasz = [B / (k - 1)] / [W / (n - k)], squared Euclidean (the oracle's ch_euclid)"""
    n = x.shape[0]
    allm = x.mean(0)
    B = W = 0.0
    for c in range(1, k + 1):
        xc = x[cl == c]
        m = xc.mean(0)
        B += xc.shape[0] * np.sum((m - allm) ** 2)
        W += np.sum((xc - m) ** 2)
    return (B / (k - 1)) / (W / (n - k)) if W > 0 else np.inf


def gaussian_clusters(seed, n, p, g):
    """Seeded Gaussian clusters with 5 % of the labels reassigned and one singleton cluster (label g + 1, cell n // 2).  Draw order from
    one default_rng(seed): centres, true cluster, noise, mask, replacement labels."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(scale=3, size=(g, p))
    cluster = rng.integers(0, g, n)
    x = centres[cluster] + rng.normal(size=(n, p))
    mask = rng.random(n) < 0.05
    repl = rng.integers(0, g, n)
    labels = np.where(mask, repl, cluster) + 1
    labels[n // 2] = g + 1
    return np.ascontiguousarray(x), labels.astype(np.int64)


def exact_case(seed=5):
    """490 cells, 6 integer features in 0 .. 3, six clusters, manhattan: every distance and every per-cluster sum is an exact integer.
    Cluster 11 is an exact copy of cluster 3 (every outside cell has two equal means), {u, v} (label 40) sits beside the one-cell
    cluster {w} (label -7) with d(u, v) == d(u, w) == 1 (a == b for u).  Cells shuffled, labels not 1 .. k."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, size=(160, 6))
    Cc = rng.integers(0, 4, size=(100, 6))
    Dd = rng.integers(0, 4, size=(67, 6))
    uvw = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]])
    x = np.concatenate([A, A, Cc, Dd, uvw]).astype(np.float64)
    labels = np.concatenate([np.full(160, 11), np.full(160, 3), np.full(100, 0), np.full(67, 4), [40, 40, -7]])
    o = rng.permutation(x.shape[0])
    u = int(np.flatnonzero(o == 487)[0])                        # where u went
    return np.ascontiguousarray(x[o]), labels[o].astype(np.int64), u
