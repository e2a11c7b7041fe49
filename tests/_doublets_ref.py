"""The doublet detection of DESIGN.md §24 restated in numpy / scipy, and the tests' inputs.

round(x) = floor(x + 0.5) everywhere.  The steps and the order of their operations:
  pairs      parents[s, j] = floor((double)(h(s, j) >> 11) * 2^-53 * (double)n), h(s, j) = mix(mix(seed * golden + s) + j) with §13's mix
  plan       n_sim = round(ratio n); k_adj = round(n_neighbors (1 + n_sim / n)); the default n_neighbors = max(1, round(0.5 sqrt(n))),
             lowered while its k_adj passes min(255, n + n_sim - 1)
  synthesis  doublet s = column a + column b (value of a + value of b for a shared gene), genes ascending, a shared gene once
  scores     the doublets through the fit as new cells (the transform over all genes with L = L_a + L_b, the subset, the product)
  counts     c[i] = the neighbours of row i, among the K = k_adj nearest of the (observed, simulated) rows, whose index is >= n
  table      r = n_sim / n; u = rho / r; one = 1 - rho; v = one - u; q = (c + 1) / (k_adj + 2); num = (q * rho) / r; den = one - q * v;
             score = num / den
  threshold  bin(x) = floor((x - min) / (max - min) * 256), at most 255; h smoothed by ((h[i - 1] + h[i]) + h[i + 1]) / 3 with h[-1] =
             h[1] and h[256] = h[254] while more than two local maxima stand (at most 10000 times); a local maximum is a run of equal
             values higher than the value on either side (a missing side counts as lower); with exactly two, the threshold is min +
             ((i + 0.5) * (max - min)) / 256 for the lowest bin i between them (the first of equal ones); predicted = score > threshold
The specification is the project's own, modelled on Scrublet; no parity with the scrublet or scanpy packages is claimed."""
import functools

import numpy as np
import scipy.sparse as sp

import _expr_pca_ref as ref
import _hvg_ref as hvgref

BINS = 256
MAX_SMOOTH = 10000
MAX_K = 255


def rnd(x):
    return int(np.floor(x + 0.5))


def pairs(n, n_sim, seed=0):
    s = np.arange(n_sim, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = ref.mix(np.uint64(seed) * ref.GOLD + s)
        h = ref.mix(a[:, None] + np.arange(2, dtype=np.uint64)[None, :])
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.floor(u * float(n)).astype(np.int64)


def k_adj_of(nn, n, n_sim):
    return rnd(nn * (1.0 + n_sim / n))


def plan(n, ratio=2.0, n_neighbors=None):
    """(n_sim, n_neighbors, k_adj)"""
    n_sim = rnd(ratio * n)
    cap = min(MAX_K, n + n_sim - 1)
    if n_neighbors is None:
        nn = max(1, rnd(0.5 * np.sqrt(float(n))))
        while nn > 1 and k_adj_of(nn, n, n_sim) > cap:
            nn -= 1
    else:
        nn = int(n_neighbors)
    return n_sim, nn, k_adj_of(nn, n, n_sim)


def synth(blocks, parents):
    """the doublets as a CSC matrix (genes x n_sim) by an explicit merge of the two sorted columns, and their sums L_a + L_b"""
    X = ref.concat(blocks)
    L = ref.cell_sums(X)
    ptr, idx, val = [0], [], []
    for a, b in np.asarray(parents, np.int64):
        ga, va = X.indices[X.indptr[a]:X.indptr[a + 1]], X.data[X.indptr[a]:X.indptr[a + 1]]
        gb, vb = X.indices[X.indptr[b]:X.indptr[b + 1]], X.data[X.indptr[b]:X.indptr[b + 1]]
        g = np.union1d(ga, gb)
        v = np.zeros(g.size)
        v[np.searchsorted(g, ga)] = va
        v[np.searchsorted(g, gb)] += vb
        idx.append(g)
        val.append(v)
        ptr.append(ptr[-1] + g.size)
    idx = np.concatenate(idx + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate(val + [np.zeros(0)])
    D = sp.csc_matrix((val, idx, np.array(ptr, np.int64)), shape=(X.shape[0], len(ptr) - 1))
    P = np.asarray(parents, np.int64)
    return D, L[P[:, 0]] + L[P[:, 1]]


def score_table(k_adj, r, rho):
    c = np.arange(k_adj + 1, dtype=np.float64)
    u = rho / r
    one = 1.0 - rho
    v = one - u
    q = (c + 1.0) / (float(k_adj) + 2.0)
    num = (q * rho) / r
    den = one - q * v
    return num / den


def local_maxima(h):
    at, i, nb = [], 0, len(h)
    while i < nb:
        j = i
        while j + 1 < nb and h[j + 1] == h[i]:
            j += 1
        if (i == 0 or h[i - 1] < h[i]) and (j == nb - 1 or h[j + 1] < h[i]):
            at.append(i)
        i = j + 1
    return at


def smooth(h):
    lo = np.concatenate([h[1:2], h[:-1]])
    hi = np.concatenate([h[1:], h[-2:-1]])
    return ((lo + h) + hi) / 3.0


def histogram(sim):
    mn, mx = float(sim.min()), float(sim.max())
    b = np.floor((sim - mn) / (mx - mn) * float(BINS)).astype(np.int64).clip(0, BINS - 1)
    return np.bincount(b, minlength=BINS).astype(np.float64), mn, mx - mn


def threshold(obs, sim, thr=None):
    """{"threshold" (None: not found), "threshold_found", "predicted_doublets", the rates, "passes"}"""
    obs, sim = np.asarray(obs, np.float64), np.asarray(sim, np.float64)
    out = {"threshold": None, "threshold_found": False, "predicted_doublets": None, "detected_doublet_rate": None,
           "detectable_doublet_fraction": None, "overall_doublet_rate": None, "passes": 0}
    if thr is None:
        if not sim.max() > sim.min():
            return out
        h, mn, width = histogram(sim)
        at = local_maxima(h)
        while len(at) > 2 and out["passes"] < MAX_SMOOTH:
            h = smooth(h)
            out["passes"] += 1
            at = local_maxima(h)
        if len(at) != 2:
            return out
        i = at[0] + int(np.argmin(h[at[0]:at[1] + 1]))
        thr = mn + ((i + 0.5) * width) / float(BINS)
        out["threshold_found"] = True
    out["threshold"] = float(thr)
    out["predicted_doublets"] = obs > thr
    out["detected_doublet_rate"] = float((obs > thr).sum()) / obs.size
    out["detectable_doublet_fraction"] = float((sim > thr).sum()) / sim.size
    out["overall_doublet_rate"] = out["detected_doublet_rate"] / out["detectable_doublet_fraction"] if (sim > thr).any() else 0.0
    return out


def knn_index(Z, K):
    """the K nearest other rows of every row by (squared distance, index): brute force"""
    n = Z.shape[0]
    sq = (Z * Z).sum(1)
    out = np.zeros((n, K), np.int64)
    for i0 in range(0, n, 1024):
        d = sq[i0:i0 + 1024, None] + sq[None, :] - 2.0 * (Z[i0:i0 + 1024] @ Z.T)
        d[np.arange(d.shape[0]), np.arange(i0, i0 + d.shape[0])] = np.inf
        out[i0:i0 + 1024] = np.argsort(d, axis=1, kind="stable")[:, :K]
    return out


def neighbor_counts(index, n_obs):
    return (np.asarray(index) >= n_obs).sum(1).astype(np.int64)


def knn_counts(Z, K, n_obs):
    """neighbor_counts(knn_index(Z, K), n_obs) without sorting the lists: the rows closer than the K-th distance, and of the rows at
    that distance the lowest indices"""
    n = Z.shape[0]
    sq = (Z * Z).sum(1)
    out = np.zeros(n, np.int64)
    for i0 in range(0, n, 1024):
        d = sq[i0:i0 + 1024, None] + sq[None, :] - 2.0 * (Z[i0:i0 + 1024] @ Z.T)
        d[np.arange(d.shape[0]), np.arange(i0, i0 + d.shape[0])] = np.inf
        kth = np.partition(d, K - 1, axis=1)[:, K - 1][:, None]
        less, eq = d < kth, d == kth
        sel = less | (eq & (np.cumsum(eq, axis=1) <= (K - less.sum(1))[:, None]))
        out[i0:i0 + 1024] = sel[:, n_obs:].sum(1)
    return out


def fit_observed(blocks, n_prin_comps=30, n_top_genes=2000, genes=None, normalize_total=1e4, log1p=True, scale=True):
    """the reference's variable genes and PCA of the observed cells: (fit, genes)"""
    if genes is None:
        genes = hvgref.hvg(blocks, n_top_genes)["genes"]
    fit = hvgref.pca_subset(blocks, genes, n_prin_comps, normalize_total=normalize_total, log1p=log1p, scale=scale)
    fit["normalize_total"], fit["log1p"] = normalize_total, log1p
    return fit, np.asarray(genes, np.int64)


def project(D, fit, genes):
    """the scores of the cells of D (all genes) in a fit on `genes`"""
    T, _ = ref.transform(D, fit["normalize_total"], fit["log1p"])
    Ts = T.tocsr()[genes].tocsc()
    return ref.spmm_cells(Ts, fit["center"], 1.0 / fit["scale"], fit["loadings"])


def scrublet(blocks, fit, genes, sim_doublet_ratio=2.0, expected_doublet_rate=0.1, n_neighbors=None, thr=None, seed=0):
    """steps 1 and 3 to 6 on a fit of fit_observed()"""
    X = ref.concat(blocks)
    n = X.shape[1]
    n_sim, nn, K = plan(n, sim_doublet_ratio, n_neighbors)
    par = pairs(n, n_sim, seed)
    D = X[:, par[:, 0]] + X[:, par[:, 1]]
    Z = np.vstack([fit["scores"], project(D, fit, genes)])
    counts = knn_counts(Z, K, n)
    table = score_table(K, n_sim / n, expected_doublet_rate)
    sc = table[counts]
    out = threshold(sc[:n], sc[n:], thr)
    out.update({"doublet_scores": sc[:n], "doublet_scores_sim": sc[n:], "neighbor_counts": counts, "parents": par, "n_neighbors": nn,
                "k_adj": K, "n_sim": n_sim})
    return out


def auroc(scores, positive):
    """the probability that a positive outscores a negative, ties counted half"""
    from scipy.stats import rankdata

    r = rankdata(scores)
    npos = int(positive.sum())
    nneg = positive.size - npos
    return float((r[positive].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
M_HAND = 300


@functools.lru_cache(maxsize=None)
def hand_cells():
    """(the two blocks, the parents): 40 hand-made cells of 300 genes, integer counts, and the pairs that reach every case of the merge"""
    rng = np.random.default_rng(24)
    m = M_HAND
    lists = [[], [], [0], [m - 1], range(10, 73), range(10, 74), range(10, 75), range(5, 134), range(50, 250), range(50, 250),
             range(0, m, 2), range(1, m, 2), range(100, 230), [163, 164, 290], range(36, 100), range(100, 164)]
    sizes = [1, 63, 64, 65, 129, 200, 0, 7, 30, 128, 127, 64, 192, 193, 256, 300, 2, 90, 150, 10, 64, 65, 63, 33]
    lists += [np.sort(rng.choice(m, s, replace=False)) for s in sizes]
    assert len(lists) == 40
    cols = []
    for g in lists:
        g = np.asarray(list(g), np.int32)
        cols.append(sp.csc_matrix((rng.integers(1, 10, size=g.size).astype(np.float64), g, np.array([0, g.size])), shape=(m, 1)))
    X = sp.hstack(cols, format="csc")
    X.sort_indices()
    par = [(0, 1), (0, 8), (8, 0), (5, 5), (0, 0), (8, 9), (10, 11), (11, 10), (2, 3), (2, 10), (3, 11), (2, 2), (4, 5), (5, 6), (6, 7),
           (7, 8), (12, 13), (13, 12), (14, 15), (15, 14), (5, 14), (4, 25), (30, 7), (16, 31), (17, 18), (19, 20), (21, 39), (35, 36),
           (31, 31), (29, 10), (22, 38), (37, 24), (26, 27), (28, 8), (33, 32), (34, 12), (23, 6), (9, 30), (36, 3), (38, 2)]
    return ref.ragged(X, [17]), np.array(par, np.int64)


def triangle_scores():
    """simulated scores whose 256-bin histogram is a triangle: one mode from the start"""
    cnt = np.minimum(np.arange(BINS), BINS - 1 - np.arange(BINS)) + 1
    centre = (np.arange(BINS) + 0.5) / BINS
    sim = np.repeat(centre, cnt)
    return np.concatenate([[0.0], sim, [1.0]])              # (the ends pin min and max; they fall into bins 0 and 255)


def two_mode_scores(seed=3):
    """(observed, simulated): a mixture around 0.08 and around 0.55"""
    rng = np.random.default_rng(seed)
    sim = np.concatenate([rng.beta(4, 40, 1200), rng.beta(30, 25, 800)])
    obs = np.concatenate([rng.beta(4, 40, 900), rng.beta(30, 25, 100)])
    return obs, sim


N_QUALITY, M_QUALITY, G_QUALITY, TOP_QUALITY, SHARE_QUALITY = 1500, 800, 6, 300, 0.08


@functools.lru_cache(maxsize=None)
def quality_input():
    """(X, is_doublet): the planted input with 8 % of the cells replaced by the sum of two cells of different clusters"""
    X, lab = ref.planted(N_QUALITY, M_QUALITY, G_QUALITY)
    rng = np.random.default_rng(8)
    nd = rnd(SHARE_QUALITY * N_QUALITY)
    where = np.sort(rng.choice(N_QUALITY, nd, replace=False))
    rest = np.setdiff1d(np.arange(N_QUALITY), where)
    a = rng.choice(rest, nd)
    b = np.array([rng.choice(rest[lab[rest] != lab[i]]) for i in a])
    S = (X[:, a] + X[:, b]).tocsc()
    cols = [X[:, i] for i in range(N_QUALITY)]
    for j, i in enumerate(where):
        cols[i] = S[:, j]
    Y = sp.hstack(cols, format="csc")
    Y.sort_indices()
    is_d = np.zeros(N_QUALITY, bool)
    is_d[where] = True
    return Y, is_d


@functools.lru_cache(maxsize=None)
def quality_reference():
    """the reference on the quality input over the seeds 0 .. 4: per seed (AUROC, the share of the planted doublets above the found
    threshold), and the floors: the worst value less the seed-to-seed spread (§13's and §14's rule)"""
    X, is_d = quality_input()
    fit, genes = fit_observed(X, 30, TOP_QUALITY)
    rows = []
    for seed in range(5):
        r = scrublet(X, fit, genes, seed=seed)
        share = float(r["predicted_doublets"][is_d].mean()) if r["threshold_found"] else 0.0
        rows.append((auroc(r["doublet_scores"], is_d), share, r["threshold"]))
    au, sh = np.array([q[0] for q in rows]), np.array([q[1] for q in rows])
    return {"rows": rows, "auroc_floor": float(au.min() - (au.max() - au.min())), "share_floor": float(sh.min() - (sh.max() - sh.min()))}
