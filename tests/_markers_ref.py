"""A numpy restatement of get_marker_genes' per-gene pass (R/get_marker_genes.R:120-152) and the seeded inputs of the marker tests.
Test infrastructure.  Written from the R lines: rank() with average ranks over all cells, aggregate(..., mean) per cluster, order(-mean
rank)[1:rr], ROCR's auc (== Mann-Whitney U / (n1 n2)), which.max (the first maximum, in the order the clusters were tried), wilcox.test's
normal approximation with continuity and tie correction, and the fold change mean(cluster) / max(mean(other clusters)).

Everything that decides something is an integer: 2 x rank is an int64, so are the per-cluster rank sums and the tie term, and ties between
mean ranks or AUROCs are found by cross-multiplying the integers, never by comparing rounded quotients."""
import math

import numpy as np

EPS53 = 2.0 ** -53


def rank_sums(X, label, G):
    """the part of marker_stats that does not depend on theta or ng (the ranking is most of its time): pass it on as `pre` when the same
    input is needed at several ng"""
    from scipy.stats import rankdata

    X = np.ascontiguousarray(X, np.float64)
    m, n = X.shape
    label = np.asarray(label, np.int64)
    assert label.shape == (n,) and label.min() >= 1 and label.max() <= G and n < 46000          # (n < 46000: the int64 cross products)
    csize = np.bincount(label - 1, minlength=G).astype(np.int64)
    assert csize.min() > 0
    order = np.argsort(label, kind="stable")
    starts = np.concatenate([[0], np.cumsum(csize)[:-1]])
    r2 = np.rint(2.0 * rankdata(X, method="average", axis=1)).astype(np.int64)          # 2 x average rank: exact
    assert np.array_equal(r2.sum(1), np.full(m, n * (n + 1), np.int64))
    s2 = np.add.reduceat(r2[:, order], starts, axis=1)                        # (m, G) int64
    del r2
    S = np.sort(X, axis=1)                                                    # the tie term
    new = np.ones((m, n), bool)
    new[:, 1:] = S[:, 1:] != S[:, :-1]
    at = np.flatnonzero(new.ravel())
    t = np.diff(np.append(at, m * n)).astype(np.int64)                        # run lengths; a run never crosses a row (each row opens one)
    tie3 = np.add.reduceat(t * t * t - t, np.flatnonzero(at % n == 0))
    return {"csize": csize, "order": order, "starts": starts, "s2": s2, "tie3": tie3, "shape": (m, n, G)}


def marker_stats(X, label, G, theta=1e-4, ng=1, pre=None):
    """X: (m, n) genes x cells, float64.  label: 1..G, every cluster non-empty.  Returns (table, info): table (m, 5) = (auc, icluster,
    pvalue, sparsity, FC); info holds what a test needs to state its premises, per gene:
      mr_margin   mean rank of the picked (first tried) cluster minus the next one's; exactly 0 for an exact tie; inf where sparsity <= theta
      mr_tie      that tie, decided on integers
      auc_margin  best AUROC minus the second-best among the tried clusters (inf if only one was tried)
      auc_tie     the two are the same rational number
      sumabs      (m, G) sum |x| per cluster;  sumx (m, G) the exact sums, rounded once;  csize (G,)
      counts      the gene's values are all whole numbers (every partial sum is then exact in a double, in any order)
      s2          (m, G) 2 x rank sums;  tie3 (m,) sum over tie groups of t^3 - t;  tried (m, rr) the clusters in the order they were tried"""
    from scipy.special import erfc

    X = np.ascontiguousarray(X, np.float64)
    m, n = X.shape
    pre = rank_sums(X, label, G) if pre is None else pre
    assert pre["shape"] == (m, n, G)
    csize, order, starts, s2, tie3 = pre["csize"], pre["order"], pre["starts"], pre["s2"], pre["tie3"]
    Xo = X[:, order]                                                          # clusters are contiguous column ranges now

    nz = np.count_nonzero(X, axis=1)
    dp = nz / float(n)
    live = dp > theta
    rr = max(1, min(int(ng), G))

    # order(-s$r)[1:rr]: a mean rank is s2 / (2 csize), one correctly rounded division of two integers below 2^53 -- equal rationals
    # give equal doubles, and distinct ones differ by at least 2 / n^2, far above an ulp of n: the stable sort of the doubles is exact
    mr = s2 / (2.0 * csize)
    tried = np.argsort(-mr, axis=1, kind="stable")[:, :rr]                    # (m, rr), 0-based
    rows = np.arange(m)
    if G > 1:
        first2 = np.argsort(-mr, axis=1, kind="stable")[:, :2]
        a, b = first2[:, 0], first2[:, 1]
        mr_margin = mr[rows, a] - mr[rows, b]
        mr_tie = s2[rows, a] * csize[b] == s2[rows, b] * csize[a]
        assert np.array_equal(mr_tie, mr_margin == 0.0)
    else:
        mr_margin, mr_tie = np.full(m, np.inf), np.zeros(m, bool)

    # ROCR's auc of the ranks against "is in cluster c": (R1 - n1 (n1 + 1) / 2) / (n1 n2), as one quotient of integers
    n1 = csize[tried]                                                         # (m, rr)
    num = np.take_along_axis(s2, tried, 1) - n1 * (n1 + 1)
    den = 2 * n1 * (n - n1)
    auc_tried = num / den.astype(np.float64)
    pos = np.argmax(auc_tried, axis=1)                                        # which.max: the first maximum
    best = tried[rows, pos]
    auc = auc_tried[rows, pos]
    if rr > 1:
        rest = auc_tried.copy()
        rest[rows, pos] = -np.inf
        pos2 = np.argmax(rest, axis=1)
        auc_margin = auc - rest[rows, pos2]
        assert np.abs(num).max() < 2 ** 31 * n and den.max() < 2 ** 31
        auc_tie = num[rows, pos] * den[rows, pos2] == num[rows, pos2] * den[rows, pos]
    else:
        auc_margin, auc_tie = np.full(m, np.inf), np.zeros(m, bool)

    # wilcox.test(x1, x2): W - n1 n2 / 2 = (s2 - n1 (n + 1)) / 2, continuity 0.5 towards zero, sigma with the tie term
    b1 = csize[best]
    b2 = n - b1
    A = s2[rows, best] - b1 * (n + 1)                                         # 2 (W - n1 n2 / 2), an integer
    znum = (A - np.sign(A)) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.sqrt((b1 * b2 / 12.0) * ((n + 1.0) - tie3 / (float(n) * (n - 1.0))))
        p = erfc(np.abs(znum / sigma) / math.sqrt(2.0))

    # aggregate(r0 ~ ig, mean): exact sums.  Whole-number genes sum exactly in doubles; the others go through math.fsum
    sumx = np.add.reduceat(Xo, starts, axis=1)
    sumabs = np.add.reduceat(np.abs(Xo), starts, axis=1)
    counts = np.all(Xo == np.rint(Xo), axis=1) & (sumabs.sum(1) < 2.0 ** 52)
    ends = starts + csize
    for g in np.flatnonzero(~counts & live):
        row = Xo[g]
        sumx[g] = [math.fsum(row[s:e][row[s:e] != 0.0].tolist()) for s, e in zip(starts, ends)]
    mean = sumx / csize
    y1 = mean[rows, best]
    other = mean.copy()
    other[rows, best] = -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        fc = y1 / other.max(1)

    table = np.zeros((m, 5))
    table[:, 0] = np.where(live, auc, 0.0)
    table[:, 1] = np.where(live, best + 1, 0)
    table[:, 2] = np.where(live, p, 1.0)
    table[:, 3] = dp
    table[:, 4] = np.where(live, fc, 0.0)
    info = {"mr_margin": np.where(live, mr_margin, np.inf), "mr_tie": mr_tie & live, "auc_margin": np.where(live, auc_margin, np.inf),
            "auc_tie": auc_tie & live, "sumabs": sumabs, "sumx": sumx, "csize": csize, "counts": counts, "s2": s2, "tie3": tie3,
            "tried": tried, "live": live, "mean_rank": mr, "pre": pre}
    return table, info


def fc_bound(table, info):
    """Relative bound on FC = y1 / y2 for a sum of n_c doubles added in ANY order (an LDS atomic sum): each cluster sum is within
    n_c 2^-53 sum|x| of exact, so the quotient is within e1 / |y1| + e2 / |y2| + 2^-51 (the two divisions by the sizes and the quotient).
    Whole-number genes: every partial sum is an exact integer, e = 0.  Returns (m,) with inf where FC is not finite or sparsity <= theta
    (those rows are compared for equality instead)."""
    m = table.shape[0]
    csize, sumabs, sumx = info["csize"], info["sumabs"], info["sumx"]
    mean = sumx / csize
    rows = np.arange(m)
    best = np.maximum(table[:, 1].astype(np.int64) - 1, 0)
    other = mean.copy()
    other[rows, best] = -np.inf
    second = np.argmax(other, axis=1)
    e = csize * EPS53 * sumabs * (1.0 + 2.0 ** -40)                           # absolute error of each cluster SUM
    e[info["counts"]] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = e[rows, best] / np.abs(sumx[rows, best]) + e[rows, second] / np.abs(sumx[rows, second]) + 2.0 ** -51
    return np.where(np.isfinite(table[:, 4]) & info["live"] & (table[:, 4] != 0.0), rel, np.inf)


def holm(p):
    """stats::p.adjust(p, "holm")"""
    p = np.asarray(p, np.float64)
    k = p.size
    o = np.argsort(p, kind="stable")
    out = np.empty(k)
    out[o] = np.minimum(1.0, np.maximum.accumulate((k - np.arange(k)) * p[o]))
    return out


# ---- seeded inputs.  Every value is built in float32 and widened: the block format is fp32 and sharp_marker_genes casts to it ----------

def labels_of_sizes(rng, sizes):
    """a shuffled label vector 1..G with the given cluster sizes"""
    lab = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    rng.shuffle(lab)
    return lab.astype(np.int32)


def balanced_labels(rng, n, G):
    sizes = np.full(G, n // G)
    sizes[: n % G] += 1
    return labels_of_sizes(rng, sizes)


def count_matrix(rng, m, label, G, density=0.15, lam=3.0, effect=4.0, up_density=None):
    """sparse whole-number counts: gene g is raised in cluster g % G.  (m, n) float64 holding fp32-exact values."""
    n = label.size
    up = (np.arange(m)[:, None] % G) == (label[None, :] - 1)
    X = rng.poisson(np.where(up, lam * effect, lam)).astype(np.float32)
    up_density = min(1.0, 3 * density) if up_density is None else up_density
    X *= rng.random((m, n), dtype=np.float32) < np.where(up, np.float32(up_density), np.float32(density))
    return X.astype(np.float64)


def continuous_gene(rng, label, k, shift=1.0, negative=False):
    """k non-zero fp32 values at random cells (the rest zero); cluster 1's cells are shifted up"""
    n = label.size
    x = np.zeros(n, np.float32)
    at = rng.choice(n, k, replace=False)
    v = rng.gamma(2.0, 1.0, k).astype(np.float32) + np.float32(shift) * (label[at] == 1)
    if negative:
        v = np.where(rng.random(k) < 0.4, -v, v).astype(np.float32)
    x[at] = np.where(v == 0, np.float32(1.0), v)
    return x.astype(np.float64)


def case_two_tiles(seed=11):
    """m = 16384 + 37, n = 600, G = 4: a second gene tile with a ragged width of 37.  No n1 (n - n1) is a multiple of 5, so no AUROC
    = k / (2 n1 n2) can be exactly 0.7 or 0.85, the thresholds of the front ends' selections"""
    rng = np.random.default_rng(seed)
    m, n, G = 16384 + 37, 600, 4
    label = labels_of_sizes(rng, [171, 149, 158, 122])
    X = count_matrix(rng, m, label, G, density=0.2, up_density=0.9)
    X[16383] = continuous_gene(rng, label, n)                                 # last gene of tile 0: dense, no zero
    X[16384] = 0.0                                                            # first gene of tile 1: all zero
    X[m - 1] = 0.0
    X[m - 1, [5, 17, 400]] = [2.5, 0.5, 0.5]                                  # last gene of the ragged tile: three non-zeros
    X[7] = 0.0
    X[16390] = continuous_gene(rng, label, 300, negative=True)
    return X, label, G


def case_full_tile(seed=12):
    """m = 16384 exactly, n = 64, G = 2: whole-number counts, so every gene has ties (the normal approximation is what R uses too)"""
    rng = np.random.default_rng(seed)
    m, n, G = 16384, 64, 2
    label = labels_of_sizes(rng, [35, 29])
    X = count_matrix(rng, m, label, G, density=0.4)
    X[0] = 0.0
    X[m - 1] = 0.0
    X[m - 1, [1, 2, 63]] = [1.0, 4.0, 1.0]
    return X, label, G


LONG_LENGTHS = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 2175, 2176, 2177]


def case_long_lists(seed=13):
    """m = 48, n = 20011, G = 6: the gene's list length (its non-zero cells) is planted; genes 0..21 take LONG_LENGTHS, gene 22 has no
    zero at all (length n), the rest are counts of mixed density and continuous genes of lengths in between"""
    rng = np.random.default_rng(seed)
    m, n, G = 48, 20011, 6
    label = labels_of_sizes(rng, [5000, 4011, 3500, 3000, 2500, 2000])
    X = count_matrix(rng, m, label, G, density=0.3)
    for g, k in enumerate(LONG_LENGTHS):
        X[g] = continuous_gene(rng, label, k, negative=(g % 3 == 2)) if k else 0.0
    X[22] = continuous_gene(rng, label, n)
    X[23] = continuous_gene(rng, label, n - 1, negative=True)
    X[24] = X[24] + 1.0                            # whole numbers, no zero: t0 == 0 with long tie groups
    for g, k in ((25, 5000), (26, 10000), (27, 4353), (28, 2304)):
        X[g] = continuous_gene(rng, label, k, negative=(g == 26))
    return X, label, G


def case_long_many(seed=14):
    """m = 3000, n = 9001, G = 6, a tenth of the genes dense: long segments with at least partitioning_threshold segments"""
    rng = np.random.default_rng(seed)
    m, n, G = 3000, 9001, 6
    label = labels_of_sizes(rng, [2500, 2001, 1500, 1300, 1000, 700])
    X = count_matrix(rng, m, label, G, density=0.05)
    dense = np.arange(0, m, 10)
    X[dense] = count_matrix(rng, dense.size, label, G, density=0.8, lam=6.0)
    X[dense[::3]] += 1.0                                                      # no zero at all
    for g, k in ((1, 2176), (11, 2177), (21, 2048), (31, 2049), (41, 128), (51, 129), (61, n)):
        X[g] = continuous_gene(rng, label, k, negative=(g == 31))
    X[2] = 0.0
    return X, label, G


def case_many_clusters(G, seed=15):
    """m = 64, n = 4096.  G = 256: cluster 256 is ONE cell and gene 5 is high in that cell alone, so it is gene 5's best cluster"""
    rng = np.random.default_rng(seed + G)
    m, n = 64, 4096
    sizes = np.full(G, n // G)
    sizes[: n % G] += 1
    if G == 256:
        sizes[-1] = 1
        sizes[0] += n // G - 1
    label = labels_of_sizes(rng, sizes)
    X = count_matrix(rng, m, label, G, density=0.5, lam=5.0)
    X[3] = continuous_gene(rng, label, n)
    X[4] = continuous_gene(rng, label, 1000, negative=True)
    if G == 256:
        X[5] = np.minimum(X[5], 20.0)
        X[5, label == 256] = 1000.0
    return X, label, G


RANK_N, RANK_G, RANK_THETA = 2000, 4, 1e-3


def case_rank_arithmetic(seed=16):
    """m = 40 planted genes, n = 2000, G = 4 clusters of 500 cells: label = 1 + (cell % 4).  Returns X, label, G and the gene indices."""
    rng = np.random.default_rng(seed)
    m, n, G = 40, RANK_N, RANK_G
    label = (1 + np.arange(n) % G).astype(np.int32)
    X = count_matrix(rng, m, label, G, density=0.3)
    idx = {}
    f = np.float32
    # negative tie groups: few distinct negative values, many cells each
    g = idx["negative_ties"] = 0
    X[g] = rng.choice(np.array([-3.0, -1.5, -1.5, -0.25, 0.0, 0.0], f), n).astype(np.float64) - 1.0 * (label == 2) * (rng.random(n) < 0.5)
    # negatives, zeros and positives in one gene, with ties in all three
    g = idx["three_signs"] = 1
    X[g] = rng.choice(np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 0.5, 7.0], f), n).astype(np.float64) + 3.0 * (label == 3) * (rng.random(n) < 0.3)
    # no zero at all: t0 == 0
    g = idx["no_zero"] = 2
    X[g] = rng.integers(1, 6, n).astype(np.float64) + 2.0 * (label == 4)
    g = idx["no_zero_signed"] = 3
    X[g] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.integers(1, 4, n) + 1.5 * (label == 1)
    # sparsity == theta exactly: 2 non-zeros of 2000 against theta = 1e-3 -> not > theta -> (0, 0, 1, theta, 0)
    g = idx["at_theta"] = 4
    X[g] = 0.0
    X[g, [10, 11]] = [3.0, 9.0]
    g = idx["just_above_theta"] = 5
    X[g] = 0.0
    X[g, [10, 11, 12]] = [3.0, 9.0, 1.0]
    # equal mean ranks of the two best clusters (2 and 3; 1 and 4 lower): the same multiset of values in both
    g = idx["equal_mean_rank"] = 6
    X[g] = 0.0
    vals = rng.integers(1, 9, 120).astype(np.float64)
    c2, c3, c1 = np.flatnonzero(label == 2), np.flatnonzero(label == 3), np.flatnonzero(label == 1)
    X[g, rng.choice(c2, 120, replace=False)] = vals
    X[g, rng.choice(c3, 120, replace=False)] = rng.permutation(vals)
    X[g, rng.choice(c1, 40, replace=False)] = rng.integers(1, 9, 40)
    # equal AUROC with ng = 4: clusters 3 and 4 hold the same values and beat 1 and 2, a continuous gene (no other ties among non-zeros)
    g = idx["equal_auroc"] = 7
    X[g] = 0.0
    v = (rng.gamma(2.0, 1.0, 200).astype(f) + f(0.5)).astype(np.float64)
    c4 = np.flatnonzero(label == 4)
    X[g, rng.choice(c3, 200, replace=False)] = v
    X[g, rng.choice(c4, 200, replace=False)] = rng.permutation(v)
    X[g, rng.choice(c1, 50, replace=False)] = rng.gamma(2.0, 1.0, 50).astype(f)
    # all cells the same non-zero value: sigma = 0, p = NaN
    g = idx["all_tied"] = 8
    X[g] = 2.5
    # non-zero in one cluster only: the other means are 0, FC = inf
    g = idx["one_cluster_only"] = 9
    X[g] = 0.0
    X[g, rng.choice(c2, 77, replace=False)] = rng.integers(1, 5, 77)
    # -0.0 is a zero: in a dense block it fails x != 0; in a sparse block it is a STORED entry that must be dropped
    g = idx["minus_zero"] = 10
    X[g, ::3] = -0.0
    # mixed sign with heavy cancellation in the cluster sums
    g = idx["cancelling"] = 11
    base = rng.gamma(2.0, 100.0, n // 2).astype(f)
    x = np.zeros(n, f)
    x[0::2] = base
    x[1::2] = -base * f(1.0 + 2.0 ** -10)
    x[label == 1] += f(0.125)
    X[g] = x
    return X, label, G, idx


def case_layouts(seed=17):
    """m = 130, four blocks of 400 / 0 / 1 / 650 cells, G = 5"""
    rng = np.random.default_rng(seed)
    m, G = 130, 5
    sizes = [400, 0, 1, 650]
    n = sum(sizes)
    label = balanced_labels(rng, n, G)
    X = count_matrix(rng, m, label, G, density=0.2)
    X[3] = continuous_gene(rng, label, n)
    X[4] = continuous_gene(rng, label, 500, negative=True)
    X[5] = 0.0
    X[m - 1] = continuous_gene(rng, label, 40)
    return X, label, G, sizes
