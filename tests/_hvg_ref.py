"""Variable-gene selection and the gene subset of DESIGN.md §22, restated in numpy, and the tests' case builders.

Selection (raw counts, genes x cells): mu and var are §21's gene statistics of the untransformed values.  Over the N genes with var > 0,
x = log10 mu and y = log10 var; the loess below gives fit; sigma^2 = 10^fit, clip = mu + sigma sqrt(n), and
vs = (sum over the stored entries of (min(x, clip) - mu)^2 + (n - stored) mu^2) / ((n - 1) sigma^2), 0 for a constant gene.  The genes
are ordered by vs descending, ties by the lower index; the first min(n_top_genes, N) are selected.

Loess at point i (no robustness iterations): q = min(N, max(3, ceil(span N))); h = the q-th smallest |x_j - x_i| (j = i counted), taken
in float64 whatever the sums' type; h = 0: the mean of y over x_j = x_i; else the points with |x_j - x_i| < h, u = (x_j - x_i) / h,
w = (1 - |u|^3)^3, S_k = sum w u^k, T_k = sum w y u^k, and the intercept of the weighted quadratic by LDL^T without pivoting: p0 = S0,
p1 = S2 - S1^2 / S0, p2 the Schur complement; degree 1 when p2 <= 2^-30 S0, degree 0 (the weighted mean) when p1 <= 2^-30 S0.  The sums run
in `dtype` (float64 or longdouble), so that the reference states its own rounding.

Subset: transform the full matrix, take the rows, then _expr_pca_ref.pca(..., normalize_total=None, log1p=False) on the result."""
import functools

import numpy as np
import scipy.sparse as sp

import _expr_pca_ref as ref

PIVOT = 2.0 ** -30


def loess_q(N, span):
    return int(min(N, max(3, int(np.ceil(span * N)))))


def loess(x, y, span=0.3, dtype=np.float64):
    """{"fit", "bandwidth", "degree", "p1", "p2" (the pivots over S0; nan where none was formed), "window" (the points that took part)}
    at every point, in the caller's order"""
    x, y = np.asarray(x, np.float64) + 0.0, np.asarray(y, np.float64)
    N = x.size
    q = loess_q(N, span)
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order].astype(dtype)
    xd = xs.astype(dtype)
    out = {key: np.zeros(N) for key in ("fit", "bandwidth")}
    out.update(degree=np.zeros(N, np.int64), window=np.zeros(N, np.int64), p1=np.full(N, np.nan), p2=np.full(N, np.nan))
    for i in range(N):
        xi = xs[i]
        a, b = max(0, i - q + 1), min(N, i + q)
        h = np.partition(np.abs(xs[a:b] - xi), q - 1)[q - 1]                     # (the q nearest lie within q places of i)
        if h > 0:
            lo = a + int(np.searchsorted(-(xi - xs[a:i + 1]), -h, side="right"))   # the first j with x_i - x_j < h
            hi = i + int(np.searchsorted(xs[i:b] - xi, h, side="left"))          # the first j with x_j - x_i >= h
        else:
            lo, hi = int(np.searchsorted(xs, xi, side="left")), int(np.searchsorted(xs, xi, side="right"))
        s = order[i]
        out["bandwidth"][s], out["window"][s] = h, hi - lo
        if not h > 0:
            out["fit"][s] = float(ys[lo:hi].sum(dtype=dtype) / dtype(hi - lo))
            continue
        u = (xd[lo:hi] - xd[i]) / dtype(h)
        c = 1 - np.abs(u) ** 3
        w = c * c * c
        u2 = u * u
        wy = w * ys[lo:hi]
        S0, S1, S2, S3, S4 = w.sum(), (w * u).sum(), (w * u2).sum(), (w * (u2 * u)).sum(), (w * (u2 * u2)).sum()
        T0, T1, T2 = wy.sum(), (wy * u).sum(), (wy * u2).sum()
        l10, l20 = S1 / S0, S2 / S0
        p1 = S2 - S1 * l10
        out["p1"][s] = float(p1 / S0)
        if not p1 > PIVOT * S0:
            out["fit"][s] = float(T0 / S0)
            continue
        l21 = (S3 - l20 * S1) / p1
        p2 = S4 - l20 * S2 - l21 * l21 * p1
        out["p2"][s] = float(p2 / S0)
        z1 = T1 - l10 * T0
        if not p2 > PIVOT * S0:
            out["degree"][s] = 1
            out["fit"][s] = float(T0 / S0 - l10 * (z1 / p1))
            continue
        out["degree"][s] = 2
        b2 = (T2 - l20 * T0 - l21 * z1) / p2
        b1 = z1 / p1 - l21 * b2
        out["fit"][s] = float(T0 / S0 - l10 * b1 - l20 * b2)
    return out


def bandwidth_brute(x, span):
    """h_i as the q-th order statistic of |x_j - x_i| over all j, by a full sort"""
    x = np.asarray(x, np.float64)
    q = loess_q(x.size, span)
    return np.sort(np.abs(x[None, :] - x[:, None]), axis=1)[:, q - 1]


def _segment_sums(values, ptr, dtype):
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros(ptr.size - 1, dtype)
    some = np.diff(ptr) > 0
    if some.any():
        out[some] = np.add.reduceat(np.asarray(values, dtype), ptr[:-1][some])
    return out


def hvg(blocks, n_top_genes=2000, span=0.3, dtype=np.float64):
    """the selection of DESIGN.md §22 as highly_variable_genes() returns it, with the loess's own record under "loess\""""
    X = ref.concat(blocks)
    m, n = X.shape
    if X.nnz and X.data.min() < 0:
        raise ValueError("a negative value")
    mu, var, _, stored = ref.gene_stats(X)
    fg = np.flatnonzero(var > 0)
    N = fg.size
    if N < 1:
        raise ValueError("every gene is constant")
    lo = loess(np.log10(mu[fg]), np.log10(var[fg]), span, dtype)
    sig2 = np.zeros(m)
    sig2[fg] = np.power(10.0, lo["fit"])
    clip = mu + np.sqrt(sig2) * np.sqrt(float(n))
    R = X.tocsr()
    rows = np.repeat(np.arange(m), np.diff(R.indptr))
    d = np.minimum(R.data, clip[rows]).astype(dtype) - mu[rows].astype(dtype)
    SS = _segment_sums(d * d, R.indptr, dtype)
    vs = np.zeros(m)
    mud = mu.astype(dtype)
    vs[fg] = ((SS + (n - stored) * mud * mud) / ((n - 1) * sig2.astype(dtype).clip(min=np.finfo(np.float64).tiny)))[fg].astype(np.float64)
    order = fg[np.lexsort((fg, -vs[fg]))]
    ns = min(int(n_top_genes), N)
    rank = np.full(m, -1, np.int64)
    rank[order[:ns]] = np.arange(ns)
    dc = np.bincount(lo["degree"], minlength=3)
    return {"means": mu, "variances": var, "variances_expected": sig2, "variances_norm": vs, "rank": rank, "highly_variable": rank >= 0,
            "genes": np.flatnonzero(rank >= 0), "n_selected": ns, "span": span, "q": loess_q(N, span), "degree_counts": dc, "order": order,
            "clip": clip, "clipped": np.bincount(rows, weights=R.data > clip[rows], minlength=m).astype(np.int64), "stored": stored,
            "loess": lo}


def cut_gap(r, n_top):
    """the relative gap of vs across the cut at n_top: (the last selected - the first left out) / the last selected"""
    o, v = r["order"], r["variances_norm"]
    return np.inf if n_top >= o.size else (v[o[n_top - 1]] - v[o[n_top]]) / v[o[n_top - 1]]


def rel_diff(a, b, keys=("variances_expected", "variances_norm")):
    """the largest relative difference of the two results' fitted and standardised variances over the genes that vary"""
    out = 0.0
    for key in keys:
        ok = a[key] > 0
        out = max(out, float((np.abs(a[key] - b[key])[ok] / a[key][ok]).max()))
    return out


def pca_subset(blocks, genes, n_components=50, oversample=10, n_iter=4, normalize_total=1e4, log1p=True, scale=False, seed=0):
    """the fit on a gene subset: the transform of the full matrix (cell sums over all genes), the rows, then §21's fit untransformed"""
    T, _ = ref.transform(blocks, normalize_total, log1p)
    Ts = T.tocsr()[np.asarray(genes, np.int64)].tocsc()
    Ts.sort_indices()
    return ref.pca(Ts, n_components, oversample, n_iter, None, False, scale, seed)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def raised_genes(n, m, G, seed=1):
    """the genes that _expr_pca_ref.planted(n, m, G, seed) raised in some cluster (its draws replayed)"""
    rng = np.random.default_rng(seed)
    rng.gamma(0.3, size=m)
    up = np.zeros(m, bool)
    for _ in range(G):
        g = rng.choice(m, m // 10, replace=False)
        rng.uniform(3.0, 8.0, size=g.size)
        up[g] = True
    return up


@functools.lru_cache(maxsize=None)
def clip_input():
    """(X, labels, the genes given outliers): planted(1500, 800, 6) with outliers, because on planted as it stands no gene reaches its
    clip.  Twelve genes get one cell of 10^4 x their mean count: the three with the most stored entries (more than a chunk's) and nine
    spread over the range of means; five more, of moderate mean, get four such cells each."""
    X, lab = ref.planted(1500, 800, 6)
    D = X.toarray()
    mean = D.mean(1)
    by_count = np.argsort(-(D != 0).sum(1), kind="stable")
    rng = np.random.default_rng(22)
    one = np.concatenate([by_count[:3], rng.choice(np.setdiff1d(np.flatnonzero(mean > 0.01), by_count[:3]), 9, replace=False)])
    several = rng.choice(np.setdiff1d(np.flatnonzero((mean > 0.05) & (mean < 2.0)), one), 5, replace=False)
    for g in np.concatenate([one, several]):
        cells = rng.choice(D.shape[1], 1 if g in one else 4, replace=False)
        D[g, cells] = np.ceil(1e4 * mean[g])
    return sp.csc_matrix(D), lab, np.sort(np.concatenate([one, several]))


def gene_count_case(chunk):
    """genes with 0 (constant: absent), 1, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 entries, a gene present in every cell, a gene with
    the same value in every cell (constant), and forty random ones; stored zeros among the values"""
    n = 2 * chunk + 50
    counts = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, n, n] + list(np.random.default_rng(3).integers(2, 90, size=40))
    X = ref.from_gene_counts(counts, n, 4).tolil()
    X[7, :] = 3.0
    X = sp.csc_matrix(X.tocsc())
    X.sort_indices()
    return X


def tie_case():
    """(X, two groups of three genes with identical rows): planted(400, 120, 3) in which two genes on either side repeat the row of
    each of the two genes with the most counts: equal vs, the lower index wins"""
    D = ref.planted(400, 120, 3)[0].toarray()
    a, b = (int(g) for g in np.argsort(-D.sum(1), kind="stable")[:2])
    others = [g for g in (7, 90, 3, 50, 8, 91) if g not in (a, b)][:4]
    D[others[0]] = D[others[1]] = D[a]
    D[others[2]] = D[others[3]] = D[b]
    return sp.csc_matrix(D), [sorted([a, others[0], others[1]]), sorted([b, others[2], others[3]])]


def loess_cases():
    """name: (x, y, span) for the loess stage"""
    rng = np.random.default_rng(5)
    cases = {}
    for N in (1, 2, 3, 7):
        x = rng.normal(size=N)
        cases["n%d" % N] = (x, 1.0 + 0.5 * x - 0.3 * x * x, 1.0)
    for win in (63, 64, 65, 129):                                                # the lane stride: win points take part (the q-th weighs 0)
        q, N = win + 1, 2 * win + 13
        x = rng.uniform(-2.0, 1.0, size=N)                                       # negative and positive x mixed: the sort key
        cases["window%d" % win] = (x, np.sin(2 * x) + 0.1 * rng.normal(size=N), (q - 0.5) / N)
    # a tie group that straddles the window's edge: points at distance exactly h carry weight 0
    x = np.concatenate([np.arange(10.0), np.full(6, 12.0), np.arange(14.0, 30.0)])
    cases["edge_ties"] = (x, np.cos(x / 5.0), 5.5 / x.size)
    # at least q equal x: h = 0
    x = np.concatenate([np.full(9, -1.5), rng.uniform(0, 1, size=11), np.full(12, 2.0)])
    cases["h0"] = (x[rng.permutation(x.size)], rng.normal(size=x.size), 7.5 / x.size)
    # q = 7.  Windows with two distinct x within h (degree 1): at 0 the seven nearest are 0 0 0 1 1 1 5, so h = 5 and 0, 1 take part;
    # likewise at 1, 5 and 6.  Eight equal x at 20: h = 0.  One distinct x within h > 0 (degree 0): at 40 the nearest are six 40s and 41
    x = np.array([0.0] * 3 + [1.0] * 3 + [5.0] * 3 + [6.0] * 3 + [20.0] * 8 + [40.0] * 6 + [41.0])
    cases["two_one"] = (x[rng.permutation(x.size)], rng.normal(size=x.size), 6.5 / x.size)
    x = rng.normal(size=4099) * 1.3
    cases["n4099"] = (x, 0.8 * x + 0.2 * x * x + 0.3 * rng.normal(size=4099), 0.3)
    return cases


@functools.lru_cache(maxsize=None)
def loess_reference(name):
    """(the float64 run, the longdouble run) of a loess case"""
    x, y, span = loess_cases()[name]
    return loess(x, y, span, np.float64), loess(x, y, span, np.longdouble)


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """the longdouble and the float64 selection of a named input, and the reference's own rounding spread: float64 against longdouble,
    and the same input with genes and cells stored in three random orders"""
    X = {"small": lambda: ref.planted_case("small")[0], "large": lambda: ref.planted_case("large")[0], "clip": lambda: clip_input()[0]}[name]()
    want, f64 = hvg(X, dtype=np.longdouble), hvg(X)
    spread = rel_diff(want, f64)
    for sd in (11, 12, 13):
        Xp, go, co = ref.permuted(X, sd)
        p = hvg(Xp)
        back = {}
        for key in ("variances_expected", "variances_norm"):
            back[key] = np.empty_like(p[key])
            back[key][go] = p[key]
        spread = max(spread, rel_diff(f64, back))
    return {"X": X, "want": want, "f64": f64, "spread": spread}


TOL_FLOOR = 2.0 ** -52
# the n_top_genes that the GPU tests select at: the CPU test asserts the margin of each cut
N_TOP = {"small": (50, 200), "large": (200, 500), "clip": (50, 100)}
