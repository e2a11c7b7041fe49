"""A numpy restatement of rank_genes_groups and the seeded inputs of its tests.  Test infrastructure.

Everything that decides a rank is an integer: 2 x average rank comes from scipy.stats.rankdata(method="average") * 2 as an int64, so
do the rank sums, U and the tie terms.  From the integers on, z is computed in longdouble; the sums behind the means and the t-test
are longdouble sums of the transformed values.  The functions return what a test needs to state its premises (the sums of |x| and
x^2, the stored counts) next to the results.

The transform is tests/_expr_pca_ref.transform.  A device log1p may differ from numpy's in the last bits, which could reorder two
values that are almost equal: rank_margin() states, on the CPU, that a case's transformed values are either bitwise equal before the
logarithm or far apart after it, so the ranks do not depend on those bits."""
import math

import numpy as np
import scipy.sparse as sp

import _expr_pca_ref as E
import _markers_ref as M

EPS = 2.0 ** -53
LD = np.longdouble


def tie_terms(A):
    """per row of A: the sum over tie groups of t^3 - t (int64)"""
    m, n = A.shape
    S = np.sort(A, axis=1)
    out = np.zeros(m, np.int64)
    for j in range(m):
        _, t = np.unique(S[j], return_counts=True)
        t = t.astype(np.int64)
        out[j] = int((t * t * t - t).sum())
    return out


def bh(p):
    """Benjamini-Hochberg of one vector (NaN in, NaN out): sorted ascending (stable), p m / rank, the running minimum from the top"""
    p = np.asarray(p, np.float64)
    if np.isnan(p).any():
        assert np.isnan(p).all()
        return p.copy()
    m = p.size
    o = np.argsort(p, kind="stable")
    v = p[o] * (float(m) / np.arange(1, m + 1))
    v = np.minimum.accumulate(np.minimum(v, 1.0)[::-1])[::-1]
    out = np.empty(m)
    out[o] = v
    return out


def order_of(scores):
    """per row: the genes by score descending, ties to the lower gene, NaN last"""
    s = np.asarray(scores, np.float64)
    key = np.where(np.isnan(s), np.inf, -(s + 0.0))
    return np.argsort(key, axis=1, kind="stable").astype(np.int64)


def dense(blocks, normalize_total=1e4, log1p=True, genes=None):
    """(A, U): the transformed values as a dense m x n array (the kept genes' rows), and the values before the logarithm"""
    T, _ = E.transform(blocks, normalize_total, log1p)
    U, _ = E.transform(blocks, normalize_total, False)
    A, Ud = T.toarray(), U.toarray()
    if genes is not None:
        A, Ud = A[np.asarray(genes)], Ud[np.asarray(genes)]
    return A + 0.0, Ud + 0.0


def rank_margin(blocks, normalize_total=1e4, log1p=True):
    """the smallest relative gap between two distinct transformed values of one gene; asserts that values equal after the logarithm
    were equal before it.  With no logarithm the device's values are the reference's bit for bit (one product of the same doubles) and
    the margin is not needed: inf."""
    if not log1p:
        return np.inf
    A, U = dense(blocks, normalize_total, log1p)
    worst = np.inf
    for j in range(A.shape[0]):
        o = np.argsort(U[j], kind="stable")
        a, u = A[j, o], U[j, o]
        du, da = np.diff(u) != 0, np.diff(a)
        assert np.array_equal(du, da != 0), "a tie made or broken by the logarithm's rounding"
        if du.any():
            worst = min(worst, float((da[du] / np.maximum(np.abs(a[1:][du]), 1e-300)).min()))
    return worst


def reference(blocks, codes, G, method="wilcoxon", ref=-1, normalize_total=1e4, log1p=True, genes=None, tie_correct=True, continuity=False):
    """the whole table.  codes: dense group codes.  Returns a dict of G x m arrays: the integers rank2, ties, nz; the float64 results
    scores, pvals, pvals_adj, logfoldchanges, auc, means, means_ref, pct, pct_ref, df, order; and the premises sumabs / sumsq / stored of the
    group and of what it is tested against (suffix _ref), sizes n_g / n_r."""
    from scipy.special import erfc
    from scipy.stats import rankdata
    from scipy.stats import t as tdist

    A, _ = dense(blocks, normalize_total, log1p, genes)
    T, _ = E.transform(blocks, normalize_total, log1p)
    stored = np.zeros(T.shape, bool)                          # the pattern of stored entries (explicit zeros count as stored)
    Tc = sp.csc_matrix(T)
    stored[Tc.indices, np.repeat(np.arange(T.shape[1]), np.diff(Tc.indptr))] = True
    if genes is not None:
        stored = stored[np.asarray(genes)]
    m, n = A.shape
    codes = np.asarray(codes, np.int64)
    sizes = np.bincount(codes, minlength=G).astype(np.int64)
    assert codes.shape == (n,) and sizes.min() > 0
    names_f = ("scores", "pvals", "pvals_adj", "logfoldchanges", "auc", "means", "means_ref", "pct", "pct_ref", "df", "sumabs", "sumabs_ref",
               "sumsq", "sumsq_ref", "z_exact")
    out = {k: np.full((G, m), np.nan) for k in names_f}
    for k in ("rank2", "ties", "nz", "nz_ref", "stored", "stored_ref"):
        out[k] = np.full((G, m), -1, np.int64)
    out["n_g"], out["n_r"] = sizes.copy(), np.where(np.arange(G) == ref, 0, (n - sizes) if ref < 0 else sizes[max(ref, 0)])
    all_ties = tie_terms(A) if ref < 0 else None
    r2_all = np.rint(2.0 * rankdata(A, method="average", axis=1)).astype(np.int64) if ref < 0 else None
    AL, A2 = A.astype(LD), A.astype(LD) ** 2
    for g in range(G):
        if g == ref:
            continue
        in_g = codes == g
        other = ~in_g if ref < 0 else codes == ref
        ng, nr = int(in_g.sum()), int(other.sum())
        N = ng + nr
        if ref < 0:
            R2, tie = r2_all[:, in_g].sum(1), all_ties
        else:
            S = in_g | other
            sub = A[:, S]
            R2 = np.rint(2.0 * rankdata(sub, method="average", axis=1)).astype(np.int64)[:, in_g[S]].sum(1)
            tie = tie_terms(sub)
        U2 = R2 - ng * (ng + 1)
        out["rank2"][g], out["ties"][g] = R2, tie
        out["nz"][g], out["nz_ref"][g] = (A[:, in_g] != 0).sum(1), (A[:, other] != 0).sum(1)
        out["stored"][g], out["stored_ref"][g] = stored[:, in_g].sum(1), stored[:, other].sum(1)
        sg, sr = AL[:, in_g].sum(1), AL[:, other].sum(1)
        qg, qr = A2[:, in_g].sum(1), A2[:, other].sum(1)
        out["sumabs"][g], out["sumabs_ref"][g] = np.abs(A[:, in_g]).sum(1), np.abs(A[:, other]).sum(1)
        out["sumsq"][g], out["sumsq_ref"][g] = qg.astype(np.float64), qr.astype(np.float64)
        mg, mr = sg / ng, sr / nr
        out["means"][g], out["means_ref"][g] = mg.astype(np.float64), mr.astype(np.float64)
        out["pct"][g], out["pct_ref"][g] = out["nz"][g] / float(ng), out["nz_ref"][g] / float(nr)
        out["auc"][g] = (U2.astype(LD) / LD(2 * ng * nr)).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            if log1p:
                lfc = np.log2((np.expm1(mg) + LD(1e-9)) / (np.expm1(mr) + LD(1e-9)))
            else:
                lfc = np.log2((mg + LD(1e-9)) / (mr + LD(1e-9)))
        out["logfoldchanges"][g] = lfc.astype(np.float64)
        if method == "wilcoxon":
            n3 = N * N * N - N
            Tcorr = (LD(n3) - tie.astype(LD)) / LD(n3) if tie_correct else np.ones(m, LD)
            sig2 = LD(ng) * LD(nr) * LD(N + 1) / LD(12) * Tcorr
            d2 = U2 - ng * nr
            d = d2.astype(LD) / 2 - (np.sign(d2).astype(LD) / 2 if continuity else 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                z = np.where(sig2 > 0, d / np.sqrt(np.where(sig2 > 0, sig2, 1)), LD(0))
            zf = z.astype(np.float64)
            out["scores"][g], out["z_exact"][g] = zf, zf
            out["pvals"][g] = np.where(sig2 > 0, erfc(np.abs(zf) / math.sqrt(2.0)), 1.0)
            out["df"][g] = 0.0
        else:
            assert ng >= 2 and nr >= 2
            vg = np.maximum(qg - ng * mg * mg, 0) / (ng - 1) / ng
            vr = np.maximum(qr - nr * mr * mr, 0) / (nr - 1) / nr
            some = (vg + vr) > 0
            with np.errstate(invalid="ignore", divide="ignore"):
                t = np.where(some, (mg - mr) / np.sqrt(np.where(some, vg + vr, 1)), LD(0))
                df = np.where(some, (vg + vr) ** 2 / np.where(some, vg * vg / (ng - 1) + vr * vr / (nr - 1), 1), LD(0))
            tf, dff = t.astype(np.float64), df.astype(np.float64)
            out["scores"][g], out["df"][g] = tf, dff
            out["pvals"][g] = np.where(some, 2.0 * tdist.sf(np.abs(tf), np.where(some, dff, 1.0)), 1.0)
        out["pvals_adj"][g] = bh(out["pvals"][g])
    out["order"] = order_of(out["scores"])
    out["sizes"] = sizes
    return out


def score_margin(scores, bound):
    """the premise of the order check: per group, two neighbouring reference scores are exactly tied or further apart than the sum of
    their bounds.  Returns the smallest (gap / bound sum) over the untied neighbours (inf if none); asserts it exceeds 1."""
    worst = np.inf
    for g in range(scores.shape[0]):
        s = scores[g]
        if np.isnan(s).all():
            continue
        o = np.argsort(-s, kind="stable")
        gap = -np.diff(s[o])
        need = bound[g][o][1:] + bound[g][o][:-1]
        live = gap > 0
        if live.any():
            worst = min(worst, float((gap[live] / np.maximum(need[live], 1e-300)).min()))
    assert worst > 1.0, f"two reference scores closer than their bounds ({worst:.3g})"
    return worst


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------------

def _primes(k, above):
    out, c = [], above + 1
    while len(out) < k:
        if all(c % d for d in range(2, int(c ** 0.5) + 1)):
            out.append(c)
        c += 1
    return np.array(out, np.int64)


def count_case(n, m, G, seed, chunk, sizes=None, share=6):
    """whole-number counts for the transformed path: m genes x n cells, gene g raised in group g % G.  The last gene fills every cell's
    total up to a prime above every count, `share` cells to a prime: two cells' normalised values are then equal only for equal counts
    and equal totals, so the logarithm's rounding decides no rank (rank_margin() asserts it).  Planted rows:
      0  no stored entry            1  stored in every cell (n > 2 chunks: several chunks of the statistics kernel)
      2  heavy ties from small counts, dense     3  stored explicit zeros and -0.0 among counts
    Returns (X csc with the explicit zeros kept, codes)."""
    rng = np.random.default_rng(seed)
    assert n > 2 * chunk and m >= 8
    if sizes is None:
        codes = rng.permutation(np.arange(n) % G)
    else:
        codes = rng.permutation(np.repeat(np.arange(G), sizes))
    D = M.count_matrix(rng, m, (codes + 1).astype(np.int32), G, density=0.12)
    D[0] = 0.0
    D[1] = rng.integers(1, 40, n) + 6.0 * (codes == 1 % G)
    D[2] = rng.integers(0, 3, n) + (codes == 0) * rng.integers(0, 2, n)
    D[m - 1] = 0.0
    tot = D.sum(0)
    primes = _primes((n + share - 1) // share, int(max(tot.max(), D.max())) + 1)
    D[m - 1] = np.repeat(primes, share)[:n][rng.permutation(n)] - tot
    assert D[m - 1].min() >= 1
    X = sp.csc_matrix(D).tolil()
    X = sp.csc_matrix(X)
    # explicit zeros and -0.0 in gene 3, at cells where it holds nothing
    free = np.flatnonzero(D[3] == 0)[:40]
    Z = sp.csc_matrix((np.where(np.arange(free.size) % 2 == 0, 0.0, -0.0), (np.full(free.size, 3), free)), shape=X.shape)
    X = _add_pattern(X, Z)
    return X, codes.astype(np.int32)


def _add_pattern(X, Z):
    """X with Z's stored entries added to its pattern, values kept as they are (explicit zeros survive)"""
    X, Z = sp.coo_matrix(X), sp.coo_matrix(Z)
    row, col, dat = np.concatenate([X.row, Z.row]), np.concatenate([X.col, Z.col]), np.concatenate([X.data, Z.data])
    o = np.lexsort((row, col))
    row, col, dat = row[o], col[o], dat[o]
    assert not ((np.diff(row) == 0) & (np.diff(col) == 0)).any()
    ptr = np.zeros(X.shape[1] + 1, np.int64)
    np.add.at(ptr, col + 1, 1)
    return sp.csc_matrix((dat, row.astype(np.int32), np.cumsum(ptr).astype(np.int32)), shape=X.shape)


def raw_case(n, m, G, seed, chunk, sizes=None):
    """values for the path without a transform (normalize_total=None, log1p=False): float32-exact, so get_marker_genes sees the same
    numbers.  Planted rows:
      0  no stored entry     1  continuous, stored in every cell, no ties     2  all equal and non-zero (sigma = 0)
      3  negatives, stored zeros, -0.0 and positives, with ties in all three: the zero run sits in the middle of the list
      4  heavy ties from small integer counts     5  continuous with negatives, half the cells
    the rest: sparse counts, gene g raised in group g % G.  Returns (X csc, codes)."""
    rng = np.random.default_rng(seed)
    assert n > 2 * chunk and m >= 8
    if sizes is None:
        codes = rng.permutation(np.arange(n) % G)
    else:
        codes = rng.permutation(np.repeat(np.arange(G), sizes))
    lab = (codes + 1).astype(np.int32)
    D = M.count_matrix(rng, m, lab, G, density=0.15)
    D[0] = 0.0
    D[1] = M.continuous_gene(rng, lab, n)
    D[2] = 2.5
    D[3] = rng.choice(np.array([-2.0, -0.5, -0.5, 0.0, 0.0, 0.5, 0.5, 7.0]), n) + 3.0 * (codes == 2 % G) * (rng.random(n) < 0.3)
    D[4] = rng.integers(0, 4, n) + (codes == 0) * rng.integers(0, 3, n)
    D[5] = M.continuous_gene(rng, lab, n // 2, negative=True)
    X = sp.csc_matrix(D)
    free = np.flatnonzero(D[3] == 0)[:60]
    Z = sp.csc_matrix((np.where(np.arange(free.size) % 2 == 0, 0.0, -0.0), (np.full(free.size, 3), free)), shape=X.shape)
    return _add_pattern(X, Z), codes.astype(np.int32)


def pairs_case(chunk, seed=5):
    """G = 1024 groups of two cells, n = 2048, no transform"""
    return raw_case(2048, 24, 1024, seed, min(chunk, 1000))


def planted_case(seed=9):
    """the planted-cluster counts of _markers_ref.count_matrix: gene g is raised in group g % G"""
    rng = np.random.default_rng(seed)
    n, m, G = 1200, 60, 5
    codes = rng.permutation(np.arange(n) % G)
    D = M.count_matrix(rng, m, (codes + 1).astype(np.int32), G, density=0.3, effect=6.0)
    return sp.csc_matrix(D), codes.astype(np.int32), G
