"""CPU tests that pin tests/_markers_ref.py -- the numpy restatement of get_marker_genes' per-gene pass the GPU edge tests compare with --
against the oracle and against scipy's Mann-Whitney, and that assert the premise of every planted edge on the restatement alone."""
import numpy as np
import pytest

import _markers_ref as R


def _rel(a, b):
    """largest relative difference; equal values (inf included) and NaN on both sides count as 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.abs(b)
    d[(a == b) | (np.isnan(a) & np.isnan(b))] = 0.0
    assert not np.isnan(d).any()
    return d.max()


def _small(shape):
    m, n, G, seed = shape
    rng = np.random.default_rng(seed)
    label = R.balanced_labels(rng, n, G)
    X = R.count_matrix(rng, m, label, G, density=0.25)
    X[0] = 0.0
    X[1] = R.continuous_gene(rng, label, n)                                   # dense, no ties
    X[2] = R.continuous_gene(rng, label, n // 2, negative=True)               # negatives rank below the zeros
    X[3] = X[3] + 1.0                                                         # counts without a zero
    X[4, :] = 0.0
    X[4, :3] = [2.5, 0.5, 0.5]
    return X, label, G


@pytest.mark.parametrize("shape", [(60, 151, 3, 1), (200, 640, 7, 2), (37, 2003, 12, 3)])
def test_restatement_matches_oracle(oracle, shape):
    """icluster and sparsity equal; auc and FC within 1e-13 relative (measured: 2.2e-16 and 0: both sides are one quotient of exact
    numbers).  The p-value needs more where it is tiny: p = erfc(|z| / sqrt 2) has d ln p / d ln z ~ -z^2, so the few roundings of z on
    each side (8 half-ulps allowed here) appear multiplied by z^2.  Measured at these shapes: 6.3e-14, a third of that bound at most; on
    the GPU cases' inputs up to 2.0e-13 at z = 21 (p = 1e-102), against 8 z^2 2^-53 = 3.9e-13 there.  Where z^2 < 112 the plain 1e-13
    is what is asserted."""
    from scipy.special import erfcinv

    X, label, G = _small(shape)
    pre = None
    for ng in (1, G):
        tab, info = R.marker_stats(X, label, G, theta=1e-4, ng=ng, pre=pre)
        pre = info["pre"]
        ref = oracle.marker_genes(X, label, G, theta=1e-4, ng=ng)
        assert np.array_equal(tab[:, 1], ref[:, 1]) and np.array_equal(tab[:, 3], ref[:, 3])
        assert np.all(info["auc_tie"] | (info["auc_margin"] > 1e-9))          # the oracle's pick could not differ by a rounding
        print(shape, ng, "auc", _rel(tab[:, 0], ref[:, 0]), "FC", _rel(tab[:, 4], ref[:, 4]))
        assert _rel(tab[:, 0], ref[:, 0]) <= 1e-13 and _rel(tab[:, 4], ref[:, 4]) <= 1e-13
        z2 = 2.0 * erfcinv(np.maximum(ref[:, 2], 1e-300)) ** 2
        tol = np.maximum(1e-13, 8.0 * z2 * R.EPS53)
        with np.errstate(all="ignore"):
            d = np.abs(tab[:, 2] - ref[:, 2]) / ref[:, 2]
        d[tab[:, 2] == ref[:, 2]] = 0.0
        print(shape, ng, "p: max relative", d.max(), "max of difference / bound", (d / tol).max())
        assert np.all(d <= tol)
        assert tab[0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]


def test_restatement_matches_scipy_mannwhitney():
    """a dozen genes, a negative-valued and a dense one among them: U / (n1 n2) and the asymptotic two-sided p with continuity"""
    from scipy import stats

    X, label, G = _small((12, 640, 5, 4))
    tab, info = R.marker_stats(X, label, G, theta=1e-4, ng=G)
    checked = 0
    for g in range(12):
        if not info["live"][g]:
            continue
        c = int(tab[g, 1])
        a, b = X[g, label == c], X[g, label != c]
        u = stats.mannwhitneyu(a, b, alternative="two-sided", method="asymptotic", use_continuity=True)
        assert abs(u.statistic / (a.size * b.size) - tab[g, 0]) < 1e-13
        assert abs(u.pvalue - tab[g, 2]) <= 1e-11 * u.pvalue                  # (scipy goes through norm.sf: its own roundings times z^2)
        others = [X[g, label == k].mean() for k in range(1, G + 1) if k != c]
        assert abs(a.mean() / max(others) - tab[g, 4]) <= 1e-13 * abs(tab[g, 4])
        # the cluster is the best AUROC of all of them (ng = G tries every cluster)
        aucs = [stats.mannwhitneyu(X[g, label == k], X[g, label != k]).statistic / (np.sum(label == k) * np.sum(label != k))
                for k in range(1, G + 1)]
        assert int(np.argmax(aucs)) + 1 == c
        checked += 1
    assert checked == 11 and X[2].min() < 0 and np.count_nonzero(X[1]) == 640


def test_planted_edges_hold_on_the_reference():
    """every edge tests/test_markers_edges_gpu.py relies on is really in the input, decided on exact integers"""
    X, label, G, idx = R.case_rank_arithmetic()
    n = R.RANK_N
    assert X.shape == (40, n) and np.array_equal(np.bincount(label)[1:], [500] * 4)
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)        # fp32-exact
    t1, i1 = R.marker_stats(X, label, G, theta=R.RANK_THETA, ng=1)
    t4, i4 = R.marker_stats(X, label, G, theta=R.RANK_THETA, ng=4, pre=i1["pre"])
    s2 = i1["s2"]
    # equal mean ranks: clusters 2 and 3 have the same integer rank sum (equal sizes), above 1 and 4; the lower one is picked
    g = idx["equal_mean_rank"]
    assert s2[g, 1] == s2[g, 2] and s2[g, 1] > max(s2[g, 0], s2[g, 3]) and i1["mr_tie"][g] and i1["mr_margin"][g] == 0.0
    assert t1[g, 1] == 2.0 and t4[g, 1] == 2.0
    # equal AUROC with ng = 4: clusters 3 and 4, the same rational; which.max takes the first tried, and order() tried 3 before 4
    g = idx["equal_auroc"]
    assert s2[g, 2] == s2[g, 3] and s2[g, 2] > max(s2[g, 0], s2[g, 1]) and i4["auc_tie"][g] and i4["auc_margin"][g] == 0.0
    assert i4["tried"][g].tolist()[:2] == [2, 3] and t4[g, 1] == 3.0
    # sparsity == theta: 2 / 2000 is bitwise the double 1e-3, so "dp > theta" is false
    g = idx["at_theta"]
    assert np.count_nonzero(X[g]) == 2 and 2 / n == R.RANK_THETA and t1[g].tolist() == [0.0, 0.0, 1.0, R.RANK_THETA, 0.0]
    assert t1[idx["just_above_theta"], 1] > 0 and t1[idx["just_above_theta"], 3] == 3 / n
    # all cells tied at a non-zero value: sigma = 0, z = 0 / 0, p = NaN; the front end's ~isnan filter drops the gene
    g = idx["all_tied"]
    assert i1["tie3"][g] == n ** 3 - n and np.isnan(t1[g, 2]) and t1[g, 0] == 0.5 and t1[g, 1] == 1.0 and t1[g, 3] == 1.0
    sel = (t1[:, 3] > R.RANK_THETA) & ~np.isnan(t1[:, 2])
    assert not sel[g] and not sel[idx["at_theta"]] and sel.sum() == 38
    # no zero at all, negative tie groups, three signs, one cluster only, -0.0
    assert np.count_nonzero(X[idx["no_zero"]]) == n and np.count_nonzero(X[idx["no_zero_signed"]]) == n and X[idx["no_zero_signed"]].min() < 0
    x = X[idx["negative_ties"]]
    assert (x < 0).sum() > 500 and np.unique(x[x < 0]).size <= 8 and (x > 0).sum() == 0 and (x == 0).sum() > 100
    x = X[idx["three_signs"]]
    assert min((x < 0).sum(), (x == 0).sum(), (x > 0).sum()) > 200 and np.unique(x).size <= 12
    g = idx["one_cluster_only"]
    assert set(label[X[g] != 0].tolist()) == {2} and t1[g, 1] == 2.0 and t1[g, 4] == np.inf
    x = X[idx["minus_zero"]]
    assert np.signbit(x[::3]).all() and (x[::3] == 0).all() and t1[idx["minus_zero"], 3] == np.count_nonzero(x) / n < 0.67
    g = idx["cancelling"]
    assert R.fc_bound(t1, i1)[g] > 2.0 ** -45 and not i1["counts"][g]         # a bound set by the cancellation, not by 2^-51
    assert np.all(R.fc_bound(t1, i1)[i1["counts"] & np.isfinite(R.fc_bound(t1, i1))] == 2.0 ** -51)


def test_case_builders_plant_what_the_gpu_cases_say():
    X, label, G = R.case_two_tiles()
    m, n = X.shape
    assert (m, n, G) == (16384 + 37, 600, 4) and np.array_equal(X.astype(np.float32).astype(np.float64), X)
    assert np.count_nonzero(X[16383]) == n and not X[16384].any() and np.count_nonzero(X[m - 1]) == 3
    X, label, G = R.case_long_lists()
    assert X.shape == (48, 20011) and G == 6 and np.array_equal(X.astype(np.float32).astype(np.float64), X)
    nz = np.count_nonzero(X, axis=1)
    assert nz[:22].tolist() == R.LONG_LENGTHS and nz[22] == 20011 and nz[23] == 20010 and nz[24] == 20011
    X, label, G = R.case_many_clusters(256)
    t, i = R.marker_stats(X, label, G)
    assert i["csize"][255] == 1 and t[5, 1] == 256.0 and t[5, 0] == 1.0       # the one-cell cluster is gene 5's best cluster
    assert R.holm([0.01, 0.04, 0.03, 0.005]).tolist() == pytest.approx([0.03, 0.06, 0.06, 0.02])
