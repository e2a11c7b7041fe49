"""tests/_rank_genes_ref.py pinned on scipy and on the marker reference, and the refusals of rank_genes_groups() that need no device
(DESIGN.md §27).  No GPU."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats as st

import _markers_ref as M
import _rank_genes_ref as R

CHUNK = 512


@pytest.fixture(scope="module")
def raw():
    X, codes = R.raw_case(1025, 40, 7, 1, CHUNK)
    return X, codes, 7


@pytest.mark.parametrize("continuity", [False, True])
@pytest.mark.parametrize("ref", [-1, 2])
def test_wilcoxon_is_mannwhitneyu(raw, ref, continuity):
    """z through U and the two-sided p, with ties (counts, the zeros) and without (gene 1), for the rest and for a reference group"""
    X, codes, G = raw
    r = R.reference(X, codes, G, ref=ref, normalize_total=None, log1p=False, continuity=continuity)
    A = X.toarray()
    for g in (0, 3, 6):
        a = codes == g
        b = ~a if ref < 0 else codes == ref
        for j in (1, 3, 4, 5, 9, 17):
            res = st.mannwhitneyu(A[j, a], A[j, b], method="asymptotic", use_continuity=continuity, alternative="two-sided")
            U = (int(r["rank2"][g, j]) - int(a.sum()) * (int(a.sum()) + 1)) / 2.0
            assert U == res.statistic
            assert abs(r["pvals"][g, j] - res.pvalue) <= 1e-12 * res.pvalue + 1e-300
            assert abs(r["auc"][g, j] - res.statistic / (a.sum() * b.sum())) <= 1e-15
    assert np.isnan(r["scores"][ref]).all() if ref >= 0 else True
    # sigma = 0: every value tied
    assert (r["scores"][np.arange(G) != ref, 2] == 0).all() and (r["pvals"][np.arange(G) != ref, 2] == 1).all()


def test_tie_correction_off_is_the_plain_variance(raw):
    X, codes, G = raw
    r = R.reference(X, codes, G, normalize_total=None, log1p=False, tie_correct=False)
    n = codes.size
    ng = int((codes == 1).sum())
    U = (int(r["rank2"][1, 4]) - ng * (ng + 1)) / 2.0
    z = (U - ng * (n - ng) / 2.0) / math.sqrt(ng * (n - ng) * (n + 1) / 12.0)
    assert abs(r["scores"][1, 4] - z) <= 1e-14 * abs(z)


@pytest.mark.parametrize("ref", [-1, 0])
def test_t_test_is_welch(raw, ref):
    X, codes, G = raw
    r = R.reference(X, codes, G, method="t-test", ref=ref, normalize_total=None, log1p=False)
    A = X.toarray()
    for g in (1, 4):
        a = codes == g
        b = ~a if ref < 0 else codes == ref
        res = st.ttest_ind(A[:, a], A[:, b], axis=1, equal_var=False)
        live = np.isfinite(res.statistic)
        assert live.sum() > 30
        assert np.allclose(r["scores"][g][live], res.statistic[live], rtol=1e-10, atol=0)
        assert np.allclose(r["pvals"][g][live], res.pvalue[live], rtol=1e-9, atol=1e-300)
        assert (r["scores"][g][~live] == 0).all() and (r["pvals"][g][~live] == 1).all()      # zero variance on both sides


def test_bh_is_scipy():
    rng = np.random.default_rng(3)
    p = np.concatenate([rng.random(200) ** 3, [0.0, 1.0, 0.5, 0.5]])
    assert np.allclose(R.bh(p), st.false_discovery_control(p, method="bh"), rtol=1e-15, atol=0)
    assert np.isnan(R.bh(np.full(5, np.nan))).all()


def test_auc_is_the_marker_auroc():
    """on float32-exact values with no transform, a gene's auc for the cluster that marker_stats picks is its AUROC"""
    X, codes = R.raw_case(1025, 40, 4, 2, CHUNK)
    A = X.toarray()
    table, info = M.marker_stats(A, codes + 1, 4, theta=0.0, ng=4)
    r = R.reference(X, codes, 4, normalize_total=None, log1p=False)
    live = info["live"]
    best = table[:, 1].astype(int) - 1
    assert live.sum() >= 38
    for j in np.flatnonzero(live):
        assert r["auc"][best[j], j] == table[j, 0]
        assert r["auc"][:, j].max() == table[j, 0]


def test_planted_genes_head_their_group():
    X, codes, G = R.planted_case()
    r = R.reference(X, codes, G)
    m = X.shape[0]
    for g in range(G):
        mine = set(np.arange(g, m, G).tolist())
        assert set(r["order"][g, :len(mine)].tolist()) == mine


def test_order_ties_and_nan():
    s = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, np.nan, 2.0], [np.nan] * 7])
    assert R.order_of(s).tolist() == [[1, 2, 6, 0, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]]


def test_transformed_cases_have_a_rank_margin():
    X, codes = R.count_case(1025, 40, 7, 3, CHUNK)
    assert R.rank_margin(X) > 2.0 ** -40
    r = R.reference(X, codes, 7)
    assert (r["stored"][:, 0] == 0).all() and r["stored"][:, 1].sum() == 1025 and (r["stored"][:, 3] > r["nz"][:, 3]).any()


# ---- the wrapper's refusals that need no device -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    return sharp_amd


def test_refusals_without_a_device(sa, raw):
    X, codes, G = raw
    n = codes.size
    def f(*a, **k):
        return sa.rank_genes_groups(*a, normalize_total=None, log1p=False, **k)

    with pytest.raises(sa.SharpError, match="at least 2 groups"):
        f(X, np.zeros(n, int))
    with pytest.raises(sa.SharpError, match="one label per cell"):
        f(X, codes[:-1])
    with pytest.raises(sa.SharpError, match="at most 1024 groups"):
        f(sp.csc_matrix(np.ones((3, 1025))), np.arange(1025))
    with pytest.raises(sa.SharpError, match="reference must be"):
        f(X, codes, reference=99)
    with pytest.raises(sa.SharpError, match="reference must be"):
        f(X, codes, reference="other")
    with pytest.raises(sa.SharpError, match="method must be"):
        f(X, codes, method="logreg")
    one = codes.copy()
    one[one == 3] = 2
    one[0] = 3
    with pytest.raises(sa.SharpError, match="t-test needs at least 2 cells"):
        f(X, one, method="t-test")
    with pytest.raises(sa.SharpError, match="n_genes must be"):
        f(X, codes, n_genes=0)
    with pytest.raises(sa.SharpError, match="negative value under"):
        sa.rank_genes_groups(X, codes)
    assert "rank_genes_groups" in dir(sa)
