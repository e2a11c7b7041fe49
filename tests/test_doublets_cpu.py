"""The doublet detection's reference (tests/_doublets_ref.py) pinned on the CPU, the library's host-only entries against
it, and the quality floors that tests/test_doublets_gpu.py holds the GPU call to.  No GPU is needed."""
import os
import re

import numpy as np
import pytest

import _doublets_ref as R
from sharp_amd import doublets  # noqa: F401  (without the feature every test here fails at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sharp_doublet_plan", "sharp_doublet_pairs", "sharp_doublet_synth_csc", "sharp_doublet_project_csc", "sharp_doublet_neighbor_counts",
       "sharp_doublet_score_table", "sharp_doublet_threshold", "sharp_scrublet_csc", "sharp_C_scrublet_csc"]


@pytest.fixture(scope="module")
def sharp():
    import __graft_entry__ as g

    import sharp_amd

    if not os.path.exists(sharp_amd.so_path()):
        g.build()
    return sharp_amd


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------
def test_pairs_by_hand():
    # seed 0, s = 0: mix(0) = 0, so h(0, 0) = mix(0 + 0) = 0 and the first parent is cell 0 whatever n is
    assert R.pairs(400, 1, 0)[0, 0] == 0 and R.pairs(7, 1, 0)[0, 0] == 0
    # h(0, 1) = mix(1) = 0x5692161D100B05E5 (the splitmix64 finaliser of 1): the second parent is floor((h >> 11) 2^-53 n)
    h = 0x5692161D100B05E5
    assert int(R.ref.mix(np.uint64(1))) == h
    assert R.pairs(400, 1, 0)[0, 1] == int(np.floor(float(h >> 11) * 2.0 ** -53 * 400.0)) == 135
    assert R.pairs(400, 4, 0).tolist() == [[0, 135], [191, 340], [129, 98], [337, 279]]


def test_pairs_ranges_and_purity():
    for n, ns, seed in ((2, 50, 1), (400, 800, 0), (50000, 3000, 2 ** 53 - 1)):
        p = R.pairs(n, ns, seed)
        assert p.shape == (ns, 2) and p.min() >= 0 and p.max() < n
        assert np.array_equal(p, R.pairs(n, ns, seed))
        assert np.array_equal(p[:ns // 2], R.pairs(n, ns // 2, seed))       # (doublet s does not depend on n_sim)
        assert not np.array_equal(p, R.pairs(n, ns, seed + 1 if seed < 2 ** 53 - 1 else 0))
    p = R.pairs(400, 20000, 3)
    assert (p[:, 0] == p[:, 1]).any()                                        # a cell may meet itself
    assert abs(np.bincount(p.ravel(), minlength=400).std() / 100.0 - 0.1) < 0.02   # 40000 draws over 400 cells: Poisson(100)


def test_pairs_of_the_library(sharp):
    from sharp_amd import doublets

    for n, ns, seed in ((400, 800, 0), (7, 20, 5), (50000, 1000, 2 ** 53 - 1)):
        assert np.array_equal(doublets._pairs(n, ns, seed), R.pairs(n, ns, seed))
    with pytest.raises(sharp.SharpError, match=r"seed must be a whole number in \[0, 2\^53\)"):
        doublets._pairs(10, 5, 2 ** 53)


# ---- the plan: n_sim, the default n_neighbors and its cap -------------------------------------------------------------------------------
def test_plan_cap_rule(sharp):
    from sharp_amd import doublets

    assert R.plan(400) == (800, 10, 30)                                      # round(0.5 sqrt(400)) = 10, k_adj = 30
    assert R.plan(28900) == (57800, 85, 255)                                 # the last size at which the cap does not bind
    assert R.plan(50000) == (100000, 85, 255)                                # round(0.5 sqrt(50000)) = 112 would need 336 neighbours
    assert R.plan(50000, 3.3)[1:] == (59, 254)
    assert R.plan(3) == (6, 1, 3)
    for n in (2, 3, 10, 400, 28900, 29000, 50000, 200000):
        for ratio in (2.0, 0.5, 3.3):
            assert doublets._plan(n, ratio) == R.plan(n, ratio), (n, ratio)
    assert doublets._plan(400, 2.0, 20) == (800, 20, 60)
    with pytest.raises(sharp.SharpError, match="gives k_adj = round.* = 258 neighbours per row; the k-NN stages take at most 255"):
        doublets._plan(50000, 2.0, 86)
    with pytest.raises(sharp.SharpError, match="there are only n \\+ n_sim - 1 = 11 other rows"):
        doublets._plan(4, 2.0, 5)
    with pytest.raises(sharp.SharpError, match="sim_doublet_ratio gives fewer than 1 simulated doublet"):
        doublets._plan(4, 0.1)
    with pytest.raises(sharp.SharpError, match="need at least 2 cells"):
        doublets._plan(1, 2.0)


# ---- synthesis --------------------------------------------------------------------------------------------------------------------------
def test_synthesis_equals_scipy():
    blocks, par = R.hand_cells()
    D, L = R.synth(blocks, par)
    X = R.ref.concat(blocks)
    S = (X[:, par[:, 0]] + X[:, par[:, 1]]).tocsc()
    S.sort_indices()
    assert np.array_equal(D.indptr, S.indptr) and np.array_equal(D.indices, S.indices) and D.data.tobytes() == S.data.tobytes()
    assert np.array_equal(L, np.asarray(S.sum(0)).ravel())                  # integer counts: every order of the sum is exact
    length = np.diff(X.indptr)
    # the inputs reach the cases the merge kernel can get wrong
    assert {0, 1, 63, 64, 65, 129, 200} <= set(length.tolist())
    assert any(length[a] == 0 and length[b] == 0 for a, b in par) and any((length[a] == 0) != (length[b] == 0) for a, b in par)
    assert any(a == b and length[a] > 64 for a, b in par) and any(a < 17 <= b or b < 17 <= a for a, b in par)
    assert D[0].nnz and D[R.M_HAND - 1].nnz


# ---- the score table --------------------------------------------------------------------------------------------------------------------
def test_score_table(sharp):
    from sharp_amd import doublets

    for K, r, rho in ((30, 2.0, 0.1), (255, 0.37, 0.5), (1, 3.0, 0.01), (90, 2.0, 0.25)):
        t = R.score_table(K, r, rho)
        assert (np.diff(t) > 0).all() and t[0] > 0 and t[-1] < 1
        # the ends: q = 1 / (K + 2) and q = (K + 1) / (K + 2) in Scrublet's Bayesian formula, evaluated in extended precision
        q = (np.array([0, K], np.longdouble) + 1) / (K + 2)
        want = q * rho / r / (1 - rho - q * (1 - rho - rho / r))
        assert np.allclose(t[[0, -1]], want.astype(np.float64), rtol=1e-14, atol=0)
        # a cell whose neighbours are simulated in the share r / (1 + r) that pure chance gives scores about rho
        qc = r / (1 + r)
        assert abs(qc * rho / r / (1 - rho - qc * (1 - rho - rho / r)) - rho) < 1e-12
        # the library's table: the host function is compiled without contraction (-ffp-contract=off), so the bits agree
        assert doublets._score_table(K, r, rho).tobytes() == t.tobytes()


# ---- the threshold rule -----------------------------------------------------------------------------------------------------------------
def test_threshold_rule_by_hand():
    h = np.zeros(R.BINS)
    h[[10, 11, 12]] = [5, 9, 5]
    h[[100, 101]] = [4, 4]                                                    # (a plateau is one maximum)
    assert R.local_maxima(h) == [11, 100]
    assert R.local_maxima(np.arange(R.BINS, dtype=np.float64)) == [R.BINS - 1] and R.local_maxima(np.ones(R.BINS)) == [0]
    s = R.smooth(np.array([3.0, 0.0, 6.0, 0.0]))
    assert s.tolist() == [(0.0 + 3.0 + 0.0) / 3, 3.0, 2.0, (6.0 + 0.0 + 6.0) / 3]   # reflected ends: h[-1] = h[1], h[n] = h[n - 2]
    # two separated groups of scores: the threshold is the centre of the first of the lowest bins between the modes
    sim = np.concatenate([np.full(50, 0.0), np.full(30, 0.25), np.full(40, 1.0)])
    r = R.threshold(np.array([0.1, 0.9, 0.5]), sim)
    hist, mn, width = R.histogram(sim)
    assert R.local_maxima(hist) == [0, 64, 255] and r["threshold_found"] and r["passes"] >= 1
    assert r["predicted_doublets"].tolist() == [False, True, r["threshold"] < 0.5]
    assert r["detectable_doublet_fraction"] == float((sim > r["threshold"]).sum()) / sim.size
    assert r["overall_doublet_rate"] == r["detected_doublet_rate"] / r["detectable_doublet_fraction"]


def test_threshold_bimodal_and_unimodal(sharp):
    from sharp_amd import doublets

    obs, sim = R.two_mode_scores()
    want, got = R.threshold(obs, sim), doublets._threshold(obs, sim)
    assert want["threshold_found"] and 0.15 < want["threshold"] < 0.45            # between the modes at 0.09 and 0.55
    for key in ("threshold", "threshold_found", "passes", "detected_doublet_rate", "detectable_doublet_fraction", "overall_doublet_rate"):
        assert got[key] == want[key], key
    assert np.array_equal(got["predicted_doublets"], want["predicted_doublets"])
    # discrete scores, as the table gives them: the raw histogram has a maximum per value
    table = R.score_table(90, 2.0, 0.1)
    rng = np.random.default_rng(0)
    c = np.concatenate([rng.binomial(90, 0.3, 2000), rng.binomial(90, 0.9, 1000)])
    want, got = R.threshold(table[c[:500]], table[c]), doublets._threshold(table[c[:500]], table[c])
    assert want["threshold_found"] and want["passes"] > 10 and got["threshold"] == want["threshold"] and got["passes"] == want["passes"]
    # one mode, and no spread at all: nothing found, nothing predicted
    for sim1 in (R.triangle_scores(), np.full(100, 0.3)):
        want, got = R.threshold(sim1, sim1), doublets._threshold(sim1, sim1)
        for r in (want, got):
            assert r["threshold"] is None and not r["threshold_found"] and r["predicted_doublets"] is None and r["overall_doublet_rate"] is None
    # a given threshold is used as it is
    got = doublets._threshold(obs, sim, 0.3)
    assert got["threshold"] == 0.3 and not got["threshold_found"] and np.array_equal(got["predicted_doublets"], obs > 0.3)


# ---- the quality floors -----------------------------------------------------------------------------------------------------------------
def test_quality_floor_of_the_reference():
    """The reference on the planted input with 8 % planted doublets (1500 cells, 800 genes, 300 variable genes, 30 components), seeds
    0 .. 4.  Measured: AUROC 0.99996 .. 1.0, share of the planted doublets above the found threshold 0.958 .. 0.975; the floors
    (worst less spread) are 0.99992 and 0.942.  The GPU call is held to quality_reference()'s floors as computed where the test runs."""
    q = R.quality_reference()
    au, sh = [r[0] for r in q["rows"]], [r[1] for r in q["rows"]]
    print("AUROC", au, "share", sh, "floors", q["auroc_floor"], q["share_floor"])
    assert all(r[2] is not None for r in q["rows"])                              # a threshold was found at every seed
    assert q["auroc_floor"] == min(au) - (max(au) - min(au)) and q["share_floor"] == min(sh) - (max(sh) - min(sh))
    assert q["auroc_floor"] > 0.99 and q["share_floor"] > 0.9                   # the method works on this input at all
    X, is_d = R.quality_input()
    assert X.shape == (R.M_QUALITY, R.N_QUALITY) and is_d.sum() == 120 and (X.data == np.floor(X.data)).all()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_abi_symbols(sharp):
    from sharp_amd import _abi

    header = open(os.path.join(ROOT, "include", "sharp_hip.h")).read()
    for name in NEW:
        assert name in _abi.SIGNATURES, name
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, header), name
        assert getattr(sharp.lib(), name) is not None
    assert callable(sharp.scrublet) and callable(sharp.simulate_doublets)


def test_refusals_before_the_library(sharp):
    import scipy.sparse as sp

    X = sp.csc_matrix(np.random.default_rng(0).integers(0, 4, size=(30, 12)).astype(np.float64))
    bad = X.copy()
    bad.data[5] = -1.0
    with pytest.raises(sharp.SharpError, match="scrublet: a negative value where counts are expected"):
        sharp.scrublet(bad)
    bad.data[5] = np.inf
    with pytest.raises(sharp.SharpError, match="scrublet: a value that is NaN or infinite"):
        sharp.scrublet(bad)
    with pytest.raises(sharp.SharpError, match="scrublet: need at least 2 cells in all"):
        sharp.scrublet(X[:, :1])
    with pytest.raises(sharp.SharpError, match="scrublet: sim_doublet_ratio gives fewer than 1 simulated doublet"):
        sharp.scrublet(X, sim_doublet_ratio=0.01)
    for rho in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(sharp.SharpError, match=r"scrublet: expected_doublet_rate must lie in \(0, 1\)"):
            sharp.scrublet(X, expected_doublet_rate=rho)
    for seed in (-1, 2 ** 53, 0.5):
        with pytest.raises(sharp.SharpError, match=r"scrublet: seed must be a whole number in \[0, 2\^53\)"):
            sharp.scrublet(X, seed=seed)
    fit = {"scores": np.zeros((12, 3)), "loadings": np.zeros((31, 3)), "center": np.zeros(31), "scale": np.ones(31), "normalize_total": 1e4,
           "log1p": True, "genes": None}
    with pytest.raises(sharp.SharpError, match="scrublet: the pca was fitted on 31 genes, the blocks have 30"):
        sharp.scrublet(X, pca=fit)
    with pytest.raises(sharp.SharpError, match="n_neighbors = 9 gives k_adj = 27 neighbours per row; there are only"):
        sharp.scrublet(X[:, :4], n_neighbors=9)
