"""Variable-gene selection and gene subsets (tests/_hvg_ref.py) on the CPU: the reference's loess against what it must
reproduce, its standardised variance against a dense restatement, what it selects on the planted inputs, its own rounding spread (from
which the GPU tolerance is taken), the premises of the GPU cases, and the refusals that need no device.

Figures of the reference (printed by the tests): a quadratic at span 1, N = 7: 9e-16.  Median of vs on the planted inputs: 0.997 / 0.999.
At n_top_genes = 200 on PLANTED["large"] every selected gene is a raised one (share 1.0 against 0.726 raised overall).  Rounding spread
(float64 against longdouble sums; genes and cells stored in three random orders): 4.5e-14 small, 2.9e-14 large, 3.0e-13 on the clip
input.  Relative gaps of vs across the cuts used on the GPU: 9.5e-5 ... 3e-3."""
import numpy as np
import pytest
import scipy.sparse as sp

import _expr_pca_ref as ref
import _hvg_ref as h


def test_loess_reproduces_a_quadratic_at_span_one():
    for N in (3, 7, 40):
        x = np.random.default_rng(N).normal(size=N)
        y = 1.0 + 0.5 * x - 0.3 * x * x
        r = h.loess(x, y, 1.0)
        # at span 1 the farthest point lies at distance h and weighs 0: N - 1 points take part, so N = 3 falls to a line through two
        inner = r["window"] >= 3
        err = np.abs(r["fit"] - y)[inner].max() if inner.any() else 0.0
        print(f"quadratic at span 1, N = {N}: {err:.1e}")
        # eight sums of N terms each, solved through pivots of which the smallest is p2: (N + 8) u max|y| / (p2 / S0)
        assert err <= (N + 8) * 2.0 ** -53 * np.abs(y).max() / np.nanmin(r["p2"][inner]) if inner.any() else True
        assert (r["degree"][inner] == 2).all() and (r["window"] == N - 1).all()


@pytest.mark.parametrize("name", list(h.loess_cases()))
def test_bandwidth_is_the_qth_order_statistic(name):
    x, y, span = h.loess_cases()[name]
    assert np.array_equal(h.loess_reference(name)[0]["bandwidth"], h.bandwidth_brute(x, span))


def test_degenerate_rules_on_planted_ties():
    x, y, span = h.loess_cases()["two_one"]
    r = h.loess_reference("two_one")[0]
    assert h.loess_q(x.size, span) == 7
    for v in (0.0, 1.0, 5.0, 6.0):                                               # two distinct x within h: a line
        assert (r["degree"][x == v] == 1).all() and (r["bandwidth"][x == v] > 0).all()
    at = x == 20.0                                                               # eight equal x >= q: h = 0, the tie group's mean
    assert (r["bandwidth"][at] == 0).all() and np.allclose(r["fit"][at], y[at].mean(), rtol=1e-15) and (r["window"][at] == 8).all()
    for v, cnt in ((40.0, 6), (41.0, 1)):                                        # one distinct x within h > 0: the weighted mean
        at = x == v
        assert (r["degree"][at] == 0).all() and (r["bandwidth"][at] == 1.0).all() and (r["window"][at] == cnt).all()
        assert np.allclose(r["fit"][at], y[at].mean(), rtol=1e-15)
    # a line through two distinct x is exact
    yl = 2.0 - 3.0 * x
    rl = h.loess(x, yl, span)
    assert np.abs(rl["fit"] - yl)[np.isin(x, (0.0, 1.0, 5.0, 6.0))].max() <= 1e-13
    # the tie group at the window's edge lies at distance exactly h and takes no part
    x, y, span = h.loess_cases()["edge_ties"]
    r = h.loess_reference("edge_ties")[0]
    i = int(np.flatnonzero(x == 9.0)[0])
    # q = 6: the nearest are 9, 8, 7 and three of the seven points at distance 3 (6 and the six at 12), none of which takes part
    assert r["bandwidth"][i] == 3.0 and r["window"][i] == 3
    h0 = h.loess_reference("h0")[0]
    assert (h0["bandwidth"] == 0).sum() == 21 and (h0["bandwidth"] > 0).sum() == 11


def test_edge_ties_premise():
    x, y, span = h.loess_cases()["edge_ties"]
    assert h.loess_q(x.size, span) == 6


def dense_vs(X, sig2):
    D = X.toarray()
    n = D.shape[1]
    mu = D.mean(1)
    clip = mu + np.sqrt(sig2) * np.sqrt(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((np.minimum(D, clip[:, None]) - mu[:, None]) ** 2).sum(1) / ((n - 1) * sig2)


@pytest.mark.parametrize("name", ["small", "large", "clip"])
def test_standardised_variance_against_a_dense_restatement(name):
    r = h.reference_run(name)
    w = r["want"]
    ok = w["variances"] > 0
    assert np.allclose(w["variances_norm"][ok], dense_vs(r["X"], w["variances_expected"])[ok], rtol=1e-10)
    assert (w["variances_norm"][~ok] == 0).all() and (w["variances_expected"][~ok] == 0).all() and (w["rank"][~ok] == -1).all()
    med = np.median(w["variances_norm"][ok])
    print(f"{name}: median vs {med:.3f}, degrees {w['degree_counts']}, q {w['q']}")
    assert abs(med - 1.0) < (0.01 if name != "clip" else 0.03)
    assert w["n_selected"] == ok.sum() == w["genes"].size and np.array_equal(np.sort(w["order"]), np.flatnonzero(ok))


def test_selection_quality_on_the_large_planted_input():
    n, m, G, k = ref.PLANTED["large"]
    up = h.raised_genes(n, m, G)
    # the replay of planted()'s draws is the real thing: the raised genes have the larger means
    assert up.sum() == 1452 and up.mean() == 0.726
    w = h.reference_run("large")["want"]
    share = up[w["order"][:200]].mean()
    print(f"raised genes among the 200 selected: {share:.3f} (overall {up.mean():.3f})")
    assert share == 1.0


@pytest.mark.parametrize("name,lo,hi", [("small", 2e-14, 1e-13), ("large", 1e-14, 1e-13), ("clip", 1e-13, 1e-12)])
def test_the_references_own_rounding_spread(name, lo, hi):
    r = h.reference_run(name)
    print(f"{name}: rounding spread {r['spread']:.2e} (float64 against longdouble alone {h.rel_diff(r['want'], r['f64']):.2e})")
    assert lo < r["spread"] < hi                              # rounding, not algorithm
    assert np.array_equal(r["want"]["loess"]["bandwidth"], r["f64"]["loess"]["bandwidth"])


def test_premises_of_the_clip_input():
    from sharp_amd import expr_pca

    chunk = expr_pca._row_caps()[0]
    for name in ("small", "large"):
        assert (h.reference_run(name)["want"]["clipped"] == 0).all()             # why the clip input exists
    w = h.reference_run("clip")["want"]
    X, lab, chosen = h.clip_input()
    clipped = w["clipped"]
    print(f"clip input: {int((clipped > 0).sum())} genes clip, {int((clipped > 1).sum())} more than one entry, "
          f"{int(((clipped > 0) & (w['stored'] > chunk)).sum())} with more than {chunk} entries")
    assert (clipped > 0).sum() >= 10 and (clipped > 1).sum() >= 3 and ((clipped > 0) & (w["stored"] > chunk)).any()
    assert set(np.flatnonzero(clipped)) <= set(chosen) and chosen.size == 17


def test_premise_no_point_sits_near_a_degree_switch():
    runs = [h.loess_reference(name) for name in h.loess_cases()]
    runs += [(h.reference_run(name)["f64"]["loess"], h.reference_run(name)["want"]["loess"]) for name in ("small", "large", "clip")]
    for a, b in runs:
        assert np.array_equal(a["degree"], b["degree"]) and np.array_equal(a["bandwidth"], b["bandwidth"])
        for key in ("p1", "p2"):
            v = a[key][np.isfinite(a[key])]
            assert ((v < 2.0 ** -40) | (v > 2.0 ** -20)).all()


def test_premise_cut_margins():
    for name, tops in h.N_TOP.items():
        r = h.reference_run(name)
        tol = 100 * r["spread"]
        for nt in tops:
            gap = h.cut_gap(r["want"], nt)
            print(f"{name}: the cut at {nt}: relative gap {gap:.2e}, GPU tolerance {tol:.1e}")
            assert gap >= 1e6 * tol
            assert set(r["want"]["order"][:nt]) == set(r["f64"]["order"][:nt])


def test_premises_of_the_other_gpu_cases():
    from sharp_amd import expr_pca

    chunk = expr_pca._row_caps()[0]
    X = h.gene_count_case(chunk)
    stored = np.diff(X.tocsr().indptr)
    n = X.shape[1]
    assert stored[:8].tolist() == [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, n, n]
    w = h.hvg(X)
    assert w["variances"][0] == 0 and w["variances"][7] == 0 and w["means"][7] == 3.0 and (w["variances"][1:7] > 0).all()
    assert w["rank"][0] == -1 and w["rank"][7] == -1 and w["n_selected"] == X.shape[0] - 2
    T, groups = h.tie_case()
    t = h.hvg(T, 5)
    v, o = t["variances_norm"], list(t["order"])
    for a, b, c in groups:
        assert a < b < c and v[a] == v[b] == v[c] > 0
        assert o.index(a) + 2 == o.index(b) + 1 == o.index(c)
    cases = h.loess_cases()
    wins = {name: h.loess_reference(name)[0]["window"] for name in cases}
    for win in (63, 64, 65, 129):
        assert (wins["window%d" % win] == win).all()
        assert (cases["window%d" % win][0] < 0).any() and (cases["window%d" % win][0] > 0).any()
    assert cases["n4099"][0].size == 4099 and (4099 + 3) // 4 > 1000


def test_subset_reference_normalises_by_all_genes():
    X = ref.random_csc(60, 45, 0.3, 1, kind="counts")
    G = np.array([0, 3, 4, 17, 59])
    a = h.pca_subset(X, G, 3, 1, 2)
    T, L = ref.transform(X)
    assert np.allclose(L, np.asarray(X.sum(0)).ravel())
    mu, var, _, _ = ref.gene_stats(T)
    assert np.array_equal(a["center"], mu[G]) and np.array_equal(a["gene_var"], var[G]) and a["loadings"].shape == (5, 3)
    b = ref.pca(X[G], 3, 1, 2)                                # subset first: the cells are normalised by the kept genes' sums
    assert not np.allclose(a["center"], b["center"])


def test_refusals_that_need_no_device():
    import sharp_amd as sa

    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    for genes, msg in (([3, 1, 2], "genes must be ascending"), ([1, 2, 2, 5], "genes holds a gene twice"), ([0, 40], r"outside \[0, m\)"),
                       ([-1, 4], r"outside \[0, m\)"), ([], "genes is empty"), (np.zeros(40, bool), "genes is empty"),
                       (np.ones(39, bool), "mask has 39 entries, the blocks have 40 genes"), ([0.5, 2.0], "must hold integers"),
                       (np.zeros((2, 2), int), "one-dimensional")):
        with pytest.raises(sa.SharpError, match="expression_pca: .*" + msg):
            sa.expression_pca(X, 3, genes=genes)
        with pytest.raises(sa.SharpError, match="gene_stats: .*" + msg):
            sa.gene_stats(X, genes=genes)
    with pytest.raises(sa.SharpError, match=r"expression_pca: n_components \+ oversample must be <= min\(cells, genes\)"):
        sa.expression_pca(X, 3, oversample=2, genes=[1, 5, 9, 30])
    fit = {"loadings": np.zeros((2, 1)), "center": np.zeros(2), "scale": np.ones(2), "normalize_total": 1e4, "log1p": True,
           "genes": np.array([1, 7]), "n_genes_in": 41}
    with pytest.raises(sa.SharpError, match="the new cells have 40 genes, the fit has 41"):
        sa.expression_pca_transform(X, fit)
    fit["n_genes_in"], fit["genes"] = 40, np.array([1, 7, 9])
    with pytest.raises(sa.SharpError, match="do not belong together"):
        sa.expression_pca_transform(X, fit)
    for kw, msg in (({"span": 0.0}, "span must lie in"), ({"span": 1.5}, "span must lie in"), ({"span": float("nan")}, "span must lie in"),
                    ({"n_top_genes": 0}, "n_top_genes must be an integer >= 1"), ({"n_top_genes": 2.5}, "n_top_genes must be an integer")):
        with pytest.raises(sa.SharpError, match="highly_variable_genes: " + msg):
            sa.highly_variable_genes(X, **kw)
    bad = X.copy()
    bad.data[5] = -1.0
    with pytest.raises(sa.SharpError, match="highly_variable_genes: a negative value where counts are expected"):
        sa.highly_variable_genes(bad)
    with pytest.raises(sa.SharpError, match="highly_variable_genes: need at least 2 cells"):
        sa.highly_variable_genes(X[:, :1])


def test_the_library_refuses_again_without_the_package():
    import ctypes as C

    from sharp_amd import expr_pca
    from sharp_amd._lib import f64, i32, i64, lib

    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    args, keep = expr_pca._pointers([X])
    out = [np.zeros(30 * 8), np.zeros(40 * 8), np.zeros(8), np.zeros(8), np.zeros(40), np.zeros(40), np.zeros(40)]
    tv = C.c_double()

    def pca(genes, k=3, over=1):
        g = np.asarray(genes, np.int32)
        rc = lib().sharp_expr_pca_sub_csc(*args, 40, k, over, 2, 1e4, 1, 0, 0, *[f64(o) for o in out], C.byref(tv), i32(g) if g.size else None,
                                          g.size if g.size else 7)
        return rc, lib().sharp_last_error()

    for genes, msg in (([3, 1, 2], b"expression_pca: genes must be ascending (position 1,"), ([1, 2, 2, 5], b"genes holds a gene twice (position 2,"),
                       ([0, 40], b"genes holds an index outside [0, m) (position 1,"), ([-1, 4], b"outside [0, m) (position 0,"),
                       ([], b"expression_pca: genes is empty")):
        rc, err = pca(genes)
        assert rc != 0 and msg in err, (genes, err)
    rc, err = pca([1, 5, 9, 30], 3, 2)
    assert rc != 0 and b"n_components + oversample must be <= min(cells, genes)" in err
    st = [np.zeros(40), np.zeros(40), np.zeros(40, np.int64), np.zeros(30)]
    g = np.array([4, 4], np.int32)
    assert lib().sharp_expr_stats_sub_csc(*args, 40, 1e4, 1, f64(st[0]), f64(st[1]), i64(st[2]), f64(st[3]), i32(g), 2) != 0
    assert b"gene_stats: genes holds a gene twice" in lib().sharp_last_error()
    assert lib().sharp_expr_pca_transform_sub_csc(*args, 40, 1e4, 1, f64(out[1]), f64(st[0]), f64(np.ones(40)), 2, f64(out[0]), i32(g), 2) != 0
    assert b"expression_pca_transform: genes holds a gene twice" in lib().sharp_last_error()
    hv = [np.zeros(40) for _ in range(4)] + [np.zeros(40, np.int32) for _ in range(3)]
    ns, q, dc = C.c_int(), C.c_int(), np.zeros(3, np.int32)

    def hvg(top=5, span=0.3):
        rc = lib().sharp_expr_hvg_csc(*args, 40, top, span, *[f64(a) for a in hv[:4]], *[i32(a) for a in hv[4:]], C.byref(ns), C.byref(q), i32(dc))
        return rc, lib().sharp_last_error()

    for kw, msg in (({"top": 0}, b"highly_variable_genes: n_top_genes must be >= 1"), ({"span": 0.0}, b"highly_variable_genes: span must lie in (0, 1]"),
                    ({"span": 1.01}, b"span must lie in (0, 1]")):
        rc, err = hvg(**kw)
        assert rc != 0 and msg in err, (kw, err)
    x = np.zeros(4)
    fit, deg = np.zeros(4), np.zeros(4, np.int32)
    assert lib().sharp_hvg_loess(f64(x), f64(x), 0, 0.3, f64(fit), f64(fit), i32(deg)) != 0 and b"hvg_loess: need 1 <= npts" in lib().sharp_last_error()
    assert lib().sharp_hvg_loess(f64(x), f64(x), 4, 2.0, f64(fit), f64(fit), i32(deg)) != 0 and b"hvg_loess: span must lie" in lib().sharp_last_error()
    x[2] = np.inf
    assert lib().sharp_hvg_loess(f64(x), f64(x), 4, 0.5, f64(fit), f64(fit), i32(deg)) != 0 and b"x and y must be finite (point 2," in lib().sharp_last_error()
    del keep


def test_the_reference_idiom():
    """README's idiom restated on the CPU: select, fit the PCA on the selected genes, neighbours, SNN graph, Louvain.  The ARI it reaches
    against the planted clusters of the clip input is what tests/test_hvg_gpu.py::test_the_readme_idiom is held to."""
    import _louvain_ref as lref
    import _snn_ref as sref
    import _umap_ref as uref

    X, lab, _ = h.clip_input()
    hv = h.hvg(X, 200)
    fit = h.pca_subset(X, hv["genes"], 10)
    idx, _ = uref.knn_lists(fit["scores"], 19)
    g = sref.snn_scipy(idx)
    lv = lref.louvain(g[0], g[1], g[2])
    ari = lref.adjusted_rand(lv["membership"], lab)
    print(f"the reference idiom on the clip input: ARI {ari:.4f}")
    assert ari >= 0.98
