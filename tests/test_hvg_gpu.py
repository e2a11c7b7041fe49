"""Variable-gene selection and gene subsets on the GPU (csrc/hvg.hip, the expr_subset kernels of csrc/expr_pca.hip) against
tests/_hvg_ref.py.

Tolerances, taken from the reference and never tuned:
  * loess stage: against the longdouble reference, 100 x max(that case's float64-against-longdouble difference of the reference,
    2^-52 max|y|); bandwidth and degree equal (tests/test_hvg_cpu.py asserts that no point of a case sits near a degree switch).
  * whole calls: means and variances are gene_stats(blocks, None, False) bit for bit; variances_expected and variances_norm within
    100 x the reference's rounding spread of that input (float64 against longdouble sums and three stored orders; 4.5e-14 / 2.9e-14 /
    3.0e-13 on the small, large and clip inputs), relative to the longdouble reference.  The selected set equals the reference's at the
    n_top_genes whose margin the CPU test asserts (the gap across the cut is at least 10^6 x this tolerance).
  * subset with the transform on: tests/test_expr_pca_gpu.py's tolerances, 100 x §21's recorded spread.
  * end to end: the reference idiom (tests/test_hvg_cpu.py::test_the_reference_idiom) reaches ARI 0.985 on the clip input; the GPU's lists
    may differ from the reference's where two neighbours tie within rounding, for which 0.015 is left: ARI >= 0.97."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _expr_pca_ref as ref
import _hvg_ref as h

pytestmark = pytest.mark.gpu
U = 2.0 ** -52


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def chunk(sa):
    from sharp_amd import expr_pca

    return expr_pca._row_caps()[0]


# ---- the loess stage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(h.loess_cases()))
def test_loess_stage(sa, name):
    from sharp_amd import hvg

    x, y, span = h.loess_cases()[name]
    f64, ld = h.loess_reference(name)
    fit, bw, deg = hvg._loess(x, y, span)
    tol = 100 * max(np.abs(f64["fit"] - ld["fit"]).max(), U * np.abs(y).max())
    err = np.abs(fit - ld["fit"]).max()
    print(f"loess {name}: N {x.size} q {h.loess_q(x.size, span)} |gpu - longdouble| {err:.2e} tolerance {tol:.2e} degrees {np.bincount(deg, minlength=3)}")
    assert np.array_equal(bw, ld["bandwidth"]) and np.array_equal(deg, ld["degree"])
    assert err <= tol
    if name.startswith("window"):                                                # the first and the last point: one-sided windows
        for i in (int(np.argmin(x)), int(np.argmax(x))):
            assert abs(fit[i] - ld["fit"][i]) <= tol and bw[i] == np.sort(np.abs(x - x[i]))[h.loess_q(x.size, span) - 1]
    a, b, c = hvg._loess(x, y, span)
    assert a.tobytes() == fit.tobytes() and b.tobytes() == bw.tobytes() and np.array_equal(c, deg)


def test_loess_ties_stay_in_the_callers_order_and_zero_has_one_sign(sa):
    from sharp_amd import hvg

    x = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 2.0, -2.0])
    y = np.arange(8.0)
    r = h.loess(x, y, 0.5, np.longdouble)
    fit, bw, deg = hvg._loess(x, y, 0.5)
    assert np.array_equal(bw, r["bandwidth"]) and np.array_equal(deg, r["degree"]) and np.abs(fit - r["fit"]).max() <= 100 * U * 8
    assert (bw[[0, 1, 4, 5]] == 0).all() and (fit[[0, 1, 4, 5]] == (0 + 1 + 4 + 5) / 4).all()


# ---- whole calls ------------------------------------------------------------------------------------------------------------------------
def check_call(sa, X, got, want, tol, n_top):
    st = sa.gene_stats(X, None, False)
    assert got["means"].tobytes() == st["mean"].tobytes() and got["variances"].tobytes() == st["var"].tobytes()
    ok = want["variances"] > 0
    assert np.array_equal(got["variances"] > 0, ok)
    for key in ("variances_expected", "variances_norm"):
        assert (got[key][~ok] == 0).all()
        d = (np.abs(got[key] - want[key])[ok] / want[key][ok]).max()
        print(f"  {key}: {d:.2e} (tolerance {tol:.1e})")
        assert d <= tol
    # rank: the lexicographic order of the GPU's own variances_norm
    fg = np.flatnonzero(ok)
    order = fg[np.lexsort((fg, -got["variances_norm"][fg]))]
    ns = min(n_top, fg.size)
    rank = np.full(ok.size, -1)
    rank[order[:ns]] = np.arange(ns)
    assert np.array_equal(got["rank"], rank) and got["n_selected"] == ns
    assert np.array_equal(got["highly_variable"], rank >= 0) and np.array_equal(got["genes"], np.flatnonzero(rank >= 0))
    assert got["genes"].dtype == np.int64 and got["highly_variable"].dtype == np.bool_
    assert got["q"] == want["q"] and np.array_equal(got["degree_counts"], want["degree_counts"])


@pytest.mark.parametrize("name", ["small", "large", "clip"])
def test_call_against_the_reference(sa, name):
    r = h.reference_run(name)
    tol = 100 * r["spread"]
    for n_top in h.N_TOP[name]:
        got = sa.highly_variable_genes(r["X"], n_top)
        check_call(sa, r["X"], got, r["want"], tol, n_top)
        assert set(got["genes"]) == set(r["want"]["order"][:n_top])
    assert got["span"] == 0.3


def case_spread(X, **kw):
    """the reference's float64-against-longdouble difference on an input without a recorded spread"""
    want = h.hvg(X, dtype=np.longdouble, **kw)
    return want, max(h.rel_diff(want, h.hvg(X, **kw)), U)


def test_gene_counts_at_the_chunk_boundaries_and_constant_genes(sa, chunk):
    X = h.gene_count_case(chunk)
    want, spread = case_spread(X, span=0.5)
    got = sa.highly_variable_genes(X, 10, span=0.5)
    check_call(sa, X, got, want, 100 * spread, 10)
    assert got["rank"][0] == -1 and got["rank"][7] == -1 and got["variances_norm"][7] == 0 and got["means"][7] == 3.0
    # n_top_genes above N: every gene that varies, never a constant one
    more = sa.highly_variable_genes(X, 10 ** 6, span=0.5)
    check_call(sa, X, more, want, 100 * spread, 10 ** 6)
    assert more["n_selected"] == X.shape[0] - 2 and not more["highly_variable"][[0, 7]].any() and more["highly_variable"].sum() == X.shape[0] - 2


def test_equal_rows_the_lower_index_wins(sa):
    X, groups = h.tie_case()
    got = sa.highly_variable_genes(X, X.shape[0])
    v, r = got["variances_norm"], got["rank"]
    for a, b, c in groups:
        assert v[a] == v[b] == v[c] > 0 and r[a] + 2 == r[b] + 1 == r[c]
    a, b, c = groups[0]
    cut = sa.highly_variable_genes(X, int(r[a]) + 2)             # the cut falls inside the group: the two lower genes are kept
    assert cut["highly_variable"][[a, b]].all() and not cut["highly_variable"][c]


def test_two_calls_and_ragged_blocks_give_the_same_bits(sa):
    X = h.clip_input()[0]
    a = sa.highly_variable_genes(X, 100)
    b = sa.highly_variable_genes(X, 100)
    c = sa.highly_variable_genes(ref.ragged(X, [401, 401, 1101]), 100)
    assert [p.shape[1] for p in ref.ragged(X, [401, 401, 1101])] == [401, 0, 700, 399]
    for key in ("means", "variances", "variances_expected", "variances_norm", "rank", "highly_variable", "genes", "degree_counts"):
        assert a[key].tobytes() == b[key].tobytes() == c[key].tobytes(), key


def test_refusals_on_the_device(sa):
    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    same = sp.csc_matrix(np.repeat(np.arange(40.0)[:, None] % 7, 30, axis=1))
    with pytest.raises(sa.SharpError, match="highly_variable_genes: every gene is constant"):
        sa.highly_variable_genes(same)
    # past the package's check: the library names the negative value itself
    from sharp_amd import expr_pca
    from sharp_amd._lib import f64, i32

    bad = X.copy()
    bad.data[int(bad.indptr[4])] = -2.0
    args, keep = expr_pca._pointers([bad])
    out = [np.zeros(40) for _ in range(4)] + [np.zeros(40, np.int32) for _ in range(3)]
    ns, q, dc = C.c_int(), C.c_int(), np.zeros(3, np.int32)
    rc = sa.lib().sharp_expr_hvg_csc(*args, 40, 5, 0.3, *[f64(a) for a in out[:4]], *[i32(a) for a in out[4:]], C.byref(ns), C.byref(q), i32(dc))
    assert rc != 0 and "highly_variable_genes: a negative value where counts are expected (cell 4, counted from 0)" in sa.lib().sharp_last_error().decode()
    del keep


# ---- the subset -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """planted small, the 200 genes its reference selects, and the GPU fit on them (made once)"""
    X = ref.planted_case("small")[0]
    return X, h.reference_run("small")["want"]["order"][:200].copy()


@pytest.fixture(scope="module")
def small_fit(sa, small):
    X, G = small
    return sa.expression_pca(X, 10, genes=np.sort(G))


def test_gene_stats_of_a_subset_are_the_full_calls_rows(sa, small):
    X, G = small
    G = np.sort(G)
    full, sub = sa.gene_stats(X), sa.gene_stats(X, genes=G)
    for key in ("mean", "var", "nnz"):
        assert sub[key].tobytes() == full[key][G].tobytes(), key
    assert sub["cell_sum"].tobytes() == full["cell_sum"].tobytes()
    mask = np.zeros(X.shape[0], bool)
    mask[G] = True
    assert sa.gene_stats(X, genes=mask)["var"].tobytes() == sub["var"].tobytes()
    parts = ref.ragged(X, [0, 500, 500, 1203])
    assert sa.gene_stats(parts, genes=G)["var"].tobytes() == sub["var"].tobytes()


def test_subset_without_a_transform_equals_the_subset_matrix(sa, small):
    X, G = small
    G = np.sort(G)
    parts = ref.ragged(X, [401, 401, 1101])
    a = sa.expression_pca(parts, 10, normalize_total=None, log1p=False, scale=True, genes=G)
    b = sa.expression_pca([sp.csc_matrix(p.tocsr()[G]) for p in parts], 10, normalize_total=None, log1p=False, scale=True)
    for key in ("scores", "loadings", "singular_values", "sdev", "center", "scale", "gene_var"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["total_var"] == b["total_var"]
    assert (a["n_genes"], a["n_genes_in"], b["n_genes"], b["n_genes_in"], b["genes"]) == (200, 800, 200, 200, None) and np.array_equal(a["genes"], G)


def test_subset_with_the_transform_against_the_reference(sa, small, small_fit):
    X, G = small
    G = np.sort(G)
    want, got = h.pca_subset(X, G, 10), small_fit
    sp_ = ref.reference_run("small", False)["spread"]
    ds = np.abs(got["singular_values"] - want["singular_values"]).max() / want["singular_values"][0]
    dsc = np.abs(got["scores"] - want["scores"]).max() / np.abs(want["scores"]).max()
    dl = np.abs(got["loadings"] - want["loadings"]).max()
    print(f"subset of 200: s {ds:.2e} (spread {sp_['s']:.2e}) scores {dsc:.2e} ({sp_['scores']:.2e}) loadings {dl:.2e} ({sp_['loadings']:.2e})")
    assert ds <= 100 * sp_["s"] and dsc <= 100 * sp_["scores"] and dl <= 100 * sp_["loadings"]
    assert got["loadings"].shape == (200, 10) and got["center"].shape == got["scale"].shape == got["gene_var"].shape == (200,)
    st = sa.gene_stats(X)
    assert got["center"].tobytes() == st["mean"][G].tobytes() and got["gene_var"].tobytes() == st["var"][G].tobytes()
    # not what subsetting first computes: that normalises a cell by the kept genes' sum
    first = sa.expression_pca(sp.csc_matrix(X.tocsr()[G]), 10)
    assert not np.allclose(first["center"], got["center"])


def test_all_genes_give_the_bits_of_the_call_without_genes(sa):
    X = ref.planted(600, 300, 4)[0]
    a = sa.expression_pca(X, 8, scale=True)
    b = sa.expression_pca(X, 8, scale=True, genes=np.arange(300))
    c = sa.expression_pca(X, 8, scale=True, genes=np.ones(300, bool))
    for key in ("scores", "loadings", "singular_values", "center", "scale", "gene_var"):
        assert a[key].tobytes() == b[key].tobytes() == c[key].tobytes(), key
    assert a["genes"] is None and a["n_genes"] == a["n_genes_in"] == 300 and np.array_equal(b["genes"], np.arange(300))


def boundary_block():
    """200 genes x 40 cells; genes 0 .. 99 are kept.  Cell 0 holds entries of dropped genes only, cells 1, 2, 3 keep 63, 64 and 65 entries
    beside 70 dropped ones, cell 4 holds nothing, the others are random"""
    rng = np.random.default_rng(8)
    D = np.zeros((200, 40))
    D[100 + rng.choice(100, 30, replace=False), 0] = rng.integers(1, 9, size=30)
    for c, kept in ((1, 63), (2, 64), (3, 65)):
        D[rng.choice(100, kept, replace=False), c] = rng.integers(1, 9, size=kept)
        D[100 + rng.choice(100, 70, replace=False), c] = rng.integers(1, 9, size=70)
    D[:, 5:] = rng.poisson(0.4, size=(200, 35))
    return sp.csc_matrix(D)


def test_subset_boundaries(sa):
    X = boundary_block()
    G = np.arange(100)
    kept = np.diff(sp.csc_matrix(X.tocsr()[G]).indptr)
    assert kept[:5].tolist() == [0, 63, 64, 65, 0] and np.diff(X.indptr)[:5].tolist() == [30, 133, 134, 135, 0]
    full, sub = sa.gene_stats(X), sa.gene_stats(X, genes=G)
    assert sub["mean"].tobytes() == full["mean"][G].tobytes() and sub["var"].tobytes() == full["var"][G].tobytes()
    # the fit on the compacted entries: without a transform, the bits of the fit on the subset matrix
    raw = {"normalize_total": None, "log1p": False}
    a, b = sa.expression_pca(X, 3, 2, genes=G, **raw), sa.expression_pca(sp.csc_matrix(X.tocsr()[G]), 3, 2, **raw)
    assert all(a[key].tobytes() == b[key].tobytes() for key in ("scores", "loadings", "singular_values", "center", "gene_var"))
    # with it, the scores are the transform's; a cell that loses every entry scores as an empty one
    got = sa.expression_pca(X, 3, 2, genes=G)
    sc = sa.expression_pca_transform(X, got)
    assert sc.tobytes() == got["scores"].tobytes() and (sc[0] == sc[4]).all()
    # only the first and the last gene kept
    ends = sa.gene_stats(X, genes=[0, 199])
    assert ends["mean"].tobytes() == full["mean"][[0, 199]].tobytes() and ends["var"].tobytes() == full["var"][[0, 199]].tobytes()
    assert ends["nnz"].tolist() == full["nnz"][[0, 199]].tolist() and ends["cell_sum"].tobytes() == full["cell_sum"].tobytes()
    # one gene with l = 1
    g = int(np.argmax(full["var"]))
    one, alone = sa.expression_pca(X, 1, oversample=0, genes=[g], **raw), sa.expression_pca(sp.csc_matrix(X.tocsr()[[g]]), 1, oversample=0, **raw)
    assert one["loadings"].tolist() == [[1.0]] and one["scores"].tobytes() == alone["scores"].tobytes()
    assert one["singular_values"].tobytes() == alone["singular_values"].tobytes()
    t = sa.expression_pca(X, 1, oversample=0, genes=[g])
    assert t["loadings"].tolist() == [[1.0]] and t["center"][0] == full["mean"][g] and t["gene_var"][0] == full["var"][g]
    T = ref.transform(X)[0].toarray()
    assert np.abs(t["scores"][:, 0] - (T[g] - full["mean"][g])).max() <= 8 * ref.U * np.abs(T[g]).max()       # (t - mu) 1, one rounding each


def test_transform_of_a_subset_fit(sa, small, small_fit):
    X, G = small
    fit = small_fit
    got = sa.expression_pca_transform(X, fit)
    assert got.tobytes() == fit["scores"].tobytes()              # the same kernel on the same values
    parts = ref.ragged(X, [1, 700, 700, 1203])
    assert np.concatenate([sa.expression_pca_transform(b, fit) for b in parts]).tobytes() == got.tobytes()
    assert sa.expression_pca_transform(parts, fit).tobytes() == got.tobytes()
    assert sa.expression_pca_transform(X[:, :0], fit).shape == (0, 10)
    with pytest.raises(sa.SharpError, match="the new cells have 200 genes, the fit has 800"):
        sa.expression_pca_transform(sp.csc_matrix(X.tocsr()[np.sort(G)]), fit)


def test_subset_refusals_by_name(sa):
    from sharp_amd import expr_pca
    from sharp_amd._lib import f64, i32

    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    with pytest.raises(sa.SharpError, match=r"expression_pca: n_components \+ oversample must be <= min\(cells, genes\)"):
        sa.expression_pca(X, 3, oversample=2, genes=[1, 5, 9, 30])
    args, keep = expr_pca._pointers([X])
    out = [np.zeros(30 * 8), np.zeros(40 * 8), np.zeros(8), np.zeros(8), np.zeros(40), np.zeros(40), np.zeros(40)]
    tv = C.c_double()

    def pca(genes, k=3, over=1):
        g = np.asarray(genes, np.int32)
        rc = sa.lib().sharp_expr_pca_sub_csc(*args, 40, k, over, 2, 1e4, 1, 0, 0, *[f64(o) for o in out], C.byref(tv), i32(g), g.size)
        return rc, sa.lib().sharp_last_error().decode()

    assert pca([1, 5, 9, 30, 31])[0] == 0
    for genes, kw, msg in (([3, 1, 2], {}, "genes must be ascending"), ([1, 2, 2, 5], {}, "genes holds a gene twice"), ([0, 40], {}, "outside [0, m)"),
                           ([1, 5, 9, 30], {"k": 3, "over": 2}, "must be <= min(cells, genes)")):
        rc, err = pca(genes, **kw)
        assert rc != 0 and "expression_pca: " in err and msg in err, err
    del keep


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_the_readme_idiom(sa):
    import _louvain_ref as lref

    X, lab, _ = h.clip_input()
    hv = sa.highly_variable_genes(X, 200)
    pc = sa.expression_pca(X, 10, genes=hv["genes"])
    nb = sa.knn(pc["scores"], 19)
    lv = sa.louvain_snn(nb[0])
    ari = lref.adjusted_rand(lv["membership"], lab)
    print(f"README idiom on the clip input: ARI {ari:.4f}")
    assert ari >= 0.97
