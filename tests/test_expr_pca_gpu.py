"""The truncated PCA of sparse expression blocks on the GPU (csrc/expr_pca.hip) against tests/_expr_pca_ref.py.

Tolerances, derived per entry and computed from the reference, never tuned (u = 2^-53):
  * A product entry is a sum of N products plus the shift.  Any order of N additions of rounded products is within N u sum|terms| of the
    exact sum to first order; the transform's division, its product and log1p, the weight and the subtraction of the shift add a few
    roundings per term, which the 8 covers.  Cell side: |Y - Y_ref| <= (N + 8) u (|T|^T |Bs| + |mu|^T |Bs|), N the cell's stored entries.
    Gene side: (N + 8) u |w_g| (|T| |Q| + |mu_g| sum|Q|), N the gene's stored entries.
  * mean: (N + 8) u sum|t| / n.  var: (N + 8) u (sum (|t| + |mu|)^2 + (n - N) mu^2) / (n - 1): every term of the variance is a square,
    and mu's own error enters in second order only (the derivative of the sum in mu is zero at the mean).  Cell sums: (N + 8) u sum|t|.
  * orth: ||Q^T Q - I|| and ||Y - Q (Q^T Y)|| / ||Y|| at most 100 x the reference's own figures (at least 100 u).
  * whole calls: 100 x the reference's rounding spread (the same input with cells and genes stored in three random orders), which
    this file computes through _expr_pca_ref.reference_run.  The factor covers what the permutations do not exercise: log1p's last
    bits and the host QL solver against LAPACK.  The planted singular values lie within twice the reference's own error against the
    dense spectrum.

scores = A loadings, the cell-side product with the loadings: expression_pca_transform on the fitted cells runs the same kernel on the same
values, so test_transform_of_the_fitted_cells_equals_scores holds within the product bound (the subspace's Q W diag(s) = Q Q^T A loadings
would agree only as far as a component has converged: 1e-4 ... 3e-3 of max|scores| on the planted components, 4e-2 ... 6e-2 on the
noise components, measured on one MI355X and on the reference alike)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _expr_pca_ref as ref

pytestmark = pytest.mark.gpu
U = ref.U
LS = (1, 60, 64, 65, 128)


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def caps(sa):
    from sharp_amd import expr_pca

    return expr_pca._row_caps()


@pytest.fixture(scope="module")
def cases(caps):
    out = ref.stage_cases(*caps)
    out["m1"] = ref.random_csc(1, 50, 0.6, 31)
    return out


def stage(sa, name, blocks, M, l, total=1e4, lg=True, scale=False):
    """sharp_expr_spmm_cells / _genes on a list of scipy blocks"""
    from sharp_amd import expr_pca
    from sharp_amd._lib import check, f64

    blocks = [b.tocsc() for b in blocks]
    m, n = blocks[0].shape[0], sum(b.shape[1] for b in blocks)
    args, keep = expr_pca._pointers(blocks)
    M = np.ascontiguousarray(M, np.float64)
    out = np.zeros((n if name == "cells" else m, l))
    check(getattr(sa.lib(), "sharp_expr_spmm_" + name)(*args, m, float(total or 0), int(lg), int(scale), f64(M), l, f64(out)))
    del keep
    return out


def gpu_orth(sa, Y):
    from sharp_amd._lib import check, f64

    Y = np.ascontiguousarray(Y, np.float64)
    Q = np.zeros_like(Y)
    check(sa.lib().sharp_expr_orth(f64(Y), Y.shape[0], Y.shape[1], f64(Q)))
    return Q


def ref_stats(X, total=1e4, lg=True, scale=False):
    T, _ = ref.transform(X, total, lg)
    mu, var, nnz, stored = ref.gene_stats(T)
    sd, w = ref.weights(var, scale)
    return T, mu, var, nnz, stored, w


def within(got, want, bound, what):
    over = np.abs(got - want) - bound
    assert (over <= 0).all(), f"{what}: {int((over > 0).sum())} entries beyond the bound, the worst by {over.max():.3e} (bound there {bound.ravel()[over.argmax()]:.3e})"


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("name", ["cells", "genes", "full", "slab-1", "slab+0", "slab+1", "m70000", "n2", "m1"])
def test_products(sa, cases, name, l):
    X = cases[name]
    m, n = X.shape
    scale = l in (60, 65)
    T, mu, var, nnz, stored, w = ref_stats(X, scale=scale)
    rng = np.random.default_rng(l)
    B, Q = rng.normal(size=(m, l)), rng.normal(size=(n, l))
    Y = stage(sa, "cells", [X], B, l, scale=scale)
    within(Y, ref.spmm_cells(T, mu, w, B), ref.spmm_cells_bound(T, mu, w, B), "cell side")
    Z = stage(sa, "genes", [X], Q, l, scale=scale)
    within(Z, ref.spmm_genes(T.tocsr(), mu, w, Q), ref.spmm_genes_bound(T, mu, w, Q, stored), "gene side")
    assert np.isfinite(Y).all() and np.isfinite(Z).all()


@pytest.mark.parametrize("total,lg", [(None, False), (None, True), (50.0, False)])
def test_products_under_the_other_transforms(sa, cases, total, lg):
    X = cases["cells"]
    T, mu, var, nnz, stored, w = ref_stats(X, total, lg, True)
    rng = np.random.default_rng(5)
    B, Q = rng.normal(size=(X.shape[0], 9)), rng.normal(size=(X.shape[1], 9))
    within(stage(sa, "cells", [X], B, 9, total, lg, True), ref.spmm_cells(T, mu, w, B), ref.spmm_cells_bound(T, mu, w, B), "cell side")
    within(stage(sa, "genes", [X], Q, 9, total, lg, True), ref.spmm_genes(T.tocsr(), mu, w, Q), ref.spmm_genes_bound(T, mu, w, Q, stored),
           "gene side")


@pytest.mark.parametrize("name", ["cells", "genes", "full"])
def test_blocks_give_the_bits_of_one_block(sa, cases, name):
    """an empty first block, an empty block in the middle, an empty last block, ragged sizes: the same cells as one block"""
    X = cases[name]
    n = X.shape[1]
    parts = ref.ragged(X, [0, n // 3, n // 3, n - 7, n])
    assert [b.shape[1] for b in parts] == [0, n // 3, 0, n - 7 - n // 3, 7, 0]
    rng = np.random.default_rng(1)
    B, Q = rng.normal(size=(X.shape[0], 65)), rng.normal(size=(n, 65))
    assert stage(sa, "cells", parts, B, 65).tobytes() == stage(sa, "cells", [X], B, 65).tobytes()
    assert stage(sa, "genes", parts, Q, 65, scale=True).tobytes() == stage(sa, "genes", [X], Q, 65, scale=True).tobytes()
    a, b = sa.gene_stats(parts), sa.gene_stats(X)
    assert all(a[key].tobytes() == b[key].tobytes() for key in ("mean", "var", "nnz", "cell_sum"))


@pytest.mark.parametrize("name", ["cells", "genes", "full", "slab+1", "m70000", "n2", "m1"])
@pytest.mark.parametrize("total,lg", [(1e4, True), (None, False)])
def test_statistics_and_cell_sums(sa, cases, name, total, lg):
    X = cases[name]
    m, n = X.shape
    T, mu, var, nnz, stored, _ = ref_stats(X, total, lg)
    got = sa.gene_stats(X, total, lg)
    aT = abs(T)
    sum_abs = np.asarray(aT.sum(1)).ravel()
    within(got["mean"], mu, (stored + 8) * U * sum_abs / n, "mean")
    sq = np.asarray((aT + sp.csc_matrix((np.abs(mu)[T.indices], T.indices, T.indptr), shape=T.shape)).power(2).sum(1)).ravel()
    within(got["var"], var, (stored + 8) * U * (sq + (n - stored) * mu * mu) / (n - 1), "var")
    assert np.array_equal(got["nnz"], nnz)
    cs = np.asarray(aT.sum(0)).ravel()
    within(got["cell_sum"], np.asarray(T.sum(0)).ravel(), (np.diff(T.indptr) + 8) * U * cs, "cell sums")
    const = var == 0
    assert (got["var"][const] == 0).all() and (got["mean"][const] == mu[const]).all()


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_orth(sa, caps, l, d):
    rows = caps[1] + d
    rng = np.random.default_rng(100 + l)
    Y = rng.normal(size=(rows, l)) @ np.diag(np.logspace(0, 3, l)) @ (np.eye(l) + 0.3 * rng.normal(size=(l, l)))
    Q, Qr = gpu_orth(sa, Y), ref.orth(Y)

    def figures(Q):
        return np.abs(Q.T @ Q - np.eye(l)).max(), np.linalg.norm(Y - Q @ (Q.T @ Y)) / np.linalg.norm(Y)

    (g1, g2), (r1, r2) = figures(Q), figures(Qr)
    print(f"orth rows {rows} l {l}: gpu {g1:.2e} {g2:.2e} reference {r1:.2e} {r2:.2e}")
    assert g1 <= 100 * max(r1, U) and g2 <= 100 * max(r2, U)


def test_orth_of_few_rows(sa):
    for rows, l in ((1, 1), (2, 2), (129, 128), (70, 65)):
        Y = np.random.default_rng(rows).normal(size=(rows, l))
        Q = gpu_orth(sa, Y)
        assert np.abs(Q.T @ Q - np.eye(l)).max() <= 100 * max(np.abs(ref.orth(Y).T @ ref.orth(Y) - np.eye(l)).max(), U)


# ---- whole calls ------------------------------------------------------------------------------------------------------------------------
CONFIGS = [("small", False), ("small", True), ("large", False), ("large", True)]


@pytest.fixture(scope="module")
def fits(sa):
    """the GPU fit of every planted input, made once"""
    cache = {}

    def get(name, scale):
        if (name, scale) not in cache:
            X, p, k = ref.planted_case(name)
            cache[name, scale] = sa.expression_pca(X, k, scale=scale)
        return cache[name, scale]

    return get


@pytest.mark.parametrize("name,scale", CONFIGS)
def test_fit_against_the_reference(sa, fits, name, scale):
    r, got = ref.reference_run(name, scale), fits(name, scale)
    want, sp_, p = r["fit"], r["spread"], r["planted"]
    ds = np.abs(got["singular_values"] - want["singular_values"]).max() / want["singular_values"][0]
    dsc = np.abs(got["scores"] - want["scores"]).max() / np.abs(want["scores"]).max()
    dl = np.abs(got["loadings"] - want["loadings"]).max()
    err = np.abs(got["singular_values"] - r["dense"]) / r["dense"]
    print(f"{name} scale {scale}: s {ds:.2e} (spread {sp_['s']:.2e}) scores {dsc:.2e} ({sp_['scores']:.2e}) loadings {dl:.2e} "
          f"({sp_['loadings']:.2e}); planted against dense {err[:p].max():.2e} (reference {r['err'][:p].max():.2e})")
    assert ds <= 100 * sp_["s"] and dsc <= 100 * sp_["scores"] and dl <= 100 * sp_["loadings"]
    assert (err[:p] <= 2 * r["err"][:p]).all()
    n = want["scores"].shape[0]
    assert np.array_equal(got["sdev"], got["singular_values"] / np.sqrt(n - 1.0))
    X = ref.planted_case(name)[0]
    T, mu, var, nnz, stored, w = ref_stats(X, scale=scale)
    assert np.allclose(got["center"], mu, rtol=1e-12, atol=1e-300) and np.allclose(got["gene_var"], var, rtol=1e-11, atol=1e-300)
    assert np.allclose(got["scale"], want["scale"], rtol=1e-12) and np.isclose(got["total_var"], want["total_var"], rtol=1e-11)
    assert (got["normalize_total"], got["log1p"], got["scaled"], got["n_components"], got["oversample"], got["n_iter"]) == \
        (1e4, True, scale, ref.PLANTED[name][3], 10, 4)


def test_two_calls_and_ragged_blocks_give_the_same_bits(sa, fits):
    X, p, k = ref.planted_case("small")
    a = fits("small", True)
    b = sa.expression_pca(X, k, scale=True)
    n = X.shape[1]
    c = sa.expression_pca(ref.ragged(X, [401, 402, 1101]), k, scale=True)
    for key in ("scores", "loadings", "singular_values", "sdev", "center", "scale", "gene_var"):
        assert a[key].tobytes() == b[key].tobytes() == c[key].tobytes(), key
    assert a["total_var"] == b["total_var"] == c["total_var"] and n == 1500
    other = sa.expression_pca(X, k, scale=True, seed=1)
    assert other["scores"].tobytes() != a["scores"].tobytes()
    assert np.allclose(other["singular_values"][:p], a["singular_values"][:p], rtol=1e-4)


def product_bound_of_the_transform(X, fit):
    T, _ = ref.transform(X, fit["normalize_total"], fit["log1p"])
    return ref.spmm_cells_bound(T, fit["center"], 1.0 / fit["scale"], fit["loadings"])


@pytest.mark.parametrize("name,scale", CONFIGS)
def test_transform_against_the_reference_formula(sa, fits, name, scale):
    X, fit = ref.planted_case(name)[0], fits(name, scale)
    got = sa.expression_pca_transform(X, fit)
    within(got, ref.pca_transform(X, fit), product_bound_of_the_transform(X, fit), "transform")
    # block-wise calls give the bits of one call
    parts = ref.ragged(X, [1, 700, 700, 1203])
    assert np.concatenate([sa.expression_pca_transform(b, fit) for b in parts]).tobytes() == got.tobytes()
    assert sa.expression_pca_transform(parts, fit).tobytes() == got.tobytes()
    assert sa.expression_pca_transform(X[:, :0], fit).shape == (0, fit["n_components"])


@pytest.mark.parametrize("name,scale", [("small", False), ("large", True)])
def test_gene_stats_equals_the_fit(sa, fits, name, scale):
    X, fit = ref.planted_case(name)[0], fits(name, scale)
    st = sa.gene_stats(X)
    assert st["mean"].tobytes() == fit["center"].tobytes() and st["var"].tobytes() == fit["gene_var"].tobytes()


@pytest.mark.parametrize("name,k", [("m1", 1), ("n2", 1)])
def test_the_smallest_inputs(sa, cases, name, k):
    """m = 1 with l = 1, and n = 2 (rank 1 after centring): one component, which every step of the iteration reproduces"""
    X = cases[name]
    got, want = sa.expression_pca(X, k, oversample=0), ref.pca(X, k, oversample=0)
    N = max(np.diff(X.indptr).max(), np.diff(X.tocsr().indptr).max())
    tol = 100 * (N + 8) * U
    assert np.abs(got["singular_values"] - want["singular_values"]).max() <= tol * want["singular_values"][0]
    assert np.abs(got["scores"] - want["scores"]).max() <= tol * np.abs(want["scores"]).max()
    assert np.abs(got["loadings"] - want["loadings"]).max() <= tol


def raw_pca(sa, colptr, rowidx, val, m, k=3, over=2, total=1e4, lg=1):
    """sharp_expr_pca_csc on one hand-made block, past the package's checks -> (status, message)"""
    from sharp_amd._lib import f64, i32, i64

    colptr, rowidx, val = np.asarray(colptr, np.int32), np.asarray(rowidx, np.int32), np.asarray(val, np.float64)
    n = colptr.size - 1
    ncb = np.array([n], np.int64)
    P = lambda a: (C.c_void_p * 1)(a)     # noqa: E731
    out = [np.zeros(n * k), np.zeros(m * k), np.zeros(k), np.zeros(k), np.zeros(m), np.zeros(m), np.zeros(m)]
    tv = C.c_double()
    rc = sa.lib().sharp_expr_pca_csc(P(i32(colptr)), P(i32(rowidx)), P(f64(val)), i64(ncb), 1, m, k, over, 2, total, lg, 0, 0,
                                     *[f64(o) for o in out], C.byref(tv))
    return rc, sa.lib().sharp_last_error().decode()


def test_refusals(sa):
    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    cp, ri, vx = X.indptr.copy(), X.indices.copy(), X.data.copy()
    c = int(np.flatnonzero(np.diff(cp) >= 2)[3])               # a cell with two entries or more
    a = cp[c]
    assert raw_pca(sa, cp, ri, vx, 40)[0] == 0
    bad = ri.copy()
    bad[a], bad[a + 1] = ri[a + 1], ri[a]
    rc, msg = raw_pca(sa, cp, bad, vx, 40)
    assert rc != 0 and f"expression_pca: gene indices must be strictly ascending within a cell (cell {c}, counted from 0)" in msg
    bad = ri.copy()
    bad[a + 1] = bad[a]
    assert "strictly ascending within a cell (cell %d," % c in raw_pca(sa, cp, bad, vx, 40)[1]
    for v in (40, -1, 2 ** 31 - 1):
        bad = ri.copy()
        bad[a + 1] = v
        rc, msg = raw_pca(sa, cp, bad, vx, 40)
        assert rc != 0 and f"expression_pca: a gene index outside [0, m) (cell {c}, counted from 0)" in msg
    bad = vx.copy()
    bad[a] = -1.0
    rc, msg = raw_pca(sa, cp, ri, bad, 40)
    assert rc != 0 and f"expression_pca: a negative value under normalize_total / log1p (cell {c}, counted from 0)" in msg
    assert raw_pca(sa, cp, ri, bad, 40, total=0.0, lg=0)[0] == 0          # (no transform: a negative value is a value)
    for v in (np.nan, np.inf):
        bad = vx.copy()
        bad[a + 1] = v
        rc, msg = raw_pca(sa, cp, ri, bad, 40)
        assert rc != 0 and f"expression_pca: a value that is NaN or infinite (cell {c}, counted from 0)" in msg
    # the first offending cell is named, whatever else is wrong later
    bad = ri.copy()
    bad[a + 1] = 99
    bad[cp[c + 5]] = -3
    assert f"(cell {c}," in raw_pca(sa, cp, bad, vx, 40)[1]
    bad = cp.copy()
    bad[c + 1] = cp[c] - 1
    assert f"expression_pca: colptr decreases (cell {c}, counted from 0)" in raw_pca(sa, bad, ri, vx, 40)[1]
    for kw, msg in (({"k": 120, "over": 9}, "n_components + oversample must be <= 128"), ({"k": 25, "over": 6}, "must be <= min(cells, genes)"),
                    ({"k": 0}, "n_components must be >= 1")):
        rc, got = raw_pca(sa, cp, ri, vx, 40, **kw)
        assert rc != 0 and "expression_pca: " in got and msg in got
    with pytest.raises(sa.SharpError, match="n_components must be >= 1"):
        sa.expression_pca(X, 0)
    with pytest.raises(sa.SharpError, match="a negative value under normalize_total / log1p"):
        sa.expression_pca(sp.csc_matrix((bad_values(vx, a), ri, cp), shape=X.shape), 3)
    # identical cells: the rank refusal
    same = sp.csc_matrix(np.repeat(np.arange(1.0, 41.0)[:, None] % 7, 30, axis=1))
    with pytest.raises(sa.SharpError, match="expression_pca: numerical rank below n_components \\+ oversample"):
        sa.expression_pca(same, 3, oversample=2)
    with pytest.raises(sa.SharpError, match="numerical rank below n_components \\+ oversample"):
        sa.expression_pca(same, 3, oversample=2, scale=True)
    # two distinct cells repeated: rank 1 after centring, below l = 5
    two = sp.csc_matrix(np.concatenate([np.repeat(X[:, :1].toarray(), 15, axis=1), np.repeat(X[:, 1:2].toarray(), 15, axis=1)], axis=1))
    with pytest.raises(sa.SharpError, match="numerical rank below n_components \\+ oversample"):
        sa.expression_pca(two, 3, oversample=2)
    with pytest.raises(ref.RankError):
        ref.pca(two, 3, oversample=2)
    with pytest.raises(ref.RankError):
        ref.pca(same, 3, oversample=2)


def bad_values(vx, a):
    v = vx.copy()
    v[a] = -2.0
    return v


def test_the_workflow(sa):
    """README's idiom: scores -> knn -> louvain_snn"""
    X, lab = ref.planted(1500, 800, 6)
    pc = sa.expression_pca(X, 10)
    nb = sa.knn(pc["scores"], 19)
    lv = sa.louvain_snn(nb[0])
    import _louvain_ref as lref

    assert lref.adjusted_rand(lv["membership"], lab) > 0.95


@pytest.mark.parametrize("name,scale", CONFIGS)
def test_transform_of_the_fitted_cells_equals_scores(sa, fits, name, scale):
    """expression_pca_transform on the fitted cells equals `scores` within the product bound"""
    X, fit = ref.planted_case(name)[0], fits(name, scale)
    got = sa.expression_pca_transform(X, fit)
    p = ref.planted_case(name)[1]
    d = np.abs(got - fit["scores"]).max(0) / np.abs(fit["scores"]).max()
    print(f"{name} scale {scale}: |transform - scores| / max|scores|: planted {d[:p].max():.2e}, noise {d[p:].max():.2e}; "
          f"largest bound {product_bound_of_the_transform(X, fit).max():.2e}")
    within(got, fit["scores"], product_bound_of_the_transform(X, fit), "transform of the fitted cells against scores")
