"""The truncated PCA of sparse expression blocks (tests/_expr_pca_ref.py) on the CPU: the reference's implicit products
against a plain dense computation, Omega's bits, the variance formula, the sign rule, convergence on the planted inputs and the
reference's own rounding spread, the premises of the GPU tests' boundary shapes (read from the library's own caps, which need no device),
and the refusals of the package and of the library that need no device.

Convergence: on Poisson counts with planted clusters the G - 1 planted singular values converge (relative error 3e-7 at 1 500 x 800,
2e-8 at 3 000 x 2 000 against the dense spectrum); the components in the noise stay 1 - 6 % off, as for any randomised PCA, and are
not asserted."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _expr_pca_ref as ref


def py_mix(z):
    z &= 2 ** 64 - 1
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & (2 ** 64 - 1)
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & (2 ** 64 - 1)
    z ^= z >> 31
    return z


def test_omega_bits_and_range():
    for seed in (0, 1, 20261019, 2 ** 63 - 1):
        O = ref.omega(seed, np.arange(300), 128)
        assert O.min() >= -0.5 and O.max() < 0.5
        assert (np.ldexp(O + 0.5, 53) == np.round(np.ldexp(O + 0.5, 53))).all()       # multiples of 2^-53
        for g, j in ((0, 0), (1, 0), (0, 1), (299, 127), (17, 64)):
            h = py_mix(py_mix(seed * 0x9E3779B97F4A7C15 + g) + j) >> 11
            assert O[g, j] == h * 2.0 ** -53 - 0.5
    assert abs(ref.omega(3, np.arange(4000), 60).mean()) < 0.01
    # a gene's row follows its id, not its position
    assert np.array_equal(ref.omega(5, [7, 3], 9), ref.omega(5, np.arange(8), 9)[[7, 3]])


@pytest.mark.parametrize("scale", [False, True])
def test_products_against_a_dense_computation(scale):
    X = ref.random_csc(60, 45, 0.2, 1)
    T, L = ref.transform(X)
    assert np.allclose(L, np.asarray(X.sum(0)).ravel())
    D = np.log1p(X.toarray() * np.where(L > 0, 1e4 / np.where(L > 0, L, 1), 0)[None, :])
    assert np.allclose(T.toarray(), D, rtol=1e-14, atol=0)
    mu, var, nnz, stored = ref.gene_stats(T)
    _, w = ref.weights(var, scale)
    A = (D.T - D.mean(1)[None, :]) * w[None, :]
    assert np.allclose(ref.dense_A(X, scale=scale), A, rtol=1e-12, atol=1e-12)
    rng = np.random.default_rng(2)
    B, Q = rng.normal(size=(60, 7)), rng.normal(size=(45, 7))
    Y, Z = ref.spmm_cells(T, mu, w, B), ref.spmm_genes(T.tocsr(), mu, w, Q)
    assert (np.abs(Y - A @ B) <= 4 * ref.spmm_cells_bound(T, mu, w, B) + 1e-300).all()
    assert (np.abs(Z - A.T @ Q) <= 4 * ref.spmm_genes_bound(T, mu, w, Q, stored) + 1e-300).all()


def test_variance_formula():
    X = ref.random_csc(80, 37, 0.3, 3)
    X = sp.vstack([X, sp.csc_matrix(np.full((1, 37), 2.0)), sp.csc_matrix((1, 37))]).tocsc()   # a constant gene and an absent one
    for total, lg in ((1e4, True), (None, False), (None, True)):
        T, _ = ref.transform(X, total, lg)
        mu, var, nnz, stored = ref.gene_stats(T)
        D = T.toarray()
        const = D.min(1) == D.max(1)
        assert const[-1] and (const[-2] or total)
        assert np.allclose(mu, D.mean(1), rtol=1e-13, atol=1e-300)
        assert np.allclose(var[~const], D.var(1, ddof=1)[~const], rtol=1e-12)
        assert (var[const] == 0).all() and (mu[const] == D[const, 0]).all()
        assert np.array_equal(nnz, (D != 0).sum(1))
        sd, w = ref.weights(var, True)
        assert (w[const] == 0).all() and (sd[const] == 1).all() and np.allclose(w[~const] * np.sqrt(var[~const]), 1.0)
        one, w1 = ref.weights(var, False)
        assert (one == 1).all() and (w1 == 1).all()
    with pytest.raises(ValueError, match="negative"):
        ref.transform(sp.csc_matrix(np.array([[1.0, -1.0]])), None, True)
    assert ref.transform(sp.csc_matrix(np.array([[1.0, -1.0]])), None, False)[0].toarray().tolist() == [[1.0, -1.0]]
    # a cell without counts stays zero under normalize_total
    assert (ref.transform(sp.csc_matrix(np.array([[0.0, 2.0], [0.0, 1.0]])))[0].toarray()[:, 0] == 0).all()


def test_sign_rule():
    L = np.array([[0.5, -0.5, 0.1], [-0.5, 0.5, -0.7], [0.2, 0.1, 0.7]])
    S = np.arange(6.0).reshape(2, 3)
    s2, l2 = ref.sign_fix(S, L)
    assert l2[:, 0].tolist() == [0.5, -0.5, 0.2]               # the tie: gene 0 decides and is positive already
    assert l2[:, 1].tolist() == [0.5, -0.5, -0.1]              # the tie: gene 0 decides and is flipped
    assert l2[:, 2].tolist() == [-0.1, 0.7, -0.7]              # gene 1 before gene 2
    assert np.array_equal(s2, S * np.array([1.0, -1.0, -1.0]))


@pytest.mark.parametrize("name", ["small", "large"])
@pytest.mark.parametrize("scale", [False, True])
def test_convergence_and_rounding_spread(name, scale):
    """The planted singular values against the dense spectrum.  The subspace iteration damps the part of component i that lies outside
    the iterated space by (sigma_(l+1) / sigma_i)^(2 q + 1) per HMT's power scheme, and a singular value's error is the square of its
    vector's; sigma_(l+1) <= sigma_k, so (sigma_k / sigma_i)^(2 q + 1), q = n_iter = 4, bounds the relative error with room."""
    r = ref.reference_run(name, scale)
    p, dense, err, fit = r["planted"], r["dense"], r["err"], r["fit"]
    n, m, G, k = ref.PLANTED[name]
    print(name, scale, "planted", err[:p].max(), "noise", err[p:].min(), err[p:].max(), "cond", r["max_cond"], "spread", r["spread"])
    assert p == G - 1 and dense.size == k
    assert (err[:p] <= (dense[k - 1] / dense[:p]) ** 9).all()
    assert dense[p - 1] > 1.5 * dense[p]                      # the planted components stand clear of the noise
    assert r["max_cond"] < 1e3                                 # CholeskyQR2 is safe far beyond this
    assert np.allclose(fit["loadings"].T @ fit["loadings"], np.eye(k), atol=1e-12)
    # scores = A loadings: a converged component's column has the norm s; the noise components' are not asserted
    assert np.allclose(np.linalg.norm(fit["scores"][:, :p], axis=0), fit["singular_values"][:p], rtol=1e-4)
    X = ref.planted_case(name)[0]
    assert np.abs(ref.pca_transform(X, fit) - fit["scores"]).max() <= 1e-12 * np.abs(fit["scores"]).max()
    assert (fit["loadings"][np.argmax(np.abs(fit["loadings"]), 0), np.arange(k)] > 0).all()
    assert np.allclose(fit["sdev"], fit["singular_values"] / np.sqrt(n - 1.0))
    assert fit["total_var"] >= (fit["sdev"] ** 2).sum() and ((fit["scale"] == 1).all() or scale)
    # the reference's own rounding spread over three storage orders: rounding, not algorithm
    s = r["spread"]
    assert 0 < s["s"] < 1e-13 and 0 < s["scores"] < 1e-11 and 0 < s["loadings"] < 1e-11


def test_premises_of_the_gpu_boundary_cases():
    from sharp_amd import expr_pca

    chunk, slab = expr_pca._row_caps()
    assert 64 < chunk <= 4096 and 1024 <= slab <= 65536
    cases = ref.stage_cases(chunk, slab)
    cells = np.diff(cases["cells"].indptr)
    assert cells[:6].tolist() == [0, 1, 63, 64, 65, cases["cells"].shape[0]]
    genes = np.diff(cases["genes"].tocsr().indptr)
    assert genes[:6].tolist() == [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    full = cases["full"]
    assert full.shape[1] == 4099 and np.diff(full.tocsr().indptr)[0] == 4099
    assert [cases["slab%+d" % d].shape[1] for d in (-1, 0, 1)] == [slab - 1, slab, slab + 1]
    big = cases["m70000"]
    assert big.shape[0] == 70000 and 2000 < big.nnz < 10000 and big.indices.max() > 65535
    assert cases["n2"].shape[1] == 2
    mixed = cases["cells"].data
    assert (mixed == 0).any() and (mixed.astype(np.float32).astype(np.float64) != mixed).any()      # stored zeros; values fp32 cannot hold
    for X in cases.values():
        assert X.has_sorted_indices and (np.diff(X.indices)[np.diff(np.repeat(np.arange(X.shape[1]), np.diff(X.indptr))) == 0] > 0).all()
    parts = ref.ragged(cases["cells"], [0, 70, 70, 200])
    assert [b.shape[1] for b in parts] == [0, 70, 0, 130, 0] and ref.concat(parts).data.tobytes() == cases["cells"].data.tobytes()


def test_refusals_that_need_no_device():
    import sharp_amd as sa

    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    for kw, msg in (({"n_components": 0}, "n_components must be >= 1"), ({"n_components": 120, "oversample": 9}, "must be <= 128"),
                    ({"n_components": 25, "oversample": 6}, r"must be <= min\(cells, genes\)"), ({"center": False}, "uncentred variant is out of scope"),
                    ({"oversample": -1}, "oversample must be >= 0"), ({"normalize_total": -1.0}, "normalize_total must be None or a positive"),
                    ({"normalize_total": float("nan")}, "normalize_total"), ({"n_iter": -1}, "n_iter must be in"), ({"seed": -1}, "seed must be in")):
        with pytest.raises(sa.SharpError, match="expression_pca: .*" + msg):
            sa.expression_pca(X, **dict({"n_components": 5}, **kw))
    bad = X.copy()
    bad.data[5] = np.nan
    with pytest.raises(sa.SharpError, match="expression_pca: a value that is NaN or infinite"):
        sa.expression_pca(bad, 5)
    bad.data[5] = -1.0
    with pytest.raises(sa.SharpError, match="expression_pca: a negative value under normalize_total / log1p"):
        sa.expression_pca(bad, 5)
    with pytest.raises(sa.SharpError, match="gene_stats: a negative value"):
        sa.gene_stats(bad)
    with pytest.raises(sa.SharpError, match="every block must have the same genes"):
        sa.expression_pca([X, X[:39]], 5)
    with pytest.raises(sa.SharpError, match="No expression data is provided"):
        sa.expression_pca([], 5)
    with pytest.raises(sa.SharpError, match="need at least 2 cells"):
        sa.expression_pca(X[:, :1], 1, oversample=0)
    with pytest.raises(sa.SharpError, match="fit must be what expression_pca"):
        sa.expression_pca_transform(X, {"loadings": np.zeros((40, 3))})
    fit = {"loadings": np.zeros((41, 3)), "center": np.zeros(41), "scale": np.ones(41), "normalize_total": 1e4, "log1p": True}
    with pytest.raises(sa.SharpError, match="the new cells have 40 genes, the fit has 41"):
        sa.expression_pca_transform(X, fit)
    fit["center"] = np.zeros(40)
    with pytest.raises(sa.SharpError, match="do not belong together"):
        sa.expression_pca_transform(X, fit)


def test_the_library_refuses_again_without_the_package():
    """what reaches the library without the package's checks is refused by name before any device work"""
    from sharp_amd import expr_pca
    from sharp_amd._lib import f64, lib

    X = ref.random_csc(40, 30, 0.3, 1, kind="counts")
    args, keep = expr_pca._pointers([X])
    out = [np.zeros(30 * 128), np.zeros(40 * 128), np.zeros(128), np.zeros(128), np.zeros(40), np.zeros(40), np.zeros(40)]
    tv = C.c_double()

    def call(m=40, k=5, over=2, n_iter=2, total=1e4, a=args):
        rc = lib().sharp_expr_pca_csc(*a, m, k, over, n_iter, total, 1, 0, 0, *[f64(o) for o in out], C.byref(tv))
        return rc, lib().sharp_last_error()

    for kw, msg in (({"k": 0}, b"expression_pca: n_components must be >= 1"), ({"k": 120, "over": 9}, b"n_components + oversample must be <= 128"),
                    ({"k": 25, "over": 6}, b"must be <= min(cells, genes)"), ({"over": -1}, b"oversample must be >= 0"),
                    ({"m": 0}, b"need 1 <= m <= 16777216 genes"), ({"total": -1.0}, b"normalize_total must be finite and >= 0"),
                    ({"n_iter": -1}, b"n_iter must be in 0 .. 1000"), ({"a": args[:4] + (0,)}, b"need a list of at least one block")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
    rc, err = call()
    assert rc != 0 and (b"no device context" in err or b"no HIP device" in err) or rc == 0       # (0: a GPU is present)
    q = np.zeros((30, 3))
    assert lib().sharp_expr_orth(f64(q), 2, 3, f64(q)) != 0 and b"expr_orth: need l <= rows" in lib().sharp_last_error()
    assert lib().sharp_expr_orth(f64(q), 30, 129, f64(q)) != 0 and b"need 1 <= l <= 128 columns" in lib().sharp_last_error()
    del keep
