"""CPU tests that pin tests/_linalg_ref.py -- the numpy restatements tests/test_linalg_gpu.py compares the GEMM and row-preparation
kernels with -- on numpy's own product, on explicit double loops and on the oracle, and that assert the premise of every seeded input on
the restatement alone: what a GPU test relies on (a clamp that is reached, a minimum that is positive, a bound that fp64 arithmetic
meets in another summation order) is shown here, without the kernels."""
import numpy as np
import pytest

import _linalg_ref as R


# ---- gemm_ref -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", R.GEMM_SHAPES)
def test_gemm_ref_is_the_product(M, N, K):
    A, B = R.int_operand(1, K, M), R.int_operand(2, K, N)
    assert A.dtype == np.int64 and A.min() >= -8 and A.max() <= 8
    ref = R.gemm_ref(A, B)
    assert ref.dtype == np.int64 and ref.shape == (M, N)
    assert np.abs(ref).max() <= K * 64 < 2 ** 53                              # exact in fp64 in any order
    assert np.array_equal(ref, A.T @ B)
    assert np.array_equal(ref.astype(np.float64), A.astype(np.float64).T @ B.astype(np.float64))
    X, Y = np.random.default_rng(K).standard_normal((K, M)), np.random.default_rng(K + 1).standard_normal((K, N))
    cont = R.gemm_ref(X, Y)
    assert cont.dtype == np.longdouble
    # numpy's fp64 product is itself a dot product of K terms in some order: it meets the bound the GPU test asserts
    assert np.all(np.abs(X.T @ Y - cont) <= R.gemm_bound(X, Y))


def test_gemm_ref_epilogues_by_hand():
    At = np.array([[1.0, 0.5, -1.0], [1.0, 0.0, -0.5]])                     # K = 2, M = 3
    v = At.T @ At                                                            # [[2, .5, -1.5], [.5, .25, -.5], [-1.5, -.5, 1.25]]
    assert np.array_equal(R.gemm_ref(At, At, 0).astype(np.float64), v)
    assert np.array_equal(R.gemm_ref(At, At, 1).astype(np.float64), [[0, 0.5, 2], [0.5, 0, 1.5], [2, 1.5, 0]])
    assert np.array_equal(R.gemm_ref(At, At, 2).astype(np.float64), [[1, 0.5, -1], [0.5, 1, -0.5], [-1, -0.5, 1]])
    wide = R.gemm_ref(At, np.hstack([At, At]), 1)                            # the diagonal of a matrix that is not square: row == col
    assert wide.shape == (3, 6) and np.all(np.diag(wide) == 0) and wide[0, 3] == 0 and wide[1, 4] == 0.75


@pytest.mark.parametrize("M,N,K", R.EPI_CASES)
def test_epilogue_inputs_reach_both_clamps(M, N, K):
    At, Bt, same = R.eighths_operands(3, K, M, N)
    assert same == (M == N) and (not same or np.array_equal(At, Bt))
    m = At * 8
    assert np.array_equal(m, np.rint(m)) and np.abs(m).max() <= 3
    raw = R.gemm_ref(At, Bt, 0)
    r64 = raw.astype(np.float64)
    assert np.array_equal(r64, raw) and np.array_equal(r64 * 64, np.rint(r64 * 64))          # multiples of 1/64: exact in fp64
    off = ~np.eye(M, N, dtype=bool)
    assert (raw[off] > 1).any() and (raw[off] < -1).any()                    # clamped at +1 AND at -1, beside the diagonal
    d = np.diag(r64)
    assert np.all(d != 1.0) and (d > 1).any()                                # the diagonal is set, not computed
    e1, e2 = R.gemm_ref(At, Bt, 1).astype(np.float64), R.gemm_ref(At, Bt, 2).astype(np.float64)
    assert e1[off].min() == 0.0 and e1[off].max() == 2.0 and e2[off].min() == -1.0 and e2[off].max() == 1.0
    assert np.all(np.diag(e1) == 0.0) and np.all(np.diag(e2) == 1.0)
    assert np.array_equal(e1[off], 1.0 - e2[off])


# ---- nn_ref -------------------------------------------------------------------------------------------------------------------------------
def _nn_loops(Cm, n, square):
    slots = (n + 127) // 128
    out = np.full((slots, n), 1e300)
    for r in range(n):
        for c in range(n):
            if c != r:
                v = Cm[r, c] * Cm[r, c] if square else Cm[r, c]
                out[c // 128, r] = min(out[c // 128, r], v)
    return out


@pytest.mark.parametrize("n", [5, 130])
@pytest.mark.parametrize("square", [0, 1])
def test_nn_ref_equals_a_double_loop(n, square):
    Cm = np.random.default_rng(n).uniform(-2, 2, size=(n, n + 3))            # (a padded matrix: only [:n, :n] counts)
    Cm[np.arange(n), np.arange(n)] = -5.0                                     # a diagonal that would win every minimum
    got = R.nn_ref(Cm, n, square)
    assert got.shape == ((n + 127) // 128, n)
    assert np.array_equal(got, _nn_loops(Cm, n, square))
    if n == 130:
        assert np.all(got[1, :128] < 1e300) and got[0].max() < 1e300


def test_nn_ref_gives_inf_where_a_tile_holds_only_the_row_itself():
    n = 129
    Cm = np.random.default_rng(0).uniform(0.1, 2, size=(n, n))
    got = R.nn_ref(Cm, n, 0)
    assert got[1, 128] == 1e300 and np.all(got[1, :128] == Cm[:128, 128]) and np.all(got[0] < 1e300)
    assert R.nn_ref(Cm[:1, :1], 1, 0).tolist() == [[1e300]]


@pytest.mark.parametrize("n", R.NN_SIZES)
def test_row_minima_inputs_have_positive_minima(n):
    """both inputs of the row-minima test: every row's smallest off-diagonal distance is > 0, so a reduction that let the zero diagonal
    in would differ; the exact input is exact"""
    A = R.nn_exact_operand(7, n)
    assert A.shape == (R.NN_K, n) and np.array_equal(A * 8, np.rint(A * 8)) and np.abs(A * 8).max() <= 3
    raw = R.gemm_ref(A, A, 0)
    assert np.array_equal(raw.astype(np.float64) * 64, np.rint(raw.astype(np.float64) * 64))
    U = R.unit_columns(8, R.NN_K, n)
    assert np.allclose(np.linalg.norm(U, axis=0), 1.0, rtol=0, atol=1e-14) and np.abs(U.sum(0)).max() < 1e-13
    for X in (A, U):
        d = R.gemm_ref(X, X, 1).astype(np.float64)
        assert np.all(np.diag(d) == 0.0)
        for square in (0, 1):
            nn = R.nn_ref(d, n, square)
            row_min = nn.min(axis=0)
            assert np.all(row_min > 0.0) and np.all(row_min < 1e300)
            off = d + np.diag(np.full(n, np.inf))
            assert np.array_equal(row_min, (off * off if square else off).min(axis=1))


# ---- row_prep_ref ---------------------------------------------------------------------------------------------------------------------------
def _rows(n, p, lds=None):
    return R.feature_rows(11, n, p, p if lds is None else lds)


@pytest.mark.parametrize("n,p", [(15, 30), (17, 65), (129, 474)])
def test_row_prep_ref_mode0_matches_oracle(oracle, n, p):
    """1 - U U^T of the prepared rows is the oracle's as.dist(1 - cor(t(scale(t(mat))))) (R/get_opt_hclust.R:71-72)"""
    X = _rows(n, p)
    ref = R.row_prep_ref(X, n, p, 0)
    U = ref["Cr"]
    assert np.abs((U * U).sum(1) - 1).max() < 1e-17 and np.abs(U.sum(1)).max() < 1e-16
    d = (1 - U @ U.T).astype(np.float64)
    want = oracle.cor_dist(oracle.scale_rows(X))
    iu = np.triu_indices(n, 1)
    err = np.abs(d[iu] - want).max()
    print((n, p), "max |1 - U U^T - oracle|", err)
    assert err <= 64 * R.EPS53                       # the oracle rounds its means, sd and covariance to fp64: a handful of half-ulps of values <= 2
    assert np.all(ref["nrm"] == 1)


def test_row_prep_ref_modes_1_and_2_by_hand():
    S = np.array([[1.0, 0.9, 0.8], [0.25, 1.0, 0.7], [0.5, 0.125, 1.0]])    # upper triangle differs from the lower one
    ref = R.row_prep_ref(S, 3, 3, 1)
    assert np.array_equal(ref["D"], [[0, 0.75, 0.5], [0.75, 0, 0.875], [0.5, 0.875, 0]])
    c = S - S.mean(1, keepdims=True)
    assert np.allclose(ref["Cr"].astype(np.float64), c, rtol=0, atol=1e-16)
    assert np.allclose(ref["nrm"].astype(np.float64), np.linalg.norm(c, axis=1), rtol=0, atol=1e-16)
    ref2 = R.row_prep_ref(S, 3, 3, 2)
    assert np.array_equal(ref2["D"], [[0, 0.9, 0.8], [0.25, 0, 0.7], [0.5, 0.125, 0]]) and ref2["Cr"] is None and ref2["nrm"] is None


@pytest.mark.parametrize("n,p", R.ROW_SHAPES)
@pytest.mark.parametrize("pad", [0, 3])
def test_feature_rows_premises_and_bound(n, p, pad):
    """the rows' mean is within 4 sd of zero; the columns beyond p never enter; and plain fp64 arithmetic in another summation order
    than the kernels' stays within the bound the GPU test asserts -- the bound is measured against the reference, not the kernel"""
    X = _rows(n, p, p + pad)
    assert X.shape == (n, p + pad) and np.all(X[:, p:] == 1.0e6)
    assert np.array_equal(X[:, :p], _rows(n, p)[:, :p])
    ref = R.row_prep_ref(X, n, p, 0)
    assert np.all(np.abs(ref["mean"]) <= 4 * ref["sd"]) and np.all(ref["sd"] > 0)
    tol, tol_n = R.row_prep_bounds(ref, p, 0)
    assert tol.shape == (n, 1) and np.all(tol_n == 0)
    got, nrm = R.row_prep_fp64(X, n, p, 0)
    err = np.abs(got - ref["Cr"])
    print((n, p), "fp64 restatement: max error", float(err.max()), "smallest bound", float(tol.min()), "largest bound", float(tol.max()))
    assert np.all(err <= tol) and np.all(nrm == 1.0)
    assert tol.max() < 1e-10                          # ... and the bound still means something: ten digits of a unit vector's entries


@pytest.mark.parametrize("n", R.SIM_SIZES)
def test_similarity_premises_and_bound(n):
    S = R.similarity(12, n)
    iu = np.triu_indices(n, 1)
    assert np.all(np.abs(S[iu] - S.T[iu]) >= 0.01)                           # a read of the wrong triangle shows in the second digit
    assert np.all(np.diag(S) == 1.0)
    ref = R.row_prep_ref(S, n, n, 1)
    assert np.array_equal(ref["D"], ref["D"].T) and np.all(np.diag(ref["D"]) == 0.0)
    il = np.tril_indices(n, -1)
    assert np.array_equal(ref["D"][il], 1.0 - S[il])
    assert np.all(np.abs(ref["mean"]) <= 4 * ref["sd"])
    tol, tol_n = R.row_prep_bounds(ref, n, 1)
    got, nrm = R.row_prep_fp64(S, n, n, 1)
    assert np.all(np.abs(got - ref["Cr"]) <= tol) and np.all(np.abs(nrm - ref["nrm"]) <= tol_n)
    assert tol.max() < 1e-10 and (tol_n / ref["nrm"]).max() < 1e-10


@pytest.mark.parametrize("n", R.DIST_SIZES)
def test_distance_inputs_have_a_diagonal_to_overwrite(n):
    D = R.distances(13, n)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) >= 0.5)
    ref = R.row_prep_ref(D, n, n, 2)
    assert np.all(np.diag(ref["D"]) == 0.0) and np.array_equal(ref["D"] + np.diag(np.diag(D)), D)


def test_sentinel_is_a_nan_that_is_not_numpys():
    s = np.array([R.SENTINEL_BITS]).view(np.float64)[0]
    assert np.isnan(s) and np.array([np.nan]).view(np.uint64)[0] != R.SENTINEL_BITS
