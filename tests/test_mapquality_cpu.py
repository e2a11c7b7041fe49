"""CPU tests of the map scores: the numpy specification (tests/_mapquality_ref.py) against sklearn, the premises of
the GPU tests (tie-free inputs really are, the lattice really holds ties and copies), knn_recall, and the refusals that need no device."""
import numpy as np
import pytest

import _mapquality_ref as ref


@pytest.fixture(scope="module")
def sharp():
    import sharp_amd

    return sharp_amd


@pytest.mark.parametrize("case", range(3))
def test_reference_equals_sklearn(case):
    """the scores are exact rationals rounded once: the reference and sklearn 1.7 agree to the last bit or two on tie-free input, in
    both directions.  (The third case is Gaussian, not the lattice: sklearn orders exact ties by an unstable sort.)"""
    manifold = pytest.importorskip("sklearn.manifold")
    name, X, K = ref.sklearn_cases()[case]
    Y = ref.map_of(X, 11 + case)
    t, _ = ref.trustworthiness(X, Y, K)
    c, _ = ref.continuity(X, Y, K)
    st, sc = manifold.trustworthiness(X, Y, n_neighbors=K), manifold.trustworthiness(Y, X, n_neighbors=K)
    print(f"{name}, K = {K}: trustworthiness {t} (sklearn {st}), continuity {c} (sklearn {sc})")
    assert 0.5 < t < 1.0 and 0.5 < c < 1.0
    assert abs(t - st) <= 1e-15 and abs(c - sc) <= 1e-15


def test_tie_free_inputs_have_gaps():
    """no rounding of a GEMM-form distance (relative error of a few 1e-16 times a modest cancellation) can reorder a row's distances"""
    for name, X, _ in ref.sklearn_cases()[:2]:
        g = ref.min_relative_gap(X)
        print(f"{name}: smallest relative gap between consecutive distances of a row {g}")
        assert g > 1e-12


def test_lattice_holds_ties_and_copies():
    X = ref.lattice()
    assert X.shape == (257, 3) and X.min() == 0 and X.max() == 3 and np.array_equal(X, np.round(X))
    _, first = np.unique(X, axis=0, return_index=True)
    copies = X.shape[0] - first.size
    D = ref.d2_rows(X, np.arange(257))
    off = ~np.eye(257, dtype=bool)
    tied = np.array([257 - 1 - np.unique(D[i][off[i]]).size for i in range(257)])      # entries that share their distance with an earlier one
    zero = ((D == 0) & off).sum(axis=1)
    print(f"lattice: {copies} rows copy an earlier one, {tied.mean():.1f} tied entries per row, {zero.mean():.2f} rows at distance 0 per row")
    assert copies >= 257 - 64                                      # 4^3 distinct rows at the most
    assert tied.min() >= 256 - 20                                  # sums of three of {0, 1, 4, 9}: fewer than 20 values
    assert (zero > 0).sum() >= copies


def test_reference_ranks_by_hand():
    """five points on a line with a copy: d2 from row 0 = (-, 1, 1, 0, 16); ties to the lower index, the copy counts, self never"""
    X = np.array([[0.0], [1.0], [-1.0], [0.0], [4.0]])
    idx = np.array([[3, 1, 2, 4], [0, 3, 2, 4], [0, 3, 1, 4], [0, 1, 2, 4], [1, 0, 3, 2]], np.int32)
    want = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]], np.int32)
    assert np.array_equal(ref.ranks(X, idx), want)
    assert np.array_equal(ref.knn_lists(X, 4), idx)
    assert np.array_equal(ref.ranks(X, idx[:, ::-1]), want[:, ::-1])
    assert np.array_equal(ref.ranks(X, idx, rows=[4, 0]), want[[4, 0]])
    pen = ref.penalties(np.array([[1, 2, 7], [4, 5, 3]]), 3)
    assert pen.tolist() == [4, 3] and pen.dtype == np.int64
    assert ref.score(pen, 10, 3) == 1.0 - 7 * (2.0 / (10 * 3 * (20.0 - 9.0 - 1.0)))


def test_knn_recall(sharp):
    true = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], np.int32)
    assert sharp.knn_recall(true, true) == 1.0
    assert sharp.knn_recall(true[:, ::-1], true) == 1.0            # by set, not by column
    got = np.array([[3, 9, 1], [7, 8, 9], [3, 1, 0], [2, 9, 9]], np.int64)
    assert sharp.knn_recall(got, true) == (2 + 0 + 3 + 1) / 12
    assert sharp.knn_recall(got[:, :2], true) == (1 + 0 + 2 + 1) / 12          # a narrower list
    assert sharp.knn_recall(np.hstack([got, true[:, :1]]), true[:, :2]) == (1 + 1 + 2 + 1) / 8   # a wider one, fewer true neighbours
    for bad in (lambda: sharp.knn_recall(true[:3], true), lambda: sharp.knn_recall(true.astype(float), true),
                lambda: sharp.knn_recall(true[0], true[0])):
        with pytest.raises(sharp.SharpError, match="knn_recall"):
            bad()


def test_refusals_without_a_device(sharp):
    """each by name, before the library is entered (no device here: a call that got through would say so instead)"""
    X = ref.gaussian(40, 4, 1)
    Y = X[:, :2].copy()
    idx = ref.random_lists(40, 5, 2)
    with pytest.raises(sharp.SharpError, match=r"n_neighbors \(20\) should be less than n_samples / 2 \(20.0\)"):
        sharp.trustworthiness(X, Y, n_neighbors=20)
    with pytest.raises(sharp.SharpError, match=r"n_neighbors \(25\) should be less than n_samples / 2"):
        sharp.continuity(X, Y, n_neighbors=25)
    with pytest.raises(sharp.SharpError, match="X has 40 rows and Y 39"):
        sharp.trustworthiness(X, Y[:39])
    with pytest.raises(sharp.SharpError, match="X has 39 rows and Y 40"):
        sharp.continuity(X[:39], Y)
    with pytest.raises(sharp.SharpError, match="at most 255 neighbours"):
        sharp.neighbor_ranks(ref.gaussian(600, 2, 1), ref.random_lists(600, 256, 1))
    with pytest.raises(sharp.SharpError, match="need n >= 3 rows"):
        sharp.neighbor_ranks(X[:2], np.array([[1], [0]], np.int32))
    with pytest.raises(sharp.SharpError, match="K <= n - 1"):
        sharp.neighbor_ranks(X[:3], np.array([[1, 2, 0]] * 3, np.int32))
    bad = X.copy()
    bad[7, 2] = np.nan
    with pytest.raises(sharp.SharpError, match=r"NA / NaN / Inf or a value beyond 1e100 \(row 8, column 3\)"):
        sharp.neighbor_ranks(bad, idx)
    bad[7, 2] = 1e101
    with pytest.raises(sharp.SharpError, match=r"row 8, column 3"):
        sharp.trustworthiness(bad, Y)
    with pytest.raises(sharp.SharpError, match="have 39 rows, the data 40"):
        sharp.neighbor_ranks(X, idx[:39])
    with pytest.raises(sharp.SharpError, match="must hold integers"):
        sharp.neighbor_ranks(X, idx.astype(np.float64))
    with pytest.raises(sharp.SharpError, match="max_rows_per_launch"):
        sharp.neighbor_ranks(X, idx, max_rows_per_launch=-1)
    with pytest.raises(sharp.SharpError, match="have 39 rows"):
        sharp.trustworthiness(X, Y, neighbors=idx[:39])


def test_entries_report_the_missing_device(sharp, monkeypatch):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    X = ref.gaussian(40, 4, 1)
    idx = ref.random_lists(40, 5, 2)
    with pytest.raises(sharp.SharpError, match="no HIP device"):
        sharp.neighbor_ranks(X, idx)
    with pytest.raises(sharp.SharpError, match="no HIP device"):
        sharp.trustworthiness(X, X[:, :2].copy(), neighbors=idx)


def test_r_side_defines_the_map_scores():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "r", "sharp_hip.R")).read()
    for name in ("sharp_trustworthiness", "sharp_continuity"):
        formals = re.search(r"^%s <- function\(([^)]*)\)" % name, src, re.M).group(1)
        assert [a.split("=")[0].strip() for a in formals.split(",")] == ["X", "Y", "n_neighbors"], name
    assert re.search(r"^sharp_neighbor_ranks <- function\(X, index", src, re.M)
    call = re.search(r'\.C\("sharp_C_neighbor_ranks",(.*?)status = integer\(1\)\)', src, re.S).group(1)
    assert "as.integer(t(index) - 1L)" in call and "as.double(n)" in call           # 1-based at the R boundary, n as a double
