"""t-SNE from given neighbours or distances, the parts that need no device: the numpy helpers of tests/_tsne_nn_ref.py against
tests/_tsne_ref.py, and the refusals sharp_amd.tsne raises before it touches the library."""
import numpy as np
import pytest

import _tsne_nn_ref as nn
import _tsne_ref as ref


def _blobs(n, d, groups, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3, size=(groups, d))
    return centres[rng.integers(0, groups, n)] + spread * rng.normal(size=(n, d))


def _no_library(monkeypatch):
    """any use of the library from here on fails the test"""
    from sharp_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were refused")

    monkeypatch.setattr(_lib, "ensure_init", boom)
    monkeypatch.setattr(_lib, "lib", boom)


def test_helpers_agree_with_the_reference():
    X = _blobs(300, 8, 4, 31)
    X[40] = X[3]                                                     # a zero distance and ties
    K, perp = 30, 10
    ridx, rd2 = ref.knn(X, K)
    D2 = ref.sqdist_rows(X, np.arange(300))
    idx, d2 = nn.knn_from_dist(D2, K)
    assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2)
    P, Pr = nn.joint_p_from_neighbours(idx, d2, perp), ref.joint_p(X, perp)
    assert np.array_equal(P.indptr, Pr.indptr) and np.array_equal(P.indices, Pr.indices) and np.array_equal(P.data, Pr.data)
    d = D2[np.triu_indices(300, 1)]
    assert np.array_equal(nn.square_form(d, 300), D2)


def test_python_side_refusals_come_before_the_library(monkeypatch):
    import sharp_amd
    from sharp_amd import tsne

    _no_library(monkeypatch)
    idx = np.tile(np.arange(1, 11, dtype=np.int32), (40, 1))
    dist = np.ones((40, 10))
    E = sharp_amd.SharpError
    with pytest.raises(E, match="differ in shape"):
        sharp_amd.Rtsne_neighbors(idx, dist[:, :9], perplexity=3)
    with pytest.raises(E, match="n x K matrices"):
        sharp_amd.Rtsne_neighbors(idx.ravel(), dist.ravel(), perplexity=3)
    with pytest.raises(E, match="must hold integers"):
        sharp_amd.Rtsne_neighbors(idx.astype(np.float64), dist, perplexity=3)
    with pytest.raises(E, match="must hold real numbers"):
        sharp_amd.Rtsne_neighbors(idx, dist.astype(complex), perplexity=3)
    with pytest.raises(E, match="at most 255 neighbours"):
        sharp_amd.Rtsne_neighbors(np.zeros((300, 256), np.int32), np.ones((300, 256)), perplexity=3)
    with pytest.raises(E, match="K <= n - 1"):
        sharp_amd.Rtsne_neighbors(np.zeros((10, 10), np.int32), np.ones((10, 10)), perplexity=3)
    with pytest.raises(E, match="Y_init must be an n x dims matrix"):
        sharp_amd.Rtsne_neighbors(idx, dist, perplexity=3, Y_init=np.zeros((40, 3)))
    with pytest.raises(E, match="dims must be 1, 2 or 3"):
        sharp_amd.Rtsne_neighbors(idx, dist, perplexity=3, dims=4)
    with pytest.raises(E, match="repulsion must be one of"):
        sharp_amd.Rtsne_neighbors(idx, dist, perplexity=3, repulsion="fft")
    # distance input
    D = nn.square_form(np.arange(1.0, 46.0), 10)
    A = D.copy()
    A[2, 7] += 1e-12
    for call in (lambda x: sharp_amd.Rtsne(x, is_distance=True, perplexity=2), lambda x: sharp_amd.knn(x, 3, is_distance=True)):
        with pytest.raises(E, match="not symmetric"):
            call(A)
        with pytest.raises(E, match="no such length"):
            call(np.ones(44))
        with pytest.raises(E, match="dist vector or a square matrix"):
            call(np.ones((4, 5)))
        for bad in (-1.0, np.nan, np.inf):
            v = np.arange(1.0, 46.0)
            v[17] = bad
            with pytest.raises(E, match="NA / NaN / Inf or a negative value"):
                call(v)
            with pytest.raises(E, match="NA / NaN / Inf or a negative value"):
                call(nn.square_form(v, 10))
    with pytest.raises(E, match="Y_init must be an n x dims matrix"):
        sharp_amd.Rtsne(D, is_distance=True, perplexity=2, Y_init=np.zeros((9, 2)))
    with pytest.raises(E, match="1 <= K <= 255"):
        sharp_amd.knn(D, 10, is_distance=True)
    with pytest.raises(E, match="1 <= K <= 255"):
        sharp_amd.knn(np.zeros((300, 4)), 256)
    # the condensed form of a matrix: its diagonal is ignored, the order is R's
    Dd = D.copy()
    np.fill_diagonal(Dd, 7.0)
    d, n = tsne._condensed(Dd, "Rtsne")
    assert n == 10 and np.array_equal(d, np.arange(1.0, 46.0))


def test_no_cpu_path_without_a_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import sharp_amd

    X = _blobs(60, 4, 2, 32)
    idx, d2 = ref.knn(X, 9)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.Rtsne_neighbors(idx, d2, perplexity=3, squared=True, max_iter=5)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.knn(X, 9)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.knn(nn.square_form(np.arange(1.0, 46.0), 10), 3, is_distance=True)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.Rtsne(np.arange(1.0, 46.0), is_distance=True, perplexity=2, max_iter=5)
