"""t-SNE without a GPU: the numpy reference of DESIGN.md §10 (tests/_tsne_ref.py) against sklearn and against finite differences,
the C ABI of sharp_tsne / sharp_C_tsne (declared, exported, failing loudly without a device), visualization_SHARP's x1 and its figure."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _tsne_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blobs(n, d, groups, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3, size=(groups, d))
    lab = rng.integers(0, groups, n)
    return centres[lab] + spread * rng.normal(size=(n, d)), lab


def test_reference_p_matches_sklearn_joint_probabilities_nn():
    import scipy.sparse as sp
    from sklearn.manifold._t_sne import _joint_probabilities_nn

    X, _ = _blobs(400, 10, 4, 1)
    X = ref.normalize(X)
    perp = 20
    K = int(np.floor(3 * perp))
    idx, dist = ref.knn(X, K)
    n = X.shape[0]
    D = sp.csr_matrix((dist.ravel(), idx.ravel(), np.arange(0, n * K + 1, K)), shape=(n, n))
    P_sk = _joint_probabilities_nn(D, perp, 0).toarray()
    P_ref = ref.joint_p(X, perp).toarray()
    np.testing.assert_allclose(P_ref, P_sk, rtol=1e-4, atol=1e-4 * P_sk.max())
    assert abs(P_ref.sum() - 1.0) < 1e-12 and np.allclose(P_ref, P_ref.T, rtol=0, atol=1e-18)


def test_reference_gradient_is_the_kl_derivative_over_four():
    X, _ = _blobs(60, 5, 3, 2)
    P = ref.joint_p(ref.normalize(X), 5)
    Y = np.random.default_rng(3).normal(size=(60, 2))
    g = ref.gradient(P, Y)
    h = 1e-6
    fd = np.zeros_like(Y)
    for i in range(Y.shape[0]):
        for k in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, k] += h
            Ym[i, k] -= h
            fd[i, k] = (ref.kl(P, Yp) - ref.kl(P, Ym)) / (2 * h)
    np.testing.assert_allclose(g, fd / 4.0, rtol=1e-5, atol=1e-5 * np.abs(fd / 4).max())


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_reference_multiset_and_chunked_repulsion_match_the_dense_gradient(dims):
    """multiset_repulsion (m distinct positions with multiplicities) and exact_repulsion (row chunks) against ref.gradient's dense
    n x n pass: with an empty P the gradient is -rep / Z"""
    import scipy.sparse as sp

    rng = np.random.default_rng(40 + dims)
    m, n = 37, 900
    pos = rng.normal(size=(m, dims)) * 3
    cnt = rng.multinomial(n - m, np.full(m, 1.0 / m)) + 1
    assign = rng.permutation(np.repeat(np.arange(m), cnt))
    Y = pos[assign]
    g, Z = ref.gradient(sp.csr_matrix((n, n)), Y, return_z=True)
    rep, z, A = ref.multiset_repulsion(pos, cnt)
    Zm = float(cnt @ z)
    assert abs(Zm - Z) <= 1e-12 * Z
    np.testing.assert_allclose(-rep[assign] / Zm, g, rtol=0, atol=1e-12 * np.abs(g).max())
    # A: the sum of the magnitudes of rep's terms, by the definition
    d = Y[:, None, :] - Y[None, :, :]
    q2 = 1.0 / (1.0 + (d ** 2).sum(-1)) ** 2
    np.testing.assert_allclose(A[assign], (q2[:, :, None] * np.abs(d)).sum(1), rtol=1e-12, atol=0)
    assert (np.abs(rep) <= A).all()
    # all rows distinct, n no multiple of the chunk, and a chunk length of its own
    Yd = rng.normal(size=(333, dims)) * 3
    gd, Zd = ref.gradient(sp.csr_matrix((333, 333)), Yd, return_z=True)
    for chunk in (32, 100):
        rep, z, A = ref.exact_repulsion(Yd, chunk)
        assert abs(z.sum() - Zd) <= 1e-12 * Zd
        np.testing.assert_allclose(-rep / z.sum(), gd, rtol=0, atol=1e-12 * np.abs(gd).max())
    repm, zm, Am = ref.multiset_repulsion(Yd, np.ones(333))
    assert np.array_equal(repm, ref.exact_repulsion(Yd)[0]) and np.array_equal(Am, ref.exact_repulsion(Yd)[2])


def test_reference_calibration_trace_against_a_row_at_a_time_bisection():
    """calibrate(return_trace=True): the same P as without, and per row the steps and the stop margin of a scalar restatement of
    bhtsne's loop; rows that double beta for long (a tight clump) and rows that halve it (distances in the hundreds)"""
    X, _ = _blobs(300, 6, 3, 6)
    X[50:120] = X[50] + 1e-4 * np.random.default_rng(7).normal(size=(70, 6))
    X[200:] *= 30.0
    perp, K = 10, 30
    _, dist = ref.knn(X, K)
    P = ref.calibrate(dist, perp)
    Pt, steps, margin = ref.calibrate(dist, perp, return_trace=True)
    assert np.array_equal(P, Pt) and steps.shape == margin.shape == (300,)
    logU = np.log(perp)
    betas = np.zeros(300)
    for i in range(300):
        beta, lo, hi, n_steps, mg = 1.0, -ref.DBL_MAX, ref.DBL_MAX, 0, np.inf
        for _ in range(200):
            p = np.exp(-beta * dist[i])
            s = ref.DBL_MIN + p.sum()
            Hdiff = (beta * (dist[i] * p)).sum() / s + np.log(s) - logU
            n_steps += 1
            mg = min(mg, abs(abs(Hdiff) - 1e-5))
            if Hdiff < 1e-5 and -Hdiff < 1e-5:
                break
            if Hdiff > 0:
                lo = beta
                beta = beta * 2.0 if hi == ref.DBL_MAX else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -ref.DBL_MAX else (beta + lo) / 2.0
        betas[i] = beta
        assert steps[i] == n_steps and margin[i] == mg, i
        np.testing.assert_allclose(Pt[i], p / s, rtol=1e-15, atol=0)
    assert betas[50:120].min() > 2.0 ** 20 and betas[200:].max() < 0.25 and steps.max() < 200


def _declared():
    src = open(os.path.join(ROOT, "include", "sharp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(sharp_[A-Za-z0-9_]+)\s*\(", src))


@pytest.fixture(scope="module")
def so():
    import __graft_entry__ as g

    path = os.path.join(ROOT, "sharp_amd", "libsharp_hip.so")
    if not os.path.exists(path):
        g.build()
    return C.CDLL(path)


def test_tsne_entries_declared_and_exported(so):
    names = _declared()
    for n in ["sharp_tsne", "sharp_C_tsne", "sharp_tsne_prepare", "sharp_tsne_knn", "sharp_tsne_affinities", "sharp_tsne_gradient"]:
        assert n in names, n
        assert hasattr(so, n), n


def test_tsne_without_a_device_fails_loudly(so):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    so.sharp_last_error.restype = C.c_char_p
    X = np.random.default_rng(0).normal(size=(100, 5))
    Y = np.zeros((100, 2))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))       # noqa: E731
    rc = so.sharp_tsne(dp(X), C.c_longlong(100), 5, C.c_longlong(5), 2, 50, 1, 1, 0, 1, 1, C.c_double(10.0), C.c_double(0.5), 10, 250, 250,
                       C.c_double(0.5), C.c_double(0.8), C.c_double(200.0), C.c_double(12.0), None, C.c_double(10.0), dp(Y), None, None)
    assert rc != 0 and b"no device context" in so.sharp_last_error()
    st = np.array([-1], np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    I = lambda v: np.array([v], np.int32)                           # noqa: E731
    D = lambda v: np.array([v], np.float64)                         # noqa: E731
    so.sharp_C_tsne.restype = None
    ic, costs = np.zeros(20), np.zeros(100)
    args = [X, D(100), I(5), I(2), I(50), I(1), I(1), I(0), I(1), I(1), D(10.0), D(0.5), I(10), I(250), I(250), D(0.5), D(0.8), D(200.0),
            D(12.0), I(0), np.zeros(1), D(10.0), Y, ic, costs, st]
    so.sharp_C_tsne(*[P(a) for a in args])
    assert st[0] != 0
    import sharp_amd

    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.Rtsne(X, perplexity=10, max_iter=10)


def _result(n=80, p=7, ncl=3, seed=4, sparse=False):
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, ncl + 1, n)
    lab[:ncl] = np.arange(1, ncl + 1)
    x0 = np.eye(ncl)[lab - 1]
    if sparse:
        import scipy.sparse as sp

        x0 = sp.csr_matrix(x0)
    return {"x0": x0, "viE": rng.normal(size=(n, p)), "pred_clusters": lab}


def test_vis_input_three_branches_against_numpy():
    from sharp_amd.api import _vis_input

    y = _result()
    x0, viE = y["x0"], y["viE"]
    sc = lambda a: (a - a.mean(0)) / a.std(0, ddof=1)                # noqa: E731
    np.testing.assert_allclose(_vis_input(y, 2), np.hstack([2 * sc(x0), sc(viE)]), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(_vis_input(y, 0.5), np.hstack([0.5 * sc(x0), sc(viE)]), rtol=1e-14, atol=1e-14)
    assert np.array_equal(_vis_input(y, 0.01), viE)
    j = _vis_input(y, 100)
    z = x0.max() - x0.min()
    assert j.shape == x0.shape and np.abs(j - x0).max() <= z / 50 and np.abs(j - x0).max() > 0
    ys = _result(sparse=True)
    np.testing.assert_allclose(_vis_input(ys, 2), _vis_input(y, 2), rtol=0, atol=0)
    np.testing.assert_allclose(_vis_input(ys, 1000), _vis_input(y, 1000), rtol=0, atol=0)


def test_vis_input_constant_column_is_an_error_naming_it():
    import sharp_amd
    from sharp_amd.api import _vis_input

    y = _result()
    y["viE"][:, 4] = 1.5
    with pytest.raises(sharp_amd.SharpError, match="column 5 of viE"):
        _vis_input(y, 2)
    y = _result()
    y["x0"] = np.hstack([y["x0"], np.zeros((y["x0"].shape[0], 1))])
    with pytest.raises(sharp_amd.SharpError, match="column 4 of x0"):
        _vis_input(y, 2)


@pytest.mark.parametrize("filetype", ["png", "pdf"])
def test_figure_from_given_coordinates(tmp_path, filetype):
    from sharp_amd.api import _draw_sharp_map, vis_colors

    assert len(vis_colors) == 40 and vis_colors[0] == "black" and vis_colors[-1] == "lightcyan"
    import sys

    had_pyplot = "matplotlib.pyplot" in sys.modules
    Y = np.random.default_rng(5).normal(size=(300, 2))
    lab = np.repeat(np.arange(45), 300 // 45 + 1)[:300]            # more labels than colours: recycled
    f1 = str(tmp_path / f"lab.{filetype}")
    _draw_sharp_map(Y, lab, f1, filetype, res=50)
    f2 = str(tmp_path / f"nolab.{filetype}")
    _draw_sharp_map(Y, None, f2, filetype, res=50)
    assert "matplotlib.pyplot" not in sys.modules or had_pyplot       # the figure leaves pyplot (and its backend) alone
    magic = b"\x89PNG" if filetype == "png" else b"%PDF"
    for f in (f1, f2):
        assert os.path.getsize(f) > 1000
        assert open(f, "rb").read(4) == magic


def test_the_refusal_tests_unspoiled_lists_are_sound():
    """the premise of tests/test_neighbour_refusals_gpu.py: before a list is spoiled, the lists of its input pass the host check and
    name, in every row, K different rows in range, none of them the row itself"""
    from sharp_amd.tsne import _neighbour_arrays
    from test_neighbour_refusals_gpu import K, N, gaussian

    idx, dist = ref.knn(gaussian(), K)
    index, distance = _neighbour_arrays(idx, dist, "Rtsne_neighbors")
    assert index.shape == distance.shape == (N, K) and index.dtype == np.int32 and distance.dtype == np.float64
    assert ((index >= 0) & (index < N)).all() and (index != np.arange(N)[:, None]).all()
    s = np.sort(index, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), "an index twice in a row"
    assert np.isfinite(distance).all() and (distance >= 0).all()
