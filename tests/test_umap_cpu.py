"""UMAP without a GPU: the a / b curve fit of the library (sharp_umap_ab needs no device), the premises of the numpy
reference the GPU tests compare against (tests/_umap_ref.py), the refusals that happen before the library, and the quality of the
reference run that the GPU's full run is measured against."""
import ctypes as C

import numpy as np
import pytest

import _umap_ref as ref

CURVES = [(1.0, 0.01), (1.0, 0.1), (1.0, 0.5), (2.0, 0.001)]
# Against scipy.optimize.curve_fit (its default tolerances, p0 = (1, 1)) the largest |difference| in a or b over CURVES was measured at
# 5.03e-7 (scipy stops at ftol = 1e-8; the library's fit is at first-order optimality to 1e-14): a factor 10 on that.  DESIGN.md §13.
SCIPY_TOL = 5e-6


@pytest.fixture(scope="module")
def sharp():
    import os

    import __graft_entry__ as g

    import sharp_amd

    if not os.path.exists(sharp_amd.so_path()):
        g.build()
    return sharp_amd


# ---- 1. the curve ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread,min_dist", CURVES)
def test_curve_fit_is_first_order_optimal(sharp, spread, min_dist):
    a, b = sharp.umap_ab(spread, min_dist)
    assert a > 0 and b > 0
    r, J = ref.curve_residual_jacobian(a, b, spread, min_dist)
    assert np.linalg.norm(J.T @ r) <= 1e-8 * np.linalg.norm(J) * np.linalg.norm(r)


def test_curve_fit_agrees_with_scipy(sharp):
    opt = pytest.importorskip("scipy.optimize")
    worst = 0.0
    for spread, min_dist in CURVES:
        a, b = sharp.umap_ab(spread, min_dist)
        x, y = ref.curve_points(spread, min_dist)
        p, _ = opt.curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2.0 * b)), x, y)
        worst = max(worst, abs(p[0] - a), abs(p[1] - b))
    print("largest |a or b difference| against scipy:", worst)
    assert worst <= SCIPY_TOL


@pytest.mark.parametrize("spread,min_dist,what", [(1.0, 3.0, "below 3 spread"), (1.0, 3.5, "below 3 spread"), (0.0, 0.1, "spread must be positive"),
                                                  (-1.0, 0.1, "spread must be positive"), (np.nan, 0.1, "finite"), (1.0, np.inf, "finite"),
                                                  (np.inf, 0.1, "finite"), (1.0, -0.1, "min_dist must be >= 0")])
def test_curve_refusals(sharp, spread, min_dist, what):
    with pytest.raises(sharp.SharpError, match=what):
        sharp.umap_ab(spread, min_dist)


def test_curve_dotc_twin_needs_no_device(sharp):
    L = sharp.lib()
    a, b, st = (C.c_double * 1)(), (C.c_double * 1)(), (C.c_int * 1)(-1)
    L.sharp_C_umap_ab((C.c_double * 1)(1.0), (C.c_double * 1)(0.01), a, b, st)
    assert st[0] == 0 and (a[0], b[0]) == sharp.umap_ab(1.0, 0.01)
    L.sharp_C_umap_ab((C.c_double * 1)(1.0), (C.c_double * 1)(4.0), a, b, st)
    assert st[0] == 2                                                # SHARP_ERR_ARG


# ---- 2. premises of the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 40, 1025, 2 ** 20, 2 ** 31 - 1, 3 * 2 ** 29])
def test_draw_is_in_range(n):
    e = np.arange(20000, dtype=np.uint64) * np.uint64(7919)
    for ep, s in ((0, 0), (1, 4), (499, 2)):
        k = ref.draw(10, ep, e, s, n)
        assert k.min() >= 0 and k.max() < n
    # the largest 53-bit fraction still lands below n
    assert np.floor(float(2 ** 53 - 1) * 2.0 ** -53 * float(n)) < n
    if n >= 40:
        assert np.unique(ref.draw(10, 1, e, 0, n)).size > 30         # (it does spread)


def test_draw_depends_on_seed_epoch_edge_and_sample():
    e = np.arange(1000, dtype=np.uint64)
    base = ref.draw(10, 3, e, 1, 10 ** 6)
    for other in (ref.draw(11, 3, e, 1, 10 ** 6), ref.draw(10, 4, e, 1, 10 ** 6), ref.draw(10, 3, e + np.uint64(1), 1, 10 ** 6),
                  ref.draw(10, 3, e, 2, 10 ** 6)):
        assert (other != base).mean() > 0.99
    assert np.array_equal(ref.draw(-1, 3, e, 1, 10 ** 6), ref.draw(2 ** 64 - 1, 3, e, 1, 10 ** 6))   # (the seed is taken mod 2^64)


@pytest.mark.parametrize("n_epochs", [1, 2, 7, 200, 500])
def test_firing_count_over_a_run(n_epochs):
    r = np.concatenate([[0.0, 1.0, 1.0 / n_epochs, 0.5, 1.0 - 2.0 ** -53], np.random.default_rng(0).uniform(0, 1, 500)])
    count = sum(ref.fires(ep, r).astype(np.int64) for ep in range(n_epochs))
    assert np.array_equal(count, np.floor((n_epochs - 1) * r).astype(np.int64))
    assert not ref.fires(0, r).any()


def test_mirrored_entries_fire_together():
    idx, d, _ = ref.graph_case()
    rp, col, val, _, _ = ref.graph(idx[:, :14], d[:, :14])
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    key = row.astype(np.int64) * n + col
    mirror = np.searchsorted(key, col.astype(np.int64) * n + row)
    assert np.array_equal(key[mirror], col.astype(np.int64) * n + row)      # the pattern is symmetric
    assert np.array_equal(val[mirror], val)                                   # and so are the values, bit for bit
    for ep in (1, 7, 199):
        f = ref.fires(ep, val / val.max())
        assert np.array_equal(f[mirror], f)


@pytest.mark.parametrize("K", [14, 64, 65, 255])
def test_reference_sigma_does_not_depend_on_the_summation_order(K):
    """The GPU sums a row in another order than numpy; a row's sigma can then differ only when an iterate of the bisection lands within
    rounding of the 1e-5 threshold.  On the graph tests' input at least 99 % of the rows keep their sigma to 1e-12 relative."""
    idx, d, _ = ref.graph_case()
    rho, sigma, _, _ = ref.smooth_knn(d[:, :K])
    rho2, sigma2, _, _ = ref.smooth_knn(d[:, :K], order=np.random.default_rng(K).permutation(K))
    assert np.array_equal(rho, rho2)
    assert (np.abs(sigma - sigma2) <= 1e-12 * sigma).mean() >= 0.99


# ---- 3. refusals that need no device ----------------------------------------------------------------------------------------------------
def test_refusals_before_the_library(sharp):
    X = np.random.default_rng(0).normal(size=(40, 5))
    idx = (np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40
    nd = np.ones((40, 3))
    for nn in (1, 0, 257, 40, 41):
        with pytest.raises(sharp.SharpError, match="n_neighbors"):
            sharp.umap(X, n_neighbors=nn)
    for dims in (0, 4):
        with pytest.raises(sharp.SharpError, match="n_components must be 1, 2 or 3"):
            sharp.umap(X, n_components=dims)
        with pytest.raises(sharp.SharpError, match="n_components must be 1, 2 or 3"):
            sharp.umap_neighbors(idx, nd, n_components=dims)
    for init in (np.zeros((40, 3)), np.zeros((39, 2)), np.zeros(80)):
        with pytest.raises(sharp.SharpError, match="n x n_components matrix"):
            sharp.umap(X, init=init)
        with pytest.raises(sharp.SharpError, match="n x n_components matrix"):
            sharp.umap_neighbors(idx, nd, init=init)
    with pytest.raises(sharp.SharpError, match="init must be one of"):
        sharp.umap(X, init="spectral")
    with pytest.raises(sharp.SharpError, match="needs the data"):
        sharp.umap_neighbors(idx, nd, init="pca")
    with pytest.raises(sharp.SharpError, match="metric 'cosine' is not supported"):
        sharp.umap(X, metric="cosine")
    with pytest.raises(sharp.SharpError, match="metric 'cosine' is not supported"):
        sharp.umap_neighbors(idx, nd, metric="cosine")
    for name in ("local_connectivity", "set_op_mix_ratio", "bandwidth"):
        with pytest.raises(sharp.SharpError, match=f"{name} = 2 is not supported"):
            sharp.umap(X, **{name: 2})
    with pytest.raises(sharp.SharpError, match="both a and b"):
        sharp.umap(X, a=1.0)
    with pytest.raises(sharp.SharpError, match="at least n_components columns"):
        sharp.umap(X[:, :1], n_components=2)
    with pytest.raises(sharp.SharpError, match="at most 255 neighbours"):
        sharp.umap_neighbors(np.zeros((300, 256), np.int32), np.ones((300, 256)))
    with pytest.raises(sharp.SharpError, match="umap: X must be a matrix"):
        sharp.umap(np.zeros(40))
    with pytest.raises(sharp.SharpError, match="method must be"):
        sharp.visualization_SHARP({"x0": X, "viE": X}, method="pca", plot=False)


def _entries(s):
    from sharp_amd.umap import _epochs, _graph

    X = np.random.default_rng(0).normal(size=(40, 5))
    idx = ((np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40).astype(np.int32)
    nd = np.random.default_rng(1).uniform(0.5, 2.0, size=(40, 3))
    rp = np.arange(41, dtype=np.int64)
    col = ((np.arange(40) + 1) % 40).astype(np.int32)
    return {
        "umap": lambda: s.umap(X, n_neighbors=5),
        "umap-random-ret_nn": lambda: s.umap(X, n_neighbors=5, init="random", ret_nn=True, pca=3),
        "umap_neighbors": lambda: s.umap_neighbors(idx, nd),
        "umap_neighbors-init": lambda: s.umap_neighbors(idx, nd, squared=True, init=np.zeros((40, 2)), a=1.5, b=0.9),
        "graph": lambda: _graph(idx, nd),
        "epochs": lambda: _epochs(rp, col, np.ones(40), np.zeros((40, 2)), 10, 0, 10, 1.5, 0.9),
        "visualization_SHARP-umap": lambda: s.visualization_SHARP({"x0": X, "viE": X}, method="umap", plot=False, n_neighbors=5),
    }


@pytest.mark.parametrize("name", ["umap", "umap-random-ret_nn", "umap_neighbors", "umap_neighbors-init", "graph", "epochs",
                                  "visualization_SHARP-umap"])
def test_every_entry_reports_the_missing_device(sharp, monkeypatch, name):
    """as tests/test_abi_cpu.py: with the package told that device 0 is initialised each call converts its arguments and enters the
    library, which has no context: its SharpError, never a ctypes.ArgumentError"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    monkeypatch.setattr(sharp._lib, "_initialised_device", 0)
    with pytest.raises(sharp.SharpError, match="no device context|no HIP device"):
        _entries(sharp)[name]()


def test_dotc_twins_report_the_missing_device(sharp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = sharp.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    X = np.random.default_rng(0).normal(size=(40, 5))
    idx = ((np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40).astype(np.int32)
    Y, st = np.zeros((40, 2)), I(-1)
    tail = [I(2), I(10), D(1.0), D(0.01), D(1.0), np.zeros(2), I(5), D(1.0), I(1), np.zeros(1)]
    L.sharp_C_umap(*[P(v) for v in [X, D(40), I(5), I(5)] + tail + [I(0), I(1), D(10.0), Y, I(0), np.zeros(1, np.int32), np.zeros(1), st]])
    assert st[0] == 3                                                # SHARP_ERR_NO_DEVICE
    st[0] = -1
    L.sharp_C_umap_neighbors(*[P(v) for v in [idx, np.ones((40, 3)), D(40), I(3), I(0)] + tail + [D(10.0), Y, st]])
    assert st[0] == 3
    assert b"no device context" in L.sharp_last_error()


# ---- 4. the quality of the reference run ------------------------------------------------------------------------------------------------
def test_reference_run_separates_the_blobs(sharp):
    """1 500 x 10, six blobs, 500 epochs, the library's a / b at the defaults.  Trustworthiness (sklearn, 15 neighbours) of this run
    over the seeds 10, 1, 2, 3, 4, recorded in DESIGN.md §13: 0.96072, 0.95996, 0.96054, 0.96081, 0.96002."""
    X, lab = ref.blobs()
    Y = ref.run(X, ab=sharp.umap_ab(1.0, 0.01), seed=10)
    assert np.isfinite(Y).all()
    assert ref.knn_purity(Y, lab, 15) == 1.0
