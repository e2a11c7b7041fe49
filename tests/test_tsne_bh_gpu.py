"""The Barnes-Hut repulsion on the MI355X (sharp_tsne_bh, sharp_tsne_gradient_bh, Rtsne(repulsion="barnes_hut")) against the numpy
reference of DESIGN.md §10 (tests/_tsne_bh_ref.py) and the exact GPU path."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _tsne_bh_ref as bh
import _tsne_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import sharp_amd
    from sharp_amd import tsne

    sharp_amd.init(0)
    return tsne


def _blobs(n, d, groups, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3, size=(groups, d))
    lab = rng.integers(0, groups, n)
    return centres[lab] + spread * rng.normal(size=(n, d)), lab


def _mixture(n, dims, seed, groups=8):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 25, size=(groups, dims))
    return centres[rng.integers(0, groups, n)] + 3 * rng.normal(size=(n, dims))


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_gradient_stage_matches_reference(T, dims):
    X, _ = _blobs(2500, 20, 6, 80 + dims)
    rp, col, val = T._affinities(ref.prepare(X, True, 50), 25)
    P = sp.csr_matrix((val, col, rp), shape=(2500, 2500))
    Y = _mixture(2500, dims, 90 + dims) * 0.2
    Y[[11, 1200, 2400]] = Y[3]                       # exact duplicates: one leaf
    Y[500] = Y[501]
    for theta in (0.25, 0.5, 0.8):
        g, Z = T._gradient_bh(rp, col, val, Y, theta)
        gr, Zr = bh.bh_gradient(P, Y, theta, return_z=True)
        np.testing.assert_allclose(Z, Zr, rtol=1e-6)
        np.testing.assert_allclose(g, gr, rtol=0, atol=1e-5 * np.abs(gr).max())


def test_theta_zero_is_the_exact_path(T):
    import sharp_amd

    X, _ = _blobs(900, 12, 4, 30)
    a = sharp_amd.Rtsne(X, perplexity=15, max_iter=120, theta=0.0, repulsion="barnes_hut")
    b = sharp_amd.Rtsne(X, perplexity=15, max_iter=120, theta=0.0)
    assert np.array_equal(a["Y"], b["Y"]) and np.array_equal(a["itercosts"], b["itercosts"]) and np.array_equal(a["costs"], b["costs"])


def test_ten_iterations_from_y_init(T):
    import sharp_amd

    X, _ = _blobs(1200, 20, 4, 15)
    Y0 = np.random.default_rng(16).normal(size=(1200, 2)) * 1e-2
    out = sharp_amd.Rtsne(X, perplexity=20, max_iter=10, Y_init=Y0, stop_lying_iter=5, mom_switch_iter=5, theta=0.5, repulsion="barnes_hut")
    P = ref.joint_p(ref.prepare(X, True, 50), 20)
    Yr, cr = bh.optimise(P, Y0, 0.5, max_iter=10, stop_lying_iter=5, mom_switch_iter=5)
    np.testing.assert_allclose(out["Y"], Yr, rtol=0, atol=1e-6 * np.abs(Yr).max())
    assert out["itercosts"].shape == (1,)
    np.testing.assert_allclose(out["itercosts"], cr, rtol=1e-5)


def _golden_data(g):
    from oracle import pyoracle as orc

    orc.build()
    X = np.log2(orc.synth_fill(g["seed"], g["m"], 0, g["n"], g["G"], g["nmark"]).T + 1.0)
    lab = orc.synth_cluster(g["seed"], range(g["n"]), g["G"])
    return X, lab


def test_full_run_quality_and_bitwise_repeat(T):
    import sharp_amd
    from sklearn.manifold import trustworthiness

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "tsne_full_run.json")))
    X, lab = _golden_data(g)
    kw = dict(perplexity=g["perplexity"], max_iter=g["max_iter"], seed=g["tsne_seed"], theta=0.5, repulsion="barnes_hut")
    a = sharp_amd.Rtsne(X, **kw)
    b = sharp_amd.Rtsne(X, **kw)
    assert np.array_equal(a["Y"], b["Y"]) and np.array_equal(a["itercosts"], b["itercosts"])   # bitwise
    assert a["Y"].shape == (g["n"], 2) and a["itercosts"].shape == (20,)
    assert abs(a["itercosts"][-1] - g["final_kl"]) <= 0.05 * g["final_kl"], (a["itercosts"][-1], g["final_kl"])
    assert trustworthiness(ref.prepare(X, True, 50), a["Y"], n_neighbors=10) >= 0.9
    D = ((a["Y"][:, None, :] - a["Y"][None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, 1)[:, :10]
    assert (lab[nn] == lab[:, None]).mean() >= 0.95


def test_large_n_against_the_exact_gradient(T):
    """one gradient at n = 200 000 with no attraction (an empty P): dY = -rep / Z, Barnes-Hut against the exact GPU path"""
    n = 200000
    Y = _mixture(n, 2, 3)
    rp = np.zeros(n + 1, np.int64)
    col = np.zeros(1, np.int32)
    val = np.zeros(1)
    ge, Ze = T._gradient_bh(rp, col, val, Y, 0.0)        # theta = 0: the exact path
    ez, er = [], []
    for theta in (0.2, 0.5, 0.8):
        g, Z = T._gradient_bh(rp, col, val, Y, theta)
        ez.append(abs(Z - Ze) / Ze)
        er.append(np.linalg.norm(g - ge) / np.linalg.norm(ge))
    assert ez[0] < ez[1] < ez[2] and er[0] < er[1] < er[2], (ez, er)
    assert er[1] <= 0.1 and ez[1] <= 0.05, (ez, er)


def test_argument_errors(T):
    import sharp_amd

    X, _ = _blobs(300, 6, 3, 31)
    for bad in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(sharp_amd.SharpError, match="Incorrect theta"):
            sharp_amd.Rtsne(X, perplexity=10, max_iter=5, theta=bad, repulsion="barnes_hut")
    with pytest.raises(sharp_amd.SharpError, match="repulsion"):
        sharp_amd.Rtsne(X, perplexity=10, max_iter=5, repulsion="Barnes-Hut")
    rp, col, val = T._affinities(ref.prepare(X, True, 50), 10)
    with pytest.raises(sharp_amd.SharpError, match="Incorrect theta"):
        T._gradient_bh(rp, col, val, np.zeros((300, 2)), -1.0)
    assert sharp_amd.Rtsne(X, perplexity=10, max_iter=5, theta=1.0, repulsion="barnes_hut")["Y"].shape == (300, 2)   # still usable
    assert sharp_amd.Rtsne(X, perplexity=10, max_iter=5, theta=5.0)["Y"].shape == (300, 2)                           # exact: any theta


def test_dotc_tsne_bh_all_pointer_call(T):
    import sharp_amd

    L = sharp_amd.lib()
    X, _ = _blobs(600, 10, 3, 22)
    Y0 = np.random.default_rng(23).normal(size=(600, 2)) * 1e-2
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    Y, ic, costs, st = np.zeros((600, 2)), np.zeros(2), np.zeros(600), I(-1)
    args = [np.ascontiguousarray(X), D(600), I(10), I(2), I(50), I(1), I(1), I(0), I(1), I(0), D(15.0), D(0.5), I(60), I(0), I(0), D(0.5),
            D(0.8), D(200.0), D(12.0), I(1), Y0, D(10.0), Y, ic, costs, st]
    L.sharp_C_tsne_bh.restype = None
    L.sharp_C_tsne_bh(*[P(a) for a in args])
    assert st[0] == 0
    want = sharp_amd.Rtsne(X, perplexity=15, max_iter=60, Y_init=Y0, theta=0.5, repulsion="barnes_hut")
    assert np.array_equal(Y, want["Y"]) and np.array_equal(ic, want["itercosts"]) and np.array_equal(costs, want["costs"])
    st[0] = -1
    args[11] = D(2.0)                                                # a rejected theta: status + message
    L.sharp_C_tsne_bh(*[P(a) for a in args])
    assert st[0] != 0 and "theta" in L.sharp_last_error().decode().lower()


def test_visualization_sharp_barnes_hut(T, oracle):
    import sharp_amd

    X = oracle.synth_fill(20261003, 1500, 0, 1200, 4, 200)
    res = sharp_amd.SHARP(X, rN_seed=2103, ensize_K=3)
    v = sharp_amd.visualization_SHARP(res, repulsion="barnes_hut", plot=False, max_iter=300)
    assert v["Y"].shape == (1200, 2) and np.isfinite(v["Y"]).all() and v["filename"] is None
