"""t-SNE on the MI355X (sharp_tsne and its stages) against the numpy reference of DESIGN.md §10 (tests/_tsne_ref.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

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


def test_knn_exact_with_duplicates_and_near_duplicates(T):
    X, _ = _blobs(3000, 20, 6, 11)
    X[100] = X[7]                                   # exact duplicates
    X[2500] = X[7]
    X[200] = X[9] + 1e-7                            # near duplicates
    X[201] = X[9] - 3e-7
    K = 90
    idx, dist = T._knn(X, K)
    ridx, rdist = ref.knn(X, K)
    assert np.array_equal(idx, ridx)
    np.testing.assert_allclose(dist, rdist, rtol=1e-12, atol=1e-300)
    assert idx[7, 0] == 100 and idx[7, 1] == 2500 and dist[7, 0] == 0.0


def test_knn_several_launches_rows_checked_against_brute_force(T):
    """n large enough for the k-NN to go out as several row launches; 120 rows checked against numpy"""
    X, _ = _blobs(200000, 8, 12, 24, spread=0.5)
    K = 45
    idx, dist = T._knn(X, K)
    rows = np.random.default_rng(25).choice(X.shape[0], 120, replace=False)
    D = ref.sqdist_rows(X, rows)
    D[np.arange(rows.size), rows] = np.inf
    o = np.argsort(D, axis=1, kind="stable")[:, :K]
    assert np.array_equal(idx[rows], o)
    np.testing.assert_allclose(dist[rows], np.take_along_axis(D, o, 1), rtol=1e-12, atol=1e-300)


def test_non_finite_input_raises(T):
    import sharp_amd

    X, _ = _blobs(500, 6, 3, 26)
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[17, 3] = bad
        for pca in (True, False):
            with pytest.raises(sharp_amd.SharpError, match="NA / NaN / Inf"):
                sharp_amd.Rtsne(Xb, perplexity=10, max_iter=5, pca=pca)
        with pytest.raises(sharp_amd.SharpError, match="NA / NaN / Inf"):
            T._knn(Xb, 20)
    with pytest.raises(sharp_amd.SharpError, match="overflow"):          # finite, but squared distances would overflow
        T._knn(X * 1e160, 20)
    with pytest.raises(sharp_amd.SharpError, match="overflow"):
        sharp_amd.Rtsne(X * 1e160, perplexity=10, max_iter=5, pca=False, normalize=False)
    Y0 = np.zeros((500, 2))
    Y0[3, 1] = np.nan
    with pytest.raises(sharp_amd.SharpError, match="Y_init"):
        sharp_amd.Rtsne(X, perplexity=10, max_iter=5, Y_init=Y0)
    assert sharp_amd.Rtsne(X, perplexity=10, max_iter=5, pca=False)["Y"].shape == (500, 2)   # the library is still usable


def test_pca_subspace_matches_eigh(T):
    rng = np.random.default_rng(12)
    X = rng.normal(size=(5000, 120)) @ rng.normal(size=(120, 120)) * 0.1 + rng.normal(size=120)
    out = T._prepare(X, pca=True, initial_dims=30, normalize=False)
    want, _ = ref.pca(X, 30)
    assert out.shape == (5000, 30)
    # principal angles between the spans, and the signed components themselves (same sign convention)
    qa, _ = np.linalg.qr(out)
    qb, _ = np.linalg.qr(want)
    s = np.linalg.svd(qa.T @ qb, compute_uv=False)
    assert s.min() > 1 - 1e-10
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-8 * np.abs(want).max())
    norm = T._prepare(X, pca=True, initial_dims=30)
    np.testing.assert_allclose(norm, ref.normalize(want), rtol=0, atol=1e-8)


def test_affinities_and_gradient_match_reference(T):
    X, _ = _blobs(1500, 30, 5, 13)
    Xp = ref.prepare(X, True, 50)
    rp, col, val = T._affinities(Xp, 30)
    P = ref.joint_p(Xp, 30)
    assert np.array_equal(rp, P.indptr) and np.array_equal(col, P.indices)
    np.testing.assert_allclose(val, P.data, rtol=1e-10, atol=0)
    Y = np.random.default_rng(14).normal(size=(1500, 2)) * 3
    g = T._gradient(rp, col, val, Y)
    gr = ref.gradient(P, Y)
    assert np.linalg.norm(g - gr) <= 1e-5 * np.linalg.norm(gr)
    np.testing.assert_allclose(g, gr, rtol=0, atol=1e-5 * np.abs(gr).max())


def test_ten_iterations_from_y_init(T):
    import sharp_amd

    X, _ = _blobs(1200, 20, 4, 15)
    Y0 = np.random.default_rng(16).normal(size=(1200, 2)) * 1e-2
    out = sharp_amd.Rtsne(X, perplexity=20, max_iter=10, Y_init=Y0, stop_lying_iter=5, mom_switch_iter=5)
    P = ref.joint_p(ref.prepare(X, True, 50), 20)
    Yr, cr = ref.optimise(P, Y0, max_iter=10, stop_lying_iter=5, mom_switch_iter=5)
    ext = np.abs(Yr).max()
    np.testing.assert_allclose(out["Y"], Yr, rtol=0, atol=1e-6 * ext)
    assert out["itercosts"].shape == (1,)
    np.testing.assert_allclose(out["itercosts"], cr, rtol=1e-5)
    np.testing.assert_allclose(out["costs"].sum(), cr[-1], rtol=1e-5)


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
    a = sharp_amd.Rtsne(X, perplexity=g["perplexity"], max_iter=g["max_iter"], seed=g["tsne_seed"])
    b = sharp_amd.Rtsne(X, perplexity=g["perplexity"], max_iter=g["max_iter"], seed=g["tsne_seed"])
    assert np.array_equal(a["Y"], b["Y"]) and np.array_equal(a["itercosts"], b["itercosts"])   # bitwise
    assert a["Y"].shape == (g["n"], 2) and a["itercosts"].shape == (20,) and a["origD"] == 50 and a["N"] == g["n"]
    assert abs(a["itercosts"][-1] - g["final_kl"]) <= 0.01 * g["final_kl"], (a["itercosts"][-1], g["final_kl"])
    assert trustworthiness(ref.prepare(X, True, 50), a["Y"], n_neighbors=10) >= 0.9
    # 10-NN label agreement in 2-D
    D = ((a["Y"][:, None, :] - a["Y"][None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, 1)[:, :10]
    assert (lab[nn] == lab[:, None]).mean() >= 0.95


def test_start_from_seed_matches_reference_stream(T):
    import sharp_amd
    from oracle import pyoracle as orc

    X, _ = _blobs(400, 8, 3, 17)
    out = sharp_amd.Rtsne(X, perplexity=10, max_iter=1, stop_lying_iter=0, mom_switch_iter=0, seed=10)
    orc.build()
    Y0 = ref.init_y(400, 2, 10, orc.runif)
    P = ref.joint_p(ref.prepare(X, True, 50), 10)
    Yr, _ = ref.optimise(P, Y0, max_iter=1, stop_lying_iter=0, mom_switch_iter=0)
    np.testing.assert_allclose(out["Y"], Yr, rtol=0, atol=1e-6 * np.abs(Yr).max())


def test_dims_three_and_one(T):
    import sharp_amd

    X, _ = _blobs(800, 12, 4, 18)
    Y0 = np.random.default_rng(19).normal(size=(800, 3)) * 1e-2
    out = sharp_amd.Rtsne(X, dims=3, perplexity=15, max_iter=10, Y_init=Y0)
    P = ref.joint_p(ref.prepare(X, True, 50), 15)
    Yr, _ = ref.optimise(P, Y0, max_iter=10, stop_lying_iter=0, mom_switch_iter=0)
    np.testing.assert_allclose(out["Y"], Yr, rtol=0, atol=1e-6 * np.abs(Yr).max())
    one = sharp_amd.Rtsne(X, dims=1, perplexity=15, max_iter=50)
    assert one["Y"].shape == (800, 1) and np.isfinite(one["Y"]).all()


def test_argument_errors(T):
    import sharp_amd

    X, _ = _blobs(100, 5, 2, 20)
    with pytest.raises(sharp_amd.SharpError, match="Perplexity is too large"):
        sharp_amd.Rtsne(X, perplexity=34, max_iter=5)
    Xb, _ = _blobs(1000, 5, 2, 21)
    with pytest.raises(sharp_amd.SharpError, match="above 85"):
        sharp_amd.Rtsne(Xb, perplexity=86, max_iter=5)
    Xd = Xb.copy()
    Xd[5] = Xd[9]
    with pytest.raises(sharp_amd.SharpError, match="duplicates"):
        sharp_amd.Rtsne(Xd, perplexity=10, max_iter=5)
    assert sharp_amd.Rtsne(Xd, perplexity=10, max_iter=5, check_duplicates=False)["Y"].shape == (1000, 2)


def test_visualization_sharp_on_sharp_and_unlimited(T, tmp_path, oracle):
    import sharp_amd

    X = oracle.synth_fill(20261003, 1500, 0, 1200, 4, 200)
    res = sharp_amd.SHARP(X, rN_seed=2103, ensize_K=3)
    f = str(tmp_path / "vi.png")
    v = sharp_amd.visualization_SHARP(res, label=res["pred_clusters"], filename=f, filetype="png", res=60, max_iter=300)
    assert v["Y"].shape == (1200, 2) and os.path.getsize(f) > 1000 and v["filename"] == f
    blocks = [np.asfortranarray(X[:, :600]), np.asfortranarray(X[:, 600:])]
    ru = sharp_amd.SHARP_unlimited(blocks, rN_seed=2103, ensize_K=3)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        vu = sharp_amd.visualization_SHARP(ru, max_iter=300)
    finally:
        os.chdir(cwd)
    assert vu["Y"].shape == (1200, 2) and vu["filename"] == "vi_SHARP.pdf"
    assert os.path.getsize(tmp_path / "vi_SHARP.pdf") > 1000


def test_dotc_tsne_all_pointer_call(T):
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
    L.sharp_C_tsne.restype = None
    L.sharp_C_tsne(*[P(a) for a in args])
    assert st[0] == 0
    want = sharp_amd.Rtsne(X, perplexity=15, max_iter=60, Y_init=Y0)
    assert np.array_equal(Y, want["Y"]) and np.array_equal(ic, want["itercosts"])
    st[0] = -1
    args[10] = D(300.0)                                              # a rejected perplexity: status + message
    L.sharp_C_tsne(*[P(a) for a in args])
    assert st[0] != 0 and "perplexity" in L.sharp_last_error().decode().lower()
